/*
 * pbr_ddsin.c -- BC6H_UF16 .dds files as textures the lighting pass takes (C11): the input half of pbr_ddsout.c.
 * Nothing here samples BC6H blocks: like K15 for the BC1 / BC3 / BC5 material textures, every level is decoded once, by K19
 * (GPUX_OpDecodeBC6H; csrc/bc6h_decode_core.h is the contract), into an RGBA32F or RGBA16F texture.  So the compact cube the bake
 * writes (pbr_demo ... dds PREFIX, 16 times smaller than RGBA32F) and the BC6H cubes of texconv, Compressonator or an engine cooker --
 * which use the two-region and delta modes K18 never emits -- can be shaded from.
 *
 * The file is face-major (each face with its levels, pbr_ddsout.c), the op reads a level's blocks layer after layer: the loader
 * reorders into one staging buffer and records one op per level into one graph.
 */
#include "pbr_host.h"
#include "../csrc/bc6h_decode_core.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

GPU_Texture* PBR_MakeTextureFromBC6HDDSMemory(const void* bytes, size_t size, GPU_Format target) {
    const char* fn = "PBR_MakeTextureFromBC6HDDS";
    if (target != GPU_Format_RGBA32F && target != GPU_Format_RGBA16F) { fprintf(stderr, "GPU-ERROR: %s: the target format must be RGBA32F or RGBA16F\n", fn); return NULL; }
    PBR_DDSInfoEx info;
    const int rc = PBR_ParseDDSEx(bytes, size, &info);
    if (rc != 0) { fprintf(stderr, "GPU-ERROR: %s: %s\n", fn, PBR_DDSErrorString(rc)); return NULL; }
    if (info.dxgi_format != 95) { fprintf(stderr, "GPU-ERROR: %s: DXGI format %u is not BC6H_UF16 (95)\n", fn, info.dxgi_format); return NULL; }
    uint64_t stage_off[PBR_DDS_MAX_LEVELS], stage_total = 0;
    for (uint32_t m = 0; m < info.level_count; ++m) { stage_off[m] = stage_total; stage_total += info.level_size[m] * info.layers; }
    if (stage_total > 0xFFFFFFFFu) { fprintf(stderr, "GPU-ERROR: %s: %llu bytes of blocks exceed a buffer\n", fn, (unsigned long long)stage_total); return NULL; }
    const uint32_t flags = (info.layers == 6 ? GPU_TextureFlag_Cubemap : 0) | (info.level_count > 1 ? GPU_TextureFlag_HasMipmaps : 0);
    GPU_Texture* t = GPU_MakeTexture(target, info.width, info.height, 1, flags, NULL);
    if (!t) return NULL;
    if (t->mip_level_count < info.level_count || t->layer_count != info.layers) {         /* the parser bounds the levels by the full chain */
        fprintf(stderr, "GPU-ERROR: %s: the file holds %u levels of %u layers, the texture has %u of %u\n", fn, info.level_count, info.layers,
                t->mip_level_count, t->layer_count);
        GPU_DestroyTexture(t); return NULL;
    }
    GPU_Buffer* staging = GPU_MakeBuffer((uint32_t)stage_total, GPU_BufferFlag_CPU, NULL);
    GPU_Graph* g = staging ? GPU_MakeGraph() : NULL;
    if (!g) { GPU_DestroyBuffer(staging); GPU_DestroyTexture(t); fprintf(stderr, "GPU-ERROR: %s: allocation failed\n", fn); return NULL; }
    const uint8_t* p = (const uint8_t*)bytes;
    int ok = 1;
    for (uint32_t m = 0; m < info.level_count; ++m) {                         /* face-major file -> a level's blocks layer after layer */
        if (GPUX_BC6HMipBytes(t, m) != info.level_size[m] * info.layers) { ok = 0; break; }
        for (uint32_t l = 0; l < info.layers; ++l)
            memcpy((uint8_t*)staging->data + stage_off[m] + (uint64_t)l * info.level_size[m], p + info.level_offset[l][m], (size_t)info.level_size[m]);
        GPUX_OpDecodeBC6H(g, staging, (uint32_t)stage_off[m], t, m);
    }
    if (ok) { GPU_GraphSubmit(g); GPU_GraphWait(g); }
    GPU_DestroyGraph(g);
    GPU_DestroyBuffer(staging);
    if (!ok) { fprintf(stderr, "GPU-ERROR: %s: a level's size in the file is not the texture's\n", fn); GPU_DestroyTexture(t); return NULL; }
    return t;
}

GPU_Texture* PBR_MakeTextureFromBC6HDDSFile(const char* filepath, GPU_Format target) {
    FILE* f = filepath ? fopen(filepath, "rb") : NULL;
    if (!f) { fprintf(stderr, "GPU-ERROR: PBR_MakeTextureFromBC6HDDSFile: cannot open %s\n", filepath ? filepath : "(null)"); return NULL; }
    GPU_Texture* t = NULL;
    void* buf = NULL;
    long n = -1;
    if (fseek(f, 0, SEEK_END) == 0) n = ftell(f);
    if (n > 0 && fseek(f, 0, SEEK_SET) == 0 && (buf = malloc((size_t)n)) != NULL && fread(buf, 1, (size_t)n, f) == (size_t)n)
        t = PBR_MakeTextureFromBC6HDDSMemory(buf, (size_t)n, target);
    else fprintf(stderr, "GPU-ERROR: PBR_MakeTextureFromBC6HDDSFile: cannot read %s\n", filepath);
    free(buf);
    fclose(f);
    return t;
}

void PBR_DecodeBC6HBlocks(const void* blocks, uint32_t w, uint32_t h, uint16_t* rgb_half) {
    if (!blocks || !rgb_half || w == 0 || h == 0) return;
    const uint32_t bw = (w + 3) / 4, bh = (h + 3) / 4;
    for (uint32_t by = 0; by < bh; ++by)
        for (uint32_t bx = 0; bx < bw; ++bx) {
            uint32_t words[4], rgb[16][3];
            memcpy(words, (const uint8_t*)blocks + ((size_t)by * bw + bx) * 16, 16);
            bc6hd_decode_block(words, rgb);
            for (uint32_t t = 0; t < 16; ++t) {
                const uint32_t x = 4 * bx + (t & 3), y = 4 * by + (t >> 2);
                if (x >= w || y >= h) continue;                               /* texels of a block outside the level are dropped */
                uint16_t* o = rgb_half + ((size_t)y * w + x) * 3;
                for (int c = 0; c < 3; ++c) o[c] = (uint16_t)rgb[t][c];
            }
        }
}
