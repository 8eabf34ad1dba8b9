/*
 * pbr_ddsin.c -- every way from a .dds file to a texture (C11), on top of the parsers of host/pbr_dds.c:
 * the material textures that asset_import.cpp:30-60 (LoadMeshTexture) loads, whose BC1 / BC3 / BC5 payloads go to the backend as they
 * are (it decodes them with K15); the float maps of a saved bake (host/pbr_ddsout.c); and BC6H_UF16 files.  Nothing here
 * samples BC6H blocks: every level is decoded once, by K19 (GPUX_OpDecodeBC6H; csrc/bc6h_decode_core.h is the contract), into an
 * RGBA32F or RGBA16F texture.  So the compact cube the bake writes (pbr_demo ... dds PREFIX, 16 times smaller than RGBA32F) and the
 * BC6H cubes of texconv, Compressonator or an engine cooker -- which use the two-region and delta modes K18 never emits -- can be
 * shaded from.
 *
 * The file is face-major (each face with its levels), a texture and both ops take a level layer after layer: upload_levels reorders
 * into one staging buffer and records one op per level into one graph.  Each loader is its own rule for format and level count, then
 * that function.
 */
#include "pbr_host.h"
#include "pbr_file.h"
#include "../csrc/bc6h_decode_core.h"

#include <string.h>

/* levels [0, n) of the file `p`, laid out as a parser reported (level_offset[layer][level], level_size[level]), into t: by
 * GPUX_OpDecodeBC6H if bc6h, else by GPUX_OpCopyBufferToTextureMip; blocking.  Returns t, or NULL (message on stderr) with t destroyed. */
static GPU_Texture* upload_levels(const char* fn, const uint8_t* p, uint64_t (*level_offset)[PBR_DDS_MAX_LEVELS], const uint64_t* level_size,
                                  uint32_t layers, uint32_t n, GPU_Texture* t, int bc6h) {
    uint64_t stage_off[PBR_DDS_MAX_LEVELS], stage_total = 0;
    for (uint32_t m = 0; m < n; ++m) { stage_off[m] = stage_total; stage_total += level_size[m] * layers; }
    GPU_Buffer* staging = stage_total <= 0xFFFFFFFFu ? GPU_MakeBuffer((uint32_t)stage_total, GPU_BufferFlag_CPU, NULL) : NULL;
    GPU_Graph* g = staging ? GPU_MakeGraph() : NULL;
    if (!g) {
        fprintf(stderr, "GPU-ERROR: %s: no staging buffer of %llu bytes, or no graph\n", fn, (unsigned long long)stage_total);
        GPU_DestroyBuffer(staging); GPU_DestroyTexture(t); return NULL;
    }
    for (uint32_t m = 0; m < n; ++m) {
        for (uint32_t l = 0; l < layers; ++l)
            memcpy((uint8_t*)staging->data + stage_off[m] + (uint64_t)l * level_size[m], p + level_offset[l][m], (size_t)level_size[m]);
        if (bc6h) GPUX_OpDecodeBC6H(g, staging, (uint32_t)stage_off[m], t, m);
        else GPUX_OpCopyBufferToTextureMip(g, staging, (uint32_t)stage_off[m], t, m);
    }
    GPU_GraphSubmit(g);
    GPU_GraphWait(g);
    GPU_DestroyGraph(g);
    GPU_DestroyBuffer(staging);
    return t;
}

static uint32_t texture_flags(const PBR_DDSInfoEx* info) {
    return (info->layers == 6 ? GPU_TextureFlag_Cubemap : 0) | (info->level_count > 1 ? GPU_TextureFlag_HasMipmaps : 0);
}

GPU_Texture* PBR_MakeTextureFromDDSMemory(const void* bytes, size_t size, uint32_t flags) {
    const char* fn = "PBR_MakeTextureFromDDS";
    PBR_DDSInfo info;
    const int rc = PBR_ParseDDS(bytes, size, &info);
    if (rc != 0) { fprintf(stderr, "GPU-ERROR: %s: %s\n", fn, PBR_DDSErrorString(rc)); return NULL; }
    const uint8_t* p = (const uint8_t*)bytes;
    if (!(flags & PBR_DDS_FILE_MIPS) || info.level_count == 1)                /* asset_import.cpp:53 */
        return GPU_MakeTexture(info.format, info.width, info.height, 1, 0, p + info.level_offset[0]);
    GPU_Texture* t = GPU_MakeTexture(info.format, info.width, info.height, 1, GPU_TextureFlag_HasMipmaps, NULL);
    if (!t) return NULL;
    const uint32_t n = t->mip_level_count;                                    /* counted from the smaller extent */
    if (info.level_count < n) {
        fprintf(stderr, "GPU-ERROR: %s: the file holds %u levels, the chain needs %u\n", fn, info.level_count, n);
        GPU_DestroyTexture(t); return NULL;
    }
    return upload_levels(fn, p, &info.level_offset, info.level_size, 1, n, t, 0);
}

GPU_Texture* PBR_MakeTextureFromFloatDDSMemory(const void* bytes, size_t size) {
    const char* fn = "PBR_MakeTextureFromFloatDDS";
    PBR_DDSInfoEx info;
    const int rc = PBR_ParseDDSEx(bytes, size, &info);
    if (rc != 0) { fprintf(stderr, "GPU-ERROR: %s: %s\n", fn, PBR_DDSErrorString(rc)); return NULL; }
    const GPU_Format format = info.dxgi_format == 2 ? GPU_Format_RGBA32F : info.dxgi_format == 10 ? GPU_Format_RGBA16F
                            : info.dxgi_format == 34 ? GPU_Format_RG16F : GPU_Format_Invalid;
    if (format == GPU_Format_Invalid) { fprintf(stderr, "GPU-ERROR: %s: DXGI format %u is not RGBA32F, RGBA16F or RG16F\n", fn, info.dxgi_format); return NULL; }
    GPU_Texture* t = GPU_MakeTexture(format, info.width, info.height, 1, texture_flags(&info), NULL);
    if (!t) return NULL;
    if (t->mip_level_count != info.level_count) {
        fprintf(stderr, "GPU-ERROR: %s: the file holds %u levels, the chain has %u\n", fn, info.level_count, t->mip_level_count);
        GPU_DestroyTexture(t); return NULL;
    }
    return upload_levels(fn, (const uint8_t*)bytes, info.level_offset, info.level_size, info.layers, info.level_count, t, 0);
}

GPU_Texture* PBR_MakeTextureFromBC6HDDSMemory(const void* bytes, size_t size, GPU_Format target) {
    const char* fn = "PBR_MakeTextureFromBC6HDDS";
    if (target != GPU_Format_RGBA32F && target != GPU_Format_RGBA16F) { fprintf(stderr, "GPU-ERROR: %s: the target format must be RGBA32F or RGBA16F\n", fn); return NULL; }
    PBR_DDSInfoEx info;
    const int rc = PBR_ParseDDSEx(bytes, size, &info);
    if (rc != 0) { fprintf(stderr, "GPU-ERROR: %s: %s\n", fn, PBR_DDSErrorString(rc)); return NULL; }
    if (info.dxgi_format != 95) { fprintf(stderr, "GPU-ERROR: %s: DXGI format %u is not BC6H_UF16 (95)\n", fn, info.dxgi_format); return NULL; }
    GPU_Texture* t = GPU_MakeTexture(target, info.width, info.height, 1, texture_flags(&info), NULL);
    if (!t) return NULL;
    if (t->mip_level_count < info.level_count || t->layer_count != info.layers) {         /* the parser bounds the levels by the full chain */
        fprintf(stderr, "GPU-ERROR: %s: the file holds %u levels of %u layers, the texture has %u of %u\n", fn, info.level_count, info.layers,
                t->mip_level_count, t->layer_count);
        GPU_DestroyTexture(t); return NULL;
    }
    for (uint32_t m = 0; m < info.level_count; ++m)
        if (GPUX_BC6HMipBytes(t, m) != info.level_size[m] * info.layers) {
            fprintf(stderr, "GPU-ERROR: %s: a level's size in the file is not the texture's\n", fn);
            GPU_DestroyTexture(t); return NULL;
        }
    return upload_levels(fn, (const uint8_t*)bytes, info.level_offset, info.level_size, info.layers, info.level_count, t, 1);   /* the texture's other levels stay zero */
}

GPU_Texture* PBR_MakeTextureFromDDSFile(const char* filepath, uint32_t flags) {
    size_t n;
    void* buf = pbr_read_file("PBR_MakeTextureFromDDSFile", filepath, &n);
    GPU_Texture* t = buf ? PBR_MakeTextureFromDDSMemory(buf, n, flags) : NULL;
    free(buf);
    return t;
}

GPU_Texture* PBR_MakeTextureFromFloatDDSFile(const char* filepath) {
    size_t n;
    void* buf = pbr_read_file("PBR_MakeTextureFromFloatDDSFile", filepath, &n);
    GPU_Texture* t = buf ? PBR_MakeTextureFromFloatDDSMemory(buf, n) : NULL;
    free(buf);
    return t;
}

GPU_Texture* PBR_MakeTextureFromBC6HDDSFile(const char* filepath, GPU_Format target) {
    size_t n;
    void* buf = pbr_read_file("PBR_MakeTextureFromBC6HDDSFile", filepath, &n);
    GPU_Texture* t = buf ? PBR_MakeTextureFromBC6HDDSMemory(buf, n, target) : NULL;
    free(buf);
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
