/*
 * pbr_ddsout.c -- the bake's maps as .dds files an engine loads (C11): one DX10-header container per texture with the
 * whole mip chain, the way cmft, IBLBaker and cmgen write theirs, on top of PBR_BuildDDSHeader (host/pbr_dds.c: the header bytes and
 * where every layer's levels go).  Float textures go out as they are (RGBA32F = DXGI 2, RGBA16F = 10, RG16F = 34) or narrowed to
 * RGBA16F on the host (the fp32 -> fp16 conversion of csrc/bc6h_format.h); BC6H_UF16 (DXGI 95) is encoded on the device by K18, at its
 * one-region or its two-region quality (csrc/bc6h_core.h, csrc/bc6h2_core.h are the contracts): the same container either way.  The
 * files load back through host/pbr_ddsin.c, so a bake can be saved and shaded later without the source environment.
 *
 * The file is face-major (each face with its levels), texture memory level-major: the writer reorders.
 */
#include "pbr_host.h"
#include "../csrc/bc6h_format.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint32_t same_dxgi(GPU_Format f) { return f == GPU_Format_RGBA32F ? 2u : f == GPU_Format_RGBA16F ? 10u : f == GPU_Format_RG16F ? 34u : 0u; }
static uint32_t level_dim(uint32_t d, uint32_t m) { const uint32_t v = d >> m; return v ? v : 1; }

void* PBR_EncodeTextureDDS(GPU_Texture* texture, uint32_t first_mip, uint32_t mip_count, int out_format, size_t* out_size) {
    const char* fn = "PBR_EncodeTextureDDS";
    if (out_size) *out_size = 0;
    if (!texture || !out_size || texture->depth != 1 || first_mip >= texture->mip_level_count) { fprintf(stderr, "GPU-ERROR: %s: bad arguments\n", fn); return NULL; }
    if (mip_count == 0) mip_count = texture->mip_level_count - first_mip;
    if (mip_count > texture->mip_level_count - first_mip || mip_count > PBR_DDS_MAX_LEVELS) { fprintf(stderr, "GPU-ERROR: %s: bad level range\n", fn); return NULL; }
    const uint32_t src_dxgi = same_dxgi(texture->format);
    uint32_t dxgi = 0;
    if (out_format == PBR_DDS_OUT_SAME) dxgi = src_dxgi;
    else if (out_format == PBR_DDS_OUT_RGBA16F && (src_dxgi == 2 || src_dxgi == 10)) dxgi = 10;
    else if ((out_format == PBR_DDS_OUT_BC6H_UF16 || out_format == PBR_DDS_OUT_BC6H_UF16_2R) && (src_dxgi == 2 || src_dxgi == 10)) dxgi = 95;
    if (!dxgi) { fprintf(stderr, "GPU-ERROR: %s: texture format %d cannot be written as output format %d\n", fn, (int)texture->format, out_format); return NULL; }
    const uint32_t layers = texture->layer_count, w0 = level_dim(texture->width, first_mip), h0 = level_dim(texture->height, first_mip);
    uint8_t header[148];
    PBR_DDSInfoEx lay;
    const uint64_t total = PBR_BuildDDSHeader(dxgi, w0, h0, layers, mip_count, header, &lay);
    if (!total) { fprintf(stderr, "GPU-ERROR: %s: a %u x %u texture of %u layers and %u levels has no DDS form\n", fn, w0, h0, layers, mip_count); return NULL; }

    /* every level, all layers, into one mapped buffer in texture order (level-major), by one graph */
    const int bc6h = dxgi == 95;
    const uint32_t quality = out_format == PBR_DDS_OUT_BC6H_UF16_2R ? GPUX_BC6H_TwoRegions : GPUX_BC6H_OneRegion;
    uint64_t stage_off[PBR_DDS_MAX_LEVELS], stage_total = 0;
    for (uint32_t m = 0; m < mip_count; ++m) {
        stage_off[m] = stage_total;
        stage_total += bc6h ? GPUX_BC6HMipBytes(texture, first_mip + m) : GPUX_TextureMipBytes(texture, first_mip + m);
    }
    if (stage_total > 0xFFFFFFFFu) { fprintf(stderr, "GPU-ERROR: %s: %llu bytes exceed a buffer (write fewer levels per file)\n", fn, (unsigned long long)stage_total); return NULL; }
    uint8_t* file = (uint8_t*)malloc((size_t)total);
    GPU_Buffer* staging = file ? GPU_MakeBuffer((uint32_t)stage_total, GPU_BufferFlag_CPU, NULL) : NULL;
    GPU_Graph* g = staging ? GPU_MakeGraph() : NULL;
    if (!g) { GPU_DestroyBuffer(staging); free(file); fprintf(stderr, "GPU-ERROR: %s: allocation failed\n", fn); return NULL; }
    for (uint32_t m = 0; m < mip_count; ++m) {
        if (bc6h) GPUX_OpEncodeBC6HEx(g, texture, first_mip + m, staging, (uint32_t)stage_off[m], quality);
        else GPUX_OpCopyTextureMipToBuffer(g, texture, first_mip + m, staging, (uint32_t)stage_off[m]);
    }
    GPU_GraphSubmit(g);
    GPU_GraphWait(g);
    memcpy(file, header, sizeof header);
    const uint8_t* staged = (const uint8_t*)staging->data;
    const int narrow = dxgi == 10 && src_dxgi == 2;                           /* RGBA32F -> RGBA16F on the host, sign and Inf kept */
    for (uint32_t l = 0; l < layers; ++l)
        for (uint32_t m = 0; m < mip_count; ++m) {
            uint8_t* dst = file + lay.level_offset[l][m];
            if (!narrow) { memcpy(dst, staged + stage_off[m] + (uint64_t)l * lay.level_size[m], (size_t)lay.level_size[m]); continue; }
            const uint64_t n = lay.level_size[m] / 2;                         /* components */
            const uint8_t* src = staged + stage_off[m] + (uint64_t)l * n * 4;
            for (uint64_t i = 0; i < n; ++i) {
                uint32_t fbits;
                memcpy(&fbits, src + 4 * i, 4);
                const uint32_t hbits = bc6h_f16_from_f32(fbits);
                dst[2 * i] = (uint8_t)hbits; dst[2 * i + 1] = (uint8_t)(hbits >> 8);
            }
        }
    GPU_DestroyGraph(g);
    GPU_DestroyBuffer(staging);
    *out_size = (size_t)total;
    return file;
}

int PBR_WriteTextureDDS(const char* path, GPU_Texture* texture, uint32_t first_mip, uint32_t mip_count, int out_format) {
    size_t size = 0;
    void* bytes = path ? PBR_EncodeTextureDDS(texture, first_mip, mip_count, out_format, &size) : NULL;
    if (!bytes) return 1;
    FILE* f = fopen(path, "wb");
    int ok = f && fwrite(bytes, 1, size, f) == size;
    if (f && fclose(f) != 0) ok = 0;
    free(bytes);
    if (!ok) fprintf(stderr, "GPU-ERROR: PBR_WriteTextureDDS: cannot write %s\n", path);
    return ok ? 0 : 1;
}
