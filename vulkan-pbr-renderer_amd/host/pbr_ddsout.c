/*
 * pbr_ddsout.c -- the bake's maps as .dds files an engine loads (C11): one DX10-header container per texture with the
 * whole mip chain, the way cmft, IBLBaker and cmgen write theirs.  Float textures go out as they are (RGBA32F = DXGI 2, RGBA16F = 10,
 * RG16F = 34) or narrowed to RGBA16F on the host; BC6H_UF16 (DXGI 95) is encoded on the device by K18 (csrc/bc6h_core.h is the
 * contract, also of the host's fp32 -> fp16 conversion).  The float files load back (PBR_MakeTextureFromFloatDDS*), so a bake can be
 * saved and shaded later without the source environment; BC6H files load through host/pbr_ddsin.c (K19).
 *
 * File layout (Microsoft's DDS programming guide): "DDS " magic, the 124-byte DDS_HEADER, the 20-byte DDS_HEADER_DXT10, then for a
 * cube the six faces in the order +X -X +Y -Y +Z -Z (the texture's layer order, face_texel_dir), each face with its levels largest
 * first, tight.  Texture memory is level-major, so writer and loader reorder.
 */
#include "pbr_host.h"
#include "../csrc/bc6h_core.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
#define FOURCC(a, b, c, d) ((uint32_t)(a) | ((uint32_t)(b) << 8) | ((uint32_t)(c) << 16) | ((uint32_t)(d) << 24))

enum { DDS_HEADER_BYTES = 148 };

/* bytes of one block (block-compressed) or one texel of a DXGI format this layer reads or writes; 0: not one of them */
static uint32_t dxgi_unit(uint32_t dxgi, int* block) {
    *block = dxgi == 71 || dxgi == 77 || dxgi == 83 || dxgi == 95;
    switch (dxgi) {
    case 2: return 16;                                                        /* R32G32B32A32_FLOAT */
    case 10: return 8;                                                        /* R16G16B16A16_FLOAT */
    case 34: return 4;                                                        /* R16G16_FLOAT */
    case 28: return 4;                                                        /* R8G8B8A8_UNORM */
    case 71: return 8;                                                        /* BC1_UNORM */
    case 77: case 83: case 95: return 16;                                     /* BC3_UNORM, BC5_UNORM, BC6H_UF16 */
    default: return 0;
    }
}
static uint32_t full_chain(uint32_t width, uint32_t height) {
    uint32_t full = 1;
    for (uint32_t s = width > height ? width : height; s > 1; s >>= 1) full++;
    return full;
}
/* offsets of every (layer, level) from `header` on, face-major; returns the end of the last one */
static uint64_t fill_layout(PBR_DDSInfoEx* out, uint64_t header, uint32_t unit, int block) {
    uint64_t off = header;
    for (uint32_t l = 0; l < out->layers; ++l)
        for (uint32_t m = 0; m < out->level_count; ++m) {
            uint64_t w = out->width >> m, h = out->height >> m;
            if (w < 1) w = 1;
            if (h < 1) h = 1;
            out->level_size[m] = block ? ((w + 3) / 4) * ((h + 3) / 4) * unit : w * h * unit;       /* at most 2^32: no overflow */
            out->level_offset[l][m] = off;
            off += out->level_size[m];
        }
    return off;
}

int PBR_ParseDDSEx(const void* bytes, size_t size, PBR_DDSInfoEx* out) {
    if (!bytes || !out) return PBR_DDS_E_ARG;
    memset(out, 0, sizeof *out);
    const uint8_t* p = (const uint8_t*)bytes;
    if (size < 4 || rd32(p) != FOURCC('D', 'D', 'S', ' ')) return PBR_DDS_E_MAGIC;
    if (size < 128) return PBR_DDS_E_TRUNCATED;
    if (rd32(p + 4) != 124 || rd32(p + 76) != 32) return PBR_DDS_E_MAGIC;
    const uint32_t flags = rd32(p + 8), height = rd32(p + 12), width = rd32(p + 16), depth = rd32(p + 24), mips = rd32(p + 28);
    const uint32_t pf_flags = rd32(p + 80), fourcc = rd32(p + 84), caps2 = rd32(p + 112);
    if ((caps2 & 0x200000u) || ((flags & 0x800000u) && depth > 1)) return PBR_DDS_E_LAYOUT;          /* volume, DDSD_DEPTH */
    int cube = (caps2 & 0x200u) != 0;
    if (cube && (caps2 & 0xFC00u) != 0xFC00u) return PBR_DDS_E_LAYOUT;                               /* a cube with faces missing */
    uint64_t header = 128;
    uint32_t dxgi = 0;
    if (pf_flags & 0x4u) {                                                    /* DDPF_FOURCC */
        if (fourcc == FOURCC('D', 'X', 'T', '1')) dxgi = 71;
        else if (fourcc == FOURCC('D', 'X', 'T', '5')) dxgi = 77;
        else if (fourcc == FOURCC('A', 'T', 'I', '2') || fourcc == FOURCC('B', 'C', '5', 'U')) dxgi = 83;
        else if (fourcc == FOURCC('D', 'X', '1', '0')) {
            if (size < DDS_HEADER_BYTES) return PBR_DDS_E_TRUNCATED;
            header = DDS_HEADER_BYTES;
            const uint32_t dim = rd32(p + 132), misc = rd32(p + 136), array = rd32(p + 140);
            dxgi = rd32(p + 128);
            if (dim != 3 || array > 1) return PBR_DDS_E_LAYOUT;               /* TEXTURE2D only, one texture or one cube */
            if (misc & 0x4u) cube = 1;                                        /* the DX10 header decides; caps2 is optional beside it */
        } else return PBR_DDS_E_FORMAT;
    } else if ((pf_flags & 0x40u) && rd32(p + 88) == 32 && rd32(p + 92) == 0x000000FFu && rd32(p + 96) == 0x0000FF00u &&
               rd32(p + 100) == 0x00FF0000u && rd32(p + 104) == 0xFF000000u) {               /* DDPF_RGB, bytes R G B A */
        dxgi = 28;
    } else return PBR_DDS_E_FORMAT;
    int block;
    const uint32_t unit = dxgi_unit(dxgi, &block);
    if (!unit) return PBR_DDS_E_FORMAT;
    if (width == 0 || height == 0 || width > 16384 || height > 16384) return PBR_DDS_E_EXTENT;
    if (cube && width != height) return PBR_DDS_E_LAYOUT;
    const uint32_t levels = mips ? mips : 1;                                  /* 0: writers that leave the field unset */
    if (levels > full_chain(width, height) || levels > PBR_DDS_MAX_LEVELS) return PBR_DDS_E_LEVELS;
    out->dxgi_format = dxgi; out->width = width; out->height = height; out->layers = cube ? 6 : 1; out->level_count = levels;
    if (fill_layout(out, header, unit, block) > (uint64_t)size) { memset(out, 0, sizeof *out); return PBR_DDS_E_TRUNCATED; }
    return 0;
}

uint64_t PBR_BuildDDSHeader(uint32_t dxgi_format, uint32_t width, uint32_t height, uint32_t layers, uint32_t level_count, uint8_t header[148],
                            PBR_DDSInfoEx* layout) {
    int block;
    const uint32_t unit = dxgi_unit(dxgi_format, &block);
    if (!header || !unit || width == 0 || height == 0 || width > 16384 || height > 16384 || (layers != 1 && layers != 6) ||
        (layers == 6 && width != height) || level_count < 1 || level_count > full_chain(width, height) || level_count > PBR_DDS_MAX_LEVELS)
        return 0;
    PBR_DDSInfoEx info;
    memset(&info, 0, sizeof info);
    info.dxgi_format = dxgi_format; info.width = width; info.height = height; info.layers = layers; info.level_count = level_count;
    const uint64_t total = fill_layout(&info, DDS_HEADER_BYTES, unit, block);
    const int cube = layers == 6;
    memset(header, 0, DDS_HEADER_BYTES);
    wr32(header, FOURCC('D', 'D', 'S', ' '));
    wr32(header + 4, 124);
    /* CAPS | HEIGHT | WIDTH | PIXELFORMAT, MIPMAPCOUNT, LINEARSIZE (blocks: bytes of level 0) or PITCH (texels: bytes of a row) */
    wr32(header + 8, 0x1007u | (level_count > 1 ? 0x20000u : 0u) | (block ? 0x80000u : 0x8u));
    wr32(header + 12, height);
    wr32(header + 16, width);
    wr32(header + 20, block ? (uint32_t)info.level_size[0] : width * unit);
    wr32(header + 28, level_count);
    wr32(header + 76, 32);
    wr32(header + 80, 0x4u);                                                  /* DDPF_FOURCC */
    wr32(header + 84, FOURCC('D', 'X', '1', '0'));
    wr32(header + 108, 0x1000u | ((cube || level_count > 1) ? 0x8u : 0u) | (level_count > 1 ? 0x400000u : 0u));   /* TEXTURE, COMPLEX, MIPMAP */
    wr32(header + 112, cube ? 0x200u | 0xFC00u : 0u);                         /* CUBEMAP and all six faces */
    wr32(header + 128, dxgi_format);
    wr32(header + 132, 3);                                                    /* D3D10_RESOURCE_DIMENSION_TEXTURE2D */
    wr32(header + 136, cube ? 0x4u : 0u);                                     /* DDS_RESOURCE_MISC_TEXTURECUBE */
    wr32(header + 140, 1);                                                    /* one texture, or one cube */
    if (layout) *layout = info;
    return total;
}

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
    else if (out_format == PBR_DDS_OUT_BC6H_UF16 && (src_dxgi == 2 || src_dxgi == 10)) dxgi = 95;
    if (!dxgi) { fprintf(stderr, "GPU-ERROR: %s: texture format %d cannot be written as output format %d\n", fn, (int)texture->format, out_format); return NULL; }
    const uint32_t layers = texture->layer_count, w0 = level_dim(texture->width, first_mip), h0 = level_dim(texture->height, first_mip);
    uint8_t header[DDS_HEADER_BYTES];
    PBR_DDSInfoEx lay;
    const uint64_t total = PBR_BuildDDSHeader(dxgi, w0, h0, layers, mip_count, header, &lay);
    if (!total) { fprintf(stderr, "GPU-ERROR: %s: a %u x %u texture of %u layers and %u levels has no DDS form\n", fn, w0, h0, layers, mip_count); return NULL; }

    /* every level, all layers, into one mapped buffer in texture order (level-major), by one graph */
    const int bc6h = dxgi == 95;
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
        if (bc6h) GPUX_OpEncodeBC6H(g, texture, first_mip + m, staging, (uint32_t)stage_off[m]);
        else GPUX_OpCopyTextureMipToBuffer(g, texture, first_mip + m, staging, (uint32_t)stage_off[m]);
    }
    GPU_GraphSubmit(g);
    GPU_GraphWait(g);
    memcpy(file, header, DDS_HEADER_BYTES);
    const uint8_t* staged = (const uint8_t*)staging->data;
    const int narrow = dxgi == 10 && src_dxgi == 2;                           /* RGBA32F -> RGBA16F on the host, sign and Inf kept */
    for (uint32_t l = 0; l < layers; ++l)
        for (uint32_t m = 0; m < mip_count; ++m) {
            uint8_t* dst = file + lay.level_offset[l][m];
            if (!narrow) { memcpy(dst, staged + stage_off[m] + (uint64_t)l * lay.level_size[m], (size_t)lay.level_size[m]); continue; }
            const uint64_t n = lay.level_size[m] / 2;                         /* components */
            const uint8_t* src = staged + stage_off[m] + (uint64_t)l * n * 4;
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t hbits = bc6h_f16_from_f32(rd32(src + 4 * i));
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

GPU_Texture* PBR_MakeTextureFromFloatDDSMemory(const void* bytes, size_t size) {
    const char* fn = "PBR_MakeTextureFromFloatDDS";
    PBR_DDSInfoEx info;
    const int rc = PBR_ParseDDSEx(bytes, size, &info);
    if (rc != 0) { fprintf(stderr, "GPU-ERROR: %s: %s\n", fn, PBR_DDSErrorString(rc)); return NULL; }
    const GPU_Format format = info.dxgi_format == 2 ? GPU_Format_RGBA32F : info.dxgi_format == 10 ? GPU_Format_RGBA16F
                            : info.dxgi_format == 34 ? GPU_Format_RG16F : GPU_Format_Invalid;
    if (format == GPU_Format_Invalid) { fprintf(stderr, "GPU-ERROR: %s: DXGI format %u is not RGBA32F, RGBA16F or RG16F\n", fn, info.dxgi_format); return NULL; }
    const uint32_t flags = (info.layers == 6 ? GPU_TextureFlag_Cubemap : 0) | (info.level_count > 1 ? GPU_TextureFlag_HasMipmaps : 0);
    GPU_Texture* t = GPU_MakeTexture(format, info.width, info.height, 1, flags, NULL);
    if (!t) return NULL;
    if (t->mip_level_count != info.level_count) {
        fprintf(stderr, "GPU-ERROR: %s: the file holds %u levels, the chain has %u\n", fn, info.level_count, t->mip_level_count);
        GPU_DestroyTexture(t); return NULL;
    }
    uint64_t stage_off[PBR_DDS_MAX_LEVELS], stage_total = 0;
    for (uint32_t m = 0; m < info.level_count; ++m) { stage_off[m] = stage_total; stage_total += info.level_size[m] * info.layers; }
    GPU_Buffer* staging = stage_total <= 0xFFFFFFFFu ? GPU_MakeBuffer((uint32_t)stage_total, GPU_BufferFlag_CPU, NULL) : NULL;
    GPU_Graph* g = staging ? GPU_MakeGraph() : NULL;
    if (!g) { GPU_DestroyBuffer(staging); GPU_DestroyTexture(t); fprintf(stderr, "GPU-ERROR: %s: allocation failed\n", fn); return NULL; }
    const uint8_t* p = (const uint8_t*)bytes;
    for (uint32_t m = 0; m < info.level_count; ++m) {                         /* face-major file -> level-major texture */
        for (uint32_t l = 0; l < info.layers; ++l)
            memcpy((uint8_t*)staging->data + stage_off[m] + (uint64_t)l * info.level_size[m], p + info.level_offset[l][m], (size_t)info.level_size[m]);
        GPUX_OpCopyBufferToTextureMip(g, staging, (uint32_t)stage_off[m], t, m);
    }
    GPU_GraphSubmit(g);
    GPU_GraphWait(g);
    GPU_DestroyGraph(g);
    GPU_DestroyBuffer(staging);
    return t;
}

GPU_Texture* PBR_MakeTextureFromFloatDDSFile(const char* filepath) {
    FILE* f = filepath ? fopen(filepath, "rb") : NULL;
    if (!f) { fprintf(stderr, "GPU-ERROR: PBR_MakeTextureFromFloatDDSFile: cannot open %s\n", filepath ? filepath : "(null)"); return NULL; }
    GPU_Texture* t = NULL;
    void* buf = NULL;
    long n = -1;
    if (fseek(f, 0, SEEK_END) == 0) n = ftell(f);
    if (n > 0 && fseek(f, 0, SEEK_SET) == 0 && (buf = malloc((size_t)n)) != NULL && fread(buf, 1, (size_t)n, f) == (size_t)n)
        t = PBR_MakeTextureFromFloatDDSMemory(buf, (size_t)n);
    else fprintf(stderr, "GPU-ERROR: PBR_MakeTextureFromFloatDDSFile: cannot read %s\n", filepath);
    free(buf);
    fclose(f);
    return t;
}
