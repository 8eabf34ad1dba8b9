/*
 * pbr_dds.c -- .dds material textures (C11): the header parse that asset_import.cpp:30-60 (LoadMeshTexture) gets from
 * ddspp, restated with every offset checked against the file, and the upload of the levels.  BC1 / BC3 / BC5 payloads go to the
 * backend as they are; it decodes them with K15.
 *
 * File layout (Microsoft's DDS programming guide): "DDS " magic, a 124-byte DDS_HEADER whose pixel format sits at byte 76 of the
 * file, an optional 20-byte DDS_HEADER_DXT10 when the FourCC is "DX10", then the levels of the one surface, largest first, tight.
 */
#include "pbr_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
#define FOURCC(a, b, c, d) ((uint32_t)(a) | ((uint32_t)(b) << 8) | ((uint32_t)(c) << 16) | ((uint32_t)(d) << 24))

const char* PBR_DDSErrorString(int code) {
    switch (code) {
    case 0: return "ok";
    case PBR_DDS_E_ARG: return "NULL argument";
    case PBR_DDS_E_MAGIC: return "not a DDS file (magic or header size)";
    case PBR_DDS_E_TRUNCATED: return "file is shorter than its header or its levels";
    case PBR_DDS_E_FORMAT: return "pixel format is not DXT1, DXT5, ATI2 / BC5U, DXGI 71 / 77 / 83 / 28 or 32-bit RGBA";
    case PBR_DDS_E_LAYOUT: return "cube, volume and array files are not supported";
    case PBR_DDS_E_EXTENT: return "width or height is 0 or above 16384";
    case PBR_DDS_E_LEVELS: return "level count exceeds a full chain";
    default: return "unknown error";
    }
}

int PBR_ParseDDS(const void* bytes, size_t size, PBR_DDSInfo* out) {
    if (!bytes || !out) return PBR_DDS_E_ARG;
    memset(out, 0, sizeof *out);
    const uint8_t* p = (const uint8_t*)bytes;
    if (size < 4 || rd32(p) != FOURCC('D', 'D', 'S', ' ')) return PBR_DDS_E_MAGIC;
    if (size < 128) return PBR_DDS_E_TRUNCATED;
    if (rd32(p + 4) != 124 || rd32(p + 76) != 32) return PBR_DDS_E_MAGIC;
    const uint32_t flags = rd32(p + 8), height = rd32(p + 12), width = rd32(p + 16), depth = rd32(p + 24), mips = rd32(p + 28);
    const uint32_t pf_flags = rd32(p + 80), fourcc = rd32(p + 84), caps2 = rd32(p + 112);
    if ((caps2 & 0x200u) || (caps2 & 0x200000u) || ((flags & 0x800000u) && depth > 1)) return PBR_DDS_E_LAYOUT;   /* cube, volume, DDSD_DEPTH */
    size_t header = 128;
    GPU_Format format = GPU_Format_Invalid;
    if (pf_flags & 0x4u) {                                                    /* DDPF_FOURCC */
        if (fourcc == FOURCC('D', 'X', 'T', '1')) format = GPU_Format_BC1_RGBA_UN;          /* asset_import.cpp:47 */
        else if (fourcc == FOURCC('D', 'X', 'T', '5')) format = GPU_Format_BC3_RGBA_UN;
        else if (fourcc == FOURCC('A', 'T', 'I', '2') || fourcc == FOURCC('B', 'C', '5', 'U')) format = GPU_Format_BC5_UN;
        else if (fourcc == FOURCC('D', 'X', '1', '0')) {
            if (size < 148) return PBR_DDS_E_TRUNCATED;
            header = 148;
            const uint32_t dxgi = rd32(p + 128), dim = rd32(p + 132), misc = rd32(p + 136), array = rd32(p + 140);
            if (dim != 3 || (misc & 0x4u) || array > 1) return PBR_DDS_E_LAYOUT;             /* TEXTURE2D only, no cube, no array */
            if (dxgi == 71) format = GPU_Format_BC1_RGBA_UN;
            else if (dxgi == 77) format = GPU_Format_BC3_RGBA_UN;
            else if (dxgi == 83) format = GPU_Format_BC5_UN;
            else if (dxgi == 28) format = GPU_Format_RGBA8UN;
            else return PBR_DDS_E_FORMAT;
        } else return PBR_DDS_E_FORMAT;
    } else if ((pf_flags & 0x40u) && rd32(p + 88) == 32 && rd32(p + 92) == 0x000000FFu && rd32(p + 96) == 0x0000FF00u &&
               rd32(p + 100) == 0x00FF0000u && rd32(p + 104) == 0xFF000000u) {               /* DDPF_RGB, bytes R G B A */
        format = GPU_Format_RGBA8UN;
    } else return PBR_DDS_E_FORMAT;
    if (width == 0 || height == 0 || width > 16384 || height > 16384) return PBR_DDS_E_EXTENT;
    const uint32_t levels = mips ? mips : 1;                                  /* 0: writers that leave the field unset */
    uint32_t full = 1;
    for (uint32_t s = width > height ? width : height; s > 1; s >>= 1) full++;
    if (levels > full || levels > PBR_DDS_MAX_LEVELS) return PBR_DDS_E_LEVELS;
    const int bc = format != GPU_Format_RGBA8UN;
    const uint64_t unit = format == GPU_Format_BC1_RGBA_UN ? 8 : (bc ? 16 : 4);
    uint64_t off = header;
    for (uint32_t m = 0; m < levels; ++m) {
        uint64_t w = width >> m, h = height >> m;
        if (w < 1) w = 1;
        if (h < 1) h = 1;
        const uint64_t bytes_m = bc ? ((w + 3) / 4) * ((h + 3) / 4) * unit : w * h * unit;     /* at most 2^30: no overflow */
        if (off + bytes_m > (uint64_t)size) { memset(out, 0, sizeof *out); return PBR_DDS_E_TRUNCATED; }
        out->level_offset[m] = off; out->level_size[m] = bytes_m;
        off += bytes_m;
    }
    out->format = format; out->width = width; out->height = height; out->level_count = levels;
    return 0;
}

GPU_Texture* PBR_MakeTextureFromDDSMemory(const void* bytes, size_t size, uint32_t flags) {
    PBR_DDSInfo info;
    const int rc = PBR_ParseDDS(bytes, size, &info);
    if (rc != 0) { fprintf(stderr, "GPU-ERROR: PBR_MakeTextureFromDDS: %s\n", PBR_DDSErrorString(rc)); return NULL; }
    const uint8_t* p = (const uint8_t*)bytes;
    if (!(flags & PBR_DDS_FILE_MIPS) || info.level_count == 1)                /* asset_import.cpp:53 */
        return GPU_MakeTexture(info.format, info.width, info.height, 1, 0, p + info.level_offset[0]);
    GPU_Texture* t = GPU_MakeTexture(info.format, info.width, info.height, 1, GPU_TextureFlag_HasMipmaps, NULL);
    if (!t) return NULL;
    const uint32_t n = t->mip_level_count;                                    /* counted from the smaller extent */
    if (info.level_count < n) {
        fprintf(stderr, "GPU-ERROR: PBR_MakeTextureFromDDS: the file holds %u levels, the chain needs %u\n", info.level_count, n);
        GPU_DestroyTexture(t); return NULL;
    }
    const uint64_t span = info.level_offset[n - 1] + info.level_size[n - 1] - info.level_offset[0];     /* < 2^31 */
    GPU_Buffer* staging = GPU_MakeBuffer((uint32_t)span, GPU_BufferFlag_CPU, p + info.level_offset[0]);
    GPU_Graph* g = staging ? GPU_MakeGraph() : NULL;
    if (!g) { GPU_DestroyBuffer(staging); GPU_DestroyTexture(t); return NULL; }
    for (uint32_t m = 0; m < n; ++m) GPUX_OpCopyBufferToTextureMip(g, staging, (uint32_t)(info.level_offset[m] - info.level_offset[0]), t, m);
    GPU_GraphSubmit(g);
    GPU_GraphWait(g);
    GPU_DestroyGraph(g);
    GPU_DestroyBuffer(staging);
    return t;
}

GPU_Texture* PBR_MakeTextureFromDDSFile(const char* filepath, uint32_t flags) {
    FILE* f = filepath ? fopen(filepath, "rb") : NULL;
    if (!f) { fprintf(stderr, "GPU-ERROR: PBR_MakeTextureFromDDSFile: cannot open %s\n", filepath ? filepath : "(null)"); return NULL; }
    GPU_Texture* t = NULL;
    void* buf = NULL;
    long n = -1;
    if (fseek(f, 0, SEEK_END) == 0) n = ftell(f);
    if (n > 0 && fseek(f, 0, SEEK_SET) == 0 && (buf = malloc((size_t)n)) != NULL && fread(buf, 1, (size_t)n, f) == (size_t)n)
        t = PBR_MakeTextureFromDDSMemory(buf, (size_t)n, flags);
    else fprintf(stderr, "GPU-ERROR: PBR_MakeTextureFromDDSFile: cannot read %s\n", filepath);
    free(buf);
    fclose(f);
    return t;
}
