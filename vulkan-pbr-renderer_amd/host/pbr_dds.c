/*
 * pbr_dds.c -- the .dds container (C11): the header parse that asset_import.cpp:30-60 (LoadMeshTexture) gets from
 * ddspp, restated with every offset checked against the file, and the header the bake's files are written with.  Byte arithmetic
 * only: nothing here calls the GPU layer.  host/pbr_ddsin.c makes textures of what the parsers describe, host/pbr_ddsout.c files of
 * what PBR_BuildDDSHeader lays out.
 *
 * File layout (Microsoft's DDS programming guide): "DDS " magic, a 124-byte DDS_HEADER whose pixel format sits at byte 76 of the
 * file, an optional 20-byte DDS_HEADER_DXT10 when the FourCC is "DX10", then for a cube the six faces in the order +X -X +Y -Y +Z -Z
 * (the texture's layer order, face_texel_dir), each face -- or the one surface -- with its levels largest first, tight.
 */
#include "pbr_host.h"

#include <string.h>

static uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
#define FOURCC(a, b, c, d) ((uint32_t)(a) | ((uint32_t)(b) << 8) | ((uint32_t)(c) << 16) | ((uint32_t)(d) << 24))

enum { DDS_HEADER_BYTES = 148 };

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
/* the material formats, all PBR_ParseDDS accepts (asset_import.cpp:47) */
static GPU_Format material_format(uint32_t dxgi) {
    return dxgi == 71 ? GPU_Format_BC1_RGBA_UN : dxgi == 77 ? GPU_Format_BC3_RGBA_UN : dxgi == 83 ? GPU_Format_BC5_UN
         : dxgi == 28 ? GPU_Format_RGBA8UN : GPU_Format_Invalid;
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

/* both parsers.  wide: cubes and every format of dxgi_unit; otherwise one 2-D surface of a material format.  *out is zero on entry
 * and on every error. */
static int parse(const uint8_t* p, size_t size, int wide, PBR_DDSInfoEx* out) {
    if (size < 4 || rd32(p) != FOURCC('D', 'D', 'S', ' ')) return PBR_DDS_E_MAGIC;
    if (size < 128) return PBR_DDS_E_TRUNCATED;
    if (rd32(p + 4) != 124 || rd32(p + 76) != 32) return PBR_DDS_E_MAGIC;
    const uint32_t flags = rd32(p + 8), height = rd32(p + 12), width = rd32(p + 16), depth = rd32(p + 24), mips = rd32(p + 28);
    const uint32_t pf_flags = rd32(p + 80), fourcc = rd32(p + 84), caps2 = rd32(p + 112);
    if ((caps2 & 0x200000u) || ((flags & 0x800000u) && depth > 1)) return PBR_DDS_E_LAYOUT;          /* volume, DDSD_DEPTH */
    int cube = (caps2 & 0x200u) != 0;
    if (cube && (!wide || (caps2 & 0xFC00u) != 0xFC00u)) return PBR_DDS_E_LAYOUT;                    /* no cubes, or one with faces missing */
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
            if (dim != 3 || array > 1 || (!wide && (misc & 0x4u))) return PBR_DDS_E_LAYOUT;          /* TEXTURE2D only, one texture or one cube */
            if (misc & 0x4u) cube = 1;                                        /* the DX10 header decides; caps2 is optional beside it */
        } else return PBR_DDS_E_FORMAT;
    } else if ((pf_flags & 0x40u) && rd32(p + 88) == 32 && rd32(p + 92) == 0x000000FFu && rd32(p + 96) == 0x0000FF00u &&
               rd32(p + 100) == 0x00FF0000u && rd32(p + 104) == 0xFF000000u) {               /* DDPF_RGB, bytes R G B A */
        dxgi = 28;
    } else return PBR_DDS_E_FORMAT;
    int block;
    const uint32_t unit = dxgi_unit(dxgi, &block);
    if (!unit || (!wide && material_format(dxgi) == GPU_Format_Invalid)) return PBR_DDS_E_FORMAT;
    if (width == 0 || height == 0 || width > 16384 || height > 16384) return PBR_DDS_E_EXTENT;
    if (cube && width != height) return PBR_DDS_E_LAYOUT;
    const uint32_t levels = mips ? mips : 1;                                  /* 0: writers that leave the field unset */
    if (levels > full_chain(width, height) || levels > PBR_DDS_MAX_LEVELS) return PBR_DDS_E_LEVELS;
    out->dxgi_format = dxgi; out->width = width; out->height = height; out->layers = cube ? 6 : 1; out->level_count = levels;
    if (fill_layout(out, header, unit, block) > (uint64_t)size) { memset(out, 0, sizeof *out); return PBR_DDS_E_TRUNCATED; }
    return 0;
}

int PBR_ParseDDSEx(const void* bytes, size_t size, PBR_DDSInfoEx* out) {
    if (!bytes || !out) return PBR_DDS_E_ARG;
    memset(out, 0, sizeof *out);
    return parse((const uint8_t*)bytes, size, 1, out);
}

int PBR_ParseDDS(const void* bytes, size_t size, PBR_DDSInfo* out) {
    if (!bytes || !out) return PBR_DDS_E_ARG;
    memset(out, 0, sizeof *out);
    PBR_DDSInfoEx ex;
    memset(&ex, 0, sizeof ex);
    const int rc = parse((const uint8_t*)bytes, size, 0, &ex);
    if (rc != 0) return rc;
    out->format = material_format(ex.dxgi_format); out->width = ex.width; out->height = ex.height; out->level_count = ex.level_count;
    memcpy(out->level_offset, ex.level_offset[0], sizeof out->level_offset);
    memcpy(out->level_size, ex.level_size, sizeof out->level_size);
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
