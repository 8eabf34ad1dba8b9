// sanitizer harness for the extended .dds parser and the header writer (host/pbr_dds.c alone, run on CPU only): every header
// PBR_BuildDDSHeader writes (eight formats, 2-D and cube, every level count) must parse back to the layout the writer used, one byte
// short must be rejected, and a few thousand mutations (bit flips, truncations, huge extents, lying level counts, random layouts)
// must either be rejected or describe (layer, level) ranges inside the buffer, which is an exact-size heap copy.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "pbr_host.h"

static uint32_t rs = 2463534242u;
static uint32_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 17; rs ^= rs << 5; return rs; }
static void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

static const uint32_t DXGI[8] = {2, 10, 34, 95, 28, 71, 77, 83};

/* parse an exact-size heap copy; 1 accepted, 0 rejected; ends the run on an accepted range outside the buffer */
static int parse_checked(const uint8_t* bytes, size_t n, PBR_DDSInfoEx* info) {
    uint8_t* exact = (uint8_t*)malloc(n ? n : 1);
    memcpy(exact, bytes, n);
    const int rc = PBR_ParseDDSEx(exact, n, info);
    if (rc == 0) {
        if (info->level_count < 1 || info->level_count > PBR_DDS_MAX_LEVELS || !info->width || !info->height || (info->layers != 1 && info->layers != 6)) {
            fprintf(stderr, "accepted a bad description\n"); exit(5);
        }
        uint64_t prev_end = 128;
        for (uint32_t l = 0; l < info->layers; ++l)
            for (uint32_t m = 0; m < info->level_count; ++m) {
                const uint64_t o = info->level_offset[l][m], s = info->level_size[m];
                if (s == 0 || o < prev_end || o > n || s > n - o) { fprintf(stderr, "layer %u level %u [%llu, +%llu) outside %zu bytes\n", l, m, (unsigned long long)o, (unsigned long long)s, n); exit(6); }
                volatile uint8_t first = exact[o], last = exact[o + s - 1];      /* touch both ends: ASan checks them */
                (void)first; (void)last;
                prev_end = o + s;
            }
    } else if (!PBR_DDSErrorString(rc) || rc >= 0) { fprintf(stderr, "bad error code %d\n", rc); exit(7); }
    free(exact);
    return rc == 0;
}

static int same_layout(const PBR_DDSInfoEx* a, const PBR_DDSInfoEx* b) {
    if (a->dxgi_format != b->dxgi_format || a->width != b->width || a->height != b->height || a->layers != b->layers || a->level_count != b->level_count) return 0;
    return memcmp(a->level_offset, b->level_offset, sizeof a->level_offset) == 0 && memcmp(a->level_size, b->level_size, sizeof a->level_size) == 0;
}

int main(void) {
    long accepted = 0, rejected = 0;
    PBR_DDSInfoEx info, lay;
    static uint8_t file[148 + 6 * 70000];
    for (int k = 0; k < 8; ++k)
        for (uint32_t layers = 1; layers <= 6; layers += 5)
            for (uint32_t levels = 1; levels <= 7; ++levels) {                /* a full chain of 48 or 64 x 48 has 6 or 7 levels */
                const uint32_t w = layers == 6 ? 48 : 64, h = 48;
                const uint64_t n = PBR_BuildDDSHeader(DXGI[k], w, h, layers, levels, file, &lay);
                if (layers == 6 && levels == 7) { if (n != 0) { fprintf(stderr, "7 levels of a 48^2 cube accepted by the writer\n"); return 4; } continue; }
                if (n == 0 || n > sizeof file) { fprintf(stderr, "format %u layers %u levels %u: no header\n", DXGI[k], layers, levels); return 4; }
                if (!parse_checked(file, (size_t)n, &info) || !same_layout(&info, &lay) || info.level_offset[0][0] != 148 ||
                    info.level_offset[layers - 1][levels - 1] + info.level_size[levels - 1] != n) {
                    fprintf(stderr, "format %u layers %u levels %u: not parsed back as written\n", DXGI[k], layers, levels); return 4;
                }
                if (parse_checked(file, (size_t)n - 1, &info)) { fprintf(stderr, "format %u layers %u levels %u: accepted one byte short\n", DXGI[k], layers, levels); return 4; }
            }
    {   /* writer arguments without a DDS form; volume, array, partial cube, non-square cube, other formats */
        if (PBR_BuildDDSHeader(98, 16, 16, 1, 1, file, NULL) || PBR_BuildDDSHeader(2, 0, 16, 1, 1, file, NULL) || PBR_BuildDDSHeader(2, 16, 16385, 1, 1, file, NULL) ||
            PBR_BuildDDSHeader(2, 16, 16, 2, 1, file, NULL) || PBR_BuildDDSHeader(2, 16, 8, 6, 1, file, NULL) || PBR_BuildDDSHeader(2, 16, 16, 1, 6, file, NULL) ||
            PBR_BuildDDSHeader(2, 16, 16, 1, 0, file, NULL) || PBR_BuildDDSHeader(2, 16, 16, 1, 1, NULL, NULL)) return 8;
        PBR_BuildDDSHeader(2, 16, 16, 1, 1, file, NULL); wr32(file + 112, 0x200000); if (parse_checked(file, sizeof file, &info)) return 8;
        PBR_BuildDDSHeader(2, 16, 16, 1, 1, file, NULL); wr32(file + 8, 0x80100F); wr32(file + 24, 4); if (parse_checked(file, sizeof file, &info)) return 8;
        PBR_BuildDDSHeader(2, 16, 16, 1, 1, file, NULL); wr32(file + 140, 6); if (parse_checked(file, sizeof file, &info)) return 8;
        PBR_BuildDDSHeader(2, 16, 16, 6, 1, file, NULL); wr32(file + 112, 0x200 | 0x7C00); if (parse_checked(file, sizeof file, &info)) return 8;
        PBR_BuildDDSHeader(2, 16, 16, 6, 1, file, NULL); wr32(file + 12, 8); if (parse_checked(file, sizeof file, &info)) return 8;
        PBR_BuildDDSHeader(2, 16, 16, 1, 1, file, NULL); wr32(file + 128, 98); if (parse_checked(file, sizeof file, &info)) return 8;        /* BC7 */
        PBR_BuildDDSHeader(2, 16, 16, 1, 1, file, NULL); wr32(file + 132, 4); if (parse_checked(file, sizeof file, &info)) return 8;         /* TEXTURE3D */
        if (PBR_ParseDDSEx(NULL, 10, &info) != PBR_DDS_E_ARG || PBR_ParseDDSEx(file, 10, NULL) != PBR_DDS_E_ARG) return 8;
    }
    for (int iter = 0; iter < 6000; ++iter) {
        const uint32_t layers = (rnd() & 1) ? 6 : 1, w = 1 + rnd() % 96, h = layers == 6 ? w : 1 + rnd() % 96;
        uint32_t full = 1;
        for (uint32_t s = w > h ? w : h; s > 1; s >>= 1) full++;
        const uint32_t levels = 1 + rnd() % full;
        const uint64_t total = PBR_BuildDDSHeader(DXGI[rnd() % 8], w, h, layers, levels, file, NULL);
        if (total == 0) { fprintf(stderr, "no header for %u x %u, %u layers, %u levels\n", w, h, layers, levels); return 9; }
        size_t n = total > sizeof file ? sizeof file : (size_t)total;
        const size_t hs = 148;
        switch (rnd() % 7) {
        case 0: n = rnd() % (n + 1); break;                                                          /* truncate */
        case 1: for (int k = 0; k < 1 + (int)(rnd() % 6); ++k) file[rnd() % hs] ^= (uint8_t)(1u << (rnd() % 8)); break;   /* bit flips in the header */
        case 2: wr32(file + 12 + 4 * (rnd() & 1), (rnd() & 1) ? 0xFFFFFFFFu - rnd() % 8 : (1u << (14 + rnd() % 18)) + rnd() % 3); break;   /* huge extents */
        case 3: wr32(file + 28, (rnd() & 1) ? 10 + rnd() % 100 : 0x80000000u + rnd()); break;        /* lying level count */
        case 4: wr32(file + 12, rnd()); wr32(file + 16, rnd()); wr32(file + 28, rnd()); break;
        case 5: break;                                                                               /* as written (or cut at the buffer's size) */
        default: for (size_t k = rnd() % hs; k < hs; ++k) file[k] = (uint8_t)rnd(); break;           /* garbage tail of the header */
        }
        if (parse_checked(file, n, &info)) accepted++; else rejected++;
    }
    printf("ok: %ld mutated files accepted, %ld rejected\n", accepted, rejected);
    return 0;
}
