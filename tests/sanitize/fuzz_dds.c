// sanitizer harness for the .dds header parser (host/pbr_dds.c, run on CPU only): the fixture header (argv[1], 128 bytes), synthesised
// headers of every accepted kind, and a few thousand mutations of them (bit flips, truncations, huge extents, lying level counts).
// Whatever PBR_ParseDDS accepts must describe levels that lie inside the buffer, which is an exact-size heap copy.  Links against
// pbr_dds.c alone: the container code calls nothing of the GPU layer.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "pbr_host.h"

static uint32_t rs = 2463534242u;
static uint32_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 17; rs ^= rs << 5; return rs; }
static void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* kind 0..2: FourCC DXT1 / DXT5 / ATI2, 3: BC5U, 4..7: DX10 with DXGI 71 / 77 / 83 / 28, 8: legacy RGBA masks */
static size_t make_header(uint8_t* h, int kind, uint32_t w, uint32_t ht, uint32_t mips) {
    memset(h, 0, 148);
    memcpy(h, "DDS ", 4);
    wr32(h + 4, 124); wr32(h + 8, 0x1007u | (mips > 1 ? 0x20000u : 0)); wr32(h + 12, ht); wr32(h + 16, w); wr32(h + 28, mips);
    wr32(h + 76, 32); wr32(h + 108, 0x1000);
    static const char* cc[4] = {"DXT1", "DXT5", "ATI2", "BC5U"};
    static const uint32_t dxgi[4] = {71, 77, 83, 28};
    if (kind < 4) { wr32(h + 80, 0x4); memcpy(h + 84, cc[kind], 4); return 128; }
    if (kind < 8) { wr32(h + 80, 0x4); memcpy(h + 84, "DX10", 4); wr32(h + 128, dxgi[kind - 4]); wr32(h + 132, 3); wr32(h + 140, 1); return 148; }
    wr32(h + 80, 0x41); wr32(h + 88, 32); wr32(h + 92, 0xFFu); wr32(h + 96, 0xFF00u); wr32(h + 100, 0xFF0000u); wr32(h + 104, 0xFF000000u);
    return 128;
}
static uint64_t payload(int kind, uint32_t w, uint32_t h, uint32_t mips) {
    const int bc = !(kind == 7 || kind == 8);
    const uint64_t unit = (kind == 0 || kind == 4) ? 8 : (bc ? 16 : 4);
    uint64_t n = 0;
    for (uint32_t m = 0; m < mips; ++m) {
        uint64_t lw = w >> m ? w >> m : 1, lh = h >> m ? h >> m : 1;
        n += bc ? ((lw + 3) / 4) * ((lh + 3) / 4) * unit : lw * lh * unit;
    }
    return n;
}
/* parse an exact-size heap copy; 1 accepted, 0 rejected; aborts the run on an accepted level outside the buffer */
static int parse_checked(const uint8_t* bytes, size_t n, PBR_DDSInfo* info) {
    uint8_t* exact = (uint8_t*)malloc(n ? n : 1);
    memcpy(exact, bytes, n);
    const int rc = PBR_ParseDDS(exact, n, info);
    if (rc == 0) {
        if (info->level_count < 1 || info->level_count > PBR_DDS_MAX_LEVELS || !info->width || !info->height) { fprintf(stderr, "accepted a bad description\n"); exit(5); }
        uint64_t prev_end = 0;
        for (uint32_t m = 0; m < info->level_count; ++m) {
            const uint64_t o = info->level_offset[m], s = info->level_size[m];
            if (s == 0 || o < 128 || o < prev_end || o > n || s > n - o) { fprintf(stderr, "level %u [%llu, +%llu) outside %zu bytes\n", m, (unsigned long long)o, (unsigned long long)s, n); exit(6); }
            volatile uint8_t first = exact[o], last = exact[o + s - 1];          /* touch both ends: ASan checks them */
            (void)first; (void)last;
            prev_end = o + s;
        }
    } else if (!PBR_DDSErrorString(rc) || rc >= 0) { fprintf(stderr, "bad error code %d\n", rc); exit(7); }
    free(exact);
    return rc == 0;
}

int main(int argc, char** argv) {
    long accepted = 0, rejected = 0;
    PBR_DDSInfo info;
    static uint8_t file[148 + 70000];
    if (argc > 1) {                                                            /* the recorded header of a real 2048^2 DXT1 file with 12 levels */
        FILE* f = fopen(argv[1], "rb");
        uint8_t head[128];
        if (!f || fread(head, 1, 128, f) != 128) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        fclose(f);
        const size_t total = 128 + 2796216;
        uint8_t* big = (uint8_t*)calloc(1, total);
        memcpy(big, head, 128);
        if (!parse_checked(big, total, &info) || info.format != GPU_Format_BC1_RGBA_UN || info.width != 2048 || info.height != 2048 || info.level_count != 12 ||
            info.level_offset[0] != 128 || info.level_size[0] != 2097152 || info.level_size[11] != 8) { fprintf(stderr, "fixture header misparsed\n"); return 3; }
        if (parse_checked(big, total - 1, &info) || parse_checked(big, 128, &info)) { fprintf(stderr, "truncated fixture accepted\n"); return 3; }
        free(big);
    }
    for (int kind = 0; kind < 9; ++kind) {                                    /* every accepted kind, with and without levels */
        static const GPU_Format want[9] = {GPU_Format_BC1_RGBA_UN, GPU_Format_BC3_RGBA_UN, GPU_Format_BC5_UN, GPU_Format_BC5_UN, GPU_Format_BC1_RGBA_UN,
                                           GPU_Format_BC3_RGBA_UN, GPU_Format_BC5_UN, GPU_Format_RGBA8UN, GPU_Format_RGBA8UN};
        for (uint32_t mips = 0; mips <= 7; ++mips) {
            const size_t hs = make_header(file, kind, 64, 48, mips);
            const size_t n = hs + (size_t)payload(kind, 64, 48, mips ? mips : 1);
            if (!parse_checked(file, n, &info) || info.format != want[kind] || info.width != 64 || info.height != 48 || info.level_count != (mips ? mips : 1) ||
                info.level_offset[0] != hs) { fprintf(stderr, "kind %d mips %u not accepted as written\n", kind, mips); return 4; }
            if (parse_checked(file, n - 1, &info)) { fprintf(stderr, "kind %d mips %u: accepted one byte short\n", kind, mips); return 4; }
        }
        make_header(file, kind, 64, 48, 8);                                   /* a full chain of 64 x 48 has 7 levels */
        if (parse_checked(file, sizeof file, &info)) { fprintf(stderr, "kind %d: 8 levels of 64 x 48 accepted\n", kind); return 4; }
    }
    {   /* cube, volume, array, other formats */
        make_header(file, 0, 16, 16, 1); wr32(file + 112, 0x200); if (parse_checked(file, 4096, &info)) return 8;
        make_header(file, 0, 16, 16, 1); wr32(file + 112, 0x200000); if (parse_checked(file, 4096, &info)) return 8;
        make_header(file, 0, 16, 16, 1); wr32(file + 8, 0x801007); wr32(file + 24, 4); if (parse_checked(file, 4096, &info)) return 8;
        make_header(file, 4, 16, 16, 1); wr32(file + 140, 6); if (parse_checked(file, 4096, &info)) return 8;
        make_header(file, 4, 16, 16, 1); wr32(file + 136, 4); if (parse_checked(file, 4096, &info)) return 8;
        make_header(file, 4, 16, 16, 1); wr32(file + 128, 98); if (parse_checked(file, 4096, &info)) return 8;       /* BC7 */
        make_header(file, 0, 16, 16, 1); memcpy(file + 84, "DXT3", 4); if (parse_checked(file, 4096, &info)) return 8;
        make_header(file, 8, 16, 16, 1); wr32(file + 92, 0xFF0000u); wr32(file + 100, 0xFFu); if (parse_checked(file, 4096, &info)) return 8;   /* BGRA */
    }
    for (int iter = 0; iter < 6000; ++iter) {
        const int kind = (int)(rnd() % 9);
        uint32_t w = 1 + rnd() % 96, h = 1 + rnd() % 96, mips = rnd() % 9;
        const size_t hs = make_header(file, kind, w, h, mips);
        size_t n = hs + (size_t)payload(kind, w, h, mips ? mips : 1);
        if (n > sizeof file) n = sizeof file;
        switch (rnd() % 6) {
        case 0: n = rnd() % (n + 1); break;                                                          /* truncate */
        case 1: for (int k = 0; k < 1 + (int)(rnd() % 6); ++k) file[rnd() % hs] ^= (uint8_t)(1u << (rnd() % 8)); break;   /* bit flips in the header */
        case 2: wr32(file + 12 + 4 * (rnd() & 1), (rnd() & 1) ? 0xFFFFFFFFu - rnd() % 8 : (1u << (14 + rnd() % 18)) + rnd() % 3); break;   /* huge extents */
        case 3: wr32(file + 28, (rnd() & 1) ? 10 + rnd() % 100 : 0x80000000u + rnd()); break;        /* lying level count */
        case 4: wr32(file + 12, rnd()); wr32(file + 16, rnd()); wr32(file + 28, rnd()); break;
        default: for (size_t k = rnd() % hs; k < hs; ++k) file[k] = (uint8_t)rnd(); break;           /* garbage tail of the header */
        }
        if (parse_checked(file, n, &info)) accepted++; else rejected++;
    }
    printf("ok: %ld mutated files accepted, %ld rejected\n", accepted, rejected);
    return 0;
}
