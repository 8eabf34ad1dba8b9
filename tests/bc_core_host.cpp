// csrc/bc_core.h compiled for the host: <format 0..3> <width> <height> <blocks file> <rgba8 file>.  Decodes the level exactly as the
// K15 kernel walks it (one 4-texel row of one block at a time, texels outside the level dropped) and writes tight RGBA8 rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bc_core.h"

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s format width height blocks.bin out.bin\n", argv[0]); return 2; }
    const int fmt = atoi(argv[1]), w = atoi(argv[2]), h = atoi(argv[3]);
    if (fmt < 0 || fmt > 3 || w < 1 || h < 1 || w > 16384 || h > 16384) return 2;
    const int bw = (w + 3) / 4, bh = (h + 3) / 4;
    const size_t nb = bc_block_bytes(fmt), need = (size_t)bw * bh * nb;
    std::vector<uint8_t> blocks(need);                                        // exact size: a sanitizer sees any over-read
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(blocks.data(), 1, need, f) != need || fgetc(f) != EOF) { fprintf(stderr, "blocks file: need exactly %zu bytes\n", need); return 3; }
    fclose(f);
    std::vector<uint8_t> out((size_t)w * h * 4);
    for (int by = 0; by < bh; ++by)
        for (int bx = 0; bx < bw; ++bx) {
            uint32_t words[4] = {0, 0, 0, 0};
            memcpy(words, blocks.data() + ((size_t)by * bw + bx) * nb, nb);
            for (int row = 0; row < 4; ++row) {
                const int y = by * 4 + row;
                if (y >= h) break;
                uint32_t px[4];
                bc_decode_row(fmt, words, row, px);
                for (int x = 0; x < 4 && 4 * bx + x < w; ++x) memcpy(out.data() + ((size_t)y * w + 4 * bx + x) * 4, &px[x], 4);
            }
        }
    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
    fclose(f);
    return 0;
}
