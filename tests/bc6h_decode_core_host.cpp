// csrc/bc6h_decode_core.h compiled for the host:
//     decode <width> <height> <layers> <blocks file> <codes file>   half codes uint16 [layers][h][w][3], texels outside the level dropped
//     widen <bits file>                                             bc6hd_f32_from_code of every code 0 .. 0x7BFF as uint32
// Decodes the level as the K19 kernel walks it -- one 4-texel row of a block at a time (bc6hd_decode_row) -- and holds every block
// against the whole-block form (bc6hd_decode_block).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bc6h_decode_core.h"

static int write_file(const char* path, const void* data, size_t bytes) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(data, 1, bytes, f) != bytes) return 4;
    return fclose(f) == 0 ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "widen") == 0) {
        std::vector<uint32_t> bits(0x7C00);
        for (uint32_t h = 0; h < 0x7C00u; ++h) bits[h] = bc6hd_f32_from_code(h);
        return write_file(argv[2], bits.data(), bits.size() * 4);
    }
    if (argc != 7 || strcmp(argv[1], "decode") != 0) { fprintf(stderr, "usage: %s decode width height layers blocks.bin codes.bin | widen bits.bin\n", argv[0]); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]), layers = atoi(argv[4]);
    if (w < 1 || h < 1 || layers < 1 || w > 16384 || h > 16384) return 2;
    const int bw = (w + 3) / 4, bh = (h + 3) / 4;
    const size_t need = (size_t)bw * bh * layers * 16;
    std::vector<uint8_t> in(need);                                            // exact size: a sanitizer sees any over-read
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(in.data(), 1, need, f) != need || fgetc(f) != EOF) { fprintf(stderr, "blocks file: need exactly %zu bytes\n", need); return 3; }
    fclose(f);
    std::vector<uint16_t> out((size_t)w * h * layers * 3);
    for (int l = 0; l < layers; ++l)
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx) {
                uint32_t words[4], whole[16][3];
                memcpy(words, in.data() + (((size_t)l * bh + by) * bw + bx) * 16, 16);
                bc6hd_decode_block(words, whole);
                for (int row = 0; row < 4; ++row) {
                    uint32_t rgb[4][3];
                    bc6hd_decode_row(words, (uint32_t)row, rgb);
                    if (memcmp(rgb, whole[4 * row], sizeof rgb) != 0) { fprintf(stderr, "row %d of block %d %d %d differs from the whole-block decode\n", row, l, by, bx); return 5; }
                    const int y = 4 * by + row;
                    for (int x = 0; x < 4 && y < h; ++x) {
                        if (4 * bx + x >= w) break;
                        uint16_t* o = out.data() + (((size_t)l * h + y) * w + 4 * bx + x) * 3;
                        for (int c = 0; c < 3; ++c) o[c] = (uint16_t)rgb[x][c];
                    }
                }
            }
    return write_file(argv[6], out.data(), out.size() * 2);
}
