// csrc/bc6h2_core.h compiled for the host: <source 0 = RGBA32F, 1 = RGBA16F> <width> <height> <layers> <texels file> <blocks file> <info file>.
// Encodes the level exactly as the K18 two-region kernel walks it: block by block, row-major within a layer, texels past the edge
// clamped.  The info file holds per block three little-endian uint64: kind, partition, squared error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bc6h2_core.h"

int main(int argc, char** argv) {
    if (argc != 8) { fprintf(stderr, "usage: %s source width height layers texels.bin blocks.bin info.bin\n", argv[0]); return 2; }
    const int src = atoi(argv[1]), w = atoi(argv[2]), h = atoi(argv[3]), layers = atoi(argv[4]);
    if (src < 0 || src > 1 || w < 1 || h < 1 || layers < 1 || w > 16384 || h > 16384) return 2;
    const size_t texel = src == 0 ? 16 : 8, need = (size_t)w * h * layers * texel;
    std::vector<uint8_t> in(need);                                            // exact size: a sanitizer sees any over-read
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(in.data(), 1, need, f) != need || fgetc(f) != EOF) { fprintf(stderr, "texels file: need exactly %zu bytes\n", need); return 3; }
    fclose(f);
    const int bw = (w + 3) / 4, bh = (h + 3) / 4;
    std::vector<uint8_t> out((size_t)bw * bh * layers * 16);
    std::vector<uint64_t> chosen((size_t)bw * bh * layers * 3);
    size_t ob = 0;
    for (int l = 0; l < layers; ++l)
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx, ++ob) {
                uint32_t codes[16][3];
                for (int t = 0; t < 16; ++t) {
                    const int x = 4 * bx + (t & 3) < w ? 4 * bx + (t & 3) : w - 1, y = 4 * by + (t >> 2) < h ? 4 * by + (t >> 2) : h - 1;
                    const uint8_t* p = in.data() + (((size_t)l * h + y) * w + x) * texel;
                    for (int c = 0; c < 3; ++c) {
                        if (src == 0) { uint32_t v; memcpy(&v, p + 4 * c, 4); codes[t][c] = bc6h_code_from_f32(v); }
                        else { uint16_t v; memcpy(&v, p + 2 * c, 2); codes[t][c] = bc6h_code_from_f16(v); }
                    }
                }
                uint32_t words[4];
                Bc6h2Info info;
                bc6h2_encode_block(codes, words, &info);
                memcpy(out.data() + 16 * ob, words, 16);
                chosen[3 * ob] = info.kind; chosen[3 * ob + 1] = info.partition; chosen[3 * ob + 2] = info.err;
            }
    f = fopen(argv[6], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
    fclose(f);
    f = fopen(argv[7], "wb");
    if (!f || fwrite(chosen.data(), 8, chosen.size(), f) != chosen.size()) return 4;
    fclose(f);
    return 0;
}
