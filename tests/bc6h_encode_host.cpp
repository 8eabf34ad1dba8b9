// csrc/bc6h_core.h and csrc/bc6h2_core.h compiled for the host:
//     <quality 0 = one region, 1 = two regions> <source 0 = RGBA32F, 1 = RGBA16F> <width> <height> <layers> <texels file> <blocks file>
//     and, at quality 1 only, <info file>.
// Encodes the level exactly as the K18 kernel walks it: block by block, row-major within a layer, texels past the edge clamped.  The
// info file holds per block three little-endian uint64: kind, partition, squared error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bc6h2_core.h"

int main(int argc, char** argv) {
    const int quality = argc > 1 ? atoi(argv[1]) : -1;
    if (quality < 0 || quality > 1 || argc != 8 + quality) {
        fprintf(stderr, "usage: %s quality source width height layers texels.bin blocks.bin [info.bin at quality 1]\n", argv[0]);
        return 2;
    }
    const int src = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]), layers = atoi(argv[5]);
    if (src < 0 || src > 1 || w < 1 || h < 1 || layers < 1 || w > 16384 || h > 16384) return 2;
    const size_t texel = src == 0 ? 16 : 8, need = (size_t)w * h * layers * texel;
    std::vector<uint8_t> in(need);                                            // exact size: a sanitizer sees any over-read
    FILE* f = fopen(argv[6], "rb");
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
                if (quality == 1) {
                    Bc6h2Info info;
                    bc6h2_encode_block(codes, words, &info);
                    chosen[3 * ob] = info.kind; chosen[3 * ob + 1] = info.partition; chosen[3 * ob + 2] = info.err;
                } else {
                    bc6h_encode_block(codes, words);
                }
                memcpy(out.data() + 16 * ob, words, 16);
            }
    f = fopen(argv[7], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
    fclose(f);
    if (quality == 1) {
        f = fopen(argv[8], "wb");
        if (!f || fwrite(chosen.data(), 8, chosen.size(), f) != chosen.size()) return 4;
        fclose(f);
    }
    return 0;
}
