// Host build of csrc/prefilter_ggx_core.h (tests/test_prefilter_ggx_cpu.py): the table, and for every texel of a size^2 level the
// frame and the direction of every kept sample, as raw fp32 on stdout:
//   uint32 kept, float wsum, float table[kept][4], then per face, y, x: float Nrm[3], T[3], B[3], d[kept][3]
// usage: prefilter_ggx_core_host roughness sample_count src_size src_levels lod_bias size
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prefilter_ggx_core.h"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const float roughness = strtof(argv[1], nullptr), bias = strtof(argv[5], nullptr);
    const uint32_t count = (uint32_t)atoi(argv[2]), n0 = (uint32_t)atoi(argv[3]), levels = (uint32_t)atoi(argv[4]);
    const int size = atoi(argv[6]);
    if (count < 1 || count > PGGX_MAX_SAMPLES || n0 < 1 || levels < 1 || size < 1) return 2;
    std::vector<float> table(4 * (size_t)count);
    float wsum = 0.0f;
    const uint32_t kept = pggx_fill_table(roughness, count, n0, levels, bias, table.data(), &wsum);
    std::vector<float> out;
    for (int face = 0; face < 6; ++face)
        for (int y = 0; y < size; ++y)
            for (int x = 0; x < size; ++x) {
                float f[9];
                pggx_texel_dir(face, x, y, size, f);
                pggx_frame(f, f + 3, f + 6);
                out.insert(out.end(), f, f + 9);
                for (uint32_t i = 0; i < kept; ++i) {
                    float d[3];
                    pggx_sample_dir(f, f + 3, f + 6, table[4 * i], table[4 * i + 1], table[4 * i + 2], d);
                    out.insert(out.end(), d, d + 3);
                }
            }
    if (fwrite(&kept, 4, 1, stdout) != 1 || fwrite(&wsum, 4, 1, stdout) != 1) return 1;
    if (kept && fwrite(table.data(), 16, kept, stdout) != kept) return 1;
    if (fwrite(out.data(), 4, out.size(), stdout) != out.size()) return 1;
    return 0;
}
