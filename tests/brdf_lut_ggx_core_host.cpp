// Host build of csrc/brdf_lut_ggx_core.h (tests/test_brdf_lut_ggx_cpu.py): the table, and for every texel of a w x h map the
// per-sample terms, as raw fp32 on stdout:
//   float table[N][3], then per y, x, sample: float tA, tB
// usage: brdf_lut_ggx_core_host w h sample_count visibility
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brdf_lut_ggx_core.h"

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const int w = atoi(argv[1]), h = atoi(argv[2]), n = atoi(argv[3]), vis = atoi(argv[4]);
    if (w < 1 || w > BLG_MAX_EXTENT || h < 1 || h > BLG_MAX_EXTENT || n < 1 || n > BLG_MAX_SAMPLES) return 2;
    if (vis != BLG_SMITH_SCHLICK && vis != BLG_SMITH_CORRELATED) return 2;
    std::vector<float> table(3 * (size_t)n);
    blg_fill_table((uint32_t)n, table.data());
    std::vector<float> out;
    out.reserve(2 * (size_t)w * h * n);
    std::vector<BlgHalf> half((size_t)n);
    for (int y = 0; y < h; ++y) {
        const float r = blg_coord(y, h), a = r * r, a2 = a * a;
        for (int i = 0; i < n; ++i) half[i] = blg_half(a2, table[3 * i], table[3 * i + 1]);
        for (int x = 0; x < w; ++x) {
            const BlgView v = blg_view(vis, blg_coord(x, w), a, a2);
            for (int i = 0; i < n; ++i) {
                float gv, omfc, fc;
                blg_sample(vis, v, half[i], &gv, &omfc, &fc);
                out.push_back(gv * omfc);
                out.push_back(gv * fc);
            }
        }
    }
    if (fwrite(table.data(), 12, (size_t)n, stdout) != (size_t)n) return 1;
    if (fwrite(out.data(), 4, out.size(), stdout) != out.size()) return 1;
    return 0;
}
