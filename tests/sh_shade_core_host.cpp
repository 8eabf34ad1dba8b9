// Host build of csrc/sh_shade_core.h (the SH9 ambient arithmetic of K5) for tests/test_sh_shade_cpu.py:
//   sh_shade_core_host eval coef.bin normals.bin k.bin e32.bin e64.bin
//        double[27], float [n][3] (raw normals of any non-zero length) -> the folded float[27], sh_shade_eval as float [n][3], and
//        sh_irradiance of sh_core.h at the normal normalised in double as double [n][3]
//   sh_shade_core_host weights out.bin
//        double[18]: sh_shade_weight(0..8), then a_i K_i as sh_irradiance itself forms them (a unit coefficient at a point where p_i = 1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sh_shade_core.h"

template <class T>
static bool read_file(const char* path, std::vector<T>& v, size_t multiple_of) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || (size_t)bytes % (sizeof(T) * multiple_of)) { fclose(f); return false; }
    v.resize((size_t)bytes / sizeof(T));
    const bool ok = fread(v.data(), sizeof(T), v.size(), f) == v.size();
    fclose(f);
    return ok;
}
template <class T>
static bool write_all(const char* path, const std::vector<T>& v) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "eval")) {
        std::vector<double> coef;
        std::vector<float> normals;
        if (!read_file(argv[2], coef, 27) || coef.size() != 27 || !read_file(argv[3], normals, 3)) return 3;
        const size_t n = normals.size() / 3;
        std::vector<float> k(27), e32(3 * n);
        std::vector<double> e64(3 * n);
        sh_shade_fold(coef.data(), k.data());
        for (size_t i = 0; i < n; ++i) {
            const float* v = &normals[3 * i];
            if (v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f) return 2;
            sh_shade_eval(k.data(), v[0], v[1], v[2], &e32[3 * i]);
            const double x = v[0], y = v[1], z = v[2], inv = 1.0 / sqrt((x * x + y * y) + z * z);
            const double d[3] = {x * inv, y * inv, z * inv};
            sh_irradiance(coef.data(), d, &e64[3 * i]);
        }
        return write_all(argv[4], k) && write_all(argv[5], e32) && write_all(argv[6], e64) ? 0 : 4;
    }
    if (argc == 3 && !strcmp(argv[1], "weights")) {
        // a point where p_i = 1 (i = 6: the origin, where 3 z^2 - 1 = -1) and every other coefficient is zero
        static const double at[9][3] = {{0, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 0}, {1, 1, 0}, {0, 1, 1}, {0, 0, 0}, {1, 0, 1}, {1, 0, 0}};
        std::vector<double> out(18);
        for (int i = 0; i < 9; ++i) {
            double coef[27] = {0.0}, e[3];
            coef[3 * i] = 1.0;
            sh_irradiance(coef, at[i], e);
            out[i] = sh_shade_weight(i);
            out[9 + i] = i == 6 ? -e[0] : e[0];
        }
        return write_all(argv[2], out) ? 0 : 4;
    }
    fprintf(stderr, "usage: %s eval coef.bin normals.bin k.bin e32.bin e64.bin | weights out.bin\n", argv[0]);
    return 2;
}
