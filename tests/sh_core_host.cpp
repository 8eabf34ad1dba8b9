// Host build of csrc/sh_core.h (the arithmetic the K17 kernels are made of) for tests/test_sh_cpu.py:
//   sh_core_host project n face0 face1 y0 y1 level.bin out.bin     float RGBA [6][n][n] -> double[27]
//   sh_core_host irradiance size coef.bin out.bin                  double[27] -> float RGBA [6][size][size]
//   sh_core_host omega n out.bin                                   double [n][n], the texel solid angles of one face
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sh_core.h"

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(T), v.size(), f);
    const bool ok = got == v.size() && fgetc(f) == EOF;
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
    if (argc == 9 && !strcmp(argv[1], "project")) {
        const int n = atoi(argv[2]), f0 = atoi(argv[3]), f1 = atoi(argv[4]), y0 = atoi(argv[5]), y1 = atoi(argv[6]);
        if (n < 1 || n > 4096 || f0 < 0 || f0 >= f1 || f1 > 6 || y0 < 0 || y0 >= y1 || y1 > n) return 2;
        std::vector<float> level((size_t)6 * n * n * 4);
        if (!read_all(argv[7], level)) return 3;
        std::vector<double> out(27);
        sh_project_level(level.data(), n, f0, f1, y0, y1, out.data());
        return write_all(argv[8], out) ? 0 : 4;
    }
    if (argc == 5 && !strcmp(argv[1], "irradiance")) {
        const int size = atoi(argv[2]);
        if (size < 1 || size > 4096) return 2;
        std::vector<double> coef(27);
        if (!read_all(argv[3], coef)) return 3;
        std::vector<float> out((size_t)6 * size * size * 4);
        for (int f = 0; f < 6; ++f)
            for (int y = 0; y < size; ++y)
                for (int x = 0; x < size; ++x) sh_irradiance_texel(coef.data(), size, f, x, y, out.data() + 4 * (((size_t)f * size + y) * size + x));
        return write_all(argv[4], out) ? 0 : 4;
    }
    if (argc == 4 && !strcmp(argv[1], "omega")) {
        const int n = atoi(argv[2]);
        if (n < 1 || n > 4096) return 2;
        std::vector<double> out((size_t)n * n);
        for (int y = 0; y < n; ++y)
            for (int x = 0; x < n; ++x) out[(size_t)y * n + x] = sh_solid_angle(n, x, y);
        return write_all(argv[3], out) ? 0 : 4;
    }
    fprintf(stderr, "usage: %s project n f0 f1 y0 y1 level.bin out.bin | irradiance size coef.bin out.bin | omega n out.bin\n", argv[0]);
    return 2;
}
