// csrc/gridview_core.h compiled for the host, with the oracle's 3-D sampler (orc_tex3d_sample of liborc.so) as its sampler: every pixel
// of a frame through gv_pixel.  tests/test_gridview_core_host.py builds it, feeds it the views of the K16 tests and compares it with the
// restatement of tests/gridview_ref.py, so the header the kernel is made of is pinned on the CPU too.  A program of its own (scene file
// in, frame file out), so that it can also be built with -fsanitize=address,undefined.
//
// scene file: int32 n, W, H; float globals[138]; uint16 grid [n^3][4].  frame file: float colour [H][W][4]; int32 step [H][W];
// float ro [H][W][3].
#include "gridview_core.h"

#include <stdint.h>
#include <stdio.h>
#include <vector>

extern "C" void orc_tex3d_sample(const uint16_t* grid, int n, const float p[3], float out[4]);

struct OracleSampler {
    const uint16_t* grid; int n;
    void operator()(const float* p, float* rgba) const { orc_tex3d_sample(grid, n, p, rgba); }
};

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s scene frame_out\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[3];
    float gl[138];
    if (fread(head, 4, 3, f) != 3 || fread(gl, 4, 138, f) != 138) return 2;
    const int n = head[0], W = head[1], H = head[2];
    if (n < 1 || n > 256 || W < 1 || H < 1 || W > 4096 || H > 4096) return 2;
    std::vector<uint16_t> grid((size_t)n * n * n * 4);
    if (fread(grid.data(), 2, grid.size(), f) != grid.size()) return 2;
    fclose(f);
    std::vector<float> colour((size_t)W * H * 4), ro((size_t)W * H * 3);
    std::vector<int32_t> step((size_t)W * H);
    const OracleSampler sampler = {grid.data(), n};
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x;
        const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
        step[i] = gv_pixel(gl + 32, gl + 132, gl[136], gl[135], fx / (float)W, fy / (float)H, fx, fy, sampler, &colour[i * 4], &ro[i * 3]);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const bool ok = fwrite(colour.data(), 4, colour.size(), o) == colour.size() && fwrite(step.data(), 4, step.size(), o) == step.size() &&
                    fwrite(ro.data(), 4, ro.size(), o) == ro.size();
    return fclose(o) == 0 && ok ? 0 : 2;
}
