// Brute-force voxeliser (no owner grid, no lists) over csrc/voxelize_core.h compiled for the host: every pixel against every triangle,
// fragments applied in (triangle, row, column) order, the last store to a voxel stays.  tests/test_voxelize_core_host.py builds it,
// feeds it the scenes of the GPU tests and compares it with the numpy reference, so the header the kernels are made of is pinned on
// the CPU too.  A program of its own (scene file in, grid file out), so that it can also be built with -fsanitize=address,undefined.
//
// scene file: int32 N, draws, sun_w, sun_h; float sun map; uint16 grid [N^3][4]; per draw int32 {floats, indices, first_vertex,
// vertex_count, instance_count, base w, h, levels, emissive w, h, levels, base bytes, emissive bytes}, float {sun[16], sun_dir[4],
// scale}, the vertex floats, the indices, the two texture chains.  grid file: int64 rejected, uint16 grid.
#include "voxelize_core.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

static uint16_t half_rn(float f) {                                             // fp32 -> fp16, round to nearest even
    uint32_t x = geo_bits(f);
    const uint16_t s = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7FFFFFFFu;
    if (x >= 0x7F800000u) return (uint16_t)(s | (x > 0x7F800000u ? 0x7E00u : 0x7C00u));
    const uint32_t E = x >> 23, m = (x & 0x7FFFFFu) | 0x800000u;
    if (E < 102) return s;                                                    // below half of the smallest subnormal
    if (E < 113) {                                                            // subnormal: units of 2^-24
        const uint32_t sh = 126 - E;
        uint32_t k = m >> sh;
        const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
        if (rem > half || (rem == half && (k & 1u))) ++k;
        return (uint16_t)(s | k);
    }
    uint32_t h = ((E - 112) << 10) | ((x & 0x7FFFFFu) >> 13);
    const uint32_t rem = x & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;                    // a carry into the exponent is the right result
    if (h >= 0x7C00u) h = 0x7C00u;
    return (uint16_t)(s | h);
}

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

struct HostDraw { std::vector<float> v; std::vector<uint32_t> ix; std::vector<uint8_t> base, emi; int vertex_count, instance_count; PbrkVoxDraw d; };

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s scene grid_out\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[4];
    if (fread(head, 4, 4, f) != 4) return 2;
    const int N = head[0], nd = head[1], sw = head[2], sh = head[3];
    if (N < 8 || N > 256 || nd < 0 || sw < 1 || sh < 1) return 2;
    std::vector<float> sun;
    std::vector<uint16_t> grid;
    if (!rd(f, sun, (size_t)sw * sh) || !rd(f, grid, (size_t)N * N * N * 4)) return 2;
    std::vector<HostDraw> draws((size_t)nd);
    for (HostDraw& h : draws) {
        int32_t q[13];
        float g[21];
        if (fread(q, 4, 13, f) != 13 || fread(g, 4, 21, f) != 21) return 2;
        if (!rd(f, h.v, (size_t)q[0]) || !rd(f, h.ix, (size_t)q[1]) || !rd(f, h.base, (size_t)q[11]) || !rd(f, h.emi, (size_t)q[12])) return 2;
        if ((long long)q[2] + q[3] > q[1]) return 2;                          // what GPU_OpDraw checks at record time
        memset(&h.d, 0, sizeof h.d);
        memcpy(h.d.sun, g, 64); memcpy(h.d.sun_dir, g + 16, 16); h.d.scale = g[20];
        h.d.first_vertex = (uint32_t)q[2]; h.vertex_count = q[3]; h.instance_count = q[4];
        h.d.vertices = h.v.data(); h.d.vertex_floats = h.v.size(); h.d.indices = h.ix.data();
        h.d.sun_depth = sun.data(); h.d.sun_w = sw; h.d.sun_h = sh;
        h.d.tex[0] = PbrkGeoTex{h.base.data(), q[5], q[6], q[7], 0};
        h.d.tex[1] = PbrkGeoTex{h.emi.data(), q[8], q[9], q[10], 0};
    }
    fclose(f);
    long long rejected = 0;
    for (const HostDraw& h : draws) {
        if (h.instance_count == 0) continue;
        for (int k = 0; k < h.vertex_count / 3; ++k) {
            VoxTri T;
            const int st = vox_setup(h.d, (uint32_t)k, N, T);
            if (st < 0) ++rejected;
            if (st <= 0) continue;
            for (int j = 0; j < N; ++j) for (int i = 0; i < N; ++i) {
                int c[3];
                if (!vox_covers(T, i, j) || !vox_coord(T, i, j, N, c)) continue;
                float rgb[3];
                vox_shade(h.d, T, i, j, rgb);
                uint16_t* o = &grid[(((size_t)c[2] * N + c[1]) * N + c[0]) * 4];
                o[0] = half_rn(rgb[0]); o[1] = half_rn(rgb[1]); o[2] = half_rn(rgb[2]); o[3] = 0x3C00u;
            }
        }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const bool ok = fwrite(&rejected, 8, 1, o) == 1 && fwrite(grid.data(), 2, grid.size(), o) == grid.size();
    return fclose(o) == 0 && ok ? 0 : 2;
}
