// Work splits of the K19 decode (development tool): row per lane, texel per lane and block per lane around the header of the
// library's kernel (bc6h_decode_core.h on bc6h_format.h), each with plain and with non-temporal stores, on cube levels of one mode (3) and of a random mode per block, into
// RGBA32F and RGBA16F.  Prints the best of three windows per variant; at 256^2 every variant must write the bytes of the first.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/ubench_bc6h_decode.hip -o tools/ubench_bc6h_decode
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../vulkan-pbr-renderer_amd/csrc/bc6h_decode_core.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)
typedef unsigned u32x4n __attribute__((ext_vector_type(4)));

template <bool NT> __device__ __forceinline__ void st16(uint4* p, uint4 v) {
    if (NT) { u32x4n q = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(q, (u32x4n*)p); } else *p = v;
}
__device__ __forceinline__ uint4 px32(const uint32_t rgb[3]) { return make_uint4(bc6hd_f32_from_code(rgb[0]), bc6hd_f32_from_code(rgb[1]), bc6hd_f32_from_code(rgb[2]), 0x3F800000u); }

// V0 / V1: row per lane (the library's kernel), plain / non-temporal
template <bool F32, bool NT>
__global__ __launch_bounds__(256) void k_row(const uint4* __restrict__ blocks, int w, int h, int bw, int bh, void* __restrict__ out) {
    const int bx = blockIdx.x * 64 + (threadIdx.x & 63), row = threadIdx.x >> 6, by = blockIdx.y, y = by * 4 + row;
    if (bx >= bw || y >= h) return;
    const size_t layer = blockIdx.z;
    const uint4 v = blocks[(layer * bh + by) * bw + bx];
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    uint32_t rgb[4][3];
    bc6hd_decode_row(words, (uint32_t)row, rgb);
    const size_t texel = (layer * h + y) * w + 4 * (size_t)bx;
    if (F32) {
        uint4* dst = (uint4*)out + texel;
#pragma unroll
        for (int x = 0; x < 4; ++x) st16<NT>(dst + x, px32(rgb[x]));
    } else {
        uint2 px[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) px[x] = make_uint2(rgb[x][0] | (rgb[x][1] << 16), rgb[x][2] | (0x3C00u << 16));
        uint4* dst = (uint4*)((uint2*)out + texel);
        st16<NT>(dst, make_uint4(px[0].x, px[0].y, px[1].x, px[1].y));
        st16<NT>(dst + 1, make_uint4(px[2].x, px[2].y, px[3].x, px[3].y));
    }
}
// V2 / V3: texel per lane (RGBA32F) resp. texel pair per lane (RGBA16F): a wave's store is contiguous
template <bool F32, bool NT>
__global__ __launch_bounds__(256) void k_texel(const uint4* __restrict__ blocks, int w, int h, int bw, int bh, void* __restrict__ out) {
    constexpr int PER = F32 ? 4 : 2;                                          // lanes per block row
    const int lane = threadIdx.x & 63, bx = blockIdx.x * (64 / PER) + lane / PER, sub = lane % PER;
    const int row = threadIdx.x >> 6, by = blockIdx.y, y = by * 4 + row;
    if (bx >= bw || y >= h) return;
    const size_t layer = blockIdx.z;
    const uint4 v = blocks[(layer * bh + by) * bw + bx];
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    Bc6hdBlock b;
    bc6hd_header(words, &b);
    const size_t texel = (layer * h + y) * w + 4 * (size_t)bx;
    if (F32) {
        uint32_t rgb[3];
        bc6hd_texel(&b, words, 4u * row + sub, rgb);
        st16<NT>((uint4*)out + texel + sub, px32(rgb));
    } else {
        uint32_t a[3], c[3];
        bc6hd_texel(&b, words, 4u * row + 2 * sub, a);
        bc6hd_texel(&b, words, 4u * row + 2 * sub + 1, c);
        st16<NT>((uint4*)((uint2*)out + texel) + sub, make_uint4(a[0] | (a[1] << 16), a[2] | (0x3C00u << 16), c[0] | (c[1] << 16), c[2] | (0x3C00u << 16)));
    }
}
// V4: block per lane
template <bool F32, bool NT>
__global__ __launch_bounds__(64) void k_block(const uint4* __restrict__ blocks, int w, int h, int bw, int bh, void* __restrict__ out) {
    const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y;
    if (bx >= bw) return;
    const size_t layer = blockIdx.z;
    const uint4 v = blocks[(layer * bh + by) * bw + bx];
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    Bc6hdBlock b;
    bc6hd_header(words, &b);
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const size_t texel = (layer * h + 4 * by + row) * w + 4 * (size_t)bx;
        uint32_t rgb[4][3];
#pragma unroll
        for (int x = 0; x < 4; ++x) bc6hd_texel(&b, words, 4u * row + x, rgb[x]);
        if (F32) {
#pragma unroll
            for (int x = 0; x < 4; ++x) st16<NT>((uint4*)out + texel + x, px32(rgb[x]));
        } else {
            uint4* dst = (uint4*)((uint2*)out + texel);
            st16<NT>(dst, make_uint4(rgb[0][0] | (rgb[0][1] << 16), rgb[0][2] | (0x3C00u << 16), rgb[1][0] | (rgb[1][1] << 16), rgb[1][2] | (0x3C00u << 16)));
            st16<NT>(dst + 1, make_uint4(rgb[2][0] | (rgb[2][1] << 16), rgb[2][2] | (0x3C00u << 16), rgb[3][0] | (rgb[3][1] << 16), rgb[3][2] | (0x3C00u << 16)));
        }
    }
}

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static const int MODES[18] = {0, 1, 2, 3, 6, 7, 10, 11, 14, 15, 18, 19, 22, 23, 26, 27, 30, 31};

static void fill(std::vector<uint64_t>& b, bool mixed) {
    for (size_t i = 0; i < b.size(); i += 2) {
        b[i] = rnd(); b[i + 1] = rnd();
        const int m = mixed ? MODES[rnd() % 18] : 3;
        b[i] = m < 2 ? ((b[i] & ~3ull) | (uint64_t)m) : ((b[i] & ~31ull) | (uint64_t)m);
    }
}

template <bool F32>
static void launch(int variant, const uint4* blocks, int n, void* out) {
    const int bw = n / 4, bh = n / 4;
    switch (variant) {
    case 0: hipLaunchKernelGGL((k_row<F32, false>), dim3((bw + 63) / 64, bh, 6), dim3(256), 0, 0, blocks, n, n, bw, bh, out); break;
    case 1: hipLaunchKernelGGL((k_row<F32, true>), dim3((bw + 63) / 64, bh, 6), dim3(256), 0, 0, blocks, n, n, bw, bh, out); break;
    case 2: hipLaunchKernelGGL((k_texel<F32, false>), dim3((bw + (F32 ? 15 : 31)) / (F32 ? 16 : 32), bh, 6), dim3(256), 0, 0, blocks, n, n, bw, bh, out); break;
    case 3: hipLaunchKernelGGL((k_texel<F32, true>), dim3((bw + (F32 ? 15 : 31)) / (F32 ? 16 : 32), bh, 6), dim3(256), 0, 0, blocks, n, n, bw, bh, out); break;
    case 4: hipLaunchKernelGGL((k_block<F32, false>), dim3((bw + 63) / 64, bh, 6), dim3(64), 0, 0, blocks, n, n, bw, bh, out); break;
    case 5: hipLaunchKernelGGL((k_block<F32, true>), dim3((bw + 63) / 64, bh, 6), dim3(64), 0, 0, blocks, n, n, bw, bh, out); break;
    }
}

int main() {
    const char* names[6] = {"row/lane", "row/lane nt", "texel/lane", "texel/lane nt", "block/lane", "block/lane nt"};
    for (int n : {256, 512, 1024, 4096}) {
        const size_t nblocks = (size_t)6 * (n / 4) * (n / 4), texels = (size_t)6 * n * n;
        uint4* dblocks; void* dout;
        CK(hipMalloc(&dblocks, nblocks * 16)); CK(hipMalloc(&dout, texels * 16));
        for (int mixed = 0; mixed < 2; ++mixed) {
            std::vector<uint64_t> hb(nblocks * 2);
            fill(hb, mixed != 0);
            CK(hipMemcpy(dblocks, hb.data(), nblocks * 16, hipMemcpyHostToDevice));
            for (int f32 = 1; f32 >= 0; --f32) {
                std::vector<uint8_t> ref;
                for (int v = 0; v < 6; ++v) {
                    const int launches = n == 4096 ? 10 : n == 1024 ? 100 : 500;
                    double best = 1e30;
                    for (int win = 0; win < 4; ++win) {
                        CK(hipDeviceSynchronize());
                        auto t0 = std::chrono::steady_clock::now();
                        for (int i = 0; i < launches; ++i) { if (f32) launch<true>(v, dblocks, n, dout); else launch<false>(v, dblocks, n, dout); }
                        CK(hipGetLastError()); CK(hipDeviceSynchronize());
                        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / launches;
                        if (win > 0 && us < best) best = us;
                    }
                    int same = -1;
                    if (n == 256) {                                           // every variant writes the bytes of variant 0
                        std::vector<uint8_t> got(texels * (f32 ? 16 : 8));
                        CK(hipMemcpy(got.data(), dout, got.size(), hipMemcpyDeviceToHost));
                        if (v == 0) ref = got;
                        same = memcmp(got.data(), ref.data(), got.size()) == 0;
                        CK(hipMemset(dout, 0, texels * 16));
                    }
                    printf("n %4d %s %s %-14s %9.2f us  same %d\n", n, mixed ? "mixed" : "mode3", f32 ? "f32" : "f16", names[v], best, same);
                    fflush(stdout);
                }
            }
        }
        CK(hipFree(dblocks)); CK(hipFree(dout));
    }
    return 0;
}
