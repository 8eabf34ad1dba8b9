// k_bc6h_decode.hip -- K19: one level of BC6H_UF16 blocks, all 14 modes -> tight RGBA32F / RGBA16F layers, by the contract
// of bc6h_decode_core.h.  The input side of K18: a .dds cube an engine cooker (or this project's own bake) wrote becomes the float
// texture the lighting pass already takes (host/pbr_ddsin.c), decoded once when it is loaded.
//
// Streaming kernel: 1 B read and 16 B (8 B) written per texel.  Two work splits, both measured:
//   row per lane (k_bc6h_decode), K15's shape: one lane owns the 4-texel row of one block (64 B resp. 32 B), lanes run along x, the four
//     waves of a workgroup are the four rows of the same 64 blocks.  Four times the waves of the other split, so it wins where a level
//     has too few blocks to put a wave on every SIMD; every lane decodes its block's header again.  It also holds the narrow path: when
//     w is no multiple of 4 the last block of a row is partial, and an RGBA16F level of a chain may start on an 8-byte boundary only --
//     those levels get one store per texel inside the level.
//   block per lane (k_bc6h_decode_block): the header is decoded once and its four rows are written by the same lane.  From
//     BLOCK_PER_LANE_MIN blocks on -- one wave for each of the 1024 SIMDs -- it is the faster one: by a few per cent on a level of one
//     mode, by up to 2.3 times on mixed modes, where the header work (every mode present in a wave is paid for) binds.
// Layers ride in grid.z.  This project's own files are mode 3 throughout (wave-uniform); foreign files mix modes inside a wave.
// Nothing is indexed by a run-time value: no scratch.  Plain stores: non-temporal ones are 4 times slower at the 64-byte lane stride.
#include "bc6h_decode_core.h"
#include "pbr_kernels.h"

template <bool F32, bool WIDE>
__global__ __launch_bounds__(256) void k_bc6h_decode(const uint4* __restrict__ blocks, int w, int h, int bw, int bh, void* __restrict__ out) {
    const int bx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int row = threadIdx.x >> 6;
    const int by = blockIdx.y;
    const int y = by * 4 + row;
    if (bx >= bw || y >= h) return;                                           // texels outside the level are dropped
    const size_t layer = blockIdx.z;
    const uint4 v = blocks[(layer * bh + by) * bw + bx];
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    uint32_t rgb[4][3];
    bc6hd_decode_row(words, (uint32_t)row, rgb);
    const size_t texel = (layer * h + y) * w + 4 * (size_t)bx;
    const int n = WIDE ? 4 : min(4, w - 4 * bx);                              // >= 1: bx < bw = ceil(w / 4)
    if (F32) {
        uint4* dst = (uint4*)out + texel;
#pragma unroll
        for (int x = 0; x < 4; ++x)
            if (x < n) dst[x] = make_uint4(bc6hd_f32_from_code(rgb[x][0]), bc6hd_f32_from_code(rgb[x][1]), bc6hd_f32_from_code(rgb[x][2]), 0x3F800000u);
    } else {
        uint2 px[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) px[x] = make_uint2(rgb[x][0] | (rgb[x][1] << 16), rgb[x][2] | (0x3C00u << 16));
        uint2* dst = (uint2*)out + texel;
        if (WIDE) {
            ((uint4*)dst)[0] = make_uint4(px[0].x, px[0].y, px[1].x, px[1].y);
            ((uint4*)dst)[1] = make_uint4(px[2].x, px[2].y, px[3].x, px[3].y);
        } else {
#pragma unroll
            for (int x = 0; x < 4; ++x) if (x < n) dst[x] = px[x];
        }
    }
}

template <bool F32>
__global__ __launch_bounds__(64) void k_bc6h_decode_block(const uint4* __restrict__ blocks, int w, int h, int bw, int bh, void* __restrict__ out) {
    const int bx = blockIdx.x * 64 + threadIdx.x;
    const int by = blockIdx.y;
    if (bx >= bw) return;
    const size_t layer = blockIdx.z;
    const uint4 v = blocks[(layer * bh + by) * bw + bx];
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    Bc6hdBlock b;
    bc6hd_header(words, &b);
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const int y = 4 * by + row;
        if (y >= h) break;                                                    // rows of the last block row outside the level are dropped
        uint32_t rgb[4][3];
#pragma unroll
        for (int x = 0; x < 4; ++x) bc6hd_texel(&b, words, (uint32_t)(4 * row + x), rgb[x]);
        const size_t texel = (layer * h + y) * w + 4 * (size_t)bx;           // w is a multiple of 4 here: the whole row is inside
        if (F32) {
            uint4* dst = (uint4*)out + texel;
#pragma unroll
            for (int x = 0; x < 4; ++x) dst[x] = make_uint4(bc6hd_f32_from_code(rgb[x][0]), bc6hd_f32_from_code(rgb[x][1]), bc6hd_f32_from_code(rgb[x][2]), 0x3F800000u);
        } else {
            uint4* dst = (uint4*)((uint2*)out + texel);
            dst[0] = make_uint4(rgb[0][0] | (rgb[0][1] << 16), rgb[0][2] | (0x3C00u << 16), rgb[1][0] | (rgb[1][1] << 16), rgb[1][2] | (0x3C00u << 16));
            dst[1] = make_uint4(rgb[2][0] | (rgb[2][1] << 16), rgb[2][2] | (0x3C00u << 16), rgb[3][0] | (rgb[3][1] << 16), rgb[3][2] | (0x3C00u << 16));
        }
    }
}

// one wave of k_bc6h_decode_block for each of the 256 x 4 SIMDs
static const uint64_t BLOCK_PER_LANE_MIN = 256u * 4u * 64u;

extern "C" int pbrk_bc6h_decode(const void* blocks, int width, int height, int layers, void* level_out, int dst_format, void* stream) {
    // at most 16384 a side: 4096 block rows in grid.y, layers in grid.z (at most 65535), every index fits its type
    if (!blocks || !level_out || width < 1 || height < 1 || width > 16384 || height > 16384 || layers < 1 || layers > 65535) return PBRK_E_ARG;
    if (dst_format != PBRK_FMT_RGBA32F && dst_format != PBRK_FMT_RGBA16F) return PBRK_E_FORMAT;
    const bool f32 = dst_format == PBRK_FMT_RGBA32F;
    if (((uintptr_t)blocks % 16) != 0 || ((uintptr_t)level_out % (f32 ? 16 : 8)) != 0) return PBRK_E_ARG;
    const int bw = (width + 3) / 4, bh = (height + 3) / 4;
    const dim3 grid((unsigned)((bw + 63) / 64), (unsigned)bh, (unsigned)layers), block(256);
    const bool wide = (width % 4) == 0 && ((uintptr_t)level_out % 16) == 0;
    hipStream_t st = (hipStream_t)stream;
    const uint4* src = (const uint4*)blocks;
    if (wide && (uint64_t)bw * (uint64_t)bh * (uint64_t)layers >= BLOCK_PER_LANE_MIN) {
        const dim3 bgrid((unsigned)((bw + 63) / 64), (unsigned)bh, (unsigned)layers), bblock(64);
        if (f32) hipLaunchKernelGGL((k_bc6h_decode_block<true>), bgrid, bblock, 0, st, src, width, height, bw, bh, level_out);
        else hipLaunchKernelGGL((k_bc6h_decode_block<false>), bgrid, bblock, 0, st, src, width, height, bw, bh, level_out);
        return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
    }
    if (f32 && wide) hipLaunchKernelGGL((k_bc6h_decode<true, true>), grid, block, 0, st, src, width, height, bw, bh, level_out);
    else if (f32) hipLaunchKernelGGL((k_bc6h_decode<true, false>), grid, block, 0, st, src, width, height, bw, bh, level_out);
    else if (wide) hipLaunchKernelGGL((k_bc6h_decode<false, true>), grid, block, 0, st, src, width, height, bw, bh, level_out);
    else hipLaunchKernelGGL((k_bc6h_decode<false, false>), grid, block, 0, st, src, width, height, bw, bh, level_out);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
