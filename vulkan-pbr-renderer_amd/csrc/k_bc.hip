// k_bc.hip -- K15: one level of BC1 / BC3 / BC5 blocks -> tight RGBA8UN rows, by the contract of bc_core.h.
//
// The reference hands its .dds material textures to Vulkan compressed (asset_import.cpp:30-60) and the sampler decodes per tap;
// here a level is decoded once when it is written, so the texel fetches of K13 / K14 stay plain RGBA8UN loads.
//
// Streaming kernel: 0.5 B (BC1) or 1 B (BC3 / BC5) read and 4 B written per texel.  Shaped for the stores: one lane owns the
// 4-texel row of one block (16 B), lanes run along x, so a wave writes 1 KiB of one output row with one instruction and reads 512 B
// or 1 KiB of consecutive blocks.  The four waves of a workgroup are the four rows of the same 64 blocks: the block bytes come from
// HBM once and from the cache three times.  Rows are 4 w bytes: when w is no multiple of 4 (or the level does not start on a 16-byte
// boundary, which happens below an odd-width level of a chain) rows are not 16-byte aligned and the last block of a row is partial --
// those levels take the narrow path, one 4-byte store per texel inside the level.
#include "bc_core.h"
#include "pbr_kernels.h"

template <int FMT, bool WIDE>
__global__ __launch_bounds__(256) void k_bc_decode(const uint32_t* __restrict__ blocks, int w, int h, int bw, uint32_t* __restrict__ out) {
    const int bx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int row = threadIdx.x >> 6;
    const int by = blockIdx.y;
    const int y = by * 4 + row;
    if (bx >= bw || y >= h) return;                                           // texels outside the level are dropped
    constexpr int WORDS = (FMT == BC_FMT_BC1_RGB || FMT == BC_FMT_BC1_RGBA) ? 2 : 4;
    const size_t b = (size_t)by * bw + bx;
    uint32_t words[WORDS];
    if (WORDS == 2) { const uint2 v = ((const uint2*)blocks)[b]; words[0] = v.x; words[1] = v.y; }
    else { const uint4 v = ((const uint4*)blocks)[b]; words[0] = v.x; words[1] = v.y; words[2] = v.z; words[3] = v.w; }
    uint32_t px[4];
    bc_decode_row(FMT, words, row, px);
    uint32_t* dst = out + (size_t)y * w + 4 * (size_t)bx;
    if (WIDE) { *(uint4*)dst = make_uint4(px[0], px[1], px[2], px[3]); return; }
    const int n = w - 4 * bx;                                                 // >= 1: bx < bw = ceil(w / 4)
    for (int x = 0; x < 4; ++x) if (x < n) dst[x] = px[x];
}

template <int FMT>
static void launch_bc(const void* blocks, int w, int h, void* out, hipStream_t st) {
    const int bw = (w + 3) / 4, bh = (h + 3) / 4;
    const dim3 grid((unsigned)((bw + 63) / 64), (unsigned)bh), block(256);
    const bool wide = (w % 4) == 0 && ((uintptr_t)out % 16) == 0;
    if (wide) hipLaunchKernelGGL((k_bc_decode<FMT, true>), grid, block, 0, st, (const uint32_t*)blocks, w, h, bw, (uint32_t*)out);
    else hipLaunchKernelGGL((k_bc_decode<FMT, false>), grid, block, 0, st, (const uint32_t*)blocks, w, h, bw, (uint32_t*)out);
}

extern "C" int pbrk_bc_decode(int format, const void* blocks, int width, int height, void* rgba8, void* stream) {
    // at most 16384 a side: the grid's y extent (block rows) stays below 65536 and every index fits its type
    if (!blocks || !rgba8 || width < 1 || height < 1 || width > 16384 || height > 16384) return PBRK_E_ARG;
    if (((uintptr_t)blocks % 8) != 0 || (format >= PBRK_BC3 && ((uintptr_t)blocks % 16) != 0) || ((uintptr_t)rgba8 % 4) != 0) return PBRK_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    switch (format) {
    case PBRK_BC1_RGB: launch_bc<BC_FMT_BC1_RGB>(blocks, width, height, rgba8, st); break;
    case PBRK_BC1_RGBA: launch_bc<BC_FMT_BC1_RGBA>(blocks, width, height, rgba8, st); break;
    case PBRK_BC3: launch_bc<BC_FMT_BC3>(blocks, width, height, rgba8, st); break;
    case PBRK_BC5: launch_bc<BC_FMT_BC5>(blocks, width, height, rgba8, st); break;
    default: return PBRK_E_ARG;
    }
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
