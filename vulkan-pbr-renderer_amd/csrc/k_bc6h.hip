// k_bc6h.hip -- K18: one level of RGBA32F / RGBA16F layers -> BC6H_UF16 blocks (mode 11), by the contract of bc6h_core.h.
//
// The output side of the bake: a prefiltered cube leaves the process as one .dds an engine loads (host/pbr_ddsout.c).  16 B (8 B) read
// and 1 B written per texel, but the time goes to the palette search: 3 candidates x 16 entries x 16 texels x 3 channels of integer
// multiply-add per block, about 10^4 VALU operations for 272 bytes of traffic.
//
// Work split: one lane owns one 4 x 4 block and runs the contract's search as written -- no cross-lane step, no LDS, the bytes are the
// contract's by construction.  Lanes run along the blocks of a layer in row-major order (layers in grid.y), so a wave reads four texel
// rows of up to 4 KiB each, every byte of which is used, and writes 1 KiB of consecutive blocks with one store.  The 16 texels stay in
// registers as 48 half codes; the loops over candidates and palette entries are kept rolled (the entry index is wave-uniform, its
// weight is scalar work), the loops over texels and channels are unrolled so that no array is indexed at run time.  Workgroups are
// single waves: nothing is shared, and a 256^2 level (4096 blocks a face) spreads over every CU.
#include "bc6h_core.h"
#include "pbr_kernels.h"

template <bool F32>
__global__ __launch_bounds__(64) void k_bc6h_encode(const void* __restrict__ level, int w, int h, int bw, int nblocks, uint4* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nblocks) return;
    const int by = b / bw, bx = b - by * bw;
    const size_t layer = blockIdx.y;
    uint32_t codes[16][3];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int x = min(4 * bx + (t & 3), w - 1), y = min(4 * by + (t >> 2), h - 1);   // the clamped edge rule
        const size_t i = (layer * h + y) * w + x;
        if (F32) {
            const uint4 v = ((const uint4*)level)[i];
            codes[t][0] = bc6h_code_from_f32(v.x); codes[t][1] = bc6h_code_from_f32(v.y); codes[t][2] = bc6h_code_from_f32(v.z);
        } else {
            const uint2 v = ((const uint2*)level)[i];
            codes[t][0] = bc6h_code_from_f16(v.x & 0xFFFFu); codes[t][1] = bc6h_code_from_f16(v.x >> 16); codes[t][2] = bc6h_code_from_f16(v.y & 0xFFFFu);
        }
    }
    uint32_t words[4];
    bc6h_encode_block(codes, words);
    out[layer * nblocks + b] = make_uint4(words[0], words[1], words[2], words[3]);
}

extern "C" uint64_t pbrk_bc6h_level_bytes(int width, int height, int layers) {
    if (width < 1 || height < 1 || layers < 1) return 0;
    return (uint64_t)((width + 3) / 4) * (uint64_t)((height + 3) / 4) * 16u * (uint64_t)layers;
}

extern "C" int pbrk_bc6h_encode(const void* level, int src_format, int width, int height, int layers, void* blocks_out, void* stream) {
    // at most 16384 a side: 4096^2 blocks per layer, every index fits its type; layers ride in grid.y
    if (!level || !blocks_out || width < 1 || height < 1 || width > 16384 || height > 16384 || layers < 1 || layers > 65535) return PBRK_E_ARG;
    if (src_format != PBRK_FMT_RGBA32F && src_format != PBRK_FMT_RGBA16F) return PBRK_E_FORMAT;
    if (((uintptr_t)level % (src_format == PBRK_FMT_RGBA32F ? 16 : 8)) != 0 || ((uintptr_t)blocks_out % 16) != 0) return PBRK_E_ARG;
    const int bw = (width + 3) / 4, bh = (height + 3) / 4, nblocks = bw * bh;
    const dim3 grid((unsigned)((nblocks + 63) / 64), (unsigned)layers), block(64);
    hipStream_t st = (hipStream_t)stream;
    if (src_format == PBRK_FMT_RGBA32F) hipLaunchKernelGGL((k_bc6h_encode<true>), grid, block, 0, st, level, width, height, bw, nblocks, (uint4*)blocks_out);
    else hipLaunchKernelGGL((k_bc6h_encode<false>), grid, block, 0, st, level, width, height, bw, nblocks, (uint4*)blocks_out);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
