// k_bc6h.hip -- K18: one level of RGBA32F / RGBA16F layers -> BC6H_UF16 blocks, at one of two quality levels: the
// one-region block (mode 11) by the contract of bc6h_core.h, or per block that block or one of the two-region cases 0, 14, 1, 30 by
// the contract of bc6h2_core.h.  One kernel template: the gather, the argument checks and the launch are the same for both.
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
//
// Two regions, the opt-in second level for blocks with a hard edge (a sun disc, a horizon, a window): the loop over the 32 partitions
// is rolled and wave-uniform: the subset mask is a scalar, every per-texel subset choice a select on a scalar bit, and the 16 texels
// stay in registers as 48 words of half code | scaled value << 16.  Per block 32 partitions x 8 entries x 16 texels of palette search
// on top of the one-region 3 x 16 x 16, about 5.3 times its palette work plus the per-subset statistics and the endpoint
// quantisation -- measured 11 times its time (profiles/bc6h_encode2.json; 251 VGPRs, no scratch: profiles/bc6h_encode2.md); the mode
// loop and the skip of blocks the one-region search already reproduces exactly are the only places where lanes of a wave part.
#include "bc6h2_core.h"
#include "pbr_kernels.h"

template <bool F32, bool TWO_REGIONS>
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
    if (TWO_REGIONS) {
        Bc6h2Info info;
        bc6h2_encode_block(codes, words, &info);
    } else {
        bc6h_encode_block(codes, words);
    }
    out[layer * nblocks + b] = make_uint4(words[0], words[1], words[2], words[3]);
}

extern "C" uint64_t pbrk_bc6h_level_bytes(int width, int height, int layers) {
    if (width < 1 || height < 1 || layers < 1) return 0;
    return (uint64_t)((width + 3) / 4) * (uint64_t)((height + 3) / 4) * 16u * (uint64_t)layers;
}

template <bool TWO_REGIONS>
static int bc6h_encode(const void* level, int src_format, int width, int height, int layers, void* blocks_out, void* stream) {
    // at most 16384 a side: 4096^2 blocks per layer, every index fits its type; layers ride in grid.y
    if (!level || !blocks_out || width < 1 || height < 1 || width > 16384 || height > 16384 || layers < 1 || layers > 65535) return PBRK_E_ARG;
    if (src_format != PBRK_FMT_RGBA32F && src_format != PBRK_FMT_RGBA16F) return PBRK_E_FORMAT;
    if (((uintptr_t)level % (src_format == PBRK_FMT_RGBA32F ? 16 : 8)) != 0 || ((uintptr_t)blocks_out % 16) != 0) return PBRK_E_ARG;
    const int bw = (width + 3) / 4, bh = (height + 3) / 4, nblocks = bw * bh;
    const dim3 grid((unsigned)((nblocks + 63) / 64), (unsigned)layers), block(64);
    hipStream_t st = (hipStream_t)stream;
    if (src_format == PBRK_FMT_RGBA32F) hipLaunchKernelGGL((k_bc6h_encode<true, TWO_REGIONS>), grid, block, 0, st, level, width, height, bw, nblocks, (uint4*)blocks_out);
    else hipLaunchKernelGGL((k_bc6h_encode<false, TWO_REGIONS>), grid, block, 0, st, level, width, height, bw, nblocks, (uint4*)blocks_out);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}

extern "C" int pbrk_bc6h_encode(const void* level, int src_format, int width, int height, int layers, void* blocks_out, void* stream) {
    return bc6h_encode<false>(level, src_format, width, height, layers, blocks_out, stream);
}
extern "C" int pbrk_bc6h_encode2(const void* level, int src_format, int width, int height, int layers, void* blocks_out, void* stream) {
    return bc6h_encode<true>(level, src_format, width, height, layers, blocks_out, stream);
}
