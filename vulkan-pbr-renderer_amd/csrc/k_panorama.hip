// k_panorama.hip -- K20 (an extension: the reference writes no image at all): one level of an RGBA32F cubemap ->
// a lat-long panorama, RGBA32F or RGBA16F.  The inverse of K6 (k_equirect.hip); the contract is in panorama_core.h.
//
// Each pixel takes its column's {cos phi, sin phi} and its row's {sin theta, cos theta} from the host-built table (the row pair is
// uniform over a wave), forms d with pano_dir, and is cube_fetch_rgba<true> of the bordered twin of the level: the project's one
// seamless sampler, exact coordinates, four taps, lerp_fma along x and then y, all four channels.  Streaming kernel: 16 or 8 bytes
// written per pixel, the level read through the caches.  K6's shape: 64 lanes along x, 4 rows per workgroup.
#include <hip/hip_fp16.h>

#include "pbr_device.h"
#include "pbr_kernels.h"
#include "panorama_core.h"

template <bool HALF>
__global__ __launch_bounds__(256) void k_cube_to_panorama(const float4* __restrict__ lvl, int n, const double* __restrict__ table,
                                                          void* __restrict__ out, int w, int h) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    float d[3];
    pano_dir(table + 2 * x, table + 2 * (w + y), d);
    const float4 r = cube_fetch_rgba<true>(lvl, n, mk3(d[0], d[1], d[2]));
    const size_t pi = (size_t)y * w + x;
    if (HALF) {
        __half2 lo = __halves2half2(__float2half_rn(r.x), __float2half_rn(r.y));
        __half2 hi = __halves2half2(__float2half_rn(r.z), __float2half_rn(r.w));
        uint2 packed;
        packed.x = *reinterpret_cast<unsigned*>(&lo);
        packed.y = *reinterpret_cast<unsigned*>(&hi);
        ((uint2*)out)[pi] = packed;
    } else {
        ((float4*)out)[pi] = r;
    }
}

extern "C" int pbrk_cube_to_panorama(const void* bordered_level, int n, const void* table, void* out, int out_format, int w, int h, void* stream) {
    if (!bordered_level || !table || !out || n < 1 || n > PANO_MAX_EXTENT || w < 1 || h < 1 || w > PANO_MAX_EXTENT || h > PANO_MAX_EXTENT) return PBRK_E_ARG;
    if (out_format != PBRK_FMT_RGBA32F && out_format != PBRK_FMT_RGBA16F) return PBRK_E_FORMAT;
    const dim3 grid((w + 63) / 64, (h + 3) / 4), block(256);
    if (out_format == PBRK_FMT_RGBA16F)
        hipLaunchKernelGGL(k_cube_to_panorama<true>, grid, block, 0, (hipStream_t)stream, (const float4*)bordered_level, n, (const double*)table, out, w, h);
    else
        hipLaunchKernelGGL(k_cube_to_panorama<false>, grid, block, 0, (hipStream_t)stream, (const float4*)bordered_level, n, (const double*)table, out, w, h);
    return hipGetLastError() == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
