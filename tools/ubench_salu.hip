// Where the scalar unit starts to set the pace: ns per VALU wave-instruction per SIMD for independent v_fma_f32 mixed with plain
// scalar ALU instructions at SALU:VALU ratios 0 .. 2, 8 waves per SIMD on every CU, timed by wall clock (HIP events).  A gfx950 CU
// has four SIMDs and one scalar unit: once the CU's SALU stream needs more issue cycles than the SIMDs' VALU streams, the time per
// VALU instruction grows with the ratio.  Development tool.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_salu.hip -o tools/ubench_salu
#include <hip/hip_runtime.h>
#include <stdio.h>

#define ITERS 8192
#define V(x) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x) : "v"(a), "v"(b))
// one scalar ALU instruction of the mix (index j cycles over the kinds the region kernel's loop runs); independent chains
#define S(j)                                                                                                      \
    do {                                                                                                          \
        switch ((j) & 7) {                                                                                        \
        case 0: asm volatile("s_add_u32 %0, %0, %1" : "+s"(s0) : "s"(k) : "scc"); break;                          \
        case 1: asm volatile("s_and_b64 %0, %0, %1" : "+s"(m0) : "s"(m1) : "scc"); break;                         \
        case 2: asm volatile("s_ff1_i32_b32 %0, %1" : "=s"(s1) : "s"(s2)); break;                                 \
        case 3: asm volatile("s_lshl_b32 %0, %0, 1" : "+s"(s2) : : "scc"); break;                                 \
        case 4: asm volatile("s_xor_b32 %0, %0, %1" : "+s"(s3) : "s"(k) : "scc"); break;                          \
        case 5: asm volatile("s_bcnt1_i32_b64 %0, %1" : "=s"(s4) : "s"(m1) : "scc"); break;                       \
        case 6: asm volatile("s_andn2_b64 %0, %0, %1" : "+s"(m1) : "s"(m0) : "scc"); break;                       \
        default: asm volatile("s_sub_u32 %0, %0, %1" : "+s"(s5) : "s"(k) : "scc"); break;                         \
        }                                                                                                         \
    } while (0)

// NS scalar instructions per 8 FMAs, spread evenly between them (plus the loop's own counter, compare and branch once per 8 iterations)
template <int NS>
__global__ __launch_bounds__(256) void k(float* out, unsigned* sout, float a, float b, unsigned salt) {
    float x0 = a + threadIdx.x * 1e-6f, x1 = x0 + 1.f, x2 = x0 + 2.f, x3 = x0 + 3.f, x4 = x0 + 4.f, x5 = x0 + 5.f, x6 = x0 + 6.f, x7 = x0 + 7.f;
    unsigned k = salt, s0 = salt, s1 = 0, s2 = salt | 1u, s3 = salt + 3, s4 = 0, s5 = salt + 5;
    unsigned long long m0 = ~0ull ^ salt, m1 = 0x5555aaaa5555aaaaull ^ salt;
#pragma unroll 8
    for (int i = 0; i < ITERS; ++i) {
        // slot t (0..15) of the iteration: even slots hold the FMAs, odd slots a scalar instruction while NS allows
#define SLOT(t, x) V(x); if ((t) < NS) S(t); if ((t) + 8 < NS) S((t) + 8);
        SLOT(0, x0) SLOT(1, x1) SLOT(2, x2) SLOT(3, x3) SLOT(4, x4) SLOT(5, x5) SLOT(6, x6) SLOT(7, x7)
#undef SLOT
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
    if ((threadIdx.x & 63) == 0) sout[blockIdx.x * 4 + (threadIdx.x >> 6)] = s0 + s1 + s2 + s3 + s4 + s5 + (unsigned)(m0 ^ m1);
}

template <int NS> void run(int cus) {
    const int wps = 8, blocks = cus * wps;                 // 256 threads = 4 waves = one per SIMD; wps blocks per CU
    float* d; unsigned* so;
    (void)hipMalloc(&d, (size_t)blocks * 256 * 4); (void)hipMalloc(&so, (size_t)blocks * 4 * 4);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(k<NS>, dim3(blocks), dim3(256), 0, 0, d, so, 0.999f, 0.001f, 3u);
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(k<NS>, dim3(blocks), dim3(256), 0, 0, d, so, 0.999f, 0.001f, 3u);
        (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    const double valu_per_simd = (double)ITERS * 8 * wps;             // wps waves share a SIMD
    const double ns = best * 1e6 / valu_per_simd;
    const double salu_per_cu = (double)ITERS * NS * wps * 4;          // four SIMDs' waves share the CU's scalar unit
    printf("SALU:VALU %.3f  (%2d per 8 FMAs)  %8.3f ms  %.3f ns per VALU instruction per SIMD  %.3f ns per SALU instruction per CU  %.2f G SALU/s per CU\n",
           NS / 8.0, NS, best, ns, NS ? best * 1e6 / salu_per_cu : 0.0, NS ? salu_per_cu / (best * 1e6) : 0.0);
    (void)hipFree(d); (void)hipFree(so);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
}
int main() {
    hipDeviceProp_t pr;
    (void)hipGetDeviceProperties(&pr, 0);
    const int cus = pr.multiProcessorCount;
    printf("%s, %d CUs, 8 waves per SIMD, %d iterations of 8 independent v_fma_f32 + NS scalar ALU instructions\n", pr.gcnArchName, cus, ITERS);
    run<0>(cus); run<2>(cus); run<4>(cus); run<6>(cus); run<8>(cus); run<10>(cus); run<12>(cus); run<16>(cus);
    return 0;
}
