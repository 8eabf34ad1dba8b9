// k_mc_prep.hip -- what the region kernel (k_mc_region.hip) needs once per LAUNCH instead of once per tile: the maxima of the absorbed-word
// test (header 2f, k_mc_prep), the launch-level cut and the early end of a pass (2g and 2l, k_mc_cut), their host twins, and the ring of
// scratch slots they write to.
#include "pbr_device.h"
#include "pbr_kernels.h"
#include "k_mc_internal.h"

// ---- the launch's maxima (header, 2f) ----
// out[0 .. NW): per mask word, the largest bit pattern of its samples' weights; out[NW .. NW + NR): per region, the largest bit
// pattern of the R, G, B of exactly the texels the region kernel stages for it (rx <= rcx, ry <= rcy: apron included).  Compared as
// unsigned integers, as the lemma at absorb_threshold wants: a negative, -0, inf or NaN orders at or above +inf's pattern.
// Block b < NR reduces region b; the blocks behind take 256 words each, one per thread.
// Header 2g: out[NW + NR + 4 .. + NR): per region, the SMALLEST such bit pattern (k_mc_cut's m; a negative or -0 texel hides from it but
// not from the largest pattern, which then switches the cut off).
__global__ __launch_bounds__(256) void k_mc_prep(const float4* __restrict__ src, int n, int G, int RC, int NR,
                                                 const float4* __restrict__ tab, int n_tab, int NW, unsigned* __restrict__ out) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= NR) {
        const int w = ((int)blockIdx.x - NR) * 256 + tid;
        if (w >= NW) return;
        unsigned m = 0u;
        for (int i = w << 5; i < min((w << 5) + 32, n_tab); ++i) m = max(m, __float_as_uint(tab[i].w));
        out[w] = m;
        return;
    }
    __shared__ unsigned red, redlo;
    if (tid == 0) { red = 0u; redlo = 0xffffffffu; }
    __syncthreads();
    const int r = (int)blockIdx.x, nb = n + 2;
    const int f = r / (G * G), gy = (r / G) % G, gx = r % G;
    const int ox = gx * RC, oy = gy * RC;
    const int cols = min(RC, n + 1 - ox) + 1, rows = min(RC, n + 1 - oy) + 1;
    const float4* __restrict__ fsrc = src + ((size_t)f * nb + oy) * nb + ox;
    unsigned m = 0u, lo = 0xffffffffu;
    for (int k = tid; k < rows * cols; k += 256) {
        const int ry = k / cols, rx = k - ry * cols;
        const float4 v = fsrc[ry * nb + rx];
        m = max(m, max(__float_as_uint(v.x), max(__float_as_uint(v.y), __float_as_uint(v.z))));
        lo = min(lo, min(__float_as_uint(v.x), min(__float_as_uint(v.y), __float_as_uint(v.z))));
    }
    atomicMax(&red, m);
    atomicMin(&redlo, lo);
    __syncthreads();
    if (tid == 0) { out[NW + r] = red; out[NW + NR + 4 + r] = redlo; }
}

// ---- the launch's cut (header, 2g) ----
// One wave behind k_mc_prep on the same stream: lanes 0 .. S - 1 add up the weights of their slice's head word in double, in index order;
// lane 0 folds the regions' extrema and writes the first cut word of each slice to out[NW + NR .. + 4) (mc_launch_cut_s, k_mc_internal.h).
// S (1, 2 or 4) is the slice count of the region kernel behind it; all four slots are written, slot j with the cut of slice j % S.
// Header 2l: out[NW + 2 NR + 4 .. + 4), behind the regions' minima: per slice the first word from which the word maxima never rise again
// (mc_mono_from), slots as for the cut.
__global__ __launch_bounds__(64) void k_mc_cut(const float4* __restrict__ tab, int n_tab, int NW, int NR, int S, unsigned* __restrict__ out) {
    __shared__ double H[4];
    const int tid = threadIdx.x;
    if (tid < 4) {
        double h = 0.0;
        if (tid < S && NW > S)
            for (int i = 0; i < 32; ++i) h += (double)tab[(tid << 5) + i].w;
        H[tid] = h;
    }
    __syncthreads();
    if (tid != 0) return;
    unsigned M = 0u, m = 0xffffffffu;
    for (int r = 0; r < NR; ++r) { M = max(M, out[NW + r]); m = min(m, out[NW + NR + 4 + r]); }
    int cut4[4];
    mc_launch_cut_s(out, NW, S, H, m, M, cut4);
    for (int s = 0; s < 4; ++s) out[NW + NR + s] = (unsigned)cut4[s % S];
    // header 2l: per slice, the first word from which the word maxima never rise again, behind the regions' minima
    int mono4[4];
    mc_mono_from(out, NW, S, mono4);
    for (int s = 0; s < 4; ++s) out[NW + 2 * NR + 4 + s] = (unsigned)mono4[s % S];
}

// The same cut on the host, from the table's weights and the level's extrema (bit patterns): what k_mc_cut writes for them.  Needs no GPU.
// cut4[s]: the first cut word of slice s (see mc_launch_cut).  Returns the number of words cut, or -1 for bad arguments.
extern "C" int pbrk_mc_launch_cut(const float* weights, int n, unsigned min_bits, unsigned max_bits, int* cut4) {
    return pbrk_mc_launch_cut_slices(weights, n, 4, min_bits, max_bits, cut4);
}
// The same for a launch of S slices per workgroup (S = 1, 2 or 4; mc_launch_cut_s): cut[s], s < S.
extern "C" int pbrk_mc_launch_cut_slices(const float* weights, int n, int S, unsigned min_bits, unsigned max_bits, int* cut4) {
    if (!weights || !cut4 || n < 1 || n > 8192 || (S != 1 && S != 2 && S != 4)) return -1;
    const int NW = (n + 31) / 32;
    unsigned wbits[256];
    for (int w = 0; w < NW; ++w) {
        unsigned m = 0u;
        for (int i = w << 5; i < (w << 5) + 32 && i < n; ++i) {
            union { float f; unsigned u; } c;
            c.f = weights[i];
            m = c.u > m ? c.u : m;
        }
        wbits[w] = m;
    }
    double H[4] = {0.0, 0.0, 0.0, 0.0};
    if (NW > S)
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < 32; ++i) H[s] += (double)weights[(s << 5) + i];
    return mc_launch_cut_s(wbits, NW, S, H, min_bits, max_bits, cut4);
}

// mc_mono_from on the host, from a table's weights: mono4[s], s < S, as k_mc_cut writes it for a launch of S slices.  Needs no GPU.
extern "C" int pbrk_mc_mono_slices(const float* weights, int n, int S, int* mono4) {
    if (!weights || !mono4 || n < 1 || n > 8192 || (S != 1 && S != 2 && S != 4)) return -1;
    const int NW = (n + 31) / 32;
    unsigned wbits[256];
    for (int w = 0; w < NW; ++w) {
        unsigned m = 0u;
        for (int i = w << 5; i < (w << 5) + 32 && i < n; ++i) {
            union { float f; unsigned u; } c;
            c.f = weights[i];
            m = c.u > m ? c.u : m;
        }
        wbits[w] = m;
    }
    mc_mono_from(wbits, NW, S, mono4);
    return 0;
}

// Scratch for those tables: a ring of slots in device memory, allocated once per device.  A slot is written by k_mc_prep and read
// by the region kernel behind it on the same stream; an event recorded behind that reader is waited for, in-stream, by the next
// launch that takes the slot, so launches in flight on different streams (the tile streams of GPU_GraphSubmit) never share one.
#define PREP_SLOTS 32
struct PrepRing { unsigned* dev; hipEvent_t ev[PREP_SLOTS]; bool used[PREP_SLOTS]; unsigned next; };
static PrepRing g_prep[MC_MAX_DEVICES];
static std::mutex g_prep_lock;

// The slot for one launch on `st` (its previous reader waited for), or null: no device memory, or `st` is being captured into a
// graph -- a replayed graph keeps the slot it was recorded with, and nothing would order its replays against later launches.
static unsigned* prep_acquire(hipStream_t st, int* slot_out) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (cs != hipStreamCaptureStatusNone) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MC_MAX_DEVICES) return nullptr;
    PrepRing& R = g_prep[dev];
    if (!R.dev) {
        if (hipMalloc(&R.dev, (size_t)PREP_SLOTS * PREP_SLOT_WORDS * 4) != hipSuccess) { (void)hipGetLastError(); R.dev = nullptr; return nullptr; }
        for (int i = 0; i < PREP_SLOTS; ++i) {
            R.used[i] = false;
            if (hipEventCreateWithFlags(&R.ev[i], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(R.dev); R.dev = nullptr; return nullptr; }
        }
        R.next = 0;
    }
    const int slot = (int)(R.next++ % PREP_SLOTS);
    if (R.used[slot] && hipStreamWaitEvent(st, R.ev[slot], 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *slot_out = slot;
    return R.dev + (size_t)slot * PREP_SLOT_WORDS;
}

// The ring's lock is held from here until mc_prep_release, behind the slot's reader; a launch that gets no slot holds nothing.
McPrepSlot mc_prep_acquire(hipStream_t st) {
    McPrepSlot s;
    s.hold = std::unique_lock<std::mutex>(g_prep_lock);
    s.words = prep_acquire(st, &s.slot);
    if (!s.words) s.hold.unlock();
    else (void)hipGetDevice(&s.dev);
    return s;
}
// k_mc_prep and, where the plan has a cut, k_mc_cut behind it: what they leave in the slot is RegArgs::tabmax
void mc_prep_launch(const McPrepSlot& s, const McArgs& a, const McPlan& p, hipStream_t st) {
    hipLaunchKernelGGL(k_mc_prep, dim3((unsigned)(p.NR + (p.NW + 255) / 256)), dim3(256), 0, st, a.src, a.n_src, p.G, p.RC, p.NR, a.tab, a.n_tab, p.NW, s.words);
    if (p.cut) hipLaunchKernelGGL(k_mc_cut, dim3(1), dim3(64), 0, st, a.tab, a.n_tab, p.NW, p.NR, p.nslices, s.words);
}
// behind the region kernel that read the slot
void mc_prep_release(McPrepSlot& s, hipStream_t st) {
    if (!s.words) return;
    if (hipEventRecord(g_prep[s.dev].ev[s.slot], st) == hipSuccess) g_prep[s.dev].used[s.slot] = true;
    s.words = nullptr;
    s.hold.unlock();
}
