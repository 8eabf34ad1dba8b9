// mc_refine_core.h -- the word logic of k_mc_refine_bins (k_mc_region.hip, header 2n): from "which lanes take sample i in region r"
// to the tile's new mask words and proof word.  Written once for the kernel and for a host compiler (tests/mc_refine_core_host.cpp).
//
// One mask word holds 32 samples.  The bound of region_bin left, per word, NR mask words old[r] (bit i: sample i may reach region r from
// some texel of the tile) and one proof word (bit i: every texel takes sample i in the one region flagged for it).
//   need  = the samples the kernel looks at: flagged and unproved, or flagged for more than one region.  A sample the bound proved
//           for its only region is exact already.
//   hit[r]  bit i: some lane of the slice's waves takes sample i in region r (OR of the waves' mc_refine_ballot).
//   part[r] bit i: some wave of the slice had a lane that does not take sample i in r (a wave with no lane in r among them).
// New mask word of region r: old[r] outside need; inside need exactly the hits -- but never a bit the bound had not set: such a hit is
// counted (unset) and dropped.  New proof bit inside need: exactly one region is hit and every lane of every wave is in it (hit and
// not part): region_bin's SOLE for free.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_REFINE_FN __host__ __device__ inline
#else
#define MC_REFINE_FN inline
#endif

MC_REFINE_FN unsigned mc_refine_popc(unsigned v) {
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (((v + (v >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24;
}

// the samples of a word that need the lanes' decision; old[r * stride]: region r's mask word
MC_REFINE_FN unsigned mc_refine_need(const unsigned* old, int stride, int NR, unsigned proved) {
    unsigned once = 0u, twice = 0u;
    for (int r = 0; r < NR; ++r) {
        const unsigned m = old[r * stride];
        twice |= once & m;
        once |= m;
    }
    return (once & ~proved) | twice;
}

// one wave's answer for (region, sample i): b = the lanes that take the sample in the region
MC_REFINE_FN void mc_refine_ballot(unsigned long long b, int i, unsigned& hit, unsigned& part) {
    if (b != 0ull) hit |= 1u << i;
    if (b != ~0ull) part |= 1u << i;
}

// The word's new masks (out[r * ostride]) and proof word (returned) from the slice's combined hit[] / part[] (stride hstride).
// unset: += the hits on a bit the bound had not set (must stay 0: the bound is rigorous); they are not written.
MC_REFINE_FN unsigned mc_refine_word(const unsigned* old, int stride, int NR, unsigned proved, unsigned need, const unsigned* hit,
                                     const unsigned* part, int hstride, unsigned* out, int ostride, unsigned long long* unset) {
    unsigned once = 0u, twice = 0u, full = 0u;
    for (int r = 0; r < NR; ++r) {
        const unsigned o = old[r * stride], h = hit[r * hstride] & need;
        *unset += mc_refine_popc(h & ~o);
        twice |= once & h;
        once |= h;
        full |= h & ~part[r * hstride];
        out[r * ostride] = (o & ~need) | (h & o);
    }
    return (proved & ~need) | (once & ~twice & full & need);
}
