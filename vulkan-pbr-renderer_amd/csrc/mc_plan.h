// mc_plan.h -- which kernel serves a level of the Monte-Carlo filter (k_mc_region.hip, header 2a - 2n), decided in ONE place.
//   McShape<RS, SUB, TILE>: the compile-time facts of a kernel shape; k_mc_region, k_mc_refine_bins and mc_plan all read them.
//   mc_for_shape:           the one ladder from (RS, G, tile) to <RS, SUB, TILE>; the region launch and the refine launch both take it.
//   McSwitches:             the process switches (pbrk_mc_set_*), resolved against their defaults and the environment in mc_switches().
//   mc_plan:                level + dispatch + switches + counters + "a k_mc_prep slot was obtained" -> everything a launch decides.
// Plain host C++: no HIP call, no global but the switches handed in.
#pragma once
#include "pbr_kernels.h"

#define REG_MAX_S 16
// Header 2g, decided per 66^2 shape by measurement: head words first (and with it the launch-level cut) on the quarter-face shape
// (SUB) / on the whole-face shape (G == 1).  0 keeps the shape's earlier order and bytes.
#ifndef MC_HEAD_FIRST_SUB
#define MC_HEAD_FIRST_SUB 1
#endif
#ifndef MC_HEAD_FIRST_G1
#define MC_HEAD_FIRST_G1 1
#endif
// Header 2i, decided per whole-face shape by measurement: under RUNS the samples binning proves for the whole tile run as test-free runs
// (CERT in k_mc_region).  The 34^2 shape takes them; MC_CERT_G1 is the 66^2 whole-face shape: 0 keeps the machine code it had without.
#ifndef MC_CERT_G1
#define MC_CERT_G1 1
#endif

// Header 2j, decided per shape by measurement: the folded instantiation of the 66^2 whole-face shape keeps a tap's four texels alive with
// one statement, so that their LDS reads wait once (tap_accumulate, JOIN).  0 keeps the two waits; the other shapes lose or gain nothing with it.
#ifndef MC_TAP_JOIN_G1
#define MC_TAP_JOIN_G1 1
#endif

// Header 2h: 32 x 32 tiles x 1 slice on the quarter-face shape where mc_tile32's rule holds.  0 keeps 16 x 16 x 4 and the parent's bytes
// (pbrk_mc_set_tile32(1) still selects the tile).
#ifndef MC_TILE32_SUB
#define MC_TILE32_SUB 1
#endif
// Header 2l, decided by measurement: the 34^2 shape has no absorbed words and loses only the count with its net; 0 keeps its net always.
#ifndef MC_NET_OFF_34
#define MC_NET_OFF_34 1
#endif
// Header 2l, decided by measurement: the net-less kernel ends a pass at the first absorbed word behind which the slice's word maxima never rise.
#ifndef MC_MONO_EXIT
#define MC_MONO_EXIT 1
#endif
#ifndef MC_TILE32_MIN_SIZE
#define MC_TILE32_MIN_SIZE 1024
#endif
#ifndef MC_RESIDENT_TILE8
#define MC_RESIDENT_TILE8 1                            // outputs of 128^2 .. 255^2 take 8 x 8 tiles x 16 slices; 0: they keep the level-in-LDS kernel
#endif
// k_mc_resident: every face is staged with the row pitch of the 18^2 shape, whatever n_src <= 16 is: face f's block starts RES_FACE_BYTES f behind the base.
#define RES_RS 18
#define RES_FACE_BYTES (RES_RS * RES_RS * 16)
#define PREP_SLOT_WORDS 4096                                    // k_mc_prep's scratch slot: NW <= 256; NR (NW + 1) words of masks fit 80 KB of LDS behind the region

template <int RS_, bool SUB_, int TILE_>
struct McShape {
    static constexpr int RS = RS_, TILE = TILE_, REG_TX = TILE_ * TILE_, REG_S = 1024 / REG_TX;
    static constexpr bool SUB = SUB_;
    // see the header, 2c: compiled for the 66^2 region shapes only.  The 34^2 / 18^2 levels of C4 (mips 3, 4: weights fall to ~e^-6)
    // never absorb a word, and the test alone cost them 7 % (measured); without it their code is that of round 3
    static constexpr bool ABS = RS_ == 66;
    // see the header, 2e: the order pays through the absorbed words, so it is taken where they are compiled.  The 34^2 / 18^2 shapes keep
    // index order and their bytes: there the reordered sums bought nothing and moved C4 mip 3 to 2.5e-5 from the direct kernel,
    // past the 2e-5 of the every-texel cross-check (test_gpu_configs.py)
    static constexpr bool OWN_FIRST = ABS;
    // see the header, 2g: head words first, then the tail words; decided per 66^2 shape (MC_HEAD_FIRST_SUB / MC_HEAD_FIRST_G1)
    static constexpr bool TWO = RS_ == 66 && (SUB_ ? MC_HEAD_FIRST_SUB != 0 : MC_HEAD_FIRST_G1 != 0);
    // see the header, 2i: the run loop (RUNS) loses on the 18^2 shape, which has no such instantiation
    static constexpr bool HAS_RUNS = RS_ != 18;
    // see the header, 2l: the lean run loop has a form without the completeness net
    static constexpr bool NET_OFF = HAS_RUNS && (RS_ != 34 || MC_NET_OFF_34 != 0);
    // Header 2n: the shapes whose recorded flags are refined under the default rule, decided per shape by measurement (profiles/exact_bins.md;
    // a shape is in when its replaying kernel, levels one after another, falls by more than five times the larger sigma of its two rows).
    //   <34, false, 16> (C4 mip 3): 10.77 -> 10.13 ms, sigma 0.09: in.
    //   <66, true, 32>  (C4 mip 1):  7.15 ->  6.70 ms, sigma 0.17: a fall of 2.6 sigma, out.
    //   <66, false, 16> (C4 mip 2): 21.32 -> 21.25 ms, sigma 0.29: out.
    //   <66, true, 16>: on no level of the measured job; out.
    // pbrk_mc_set_exact_bins(1) refines every shape that has k_mc_refine_bins (tests, A-B runs).
    static constexpr bool EXACT_DEFAULT = RS_ == 34;
};

// f(McShape<RS, SUB, TILE>{}) for the shape that serves (RS, G regions per face edge, tile)
template <class F>
static inline void mc_for_shape(int RS, int G, int tile, F&& f) {
    if (tile == 32) f(McShape<66, true, 32>{});
    else if (RS == 18) f(McShape<18, false, 16>{});
    else if (RS == 34) f(McShape<34, false, 16>{});
    else if (G == 1) f(McShape<66, false, 16>{});
    else f(McShape<66, true, 16>{});
}

// Dynamic LDS of the three kernel families, in bytes: each is the pointer chain at the top of its kernel, and moves with it.
//   k_mc_region: the staged region (RS^2 texels), then in words skc[4] | masks[NR NW] | any[NR] | dmax[1] | cmask[NW], and with absorbed
//   words wmax[NW] | rmax[NR]; never less than the slices' partial sums (REG_S * REG_TX = 1024 texel-slices, whatever the tile)
static inline size_t mc_region_lds(int RS, int NR, int NW, bool absorb) {
    const size_t lds = (size_t)RS * RS * 16 + (4 + (size_t)NR * NW + NR + 1 + NW) * 4 + (absorb ? (size_t)(NW + NR) * 4 : 0);
    return lds < (size_t)1024 * 3 * 4 ? (size_t)1024 * 3 * 4 : lds;
}
//   k_mc_resident: the level (6 faces), then masks[6 NW] | any[6] | dmax[1] | cmask[NW]; the slices' partial sums overlay the level (12 KB of its 30)
static inline size_t mc_resident_lds(int NW) { return (size_t)6 * RES_FACE_BYTES + ((size_t)6 * NW + 6 + 1 + NW) * 4; }
//   k_mc_refine_bins: old[NR NW + NW] | need[NW] | hit[NR NW] | part[NR NW] | tot[8]
static inline size_t mc_refine_lds(int NR, int NW) { return ((size_t)3 * NR * NW + 2 * (size_t)NW + 8) * 4; }

// ---- a declined level: the kernels of k_mc.hip.  Both rules read the LEVEL alone (deterministic under sharding) ----
// The level-in-LDS kernel k_mc_filter_lds<S>: S slices of the sample table, or 0 where the level does not fit or loses there.
static inline int mc_lds_slices(int mode, int n_src, int size) {
    const size_t lvl_bytes = (size_t)6 * (n_src + 2) * (n_src + 2) * 16, texels = (size_t)6 * size * size;
    if (!mode || lvl_bytes > 112 * 1024) return 0;
    // Measured (C4 / C2 on MI355X): with a 111 KB level only one 1024-thread workgroup fits per CU (16 waves) and the
    // VALU-bound loop runs at ~4.4 clk/instruction; the direct kernel (32 waves/CU, 3 loads/sample) then wins on big
    // outputs.  Small levels (several workgroups per CU) and small outputs (launch-limited) win with LDS.
    if (lvl_bytes > 48 * 1024 && texels > ((size_t)1 << 19)) return 0;
    int S = 1;                                                      // at least 512 workgroups of 1024 threads
    while (S < 1024 && texels * (size_t)S < (size_t)512 * 1024) S <<= 1;
    return S;
}
// The direct kernel k_mc_filter<S, ..>.  Enough workgroups to fill 256 CUs several times over: split the sample table when texels are
// few.  Never fewer than 4 slices: a 256-texel workgroup walking all 8192 samples runs for ~5.6 ms, and a share of the level (one rank's
// tiles) that is only a few such rounds long loses up to a round in its tail; 4 slices of 64 texels (one wave each, table entries still
// wave-uniform scalar loads) cost nothing and cut that tail by four (8-way share: 18.1 -> 17.3 ms mean).
static inline int mc_direct_slices(int size) {
    int S = 4;
    while (S < 256 && (size_t)6 * size * size * (size_t)S < (size_t)2048 * 256) S <<= 1;
    return S;
}

// The process switches.  -1 where a switch has a default RULE (tile32, net, bin_cache, exact_bins: see mc_plan); mc_switches() has already
// replaced the -1 of region / lds / resident / bin_cache / exact_bins by the environment's word or the default.
struct McSwitches { int region, lds, absorb, runs, lean, launch_cut, tile32, fold, net, resident, bin_cache, exact_bins; };
McSwitches mc_switches();
bool mc_counters_wanted();                      // PBR_MC_STATS

enum { MC_DECLINED = 0, MC_REGION = 1, MC_RESIDENT = 2 };
typedef PbrkMcPlan McPlan;
McPlan mc_plan(const McSwitches& sw, int n_src, int n_tab, int size, int face0, int nfaces, int y0, int rows, bool counters, bool have_prep);

// What the last k_mc_region launch took (pbrk_mc_last_fold, _last_net, _launch_cut_stats) and whether the last recording one was refined
struct McLast { McPlan plan; const unsigned* cut; int refined; };
extern McLast g_mc_last;
