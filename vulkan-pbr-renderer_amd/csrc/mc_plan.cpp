// mc_plan.cpp -- the launch plan of the Monte-Carlo filter's region and resident kernels, the process switches and what the last launch
// took (mc_plan.h).  The kernels are in k_mc_region.hip; its header's 2a - 2n say what each decision is about.
#include "mc_plan.h"
#include "k_mc_internal.h"

#include <stdlib.h>

// ---- the switches (tests / A-B runs).  One block, set by pbrk_mc_set_*, resolved by mc_switches() ----
//   region, lds  which kernel serves a level: -1 = the environment variable PBR_MC_REGION / PBR_MC_LDS, else the default 1
//   absorb       skipping of absorbed words (header 2c; the outputs are the same bit for bit either way)
//   runs         the round-5 loop of the 66^2 shapes (k_mc_region RUNS; same bytes)
//   lean         the prologue of header 2f (k_mc_region LEAN; 0: the prologue before it; same bytes)
//   launch_cut   the launch-level cut of header 2g (same bytes)
//   tile32       the 32 x 32 tile of header 2h: -1 the rule of mc_tile32 (default), 0 never, 1 wherever the shape allows it (quarter faces,
//                NW <= 64) whatever the output size.  The tile changes the order of a texel's sum: not the same bytes as 16 x 16 x 4
//   fold         half_n folded into the frame rows on power-of-two levels (header 2j; same bytes)
//   net          the completeness net of the header's step 3 (2l; same bytes): -1 the default rule -- on when the device counters are on
//                (PBR_MC_STATS=1), off otherwise --, 0 off wherever a net-less instantiation exists (the lean run loops), 1 always on.
//                The rule reads nothing of the dispatch
//   resident     header 2k: 0: such a level runs the kernel it ran before (n_src = 16: k_mc_region<18, ..>; smaller: the level-in-LDS
//                kernel); -1: the environment variable PBR_MC_RESIDENT, else the default 1
//   bin_cache    header 2m: -1 the environment (PBR_MC_BIN_CACHE=0|1), else on exactly when the device counters are off
//   exact_bins   header 2n: -1 the environment (PBR_MC_EXACT_BINS=0|1), else the counters' rule and McShape::EXACT_DEFAULT
static McSwitches g_sw = {-1, -1, 1, 1, 1, 1, -1, 1, -1, -1, -1, -1};

// the environment's word for a switch, read once: `unset` where the variable is not set
struct McEnv { int region, lds, resident, bin_cache, exact_bins, stats; };
static int env_int(const char* name, int unset, bool as_flag) {
    const char* e = getenv(name);
    return e ? (as_flag ? (atoi(e) ? 1 : 0) : atoi(e)) : unset;
}
static const McEnv& mc_env() {
    static const McEnv env = {env_int("PBR_MC_REGION", 1, false), env_int("PBR_MC_LDS", 1, false), env_int("PBR_MC_RESIDENT", 1, true),
                              env_int("PBR_MC_BIN_CACHE", -1, true), env_int("PBR_MC_EXACT_BINS", -1, true), env_int("PBR_MC_STATS", 0, false)};
    return env;
}
McSwitches mc_switches() {
    const McEnv& env = mc_env();
    McSwitches sw = g_sw;
    if (sw.region < 0) sw.region = env.region;
    if (sw.lds < 0) sw.lds = env.lds;
    if (sw.resident < 0) sw.resident = env.resident;
    if (sw.bin_cache < 0) sw.bin_cache = env.bin_cache;
    if (sw.exact_bins < 0) sw.exact_bins = env.exact_bins;
    return sw;
}
bool mc_counters_wanted() { return mc_env().stats != 0; }

static int tri(int mode) { return mode < 0 ? -1 : (mode ? 1 : 0); }
extern "C" void pbrk_mc_set_kernels(int region, int lds) { g_sw.region = region; g_sw.lds = lds; }
extern "C" void pbrk_mc_set_absorb(int on) { g_sw.absorb = on ? 1 : 0; }
extern "C" void pbrk_mc_set_runs(int on) { g_sw.runs = on ? 1 : 0; }
extern "C" void pbrk_mc_set_prologue(int lean) { g_sw.lean = lean ? 1 : 0; }
extern "C" void pbrk_mc_set_launch_cut(int on) { g_sw.launch_cut = on ? 1 : 0; }
extern "C" void pbrk_mc_set_tile32(int mode) { g_sw.tile32 = tri(mode); }
extern "C" void pbrk_mc_set_fold(int on) { g_sw.fold = on ? 1 : 0; }
extern "C" void pbrk_mc_set_net(int mode) { g_sw.net = tri(mode); }
extern "C" void pbrk_mc_set_resident(int on) { g_sw.resident = tri(on); }
extern "C" void pbrk_mc_set_bin_cache(int mode) { g_sw.bin_cache = tri(mode); }
extern "C" void pbrk_mc_set_exact_bins(int mode) { g_sw.exact_bins = tri(mode); }

// Which tile serves a level (header 2h): a function of the level alone -- n_src, n_tab, the output size -- never of the dispatch's faces
// or rows, so a row shard equals the full dispatch bit for bit.  32 x 32 x 1 needs the quarter-face shape (its body is the shortest and
// its prologue the largest share) and NW <= 64 (one ballot of region_pass_runs); the rule adds size >= MC_TILE32_MIN_SIZE: below it
// the level has too few 32 x 32 tiles to fill the chip (profiles/r09_tile32.md).
static bool mc_tile32(const McSwitches& sw, int n_src, int n_tab, int size) {
    if (n_src <= 64 || (n_tab + 31) / 32 > 64) return false;
    const int mode = sw.tile32 < 0 ? (MC_TILE32_SUB ? -1 : 0) : sw.tile32;
    return mode > 0 || (mode < 0 && size >= MC_TILE32_MIN_SIZE);
}

// Every rule reads the level alone -- n_src, n_tab, the output size -- or the process (switches, counters), never the dispatch's faces or rows:
// a row shard equals the full dispatch bit for bit.  Only what the bin cache may do (bin_eligible, whole) depends on the window.
McPlan mc_plan(const McSwitches& sw, int n_src, int n_tab, int size, int face0, int nfaces, int y0, int rows, bool counters, bool have_prep) {
    McPlan p = {};
    p.family = MC_DECLINED;
    p.lds_slices = mc_lds_slices(sw.lds, n_src, size);              // what a declined level runs: the level-in-LDS kernel, else the direct one
    p.direct_slices = mc_direct_slices(size);
    if (!sw.region || n_tab < 1 || n_tab > 8192) return p;
    p.NW = (n_tab + 31) / 32;                                       // mask words per region
    p.stats = counters ? 1 : 0;
    p.whole = face0 == 0 && nfaces == 6 && y0 == 0 && rows == size;
    p.bin_cache = sw.bin_cache < 0 ? !counters : sw.bin_cache != 0;
    const bool pow2 = (n_src & (n_src - 1)) == 0;                   // header 2j: FOLD from n_src alone
    // Header 2k, asked first: n_src <= 16 and an output of 256^2 or more take 16 x 16 tiles x 4 slices, outputs of 128^2 .. 255^2 take
    // 8 x 8 tiles x 16 slices (MC_RESIDENT_TILE8), smaller ones stay on the level-in-LDS kernel of k_mc.hip.  The tiles are anchored at row
    // 0 of the face, so every dispatch may replay its binning; the entries are never refined (2n: the bytes would move).
    if (sw.resident && n_src <= 16 && size >= (MC_RESIDENT_TILE8 ? 128 : 256)) {
        p.family = MC_RESIDENT;
        p.RS = RES_RS; p.G = 1; p.RC = n_src + 1; p.NR = 6;
        p.tile = size >= 256 ? 16 : 8; p.nslices = 1024 / (p.tile * p.tile);
        p.fold = sw.fold && pow2;
        p.lds = (int)mc_resident_lds(p.NW);
        p.bin_eligible = 1;
        p.bin_flavour = (1 << 16) | p.tile;
        return p;
    }
    // shape conditions (level only): source too big for LDS as a whole, enough 16x16 tiles to fill the chip twice over
    if (n_src < 16 || size < 256) return p;
    if (n_src <= 16) { p.RS = 18; p.G = 1; p.RC = n_src + 1; }
    else if (n_src <= 32) { p.RS = 34; p.G = 1; p.RC = n_src + 1; }
    else if (n_src <= 64) { p.RS = 66; p.G = 1; p.RC = n_src + 1; }
    else { p.RS = 66; p.RC = 65; p.G = (n_src + 1 + 64) / 65; }
    p.NR = 6 * p.G * p.G;
    // Tile size: 16 x 16 output texels x 4 slices of the sample table, but for the quarter-face level with a short table and a big
    // output (mc_tile32: header 2h), which takes 32 x 32 texels x 1 slice.  Measured and dropped: 8 x 8 tiles x 16
    // slices (halve the frame spread, pay four times the per-tile work: C4 mip 2 44.0 -> 53.5 ms), 32 x 16 tiles, and 32 x 32 tiles on
    // the whole-face and the small shapes (no gain on the big levels, losses on the small ones).
    p.tile = mc_tile32(sw, n_src, n_tab, size) ? 32 : 16; p.nslices = 1024 / (p.tile * p.tile);
    bool two = false, has_runs = false, net_off = false, abs = false, exact_default = false;
    mc_for_shape(p.RS, p.G, p.tile, [&](auto sh) {
        two = sh.TWO; has_runs = sh.HAS_RUNS; net_off = sh.NET_OFF; abs = sh.ABS; exact_default = sh.EXACT_DEFAULT;
    });
    // where wmax[] and rmax[] do not fit, the level runs without absorbed words; two workgroups per CU or not at all
    p.absorb = abs ? sw.absorb : 0;
    if (mc_region_lds(p.RS, p.NR, p.NW, p.absorb != 0) > 80 * 1024) p.absorb = 0;
    const size_t lds = mc_region_lds(p.RS, p.NR, p.NW, p.absorb != 0);
    if (lds > 80 * 1024) return p;
    p.family = MC_REGION;
    p.lds = (int)lds;
    for (int w = 0; w < p.NW; ++w) { const int c = n_tab - w * 32; p.expect[w % p.nslices] += c > 32 ? 32 : c; }
    // Lean prologue (2f): the maxima of the absorbed-word test come from k_mc_prep, once per launch, instead of from every tile.  Without
    // a scratch slot the launch takes the prologue that builds them itself: the same bytes.
    const bool want_prep = sw.lean && p.absorb;
    p.prep = want_prep && have_prep && p.NW + 2 * p.NR + 8 <= PREP_SLOT_WORDS;
    p.lean = sw.lean && (!want_prep || p.prep);
    // header 2g: the shapes that run their head words first drop the words k_mc_cut proves to be no-ops for the whole launch
    p.head_first = two;
    p.cut = p.prep && two && sw.launch_cut && p.NW > p.nslices;
    // The round-5 loop on the shapes that have it, or the pass before it.  One ballot of region_pass_runs covers 64 words per slice: a
    // longer table takes the pass before it as well (at most 8192 samples, 256 words, are admitted and mc_tile32 admits at most 64 words
    // on the one-slice tile, so today that never happens).
    p.runs = has_runs && sw.runs && p.NW <= 64 * p.nslices;
    // header 2j: only the lean run loop has the folded instantiation.  header 2l: the net is a rule of the process, never of the dispatch
    p.fold = p.runs && p.lean && sw.fold && pow2;
    p.net = !(p.runs && p.lean && net_off) || (sw.net < 0 ? counters : sw.net != 0);
    // header 2m: the lean run loops may record or replay their binning; the 66^2 shapes without a k_mc_prep slot bin as ever, the 34^2
    // shape never takes one
    p.bin_eligible = p.runs && p.lean && (p.prep || p.RS == 34) && mc_bin_window_ok(size, p.tile, y0, y0 + rows);
    p.bin_flavour = (p.RS << 8) | p.tile;
    // header 2n: behind a recording launch (a whole-level one that finds no entry) k_mc_refine_bins makes the entry's flags exact
    p.refine = p.bin_cache && p.bin_eligible && p.whole && (sw.exact_bins < 0 ? !counters && exact_default : sw.exact_bins != 0)
               && mc_refine_lds(p.NR, p.NW) <= 64 * 1024;
    return p;
}

extern "C" int pbrk_mc_plan(int n_src, int n_tab, int size, int face0, int nfaces, int y0, int rows, int counters, int have_prep, PbrkMcPlan* out) {
    if (!out || n_src < 1 || size < 1 || face0 < 0 || nfaces < 1 || face0 + nfaces > 6 || y0 < 0 || rows < 1 || y0 + rows > size) return PBRK_E_ARG;
    *out = mc_plan(mc_switches(), n_src, n_tab, size, face0, nfaces, y0, rows, counters != 0, have_prep != 0);
    return PBRK_OK;
}

// ---- what the last region-kernel launch took ----
static McPlan no_launch_yet() { McPlan p = {}; p.net = 1; p.nslices = 4; return p; }
McLast g_mc_last = {no_launch_yet(), nullptr, 0};
// 1 when the last region-kernel launch ran a FOLD instantiation, else 0 (also before the first launch)
extern "C" int pbrk_mc_last_fold(void) { return g_mc_last.plan.fold; }
// 1 when the last region-kernel launch carried the net, 0 when it ran a net-less instantiation (1 before the first launch)
extern "C" int pbrk_mc_last_net(void) { return g_mc_last.plan.net; }
extern "C" int pbrk_mc_last_exact_bins(void) { return g_mc_last.refined; }
// The cut of the last region-kernel launch, for tests and probes: out6 = the first cut word of slices 0 .. 3, NW, words cut.  A launch
// without a cut reports 0 words.  A launch of S < 4 slices reports slice j % S in entry j (one slice: its first cut word four times);
// the words cut are counted over the launch's S slices.  Waits for the device.
extern "C" int pbrk_mc_launch_cut_stats(int* out6) {
    if (!out6) return PBRK_E_ARG;
    const int NW = g_mc_last.plan.NW, S = g_mc_last.plan.nslices;
    for (int j = 0; j < 4; ++j) { const int s = j % S; out6[j] = s >= NW ? s : s + S * ((NW - s + S - 1) / S); }
    out6[4] = NW; out6[5] = 0;
    if (!g_mc_last.cut) return PBRK_OK;
    if (hipDeviceSynchronize() != hipSuccess) return PBRK_E_LAUNCH;
    int c[4];
    if (hipMemcpy(c, g_mc_last.cut, 16, hipMemcpyDeviceToHost) != hipSuccess) return PBRK_E_LAUNCH;
    for (int s = 0; s < 4; ++s) { if (s < S) out6[5] += (out6[s] - c[s]) / S; out6[s] = c[s]; }
    return PBRK_OK;
}
