/*
 * pbr_kernels.h -- low-level C ABI of the gfx950 kernels (device pointers + stream in, status out).
 *
 * This is the layer *under* the GPU_* boundary of include/gpu_hip.h: every entry point takes
 * plain device pointers and sizes, launches asynchronously on `stream` (a hipStream_t passed as
 * void*) and returns 0 or a negative PBRK_E_* code after validating shapes on the host (no launch
 * happens when validation fails).  Each entry names the reference code it replaces.
 *
 * Memory layouts (all tightly packed, little endian):
 *   cube level        float4 [6][n][n]                (RGBA32F, face order +X,-X,+Y,-Y,+Z,-Z)
 *   cube pyramid      levels 0..L-1 back to back, level l has n_l = max(1, W >> l)
 *   bordered level    float4 [6][n+2][n+2]            (apron = adjacent faces' edge texels)
 *   bordered pyramid  bordered levels back to back
 *   G-buffer planes   uchar4 [H][W] x4, float [H][W]  (base colour, normal, ORM, emissive, depth)
 *   lit frame         half4 [H][W] or float4 [H][W]
 */
#ifndef PBR_KERNELS_H
#define PBR_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PBRK_OK = 0,
    PBRK_E_ARG = -1,        /* null pointer / non-positive size / bad range */
    PBRK_E_FORMAT = -2,     /* unsupported pixel format */
    PBRK_E_LAUNCH = -3      /* hipGetLastError() != hipSuccess after the launch */
};

enum {                      /* output formats understood by the kernels */
    PBRK_FMT_RG16F = 1,
    PBRK_FMT_RG32F = 2,
    PBRK_FMT_RGBA16F = 3,
    PBRK_FMT_RGBA32F = 4,
    PBRK_FMT_R32F = 5,      /* depth planes as sampled by the post-process passes */
    PBRK_FMT_RGBA8UN = 6,
    PBRK_FMT_BGRA8UN = 7
};

enum {                      /* shade flags (reference lighting_pass.glsl sub-blocks) */
    PBRK_SHADE_IBL = 1 << 0,     /* ambient = irradiance(N); spec = prefiltered(R, rough*4)  (:690, :699) */
    PBRK_SHADE_SHAFTS = 1 << 1,  /* light-shaft loop (:622-651); visibility == 1 unless PBRK_SHADE_SHADOWS */
    PBRK_SHADE_SHADOWS = 1 << 2, /* sun shadow: 4 PCF taps of the sun depth map (:594-608) + shaft visibility (:646) */
    PBRK_SHADE_GI = 1 << 3,      /* the live ambient / specular terms: SampleRadianceWithScreenSpaceTrace (:273-424, :685, :701) */
    PBRK_SHADE_SH9 = 1 << 4      /* with PBRK_SHADE_IBL only: ambient = the SH9 irradiance of sh9_coef at N (csrc/sh_shade_core.h) in place of the
                                    irradiance cube, which is then neither required nor read; under PBRK_SHADE_GI the trace replaces it as always */
};

/* sizes / offsets of the pyramid layouts, in float4 texels */
size_t pbrk_level_offset(int W, int level);
size_t pbrk_pyramid_texels(int W, int levels);
size_t pbrk_bordered_level_offset(int W, int level);
size_t pbrk_bordered_pyramid_texels(int W, int levels);
int    pbrk_mip_count(int w, int h);                    /* src/gpu/gpu_vulkan.c:1344-1351 */

/* ---- host-side tables (libm on the host, so CPU and GPU agree bit-for-bit on directions/weights) -----
 * angles[i] = (cos pitch_i, sin pitch_i, cos yaw_i, sin yaw_i), the Fibonacci hemisphere of
 * gen_prefiltered_env_map.glsl:125-128 / gen_irradiance_map.glsl:85-88 / gen_brdf_integration_map.glsl:171-174 */
void   pbrk_host_sample_angles(int nsamples, float* angles4);
/* Prefilter table (gen_prefiltered_env_map.glsl:122-143): entries (lx, ly, lz, w) for the samples
 * whose weight w = D_i*cos(pitch_i)*dw is non-zero, in index order.  Returns the entry count;
 * *alpha receives the texel-independent alpha channel sum_i(w_i)/PI evaluated in shader order. */
int    pbrk_host_prefilter_table(int nsamples, float roughness, float* table4, float* alpha);
/* Irradiance table (gen_irradiance_map.glsl:84-96): entries (lx, ly, lz, cos pitch_i). */
int    pbrk_host_irradiance_table(int nsamples, float* table4);

/* ---- K2: mip chain, replaces GPU_OpGenerateMipmaps' per-(level,face) linear blits
 *      (src/gpu/gpu_vulkan.c:1458-1483, :2786-2826): level l = 2x2 box mean of level l-1, per face. */
int pbrk_mip_chain(void* pyramid, int W, int levels, void* stream);
/* Cube-sampler convention (the reference leaves it to the driver, gpu_vulkan.c:613-634).  0 (default): exact fp32
 * tap weights.  1: texel coordinates and the LOD fraction snapped to 1/256, the sub-texel / mip-fraction resolution of real
 * texture units and of this repo's 2-D / 3-D samplers.  With 1, K3 / K4a / K4b / K5 run their general kernels (the fast ones
 * implement the default only): a switch to measure how far the outputs move between the two, not a production mode. */
/* {min, max} over the RGB values of `texels` float4 texels as fp32 bit patterns in out2_device (two unsigned, initialised by the
 * caller to {0x7F800000, 0}); a negative or NaN input reports min = 0.  Used by the tolerance-budgeted sample cut. */
int pbrk_level_minmax(const void* level, size_t texels, void* out2_device, void* stream);
void pbrk_set_cube_sampler_snap(int on);
int pbrk_get_cube_sampler_snap(void);
/* one exact 2:1 linear blit (GPU_OpBlit, gpu_vulkan.c:2786-2826) of `nlayers` square RGBA32F layers of size ns */
int pbrk_box_downsample(const void* src, int ns, void* dst, int nlayers, void* stream);
/* linear blit between whole RGBA32F subresources of any two sizes (all `nlayers` layers): the resample an odd mip level and a
 * non-2:1 GPU_OpBlit need (vkCmdBlitImage, unnormalised linear filter, clamp to edge; rule stated in oracle/pbr_oracle.c A2) */
int pbrk_blit_linear(const void* src, int ns_w, int ns_h, void* dst, int nd_w, int nd_h, int nlayers, void* stream);
/* GPU_OpClearColorF / GPU_OpClearColorI [gpu.h]: `bytes` at dst filled with a texel pattern of 1, 2, 4, 8 or 16 bytes (dst and bytes
 * multiples of the pattern size), one launch. */
int pbrk_fill_pattern(void* dst, unsigned long long bytes, const void* pattern, int pattern_bytes, void* stream);

/* ---- border build: pyramid -> bordered pyramid (seamless-cube apron; sampler state of
 *      src/gpu/gpu_vulkan.c:613-634 applied to a cube view). */
int pbrk_border_build(const void* pyramid, void* bordered, int W, int levels, void* stream);
/* the same for levels [level0, level1) of a `levels`-deep chain only (the other levels of `bordered` are left alone) */
int pbrk_border_build_range(const void* pyramid, void* bordered, int W, int levels, int level0, int level1, void* stream);

/* ---- K6 (extension): equirectangular RGBA32F panorama [h][w] -> cube level 0 [6][size][size].
 * Z-up: u = atan2(y,x)/2pi + .5 (wraps), v = acos(z/|d|)/pi (clamps); bilinear; angles in fp64. */
int pbrk_equirect_to_cube(const void* equirect_rgba32f, int w, int h, void* cube_level0, int size, void* stream);

/* ---- K7: light-grid sweep, shaders/lightgrid_sweep.glsl:9-75 (dispatch render.cpp:1064-1072).
 * image: RGBA16F [d][h][w], updated in place.  Invocations (iy, iz) in [y0,y1) x [z0,z1) each own one line of
 * PBRK_SWEEP_LEN voxels: direction 0 -> (x, iy, iz), 1 -> (iz, x, iy), 2 -> (iy, iz, x).  The line axis must be at
 * least PBRK_SWEEP_LEN long and the two ranges must lie inside the other two axes (checked; PBRK_E_ARG). */
#define PBRK_SWEEP_LEN 128
int pbrk_lightgrid_sweep(void* image_rgba16f, int w, int h, int d, int direction, int y0, int y1, int z0, int z1, void* stream);

/* ---- K1: split-sum BRDF LUT (shaders/gen_brdf_integration_map.glsl:142-210).
 * angles4: device copy of pbrk_host_sample_angles(nsamples); view_cs: device float2[size] with
 * (cos, sin) of acos((x+.5)/size) computed on the host.  Rows [y0,y1) are written. */
int pbrk_brdf_lut(void* out, int out_format, int size, int nsamples, const void* angles4,
                  const void* view_cs, int y0, int y1, void* stream);

/* ---- K4a: prefilter mip 0 = bilinear copy of one env level (gen_prefiltered_env_map.glsl:112-114).
 * src_bordered_level: bordered level of size n_src.  out: cube level [6][out_size][out_size]. */
int pbrk_prefilter_copy(const void* src_bordered_level, int n_src, void* out, int out_size,
                        int face0, int face1, int y0, int y1, void* stream);

/* ---- K4b / K3: Monte-Carlo hemisphere filter of one output level.
 * out.rgb = (sum_i w_i * bilinear(src, frame(texel) * l_i)) / divisor ; out.a = alpha.
 * Prefilter (gen_prefiltered_env_map.glsl:115-146): table from pbrk_host_prefilter_table, divisor PI.
 * Irradiance (gen_irradiance_map.glsl:81-97): table from pbrk_host_irradiance_table, divisor N, alpha 0. */
/* src_cells (optional, may be NULL): the same level in the 2x2-footprint "cells" layout built by pbrk_cells_build
 * (48 B per tap position, 3 loads per sample instead of 4; the vector-memory instruction rate bounds this kernel). */
size_t pbrk_cells_bytes(int n_src);
int pbrk_cells_build(const void* bordered_level, int n_src, void* cells, void* stream);
int pbrk_mc_filter(const void* src_bordered_level, const void* src_cells, int n_src, const void* table4, int n_entries,
                   float divisor, float alpha, void* out, int out_size,
                   int face0, int face1, int y0, int y1, void* stream);

/* self-check of the region kernel (PBR_MC_STATS=1): {wave-slices whose sample count came up short and were recomputed with
 * direct loads, all wave-slices}; the first must stay 0.  reset != 0 clears the counters after reading. */
int pbrk_mc_region_stats(unsigned long long* out2, int reset);
/* K4b / K3 kernel choice for tests and A-B runs: region = 0 skips the region kernel, lds = 0 the level-in-LDS kernel (the direct kernel
 * then serves every level); -1 = the environment (PBR_MC_REGION, PBR_MC_LDS) or the default 1.  Results agree to the order of the fp32 sums. */
void pbrk_mc_set_kernels(int region, int lds);
/* the binning's yield with the same switch: {(region, sample) flags set, samples x tiles, regions visited} summed over all tiles since the last reset */
int pbrk_mc_region_flag_stats(unsigned long long* out3);
/* samples that binning proved to tap one region from every texel of their tile (they run the body without tests), summed over tiles */
int pbrk_mc_region_window_stats(unsigned long long* out1);
/* absorbed words of the region kernel (PBR_MC_STATS=1), since the last reset: {wave-words skipped, their wave-samples, of those the
 * samples run through the count-only body}.  A tile's region passes visit 4 x (its region flags) wave-samples in all: the flag, sample,
 * region and proved-sample counters count per block of 256 texels, so a 32 x 32 tile enters them four times. */
int pbrk_mc_region_skip_stats(unsigned long long* out3);
/* skipping of mask words whose samples provably cannot change any lane's fp32 sums (default 1; tests and A-B runs): the outputs are
 * the same bit for bit either way */
void pbrk_mc_set_absorb(int on);
/* the region kernel's round-5 loop on the 66^2 region shapes (default on; the outputs are the same bit for bit either way) */
void pbrk_mc_set_runs(int on);
/* the region kernel's prologue (default 1: per-launch maxima from a preparation kernel, binning without run-time divisions, row-wise
 * staging; 0: the prologue before it; tests and A-B runs): the outputs are the same bit for bit either way */
void pbrk_mc_set_prologue(int lean);
/* builds with PBR_MC_PHASE_STAMPS and PBR_MC_STATS=1: clocks of each workgroup's first lane, summed since the last reset, in {frames,
 * clearing + binning, staging, region passes, reduction + store}; zeros in the product build */
int pbrk_mc_region_phase_stats(unsigned long long* out5);
/* the region kernel's visiting order: the k-th region (0 .. 6 G^2 - 1) a tile of `face` stages at G regions per face edge -- its own
 * face's regions first, then the others in index order; -1 for arguments out of range.  Host-side twin of the kernel's loop. */
int pbrk_mc_region_order(int face, int G, int k);
/* the region kernel's launch-level cut on the shapes that run each slice's head word first (default 1; tests and A-B runs): mask words
 * proved, once per launch, to be no-ops for every lane are not binned at all; the outputs are the same bit for bit either way */
void pbrk_mc_set_launch_cut(int on);
/* that proof on the host: weights[n] = the table's sample weights, min_bits / max_bits = the smallest / largest R, G, B bit pattern of
 * the bordered level.  cut4[s] = the first cut mask word of slice s (words s, s + 4, ..), or the slice's first index at or behind
 * ceil(n / 32) when none is cut.  Returns the number of words cut, -1 for bad arguments.  Needs no GPU. */
int pbrk_mc_launch_cut(const float* weights, int n, unsigned min_bits, unsigned max_bits, int* cut4);
/* the same for a launch whose workgroups own S slices of the table (S = 1, 2 or 4; slice s: words s, s + S, ..): cut[s], s < S.
 * S = 4 is pbrk_mc_launch_cut. */
int pbrk_mc_launch_cut_slices(const float* weights, int n, int S, unsigned min_bits, unsigned max_bits, int* cut);
/* the cut of the last region-kernel launch: {first cut word of slices 0 .. 3, mask words per region, words cut}; a launch of S < 4
 * slices reports slice j % S in entry j and counts the words cut over its S slices; waits for the device */
int pbrk_mc_launch_cut_stats(int* out6);
/* the region kernel's tile on the quarter-face shape with at most 64 mask words: -1 (default) 32 x 32 texels x 1 slice where the
 * level's output size reaches the measured threshold, 0 never, 1 wherever the shape allows it.  Every other level keeps 16 x 16 x 4.
 * The two tiles add a texel's samples in different orders: close, not the same bytes.  Tests and A-B runs. */
void pbrk_mc_set_tile32(int mode);
/* half_n folded into the frame rows of the region kernel's run loop (k_mc_region.hip, 2j) on levels whose edge is a power of two: one
 * multiply less per proved sample.  Default 1; bit-identical either way; every other level keeps the multiply whatever the switch
 * says.  Tests and A-B runs. */
void pbrk_mc_set_fold(int on);
/* 1 when the last region-kernel launch ran a folded instantiation, else 0 */
int pbrk_mc_last_fold(void);
/* the completeness net of the region kernel (k_mc_region.hip, step 3 and 2l): every wave counts the (texel, sample) pairs it takes and
 * recomputes its slice when the count is short.  -1 (default): on when the device counters are on (PBR_MC_STATS=1), off otherwise;
 * 0: off wherever a net-less instantiation exists (the lean run loops); 1: always on.  Bit-identical either way.  Tests and A-B runs. */
void pbrk_mc_set_net(int mode);
/* 1 when the last region-kernel launch carried the net, 0 when it ran a net-less instantiation */
int pbrk_mc_last_net(void);
/* host twin of what k_mc_cut writes for the net-less kernel's early end of a pass (k_mc_region.hip, 2l): mono4[s], s < S (S = 1, 2 or 4
 * slices; slice s owns the mask words s, s + S, ..), is the first word of slice s from which the slice's largest weights per word never
 * rise again; a slice without words gets s.  n <= 8192 weights.  Returns 0, or -1 for bad arguments.  Needs no GPU. */
int pbrk_mc_mono_slices(const float* weights, int n, int S, int* mono4);
/* levels of at most 16^2 texels with outputs of 256^2 and more, resident in LDS as a whole (k_mc_region.hip, 2k): the samples binning
 * proves for a whole tile run test-free per face, every other sample once, each lane on its own face.  1 on, 0: the kernel such a level ran
 * before, -1 (default) = the environment (PBR_MC_RESIDENT) or 1.  The two add a texel's samples in different orders: close, not the same bytes.  Tests and A-B runs. */
void pbrk_mc_set_resident(int on);
/* that kernel's counters (PBR_MC_STATS=1), since the last reset: {(lane, sample) pairs whose proof did not hold -- must stay 0 --,
 * proved samples summed over tiles, pairs taken by the proved runs, pairs taken by the general pass}.  Its tiles also enter the flag
 * and wave-slice counters; the window counter counts k_mc_region's proved samples alone. */
int pbrk_mc_resident_stats(unsigned long long* out4);
/* ---- the bin cache of the region and resident kernels (k_mc_region.hip, 2m).  What a tile's binning computes -- which regions its samples
 * can reach, which samples are proved -- depends on the tile's geometry, the level's shape and the sample table, never on a texel.  The
 * first whole-level launch (six faces, every row) of a (device, kernel shape, n_src, output size, n_entries, table) writes every tile's
 * flags to device memory; every later launch whose tiles are tiles of that dispatch copies them instead of computing them.  Same samples,
 * same order, same bytes.
 * A table pointer says nothing about its contents, so only registered tables are served: pbrk_mc_table_register declares the
 * n_entries x float4 table at table4 immutable until pbrk_mc_table_unregister (which also drops what was recorded with it).  Every
 * registration is a new generation; a launch may use a prefix of a registered table (its own entry).  Return 0, or PBRK_E_ARG. */
int pbrk_mc_table_register(const void* table4, int n_entries);
int pbrk_mc_table_unregister(const void* table4);
/* -1 (default): the environment (PBR_MC_BIN_CACHE=0|1), else on exactly when the device counters are off (the rule of pbrk_mc_set_net);
 * 0: off; 1: on, with or without the counters.  Launches being captured into a graph, region-kernel launches without a k_mc_prep slot,
 * the yardstick instantiations (pbrk_mc_set_runs(0), pbrk_mc_set_prologue(0), the 18^2 shape) and region-kernel row windows that do not
 * start on a tile row and end on one or at the face's end always compute. */
void pbrk_mc_set_bin_cache(int mode);
/* bytes the cache may hold per device (default 512 MiB).  No eviction: an entry that would pass the budget is not created. */
void pbrk_mc_set_bin_cache_budget(size_t bytes);
/* frees every entry (waits for the device); the next whole-level launch records again */
void pbrk_mc_bin_cache_clear(void);
/* since the library was loaded: {recording launches, replaying launches, launches that computed though the cache was on (a launch declined
 * for the budget among them), launches declined for the budget}, and the bytes held now */
void pbrk_mc_bin_cache_stats(unsigned long long out[5]);
/* host twin of the kernels' block -> tile map (mc_tile_of_block, k_mc_internal.h) for a dispatch of faces [face0, face0 + nfaces) and rows
 * [y0, y1) of a size^2 output with tile x tile tiles (8, 16 or 32): out4 = {face, tile column, tile row counted from the dispatch's first,
 * the tile's index in the cache: (face * tiles_per_edge + y0 / tile + row) * tiles_per_edge + column}.  Needs no GPU. */
int pbrk_mc_tile_of_block(int block, int size, int tile, int face0, int nfaces, int y0, int y1, int* out4);
/* 1 when a region-kernel dispatch of rows [y0, y1) may record or replay: y0 a multiple of the tile, y1 one or the face's end.  Needs no GPU. */
int pbrk_mc_bin_window_eligible(int size, int tile, int y0, int y1);
/* ---- exact flags in the bin cache (k_mc_region.hip, 2n).  The flags a recording launch stores are a bound: a superset of what the tile's
 * texels reach.  Behind the recording launch, ahead of the event replays wait for, k_mc_refine_bins rewrites the entry in place: a flag
 * stays exactly where some lane of the tile takes the sample, a proof bit is set exactly where all lanes take it in one region, both
 * decided by the sample bodies' own arithmetic.  The recording launch itself ran on the bound's flags; replays read the refined words
 * in the same layout.  Same samples accumulated, same order, same bytes.  k_mc_region entries only: in k_mc_resident the order of a
 * texel's sum depends on what its tile proves, so its bytes would move; its entries stay as recorded.
 * -1 (default): the environment (PBR_MC_EXACT_BINS=0|1), else on exactly when the device counters are off (the rule of pbrk_mc_set_net
 * and pbrk_mc_set_bin_cache) and only for the kernel shapes whose replaying kernel measured as a gain (today the 34^2 shape: levels of
 * 17 .. 32 texels per edge; profiles/exact_bins.md); 0: off; 1: on for every k_mc_region entry, with or without the counters. */
void pbrk_mc_set_exact_bins(int mode);
/* 1 when the last recording launch was followed by the refinement, else 0 */
int pbrk_mc_last_exact_bins(void);
/* summed over the refined entries since the last reset: {(region, sample) flags before, after; proved samples before, after; stagings the
 * tiles' words ask for (regions with a flag, head and tail words counted apart where a tile runs two phases) before, after; hits on a
 * bit the bound had not set; (lane, sample) pairs that found no region}.  The last two must stay 0: the bound is rigorous.  Waits for the
 * device.  Returns 0, PBRK_E_ARG or PBRK_E_LAUNCH. */
int pbrk_mc_exact_bins_stats(unsigned long long* out8, int reset);
/* ---- the launch plan (mc_plan.h): everything the host decides about one pbrk_mc_filter dispatch, from the level (n_src, n_tab,
 * size), the dispatch (face0, nfaces, y0, rows), the process switches as they stand (pbrk_mc_set_*, environment), whether the device
 * counters are on (PBR_MC_STATS) and whether a k_mc_prep scratch slot is to be had (0: stream capture, no device memory).  Needs no GPU. */
typedef struct PbrkMcPlan {
    int family;                     /* 0: declined (the level-in-LDS or the direct kernel runs), 1: k_mc_region, 2: k_mc_resident */
    int RS, G, RC, NR, NW;          /* staged edge, regions per face edge, cells per region edge, regions, mask words per region */
    int tile, nslices;              /* TILE x TILE output texels x nslices slices of the sample table per workgroup */
    int runs, lean, fold, net;      /* the template arguments RUNS, LEAN, FOLD, NET of k_mc_region (fold: also of k_mc_resident) */
    int absorb;                     /* absorbed words are skipped (2c) */
    int head_first;                 /* the shape runs its head words first (2g) */
    int prep, cut;                  /* k_mc_prep / k_mc_cut run ahead of the kernel */
    int stats;                      /* the counters are on: k_mc_resident's STATS */
    int bin_cache, bin_eligible;    /* the bin cache is on; this dispatch may replay (and, whole, record) its binning (2m) */
    int whole;                      /* all six faces, every row */
    int refine;                     /* if this launch records, k_mc_refine_bins follows it (2n) */
    int bin_flavour;                /* the kernel shape in the cache's key */
    int lds;                        /* dynamic LDS bytes of the kernel */
    int lds_slices, direct_slices;  /* declined: k_mc_filter_lds<lds_slices> runs, or with lds_slices == 0 k_mc_filter<direct_slices, ..> */
    int expect[16];                 /* k_mc_region: samples per slice */
} PbrkMcPlan;
int pbrk_mc_plan(int n_src, int n_tab, int size, int face0, int nfaces, int y0, int rows, int counters, int have_prep, PbrkMcPlan* out);

/* ---- K5: deferred shade pass (shaders/lighting_pass.glsl:432-716, in-scope sub-blocks). */
typedef struct PbrkShadeArgs {
    int width, height;
    int x0, x1, y0, y1;                 /* pixel rectangle to shade */
    const void* base_color;             /* uchar4 [H][W] */
    const void* normal;
    const void* orm;
    const void* emissive;
    const void* depth;                  /* float [H][W] */
    const void* irradiance_bordered;    /* bordered level, size irradiance_size (IBL mode) */
    int irradiance_size;
    const void* prefiltered_bordered;   /* bordered pyramid of the prefiltered cube */
    int prefiltered_size, prefiltered_levels;
    const void* lut;                    /* half2 [S][S] */
    int lut_size;
    /* optional gather-saving twins (NULL = not available): cells of the irradiance level; cells of the prefiltered
     * levels >= prefiltered_cells_first (back to back, pbrk_cells_bytes each); 2x2-footprint cells of the LUT */
    const void* irradiance_cells;
    const void* prefiltered_cells;
    int prefiltered_cells_first;
    const void* lut_cells;              /* uint4 [(S+1)][(S+1)]: {t00,t10,t01,t11} half2, tap origin (-1,-1), clamp-to-edge */
    const void* sun_depth;              /* float [sun_depth_h][sun_depth_w] (SUN_DEPTH_MAP, render.cpp:676); PBRK_SHADE_SHADOWS */
    int sun_depth_w, sun_depth_h;
    const void* lightgrid;              /* half4 [n][n][n] (LIGHTGRID, render.cpp:678, after the sweeps); PBRK_SHADE_GI */
    int lightgrid_size;
    const void* prev_frame[8];          /* PREV_FRAME_RESULT mip chain, half4 per level (the reference binds bloom_downscale_rt, render.cpp:862) */
    int prev_frame_w, prev_frame_h;     /* level 0 extent; level l is max(1, w >> l) x max(1, h >> l) */
    int prev_frame_levels;              /* 1..8 */
    void* out;                          /* half4 or float4 [H][W] */
    int out_format;                     /* PBRK_FMT_RGBA16F / PBRK_FMT_RGBA32F */
    int flags;                          /* PBRK_SHADE_* */
    float globals[138];                 /* RendererGlobalsBuffer, render.h:122-136 (552 bytes) */
    const double* sh9_coef;             /* PBRK_SHADE_SH9: 27 doubles on the device (index 3 k + c as pbrk_sh9_project writes them), 8-byte
                                           aligned; read by the kernel when it runs, not by pbrk_shade */
} PbrkShadeArgs;
int pbrk_shade(const PbrkShadeArgs* args, void* stream);
/* K5 has two instantiations: the general kernel k_shade (every mode; with PBRK_SHADE_GI k_shade<true>) and k_shade_fast (64 x 4
 * pixel workgroups, every tap through range-checked buffer loads of the cells twins; the default for the modes without sun
 * shadows / voxel GI when the twins exist).  Both agree with the oracle at the same tolerance; they are not bit-identical. */
void pbrk_shade_set_fast(int on);                        /* 0: every mode through the general kernel k_shade (env PBR_SHADE_FAST); -1 = default */
int  pbrk_shade_last_kernel(void);                       /* instantiation of the most recent successful pbrk_shade: 0 general, 1 fast, 2 GI (-1: none yet) */
/* LUT twin for K5: one 16-byte load per bilinear LUT fetch */
int pbrk_lut_cells_build(const void* lut_half2, int size, void* cells_out, void* stream);

/* ---- K16: the light-grid visualiser of the lighting pass (lighting_pass.glsl:463-491, Globals.visualize_lightgrid != 0): every pixel of
 *      the rectangle, sky included, becomes a ray march through LIGHTGRID (up to 512 half-voxel steps, first trilinear sample with
 *      alpha > 0.3, luminance remapped by its square root).  Reads nothing else of the lighting pass's inputs.  Contract:
 *      csrc/gridview_core.h; bit-identical to a CPU evaluation of that header. ---- */
typedef struct PbrkGridViewArgs {
    int x0, x1, y0, y1;                 /* pixel rectangle to write */
    int width, height;                  /* of the target; fs_uv = (pixel + 0.5) / extent */
    const void* lightgrid;              /* half4 [n][n][n] */
    int lightgrid_size;                 /* n, 1..1024 */
    void* out;                          /* half4 or float4 [H][W] */
    int out_format;                     /* PBRK_FMT_RGBA16F / PBRK_FMT_RGBA32F */
    float globals[138];                 /* RendererGlobalsBuffer (552 bytes); read: world_space_from_clip, camera_pos, frame_idx_mod_59, lightgrid_scale */
} PbrkGridViewArgs;
int pbrk_lightgrid_view(const PbrkGridViewArgs* args, void* stream);

/* ---- K8 / K9: post-process tail.  2-D sampler = linear clamp with coordinates snapped to 1/256
 *      texel (Vulkan subTexelPrecisionBits = 8), exact fp32 lerps. ---- */
typedef struct PbrkTex2D { const void* data; int format, width, height; } PbrkTex2D;     /* device pointer, PBRK_FMT_* */

/* K8: shaders/taa_resolve.glsl:180-287 (3x3 Mitchell-Netravali resolve, variance clamp of the Catmull-Rom-filtered
 * history, velocity / off-screen rejection).  All inputs and the target have the frame's size. */
typedef struct PbrkTaaArgs {
    PbrkTex2D lighting_result;          /* RGBA16F */
    PbrkTex2D gbuffer_depth;            /* R32F */
    PbrkTex2D gbuffer_velocity;         /* RG16F */
    PbrkTex2D gbuffer_velocity_prev;    /* RG16F */
    PbrkTex2D prev_frame_result;        /* RGBA16F */
    void* out;                          /* half4 or float4 [height][width] */
    int out_format;                     /* PBRK_FMT_RGBA16F / PBRK_FMT_RGBA32F */
    int width, height, y0, y1;          /* rows [y0,y1) */
} PbrkTaaArgs;
int pbrk_taa_resolve(const PbrkTaaArgs* args, void* stream);

/* K9: shaders/final_post_process.glsl:2-10,31-34: pow(aces_approx(2 * src), 1/2.2), alpha 1.  src may have another
 * size than the target (bilinear); 8-bit targets round to nearest even. */
typedef struct PbrkFinalArgs {
    PbrkTex2D src;                      /* RGBA16F (bloom / TAA result) */
    void* out;
    int out_format;                     /* PBRK_FMT_RGBA8UN / BGRA8UN / RGBA16F / RGBA32F */
    int width, height, y0, y1;
} PbrkFinalArgs;
int pbrk_final_post_process(const PbrkFinalArgs* args, void* stream);

/* K10 / K11: one pass of the bloom chain (render.cpp:1139-1176): bloom_downsample.glsl:38-98 (13 bilinear taps; firefly
 * clamp when dst_mip_level == 1) or bloom_upsample.glsl:23-58 (3x3 tent at radius 1.5 source texels; x0.06 when
 * dst_mip_level == 0) from `src` into an RGBA16F target of dst_width x dst_height.  blend_additive: target = fp16(colour +
 * target) with alpha = 1 (VK_BLEND_FACTOR_ONE / ONE, alpha ONE / ZERO; gpu_vulkan.c:1828-1842). */
typedef struct PbrkBloomArgs {
    PbrkTex2D src;                      /* RGBA16F (a mip of a texture: data points at the level, width/height are the level's) */
    void* dst;                          /* half4 [dst_height][dst_width] */
    int dst_width, dst_height;
    int dst_mip_level;                  /* the shader's push constant */
    int upsample;                       /* 0: bloom_downsample.glsl, 1: bloom_upsample.glsl */
    int blend_additive;
    int y0, y1;
    const void* blend_src;              /* blend_additive: the operand added to the pass's result, same layout as dst; NULL = dst itself */
} PbrkBloomArgs;
int pbrk_bloom_pass(const PbrkBloomArgs* args, void* stream);
/* The three instantiations of a bloom pass give the same bits: one pixel per thread; two (downsample) or 2 x 2 (upsample) pixels per thread
 * (exact 2 : 1 passes with even sizes and at least quad_min_pixels target pixels; default 100000, env PBR_BLOOM_QUAD_MIN_PIXELS); four lanes per pixel (general-sampler
 * passes of at most small_max_pixels target pixels; default 40000, env PBR_BLOOM_SMALL_MAX_PIXELS).  Negative = default. */
void pbrk_bloom_set_thresholds(long long quad_min_pixels, long long small_max_pixels);

/* ---- K12 (N5): the sun depth pass (sun_depth_pass.glsl: gl_Position = sun_space_from_world * vec4(p, 1), no fragment output, LESS
 *      depth test + write into a D32F target) as a compute rasteriser.  The draws of one render-pass instance are one job: draw d
 *      covers job triangles [first_tri, next draw's first_tri) and reads indices first_index + 3 t' + k (32-bit) of the index buffer,
 *      vertex = index + vertex_offset.  Contract (coverage, tie rule, depth arithmetic, guard band): DESIGN.md K12.
 *      Setup (one thread per triangle: transform, snap, reject, bin into 32 x 32-pixel tiles) then one workgroup per tile keeping the
 *      per-pixel minimum in registers; no global atomics on the depth map, no read-back.  `scratch` holds pbrk_raster_scratch_bytes;
 *      `draws` is device memory (PbrkRasterDraw[draw_count], first_tri ascending, every draw at least one triangle). ---- */
typedef struct PbrkRasterDraw {
    float m[16];                  /* sun_space_from_world, column-major, as snapshotted at submit */
    uint32_t first_tri, first_index, vertex_offset, pad;
} PbrkRasterDraw;
typedef struct PbrkRasterArgs {
    const void* vertices;         /* position = first 3 floats of each vertex */
    uint32_t vertex_stride;       /* bytes, multiple of 4 */
    uint32_t vertex_count;        /* vertices in the bound buffer: a larger vertex index skips its triangle (counted) */
    const uint32_t* indices;
    const PbrkRasterDraw* draws;
    uint32_t draw_count, tri_count;
    float* depth;                 /* width x height fp32, tight rows */
    int width, height;            /* at most 16384 each */
    void* scratch;
    unsigned long long* rejected; /* device counter: += triangles skipped for an index, a non-finite value or the guard band */
} PbrkRasterArgs;
size_t pbrk_raster_scratch_bytes(uint32_t tri_count, int width, int height);
int pbrk_raster_setup(const PbrkRasterArgs* args, void* stream);    /* K12.setup: clear bins, transform + bin, scan, fill */
int pbrk_raster_tiles(const PbrkRasterArgs* args, void* stream);    /* K12.tiles: per-tile depth minimum, one store per pixel */

/* ---- K13: the geometry pass (geometry_pass.glsl, render.cpp:1076-1115) as a compute rasteriser on K12's structure: setup (one
 *      thread per triangle: vertex stage, clip, fan, snap, bin), then one workgroup per 32 x 32 tile (a 2 x 2 quad per lane) that
 *      first finds each pixel's winner (depth, then triangle number; the alpha test before the depth write) and then shades it once.
 *      Contract: DESIGN.md K13.  Vertices are the 44-B Vertex of render.h:31-36; every draw names its own buffers and textures. ---- */
typedef struct PbrkGeoTex { const void* texels; int width, height, levels, pad; } PbrkGeoTex;    /* RGBA8UN, levels back to back */
typedef struct PbrkGeoDraw {
    float m[16], m_old[16];       /* clip_space_from_world, old_clip_space_from_world: column-major, as snapshotted at submit */
    float jitter[2], jitter_prev[2];
    PbrkGeoTex tex[4];            /* TEX0 (base colour), TEX1 (normal), TEX_ORM, TEX_EMISSIVE */
    const void* vertices; const uint32_t* indices;
    uint32_t vertex_count, first_tri, first_index, vertex_offset;
} PbrkGeoDraw;
typedef struct PbrkGeometryArgs {
    const PbrkGeoDraw* draws;     /* device memory, first_tri ascending, every draw at least one triangle */
    uint32_t draw_count, tri_count;
    void* color[4];               /* base colour, normal, ORM, emissive: RGBA8UN, width x height, tight rows */
    void* velocity;               /* RG16F */
    float* depth;                 /* D32F */
    int width, height;            /* at most 16384 each */
    void* scratch;
    unsigned long long* rejected;
} PbrkGeometryArgs;
size_t pbrk_geometry_scratch_bytes(uint32_t tri_count, int width, int height);
int pbrk_geometry_setup(const PbrkGeometryArgs* args, void* stream);
int pbrk_geometry_tiles(const PbrkGeometryArgs* args, void* stream);
/* mip chain of a 2-D RGBA8UN texture with power-of-two extents (levels back to back): each level is the 2 x 2 box of the one above,
 * averaged in fp32 on the decoded values, stored as rint(255 x) */
int pbrk_mip_chain_rgba8(void* pyramid, int width, int height, int levels, void* stream);

/* ---- K14: the voxelise pass (lightgrid_voxelize.glsl, render.cpp:1039-1056) as a compute rasteriser: conservative coverage of an
 *      N x N target, one store per fragment into the N^3 RGBA16F light grid; among the fragments of one voxel the largest
 *      (triangle number, pixel row, pixel column) wins.  Contract: DESIGN.md K14.  Setup (one lane per triangle: vertex stage, snap,
 *      conservative box walk, a 64-bit atomicMax of the fragment's key into an N^3 owner grid in `scratch`; triangles with a large
 *      box go to a list that one workgroup per triangle covers), then resolve (one lane per owned voxel shades its winner and
 *      stores 8 bytes).  Vertices and indices are the raw SSBO0 / SSBO1 of the draw's descriptor set. ---- */
typedef struct PbrkVoxDraw {
    float sun[16];                /* sun_space_from_world, column-major, as snapshotted at submit */
    float sun_dir[4];             /* sun_direction */
    float scale;                  /* lightgrid_scale */
    uint32_t first_tri, first_vertex, pad;
    const float* vertices; unsigned long long vertex_floats;      /* SSBO0 and its length in floats: a read past it is checked */
    const uint32_t* indices;                                      /* SSBO1: [first_vertex, first_vertex + 3 x triangles) is in range */
    const float* sun_depth; int sun_w, sun_h;                     /* SUN_DEPTH_MAP */
    PbrkGeoTex tex[2];            /* TEX0 (base colour), TEX_EMISSIVE */
} PbrkVoxDraw;
typedef struct PbrkVoxelizeArgs {
    const PbrkVoxDraw* draws;     /* device memory, first_tri ascending, every draw at least one triangle */
    uint32_t draw_count, tri_count;
    void* grid;                   /* RGBA16F [n][n][n], updated in place */
    int n;                        /* multiple of 8, 8 .. 256 */
    void* scratch;
    unsigned long long* rejected;
    unsigned long long* fragments;    /* device counter (may be NULL): += fragments kept, i.e. stores the shader would have issued */
} PbrkVoxelizeArgs;
size_t pbrk_voxelize_scratch_bytes(uint32_t tri_count, int n, int n_again);   /* n_again: ignored (the raster jobs' common signature) */
int pbrk_voxelize_cover(const PbrkVoxelizeArgs* args, void* stream);    /* K14.cover: clear the owner grid, setup + small boxes, large boxes */
int pbrk_voxelize_resolve(const PbrkVoxelizeArgs* args, void* stream);  /* K14.resolve */

/* ---- K15: block-compressed material textures (the .dds files of asset_import.cpp:30-60).  One level of BC1 / BC3 / BC5 blocks
 *      (ceil(width / 4) x ceil(height / 4), row major, 8 or 16 bytes each; 8- resp. 16-byte aligned) -> width x height RGBA8UN, tight
 *      rows (4-byte aligned), texels outside the level dropped.  Any extent from 1 to 16384.  Contract (bit replication, truncating
 *      division, BC5 = (R, G, 0, 255)): csrc/bc_core.h, DESIGN.md K15. ---- */
enum { PBRK_BC1_RGB = 0, PBRK_BC1_RGBA = 1, PBRK_BC3 = 2, PBRK_BC5 = 3 };
int pbrk_bc_decode(int format, const void* blocks, int width, int height, void* rgba8, void* stream);

/* ---- K17: the nine-coefficient spherical-harmonic (SH9) form of the environment's diffuse lighting (the reference
 *      has none).  Contract -- directions, exact texel solid angles, basis order, the E / (2 pi) normalisation of
 *      gen_irradiance_map.glsl:84-97, no clamp: csrc/sh_core.h, DESIGN.md K17.  n and size: any value from 1 to 16384.
 *      project: rows [y0, y1) of faces [face0, face1) of one level -> double[27] (index 3 k + c), a partial sum that callers add
 *      themselves; two launches (one 27-double partial per workgroup into `scratch`, then one workgroup adds them in index order),
 *      no floating-point atomics: equal arguments give equal bytes.  scratch: pbrk_sh9_scratch_bytes(n) bytes, 8-byte aligned.
 *      irradiance: the same sub-range of a size^2 level from 27 device doubles, alpha 0.  Nothing is read back. ---- */
size_t pbrk_sh9_scratch_bytes(int n);
int pbrk_sh9_project(const void* level /* float4 [6][n][n] */, int n, int face0, int face1, int y0, int y1,
                     void* scratch, double* out27_device, void* stream);
int pbrk_sh9_irradiance(const double* coef27_device, void* out_level /* float4 [6][size][size] */, int size,
                        int face0, int face1, int y0, int y1, void* stream);

/* ---- K18: BC6H_UF16 encode of one level (the output side of the bake, host/pbr_ddsout.c).  `layers` images of
 *      width x height RGBA32F (16-byte aligned) or RGBA16F (8-byte aligned) texels, tight, layer after layer -> ceil(width / 4) x
 *      ceil(height / 4) blocks of 16 bytes per layer, row major within a layer, layer after layer (16-byte aligned).  Mode 11 only;
 *      texels past the edge of the level repeat the last row / column.  Any extent from 1 to 16384, 1 to 65535 layers; another source
 *      format is PBRK_E_FORMAT.  Contract (half codes, candidates, index and anchor rules, integer only): csrc/bc6h_core.h, DESIGN.md K18. ---- */
uint64_t pbrk_bc6h_level_bytes(int width, int height, int layers);      /* 0 for a non-positive argument */
int pbrk_bc6h_encode(const void* level, int src_format /* PBRK_FMT_RGBA32F / PBRK_FMT_RGBA16F */, int width, int height, int layers,
                     void* blocks_out, void* stream);
/* the two-region quality level: the same arguments, checks, error codes and layout; per block mode 11 or one of the two-region cases
 * 0, 14, 1, 30, whichever has the lower squared half-code error (mode 11 on a tie).  Contract: csrc/bc6h2_core.h. */
int pbrk_bc6h_encode2(const void* level, int src_format /* PBRK_FMT_RGBA32F / PBRK_FMT_RGBA16F */, int width, int height, int layers,
                      void* blocks_out, void* stream);

/* ---- K19: BC6H_UF16 decode of one level, all 14 modes (the input side, host/pbr_ddsin.c).  `layers` images of
 *      ceil(width / 4) x ceil(height / 4) blocks, laid out as pbrk_bc6h_encode writes them (16-byte aligned) -> width x height RGBA32F
 *      (16-byte aligned) or RGBA16F (8-byte aligned) texels, tight, layer after layer.  RGBA16F gets the half codes 0 .. 0x7BFF as they
 *      are, RGBA32F their exact widening (subnormal halves included, done in integers); alpha is 1.0; texels of a block outside the level
 *      are dropped; a block of a reserved mode gives zeros.  Any extent from 1 to 16384, 1 to 65535 layers; another target format is
 *      PBRK_E_FORMAT, anything else PBRK_E_ARG, with nothing launched.  Contract (integer only): csrc/bc6h_decode_core.h, DESIGN.md K19. ---- */
int pbrk_bc6h_decode(const void* blocks, int width, int height, int layers, void* level_out,
                     int dst_format /* PBRK_FMT_RGBA32F / PBRK_FMT_RGBA16F */, void* stream);

/* ---- K20: one level of an RGBA32F cube -> a w x h lat-long panorama (the inverse of K6).  bordered_level: the n^2
 *      level inside the bordered twin ([6][n+2][n+2] float4, pbrk_border_build).  table: device double[2 w + 2 h] as pano_fill_table
 *      (csrc/panorama_core.h) writes it -- {cos phi, sin phi} per column, then {sin theta, cos theta} per row.  out: w x h RGBA32F
 *      (16-byte aligned) or RGBA16F (8-byte aligned) texels, tight rows; fp16 by v_cvt_f16_f32 (round to nearest even).  n, w and h:
 *      any value from 1 to 16384.  Another target format is PBRK_E_FORMAT, anything else PBRK_E_ARG, with nothing launched.
 *      Contract: csrc/panorama_core.h, DESIGN.md K20. ---- */
int pbrk_cube_to_panorama(const void* bordered_level, int n, const void* table, void* out,
                          int out_format /* PBRK_FMT_RGBA32F / PBRK_FMT_RGBA16F */, int w, int h, void* stream);

/* ---- K21: faces [face0, face1) x rows [y0, y1) of one out_size^2 level of the specular cube by GGX importance sampling with filtered
 *      lookups.  src_bordered: the bordered twin of the whole source cube, level 0 first (pbrk_border_build; the
 *      levels the table names must hold their apron).  table: device uint4[2 * kept], per kept sample {l.x, l.y, l.z, f} as fp32 bits
 *      and {pbrk_bordered_level_offset and size of level l0, the same of level l1}, f the blend towards l1; wsum: the fp32 sum of
 *      the l.z.  out: the whole level, [6][out_size][out_size] RGBA32F; alpha 1; texels outside the range are not touched.  A
 *      texel's bytes do not depend on the range.  kept 0 .. 4096 (0: 0 / 0), out_size 1 .. 16384; anything else is PBRK_E_ARG with
 *      nothing launched.  Contract: csrc/prefilter_ggx_core.h, DESIGN.md K21. ---- */
int pbrk_prefilter_ggx(const void* src_bordered, const void* table, int kept, float wsum, void* out, int out_size,
                       int face0, int face1, int y0, int y1, void* stream);

/* ---- K22: rows [y0, y1) of a w x h split-sum BRDF LUT by GGX importance sampling: texel (x, y) is (A, B) at
 *      N.V = (x + .5) / w and roughness (y + .5) / h, RGBA32F stores (A, B, 0, 1).  table: device float[3 * nsamples], {xi1, cos phi,
 *      sin phi} per sample (GPUX_BrdfLutGGXSamples).  visibility: 0 Smith-Schlick with k = a / 2, 1 height-correlated Smith.  Texels
 *      outside the rows are not touched; a texel's bytes do not depend on the rows.  w, h 1 .. 4096, nsamples 1 .. 4096; anything else
 *      is PBRK_E_ARG / PBRK_E_FORMAT with nothing launched.  Contract: csrc/brdf_lut_ggx_core.h, DESIGN.md K22. ---- */
int pbrk_brdf_lut_ggx(void* out, int out_format /* PBRK_FMT_RG16F / RG32F / RGBA32F */, int w, int h, int nsamples, int visibility,
                      const void* table, int y0, int y1, void* stream);

/* ---- diagnostics: the device samplers of the widened passes evaluated at caller-supplied coordinates, so that tests can feed them
 *      NaN / inf / 1e30 / boundary values directly (a ray that has marched far away must never become an out-of-bounds read).
 *      which: 0 = LIGHTGRID (RGBA16F n^3, coords xyz), 1 = sampler2DShadow (R32F w x h, coords u, v, ref; result in out[0]),
 *      2 = the post-process 2-D sampler (RGBA16F w x h, coords u, v), 3 = LIGHTGRID as K16 reads it (alpha and colour fetched
 *      separately; the same bits as 0).  coords: device float[count][3]; out: device float[count][4]. */
int pbrk_debug_sample(int which, const void* texture, int w, int h, int d, const void* coords, int count, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
