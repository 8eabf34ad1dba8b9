// k_mc_region.hip -- K4b / K3 for source levels too big for LDS as a whole: taps served from LDS-staged REGIONS.
// The device code of k_mc_region, k_mc_refine_bins and k_mc_resident and their thin launchers.  Which kernel serves a level: mc_plan.cpp;
// k_mc_prep, k_mc_cut and their scratch ring: k_mc_prep.hip; the bin cache's host side: mc_bins.cpp.
//
// Same sum as k_mc.hip (gen_prefiltered_env_map.glsl:115-146, gen_irradiance_map.glsl:81-97):
//   out.rgb(texel) = ( sum_i w_i * bilinear(src, frame(texel) * l_i) ) / divisor
//
// Why: the direct kernel moves 48 B per (texel, sample) through the vector L1 (64 B/clk/CU): 48 clk per wave-sample per
// CU whatever the hit rate, above its ~40 clk of VALU work.  LDS delivers 256 B/clk/CU, but only levels up to 32^2 fit as a
// whole.  Here the bordered source level is cut into regions of at most 66 x 66 texels (70 KB: a whole face at n = 64, a
// quarter face at n = 128), and a 1024-thread workgroup (16 x 16 output texels x 4 slices of the sample table, two workgroups
// per CU) walks the regions one after the other:
//   1. binning (once per tile): every sample direction is pushed through the tile-centre frame; a rigorous bound on how far
//      any texel of the tile can move it (|M_texel - M_centre|_F) yields the regions it can reach; one bit per (region,
//      sample) in LDS.  ~1 % of the work.
//   2. per flagged region: stage it in LDS, then every wave runs the flagged samples of its slice.  The face is known per
//      pass, so the cube projection is a static signed permutation folded into the frame (no v_cube*), each lane tests
//      exactly whether ITS direction falls into this region's cells (the hardware's tie rule: z >= y >= x), and lanes that
//      do not are masked (weight 0): they meet the sample again in the pass of their own region.
//   3. every wave counts the (lane, sample) pairs it has accumulated (scalar popcount of the exec mask).  A total short of
//      64 x the slice's sample count would mean the bound of step 1 missed a region; the wave then recomputes its slice with
//      direct loads (never observed; counter in stats[0]).
//   2b. (round 3, quarter-face levels) binning also PROVES, for 94 % of the samples, that every texel of the tile taps the SAME
//      region of the same face (the bound of step 1 read as "certainly" instead of "possibly"): those run a body without the
//      in-face / in-region tests, their six ballots, the exec masking and the pair count -- 37 instead of 45 instructions.
//      Measured (one box, A/B): C4 mip 1 36.7 -> 35.1 ms.  The same on the whole-face levels (39 -> 37 instructions) LOSES
//      3-5 % -- the wave-uniform choice of body per sample costs more than two comparisons -- so the round-3 pass compiles it for
//      SUB only (2i: the run loop of 2d has no such choice); two separate loops (proved samples, then the rest) were slower on every
//      level.
//   2c. (round 4, absorbed words) a mask word whose samples provably cannot change any lane's fp32 sums is not accumulated
//      (the lemma at absorb_threshold); its samples only run the count-only body, so the check of step 3 still sees every pair.
//      Compiled for the 66^2 region shapes only (ABS).
//   2d. (round 5, 66^2 shapes, RUNS) less scalar work per sample: only non-empty words, runs of proved samples without a per-sample
//      test, counts per lane (one ballot chain), a barrier per visited region only (region_pass_runs; C4 72.2 -> 66.2 ms, same bytes).
//   2e. (round 6, visiting order) a tile visits the regions of its OWN face first, then all the others in index order
//      (mc_region_visit, k_mc_internal.h).  The own face holds a texel's big terms (small angles, large weights); met first, they
//      make the sums every later word is tested against in 2c, so the neighbours' tail words are absorbed on every face and not
//      only on the faces whose index happens to be the lowest (C4 mip 2: 0.439 -> 0.478 of the wave-samples absorbed, the six
//      faces 0.47-0.49 instead of 0.40-0.47; profiles/r06_order.md).
//      Taken by the 66^2 shapes, where words are absorbed; the 34^2 / 18^2 shapes keep index order (OWN_FIRST in k_mc_region).
//   2f. (round 7, prologue, LEAN) work every tile repeated for a result that is the same for the whole launch, and arithmetic the flags
//      do not need.  (i) The two maxima of the absorbed-word test (2c) -- per mask word the largest weight, per region the largest staged
//      R, G, B -- come from k_mc_prep, launched once on the same stream ahead of the region kernel, and are read with scalar loads; the
//      per-sample LDS atomic of binning and the per-staging max / butterfly / atomic are gone, with their LDS arrays' clearing.  (ii) Binning
//      knows G and RC at compile time (one region per face: r = f, no division; quarter faces: RC = 65) and takes the hardware
//      reciprocal and square root inside the slack its bound already carries (region_bin).  (iii) The 66^2 shapes stage by rows -- a wave
//      per row, a lane per column, all of a thread's loads ahead of its first LDS write.  The 34^2 / 18^2 shapes keep their staging (two
//      sweeps with a constant divisor: under 1 % of their kernels).  Flags may differ from the earlier prologue's by the rounding of (ii);
//      the samples accumulated, their order and the absorb decisions do not: same bytes (pbrk_mc_set_prologue(0) keeps the earlier
//      prologue as the yardstick, tests/test_gpu_mc_prologue.py).
//   2g. (round 8, head words first; the launch-level cut) slice s of the sample table owns the mask words s, s + 4, ..: word s is its
//      head, the others its tail.  A tile runs the head words over every region flagged for them (visiting order of 2e), then the
//      tail words the same way; any[r] carries one flag per phase and a region is staged for a phase only when that phase has a
//      sample in it.  After the head phase every lane holds all 32 head samples of its slice, whichever regions they fell in, so its
//      sums are at least H_s m (1 - 2^-12) -- H_s the head word's weights added up, m the smallest R, G, B of the bordered level --
//      for EVERY lane of EVERY tile of the launch.  That turns "beyond sample ~450 nothing can change any sum", which every tile of
//      C4 mip 1 rediscovered word by word (2c: a threshold test per word and region, count-only bodies for the unproved samples,
//      binning and mask words for all 1389 samples), into one inequality per word and launch (mc_launch_cut, k_mc_internal.h):
//      k_mc_cut, one wave behind k_mc_prep, writes the first cut word of each slice behind the maxima.  The kernel does not bin the
//      samples of cut words (a thread's samples all belong to one slice: its loop simply ends earlier), so they hold no mask bit, flag
//      no region and are never visited; the slice's expected count is formed in the kernel by crediting them up front.  Dropping
//      them is exact -- every FMA of theirs would have returned its sum unchanged -- so a launch without a k_mc_prep result
//      (pbrk_mc_set_prologue(0), pbrk_mc_set_absorb(0), stream capture, no free ring slot, pbrk_mc_set_launch_cut(0)) just keeps them:
//      same bytes.  The words that remain keep the per-word test of 2c.  Under PBR_MC_STATS the cut samples still run through the flag
//      computation and are counted as absorbed (stats[2], [6], [7]: the counters keep their meaning), then their bits are cleared.
//      Tables of at most 128 samples have no tail: one phase.  Per shape (MC_HEAD_FIRST_SUB / MC_HEAD_FIRST_G1; DESIGN.md 4, "K4b,
//      round 8"); the 34^2 / 18^2 shapes keep their order and bytes.
//   2h. (round 9, 32 x 32 tiles x 1 slice on the quarter-face shape) after 2b-2g a tile of C4 mip 1 keeps 512 of 1389 samples and
//      accumulates about a fifth of the wave-samples flagged for it, but still pays a whole prologue -- binning, 3.6 stagings of 70 KB
//      (most of them twice: head and tail phase), the barriers, the four-slice tree -- for 256 texels: about half of its clocks do not
//      depend on the texels it holds.  TILE = 32 shares that prologue between 1024 texels: one slice (REG_S = 1024 / TILE^2 = 1), sixteen
//      waves in a 4 x 4 grid of 8 x 8 quadrants, word 0 the head and every other word the tail, one accumulator per texel (so a lane's
//      sums are those of the whole table: the per-word test of 2c passes two bits earlier, and the launch cut, mc_launch_cut_s with
//      S = 1, weighs the heaviest head word H_0 against the whole table).  The wider tile spreads its frames further: more samples are
//      flagged for two regions and fewer are proved (2b).  A texel's sum is added in one chain instead of four partial ones: close to
//      the 16 x 16 x 4 bytes, not equal.  One ballot of region_pass_runs covers 64 words here, so the tile serves tables of at most
//      2048 samples.  Which levels take it is mc_tile32's rule (mc_plan.cpp; level shape and output size only; pbrk_mc_set_tile32; MC_TILE32_SUB);
//      every other level keeps 16 x 16 x 4 and its bytes.  DESIGN.md 4, "K4b, round 9"; profiles/r09_tile32.md.
//   2i. (round 10, proved runs on the whole-face shapes) the run loop of 2d walks the proved samples below the next tested one as a
//      tight loop found with bit operations per run, so the proof of 2b costs no choice per sample.  It was only ever compiled for
//      SUB; CERT now holds under RUNS on the whole-face shapes too: the 66^2 one (MC_CERT_G1; both LEAN values) and the 34^2 one, which
//      gets the RUNS instantiation for it (no absorb test, index order, one phase as before; counts per lane).  A proved sample runs
//      37 VALU instructions instead of 40 and no exec join.  The samples accumulated, their order and arithmetic do not change: same
//      bytes; pbrk_mc_set_runs(0) keeps region_pass with CERT = SUB as the yardstick.  The proof is read per SAMPLE by every pass
//      (cmask has no region index), so it must hold for exactly one flagged region: on these shapes binning sets the bit only when
//      one face alone is flagged (region_bin, SOLE) -- in C4 mip 2 one (tile, sample) pair of 2e8 met the two rounded inequalities
//      within an ulp, was proved on +X and flagged on +Y, and the +Y pass credited it again (four wave-slices recomputed by step 3).
//      The quarter-face shape keeps its binning (one region per sample there as well, and the same ulp could meet it; not seen, and step
//      3 catches it).  Measured (profiles/r10_certain_g1.md): C4 mip 2 24.45 -> 23.65 ms, mip 3 11.67 -> 11.09 ms, the job 50.2 -> 48.9 ms.
//      The 18^2 shape (mip 4) LOSES with the run loop (3.71 -> 4.11 ms: 78 % proved, runs of three or four samples): it keeps the
//      round-3 pass and has no RUNS instantiation.  A table of more than 64 words per slice would take the round-3 pass (mc_plan).
//   2j. (round 11, half_n folded into the frame rows; FOLD) a sample body forms (sc, tc, ma) = Pframe e, h = rcp(ma) half_n and the tap
//      coordinates u = fma(sc, h, off), v = fma(tc, h, off).  Lemma: when half_n = 2^k (n_src a power of two), multiplying the six
//      entries of the sc and tc rows of Pframe by half_n, once per (region, pass), gives sc' = 2^k sc and tc' = 2^k tc bit for bit --
//      every product and every FMA of to_face's chain is the earlier one times 2^k, and rounding to nearest commutes with a power of
//      two -- and fma(sc', rcp(ma), off) rounds the same exact number as fma(sc, rcp(ma) 2^k, off): the same u, v, taps, weights and
//      sums.  The proved body (certain_sample) loses its multiply: 36 VALU instead of 37.  The tested body (lane_sample) compares the
//      scaled coordinates with ma_s = ma half_n (exact): ma_s > |sc'| is ma > |sc|, so the in-face decisions, and with them the
//      partition of the directions among the faces, stay; its multiply has only moved (44 / 40 VALU as before).  Condition: no
//      non-zero intermediate is subnormal and nothing overflows.  The rows are components of unit vectors and the table entries
//      components of unit directions, each 0 or at least ~1e-8 in magnitude, so no non-zero product comes near 2^-126, and 2^k <= 512
//      is far from overflow.  A violation could change at most a term of subnormal size in sc or tc, which no comparison and no
//      tap can see: it is far below half an ulp of any sum it enters.  When n_src is NO power of two the scaled rows are rounded,
//      sc' is no longer half_n sc, and two neighbouring faces would compare differently rounded copies of what are today the same
//      three numbers, permuted: their in-face tests would stop being one partition of the directions, and step 3 would heal
//      wave-slices.  Such levels keep the multiply: the fold is a compile-time flag of k_mc_region, instantiated for the four lean run
//      loops (RUNS and LEAN: <66, true, 32>, <66, true, 16>, <66, false, 16>, <34, false, 16>) and chosen by the host from n_src alone
//      (mc_plan: a row shard equals the full dispatch), under pbrk_mc_set_fold (default 1; pbrk_mc_last_fold tells what the last
//      launch took).  FOLD = false is the machine code the instantiation had before.  heal_slice, binning and the direct kernel
//      are untouched; the 18^2 shape has no proved body and no folded instantiation.  Measured (profiles/r11_fold.md): C4 mip 2 falls
//      by 0.2 ms, mip 3 by 0.13, mip 1 by 0.05, the job by 0.4 ms (48.94 -> 48.53), in four sessions: under the 0.5 ms the round asked of a gain.
//      Taking consecutive proved samples two at a time (one 32-byte scalar fetch, no bit search per sample) was built on top, LOST
//      11-14 % on every shape and is not in the library: 5.5 SALU per sample instead of 9, but the LDS reads of a tap waited three times.
//      That pointed at the waits: the four empty asm statements of tap_accumulate are four uses, and the compiler waits ahead of each
//      use -- on the 66^2 shapes the reads go out two and two.  The folded instantiation of the 66^2 whole-face shape keeps the four
//      texels alive with ONE statement (JOIN, MC_TAP_JOIN_G1): all four reads fly, one wait; same instructions and arithmetic.  Mip 2
//      23.75 -> 22.99 ms, the job 48.94 -> 47.92 ms; the 34^2 shape (its loop already waits once) and the 18^2 shape lose with it, the
//      quarter-face shape gains nothing: they keep the four statements.
//   2k. (levels of at most 16^2 texels stay resident; k_mc_resident) the 18^2 shape staged one face at a time -- six barriers, a sample met
//      once per flagged face (1.246 faces per sample on C4 mip 4), every visit the tested body with its two ballots, since only 78.5 % of the
//      samples are proved and the run loop of 2i, cut into runs of three or four by the tested ones, lost there.  But the whole bordered
//      level is 6 x 18^2 x 16 B = 31 KB.  k_mc_resident stages it once per tile and then (i) runs, face by face in index order, the samples
//      binning proves for the tile (region_bin with PROOF and SOLE: one flagged face, every texel on it, taps inside its block) as
//      certain_sample -- with the unproved samples gone from the face passes a word's proved bits of a face ARE one run, masks[f][w] &
//      cmask[w], nothing splits it -- and (ii) takes every other sample ONCE in a general pass over ~cmask, each lane selecting the face of
//      its own direction with v_cube* as the direct kernel does and tapping that face's block through tap_accumulate with a per-lane base
//      (general_sample).  No pair is visited twice, there is no count-only body, the faces need not partition the directions consistently
//      (a tie on a cube edge may go to either face: the apron makes both give the same tap up to rounding), and the completeness count and
//      heal_slice have no role: the general pass takes all 64 lanes, and a proved sample is credited without a test in k_mc_region as well.
//      In their place the PBR_MC_STATS instantiation re-evaluates, per proved (lane, sample), on_face and the tap bounds (proof_violation;
//      pbrk_mc_resident_stats, slot 0: must stay 0) and counts the pairs each pass takes.  No absorb test, no head / tail phases, no launch
//      cut: at roughness 0.6 every one of the 8192 weights is needed.  C2's 16 -> 256^2 level runs the 1389-sample table of roughness 0.03,
//      most of which a launch cut could drop; that cut is left out of this kernel.
//      Rule (mc_plan, resident asked ahead of region): n_src <= 16, n_tab <= 8192 and an output of 256^2 or more take 16 x 16
//      tiles x 4 slices, the work split, tree, divisor and alpha store of k_mc_region; outputs of 128^2 .. 255^2 take 8 x 8 tiles x 16
//      slices (one wave holds a tile and a slice, a 16-way tree; MC_RESIDENT_TILE8), smaller ones stay on the level-in-LDS kernel of
//      k_mc.hip.  FOLD where n_src is a power of two, the unfolded body elsewhere (n_src = 12).  The ORDER of a texel's sum now depends on
//      what its tile proves, so the tiles are anchored at row 0 of the face, not at the dispatch's first row, and their frames, spread and
//      centre are those of the whole tile whatever rows the dispatch holds: a texel has the same tile, proof and order in every dispatch,
//      a row shard equals the full dispatch bit for bit, and a dispatch that starts or ends inside a tile computes the tile and stores its
//      own rows.  A slice adds its proved samples by face and index, then the rest by index, and in both the samples of one mask word are
//      summed on their own and enter the slice's sum as one term ("Word sums" at k_mc_resident: on a level of ones 6.6e-7 from the direct
//      kernel where sums taken straight, and k_mc_region<18, ..>, stand at 2.6e-6): the levels this kernel takes move by a re-association
//      (C4 mip 4: at most 4.9e-6 relative, 63 ulp); pbrk_mc_set_resident(0) / PBR_MC_RESIDENT=0 give the earlier kernels and bytes.  At
//      most 47 VGPRs, no spill, no scratch; 36 VALU per proved sample, 43 per general one, six per word and pass; every k_mc_region
//      instantiation keeps its opcode sequence.  Measured (profiles/resident_levels.md).
//   2l. (the completeness net out of the product kernel; NET) step 3 adds nothing to any sum.  It was there to catch a flag binning failed to
//      set: every wave counts the pairs it takes (cnt += 1 under the exec mask of every tested sample, a popcount per word for the proved
//      ones, cut_credit for the words of the launch cut), an absorbed word (2c) still walks its unproved samples through the count-only body
//      -- frame transform, in-face and in-region tests, ballot, its own table load, no taps -- only so that the count stays complete, and a
//      wave whose count is short of expect[s] recomputes its slice (heal_slice; seen once, the ulp case of 2i, which SOLE closed).  NET = false is the lean run loop (RUNS and LEAN, both FOLD values: <66, true, 32>,
//      <66, true, 16>, <66, false, 16>, <34, false, 16>) without cnt, the credits, the read of expect[], the final ballot and heal_slice; an
//      absorbed word ends at `continue` behind its threshold test.  Every test that decides what is accumulated stays (the wave-uniform
//      early exit of SUB, every `in`): the samples accumulated, their order and arithmetic are the same, so are the bytes.  With heal_slice
//      gone nothing behind the passes reads the frame, and B is formed again from T and R per staging (the same products and differences)
//      instead of living across the passes: the quarter-face instantiations otherwise spill one VGPR.  At most 61 VGPRs, no VGPR spill, no scratch.
//      The 34^2 shape has no absorbed words and loses only the count (MC_NET_OFF_34).  Every NET = true instantiation and k_mc_prep keep
//      their opcode sequences; RegArgs keeps its layout.
//      The early end of a pass (MC_MONO_EXIT): with no count-only bodies an absorbed word costs only its test -- two LDS reads through
//      readfirstlane, a scalar load, three compares, a ballot -- and the tail of a pass is a run of such words.  If the slice's word maxima
//      never rise from word k on, then once a word w >= k is absorbed in a pass every later word of that pass is absorbed too: the sums do
//      not move over skipped words and absorb_threshold is monotone in the word maximum for one region maximum.  The pass ends there: same
//      bytes.  k_mc_cut writes k per slice behind the regions' minima (mc_mono_from, k_mc_internal.h; pbrk_mc_mono_slices is its host twin;
//      q.cut bit 1 says it is there: a launch without k_mc_cut walks every word as before); the reference's tables are monotone from their
//      head words on (k = s).  Only NET = false takes the exit; under the counters the words it leaves are credited to stats[6] and [7].
//      Where the net still runs: whenever the device counters are on (PBR_MC_STATS=1: the whole test suite, so every healed == 0 it asserts
//      is the real check), under pbrk_mc_set_net(1), and in every instantiation that has no net-less form (the 18^2 shape, RUNS = false,
//      LEAN = false: the yardsticks of pbrk_mc_set_runs / _prologue).  pbrk_mc_set_net(-1), the default, reads the counters' state and nothing
//      of the dispatch, so a row shard equals the full dispatch; pbrk_mc_last_net tells what the last launch took.  With the net off and the
//      counters on, stats[1] is still counted, [0] and [8] stay 0, [2] .. [7] keep their meaning.  What guards the product path: the byte
//      comparison against the checked instantiation on every shape, table length, row shard, work unit and hostile level of
//      tests/test_gpu_mc_net.py (C4 mips 1 - 3 at full size among them), and the every-texel cross-check against the direct kernel in
//      tests/test_gpu_configs.py.  As k_mc_resident (2k), which never had a net in its product kernel.  Measured: profiles/net_off.md.
//   2m. (binning once per process; the bin cache) region_bin reads the tile's geometry, the level's shape and the sample table, and no texel:
//      for one (kernel shape, n_src, output size, table) every call recomputes the same masks[] and cmask[] in every tile -- a hot reload, a new
//      environment at the same sizes, a probe refreshed each frame -- and the tile-centre frame with its correctly rounded divisions and roots
//      exists only to feed it.  With the sample loops at a quarter of their first length that is 3 - 6 % of a tile's VALU instructions on C4's
//      big levels and 13 % on mip 5.  RegArgs carries two pointers: bins_out (record) -- the first whole-level launch (six faces, every row) bins
//      as ever, but EVERY sample (region_bin's keep_cut: the launch cut depends on the level's texels and moves from call to call; a cut sample sets
//      its mask bit and flags no region), stores the tile's words to device memory (region_bin_record), then clears the cut words as the counters'
//      block does -- and bins (replay) -- every later launch whose tiles are tiles of that dispatch copies them, 16 bytes per lane, zeroes the
//      words at or behind its slice's cut, and rebuilds any[] from the words that are left (region_bin_replay); no centre frame, no dmax, no
//      sample touched.  The flags are the recorded launch's bit for bit, so the samples taken, their order, the absorb decisions and every
//      output byte are what they were; under PBR_MC_STATS the uncut words are loaded and the counters' block counts and clears them: every
//      counter keeps its value.  The branch is workgroup-uniform and sits in the prologue; the sample loops have no new parameter (BINS = RUNS
//      && LEAN is a name for existing ones).  Who takes part: the lean run loops (both FOLD and NET values) and the four forms of
//      k_mc_resident.  Everything else bins as ever: the yardsticks (RUNS = false, LEAN = false, the 18^2 shape), a 66^2 launch without a
//      k_mc_prep slot, stream capture, an unregistered table (pbrk_mc_table_register: a pointer says nothing about its contents; each
//      registration is a generation), and region-kernel row windows that do not start on a tile row of the whole-level dispatch and end on one
//      or at the face's end (mc_bin_window_ok: the tiles start at the dispatch's first row and their frames clamp at its last; ragged shards,
//      the partitions of a multi-GPU job among them).  k_mc_resident's tiles are anchored at row 0 of the face: every dispatch of it may
//      replay.  Tiles lie [face][tile row from row 0][tile column] (mc_bin_tile_index; pbrk_mc_tile_of_block is the host twin of the block ->
//      tile map), (NR + 1) NW words each on a stride of whole 16-byte groups (mc_bin_tile_words).  Host: one entry per {device, kernel shape,
//      n_src, output size, n_entries, table, generation}, an event behind the recording launch that a replay on any stream waits for, one lock,
//      no eviction, a budget (512 MiB per device by default; C4 holds 345 MB beside 2.1 GB of outputs) past which an entry is not created.
//      pbrk_mc_set_bin_cache(-1), the default, is on exactly when the device counters are off -- the rule of pbrk_mc_set_net -- so the suite
//      keeps its paths and tests/test_gpu_mc_bin_cache.py asks for both states by name.  At most 64 VGPRs, no spill, no scratch (the net-carrying
//      instantiations form the texel index again ahead of the reduction to stay there).  Measured: profiles/bin_cache.md.
//   2n. (exact flags in the bin cache; k_mc_refine_bins) the flags of 2m are still region_bin's: one ball around the tile-centre direction,
//      inflated, six face tests with sqrt(2) delta of slack -- a superset of what any texel reaches.  A sample flagged for a region no lane
//      takes it in still runs there (frame transform, in-face test, exec join, on SUB an early exit); a sample every lane takes in one
//      region but the bound cannot prove runs the tested body and cuts a proved run in two; a region with one spurious flag is staged.
//      Since 2m binning is paid once per (kernel shape, level shape, table), so it may cost far more than a bound: behind the recording
//      launch, on its stream and ahead of the event replays wait for, k_mc_refine_bins rewrites the entry's words in place.  One workgroup
//      per recorded tile holds the frames every replaying thread of that tile will hold (texel_of_thread, the clamps of the whole-level
//      dispatch), and for each sample the bound left unproved or flagged for more than one region every lane runs lane_sample's count-only
//      form -- the tested body's own to_face, on_face, reciprocal, tap coordinates and cell comparisons under the view REGION_VIEW_FRAME
//      sets up for visit, with the FOLD the replays will take -- against the regions the bound flagged for it (and, in a wave where a lane
//      finds none of them, against all the others).  The ballots become words
//      (mc_refine_core.h): a flag stays exactly where some lane of the slice's waves takes the sample, a proof bit is set exactly where
//      one region is hit and every lane is in it (SOLE for free; on SUB the cell test then holds for all lanes, which is what
//      certain_sample assumes).  A bit the bound had not set is never set; such hits and lanes that find no region are counted
//      (pbrk_mc_exact_bins_stats: both must stay 0 -- the bound is rigorous).  Cut words are refined like the rest: the cache holds every
//      sample.  The replaying kernels read the same words in the same layout: no instruction of k_mc_region changes, RegArgs, the cache's
//      layout, key and budget stay.  Bytes: a pair is accumulated in the pass of the region the lane's own test puts it in, in index
//      order, whichever body it takes; a flag no lane answers to added nothing; a tested sample all 64 lanes take runs the same twelve
//      FMAs on the same taps as a proved one; an absorbed-word test that no longer happens decided nothing that was accumulated.  The
//      recording launch itself ran on the bound's flags.  k_mc_resident's entries are NOT refined: there the order of a texel's sum depends
//      on what its tile proves, so its bytes would move.  pbrk_mc_set_exact_bins(-1), the default, is on exactly when the device counters
//      are off (the rule of pbrk_mc_set_net and pbrk_mc_set_bin_cache; PBR_MC_EXACT_BINS=0|1) and, per shape by measurement (McShape::EXACT_DEFAULT),
//      today for the 34^2 shape alone: C4 mip 3 10.77 -> 10.13 ms.  The quarter-face level gained 0.45 ms of 7.15 and the 66^2 whole-face
//      level 0.07 of 21.3, both inside five sigma of their launches: they keep the bound's flags unless pbrk_mc_set_exact_bins(1) asks.
//      pbrk_mc_last_exact_bins tells what the last recording did.  48 VGPRs, no scratch; no texel is staged.  Measured: profiles/exact_bins.md.
// Each (texel, sample) pair is accumulated exactly once, in an order (66^2 shapes: head phase then tail phase; in each, own face's
// regions, then the other regions in index order; else regions in index order; sample index inside a region) that depends on the
// level's shape and the texel's face only, not on the tile: a row-sharded dispatch equals a full one bit for bit.
#include "pbr_device.h"
#include "pbr_kernels.h"
#include "k_mc_internal.h"
#include "mc_bins.h"
#include "mc_refine_core.h"

#include <type_traits>

typedef float v4f __attribute__((ext_vector_type(4)));
// The sample table is read-only for the whole launch: a pointer into the constant address space makes every wave-uniform
// read of it a scalar load (behind the kernel's barriers / LDS atomics the compiler no longer proves that for a global pointer
// and falls back to 64-lane vector loads of one address).
typedef const __attribute__((address_space(4))) v4f* ctab_t;
typedef const __attribute__((address_space(3))) v4f* lds_v4f_p;
// the launch's maxima (k_mc_prep): read-only for the region kernel, so wave-uniform reads of them are scalar loads as well
typedef const __attribute__((address_space(4))) unsigned* cu32_t;

// A 1024-thread workgroup owns a TILE x TILE block of output texels and 1024 / TILE^2 slices of the sample table:
//   TILE 16: 256 texels x 4 slices (waves 4s .. 4s+3 own slice s);  TILE 32 (header 2h): 1024 texels x 1 slice.
// The smaller tile halves the frame spread delta the region flags are built from (fewer samples flagged for two regions) and
// pays four times the binning / staging per texel: it wins where regions are small next to that spread (n_src <= 32).
// The shapes' compile-time facts (McShape) and the MC_* switches of the measurements behind them: mc_plan.h.

struct RegArgs {
    McArgs a;
    int G;                      // regions per face edge
    int RC;                     // tap positions (cells) per region edge; the last region of a row may hold fewer
    int NR;                     // 6 * G * G
    int NW;                     // mask words per region = ceil(n_tab / 32)
    int expect[REG_MAX_S];      // samples per slice
    int pole_row[2];            // faces +X / -X: tile row (relative to the dispatch's first row, clamped) nearest to the pole of the tangent frame
    const unsigned* tabmax;     // lean prologue, absorb: [NW] largest weight bit pattern per mask word, then [NR] largest staged R, G, B bit pattern per
                                // region (k_mc_prep, once per launch); null with the parent's prologue
    int cut;                    // header 2g: tabmax holds, behind the maxima, the first cut word of each slice (k_mc_cut); 0: no word is dropped;
                                // bit 1 (header 2l): and, behind the regions' minima, the first word of each slice with no rise behind it
    int absorb;                 // skip mask words whose samples are absorbed by every lane's sums (pbrk_mc_set_absorb; bit-identical)
    unsigned long long* stats;  // optional: [0] += healed wave-slices, [1] += all wave-slices, [2] += (region, sample) flags, [3] += samples per tile, [4] += regions visited,
                                // [5] += proved samples (CERT), [6] += absorbed wave-words, [7] += their wave-samples, [8] += of those run through the
                                // count-only body (a tile's region passes run 4 x [2] wave-samples in all: [2] .. [5] count per block of 256 texels, a 32 x 32 tile four times); PBR_MC_PHASE_STAMPS builds: [9..13] += clocks of
                                // a workgroup's first lane in frames, clearing + binning, staging, region passes, reduction + store;
                                // k_mc_resident (2k): [1] .. [4] per tile as above ([0] and [5] stay: nothing is recomputed, and [5] counts k_mc_region's proved
                                // samples alone), [16] += (lane, sample) pairs whose proof did not hold, [17] += proved samples per tile, [18] / [19] += pairs
                                // taken by the proved runs / by the general pass
    const unsigned* bins;       // header 2m, replay: every tile's flags as an earlier launch of this (kernel shape, level shape, table) recorded them
                                // (mc_bin_tile_index, mc_bin_tile_words); the tile copies its words instead of binning.  null: bin
    unsigned* bins_out;         // header 2m, record: bin every sample (the cut ones too) and store the tile's flags there.  null: do not
};

// direction -> (sc, tc, ma) of face f: the table of v_cubesc / v_cubetc / v_cubema (gen_prefiltered_env_map.glsl:12-23)
__device__ __forceinline__ void face_coords(int f, float x, float y, float z, float& sc, float& tc, float& ma) {
    switch (f) {
    case 0: sc = -z; tc = -y; ma = x; break;
    case 1: sc = z; tc = -y; ma = -x; break;
    case 2: sc = x; tc = z; ma = y; break;
    case 3: sc = x; tc = -z; ma = -y; break;
    case 4: sc = x; tc = -y; ma = z; break;
    default: sc = -x; tc = -y; ma = -z; break;
    }
}

// What a sample body needs of the staged region: set up once per (region, pass) in k_mc_region's visit, wave-uniform but for the frame.
struct RegionView {
    unsigned lds_base;          // LDS byte address of the staged region less its origin's: taps are addressed with face coordinates
    f3 Pb, Pt, Pr;              // the texel's frame under the face's signed permutation: rows give (sc, tc, ma) directly
    float half_n, off;          // bordered tap coordinates u = sc / ma * half_n + off, in [0.5, n + 0.5]
    float ulo, uhi, vlo, vhi;   // the region's cells (SUB): [ulo, uhi) x [vlo, vhi)
};

// (sc, tc, ma) = permuted frame * local direction, same FMA order as the direct kernel's L
__device__ __forceinline__ void to_face(const v4f e, const RegionView& V, float& sc, float& tc, float& ma) {
    sc = fmaf(e.x, V.Pb.x, fmaf(e.y, V.Pt.x, e.z * V.Pr.x));
    tc = fmaf(e.x, V.Pb.y, fmaf(e.y, V.Pt.y, e.z * V.Pr.y));
    ma = fmaf(e.x, V.Pb.z, fmaf(e.y, V.Pt.z, e.z * V.Pr.z));
}

// The frame's part of a RegionView for face f and the region's cells [ox, ox + rcx) x [oy, oy + rcy): the signed permutation of the
// frame, FOLD (header, 2j) six exact multiplies per staging for one per sample.  k_mc_region's visit and k_mc_refine_bins (2n) both
// set their views up with these statements, so the lanes of the second decide with the numbers the first will hold.  A macro, not a
// function: behind a call boundary the compiler orders two moves of the folded net-carrying instantiations differently, and every
// k_mc_region instantiation is to keep its opcode sequence.
#define REGION_VIEW_FRAME(V, FOLD, f, B, T, R, half_n, off, ox, oy, rcx, rcy)                                                   \
    do {                                                                                                                        \
        face_coords(f, B.x, B.y, B.z, V.Pb.x, V.Pb.y, V.Pb.z);                                                                  \
        face_coords(f, T.x, T.y, T.z, V.Pt.x, V.Pt.y, V.Pt.z);                                                                  \
        face_coords(f, R.x, R.y, R.z, V.Pr.x, V.Pr.y, V.Pr.z);                                                                  \
        V.half_n = half_n; V.off = off;                                                                                         \
        if (FOLD) {                                                                                                             \
            V.Pb.x *= half_n; V.Pt.x *= half_n; V.Pr.x *= half_n;                                                               \
            V.Pb.y *= half_n; V.Pt.y *= half_n; V.Pr.y *= half_n;                                                               \
        }                                                                                                                       \
        V.ulo = (float)ox; V.uhi = (float)(ox + rcx); V.vlo = (float)oy; V.vhi = (float)(oy + rcy);                             \
    } while (0)

// In-face test.  CLS = major axis of the region's face (0: x, 1: y, 2: z): the hardware's tie rule (z >= y >= x) in two comparisons.
template <int CLS>
__device__ __forceinline__ void on_face(float sc, float tc, float ma, bool& c1, bool& c2) {
    if (CLS == 0) { c1 = ma > fabsf(sc); c2 = ma > fabsf(tc); }
    else if (CLS == 1) { c1 = ma >= fabsf(sc); c2 = ma > fabsf(tc); }
    else { c1 = ma >= fabsf(sc); c2 = ma >= fabsf(tc); }
}

// The bilinear tap at bordered coordinates (u, v) of the staged region, weight w folded in: THE chain of twelve FMAs every lemma of
// this file speaks about (absorbed words, the launch cut, "a row shard equals the full dispatch"); every sample body ends in it.
// JOIN (header, 2j): the four texels are kept alive by ONE statement.  Each empty asm is a use of its read, and the compiler waits for a
// read ahead of its first use: four statements split the reads into two groups with a wait behind each, one statement lets all four
// fly and waits once.  Same instructions otherwise, same arithmetic; taken where it measured as a gain (MC_TAP_JOIN_G1).
// VBASE (header, 2k): the base differs per lane (each lane taps the face its own direction falls on) and rides in a vector register.
template <int RS, bool JOIN = false, bool VBASE = false>
__device__ __forceinline__ void tap_accumulate(float w, float u, float v, unsigned lds_base, float& ar, float& ag, float& ab) {
    const int il = (int)u, jl = (int)v;
    const float a = __builtin_amdgcn_fractf(u), b = __builtin_amdgcn_fractf(v);
    // whole 16-byte texels: ds_read_b128 runs at 256 B/clk/CU, the 12-byte form the compiler would pick at 96 (the
    // empty asm keeps the fourth component alive); LDS byte address = jl * row + (il << 4) + base (the region's origin
    // is folded into the base) in one shift-add and one 24-bit multiply-add
    unsigned t16, addr;
    if constexpr (VBASE) asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(t16) : "v"(il), "v"(lds_base));
    else asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(t16) : "v"(il), "s"(lds_base));
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(addr) : "v"(jl), "s"(RS * 16), "v"(t16));
    lds_v4f_p tp = (lds_v4f_p)(unsigned long long)addr;
    v4f q00 = tp[0], q10 = tp[1], q01 = tp[RS], q11 = tp[RS + 1];
    if (JOIN) asm("" : "+v"(q00), "+v"(q10), "+v"(q01), "+v"(q11));
    else { asm("" : "+v"(q00)); asm("" : "+v"(q10)); asm("" : "+v"(q01)); asm("" : "+v"(q11)); }
    // weights of the four taps with the sample weight folded in
    const float wa = w * a;
    const float w11 = wa * b;
    const float w10 = wa - w11;
    const float wt = w - wa;
    const float w01 = wt * b;
    const float w00 = wt - w01;
    ar = fmaf(w11, q11.x, fmaf(w01, q01.x, fmaf(w10, q10.x, fmaf(w00, q00.x, ar))));
    ag = fmaf(w11, q11.y, fmaf(w01, q01.y, fmaf(w10, q10.y, fmaf(w00, q00.y, ag))));
    ab = fmaf(w11, q11.z, fmaf(w01, q01.z, fmaf(w10, q10.z, fmaf(w00, q00.z, ab))));
}

// One sample of a pass: accumulate it in the lanes whose direction falls into the staged region.
// ACC = false: the count-only body of an absorbed word -- the same frame transform, predicates, ballots and pair count, no taps.
template <int RS, bool SUB, int CLS, bool ACC = true>
__device__ __forceinline__ void region_sample(const v4f e, const RegionView& V, float& ar, float& ag, float& ab, unsigned& cnt) {
    float sc, tc, ma;
    to_face(e, V, sc, tc, ma);
    // each comparison's lane mask is taken by its own ballot (the compiler folds a ballot of ONE comparison into the v_cmp's
    // SGPR result, not a ballot of their conjunction)
    bool c1, c2;
    on_face<CLS>(sc, tc, ma, c1, c2);
    unsigned long long inm = __builtin_amdgcn_ballot_w64(c1) & __builtin_amdgcn_ballot_w64(c2);
    // Lanes whose direction is not on this face (or, SUB, not in this region's cells) sit the sample out under the exec
    // mask; a wave none of whose lanes is on the face skips the rest.  The (lane, sample) pairs taken are counted per wave
    // with scalar instructions.
    if (inm == 0) return;
    if (!ACC && !SUB) { cnt += (unsigned)__builtin_popcountll(inm); return; }
    bool in = c1 && c2;
    const float h = __builtin_amdgcn_rcpf(ma) * V.half_n;
    const float u = fmaf(sc, h, V.off), v = fmaf(tc, h, V.off);
    if (SUB) {
        // floor(u) in [ox, ox + rcx) <=> u in [ox, ox + rcx) (integer bounds): four float comparisons, no integer arithmetic
        const bool c3 = u >= V.ulo, c4 = u < V.uhi, c5 = v >= V.vlo, c6 = v < V.vhi;
        inm &= __builtin_amdgcn_ballot_w64(c3) & __builtin_amdgcn_ballot_w64(c4) & __builtin_amdgcn_ballot_w64(c5) & __builtin_amdgcn_ballot_w64(c6);
        in = in && c3 && c4 && c5 && c6;
    }
    cnt += (unsigned)__builtin_popcountll(inm);
    if (ACC && in) tap_accumulate<RS>(e.w, u, v, V.lds_base, ar, ag, ab);
}

// The same sample when binning has proved that EVERY texel of the tile taps this region of this face: all 64 lanes are in, so
// the tests, ballots and the exec mask fall away.
// FOLD (header, 2j): the sc and tc rows of V carry half_n, so sc and tc arrive scaled and the reciprocal is taken as it is.
template <int RS, bool FOLD = false, bool JOIN = false>
__device__ __forceinline__ void certain_sample(const v4f e, const RegionView& V, float& ar, float& ag, float& ab) {
    float sc, tc, ma;
    to_face(e, V, sc, tc, ma);
    const float h = FOLD ? __builtin_amdgcn_rcpf(ma) : __builtin_amdgcn_rcpf(ma) * V.half_n;
    tap_accumulate<RS, JOIN>(e.w, fmaf(sc, h, V.off), fmaf(tc, h, V.off), V.lds_base, ar, ag, ab);
}

// ---- scalar-lean loop (round 5, 66^2 shapes) ----
// The same sample as region_sample, counted PER LANE: cnt += 1 in the lanes that take it, under the exec mask the body runs with
// anyway.  That drops the second ballot chain (one 4-way s_and_b64 chain for the count, another for the exec mask) and the
// s_bcnt1; only the wave-uniform early exit of SUB keeps a ballot.
// FOLD (header, 2j): sc and tc arrive scaled by half_n; the in-face test compares them with ma half_n (exact: the same decisions), and
// the multiply of the reciprocal has moved there.
// NET = false (header, 2l): the pair is not counted; every test that decides what is accumulated stays.
template <int RS, bool SUB, int CLS, bool ACC = true, bool FOLD = false, bool JOIN = false, bool NET = true>
__device__ __forceinline__ void lane_sample(const v4f e, const RegionView& V, float& ar, float& ag, float& ab, unsigned& cnt) {
    float sc, tc, ma;
    to_face(e, V, sc, tc, ma);
    bool c1, c2;
    on_face<CLS>(sc, tc, FOLD ? ma * V.half_n : ma, c1, c2);
    bool in = c1 && c2;
    if (SUB && __builtin_amdgcn_ballot_w64(in) == 0ull) return;    // no lane on the face: skip the projection
    const float h = FOLD ? __builtin_amdgcn_rcpf(ma) : __builtin_amdgcn_rcpf(ma) * V.half_n;
    const float u = fmaf(sc, h, V.off), v = fmaf(tc, h, V.off);
    if (SUB) in = in && u >= V.ulo && u < V.uhi && v >= V.vlo && v < V.vhi;
    if (in) {
        if (NET) cnt += 1u;
        if (ACC) tap_accumulate<RS, JOIN>(e.w, u, v, V.lds_base, ar, ag, ab);
    }
}

// f(entry) for the samples of mask m in index order; the next entry's scalar load is issued before the current sample computes
template <typename F>
__device__ __forceinline__ void each_sample(unsigned m, ctab_t tw, F&& f) {
    if (m == 0u) return;
    v4f e = tw[__builtin_ctz(m)];
    m &= m - 1u;
    while (m) {
        const v4f en = tw[__builtin_ctz(m)];
        m &= m - 1u;
        f(e);
        e = en;
    }
    f(e);
}

// ---- absorbed words (round 4) ----
// Lemma.  acc' = fma(x, y, acc) is rounded once, to nearest even.  If acc is a normal positive float and 0 <= x y <= acc 2^-25, then
// acc' == acc: with 2^e <= acc < 2^(e+1), acc 2^-25 < 2^(e-24) = ulp(acc) / 2, so the exact sum acc + x y lies less than half an ulp
// above acc and rounds back to it.  acc being unchanged, the same bound covers the next FMA of the chain.
// A sample's tap weights (wa, w11, w10, wt, w01, w00 of tap_accumulate) are formed from its weight w >= 0 and
// a, b in [0, 1) by monotone roundings: each lies in [0, w].  Its taps are texels of the staged region, so with M = the largest
// R, G, B component staged for the region (border included; all finite and >= +0) every product of the sample's twelve FMAs is <= w M.
// A mask word whose largest weight is W is therefore a no-op for a lane when W M <= acc 2^-25 holds for each of its three sums; a
// wave skips the word only when that holds for all 64 lanes, so what it still accumulates keeps the order (region as visited, sample index).
// In fp32: T = fl(fl(W M) (1 + 2^-20)) 2^25 (the scaling is exact; an overflow gives +inf) and the test acc >= max(T, 2^-100).  For
// acc >= 2^-100, acc 2^-25 >= 2^-125 is normal and exact; if W M > acc 2^-25 (normal range), fl(W M) >= W M (1 - 2^-24) and the
// inflation keeps T > acc: a passing test implies the bound.  A NaN T fails every comparison, and so does a NaN sum.  A weight or
// texel whose bit pattern is not below that of +inf (negative, -0, inf, NaN) switches the word / the region off.
__device__ __forceinline__ float absorb_threshold(float wmax, float m) {
    const float t = wmax * m * 1.00000095367431640625f * 0x1p25f;        // (W M) (1 + 2^-20) 2^25, left to right
    return t < 0x1p-100f ? 0x1p-100f : t;                               // NaN stays NaN
}

// skc (stats only): the workgroup's LDS counters {absorbed wave-words, their wave-samples, of those run through the count-only body}, for one
// absorbed word: m its flagged samples, mu those not proved -- by value: formed in this lane-0 branch, the mask the caller walks next turns per-lane.
__device__ __forceinline__ void count_absorbed(unsigned* skc, unsigned m, unsigned mu) {
    if (skc && (threadIdx.x & 63) == 0) {
        atomicAdd(&skc[0], 1u);
        atomicAdd(&skc[1], (unsigned)__builtin_popcount(m));
        atomicAdd(&skc[2], (unsigned)__builtin_popcount(mu));
    }
}

// One pass over the flagged samples of the words w0, w0 + REG_S, .. below w1 of this wave's slice (the whole slice, or the head word /
// the tail words of header 2g) for the staged region V.  Samples are taken two at a time so that the
// second table entry's scalar load is in flight while the first sample computes.
// cwords holds, per mask word, the samples proved to be in this region for the whole tile.  CERT: they run certain_sample; else
// they are only credited in absorbed words.  cwords + NW (LEAN: wmg, the launch's table): per mask word, the bit pattern of its largest weight.  rbits: the bit
// pattern of the staged region's largest component, not below +inf's where absorbed words must not be skipped.  skc: see count_absorbed.
template <int RS, bool SUB, int CLS, int REG_S, bool CERT, bool LEAN>
__device__ __forceinline__ void region_pass(const RegionView& V, const unsigned* __restrict__ mwords, const unsigned* __restrict__ cwords, cu32_t wmg,
                                            unsigned rbits, unsigned* skc, int NW, int w0, int w1, ctab_t tab,
                                            float& ar, float& ag, float& ab, unsigned& cnt) {
    unsigned mnext = w0 < w1 ? (unsigned)__builtin_amdgcn_readfirstlane((int)mwords[w0]) : 0u;
    unsigned cnext = (CERT && w0 < w1) ? (unsigned)__builtin_amdgcn_readfirstlane((int)cwords[w0]) : 0u;
    for (int w = w0; w < w1; w += REG_S) {
        unsigned m = mnext;
        unsigned c = cnext;
        mnext = w + REG_S < w1 ? (unsigned)__builtin_amdgcn_readfirstlane((int)mwords[w + REG_S]) : 0u;
        if (CERT) {
            cnext = w + REG_S < w1 ? (unsigned)__builtin_amdgcn_readfirstlane((int)cwords[w + REG_S]) : 0u;
            cnt += 64u * (unsigned)__builtin_popcount(m & c);              // every lane takes every proved sample
        }
        ctab_t tw = tab + (w << 5);
        const unsigned wb = (rbits < 0x7f800000u && m != 0u) ? (LEAN ? wmg[w] : (unsigned)__builtin_amdgcn_readfirstlane((int)cwords[NW + w])) : 0x7f800000u;
        if (wb < 0x7f800000u) {
            const float T = absorb_threshold(__uint_as_float(wb), __uint_as_float(rbits));
            if (__builtin_amdgcn_ballot_w64(!(ar >= T && ag >= T && ab >= T)) == 0ull) {
                // absorbed for all 64 lanes: proved samples are credited, the rest run the count-only body (the net of step 3)
                if (!CERT) {
                    c = (unsigned)__builtin_amdgcn_readfirstlane((int)cwords[w]);
                    cnt += 64u * (unsigned)__builtin_popcount(m & c);
                }
                count_absorbed(skc, m, m & ~c);
                m &= ~c;
                while (m) {
                    const int i0 = __builtin_ctz(m);
                    m &= m - 1u;
                    region_sample<RS, SUB, CLS, false>(tw[i0], V, ar, ag, ab, cnt);
                }
                continue;
            }
        }
        while (m) {
            const int i0 = __builtin_ctz(m);
            m &= m - 1u;
            const bool two = m != 0u;
            const int i1 = two ? __builtin_ctz(m) : i0;
            m &= m - 1u;                                                   // no-op when m is already 0
            const v4f e0 = tw[i0];
            const v4f e1 = tw[i1];
            // samples in index order whichever body they take: the order of a texel's sum stays (region as visited, sample index)
            if (CERT && ((c >> i0) & 1u)) certain_sample<RS>(e0, V, ar, ag, ab);
            else region_sample<RS, SUB, CLS>(e0, V, ar, ag, ab, cnt);
            if (two) {
                if (CERT && ((c >> i1) & 1u)) certain_sample<RS>(e1, V, ar, ag, ab);
                else region_sample<RS, SUB, CLS>(e1, V, ar, ag, ab, cnt);
            }
        }
    }
}

// region_pass with less scalar work per word and per sample (round 5, 66^2 shapes; RUNS in k_mc_region).  Same words, samples,
// bodies, absorb decisions and FMA order; cnt counts per LANE (every lane of a complete wave ends at expect[s]):
//   * only the non-empty words of the slice are visited: one LDS read per lane (lane k: word s + REG_S k; one ballot covers 64 REG_S
//     words -- NW <= 256 with four slices, NW <= 64 with one: mc_tile32 keeps longer tables off the one-slice tile) and a ballot,
//     masked by wsel (bit k: word s + REG_S k belongs to this pass -- all, the head word alone, or the tail words: header 2g);
//   * CERT: the proved samples below the next tested one run as a run of certain_sample (no per-sample proved-bit test, no exec
//     join), then the tested one, in index order;
//   * tested samples use lane_sample (one ballot chain), and every loop issues the next table entry's load ahead of the body.
// NET = false (header, 2l): nothing is counted and cnt is not touched.  An absorbed word ends behind its threshold test -- no credit, no
// count-only walk, no read of cwords for the credit.
template <int RS, bool SUB, int CLS, int REG_S, bool CERT, bool LEAN, bool FOLD, bool NET = true>
__device__ __forceinline__ void region_pass_runs(const RegionView& V, const unsigned* __restrict__ mwords, const unsigned* __restrict__ cwords, cu32_t wmg,
                                                 unsigned rbits, unsigned* skc, int NW, int s, unsigned long long wsel, ctab_t tab,
                                                 float& ar, float& ag, float& ab, unsigned& cnt, const RegArgs& q) {
    const int wl = s + REG_S * (int)(threadIdx.x & 63);
    unsigned long long nz = __builtin_amdgcn_ballot_w64(wl < NW && mwords[wl] != 0u) & wsel;
    // header 2j: with the fold, the 66^2 whole-face shape also takes the tap whose four reads wait once (per shape, by measurement)
    constexpr bool JOIN = FOLD && RS == 66 && !SUB && MC_TAP_JOIN_G1 != 0;
    auto tested = [&](const v4f e) { lane_sample<RS, SUB, CLS, true, FOLD, JOIN, NET>(e, V, ar, ag, ab, cnt); };
    while (nz) {
        const int w = s + REG_S * (int)__builtin_ctzll(nz);
        nz &= nz - 1ull;
        const unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)mwords[w]);
        unsigned c = CERT ? (unsigned)__builtin_amdgcn_readfirstlane((int)cwords[w]) : 0u;
        ctab_t tw = tab + (w << 5);
        const unsigned wb = rbits < 0x7f800000u ? (LEAN ? wmg[w] : (unsigned)__builtin_amdgcn_readfirstlane((int)cwords[NW + w])) : 0x7f800000u;
        if (wb < 0x7f800000u) {
            const float T = absorb_threshold(__uint_as_float(wb), __uint_as_float(rbits));
            if (__builtin_amdgcn_ballot_w64(!(ar >= T && ag >= T && ab >= T)) == 0ull) {
                if (!NET) {                                                // absorbed for all 64 lanes: the sums do not change, the word ends here
                    count_absorbed(skc, m, 0u);
                    // Header 2l: the slice's word maxima do not rise from word mono on (mc_mono_from; k_mc_cut wrote it behind the regions' minima,
                    // q.cut bit 1), so every later word of this pass has a threshold no larger and meets the same sums -- absorbed as well.  The
                    // pass ends; under the counters the words it leaves are credited.  Read here, not ahead of the pass: it would live in a scalar
                    // register across every sample of the pass, and the loop has none to spare.
                    if (MC_MONO_EXIT == 0 || !(q.cut & 2) || w < (int)wmg[NW + 2 * q.NR + 4 + s]) continue;
                    if (skc)
                        while (nz) {
                            const int wr = s + REG_S * (int)__builtin_ctzll(nz);
                            nz &= nz - 1ull;
                            count_absorbed(skc, (unsigned)__builtin_amdgcn_readfirstlane((int)mwords[wr]), 0u);
                        }
                    break;
                }
                if (!CERT) c = (unsigned)__builtin_amdgcn_readfirstlane((int)cwords[w]);
                cnt += (unsigned)__builtin_popcount(m & c);                // every lane takes every proved sample
                count_absorbed(skc, m, m & ~c);
                each_sample(m & ~c, tw, [&](const v4f e) { lane_sample<RS, SUB, CLS, false, FOLD>(e, V, ar, ag, ab, cnt); });
                continue;
            }
        }
        if (!CERT) { each_sample(m, tw, tested); continue; }
        if (NET) cnt += (unsigned)__builtin_popcount(m & c);
        unsigned mc = m & c, mu = m & ~c;
        for (;;) {
            const unsigned below = mu ? (mu & (0u - mu)) - 1u : ~0u;     // the samples before the next tested one (all: none left)
            each_sample(mc & below, tw, [&](const v4f e) { certain_sample<RS, FOLD, JOIN>(e, V, ar, ag, ab); });
            mc &= ~below;
            if (!mu) break;
            const int it = __builtin_ctz(mu);
            mu &= mu - 1u;
            tested(tw[it]);
        }
    }
}

// Binning (once per tile): which regions of the source level can the samples reach from ANY texel of the tile?  Every sample
// direction is pushed through the tile-centre frame; a rigorous bound on how far a texel's own frame can move it yields the
// regions; one bit per (region, sample) in `masks`, any[r] != 0 when region r has a bit.  Leaves with a barrier pending: callers
// synchronise before reading the masks.
// cmask (PROOF, [NW]): bit i set when sample i is PROVED to tap one region of one face from every texel of the tile -- certainly
// on the face (ma' - |sc'| >= (ma - |sc|) - sqrt(2) delta > 0), its tap bounds inside the face and inside one region's cells.  Such
// a sample has exactly one region flag.  wmax (optional, [NW]): per mask word, the largest bit pattern of its samples' weights (for
// weights >= +0 the largest weight; anything else orders above +inf).  The ntail words behind dmax are zeroed with the masks.
// SOLE (header, 2i; one region per face): the bit is set only when that face is the ONLY one flagged for the sample.  The inequalities
// say so (ma - sqrt(2) delta > |sc| on one face excludes ma' + sqrt(2) delta >= |sc'| on every other), but both sides are rounded:
// when they meet within an ulp a sample was proved on one face and flagged on its neighbour, and the neighbour's pass, which reads
// the proof per sample and not per region, took it as proved there too.
// LEAN (header, 2f): G and RC are compile-time facts -- G1: one region per face, r = f and no division; else the quarter-face shape,
// RC = 65 -- and the reach bound takes v_rcp_f32 / v_sqrt_f32 (1 ulp each) for the two divisions and two square roots.  That
// moves mu, mv by less than 5e-7 relative (rl enters three times, the root once: 4 x 2^-23 and their roundings), inside the 1.0001
// they carry, and uc, vc by less than 2^-22 (|sc / ma| + 1) half_n texel, under 1e-3 texel up to n = 1024, inside the 0.05: the flags
// stay a superset of what any texel of the tile reaches, and "certain" is claimed under the same inequalities.
// TWO (header, 2g): any[r] holds two flags, byte 0 for the head words (0 .. S - 1: the samples below head_end = 32 S, S the workgroup's
// slices) and byte 1 for the tail words.  lim: the first sample index this thread does not bin -- 32 x the cut word of its slice (a
// thread's samples i = tid + 1024 k all fall into slice (tid >> 5) % S), n_tab without a cut.  keep_cut (counters only): the samples behind lim still run and set their mask bits, but no
// region flag; the caller counts and clears those bits.
template <bool LEAN, bool G1, bool TWO, bool PROOF, bool SOLE>
__device__ __forceinline__ void region_bin(unsigned* masks, unsigned* any, unsigned* dmax, int NR, int NW, int G, int RC, int n,
                                           f3 R, f3 T, f3 B, f3 Rc, f3 Tc, f3 Bc, ctab_t tab, int n_tab, int tid,
                                           unsigned* cmask, unsigned* wmax, int ntail, int lim, bool keep_cut, int head_end) {
    const float nf = (float)n;
    const float half_n = 0.5f * nf;
    const float off = 0.5f * nf + 0.5f;
    for (int k = tid; k < NR * NW + NR + 1 + ntail; k += 1024) masks[k] = 0u;
    __syncthreads();
    {
        f3 dR = sub3(R, Rc), dT = sub3(T, Tc), dB = sub3(B, Bc);
        float d2 = dot3(dR, dR) + dot3(dT, dT) + dot3(dB, dB);
        atomicMax(dmax, __float_as_uint(sqrtf(d2)));                 // non-negative floats order like their bit patterns
    }
    __syncthreads();
    // |L_texel - L_centre| <= |M_texel - M_centre|_2 for a unit local direction.  Both frames are orthonormal, so M_t - M_c =
    // (Rot - I) M_c with singular values {0, 2 sin(theta/2), 2 sin(theta/2)}: the spectral norm is the Frobenius norm / sqrt(2).
    // Inflated for the frames' own rounding (1e-7) and that of both evaluations.
    const float delta = __uint_as_float(*dmax) * 0.70710678f * 1.001f + 4e-6f;
    const int i_end = (TWO && !keep_cut) ? min(n_tab, lim) : n_tab;
    for (int i = tid; i < i_end; i += 1024) {
        const v4f e = tab[i];
        // TWO: the byte of any[r] this sample flags -- 0 head, 1 tail, 2 (never read) a cut sample run for the counters
        const int ab = TWO ? (i >= lim ? 2 : (i >= head_end ? 1 : 0)) : 0;
        const float Lx = fmaf(e.x, Bc.x, fmaf(e.y, Tc.x, e.z * Rc.x));
        const float Ly = fmaf(e.x, Bc.y, fmaf(e.y, Tc.y, e.z * Rc.y));
        const float Lz = fmaf(e.x, Bc.z, fmaf(e.y, Tc.z, e.z * Rc.z));
        const unsigned bit = 1u << (i & 31);
        if (!LEAN && wmax) atomicMax(&wmax[i >> 5], __float_as_uint(e.w));
        [[maybe_unused]] int nflag = 0;                                    // SOLE: the faces flagged for this sample, and whether one of them proved it
        [[maybe_unused]] bool proved = false;
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            float sc, tc, ma;
            face_coords(f, Lx, Ly, Lz, sc, tc, ma);
            // A direction L' with |L' - L|_2 <= delta has ma' - |sc'| <= (ma - |sc|) + sqrt(2) delta: face f needs that >= 0 (same for tc)
            const float d2 = 1.41421357f * delta;
            if (!(ma + d2 >= fabsf(sc)) || !(ma + d2 >= fabsf(tc))) continue;
            int lo_u = 0, hi_u = n, lo_v = 0, hi_v = n;
            const float mlo = ma - delta;
            bool certain = false;
            if (mlo > 0.2f) {
                // g(L) = sc / ma has |grad g| = sqrt(1 + g^2) / ma; along the segment L -> L' (ma >= ma - delta, |g| <= (|sc| + delta) /
                // (ma - delta)) that is bounded, so |g(L') - g(L)| <= delta sqrt(1 + gmax^2) / (ma - delta); + 0.05 texel for rcp / fma rounding
                const float rm = LEAN ? __builtin_amdgcn_rcpf(ma) : 1.0f / ma, rl = LEAN ? __builtin_amdgcn_rcpf(mlo) : 1.0f / mlo;
                const float ru = sc * rm, rv = tc * rm;
                const float gu = (fabsf(sc) + delta) * rl, gv = (fabsf(tc) + delta) * rl;
                const float su = fmaf(gu, gu, 1.0f), sv = fmaf(gv, gv, 1.0f);
                const float mu = delta * (LEAN ? __builtin_amdgcn_sqrtf(su) : sqrtf(su)) * rl * half_n * 1.0001f + 0.05f;
                const float mv = delta * (LEAN ? __builtin_amdgcn_sqrtf(sv) : sqrtf(sv)) * rl * half_n * 1.0001f + 0.05f;
                const float uc = fmaf(ru, half_n, off), vc = fmaf(rv, half_n, off);
                const float ul = floorf(uc - mu), uh = floorf(uc + mu), vl = floorf(vc - mv), vh = floorf(vc + mv);
                if (uh < 0.0f || ul > nf || vh < 0.0f || vl > nf) continue;      // cannot be on this face at all
                lo_u = (int)fmaxf(ul, 0.0f); hi_u = (int)fminf(uh, nf);
                lo_v = (int)fmaxf(vl, 0.0f); hi_v = (int)fminf(vh, nf);
                certain = PROOF && cmask && ma - d2 > fabsf(sc) && ma - d2 > fabsf(tc) && ul >= 0.0f && uh <= nf && vl >= 0.0f && vh <= nf;
            }
            if (SOLE) { ++nflag; proved = proved || certain; certain = false; }
            if (LEAN && G1) {                                              // RC = n + 1: every tap position of the face lies in region f
                if (certain) atomicOr(&cmask[i >> 5], bit);
                atomicOr(&masks[f * NW + (i >> 5)], bit);
                if (TWO) ((unsigned char*)any)[4 * f + ab] = 1;
                else any[f] = 1u;
                continue;
            }
            const int rc = LEAN ? 65 : RC;
            const int gx0 = lo_u / rc, gx1 = hi_u / rc, gy0 = lo_v / rc, gy1 = hi_v / rc;
            if (certain && gx0 == gx1 && gy0 == gy1) atomicOr(&cmask[i >> 5], bit);
            for (int gy = gy0; gy <= gy1; ++gy)
                for (int gx = gx0; gx <= gx1; ++gx) {
                    const int r = (f * G + gy) * G + gx;
                    atomicOr(&masks[r * NW + (i >> 5)], bit);
                    if (TWO) ((unsigned char*)any)[4 * r + ab] = 1;
                    else any[r] = 1u;
                }
        }
        if (SOLE && proved && nflag == 1) atomicOr(&cmask[i >> 5], bit);
    }
}

// Header 2m, replay: region_bin's result for this tile as an earlier launch recorded it at src -- masks[NR][NW], then cmask[NW], every
// sample's bits, the cut ones too (the cut moves with the level's texels, the flags do not).  Coalesced 16-byte loads, a lane's four words
// written to LDS one by one (cmask sits behind any[] and dmax: no 16-byte alignment).  cutw (the launch has a cut): the first cut word of
// each of the S slices; a word at or behind its slice's cut flags no region, as a cut sample flags none in region_bin, and is zeroed --
// unless keep_cut (the counters are on): then it stays for the caller's block to count and clear, as region_bin's keep_cut leaves it.
// any[] is rebuilt as binning sets it: a word that is not zero flags its region; TWO: byte 0 for the head words (below S), byte 1 for
// the rest.  dmax stays 0: nothing reads it.  Leaves with a barrier pending, as region_bin does.
template <bool TWO, int S>
__device__ __forceinline__ void region_bin_replay(unsigned* masks, unsigned* any, int NR, int NW, const unsigned* __restrict__ src, int tid,
                                                  const unsigned* __restrict__ cutw, bool keep_cut) {
    if (tid < NR + 1) masks[NR * NW + tid] = 0u;                    // any[], dmax
    __syncthreads();                                               // also orders the caller's clearing of skc
    const int nflag = NR * NW, nw = nflag + NW;
    for (int k = tid * 4; k < nw; k += 4096) {
        const uint4 v = *(const uint4*)(src + k);
        const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k + j;
            if (kk < nw) {
                const int r = kk / NW, w = kk - r * NW;            // r == NR: cmask
                unsigned m = wv[j];
                const bool cut = cutw && w >= (int)cutw[w % S];
                if (cut && !keep_cut) m = 0u;
                masks[kk < nflag ? kk : kk + NR + 1] = m;
                if (kk < nflag && m != 0u && !cut) {
                    if (TWO) ((unsigned char*)any)[4 * r + (w >= S ? 1 : 0)] = 1;
                    else any[r] = 1u;
                }
            }
        }
    }
}

// Header 2m, record: the tile's flags as region_bin left them (every sample binned: keep_cut) go to dst in replay's layout.  The caller
// has synchronised behind region_bin; it synchronises again before it changes a word.
__device__ __forceinline__ void region_bin_record(const unsigned* masks, int NR, int NW, unsigned* __restrict__ dst, int tid) {
    const int nflag = NR * NW, nw = nflag + NW;
    for (int k = tid; k < nw; k += 1024) dst[k] = masks[k < nflag ? k : k + NR + 1];
}

// Block -> (face, tx, ty).  Tiles in plain block order: consecutive tiles go round-robin over the 8 XCDs.  An XCD-contiguous remap (one
// eighth of the grid per XCD) put all tiles around the pole of the tangent frame -- where every sample is flagged for several regions and
// a tile takes up to 3x as long -- on ONE XCD, and the launch waited for it (a single-face dispatch of a +-X face: 10.2 vs 7.6 ms).
// The whole level fits every XCD's L2, so locality has nothing to lose.
__device__ __forceinline__ void tile_of_block(const RegArgs& q, int& face, int& tx, int& ty) {
    // Longest tiles first: around the pole of the tangent frame (tangent_of: inside the +X face, its antipode inside -X) the frames
    // of a tile twist against each other, a sample lands in several regions and a tile takes up to 3x as long.  In row order those
    // tiles came last on the -X face (pole at 3/4 of its height) and the launch ended in their tail; here the rows of these two
    // faces are dealt outwards from the pole row, so the long tiles start first and the short ones fill in behind them
    // (mc_tile_of_block, k_mc_internal.h: the host's twin is pbrk_mc_tile_of_block).
    mc_tile_of_block(blockIdx.x, q.a.face0, q.a.tiles_x, q.a.tiles_per_face, q.pole_row, face, tx, ty);
}

// Output texel of thread t of a slice.  A wave covers an 8 x 8 quadrant of the tile (not 16 x 4): the smaller its extent, the fewer
// samples its lanes spread over two regions (PBR_MC_WAVE_SHAPE experiment: see DESIGN.md)
template <int TILE>
__device__ __forceinline__ void texel_of_thread(const McArgs& p, int tx, int ty, int t, int& x, int& y) {
    constexpr int QW = TILE / 8, QSH = TILE == 32 ? 2 : (TILE == 16 ? 1 : 0);   // quadrants per tile edge (a power of two) and its log2: 2 x 2 (TILE 16), 4 x 4 (TILE 32), 1 (TILE 8: k_mc_resident)
    static_assert(QW == 1 << QSH, "TILE is 8, 16 or 32");
    const int q8 = t >> 6, l8 = t & 63;
    x = tx * TILE + (q8 & (QW - 1)) * 8 + (l8 & 7);
    y = p.y0 + ty * TILE + (q8 >> QSH) * 8 + (l8 >> 3);
}

// Header 2g: the samples of a slice's cut words (cw, cw + REG_S, .. : full words, but for the table's last one), in the unit cnt counts in
template <int REG_S, bool RUNS>
__device__ __forceinline__ unsigned cut_credit(int cw, int NW, int n_tab) {
    const int last = NW - 1, kc = (last - cw) / REG_S + 1;           // cut words cw, cw + REG_S, .. <= last
    if (cw > last) return 0u;
    return (unsigned)(32 * kc - ((last - cw) % REG_S == 0 ? 32 * NW - n_tab : 0)) * (RUNS ? 1u : 64u);
}

// Staging of the lean 66^2 shapes (header 2f iii): the region's (rcx + 1) x (rcy + 1) texels at fsrc (row pitch nb) by rows.
// Wave w takes rows w, w + 16, ..: the row is wave-uniform, a lane's column is its index -- no division per texel; columns 64
// and 65 go to the first 132 threads, one texel each.  Addresses are clamped into the region, so every load is
// unconditional and all of a thread's loads are issued before its first LDS write; the guards are on the writes.
template <int RS>
__device__ __forceinline__ void stage_rows(float4* region, const float4* __restrict__ fsrc, int nb, int rcx, int rcy, int tid) {
    // The thread index is formed again per staging (opaque to the optimiser): hoisted out of the region loop, the lane's source and
    // LDS offsets stay alive across the passes and spill at the 64-VGPR budget.
    int tid_s = tid;
    asm volatile("" : "+v"(tid_s));
    const int wv = __builtin_amdgcn_readfirstlane(tid_s >> 6), ln = tid_s & 63;
    // row bases are wave-uniform (scalar); a lane adds its clamped column as a 32-bit byte offset
    const unsigned cx = (unsigned)min(ln, rcx) << 4;
    const char* const base = (const char*)fsrc;
    const unsigned rowb = (unsigned)nb << 4;
    const float4 v0 = *(const float4*)(base + (size_t)((unsigned)min(wv, rcy) * rowb) + cx);
    const float4 v1 = *(const float4*)(base + (size_t)((unsigned)min(wv + 16, rcy) * rowb) + cx);
    const float4 v2 = *(const float4*)(base + (size_t)((unsigned)min(wv + 32, rcy) * rowb) + cx);
    const float4 v3 = *(const float4*)(base + (size_t)((unsigned)min(wv + 48, rcy) * rowb) + cx);
    const float4 v4 = *(const float4*)(base + (size_t)((unsigned)min(wv + 64, rcy) * rowb) + cx);
    const int ey = tid_s >> 1, ex = 64 + (tid_s & 1);              // tid < 132: rows 0 .. 65
    const float4 ve = *(const float4*)(base + (unsigned)(min(ey, rcy) * nb + min(ex, rcx)) * 16u);
    if (ln <= rcx) {
        float4* const dst = region + wv * RS + ln;
        if (wv <= rcy) dst[0] = v0;
        if (wv + 16 <= rcy) dst[16 * RS] = v1;
        if (wv + 32 <= rcy) dst[32 * RS] = v2;
        if (wv + 48 <= rcy) dst[48 * RS] = v3;
        if (wv + 64 <= rcy) dst[64 * RS] = v4;
    }
    if (tid_s < 2 * RS && ex <= rcx && ey <= rcy) region[ey * RS + ex] = ve;
}

// Staging of every other shape: two sweeps of the workgroup over RS x RS with a constant divisor.  MAXIMA (absorb, !LEAN): the largest R, G, B
// bit pattern (any negative / inf / NaN orders above +inf) goes to *rmax_r, if given: wave maximum, one LDS atomic per wave, ahead of the caller's barrier.
template <int RS, bool MAXIMA>
__device__ __forceinline__ void stage_sweeps(float4* region, const float4* __restrict__ fsrc, int nb, int rcx, int rcy, int tid, unsigned* rmax_r) {
    unsigned vmax = 0u;
    for (int k = tid; k < RS * RS; k += 1024) {
        const int ry = k / RS, rx = k - ry * RS;
        if (rx <= rcx && ry <= rcy) {
            const float4 v = fsrc[ry * nb + rx];
            region[k] = v;
            if (MAXIMA) vmax = max(vmax, max(__float_as_uint(v.x), max(__float_as_uint(v.y), __float_as_uint(v.z))));
        }
    }
    if (MAXIMA && rmax_r) {
        // xor butterflies inside each 32-lane half (ds_swizzle: the pattern is an immediate, no lane-address registers), halves via readlane
        vmax = max(vmax, (unsigned)__builtin_amdgcn_ds_swizzle((int)vmax, (16 << 10) | 0x1f));
        vmax = max(vmax, (unsigned)__builtin_amdgcn_ds_swizzle((int)vmax, (8 << 10) | 0x1f));
        vmax = max(vmax, (unsigned)__builtin_amdgcn_ds_swizzle((int)vmax, (4 << 10) | 0x1f));
        vmax = max(vmax, (unsigned)__builtin_amdgcn_ds_swizzle((int)vmax, (2 << 10) | 0x1f));
        vmax = max(vmax, (unsigned)__builtin_amdgcn_ds_swizzle((int)vmax, (1 << 10) | 0x1f));
        const unsigned wv = max((unsigned)__builtin_amdgcn_readlane((int)vmax, 0), (unsigned)__builtin_amdgcn_readlane((int)vmax, 32));
        if ((tid & 63) == 0) atomicMax(rmax_r, wv);
    }
}

// Header, step 3: a wave that missed a sample recomputes its slice (words s, s + REG_S, ..) with direct loads, as the direct kernel would
template <int REG_S>
__device__ __forceinline__ void heal_slice(const McArgs& p, ctab_t tab, int NW, int s, f3 R, f3 T, f3 B, float& ar, float& ag, float& ab) {
    const int nb = p.n_src + 2;
    const float nf = (float)p.n_src, off = 0.5f * nf + 0.5f;
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, (int)p.src_bytes, 0x00020000);
    ar = 0.0f; ag = 0.0f; ab = 0.0f;
    for (int w = s; w < NW; w += REG_S) {
        const int i1 = min((w << 5) + 32, p.n_tab);
        for (int i = w << 5; i < i1; ++i) {
            const v4f e = tab[i];
            f3 L;
            L.x = fmaf(e.x, B.x, fmaf(e.y, T.x, e.z * R.x));
            L.y = fmaf(e.x, B.y, fmaf(e.y, T.y, e.z * R.y));
            L.z = fmaf(e.x, B.z, fmaf(e.y, T.z, e.z * R.z));
            f3 c = sample_bordered<false>(rs, L, nf, off, nb, nb * 16);
            ar = fmaf(e.w, c.x, ar); ag = fmaf(e.w, c.y, ag); ab = fmaf(e.w, c.z, ab);
        }
    }
}

// Header, step 4: the sums of texel t over the REG_S slices, by a fixed tree, end in red[3 t ..] (one slice: nothing to combine, red[] only
// hands the sums to the store).  The caller's barrier has ended every read of the staged region red[] overlays.
template <int REG_TX, int REG_S>
__device__ __forceinline__ void reduce_slices(float* red, int s, int t, float ar, float ag, float ab) {
    red[(s * REG_TX + t) * 3 + 0] = ar;
    red[(s * REG_TX + t) * 3 + 1] = ag;
    red[(s * REG_TX + t) * 3 + 2] = ab;
    __syncthreads();
    for (int stride = REG_S / 2; stride >= 1; stride >>= 1) {
        if (s < stride) {
            const int a2 = (s * REG_TX + t) * 3, b2 = ((s + stride) * REG_TX + t) * 3;
            red[a2 + 0] += red[b2 + 0];
            red[a2 + 1] += red[b2 + 1];
            red[a2 + 2] += red[b2 + 2];
        }
        __syncthreads();
    }
}

// Clock of the calling lane (PBR_MC_PHASE_STAMPS builds only: where a tile's time goes; the product build has no stamp in it)
#ifdef PBR_MC_PHASE_STAMPS
#define STAMP() ((unsigned long long)__builtin_readcyclecounter())
#else
#define STAMP() 0ull
#endif

// RUNS (66^2 shapes and the 34^2 shape): the region loop visits the flagged regions only and runs region_pass_runs (round 5; cnt per lane)
// LEAN: the prologue of header 2f (pbrk_mc_set_prologue); false: the one before it, kept as the yardstick
// FOLD (header, 2j; power-of-two levels under RUNS and LEAN): half_n rides in the sc and tc rows of the permuted frame
// NET (header, 2l): step 3, the completeness net -- the pair count, the credits, the count-only bodies, the check and heal_slice.  false:
// none of it (the lean run loops only); expect[] is not read
// The body reads: frames, bin, credit, the loop of (stage, pass) over the flagged regions, check / heal, reduce / store.
template <int RS, bool SUB, int TILE, bool RUNS = false, bool LEAN = false, bool FOLD = false, bool NET = true>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_mc_region(const RegArgs q) {
    constexpr int REG_TX = TILE * TILE, REG_S = 1024 / REG_TX;
    static_assert(!FOLD || (RUNS && LEAN && RS != 18), "FOLD: the run loop of the lean 66^2 / 34^2 shapes only");
    static_assert(NET || (RUNS && LEAN && RS != 18), "NET = false: the run loop of the lean 66^2 / 34^2 shapes only");
    // see the header, 2b and 2i: quarter faces always; whole faces only with the run loop, which pays no per-sample choice of body
    constexpr bool CERT = SUB || (RUNS && (RS != 66 || MC_CERT_G1 != 0));
    using SH = McShape<RS, SUB, TILE>;                                  // ABS (2c), OWN_FIRST (2e), TWO (2g): mc_plan.h
    constexpr bool ABS = SH::ABS;
    const bool absorb_on = ABS && q.absorb;                              // workgroup-uniform
    constexpr bool OWN_FIRST = SH::OWN_FIRST;
    // see the header, 2m: the product instantiations (the lean run loops, both FOLD and NET values) can record and replay their binning
    constexpr bool BINS = RUNS && LEAN;
    constexpr bool TWO = SH::TWO;
    const bool cut_on = TWO && LEAN && q.cut != 0;                       // workgroup-uniform: the launch's cut words are not binned
    // LDS layout: the staged region (RS^2 texels), then in words skc[4] | masks[NR NW] | any[NR] | dmax[1] | cmask[NW] | wmax[NW] | rmax[NR].
    // mc_region_lds (mc_plan.h) is this chain up to cmask, its absorb term the last two.  region_bin clears masks .. dmax and the
    // ntail words behind dmax: the arrays this launch reads.  All three move together.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_r[];
    float4* region = (float4*)smem_r;
    const unsigned lds_base = (unsigned)(unsigned long long)smem_r;      // LDS byte offset of the staged region (low half of the flat address)
    unsigned* skc = (unsigned*)(smem_r + RS * RS * 16);                  // [4] (absorb, stats) counters of the absorbed words: a fixed address
    unsigned* masks = skc + 4;
    unsigned* any = masks + q.NR * q.NW;
    unsigned* dmax = any + q.NR;
    unsigned* cmask = dmax + 1;                                          // [NW] samples proved to tap one region from the whole tile
    unsigned* wmax = cmask + q.NW;                                       // [NW] (absorb, !LEAN) largest weight (bit pattern) per mask word
    unsigned* rmax = wmax + q.NW;                                        // [NR] (absorb, !LEAN) largest staged R, G, B bit pattern per region
    const int ntail = (absorb_on && !LEAN) ? 2 * q.NW + q.NR : ((CERT || ABS) ? q.NW : 0);
    cu32_t wmg = (cu32_t)(unsigned long long)q.tabmax;                   // (absorb, LEAN) the same two for the whole launch: [NW], then [NR]
    [[maybe_unused]] const unsigned long long st0 = STAMP();
    const McArgs& p = q.a;
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid / REG_TX);
    const int t = tid % REG_TX;

    int face, tx, ty, x, y;
    tile_of_block(q, face, tx, ty);
    texel_of_thread<TILE>(p, tx, ty, t, x, y);
    const int xc = min(x, p.size - 1), yc = min(y, p.y0 + p.rows - 1);

    const f3 R = face_texel_dir(face, xc, yc, p.size);
    const f3 T = tangent_of(R);
    const f3 B = cross3(T, R);

    const int n = p.n_src, nb = n + 2;
    const float nf = (float)n;
    const float half_n = 0.5f * nf;
    const float off = 0.5f * nf + 0.5f;
    ctab_t tab = (ctab_t)(unsigned long long)p.tab;
    const int NW = q.NW, NR = q.NR, G = q.G, RC = q.RC;

    // ---- 1. binning ----
    if (ABS && tid < 4) skc[tid] = 0u;                                   // ordered by the barrier behind region_bin's clearing
    [[maybe_unused]] const unsigned long long st1 = STAMP();
    // the first cut word of this thread's slice (a vector load of one of the REG_S words behind the maxima): samples tid + 1024 k lie
    // in word (tid >> 5) + 32 k, that is in slice (tid >> 5) % REG_S
    // header 2m: this tile's place in the bin cache -- its (face, row from row 0 of the face, column) in the whole-level dispatch
    [[maybe_unused]] const size_t bin_at = (size_t)mc_bin_tile_index(face, p.y0 / TILE, ty, tx, p.tiles_x, (p.size + TILE - 1) / TILE) * mc_bin_tile_words(NR, NW);
    if (BINS && q.bins) {                                                // workgroup-uniform: no centre frame, no dmax, no sample is looked at
        region_bin_replay<TWO, REG_S>(masks, any, NR, NW, q.bins + bin_at, tid, cut_on ? q.tabmax + NW + NR : nullptr, q.stats != nullptr);
    } else {
        // tile-centre frame (evaluated redundantly per lane: wave-uniform values)
        const f3 Rc = face_texel_dir(face, min(tx * TILE + TILE / 2, p.size - 1), min(p.y0 + ty * TILE + TILE / 2, p.y0 + p.rows - 1), p.size);
        const f3 Tc = tangent_of(Rc);
        const f3 Bc = cross3(Tc, Rc);
        const bool rec = BINS && q.bins_out != nullptr;                  // workgroup-uniform
        const int lim = cut_on ? (int)q.tabmax[NW + NR + ((tid >> 5) % REG_S)] << 5 : 0x7fffffff;
        region_bin<LEAN, !SUB, TWO, CERT || ABS, CERT && !SUB>(masks, any, dmax, NR, NW, G, RC, n, R, T, B, Rc, Tc, Bc, tab, p.n_tab, tid, (CERT || ABS) ? cmask : nullptr,
                                    (absorb_on && !LEAN) ? wmax : nullptr, ntail, lim, cut_on && (q.stats != nullptr || rec), 32 * REG_S);
        if (rec) {
            // the cache holds the flags of EVERY sample: the launch cut depends on the level's texels and moves from call to call.  The cut
            // words then go, as in the counters' block below, which keeps doing it (and counting them) when the counters are on.
            __syncthreads();
            region_bin_record(masks, NR, NW, q.bins_out + bin_at, tid);
            if (cut_on && !q.stats) {
                __syncthreads();
                for (int k = tid; k < NR * NW; k += 1024) {
                    const int w = k % NW;
                    if (w >= (int)q.tabmax[NW + NR + (w % REG_S)]) masks[k] = 0u;
                }
            }
        }
    }
    [[maybe_unused]] unsigned long long st_stage = 0ull;
#ifdef PBR_MC_PHASE_STAMPS
    __syncthreads();                                               // the wait for the slowest thread's binning is charged to binning
#endif
    [[maybe_unused]] const unsigned long long st2 = STAMP();       // the diagnostics below are charged to no phase

    // ---- 2. region passes ----
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    // expect[s] less the samples of the slice's cut words, formed here as a credit: the count starts at what the cut took out, so
    // nothing of it stays alive across the passes
    unsigned cnt = (NET && cut_on) ? cut_credit<REG_S, RUNS>((int)wmg[NW + NR + s], NW, p.n_tab) : 0u;
    if (q.stats) {                                                 // diagnostics: (region, sample) flags of this tile, samples, regions visited
        __syncthreads();
        unsigned fl = 0, cfl = 0, cwd = 0;
        for (int k = tid; k < NR * NW; k += 1024) {
            const unsigned mk = masks[k];
            fl += __popc(mk);
            if (cut_on) {
                // a word of the launch's cut: binned for the counters alone.  Its flags count as absorbed wave-samples of the waves of its
                // slice (16 / REG_S: four, or all sixteen with one slice) that would have met the word (the counters keep their meaning: flagged wave-samples that are not accumulated); its bits go.
                const int w = k % NW;
                if (w >= (int)q.tabmax[NW + NR + (w % REG_S)]) { cfl += __popc(mk); cwd += mk != 0u; masks[k] = 0u; }
            }
        }
        // [2] .. [5] are counted per block of 256 texels (four waves): a 32 x 32 tile adds its flags, samples, regions and proved samples
        // four times, so "the passes visit 4 x [2] wave-samples" and every per-sample / per-tile ratio of these counters hold for both tiles
        constexpr unsigned BLK = REG_TX / 256;
        if (fl) atomicAdd(&q.stats[2], (unsigned long long)(fl * BLK));
        if (cwd) { atomicAdd(&skc[0], (16u / REG_S) * cwd); atomicAdd(&skc[1], (16u / REG_S) * cfl); }      // flushed with the tile's other absorbed words (step 4)
        if (tid == 0) { atomicAdd(&q.stats[3], (unsigned long long)p.n_tab * BLK); unsigned v = 0; for (int r = 0; r < NR; ++r) v += (any[r] & (TWO ? 0xffffu : ~0u)) != 0u; atomicAdd(&q.stats[4], (unsigned long long)(v * BLK));
                        if (CERT) { unsigned c = 0; for (int k = 0; k < NW; ++k) c += __popc(cmask[k]); atomicAdd(&q.stats[5], (unsigned long long)(c * BLK)); } }
    }
    auto visit = [&](const int r, const int ph) {                  // stage region r and run this wave's slice (TWO: its head word, ph 0, or its tail) over it
        const int f = r / (G * G);
        const int gy = (r / G) % G, gx = r % G;
        const int ox = gx * RC, oy = gy * RC;
        const int rcx = min(RC, n + 1 - ox), rcy = min(RC, n + 1 - oy);      // cells of this region; texels: one more
        const float4* __restrict__ fsrc = p.src + ((size_t)f * nb + oy) * nb + ox;
        const unsigned long long sta = STAMP();
        unsigned rbits = 0x7f800000u;                              // wave-uniform; the pattern of +inf (never below itself) when absorbed words must not be skipped
        if (LEAN && RS == 66) stage_rows<RS>(region, fsrc, nb, rcx, rcy, tid);
        else stage_sweeps<RS, ABS && !LEAN>(region, fsrc, nb, rcx, rcy, tid, (absorb_on && !LEAN) ? &rmax[r] : nullptr);
        if (absorb_on && LEAN) rbits = wmg[NW + r];                // scalar load, in flight across the barrier
        __syncthreads();
        if (absorb_on && !LEAN) rbits = (unsigned)__builtin_amdgcn_readfirstlane((int)rmax[r]);
        const unsigned long long stb = STAMP();
        RegionView V;
        V.lds_base = lds_base - (unsigned)(oy * RS + ox) * 16u;
        // signed permutation of the frame for this face
        // NET = false: nothing behind the passes reads the frame (no heal_slice), and B is formed again per staging from a copy of T that is
        // opaque to the optimiser -- the same six products and three differences, the same bits -- instead of staying alive across the passes:
        // at the 64-VGPR budget the quarter-face instantiations otherwise spill one of its components
        f3 Bv = B;
        if constexpr (!NET) {
            f3 Tq = T;
            asm volatile("" : "+v"(Tq.x), "+v"(Tq.y), "+v"(Tq.z));
            Bv = cross3(Tq, R);
        }
        REGION_VIEW_FRAME(V, FOLD, f, Bv, T, R, half_n, off, ox, oy, rcx, rcy);
        const unsigned* mw = masks + r * NW;
        unsigned* const sc = (ABS && q.stats) ? skc : nullptr;
        // the words of this pass: the whole slice, or (TWO) its head word s / its tail words s + REG_S, ..
        const unsigned long long wsel = TWO ? (ph ? ~1ull : 1ull) : ~0ull;
        const int w0 = (TWO && ph) ? s + REG_S : s, w1 = (TWO && !ph) ? min(NW, s + 1) : NW;
        auto pass = [&](auto cls) {                                // cls: the face's major axis as a compile-time constant
            constexpr int CLS = decltype(cls)::value;
            if (RUNS) region_pass_runs<RS, SUB, CLS, REG_S, CERT, LEAN, FOLD, NET>(V, mw, cmask, wmg, rbits, sc, NW, s, wsel, tab, ar, ag, ab, cnt, q);
            else region_pass<RS, SUB, CLS, REG_S, CERT, LEAN>(V, mw, cmask, wmg, rbits, sc, NW, w0, w1, tab, ar, ag, ab, cnt);
        };
        switch (f >> 1) {
        case 0: pass(std::integral_constant<int, 0>()); break;
        case 1: pass(std::integral_constant<int, 1>()); break;
        default: pass(std::integral_constant<int, 2>()); break;
        }
        st_stage += stb - sta;
    };
    [[maybe_unused]] const unsigned long long st2b = STAMP();
    // A barrier ahead of each staging: binning done / readers of the previous region done.  RUNS: it runs for the flagged regions only
    // (once per visited region instead of once per region of the level, and one for binning); any[] is final after binning, so the skip
    // needs none.  (A 64-bit mask of the visited regions kept across the passes, or a ballot search for the next one, spills VGPRs at the
    // 64-VGPR budget of the quarter-face shape.)
    if (RUNS) __syncthreads();
    for (int kk = 0; kk < (TWO ? 2 * NR : NR); ++kk) {             // TWO: all regions for the head words, then all for the tail words (one
        const int ph = TWO && kk >= NR, k = kk - (ph ? NR : 0);    // counter: a second loop variable costs a scalar register across the passes)
        const int r = OWN_FIRST ? mc_region_visit(k, face * (G * G), G * G) : k;
        if (!RUNS) __syncthreads();
        const unsigned av = RUNS ? (unsigned)__builtin_amdgcn_readfirstlane((int)any[r]) : any[r];      // workgroup-uniform
        if ((TWO ? (av >> (8 * ph)) & 0xffu : av) == 0u) continue;
        if (RUNS) __syncthreads();
        visit(r, ph);
    }

    // ---- 3. completeness check; a wave that missed a sample recomputes its slice with direct loads ----
    // cnt is a wave total (scalar): no (texel, sample) pair can be taken twice -- the in-region tests partition the tap positions
    // exactly -- so the total is right exactly when no lane missed a sample
    // RUNS: cnt per lane; a wave recomputes when any lane's count is off (a stronger test than the total)
    [[maybe_unused]] const unsigned long long st3 = STAMP();
    // NET = false: no count, no check, nothing to heal; the wave-slices are still counted
    if constexpr (NET) {
        const bool healed = RUNS ? __builtin_amdgcn_ballot_w64(cnt != (unsigned)q.expect[s]) != 0ull : cnt != 64u * (unsigned)q.expect[s];
        if (healed) heal_slice<REG_S>(p, tab, NW, s, R, T, B, ar, ag, ab);
        if (q.stats && (tid & 63) == 0) {
            if (healed) atomicAdd(&q.stats[0], 1ull);
            atomicAdd(&q.stats[1], 1ull);
        }
    } else if (q.stats && (tid & 63) == 0) atomicAdd(&q.stats[1], 1ull);

    // ---- 4. combine the slices and store ----
    __syncthreads();                                               // everybody is done with the staged region
    if (absorb_on && q.stats && tid < 3 && skc[tid]) atomicAdd(&q.stats[6 + tid], (unsigned long long)skc[tid]);
    float* red = (float*)smem_r;
    // The texel's index and coordinates are formed AGAIN from the thread index (opaque to the optimiser) instead of being kept alive across
    // the passes: at the 64-VGPR budget the quarter-face instantiation otherwise spills them (4 VGPRs, 16 bytes of scratch per lane
    // and tile: harmless in time, but rocprofv3's WRITE_SIZE of C4 mip 1 read 853 MB against 403 MB of output).
    int tid_o = tid, x_o, y_o;
    asm volatile("" : "+v"(tid_o));
    const int t_o = tid_o % REG_TX;
    reduce_slices<REG_TX, REG_S>(red, s, NET ? t_o : t, ar, ag, ab);         // t_o: the net-carrying instantiations have no register to keep t in across the passes
    texel_of_thread<TILE>(p, tx, ty, t_o, x_o, y_o);
    if (x_o < p.size && y_o < p.y0 + p.rows && s == 0) {
        float4 o;
        o.x = red[t_o * 3 + 0] / p.divisor; o.y = red[t_o * 3 + 1] / p.divisor; o.z = red[t_o * 3 + 2] / p.divisor; o.w = p.alpha;
        p.out[((size_t)face * p.size + y_o) * p.size + x_o] = o;
    }
#ifdef PBR_MC_PHASE_STAMPS
    if (q.stats && tid == 0) {                                     // [12]: the region loop less its stagings (passes, barriers, the skipped regions' tests)
        atomicAdd(&q.stats[9], st1 - st0); atomicAdd(&q.stats[10], st2 - st1); atomicAdd(&q.stats[11], st_stage);
        atomicAdd(&q.stats[12], (st3 - st2b) - st_stage); atomicAdd(&q.stats[13], STAMP() - st3);
    }
#endif
}

// ---- header 2n: exact flags in the bin cache ----
struct RefineArgs {
    McArgs a;                   // size, n_src, tab, n_tab, tiles_x of the whole-level dispatch that recorded: y0 = 0, rows = size
    int G, RC, NR, NW;          // as RegArgs
    unsigned* bins;             // the recorded words of every tile (mc_bin_tile_index, mc_bin_tile_words), rewritten in place
    unsigned long long* out;    // [8] += (region, sample) flags before, after; proved samples before, after; stagings a tile's words ask for
                                // ((region, phase) pairs with a flag) before, after; hits on a bit the bound had not set; (lane, sample)
                                // pairs that found no region.  The last two must stay 0
};

// One workgroup per recorded tile, a thread per texel and slice as in k_mc_region<RS, SUB, TILE>: the frames are those every replaying
// thread of the tile will hold.  For every sample of its slice that the bound left unproved or flagged for more than one region, a wave
// runs the count-only form of lane_sample -- the tested body's own frame transform, in-face test, reciprocal, tap coordinates and cell
// comparisons, FOLD as the entry's flavour has it -- against the regions flagged for the sample, and the words of mc_refine_core.h are
// built from the ballots.  No texel is staged or read.  At most 64 VGPRs, no scratch.
template <int RS, bool SUB, int TILE, bool FOLD>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_mc_refine_bins(const RefineArgs g) {
    constexpr int REG_TX = TILE * TILE, REG_S = 1024 / REG_TX;
    constexpr bool TWO = McShape<RS, SUB, TILE>::TWO;
    extern __shared__ __attribute__((aligned(16))) unsigned smem_f[];
    const McArgs& p = g.a;
    const int NR = g.NR, NW = g.NW, G = g.G, RC = g.RC, tid = threadIdx.x;
    const int nflag = NR * NW;
    unsigned* old = smem_f;                                        // [NR][NW] the bound's masks, then [NW] its proof words
    unsigned* need = old + nflag + NW;                             // [NW] mc_refine_need; at the end the new proof words
    unsigned* hit = need + NW;                                     // [NR][NW]; at the end the new masks
    unsigned* part = hit + nflag;                                  // [NR][NW]
    unsigned* tot = part + nflag;                                  // [8] this tile's share of g.out
    const int te = p.tiles_x, face = (int)blockIdx.x / (te * te), tf = (int)blockIdx.x % (te * te), ty = tf / te, tx = tf % te;
    unsigned* words = g.bins + (size_t)mc_bin_tile_index(face, 0, ty, tx, te, te) * mc_bin_tile_words(NR, NW);
    for (int k = tid; k < nflag + NW; k += 1024) old[k] = words[k];
    for (int k = tid; k < 2 * nflag + 8; k += 1024) hit[k] = 0u;
    __syncthreads();
    for (int w = tid; w < NW; w += 1024) {
        unsigned nd = mc_refine_need(old + w, NW, NR, old[nflag + w]);
        if (w == NW - 1 && (p.n_tab & 31)) nd &= (1u << (p.n_tab & 31)) - 1u;      // no sample behind the table's end (the bound sets none)
        need[w] = nd;
    }
    __syncthreads();

    const int s = __builtin_amdgcn_readfirstlane(tid / REG_TX), t = tid % REG_TX;
    int x, y;
    texel_of_thread<TILE>(p, tx, ty, t, x, y);
    const int xc = min(x, p.size - 1), yc = min(y, p.y0 + p.rows - 1);
    const f3 R = face_texel_dir(face, xc, yc, p.size);
    const f3 T = tangent_of(R);
    const f3 B = cross3(T, R);
    const int n = p.n_src;
    const float half_n = 0.5f * (float)n, off = 0.5f * (float)n + 0.5f;
    ctab_t tab = (ctab_t)(unsigned long long)p.tab;

    unsigned cnt = 0u;                                             // per lane: the (region, sample) pairs that took it -- one per sample looked at
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;                         // the count-only body accumulates nothing
    unsigned want = 0u;                                            // wave-uniform: the samples this slice looks at
    for (int w = s; w < NW; w += REG_S) want += (unsigned)__builtin_popcount((unsigned)__builtin_amdgcn_readfirstlane((int)need[w]));
    // Sweep 0: each sample against the regions the bound flagged for it.  The bound is rigorous, so every lane finds its region there;
    // a wave with a lane that did not (counted: tot[7]) goes on to sweep 1, the same samples against the regions the bound did NOT flag,
    // where every hit is a bit the bound had not set (counted by mc_refine_word, never written).
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int r = 0; r < NR; ++r) {
            const int f = r / (G * G), gy = (r / G) % G, gx = r % G;
            const int ox = gx * RC, oy = gy * RC;
            const int rcx = min(RC, n + 1 - ox), rcy = min(RC, n + 1 - oy);
            RegionView V;
            V.lds_base = 0u;
            REGION_VIEW_FRAME(V, FOLD, f, B, T, R, half_n, off, ox, oy, rcx, rcy);
            auto pass = [&](auto cls) {
                constexpr int CLS = decltype(cls)::value;
                for (int w = s; w < NW; w += REG_S) {
                    const unsigned o = (unsigned)__builtin_amdgcn_readfirstlane((int)old[r * NW + w]);
                    unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)need[w]) & (sweep ? ~o : o);
                    if (m == 0u) continue;
                    ctab_t tw = tab + (w << 5);
                    unsigned h = 0u, pt = 0u;
                    while (m) {
                        const int i = __builtin_ctz(m);
                        m &= m - 1u;
                        const unsigned c0 = cnt;
                        lane_sample<RS, SUB, CLS, false, FOLD, false, true>(tw[i], V, ar, ag, ab, cnt);
                        mc_refine_ballot(__builtin_amdgcn_ballot_w64(cnt != c0), i, h, pt);
                    }
                    if ((tid & 63) == 0) {
                        if (h) atomicOr(&hit[r * NW + w], h);
                        if (pt) atomicOr(&part[r * NW + w], pt);
                    }
                }
            };
            switch (f >> 1) {
            case 0: pass(std::integral_constant<int, 0>()); break;
            case 1: pass(std::integral_constant<int, 1>()); break;
            default: pass(std::integral_constant<int, 2>()); break;
            }
        }
        if (sweep == 0) {
            const unsigned long long lost = __builtin_amdgcn_ballot_w64(cnt != want);
            if (lost == 0ull) break;
            if ((tid & 63) == 0) atomicAdd(&tot[7], (unsigned)__builtin_popcountll(lost));
        }
    }
    __syncthreads();

    for (int w = tid; w < NW; w += 1024) {
        unsigned long long unset = 0ull;
        need[w] = mc_refine_word(old + w, NW, NR, old[nflag + w], need[w], hit + w, part + w, NW, hit + w, NW, &unset);
        if (unset) atomicAdd(&tot[6], (unsigned)unset);
    }
    __syncthreads();
    {
        unsigned fb = 0u, fa = 0u, pb = 0u, pa = 0u;
        for (int k = tid; k < nflag; k += 1024) { fb += __popc(old[k]); fa += __popc(hit[k]); words[k] = hit[k]; }
        for (int k = tid; k < NW; k += 1024) { pb += __popc(old[nflag + k]); pa += __popc(need[k]); words[nflag + k] = need[k]; }
        if (fb) atomicAdd(&tot[0], fb);
        if (fa) atomicAdd(&tot[1], fa);
        if (pb) atomicAdd(&tot[2], pb);
        if (pa) atomicAdd(&tot[3], pa);
        if (tid < NR) {
            // the stagings these words ask for: a region with a flag; TWO: once for the head words (below REG_S), once for the tail
            unsigned bh = 0u, bt = 0u, ah = 0u, at = 0u;
            for (int w = 0; w < NW; ++w) {
                const unsigned o = old[tid * NW + w], a2 = hit[tid * NW + w];
                if (TWO && w >= REG_S) { bt |= o; at |= a2; } else { bh |= o; ah |= a2; }
            }
            atomicAdd(&tot[4], (bh != 0u) + (bt != 0u));
            atomicAdd(&tot[5], (ah != 0u) + (at != 0u));
        }
    }
    __syncthreads();
    if (tid < 8 && tot[tid]) atomicAdd(&g.out[tid], (unsigned long long)tot[tid]);
}

// ---- levels resident in LDS as a whole (header, 2k) ----
// Every face is staged with the row pitch of the 18^2 shape, whatever n_src <= 16 is (RES_RS, RES_FACE_BYTES: mc_plan.h).

struct ResArgs {
    RegArgs q;                  // a.y0, a.rows: the rows of the 16-row tiles that hold the dispatch's rows, counted from row 0 of the face;
                                // G = 1, RC = n_src + 1, NR = 6; expect, tabmax, cut and absorb are not read
    int ys, ye;                 // the dispatch's rows [ys, ye): what is stored
};

// A sample no proof covers: each lane selects the face its own direction falls on, as the direct kernel does (v_cube*; a tie on a cube
// edge may go to either face: the apron makes both give the same tap up to rounding), and taps that face's block of the resident level.
// rcp(|2 ma|) n is rcp(ma) n / 2 bit for bit (powers of two), and by the lemma of 2j the folded form rounds the same u, v: the tap
// coordinates are those of certain_sample and of region_sample on the face chosen.  basef: the LDS byte address of face 0's block as a
// float; with the face's offset (at most 5 x 5184) it stays an integer below 2^24, exact in fp32.
__device__ __forceinline__ void general_sample(const v4f e, f3 R, f3 T, f3 B, float nf, float off, float basef, float& ar, float& ag, float& ab) {
    const float Lx = fmaf(e.x, B.x, fmaf(e.y, T.x, e.z * R.x));
    const float Ly = fmaf(e.x, B.y, fmaf(e.y, T.y, e.z * R.y));
    const float Lz = fmaf(e.x, B.z, fmaf(e.y, T.z, e.z * R.z));
    const float fid = __builtin_amdgcn_cubeid(Lx, Ly, Lz);
    const float sc = __builtin_amdgcn_cubesc(Lx, Ly, Lz);
    const float tc = __builtin_amdgcn_cubetc(Lx, Ly, Lz);
    const float h = __builtin_amdgcn_rcpf(fabsf(__builtin_amdgcn_cubema(Lx, Ly, Lz))) * nf;
    const unsigned vbase = (unsigned)fmaf(fid, (float)RES_FACE_BYTES, basef);
    tap_accumulate<RES_RS, false, true>(e.w, fmaf(sc, h, off), fmaf(tc, h, off), vbase, ar, ag, ab);
}

// PBR_MC_STATS only: 1 when the proof binning gave for this sample does not hold in this lane -- the direction is not on the face
// (on_face, the tie rule of the face's class) or its tap leaves the face's bordered block (0.5 <= u, v < n + 1.5).
template <int CLS, bool FOLD>
__device__ __forceinline__ unsigned proof_violation(const v4f e, const RegionView& V, float nf) {
    float sc, tc, ma;
    to_face(e, V, sc, tc, ma);
    bool c1, c2;
    on_face<CLS>(sc, tc, FOLD ? ma * V.half_n : ma, c1, c2);
    const float h = FOLD ? __builtin_amdgcn_rcpf(ma) : __builtin_amdgcn_rcpf(ma) * V.half_n;
    const float u = fmaf(sc, h, V.off), v = fmaf(tc, h, V.off);
    return (c1 && c2 && u >= 0.5f && u < nf + 1.5f && v >= 0.5f && v < nf + 1.5f) ? 0u : 1u;
}

// The proved samples of face F in this wave's slice (words s, s + REG_S, ..; pm: the face's flags, already masked by the proof), as runs of
// certain_sample: no test, no ballot, no exec mask, and nothing that splits a word's run.
template <int F, int REG_S, bool FOLD, bool STATS>
__device__ __forceinline__ void resident_face(const unsigned* __restrict__ pm, int NW, int s, ctab_t tab, unsigned lds_base, f3 R, f3 T, f3 B,
                                              float nf, float& ar, float& ag, float& ab, unsigned& viol, unsigned& taken) {
    RegionView V;
    V.lds_base = lds_base + (unsigned)(F * RES_FACE_BYTES);
    face_coords(F, B.x, B.y, B.z, V.Pb.x, V.Pb.y, V.Pb.z);
    face_coords(F, T.x, T.y, T.z, V.Pt.x, V.Pt.y, V.Pt.z);
    face_coords(F, R.x, R.y, R.z, V.Pr.x, V.Pr.y, V.Pr.z);
    V.half_n = 0.5f * nf; V.off = 0.5f * nf + 0.5f;
    if (FOLD) {
        V.Pb.x *= V.half_n; V.Pt.x *= V.half_n; V.Pr.x *= V.half_n;
        V.Pb.y *= V.half_n; V.Pt.y *= V.half_n; V.Pr.y *= V.half_n;
    }
    unsigned mnext = s < NW ? (unsigned)__builtin_amdgcn_readfirstlane((int)pm[s]) : 0u;
    for (int w = s; w < NW; w += REG_S) {
        const unsigned m = mnext;
        mnext = w + REG_S < NW ? (unsigned)__builtin_amdgcn_readfirstlane((int)pm[w + REG_S]) : 0u;
        if (STATS) taken += (unsigned)__builtin_popcount(m);
        if (m == 0u) continue;
        // a word's samples go to sums of their own, added to the slice's once per word ("Word sums" at k_mc_resident)
        float wr = 0.0f, wg = 0.0f, wb = 0.0f;
        each_sample(m, tab + (w << 5), [&](const v4f e) {
            certain_sample<RES_RS, FOLD>(e, V, wr, wg, wb);
            if (STATS) viol += proof_violation<(F >> 1), FOLD>(e, V, nf);
        });
        ar += wr; ag += wg; ab += wb;
    }
}

// Header 2k.  The body reads: stage the level, frames, bin, split the flags into proved-per-face and the rest, the proved runs face by
// face, the general pass, reduce / store.  STATS: the instantiation launched when the counters are on (PBR_MC_STATS=1); the product
// kernel carries none of them.
// TILE 16: 16 x 16 texels x 4 slices, a wave per 8 x 8 quadrant and slice; TILE 8 (128^2 outputs): 8 x 8 texels x 16 slices, one wave holds the
// tile and one slice (slice s: words s, s + 16, ..), the tree is 16-way.
// Word sums: the samples a pass takes from one mask word (at most 32, one FMA chain each, unchanged) are added up from zero and that sum
// is added to the slice's, once per word and pass.  A slice of 2048 samples otherwise makes 8192 roundings at the size of its whole sum --
// on a level of ones 2.6e-6 from the direct kernel, which adds each weight with one rounding, and as far as k_mc_region<18, ..> stands;
// with word sums the roundings at that size are the few hundred word additions (16 -> 256^2, level of ones: see profiles/resident_levels.md).
template <int TILE, bool FOLD, bool STATS>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_mc_resident(const ResArgs g) {
    constexpr int REG_TX = TILE * TILE, REG_S = 1024 / REG_TX, RS = RES_RS;
    // LDS layout: the level (6 RS^2 texels), then in words masks[6 NW] | any[6] | dmax[1] | cmask[NW]: region_bin's chain (mc_resident_lds, mc_plan.h)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_v[];
    float4* lvl = (float4*)smem_v;
    const unsigned lds_base = (unsigned)(unsigned long long)smem_v;
    const RegArgs& q = g.q;
    const McArgs& p = q.a;
    const int NW = q.NW;
    unsigned* masks = (unsigned*)(smem_v + 6 * RES_FACE_BYTES);
    unsigned* any = masks + 6 * NW;
    unsigned* dmax = any + 6;
    unsigned* cmask = dmax + 1;
    const int tid = threadIdx.x;
    const int s = __builtin_amdgcn_readfirstlane(tid / REG_TX);
    const int t = tid % REG_TX;
    const int n = p.n_src, nb = n + 2;
    const float nf = (float)n;

    // ---- 1. the whole bordered level, once: a plain strided copy (region_bin's barriers order it ahead of every tap) ----
    for (int k = tid; k < 6 * RS * RS; k += 1024) {
        const int f = k / (RS * RS), r = k - f * (RS * RS), ry = r / RS, rx = r - ry * RS;
        if (rx < nb && ry < nb) lvl[k] = p.src[(f * nb + ry) * nb + rx];
    }

    int face, tx, ty, x, y;
    tile_of_block(q, face, tx, ty);
    texel_of_thread<TILE>(p, tx, ty, t, x, y);
    // p.y0 + p.rows is the end of the last tile row or of the face, never of the dispatch: frames, binning and with them the order of
    // every texel's sum depend on the tile alone
    const int xc = min(x, p.size - 1), yc = min(y, p.y0 + p.rows - 1);
    const f3 R = face_texel_dir(face, xc, yc, p.size);
    const f3 T = tangent_of(R);
    const f3 B = cross3(T, R);
    ctab_t tab = (ctab_t)(unsigned long long)p.tab;

    // ---- 2. binning, with the proof (one flagged face, every texel of the tile on it, taps inside its block) ----
    // header 2m: recorded once per (tile size, level shape, table), copied from then on; p.y0 is a tile row of the face here
    const size_t bin_at = (size_t)mc_bin_tile_index(face, p.y0 / TILE, ty, tx, p.tiles_x, (p.size + TILE - 1) / TILE) * mc_bin_tile_words(6, NW);
    if (q.bins) {                                                  // workgroup-uniform
        region_bin_replay<false, REG_S>(masks, any, 6, NW, q.bins + bin_at, tid, nullptr, false);
        __syncthreads();
    } else {
        const f3 Rc = face_texel_dir(face, min(tx * TILE + TILE / 2, p.size - 1), min(p.y0 + ty * TILE + TILE / 2, p.y0 + p.rows - 1), p.size);
        const f3 Tc = tangent_of(Rc);
        const f3 Bc = cross3(Tc, Rc);
        region_bin<true, true, false, true, true>(masks, any, dmax, 6, NW, 1, n + 1, n, R, T, B, Rc, Tc, Bc, tab, p.n_tab, tid, cmask, nullptr, NW,
                                                  0x7fffffff, false, 32 * REG_S);
        __syncthreads();
        if (q.bins_out) {
            region_bin_record(masks, 6, NW, q.bins_out + bin_at, tid);
            __syncthreads();                                       // the words change below
        }
    }
    if (STATS) {                                                   // the counters of k_mc_region's binning, in its units
        unsigned fl = 0;
        for (int k = tid; k < 6 * NW; k += 1024) fl += __popc(masks[k]);
        if (fl) atomicAdd(&q.stats[2], (unsigned long long)fl);
        if (tid < NW) { const unsigned c = __popc(cmask[tid]); if (c) atomicAdd(&q.stats[17], (unsigned long long)c); }
        if (tid == 0) { atomicAdd(&q.stats[3], (unsigned long long)p.n_tab); unsigned v = 0; for (int r = 0; r < 6; ++r) v += any[r] != 0u; atomicAdd(&q.stats[4], (unsigned long long)v); }
    }
    // masks[f][w] &= cmask[w]: the proved samples of face f (one face each: SOLE); cmask[w] = every other sample of the word.  Thread w
    // alone touches word w of the seven arrays.
    if (tid < NW) {
        const unsigned c = cmask[tid];
#pragma unroll
        for (int f = 0; f < 6; ++f) masks[f * NW + tid] &= c;
        const int left = p.n_tab - (tid << 5);
        cmask[tid] = ~c & (left >= 32 ? ~0u : (1u << left) - 1u);
    }
    __syncthreads();

    // ---- 3. proved runs, face by face in index order; 4. everything else once, each lane on its own face ----
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    [[maybe_unused]] unsigned viol = 0u, taken = 0u, rest = 0u;
    if (__builtin_amdgcn_readfirstlane((int)any[0])) resident_face<0, REG_S, FOLD, STATS>(masks, NW, s, tab, lds_base, R, T, B, nf, ar, ag, ab, viol, taken);
    if (__builtin_amdgcn_readfirstlane((int)any[1])) resident_face<1, REG_S, FOLD, STATS>(masks + NW, NW, s, tab, lds_base, R, T, B, nf, ar, ag, ab, viol, taken);
    if (__builtin_amdgcn_readfirstlane((int)any[2])) resident_face<2, REG_S, FOLD, STATS>(masks + 2 * NW, NW, s, tab, lds_base, R, T, B, nf, ar, ag, ab, viol, taken);
    if (__builtin_amdgcn_readfirstlane((int)any[3])) resident_face<3, REG_S, FOLD, STATS>(masks + 3 * NW, NW, s, tab, lds_base, R, T, B, nf, ar, ag, ab, viol, taken);
    if (__builtin_amdgcn_readfirstlane((int)any[4])) resident_face<4, REG_S, FOLD, STATS>(masks + 4 * NW, NW, s, tab, lds_base, R, T, B, nf, ar, ag, ab, viol, taken);
    if (__builtin_amdgcn_readfirstlane((int)any[5])) resident_face<5, REG_S, FOLD, STATS>(masks + 5 * NW, NW, s, tab, lds_base, R, T, B, nf, ar, ag, ab, viol, taken);
    {
        const float off = 0.5f * nf + 0.5f, basef = (float)lds_base;
        unsigned mnext = s < NW ? (unsigned)__builtin_amdgcn_readfirstlane((int)cmask[s]) : 0u;
        for (int w = s; w < NW; w += REG_S) {
            const unsigned m = mnext;
            mnext = w + REG_S < NW ? (unsigned)__builtin_amdgcn_readfirstlane((int)cmask[w + REG_S]) : 0u;
            if (STATS) rest += (unsigned)__builtin_popcount(m);
            if (m == 0u) continue;
            float wr = 0.0f, wg = 0.0f, wb = 0.0f;                 // word sums, as in resident_face
            each_sample(m, tab + (w << 5), [&](const v4f e) { general_sample(e, R, T, B, nf, off, basef, wr, wg, wb); });
            ar += wr; ag += wg; ab += wb;
        }
    }
    if (STATS) {
        // [1]: wave-slices (none is ever recomputed: [0] stays); [16]: (lane, sample) pairs whose proof did not hold; [18], [19]: pairs
        // taken by the proved runs / by the general pass -- together n_tab per texel
        if (viol) atomicAdd(&q.stats[16], (unsigned long long)viol);
        if ((tid & 63) == 0) { atomicAdd(&q.stats[1], 1ull); atomicAdd(&q.stats[18], 64ull * taken); atomicAdd(&q.stats[19], 64ull * rest); }
    }

    // ---- 5. combine the slices and store: the tree, the divisor and the alpha of k_mc_region ----
    __syncthreads();                                               // everybody is done with the level
    float* red = (float*)smem_v;
    reduce_slices<REG_TX, REG_S>(red, s, t, ar, ag, ab);
    if (x < p.size && y >= g.ys && y < g.ye && s == 0) {
        float4 o;
        o.x = red[t * 3 + 0] / p.divisor; o.y = red[t * 3 + 1] / p.divisor; o.z = red[t * 3 + 2] / p.divisor; o.w = p.alpha;
        p.out[((size_t)face * p.size + y) * p.size + x] = o;
    }
}

// the visiting order of the region loops, for host-side checks: the k-th region a tile of `face` visits at G regions per face edge
extern "C" int pbrk_mc_region_order(int face, int G, int k) {
    if (face < 0 || face > 5 || G < 1 || k < 0 || k >= 6 * G * G) return -1;
    return mc_region_visit(k, face * (G * G), G * G);
}

static unsigned long long* g_reg_stats = nullptr;      // device counters, enabled by PBR_MC_STATS=1
#define REG_STATS_BYTES 160                            // 20 slots (RegArgs::stats; [16..19]: k_mc_resident)

// out[0 .. count) = the device counters RegArgs::stats[first_slot ..]
static int read_stats(unsigned long long* out, int first_slot, int count) {
    if (!g_reg_stats || !out) return PBRK_E_ARG;
    return hipMemcpy(out, g_reg_stats + first_slot, (size_t)count * 8, hipMemcpyDeviceToHost) == hipSuccess ? PBRK_OK : PBRK_E_LAUNCH;
}
extern "C" int pbrk_mc_region_stats(unsigned long long* out2, int reset) {
    const int rc = read_stats(out2, 0, 2);
    if (rc != PBRK_OK) return rc;
    return (reset && hipMemset(g_reg_stats, 0, REG_STATS_BYTES) != hipSuccess) ? PBRK_E_LAUNCH : PBRK_OK;
}
extern "C" int pbrk_mc_region_skip_stats(unsigned long long* out3) { return read_stats(out3, 6, 3); }        // absorbed words: see RegArgs::stats [6..8]
extern "C" int pbrk_mc_region_window_stats(unsigned long long* out1) { return read_stats(out1, 5, 1); }      // samples run through the test-free body (sum over tiles)
extern "C" int pbrk_mc_region_flag_stats(unsigned long long* out3) { return read_stats(out3, 2, 3); }
extern "C" int pbrk_mc_region_phase_stats(unsigned long long* out5) { return read_stats(out5, 9, 5); }       // PBR_MC_PHASE_STAMPS builds; zeros otherwise (RegArgs::stats [9..13])
// PBR_MC_STATS=1, since the last reset: {(lane, sample) pairs whose proof did not hold (must stay 0), proved samples summed over
// tiles, pairs taken by the proved runs, pairs taken by the general pass}
extern "C" int pbrk_mc_resident_stats(unsigned long long* out4) { return read_stats(out4, 16, 4); }

// The device counters (PBR_MC_STATS=1), or null
static unsigned long long* reg_stats() {
    static int stats_on = -1;
    if (stats_on < 0) {
        stats_on = mc_counters_wanted() ? 1 : 0;
        if (stats_on) { if (hipMalloc(&g_reg_stats, REG_STATS_BYTES) != hipSuccess) g_reg_stats = nullptr; else (void)hipMemset(g_reg_stats, 0, REG_STATS_BYTES); }
    }
    return g_reg_stats;
}

// ---- plan -> launch: the thin launchers of the three kernel families.  Every decision is mc_plan's (mc_plan.cpp) ----
template <int RS, bool SUB, int TILE, bool RUNS = false, bool LEAN = false, bool FOLD = false, bool NET = true>
static void launch_region_t(const RegArgs& q, unsigned grid, size_t lds, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) { (void)hipFuncSetAttribute((const void*)k_mc_region<RS, SUB, TILE, RUNS, LEAN, FOLD, NET>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr_set = true; }
    hipLaunchKernelGGL((k_mc_region<RS, SUB, TILE, RUNS, LEAN, FOLD, NET>), dim3(grid), dim3(1024), lds, st, q);
}

// The instantiation of shape SH that the plan's (runs, lean, fold, net) name.  FOLD and NET = false exist for the lean run loops only
// (header 2j, 2l), the run loop on the shapes that have it (2i).
template <class SH>
static void launch_region_shape(const McPlan& p, const RegArgs& q, unsigned grid, hipStream_t st) {
    constexpr int RS = SH::RS, TILE = SH::TILE;
    constexpr bool SUB = SH::SUB;
    const size_t lds = (size_t)p.lds;
    if constexpr (SH::HAS_RUNS) {
        if (p.runs && p.lean) {
            if constexpr (SH::NET_OFF) {
                if (!p.net) {
                    if (p.fold) launch_region_t<RS, SUB, TILE, true, true, true, false>(q, grid, lds, st);
                    else launch_region_t<RS, SUB, TILE, true, true, false, false>(q, grid, lds, st);
                    return;
                }
            }
            if (p.fold) launch_region_t<RS, SUB, TILE, true, true, true>(q, grid, lds, st);
            else launch_region_t<RS, SUB, TILE, true, true>(q, grid, lds, st);
            return;
        }
        if (p.runs) { launch_region_t<RS, SUB, TILE, true, false>(q, grid, lds, st); return; }
    }
    if (p.lean) launch_region_t<RS, SUB, TILE, false, true>(q, grid, lds, st);
    else launch_region_t<RS, SUB, TILE, false, false>(q, grid, lds, st);
}

// Behind a recording launch (t.entry >= 0) on its stream, ahead of the event replays wait for; the token holds the cache's lock.
// q: the recording launch's arguments -- a whole-level dispatch.  FOLD: the flavour the replays will take.  Returns whether it ran.
static bool launch_refine(const McPlan& p, const RegArgs& q, const McBinToken& t, hipStream_t st) {
    if (t.entry < 0 || !p.refine) return false;
    RefineArgs g;
    g.a = q.a;
    g.G = q.G; g.RC = q.RC; g.NR = q.NR; g.NW = q.NW;
    g.bins = t.record;
    g.out = mc_bins_refine_stats(t);
    if (!g.out) return false;
    const unsigned grid = (unsigned)(6 * q.a.tiles_x * q.a.tiles_x);
    const size_t lds = mc_refine_lds(p.NR, p.NW);
    mc_for_shape(p.RS, p.G, p.tile, [&](auto sh) {
        using SH = decltype(sh);
        if constexpr (SH::HAS_RUNS) {                               // the 18^2 shape never records
            if (p.fold) hipLaunchKernelGGL((k_mc_refine_bins<SH::RS, SH::SUB, SH::TILE, true>), dim3(grid), dim3(1024), lds, st, g);
            else hipLaunchKernelGGL((k_mc_refine_bins<SH::RS, SH::SUB, SH::TILE, false>), dim3(grid), dim3(1024), lds, st, g);
        }
    });
    return true;
}

// RegArgs from the plan: the fields both families fill.  tiles_y tile rows from row y0 of the face.
static void fill_args(RegArgs& q, const McArgs& a, const McPlan& p, int y0, int rows, int tiles_y) {
    q.a = a;
    q.G = p.G; q.RC = p.RC; q.NR = p.NR; q.NW = p.NW;
    for (int s = 0; s < REG_MAX_S; ++s) q.expect[s] = p.expect[s];
    q.tabmax = nullptr; q.cut = 0; q.absorb = p.absorb;
    q.stats = reg_stats();
    q.a.y0 = y0; q.a.rows = rows;
    q.a.tiles_x = (a.size + p.tile - 1) / p.tile;
    q.a.tiles_per_face = q.a.tiles_x * tiles_y;
    mc_pole_rows(a.size, y0, p.tile, tiles_y, q.pole_row);
}

// plan; prep and bin resources; arguments; launch.  The cache's lock is held from ahead of k_mc_prep until the launch, its refine pass and
// its event are enqueued; the prep ring's from the slot's acquisition until the event behind its reader.
bool launch_mc_region(McArgs a, int nfaces, hipStream_t st) {
    const McSwitches sw = mc_switches();
    const bool counters = reg_stats() != nullptr;
    McPlan p = mc_plan(sw, a.n_src, a.n_tab, a.size, a.face0, nfaces, a.y0, a.rows, counters, true);
    if (p.family != MC_REGION) return false;
    McBinToken bins = mc_bins_begin();
    McPrepSlot prep;
    if (p.prep) {
        prep = mc_prep_acquire(st);
        // no slot (see prep_acquire): the launch takes the prologue that builds the maxima itself -- the same bytes
        if (!prep.words) p = mc_plan(sw, a.n_src, a.n_tab, a.size, a.face0, nfaces, a.y0, a.rows, counters, false);
    }
    RegArgs q;
    fill_args(q, a, p, a.y0, a.rows, (a.rows + p.tile - 1) / p.tile);         // tiles start at the dispatch's first row, whatever it is
    g_mc_last.plan = p; g_mc_last.cut = nullptr;
    if (p.prep) {
        mc_prep_launch(prep, a, p, st);
        q.tabmax = prep.words;
        if (p.cut) { q.cut = 3; g_mc_last.cut = prep.words + p.NW + p.NR; }
    }
    mc_bins_plan(bins, a, p, st);
    q.bins = bins.replay; q.bins_out = bins.record;
    const unsigned grid = (unsigned)(q.a.tiles_per_face * nfaces);
    mc_for_shape(p.RS, p.G, p.tile, [&](auto sh) { launch_region_shape<decltype(sh)>(p, q, grid, st); });
    if (bins.entry >= 0) g_mc_last.refined = launch_refine(p, q, bins, st) ? 1 : 0;
    mc_bins_end(bins, st);
    mc_prep_release(prep, st);
    return true;
}

template <int TILE, bool FOLD, bool STATS>
static void launch_resident_t(const ResArgs& g, unsigned grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((k_mc_resident<TILE, FOLD, STATS>), dim3(grid), dim3(1024), lds, st, g);
}
template <int TILE>
static void launch_resident_tile(const ResArgs& g, bool fold, unsigned grid, size_t lds, hipStream_t st) {
    if (g.q.stats) { if (fold) launch_resident_t<TILE, true, true>(g, grid, lds, st); else launch_resident_t<TILE, false, true>(g, grid, lds, st); }
    else { if (fold) launch_resident_t<TILE, true, false>(g, grid, lds, st); else launch_resident_t<TILE, false, false>(g, grid, lds, st); }
}

// The tiles are anchored at row 0 of the face, not at the dispatch's first row: a texel sits in the same tile, with the same proof and the
// same order of its sum, in every dispatch that holds it, so a row shard equals the full dispatch bit for bit.  A dispatch that starts or
// ends inside a tile computes the whole tile and stores its own rows.
bool launch_mc_resident(McArgs a, int nfaces, hipStream_t st) {
    const McPlan p = mc_plan(mc_switches(), a.n_src, a.n_tab, a.size, a.face0, nfaces, a.y0, a.rows, reg_stats() != nullptr, true);
    if (p.family != MC_RESIDENT) return false;
    McBinToken bins = mc_bins_begin();
    ResArgs g;
    RegArgs& q = g.q;
    const int tile = p.tile, ty0 = a.y0 / tile, ty1 = (a.y0 + a.rows - 1) / tile;
    g.ys = a.y0; g.ye = a.y0 + a.rows;
    fill_args(q, a, p, ty0 * tile, ((ty1 + 1) * tile < a.size ? (ty1 + 1) * tile : a.size) - ty0 * tile, ty1 - ty0 + 1);
    // header 2m: every dispatch may replay; a whole-level one records
    mc_bins_plan(bins, a, p, st);
    q.bins = bins.replay; q.bins_out = bins.record;
    const unsigned grid = (unsigned)(q.a.tiles_per_face * nfaces);
    if (tile == 16) launch_resident_tile<16>(g, p.fold != 0, grid, (size_t)p.lds, st);
    else launch_resident_tile<8>(g, p.fold != 0, grid, (size_t)p.lds, st);
    mc_bins_end(bins, st);
    return true;
}
