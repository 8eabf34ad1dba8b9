// mc_bins.h -- the bin cache of the region and resident kernels (k_mc_region.hip, header 2m and 2n): the host side.
// One lock orders lookup, creation, the refine pass and the event behind a recording launch.  The lock IS the token: a launcher takes
// it with mc_bins_begin ahead of its first launch, and only mc_bins_end, behind its last, gives it back.
#pragma once
#include "k_mc_internal.h"
#include "mc_plan.h"

#include <mutex>

struct McBinToken {
    std::unique_lock<std::mutex> hold;
    int entry = -1;                     // >= 0: this launch records entry `entry`
    const unsigned* replay = nullptr;   // RegArgs::bins
    unsigned* record = nullptr;         // RegArgs::bins_out; also what k_mc_refine_bins rewrites behind the recording launch
};
McBinToken mc_bins_begin();
// The cache's part in one launch of plan p: sets t.replay, or t.record and t.entry, or neither (compute as ever).
void mc_bins_plan(McBinToken& t, const McArgs& a, const McPlan& p, hipStream_t st);
// RefineArgs::out of the current device ([8], zeroed when first asked for), or null
unsigned long long* mc_bins_refine_stats(const McBinToken& t);
// behind the recording launch and its refine pass: the event a replay on another stream waits for.  Releases the lock.
void mc_bins_end(McBinToken& t, hipStream_t st);
