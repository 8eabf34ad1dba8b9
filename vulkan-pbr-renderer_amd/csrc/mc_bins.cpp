// mc_bins.cpp -- header 2m of k_mc_region.hip: the bin cache (mc_bins.h).
// What binning computes depends on the tile's geometry, the level's shape and the sample table, never on a texel: one buffer per
// (device, kernel shape, n_src, output size, n_entries, table, generation) holds every tile's flags, written by the first whole-level
// launch and read by every eligible launch after it.  A raw table pointer says nothing about its contents, so only tables registered as
// immutable (pbrk_mc_table_register) are served; each registration is a new generation.  No eviction: an entry that would pass the budget
// is not created.  One lock orders lookup, creation and the event behind the recording launch; a replay on any stream waits for that event.
#include "mc_bins.h"

#include <vector>

struct BinTable { const void* ptr; int n; unsigned long long gen; };
struct BinEntry {
    int dev, flavour, n_src, size, n_tab; const void* tab; unsigned long long gen;
    unsigned* buf; size_t bytes; hipEvent_t ready; bool done;
};
static std::vector<BinTable> g_bin_tables;
static std::vector<BinEntry> g_bin_entries;
static std::mutex g_bin_lock;
static size_t g_bin_budget = (size_t)512 << 20;
static unsigned long long g_bin_gen = 0;
static unsigned long long g_bin_count[4];               // recording launches, replaying launches, computed though the cache was on, declined for the budget

static void bin_entry_free(BinEntry& e) { (void)hipFree(e.buf); (void)hipEventDestroy(e.ready); }   // hipFree waits for the device

extern "C" void pbrk_mc_set_bin_cache_budget(size_t bytes) { std::lock_guard<std::mutex> hold(g_bin_lock); g_bin_budget = bytes; }
extern "C" void pbrk_mc_bin_cache_clear(void) {
    std::lock_guard<std::mutex> hold(g_bin_lock);
    for (BinEntry& e : g_bin_entries) bin_entry_free(e);
    g_bin_entries.clear();
}
extern "C" void pbrk_mc_bin_cache_stats(unsigned long long out[5]) {
    if (!out) return;
    std::lock_guard<std::mutex> hold(g_bin_lock);
    for (int i = 0; i < 4; ++i) out[i] = g_bin_count[i];
    out[4] = 0;
    for (const BinEntry& e : g_bin_entries) out[4] += e.bytes;
}
extern "C" int pbrk_mc_table_unregister(const void* table4) {
    if (!table4) return PBRK_E_ARG;
    std::lock_guard<std::mutex> hold(g_bin_lock);
    for (size_t i = 0; i < g_bin_tables.size(); ++i)
        if (g_bin_tables[i].ptr == table4) {
            g_bin_tables.erase(g_bin_tables.begin() + (long)i);
            // the entries recorded with this registration can never be asked for again
            for (size_t k = g_bin_entries.size(); k-- > 0;)
                if (g_bin_entries[k].tab == table4) { bin_entry_free(g_bin_entries[k]); g_bin_entries.erase(g_bin_entries.begin() + (long)k); }
            return PBRK_OK;
        }
    return PBRK_E_ARG;
}
extern "C" int pbrk_mc_table_register(const void* table4, int n_entries) {
    if (!table4 || n_entries < 1) return PBRK_E_ARG;
    (void)pbrk_mc_table_unregister(table4);                         // registered again: a new generation
    std::lock_guard<std::mutex> hold(g_bin_lock);
    g_bin_tables.push_back({table4, n_entries, ++g_bin_gen});
    return PBRK_OK;
}
extern "C" int pbrk_mc_tile_of_block(int block, int size, int tile, int face0, int nfaces, int y0, int y1, int* out4) {
    if (!out4 || size < 1 || (tile != 8 && tile != 16 && tile != 32) || face0 < 0 || nfaces < 1 || face0 + nfaces > 6 || y0 < 0 || y0 >= y1 || y1 > size) return PBRK_E_ARG;
    const int tiles_x = (size + tile - 1) / tile, tiles_y = (y1 - y0 + tile - 1) / tile;
    if (block < 0 || block >= tiles_x * tiles_y * nfaces) return PBRK_E_ARG;
    int pole_row[2];
    mc_pole_rows(size, y0, tile, tiles_y, pole_row);
    mc_tile_of_block((unsigned)block, face0, tiles_x, tiles_x * tiles_y, pole_row, out4[0], out4[1], out4[2]);
    out4[3] = (int)mc_bin_tile_index(out4[0], y0 / tile, out4[2], out4[1], tiles_x, tiles_x);
    return PBRK_OK;
}
extern "C" int pbrk_mc_bin_window_eligible(int size, int tile, int y0, int y1) { return mc_bin_window_ok(size, tile, y0, y1) ? 1 : 0; }

McBinToken mc_bins_begin() {
    McBinToken t;
    t.hold = std::unique_lock<std::mutex>(g_bin_lock);
    return t;
}

// p.bin_eligible: a participating kernel shape and a row window whose tiles are those of the whole-level dispatch; p.whole: all six faces, all rows.
void mc_bins_plan(McBinToken& t, const McArgs& a, const McPlan& p, hipStream_t st) {
    t.replay = nullptr; t.record = nullptr; t.entry = -1;
    if (!p.bin_cache) return;
    int dev = 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const BinTable* bt = nullptr;
    for (const BinTable& b : g_bin_tables) if (b.ptr == (const void*)a.tab && a.n_tab <= b.n) bt = &b;
    if (!p.bin_eligible || !bt || hipGetDevice(&dev) != hipSuccess || hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        ++g_bin_count[2];
        return;
    }
    size_t held = 0;
    for (BinEntry& e : g_bin_entries) {
        if (e.dev != dev) continue;
        held += e.bytes;
        if (e.flavour == p.bin_flavour && e.n_src == a.n_src && e.size == a.size && e.n_tab == a.n_tab && e.tab == bt->ptr && e.gen == bt->gen) {
            if (!e.done) {
                if (hipEventQuery(e.ready) == hipSuccess) e.done = true;
                else { (void)hipGetLastError(); if (hipStreamWaitEvent(st, e.ready, 0) != hipSuccess) { (void)hipGetLastError(); ++g_bin_count[2]; return; } }
            }
            t.replay = e.buf;
            ++g_bin_count[1];
            return;
        }
    }
    if (!p.whole) { ++g_bin_count[2]; return; }                   // entries are recorded by whole-level launches only
    const size_t tiles_e = (size_t)((a.size + p.tile - 1) / p.tile);
    BinEntry e = {dev, p.bin_flavour, a.n_src, a.size, a.n_tab, bt->ptr, bt->gen, nullptr, 6 * tiles_e * tiles_e * mc_bin_tile_words(p.NR, p.NW) * 4, nullptr, false};
    if (held + e.bytes > g_bin_budget) { ++g_bin_count[3]; ++g_bin_count[2]; return; }
    if (hipMalloc(&e.buf, e.bytes) != hipSuccess) { (void)hipGetLastError(); ++g_bin_count[3]; ++g_bin_count[2]; return; }
    if (hipEventCreateWithFlags(&e.ready, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(e.buf); ++g_bin_count[2]; return; }
    g_bin_entries.push_back(e);
    t.record = e.buf;
    ++g_bin_count[0];
    t.entry = (int)g_bin_entries.size() - 1;
}
// Without the event the entry cannot be trusted: it goes.
void mc_bins_end(McBinToken& t, hipStream_t st) {
    if (t.entry >= 0 && hipEventRecord(g_bin_entries[(size_t)t.entry].ready, st) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        bin_entry_free(g_bin_entries[(size_t)t.entry]);
        g_bin_entries.erase(g_bin_entries.begin() + t.entry);
    }
    t.entry = -1;
    t.hold.unlock();
}

// ---- header 2n: the counters of k_mc_refine_bins ----
static unsigned long long* g_exact_stats[MC_MAX_DEVICES];       // RefineArgs::out, one per device
unsigned long long* mc_bins_refine_stats(const McBinToken& t) {
    int dev = 0;
    if (!t.hold.owns_lock() || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MC_MAX_DEVICES) { (void)hipGetLastError(); return nullptr; }
    if (!g_exact_stats[dev]) {
        if (hipMalloc(&g_exact_stats[dev], 64) != hipSuccess) { (void)hipGetLastError(); g_exact_stats[dev] = nullptr; return nullptr; }
        (void)hipMemset(g_exact_stats[dev], 0, 64);
    }
    return g_exact_stats[dev];
}
extern "C" int pbrk_mc_exact_bins_stats(unsigned long long* out8, int reset) {
    if (!out8) return PBRK_E_ARG;
    std::lock_guard<std::mutex> hold(g_bin_lock);
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    for (int d = 0; d < MC_MAX_DEVICES; ++d) {
        if (!g_exact_stats[d]) continue;
        unsigned long long v[8];
        if (hipMemcpy(v, g_exact_stats[d], sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return PBRK_E_LAUNCH;
        for (int i = 0; i < 8; ++i) out8[i] += v[i];
        if (reset && hipMemset(g_exact_stats[d], 0, sizeof v) != hipSuccess) return PBRK_E_LAUNCH;
    }
    return PBRK_OK;
}
