// Host build of csrc/mc_refine_core.h (the word logic of k_mc_refine_bins, k_mc_region.hip 2n) for tests/test_mc_exact_bins_cpu.py:
//   mc_refine_core_host in.bin out.bin
// in.bin:  int32 {NR, waves, cases}, then per case uint32 old[NR], uint32 proved, int8 region[waves][32][64] -- the region lane l of
//          wave v takes sample i in, or -1 for none.
// out.bin: per case uint32 {need, out[NR], proof, unset}.
// The waves are walked as the kernel walks them: per region and wave one mc_refine_ballot per needed sample, the waves' words ORed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mc_refine_core.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[3];
    if (fread(head, 4, 3, f) != 3) { fclose(f); return 3; }
    const int NR = head[0], waves = head[1], cases = head[2];
    if (NR < 1 || NR > 64 || waves < 1 || waves > 16 || cases < 0) { fclose(f); return 3; }
    std::vector<uint32_t> result;
    std::vector<unsigned> old((size_t)NR), hit((size_t)NR), part((size_t)NR);
    std::vector<int8_t> region((size_t)waves * 32 * 64);
    for (int c = 0; c < cases; ++c) {
        uint32_t proved;
        if (fread(old.data(), 4, (size_t)NR, f) != (size_t)NR || fread(&proved, 4, 1, f) != 1 || fread(region.data(), 1, region.size(), f) != region.size()) {
            fclose(f);
            return 3;
        }
        const unsigned need = mc_refine_need(old.data(), 1, NR, proved);
        for (int r = 0; r < NR; ++r) {
            hit[(size_t)r] = part[(size_t)r] = 0u;
            for (int v = 0; v < waves; ++v) {
                unsigned h = 0u, pt = 0u;
                for (int i = 0; i < 32; ++i) {
                    if (!((need >> i) & 1u)) continue;
                    unsigned long long b = 0ull;
                    for (int l = 0; l < 64; ++l)
                        if (region[((size_t)v * 32 + (size_t)i) * 64 + (size_t)l] == r) b |= 1ull << l;
                    mc_refine_ballot(b, i, h, pt);
                }
                hit[(size_t)r] |= h;
                part[(size_t)r] |= pt;
            }
        }
        unsigned long long unset = 0ull;
        // out aliases hit, as in the kernel
        const unsigned proof = mc_refine_word(old.data(), 1, NR, proved, need, hit.data(), part.data(), 1, hit.data(), 1, &unset);
        result.push_back(need);
        for (int r = 0; r < NR; ++r) result.push_back(hit[(size_t)r]);
        result.push_back(proof);
        result.push_back((uint32_t)unset);
    }
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = fwrite(result.data(), 4, result.size(), f) == result.size();
    return (fclose(f) == 0 && ok) ? 0 : 4;
}
