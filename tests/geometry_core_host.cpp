// Brute-force rasteriser (no tiles, no bins) over csrc/geometry_core.h compiled for the host: tests/test_geometry_core_host.py builds it
// and compares it with the numpy reference, so the header the kernels are made of is pinned on the CPU too.
#include "geometry_core.h"
#include <vector>
extern "C" int geo_host_raster(const PbrkGeoDraw* draws, int ndraws, const uint32_t* tri_counts, int W, int H,
                               uint8_t* c0, uint8_t* c1, uint8_t* c2, uint8_t* c3, uint16_t* vel_unused, float* velf, float* depth, int* winner) {
    int rejected = 0; unsigned t = 0;
    std::vector<GeoAttr> attrs; std::vector<std::vector<GeoCov>> covs;
    for (int d = 0; d < ndraws; ++d) for (unsigned k = 0; k < tri_counts[d]; ++k, ++t) {
        const PbrkGeoDraw& D = draws[d];
        const uint32_t* ix = D.indices + D.first_index + 3 * k;
        GeoAttr A; memset(&A, 0, sizeof A); GeoCov cov[6]; int n = 0; bool ok = true; const float* v[3];
        for (int q = 0; q < 3; ++q) { unsigned long long vi = (unsigned long long)ix[q] + D.vertex_offset; if (vi >= D.vertex_count) { ok = false; break; } v[q] = (const float*)D.vertices + vi * 11; }
        if (ok) n = geo_setup(D, v[0], v[1], v[2], W, H, A, cov);
        if (!ok || n < 0) { rejected++; n = 0; }
        A.draw = d; attrs.push_back(A); covs.push_back(std::vector<GeoCov>(cov, cov + (n > 0 ? n : 0)));
    }
    for (int j = 0; j < H; ++j) for (int i = 0; i < W; ++i) {
        float bz = depth[j * W + i]; int bt = -1;
        for (unsigned s = 0; s < attrs.size(); ++s) {
            bool cv = false; for (auto& c : covs[s]) cv = cv || geo_covers(c, i, j);
            if (!cv) continue;
            double lam[3]; float z; geo_lambda(attrs[s], i, j, W, H, lam);
            if (!geo_depth(attrs[s], lam, &z)) continue;
            if (!(z < bz)) continue;
            GeoPix P; geo_pix(attrs[s], i, j, W, H, P);
            if (geo_alpha(draws[attrs[s].draw], P) < 0.3f) continue;
            bz = z; bt = (int)s;
        }
        winner[j * W + i] = bt;
        if (bt < 0) continue;
        GeoPix P; GeoOut o; geo_pix(attrs[bt], i, j, W, H, P); geo_shade(draws[attrs[bt].draw], attrs[bt], P, i, j, W, H, o);
        size_t p = (size_t)j * W + i;
        memcpy(c0 + 4 * p, o.base, 4); memcpy(c1 + 4 * p, o.nrm, 4); memcpy(c2 + 4 * p, o.orm, 4); memcpy(c3 + 4 * p, o.emi, 4);
        velf[2 * p] = o.vel[0]; velf[2 * p + 1] = o.vel[1]; depth[p] = bz;
    }
    return rejected;
}
