// rxr_ray_refresh.h -- the host side of a ranged refit of the ray box tree (rxr_ray_accel.hip): which nodes of
// every level lie above a set of dirty sorted positions.  Nothing here needs HIP: tests/ray_refresh_walk.cpp calls it on the CPU.
//
// The tree is implicit (rxr_ray_accel.hip): leaf i covers positions [i * L, (i + 1) * L), node i of a level covers nodes
// [i * W, (i + 1) * W) of the level below, a level of n nodes has (n + W - 1) / W parents, up to one root.  A node is dirty iff a dirty
// position lies below it.  Dirty positions come as ranges [begin, end) in increasing order (a mesh's triangles keep their range of
// sorted positions); per level the dirty nodes are disjoint intervals [lo, hi], also increasing, neighbours merged.
#pragma once
#include <cstdint>
#include <vector>

constexpr uint32_t RXR_REFIT_MAX_LEVELS = 24;   // ACCEL_MAX_LEVELS of rxr_ray_accel.hip

struct RxrRefitInterval {
    uint32_t lo, hi;   // nodes lo .. hi of the level, both included
};

struct RxrRefitPlan {
    uint32_t n_levels = 0;                                   // levels of the tree; level 0 = the leaves
    uint32_t cnt[RXR_REFIT_MAX_LEVELS] = {};                 // nodes of each level
    std::vector<RxrRefitInterval> iv[RXR_REFIT_MAX_LEVELS];  // the dirty intervals of each level
    uint32_t dirty[RXR_REFIT_MAX_LEVELS] = {};               // ... and how many nodes they hold
};

// appends [lo, hi] to `v`, merged with the last interval when it touches or overlaps it (lo is never below the last interval's lo)
inline void rxr_refit_append(std::vector<RxrRefitInterval> &v, uint32_t lo, uint32_t hi) {
    if (!v.empty() && lo <= v.back().hi + 1u) {
        if (hi > v.back().hi) v.back().hi = hi;
        return;
    }
    v.push_back(RxrRefitInterval{lo, hi});
}

// ranges: n pairs (begin, end) of sorted positions, increasing in begin, each within [0, ntri]; empty ranges are skipped.
// L positions per leaf, W nodes per parent (both at least 1; W at least 2 when there is more than one leaf).
inline RxrRefitPlan rxr_refit_plan(uint32_t ntri, uint32_t L, uint32_t W, const uint32_t *ranges, uint32_t n) {
    RxrRefitPlan P;
    if (!ntri) return P;
    uint32_t nodes = (ntri + L - 1) / L;
    for (;;) {
        P.cnt[P.n_levels++] = nodes;
        if (nodes <= 1 || P.n_levels == RXR_REFIT_MAX_LEVELS) break;
        nodes = (nodes + W - 1) / W;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = ranges[2 * i], e = ranges[2 * i + 1] < ntri ? ranges[2 * i + 1] : ntri;
        if (b >= e) continue;
        rxr_refit_append(P.iv[0], b / L, (e - 1) / L);
    }
    for (uint32_t k = 1; k < P.n_levels; ++k)
        for (const RxrRefitInterval &c : P.iv[k - 1]) rxr_refit_append(P.iv[k], c.lo / W, c.hi / W);
    for (uint32_t k = 0; k < P.n_levels; ++k)
        for (const RxrRefitInterval &c : P.iv[k]) P.dirty[k] += c.hi - c.lo + 1;
    return P;
}
