// acmmp_vp_plan.h — where the view-parallel driver (acmmp_vp.cpp) puts its
// views: which rank owns a view, which views every rank computes a row band
// of, the rows of a band, and a view's slot in the padded all-gathers. The
// same rules as acmmp_amd/distributed.py (plan_views, _check_split,
// DepthExchange) and acmmp_amd/band.py (bands); tests/test_asan.py compares
// the two. Host-only and header-only: no device or collective header, so the
// plan runs in a CPU test.
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "../../include/acmmp.h"

namespace acmmp_vp {

struct Plan {
    std::vector<std::vector<int>> assignment;  // per rank, ascending: the views whose image / depth slot
                                               // and .dmb files are that rank's
    std::vector<int> split;                    // ascending: the views every rank computes a band of
    int slots = 1;                             // slots per rank in a padded all-gather
    std::vector<int> slot;                     // per view: owner rank * slots + position in the owner's list

    const std::vector<int> &owned(int rank) const { return assignment[(size_t)rank]; }
    bool is_split(int v) const { return std::binary_search(split.begin(), split.end(), v); }
    // the views `rank` computes whole: owned minus split
    std::vector<int> mine(int rank) const {
        std::vector<int> m;
        for (int v : owned(rank))
            if (!is_split(v)) m.push_back(v);
        return m;
    }

    // The halo rule, applied once with the heights of the coarsest scale
    // (later scales are larger): a view stays split only if every band holds
    // the halo; otherwise its owner computes it whole.
    void apply_halo_rule(const std::vector<int> &height) {
        const int world = (int)assignment.size();
        split.erase(std::remove_if(split.begin(), split.end(),
                                   [&](int v) { return height[(size_t)v] < world * ACMMP_BAND_HALO; }),
                    split.end());
    }
};

// LPT on `costs`: views by cost descending, then index ascending, each to the
// least loaded rank (lowest rank on ties). With split_tail the n % world
// cheapest views are split over all ranks instead, and each gets an owner
// the same way after the whole views are placed, in ascending index.
inline Plan plan_views(const std::vector<double> &costs, int world, bool split_tail) {
    const int n = (int)costs.size();
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        return costs[(size_t)a] != costs[(size_t)b] ? costs[(size_t)a] > costs[(size_t)b] : a < b;
    });
    Plan p;
    const int ntail = (split_tail && world > 1) ? n % world : 0;
    p.split.assign(order.end() - ntail, order.end());
    std::sort(p.split.begin(), p.split.end());
    std::vector<double> load((size_t)world, 0.0);
    p.assignment.assign((size_t)world, {});
    auto place = [&](int v) {
        int r = 0;
        for (int k = 1; k < world; ++k)
            if (load[(size_t)k] < load[(size_t)r]) r = k;
        p.assignment[(size_t)r].push_back(v);
        load[(size_t)r] += costs[(size_t)v];
    };
    for (int v : order)
        if (!p.is_split(v)) place(v);
    for (int v : p.split) place(v);
    p.slot.assign((size_t)n, 0);
    for (auto &a : p.assignment) {
        std::sort(a.begin(), a.end());
        p.slots = std::max(p.slots, (int)a.size());
    }
    for (int r = 0; r < world; ++r)
        for (size_t k = 0; k < p.assignment[(size_t)r].size(); ++k)
            p.slot[(size_t)p.assignment[(size_t)r][k]] = r * p.slots + (int)k;
    return p;
}

// rows [lo, hi) of band k of H rows over `world` bands (sizes differ by at most 1)
inline std::pair<int, int> band_rows(int H, int world, int k) {
    const int base = H / world, extra = H % world;
    const int lo = k * base + std::min(k, extra);
    return {lo, lo + base + (k < extra ? 1 : 0)};
}

// One padded all-gather of a map per view, [world * slots, hmax, wmax] floats
// with row pitch wmax (RCCL has no all-gatherv): every rank sends
// [slots, hmax, wmax], its k-th view in slot k.
struct GatherLayout {
    const Plan *plan = nullptr;
    int hmax = 0, wmax = 0;  // the largest view's size
    size_t map_floats() const { return (size_t)hmax * wmax; }
    size_t send_floats() const { return (size_t)plan->slots * map_floats(); }
    size_t recv_floats() const { return plan->assignment.size() * send_floats(); }
    // float offset of view v's slot in the gathered buffer, and in its owner's send buffer
    size_t recv_offset(int v) const { return (size_t)plan->slot[(size_t)v] * map_floats(); }
    size_t send_offset(int v) const { return (size_t)(plan->slot[(size_t)v] % plan->slots) * map_floats(); }
};

}  // namespace acmmp_vp
