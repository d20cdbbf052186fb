// How the Galerkin kernel (sagg.hip) cuts a row of R into groups, and what a coarse row needs to share a wavefront with
// three others.  Plain C++ for host and device: tools/galerkin_groups_host_check.cpp runs the rule on the CPU.
//
// A group starts at entry t0 of the row.  Its candidates are the next entries, as many as the entry cap, the lanes and
// the row allow; candidate k is kept when the products of candidates 0..k fit the list.  The first candidate is always
// kept (a row of A P has at most as many entries as the list has slots: the caller's business), so every group takes
// at least one entry.  The prefix sums grow with k, so the kept candidates are a prefix and their count is the group's
// size, whichever lane counts them.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GALERKIN_HD __host__ __device__
#else
#define GALERKIN_HD
#endif

struct GalerkinCaps {
    int entries;   // most R entries of a group (NODAL_SA_GG at 16-slot levels when set, else the lanes)
    int lanes;     // one R entry per lane
    int products;  // slots of the LDS list
};

// capacities of the shared path: a sub-group of 16 lanes per coarse row, four rows per wavefront
constexpr int GALERKIN_SUB_LANES = 16;
constexpr int GALERKIN_SUB_ROWS = 4;
constexpr int GALERKIN_SUB_ENTRIES = 32;    // R entries (two per lane)
constexpr int GALERKIN_SUB_PRODUCTS = 128;  // a sub-group's share of the list
constexpr int GALERKIN_SUB_COLUMNS = 16;    // columns of the coarse row (one per lane)
constexpr int GALERKIN_SUB_STRIDE = GALERKIN_SUB_PRODUCTS + 8;  // (the accumulation reads eight products per step)

GALERKIN_HD inline int galerkin_group_candidates(int remaining, const GalerkinCaps &c) {
    int n = remaining < c.entries ? remaining : c.entries;
    n = n < c.lanes ? n : c.lanes;
    return n > 0 ? n : 0;
}

// prefix: products of candidates 0..k of the group
GALERKIN_HD inline bool galerkin_group_keeps(int k, int candidates, int prefix, const GalerkinCaps &c) {
    return k < candidates && (k == 0 || prefix <= c.products);
}

// the most R entries a row of the shared path may have: NODAL_SA_GG still bounds a group
GALERKIN_HD inline int galerkin_sub_entries(int entry_cap) {
    return entry_cap < GALERKIN_SUB_ENTRIES ? entry_cap : GALERKIN_SUB_ENTRIES;
}
