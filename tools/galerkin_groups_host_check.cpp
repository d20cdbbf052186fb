// Host check of nodal_amd/csrc/galerkin_groups.h, the rule that cuts a row of R into the Galerkin kernel's groups: the
// rule is run the way the wavefront runs it (every lane judges its own candidate from the prefix sum of the products,
// the kept candidates are counted) on random and degenerate rows, and every row must come out with each entry in
// exactly one group, no group above a cap, and the same boundary whichever lane order counts it.
// Build: g++ -O1 -std=c++17 -fsanitize=address,undefined -o galerkin_groups_host_check tools/galerkin_groups_host_check.cpp
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../nodal_amd/csrc/galerkin_groups.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            printf("FAILED %s: ", #cond);                 \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

// the entries one group takes from t0 on, as the kernel finds it; `order` is the order the lanes are visited in
int take_of(const std::vector<int> &len, int t0, const GalerkinCaps &c, const std::vector<int> &order) {
    const int remaining = (int)len.size() - t0;
    const int cand = galerkin_group_candidates(remaining, c);
    std::vector<int> prefix(c.lanes, 0);
    int run = 0;
    for (int k = 0; k < c.lanes; ++k) {  // (the wavefront's inclusive scan; lanes without a candidate add nothing)
        run += k < cand ? len[t0 + k] : 0;
        prefix[k] = run;
    }
    int kept = 0;
    for (int k : order) kept += galerkin_group_keeps(k, cand, prefix[k], c) ? 1 : 0;
    // the kept candidates are a prefix: the count is the boundary
    for (int k = 0; k < c.lanes; ++k)
        CHECK(galerkin_group_keeps(k, cand, prefix[k], c) == (k < kept), "lane %d of %d kept out of order", k, kept);
    return kept;
}

void check_row(const std::vector<int> &len, const GalerkinCaps &c, std::mt19937 &rng, int expect_groups = -1) {
    std::vector<int> fwd(c.lanes), rev(c.lanes), rnd(c.lanes);
    for (int k = 0; k < c.lanes; ++k) fwd[k] = rev[c.lanes - 1 - k] = rnd[k] = k;
    std::shuffle(rnd.begin(), rnd.end(), rng);
    const int rl = (int)len.size();
    std::vector<int> owner(rl, 0);
    int groups = 0;
    for (int t0 = 0; t0 < rl; ++groups) {
        const int take = take_of(len, t0, c, fwd);
        CHECK(take == take_of(len, t0, c, rev) && take == take_of(len, t0, c, rnd), "boundary depends on the lane order at %d", t0);
        CHECK(take >= 1, "no progress at %d", t0);
        if (take < 1) return;
        CHECK(take <= c.entries && take <= c.lanes && t0 + take <= rl, "group of %d entries at %d", take, t0);
        int products = 0;
        for (int k = 0; k < take; ++k) {
            products += len[t0 + k];
            ++owner[t0 + k];
        }
        CHECK(products <= c.products, "%d products in a list of %d", products, c.products);
        // greedy: the next entry, if the caps admit one, does not fit
        if (t0 + take < rl && take < c.entries && take < c.lanes)
            CHECK(products + len[t0 + take] > c.products, "group at %d stops early", t0);
        t0 += take;
    }
    for (int t = 0; t < rl; ++t) CHECK(owner[t] == 1, "entry %d is in %d groups", t, owner[t]);
    if (expect_groups >= 0) CHECK(groups == expect_groups, "%d groups, expected %d", groups, expect_groups);
}

}  // namespace

int main() {
    std::mt19937 rng(20);
    const GalerkinCaps caps[] = {{8, 64, 128}, {40, 64, 640}, {16, 64, 1024}, {64, 64, 512}, {64, 64, 64},
                                 {64, 16, 128}, {galerkin_sub_entries(40), 64, GALERKIN_SUB_PRODUCTS}};
    // degenerate rows
    for (const GalerkinCaps &c : caps) {
        check_row({}, c, rng, 0);
        check_row({16}, c, rng, 1);  // one entry with 16 products
        check_row({0}, c, rng, 1);
        check_row(std::vector<int>(c.entries < c.lanes ? c.entries : c.lanes, 0), c, rng, 1);  // exactly at the entry / lane cap
        check_row(std::vector<int>((c.entries < c.lanes ? c.entries : c.lanes) + 1, 0), c, rng, 2);
        if (c.products % 16 == 0 && c.products / 16 <= c.entries && c.products / 16 <= c.lanes) {
            check_row(std::vector<int>(c.products / 16, 16), c, rng, 1);      // exactly at the product cap
            check_row(std::vector<int>(c.products / 16 + 1, 16), c, rng, 2);  // one entry beyond it
        }
        std::vector<int> big(3, c.products < 64 ? c.products : 64);  // entries as long as a row of A P gets
        check_row(big, c, rng);
    }
    // random rows: lengths of rows of A P up to the 16 or 64 slots of their class (never above the list)
    for (int trial = 0; trial < 20000; ++trial) {
        const GalerkinCaps &c = caps[trial % (sizeof caps / sizeof *caps)];
        const int apw = (trial & 1) && c.products >= 64 ? 64 : 16;
        std::vector<int> len(rng() % 220);
        const int mode = rng() % 3;
        for (int &x : len) x = mode == 0 ? (int)(rng() % (apw + 1)) : (mode == 1 ? (int)(rng() % 7) : apw);
        check_row(len, c, rng);
    }
    CHECK(galerkin_sub_entries(8) == 8 && galerkin_sub_entries(40) == GALERKIN_SUB_ENTRIES, "sub-group entry cap");
    CHECK(GALERKIN_SUB_ENTRIES == 2 * GALERKIN_SUB_LANES && GALERKIN_SUB_ROWS * GALERKIN_SUB_LANES == 64, "sub-group shape");
    printf("capacities rows=%d entries=%d products=%d columns=%d\n", GALERKIN_SUB_ROWS, GALERKIN_SUB_ENTRIES,
           GALERKIN_SUB_PRODUCTS, GALERKIN_SUB_COLUMNS);
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("galerkin groups ok\n");
    return 0;
}
