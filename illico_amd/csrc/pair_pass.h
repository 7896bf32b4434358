// Host scaffolding of the all-pairs families -- pairwise.hip, pairwise_ranked.hip, and nothing else -- on top of group_pass.h: the
// selection of the K groups to compare with its checks and its upload, and the staging of a host caller's `sums` plane (its three
// or four [K*K][W] result planes go through a PlaneStage, preloaded).  The limits on K, the scratch buffers (names, sizes, budget), the kernels and the points at
// which the stream is synchronised are each family's own.
#pragma once
#include "group_pass.h"

namespace {

struct PairSelection {
    std::vector<int> sel;     // the K group ids, in the caller's order
    std::vector<long long> n; // their sizes
};
// the n_sel = K groups of `sel` (null: all G, in order; the caller has checked K) with the sizes size_of(g)
template <typename SizeOf> int select_pair_groups(illico_ctx *c, int64_t G, const int64_t *sel, int64_t n_sel, SizeOf &&size_of, PairSelection *S) {
    S->sel.resize((size_t)n_sel);
    S->n.resize((size_t)n_sel);
    std::vector<char> seen((size_t)G, 0);
    for (int64_t k = 0; k < n_sel; ++k) {
        const int64_t g = sel ? sel[k] : k;
        if (g < 0 || g >= G) return fail(c, ILLICO_ERR_ARG, "sel[%lld] = %lld is no group id (0 .. %lld)", (long long)k, (long long)g, (long long)G - 1);
        if (seen[g]) return fail(c, ILLICO_ERR_ARG, "group %lld is selected twice", (long long)g);
        seen[g] = 1;
        if (size_of(g) < 0) return fail(c, ILLICO_ERR_ARG, "counts[%lld] is negative", (long long)g);
        S->sel[k] = (int)g;
        S->n[k] = size_of(g);
    }
    long long a = 0, b = 0; // the two largest selected groups: their pair is the largest test
    for (long long n : S->n) { if (n > a) { b = a; a = n; } else if (n > b) b = n; }
    if (a + b >= 2097152ll)
        return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld cells in one pair: the integer rank and tie sums hold below 2097152 cells per test", a + b);
    return ILLICO_OK;
}
// into memory the caller carved: K sizes, K ids.  Enqueued from pageable host memory: S outlives the caller's next synchronisation.
inline int upload_pair_selection(illico_ctx *c, const PairSelection &S, long long *d_n, int *d_sel) {
    HIPCHK(c, hipMemcpyAsync(d_n, S.n.data(), S.n.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_sel, S.sel.data(), S.sel.size() * 4, hipMemcpyHostToDevice, c->stream));
    return ILLICO_OK;
}

// a host caller's [G][W] sums in `scratch`, as the kernels then read them
inline int stage_pair_sums(illico_ctx *c, const double *sums, int64_t sums_ld, int64_t G, int64_t W, void *scratch, const double **d_sums, int64_t *d_sums_ld) {
    *d_sums = (const double *)scratch;
    *d_sums_ld = W;
    return copy_plane(c, scratch, W, sums, sums_ld, G, W, 8, hipMemcpyHostToDevice);
}

} // namespace
