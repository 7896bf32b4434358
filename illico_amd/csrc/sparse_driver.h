// Host-side drivers of the CSC / CSR routes, templated on the value / index types: instantiated in sparse_<type>.hip.
// run_sparse_t, at the end, is the list of the routes in the order they are tried; every route is a function over one SparseCall
// (DESIGN.md section 17).
#pragma once

#include "keyed_driver.h"
#include "host_narrow.h"
#include <thread>

static size_t seg_lds_bytes(int G) { return (size_t)((G + 3) & ~3) * 4 + SEG_NT * 4; }

// Groups per launch of k_csc_counts: all of them while their tables fit LDS the way the kernel likes it (mixed cells: two workgroups
// per CU), else equal windows of about 2000 groups (16-bit cells: about 1100), one launch per window over the same entries.
static int cscc_group_window(int G, bool w16) {
    // (16-bit cells: windows rather than a 32-value table -- genes with a value of 32 .. 63 would leave the route)
    const bool one = w16 ? cscc_lds_bytes(G, CSCC_16BIT, 64) + 8192 <= kMaxLds : cscc_lds_bytes(G, CSCC_8BIT, 32) + 8192 <= kMaxLds;
    if (one) return G;
    const int per = w16 ? 1100 : 2000;
    const int k = (G + per - 1) / per;
    return (G + k - 1) / k;
}

// How k_csc_counts lays a call's groups out in LDS: formed once per call from the context's groups and options.
struct CscCountsLayout {
    std::vector<signed char> h_slot; // per group: its row in the 32-bit side table (groups above 255 cells other than the OVO reference, which has its own table), -1 = none
    int n_big_all = 0;               // such groups
    int n_big = 0;                   // ... that the launch gives a side-table row (none under w16)
    int64_t max_ranked = 0;          // cells of the largest ranked group
    bool w16 = false;                // 16-bit cells for every group, one pass
    int Gw = 0, n_windows = 0;       // groups per launch (CscCountsParams::g_lo) and launches per batch
    int rt8 = 32;                    // table size of the 8-bit (or 16-bit) form
    bool mixed = false;              // first the mixed 8- / 4-bit cells
    bool pack16 = false;             // 16-byte statistics while every ranked group has at most 255 cells
    int cells(bool mixed_pass) const { return w16 ? CSCC_16BIT : mixed_pass ? CSCC_MIXED : CSCC_8BIT; } // the kernel's layout parameter
    int rt(bool mixed_pass) const { return mixed_pass ? 64 : rt8; }
    size_t lds(bool mixed_pass) const { return cscc_lds_bytes(Gw, cells(mixed_pass), rt(mixed_pass)); }
};
static CscCountsLayout csc_counts_layout(const illico_ctx *c) {
    CscCountsLayout L;
    const int G = (int)c->n_groups;
    const bool ovr = c->ref < 0;
    L.h_slot.assign(G, (signed char)-1);
    for (int g = 0; g < G; ++g) {
        if (g == c->ref) continue;
        if (c->h_counts[g] > 255) L.h_slot[g] = (signed char)std::min(L.n_big_all++, 127);
        L.max_ranked = std::max<int64_t>(L.max_ranked, c->h_counts[g]);
    }
    // more big groups than the side table holds: 16-bit cells for every group, while those fit LDS
    // (... or an OVO reference of 30 000 cells or more: the sweep's 32-bit terms -- 3 tS^2 -- would overflow; the 16-bit form's are 64-bit)
    L.w16 = L.n_big_all > CSCC_MAX_BIG || (!ovr && c->h_counts[c->ref] >= 30000);
    L.n_big = L.w16 ? 0 : L.n_big_all;
    // more groups than LDS holds tables for: windows of Gw groups, one launch each over the same entries -- up to 33 of them (65 535 groups:
    // the 16-bit code table's limit; 30 000 groups of ten cells at C3 shape: 52.7 ms through the per-gene sort routes when eight was the limit)
    L.Gw = cscc_group_window(G, L.w16);
    L.n_windows = (G + L.Gw - 1) / std::max(1, L.Gw);
    L.rt8 = cscc_lds_bytes(L.Gw, L.cells(false), 64) + 8192 <= kMaxLds ? 64 : 32;
    // the mixed layout pays when two workgroups fit a CU
    // (... or when 64 bytes per group do not fit at all: the mixed table still holds all 63 values where the 8-bit form would drop to 31)
    L.mixed = !L.w16 && !c->no_csc_counts_mixed && (2 * (cscc_lds_bytes(L.Gw, CSCC_MIXED, 64) + 4096) <= kMaxLds || (L.rt8 == 32 && cscc_lds_bytes(L.Gw, CSCC_MIXED, 64) + 8192 <= kMaxLds));
    L.pack16 = L.n_big == 0 && !L.w16;
    return L;
}

// Sparse OVO with groups whose (gene, group) runs outgrow what k_csc_gene / k_ovo_rank take quickly (clusters of hundreds or
// thousands of cells): regroup, then the packed rank kernel of the dense route (kernels_ovo_compact.h) on the regrouped runs
// (small_groups: groups of at most 256 cells as well -- k_csc_gene takes those in one kernel when a gene's entries fit its LDS key buffer;
//  genes that do not -- eight-byte keys: C3's 30 000 entries per gene -- are ranked by the packed kernel too, not by k_ovo_rank)
static bool sparse_packed_rank_fits(const illico_ctx *c, bool small_groups = false) {
    if (c->ref < 0 || c->no_packed_dense || (c->max_nonref <= 256 && !small_groups) || c->max_nonref > 65535) return false;
    const int64_t n_ref = c->h_counts[c->ref];
    return n_ref >= 1 && n_ref <= 65535;
}

// Average stored entries per column above which a sparse window is written out dense (the dense routes then rank it): what the per-gene
// LDS kernels hold -- 32 768 four-byte keys, half as many eight-byte ones.  OVO with eight-byte keys keeps the four-byte bound: its columns
// are regrouped in HBM and ranked by the packed kernel, whatever their length (C3 shape as CSR in float64: 14.3 ms through the dense
// window -- 19 GB of it --, 24 through k_ovo_rank).
template <typename KeyT> static double long_column(const illico_ctx *c) {
    if (sizeof(KeyT) == 8 && c->ref >= 0 && !c->no_sparse_packed_small && sparse_packed_rank_fits(c, true)) return 32768.0;
    return 32768.0 * 4.0 / (double)sizeof(KeyT);
}

// sizes the group-major CSR pass holds (kernels_csr_counts.h)
static bool csr_counts_route_fits(const illico_ctx *c, int flags, int64_t n_rows) {
    if (c->no_csr_counts_path || c->hold_csr_counts || (flags & ILLICO_FLAG_LOG1P) || c->tap || c->no_counts_path || c->big_n) return false;
    if (c->csr_n_big < 0 || n_rows >= (1ll << 30) || c->n_groups > 65535) return false;
    if (c->ref >= 0 && (c->h_counts[c->ref] < 1 || c->h_counts[c->ref] >= 30000)) return false;
    return true;
}
// what a call learns from the verdict words of the pass: true = the matrix was not for the route at all
static bool csr_counts_verdict_bad(const u32 *vd) {
    return (double)vd[0] > 0.02 * (double)vd[2] || (double)vd[1] > 0.005 * (double)vd[2] || vd[3] != 0u;
}

// ---- one description of a sparse call: what the routes share ----
template <typename InT, typename IdxT>
struct SparseCall {
    illico_ctx *c;
    bool is_csr;
    const void *data, *indices, *indptr; // the caller's three arrays (host or device)
    // device views of them: stored entry k of the caller's arrays is d_data[k - kshift] / d_indices[k - kshift]
    const InT *d_data; const IdxT *d_indices, *d_indptr;
    int64_t kshift = 0;
    const int *d_codes; // the group code of each cell; null where the indices are the codes already
    int64_t n_rows, n_cols, col_lb, col_ub;
    int dtype, flags, alternative;
    OutPlanes o;
    SparseAllow allow;
    int G;           // derived once
    bool ovr, in_dev;
    int64_t W, n_ptr;
    // More groups than the regrouping kernels' LDS histogram holds (~40 000): what the count-valued routes do not take is written out as
    // a dense window in the matrix's own type and takes the dense routes, which know no such limit (the reference has none either:
    // ovr/sparse_ovr.py:23-97, utils/groups.py:18-58).
    bool many_groups;
    CscCountsLayout cscc;     // (CSC)
    bool counts_route;        // CSC, count-valued, small groups: k_csc_counts -- when a sample of the window's stored values says they are counts at all
    bool window_route;        // CSR, count-valued, not too sparse: dense byte windows + the fused single-pass kernels; the same question
    bool csr_counts;          // CSR, count-valued, small groups: the group-major single pass (kernels_csr_counts.h); the same question
    int64_t total_nnz = 0;    // known once indptr has been fetched
    double density = 0.0;
    std::vector<IdxT> h_indptr; // all of indptr on the host (CSC: batch planning)
    u32 h_sample[4] = {0, 0, 0, 0}; // of a sample of the stored values: non-integers, integers beyond the table, samples taken
    bool sampled = false;

    int64_t nnz_between(int64_t lb, int64_t ub) const { return (int64_t)h_indptr[ub] - (int64_t)h_indptr[lb]; } // stored entries of columns [lb, ub) (CSC)
    bool is_log1p() const { return (flags & ILLICO_FLAG_LOG1P) != 0; }
    // device arrays, device planes, ILLICO_FLAG_DEFER: a pass may be enqueued as a whole and looked at later
    bool deferrable() const { return (flags & ILLICO_FLAG_DEFER) && in_dev && (flags & ILLICO_FLAG_OUTPUT_DEVICE) && !o.staged; }
    // float64 that may be looked at for holding float32 values only (route_f64_as_f32)
    bool may_narrow() const { return std::is_same<InT, double>::value && in_dev && allow.dense_window && !allow.indices_are_codes && !c->no_f64_narrowing && !c->tap && !is_log1p(); }
    int idx_dtype() const { return (int)(sizeof(IdxT) == 4 ? ILLICO_IDX_I32 : ILLICO_IDX_I64); }
    // columns [lb, ub) of the same call through the routes `a` still allows
    template <typename KeyT> int reenter(int64_t lb, int64_t ub, SparseAllow a) const {
        return run_sparse_t<InT, IdxT, KeyT>(c, is_csr, data, indices, indptr, dtype, n_rows, n_cols, lb, ub, flags, alternative, o.shifted(lb - col_lb), a);
    }
};

template <typename InT, typename IdxT>
static SparseCall<InT, IdxT> describe_sparse_call(illico_ctx *c, bool is_csr, const void *data, const void *indices, const void *indptr, int dtype, int64_t n_rows,
                                                  int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, int alternative, const OutPlanes &o, SparseAllow allow) {
    SparseCall<InT, IdxT> S;
    S.c = c; S.is_csr = is_csr; S.data = data; S.indices = indices; S.indptr = indptr;
    S.d_data = (const InT *)data; S.d_indices = (const IdxT *)indices; S.d_indptr = (const IdxT *)indptr; // (device-resident input; upload_host_arrays otherwise)
    S.d_codes = allow.indices_are_codes ? nullptr : c->d_codes;
    S.n_rows = n_rows; S.n_cols = n_cols; S.col_lb = col_lb; S.col_ub = col_ub; S.dtype = dtype; S.flags = flags; S.alternative = alternative;
    S.o = o; S.allow = allow;
    S.G = (int)c->n_groups; S.ovr = c->ref < 0; S.in_dev = flags & ILLICO_FLAG_INPUT_DEVICE;
    S.W = col_ub - col_lb; S.n_ptr = (is_csr ? n_rows : n_cols) + 1;
    S.many_groups = seg_lds_bytes(S.G) > kMaxLds;
    S.counts_route = false;
    if (!is_csr) {
        const CscCountsLayout &L = S.cscc = csc_counts_layout(c);
        const bool cells_fit = (!L.w16 || (L.max_ranked <= 65535 && !c->no_csc_counts_wide)) && L.n_windows <= (c->csc_counts_max_windows > 0 ? c->csc_counts_max_windows : 33) &&
                               (L.n_windows == 1 || (!c->no_csc_counts_windows && c->d_codes16 && !allow.indices_are_codes));
        // (big_n -- OVR over more than 2^21 - 1 cells --: the table kernels' t^3 terms could wrap; the sort-based routes hold)
        S.counts_route = !c->big_n && !c->no_csc_counts_path && !S.is_log1p() && cells_fit && n_rows < (1ll << 30) &&
                         (uint64_t)n_rows * std::max(sizeof(InT), sizeof(IdxT)) < (1ull << 32) && // (k_csc_counts forms the byte offsets of a column's entries in 32 bits)
                         (S.ovr || c->h_counts[c->ref] < (1ll << 30));
    }
    S.window_route = is_csr && !c->big_n && allow.dense_window && !c->no_dense_window_path && fused_path_allowed(c, flags) && (size_t)n_rows * 4 * 64 <= (size_t)c->scratch_bytes;
    S.csr_counts = is_csr && allow.csr_counts && S.W > 0 && csr_counts_route_fits(c, flags, n_rows);
    return S;
}

// ---- order-independent value sums (kernels_sums.h) of `nb` genes from column col0 on (or of the list d_cols) ----
template <typename InT, typename IdxT>
static int launch_csc_value_sums(const SparseCall<InT, IdxT> &S, int64_t col0, const int *d_cols, int nb, double *ssum) {
    illico_ctx *c = S.c;
    CscSumsParams P;
    P.data = S.d_data; P.indices = S.d_indices; P.indptr = S.d_indptr; P.kshift = S.kshift; P.col0 = col0; P.gene_cols = d_cols; P.codes = S.d_codes; P.codes16 = S.d_codes ? c->d_codes16 : nullptr;
    P.nb = nb; P.G = S.G; P.dt = S.dtype; P.is_log1p = S.is_log1p() ? 1 : 0; P.acc_global = nullptr; P.out_sum = ssum;
    // accumulators in LDS while they fit at all (one workgroup per CU beyond 5000 groups); in HBM through global atomics otherwise:
    // 46 times slower at 10 000 groups (29 ms against 0.65 at C3 shape), which is where the threshold used to sit
    const bool accg = csc_sums_lds_bytes(P.G, false) + 2048 > kMaxLds;
    const size_t lds = csc_sums_lds_bytes(P.G, accg);
    if (accg) {
        int rc = scratch(c, "sums_acc", (size_t)nb * 2 * P.G, &P.acc_global);
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(P.acc_global, 0, (size_t)nb * 2 * P.G * 8, c->stream));
    }
    ProfScope ps(c, KID_VALUE_SUMS);
    return dispatch_flags([&](auto ag) { return launch_kernel(c, k_csc_value_sums<InT, IdxT, decltype(ag)::value>, dim3(nb), dim3(CSUM_NT), lds, P); }, accg);
}

struct SparseBatch {
    int64_t g0, g1;   // gene range (absolute column indices)
    int64_t nnz;      // stored entries in the range
    int64_t max_gene; // largest per-gene nnz in the range
};

// split [col_lb, col_ub) so that each batch's scratch stays under the cap and its nnz below 2^31
static std::vector<SparseBatch> plan_batches(const std::vector<int64_t> &gene_nnz, int64_t col_lb, size_t per_nnz,
                                             size_t per_gene, int64_t gene_batch, size_t cap) {
    std::vector<SparseBatch> out;
    const int64_t W = (int64_t)gene_nnz.size();
    int64_t i = 0;
    while (i < W) {
        SparseBatch b{col_lb + i, col_lb + i, 0, 0};
        size_t bytes = 0;
        while (i < W) {
            int64_t c = gene_nnz[i];
            size_t add = (size_t)c * per_nnz + per_gene;
            bool full = (b.g1 > b.g0) && (bytes + add > cap || b.nnz + c > 0x7FFF0000ll || (gene_batch > 0 && b.g1 - b.g0 >= gene_batch));
            if (full) break;
            bytes += add;
            b.nnz += c;
            b.max_gene = std::max(b.max_gene, c);
            b.g1 += 1;
            ++i;
        }
        out.push_back(b);
    }
    return out;
}

// device copy of a column list (absolute indices) for the list-driven kernels / k_finalize's col_map; null when the columns are contiguous
static int upload_cols(illico_ctx *c, const std::vector<int64_t> &cols, const int **d_cols) {
    *d_cols = nullptr;
    if (cols.back() - cols.front() + 1 == (int64_t)cols.size()) return ILLICO_OK;
    int *d;
    int rc = scratch(c, "sp_collist", std::max<size_t>(cols.size(), 1), &d);
    if (rc) return rc;
    std::vector<int> h(cols.begin(), cols.end());
    HIPCHK(c, hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // h goes out of scope
    *d_cols = d;
    return ILLICO_OK;
}

// the launch of k_csc_counts for one window of the groups (kernels_csc_counts.h; its template parameters: DESIGN.md section 25)
template <typename InT, typename IdxT>
static int launch_csc_counts(illico_ctx *c, const CscCountsParams &P, int cells, int rt, bool has_big, bool ovr, size_t lds) {
    ProfScope ps(c, KID_CSC_COUNTS);
    const bool win = P.G != P.G_total; // a window of the groups (instantiated for 16-bit group codes only: the host's case)
    if (win && !P.codes16) return fail(c, ILLICO_ERR_UNSUPPORTED, "group windows need the 16-bit code table");
    // (C16F, WINF) takes three values: a window implies the 16-bit codes.  16-bit cells hold every group: no side table.
    return dispatch_flags([&](auto ovr_c, auto big_c, auto c16_c, auto win_c) {
        return dispatch_int<CSCC_MIXED, CSCC_8BIT, CSCC_16BIT>(cells, [&](auto cells_c) {
            return dispatch_int<64, 32>(rt, [&](auto rt_c) -> int {
                constexpr int CELLS = decltype(cells_c)::value, RTV = decltype(rt_c)::value;
                constexpr bool C16F = decltype(c16_c)::value, WINF = decltype(win_c)::value, BIG = decltype(big_c)::value && CELLS != CSCC_16BIT;
                if constexpr ((WINF && !C16F) || (CELLS == CSCC_MIXED && RTV != 64)) return ILLICO_OK; // (never called: checked above; CscCountsLayout::rt)
                else return launch_kernel(c, k_csc_counts<InT, IdxT, decltype(ovr_c)::value, RTV, BIG, CELLS, C16F, WINF>, dim3(P.nb), dim3(CSCC_NT), lds, P);
            });
        });
    }, ovr, has_big, win || P.codes16 != nullptr, win);
}

// k_finalize for batch genes cols[b0 ..) of a column list: through the uploaded list when there is one, else they are contiguous
template <typename InT, typename IdxT>
static int finalize_listed(const SparseCall<InT, IdxT> &S, const StatsPlanes &st, const double *gtot, int nb, const std::vector<int64_t> &cols, int64_t b0,
                           const int *d_cols, bool packed = false, bool tie_f64 = false) {
    return launch_finalize(S.c, st.s2u, st.stie, st.ssum, gtot, nb, S.flags, S.alternative, S.o, d_cols ? -S.col_lb : cols[b0] - S.col_lb, d_cols ? d_cols + b0 : nullptr,
                           packed, tie_f64);
}
// ---- k_csc_counts: count-valued CSC genes, per-group value histograms in LDS, OVO and OVR ----
// the side table's slots on the device (rare: a one-off upload + wait; a context keeps its groups for many calls)
static int upload_csc_slots(illico_ctx *c, const CscCountsLayout &L, const signed char **d_slot) {
    *d_slot = nullptr;
    if (!L.n_big_all || L.n_big_all > CSCC_MAX_BIG) return ILLICO_OK;
    signed char *d;
    int rc = scratch(c, "cscc_slot", L.h_slot.size(), &d);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d, L.h_slot.data(), L.h_slot.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!L.w16) *d_slot = d;
    return ILLICO_OK;
}
// what every launch of a call has in common; the caller adds col0 / gene_cols / nb, fallback and verdict
template <typename InT, typename IdxT>
static CscCountsParams csc_counts_params(const SparseCall<InT, IdxT> &S, const StatsPlanes &st, const signed char *d_slot) {
    illico_ctx *c = S.c;
    CscCountsParams P;
    P.data = S.d_data; P.indices = S.d_indices; P.indptr = S.d_indptr; P.kshift = S.kshift; P.gene_cols = nullptr;
    P.codes16 = S.d_codes ? c->d_codes16 : nullptr; // (sparse input holds fewer than 65 536 groups: the 16-bit table exists)
    P.counts = c->d_counts; P.G = S.G; P.ref = (int)c->ref; P.n_cells = S.n_rows; P.out_2u = st.s2u; P.out_tie = st.stie; P.out_sum = st.ssum; P.big_slot = d_slot;
    P.gene_total = S.ovr ? st.gtot : nullptr;
    P.tie_f64 = S.ovr ? 1 : 0; // (the reference's sparse OVR arithmetic, kernels_finalize.h: tie_f64_sparse)
    P.verdict = nullptr;
    P.pack16 = S.cscc.pack16 ? 1 : 0;
    P.G_total = S.G;
    return P;
}
// one launch per window of the groups (one window unless the groups outgrow LDS)
template <typename InT, typename IdxT>
static int launch_csc_counts_windows(const SparseCall<InT, IdxT> &S, CscCountsParams P, bool mixed) {
    const CscCountsLayout &L = S.cscc;
    int rc;
    for (int g_lo = 0; g_lo < S.G; g_lo += L.Gw) {
        P.g_lo = g_lo; P.G = std::min(L.Gw, S.G - g_lo);
        if ((rc = launch_csc_counts<InT, IdxT>(S.c, P, L.cells(mixed), L.rt(mixed), L.n_big > 0, S.ovr, L.lds(mixed)))) return rc;
    }
    return ILLICO_OK;
}

// `cols` in: the genes to compute; out: the genes it could not take.  First the mixed 8- / 4-bit cells (two workgroups per CU); the
// genes where a 4-bit cell overflowed are redone with 8-bit cells; genes with values outside the table are left to the general routes.
template <typename InT, typename IdxT>
static int run_csc_counts_route(const SparseCall<InT, IdxT> &S, std::vector<int64_t> &cols) {
    illico_ctx *c = S.c;
    const CscCountsLayout &L = S.cscc;
    int rc;
    const signed char *d_slot;
    if ((rc = upload_csc_slots(c, L, &d_slot))) return rc;
    if (S.d_codes && !c->d_codes16) return ILLICO_OK; // every gene stays in `cols`
    std::vector<int64_t> left;
    // pass 0: mixed cells over every gene; pass 1: 8-bit cells over the genes whose 4-bit cells overflowed (or over every
    // gene when the mixed form is not used)
    for (int pass = L.mixed ? 0 : 1; pass < 2 && !cols.empty(); ++pass) {
        const int *d_cols;
        if ((rc = upload_cols(c, cols, &d_cols))) return rc;
        const int64_t n = (int64_t)cols.size(), nb_max = stats_batch_genes(n, S.G);
        StatsPlanes st;
        if ((rc = carve_stats(c, nb_max, S.G, true, &st))) return rc;
        std::vector<int64_t> redo;
        for (int64_t b0 = 0; b0 < n; b0 += nb_max) {
            const int nb = (int)std::min<int64_t>(nb_max, n - b0);
            HIPCHK(c, hipMemsetAsync(st.flags, 0, (size_t)nb * 4, c->stream));
            CscCountsParams P = csc_counts_params(S, st, d_slot);
            P.col0 = cols[b0]; P.gene_cols = d_cols ? d_cols + b0 : nullptr; P.nb = nb; P.fallback = st.flags;
            if ((rc = launch_csc_counts_windows(S, P, pass == 0))) return rc;
            if ((rc = finalize_listed(S, st, S.ovr ? st.gtot : nullptr, nb, cols, b0, d_cols, L.pack16, S.ovr))) return rc;
            const u32 *h_fb;
            if ((rc = read_gene_flags(c, st.flags, nb, &h_fb))) return rc;
            for (int64_t j = 0; j < nb; ++j) {
                if (h_fb[j] == 2u) redo.push_back(cols[b0 + j]);
                else if (h_fb[j]) left.push_back(cols[b0 + j]);
            }
        }
        cols.swap(redo);
    }
    std::sort(left.begin(), left.end());
    cols.swap(left);
    return ILLICO_OK;
}

// ---- the deferred count passes: ILLICO_FLAG_DEFER on device-resident arrays with device planes ----
// CSC: the count-valued pass (value sample, k_csc_counts, k_finalize) is enqueued and the call returns -- no host wait at all.  Whether
// the window is count-valued is decided on the device from the sample; which genes the pass could not take (values outside the table,
// 4-bit cells that overflowed) travels to pinned memory behind an event and is looked at by the next call on the context /
// illico_ctx_synchronize (resolve_pending_csc), which recomputes exactly those columns through the ordinary routes.
template <typename InT, typename IdxT>
static int run_csc_counts_deferred(const SparseCall<InT, IdxT> &S) {
    illico_ctx *c = S.c;
    const CscCountsLayout &L = S.cscc;
    const int64_t W = S.W;
    int rc;
    const signed char *d_slot;
    if ((rc = upload_csc_slots(c, L, &d_slot))) return rc;
    u32 *d_cnt, *fb;
    if ((rc = clear_flag_words(c, &d_cnt))) return rc;
    KERNELCHK(c, k_sample_noncount_cols<InT, IdxT>, dim3((1 << 16) / 256), dim3(256), 0, S.d_data, S.d_indptr, (long long)S.col_lb,
              (long long)S.col_ub, 1 << 16, CSCC_RT, d_cnt);
    const int64_t nb_max = stats_batch_genes(W, S.G);
    StatsPlanes st;
    if ((rc = carve_stats(c, nb_max, S.G, false, &st))) return rc;
    if ((rc = scratch(c, "sp_defer_flags", (size_t)W, &fb))) return rc;
    HIPCHK(c, hipMemsetAsync(fb, 0, (size_t)W * 4, c->stream));
    for (int64_t b0 = 0; b0 < W; b0 += nb_max) {
        const int nb = (int)std::min<int64_t>(nb_max, W - b0);
        CscCountsParams P = csc_counts_params(S, st, d_slot);
        P.col0 = S.col_lb + b0; P.nb = nb; P.fallback = fb + b0; P.verdict = d_cnt;
        if ((rc = launch_csc_counts_windows(S, P, L.mixed))) return rc;
        if ((rc = launch_finalize(c, st.s2u, st.stie, st.ssum, S.ovr ? st.gtot : nullptr, nb, S.flags, S.alternative, S.o, b0, nullptr, L.pack16, S.ovr))) return rc;
    }
    int slot;
    void *pin;
    if ((rc = reserve_deferred_slot(c, (size_t)W * 4, &slot, &pin))) return rc;
    HIPCHK(c, hipMemcpyAsync(pin, fb, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = post_deferred_call(c, slot, 1, S.dtype, S.flags, S.alternative, S.n_rows, S.col_lb, S.col_ub, S.o))) return rc;
    PendingDense &q = c->pend;
    q.sp_data = S.data; q.sp_indices = S.indices; q.sp_indptr = S.indptr; q.idx_dtype = S.idx_dtype(); q.n_cols = S.n_cols;
    return ILLICO_OK;
}

// Single-kernel CSC OVO route over the genes in `cols` (in: to compute; out: the genes it could not take, which go to
// the two-kernel route): statistics + finalize per batch.  gene_nnz[j]: stored entries of gene col_lb + j.
template <typename InT, typename IdxT, typename KeyT>
static int run_csc_gene_route(const SparseCall<InT, IdxT> &S, std::vector<int64_t> &cols, const std::vector<int64_t> &gene_nnz) {
    illico_ctx *c = S.c;
    const int G = S.G;
    const int runend_cap = (int)std::max<int64_t>(1, std::min<int64_t>(c->h_counts[c->ref], 8192));
    { // genes with more entries than the kernel's LDS key buffer would only be flagged by it: when that is most of them (eight-byte
        // keys at C3's 30 000 entries per gene) the launch is skipped altogether
        const size_t fixed0 = cscg_lds_bytes(G, 0, runend_cap, sizeof(KeyT), false);
        const int64_t cap0 = fixed0 < kMaxLds ? (int64_t)((kMaxLds - fixed0) / sizeof(KeyT)) : 0;
        int64_t fit = 0;
        for (int64_t cc : cols) fit += gene_nnz[cc - S.col_lb] <= cap0 ? 1 : 0;
        if (fit * 4 < (int64_t)cols.size()) return ILLICO_OK; // every gene stays in `cols` for the two-kernel route
    }
    int rc;
    const int *d_cols;
    if ((rc = upload_cols(c, cols, &d_cols))) return rc;
    // bucket form of the reference run (no sort, short look-ups): its 16-bit table takes the run-end region
    const bool ref_buckets = !c->no_ovo_ref_buckets && cscg_lds_bytes(G, 0, runend_cap, sizeof(KeyT), true) + 16384 * sizeof(KeyT) <= kMaxLds;
    const size_t fixed = cscg_lds_bytes(G, 0, runend_cap, sizeof(KeyT), ref_buckets);
    if (fixed + 1024 * sizeof(KeyT) > kMaxLds) return ILLICO_OK; // every gene stays in `cols` for the two-kernel route
    const int key_cap = (int)((kMaxLds - fixed) / sizeof(KeyT));
    const size_t lds = cscg_lds_bytes(G, key_cap, runend_cap, sizeof(KeyT), ref_buckets);
    const int64_t n = (int64_t)cols.size(), nb_max = stats_batch_genes(n, G);
    StatsPlanes st;
    if ((rc = carve_stats(c, nb_max, G, true, &st))) return rc;
    std::vector<int64_t> left;
    for (int64_t b0 = 0; b0 < n; b0 += nb_max) {
        const int nb = (int)std::min<int64_t>(nb_max, n - b0);
        HIPCHK(c, hipMemsetAsync(st.flags, 0, (size_t)nb * 4, c->stream));
        CscGeneParams P;
        P.data = S.d_data; P.indices = S.d_indices; P.indptr = S.d_indptr; P.kshift = S.kshift; P.col0 = cols[b0];
        P.gene_cols = d_cols ? d_cols + b0 : nullptr; P.nb = nb; P.codes = S.d_codes; P.codes16 = S.d_codes ? c->d_codes16 : nullptr;
        P.counts = c->d_counts; P.G = G; P.ref = (int)c->ref; P.dt = S.dtype; P.is_log1p = S.is_log1p() ? 1 : 0;
        P.key_cap = key_cap; P.runend_cap = runend_cap; P.ref_buckets = ref_buckets ? 1 : 0; P.fallback = st.flags; P.out_2u = st.s2u; P.out_tie = st.stie; P.out_sum = st.ssum;
        {
            ProfScope ps(c, KID_CSC_GENE);
            KERNELCHK(c, k_csc_gene<InT, IdxT, KeyT>, dim3(nb), dim3(CSCG_NT), lds, P);
        }
        // the kernel adds a group's values in the order its LDS regroup happened to leave them: replace its sums by the
        // order-independent ones
        if ((rc = launch_csc_value_sums(S, cols[b0], d_cols ? d_cols + b0 : nullptr, nb, st.ssum))) return rc;
        if ((rc = finalize_listed(S, st, nullptr, nb, cols, b0, d_cols))) return rc;
        const u32 *h_fb;
        if ((rc = read_gene_flags(c, st.flags, nb, &h_fb))) return rc;
        for (int64_t j = 0; j < nb; ++j)
            if (h_fb[j]) left.push_back(cols[b0 + j]);
    }
    cols.swap(left);
    return ILLICO_OK;
}

// Single-kernel CSC OVR route (any values) over the genes in `cols` (in: to compute; out: the genes with more stored
// entries than the LDS key buffer, which go to the general route): statistics + gene totals + finalize per batch.
template <typename InT, typename IdxT, typename KeyT>
static int run_csc_ovr_route(const SparseCall<InT, IdxT> &S, int64_t max_nnz, std::vector<int64_t> &cols) {
    illico_ctx *c = S.c;
    const int G = S.G;
    const int64_t n_rows = S.n_rows;
    // the group's stored-entry count rides above bit 40 of its doubled rank sum
    if (n_rows >= (1ll << 31) || (double)c->max_nonref * 2.0 * (double)n_rows >= (double)(1ull << CSCO_CNT_SHIFT) || c->max_nonref >= (1ll << 23))
        return ILLICO_OK; // every gene stays in `cols`
    // 16384 buckets when the largest gene still fits beside them, else 8192
    int lg = 14;
    if (csco_key_cap(G, lg, sizeof(KeyT), kMaxLds) < max_nnz) lg = 13;
    int key_cap = csco_key_cap(G, lg, sizeof(KeyT), kMaxLds);
    // thousands of groups: acc[G] takes the key buffer's place -- the accumulators then live in HBM (global atomics) and the keys keep LDS
    bool accg = false;
    int g_lds = G; // groups whose accumulators stay in LDS
    if (key_cap < max_nnz) {
        int lg2 = 14;
        if (csco_key_cap(G, lg2, sizeof(KeyT), kMaxLds, true) < max_nnz) lg2 = 13;
        const int cap2 = csco_key_cap(G, lg2, sizeof(KeyT), kMaxLds, true);
        if (cap2 > key_cap) {
            accg = true; lg = lg2;
            // what the largest gene's keys leave of LDS holds the accumulators of the first groups; the others' live in HBM
            const size_t need = csco_fixed_lds_bytes(0, lg) + ((size_t)std::min<int64_t>(max_nnz, cap2) + 8) * sizeof(KeyT);
            g_lds = need < kMaxLds ? (int)std::min<size_t>((size_t)G, ((kMaxLds - need) / 8) & ~(size_t)1) : 0;
            key_cap = (int)std::min<size_t>((kMaxLds - csco_fixed_lds_bytes(g_lds, lg)) / sizeof(KeyT) - 4, 65535 - 4);
        }
    }
    if (key_cap <= 0) return ILLICO_OK;
    // short columns (a matrix of few cells: 2000 stored entries per gene): no more key slots and buckets than the longest column needs --
    // two workgroups per CU then run side by side (one's barriers under the other's passes)
    if (!accg && !c->no_csc_ovr_small_lds && max_nnz + 64 < key_cap) {
        int lg_s = lg;
        while (lg_s > 11 && (1ll << (lg_s - 1)) >= 2 * max_nnz) --lg_s;
        const int cap_s = (int)std::min<int64_t>(csco_key_cap(G, lg_s, sizeof(KeyT), kMaxLds), std::max<int64_t>((max_nnz + 64 + 1023) & ~1023ll, 2048));
        if (cap_s >= max_nnz) { lg = lg_s; key_cap = cap_s; }
    }
    int rc;
    const int *d_cols;
    if ((rc = upload_cols(c, cols, &d_cols))) return rc;
    const size_t lds = csco_fixed_lds_bytes(g_lds, lg) + (size_t)(key_cap + 4) * sizeof(KeyT);
    const int64_t n = (int64_t)cols.size(), nb_max = stats_batch_genes(n, G);
    StatsPlanes st;
    if ((rc = carve_stats(c, nb_max, G, true, &st))) return rc;
    auto kern = accg ? k_csc_ovr_gene<InT, IdxT, KeyT, true> : k_csc_ovr_gene<InT, IdxT, KeyT, false>;
    u64 *acc_g = nullptr;
    if (accg && (rc = scratch(c, "csco_acc", (size_t)nb_max * G, &acc_g))) return rc;
    std::vector<int64_t> left;
    for (int64_t b0 = 0; b0 < n; b0 += nb_max) {
        const int nb = (int)std::min<int64_t>(nb_max, n - b0);
        HIPCHK(c, hipMemsetAsync(st.flags, 0, (size_t)nb * 4, c->stream));
        CscOvrParams P;
        memset(&P, 0, sizeof P);
        P.data = S.d_data; P.indices = S.d_indices; P.indptr = S.d_indptr; P.kshift = S.kshift; P.col0 = cols[b0];
        P.gene_cols = d_cols ? d_cols + b0 : nullptr; P.nb = nb; P.codes = S.d_codes; P.codes16 = S.d_codes ? c->d_codes16 : nullptr; P.counts = c->d_counts; P.G = G; P.dt = S.dtype;
        P.is_log1p = S.is_log1p() ? 1 : 0; P.n_cells = n_rows; P.key_cap = key_cap; P.lg_buckets = lg;
        P.force_sorted = c->csc_ovr_sorted_form ? 1 : 0; P.fallback = st.flags;
        P.out_2u = st.s2u; P.out_tie = st.stie; P.tie_f64 = 1; P.acc_global = acc_g; P.g_lds = g_lds;
        if (accg) HIPCHK(c, hipMemsetAsync(acc_g, 0, (size_t)nb * G * 8, c->stream));
        {
            ProfScope ps(c, KID_CSC_OVR);
            KERNELCHK(c, kern, dim3(nb), dim3(CSCO_NT), lds, P);
        }
        if ((rc = launch_csc_value_sums(S, cols[b0], d_cols ? d_cols + b0 : nullptr, nb, st.ssum))) return rc;
        if ((rc = launch_gene_totals(c, st.ssum, G, nb, st.gtot))) return rc;
        if ((rc = finalize_listed(S, st, st.gtot, nb, cols, b0, d_cols, false, true))) return rc;
        const u32 *h_fb;
        if ((rc = read_gene_flags(c, st.flags, nb, &h_fb))) return rc;
        for (int64_t j = 0; j < nb; ++j)
            if (h_fb[j]) left.push_back(cols[b0 + j]);
    }
    cols.swap(left);
    return ILLICO_OK;
}

// ---- CSR, count-valued, rows in order: the group-major single pass (kernels_csr_counts.h) ----
// A sample of the stored values and the order of the rows' column indices are looked at ON THE DEVICE (d_verdict: the kernels leave
// every gene flagged when the matrix is not for them); then the row boundaries of the gene windows, the tables of the reference group
// (OVO) / of the whole column (OVR), the histograms of the groups above 255 cells, k_csr_counts and k_csr_big_sweep: p-values straight
// into the planes.  d_flags (device, [W] + 4 words for the verdict): the genes it could not take.  Nothing here waits for the host.
template <typename InT, typename IdxT>
static int launch_csr_counts_route(const SparseCall<InT, IdxT> &S, u32 *d_flags) {
    illico_ctx *c = S.c;
    const InT *d_data = S.d_data;
    const IdxT *d_indices = S.d_indices, *d_indptr = S.d_indptr;
    const int64_t n_rows = S.n_rows, n_cols = S.n_cols, col_lb = S.col_lb, col_ub = S.col_ub;
    const int flags = S.flags, alternative = S.alternative, G = S.G;
    const OutPlanes &o = S.o;
    const bool ovr = S.ovr;
    const int64_t W = col_ub - col_lb, Wpad = (W + 63) & ~63ll;
    const int n_big = c->csr_n_big, n_chunks = c->csr_n_chunks;
    int rc;
    u32 *d_verdict = d_flags + W;
    HIPCHK(c, hipMemsetAsync(d_flags, 0, (size_t)(W + 4) * 4, c->stream));
    KERNELCHK(c, k_sample_noncount_cols<InT, IdxT>, dim3((1 << 16) / 256), dim3(256), 0, d_data, d_indptr, 0ll, (long long)n_rows, 1 << 16, CSRC_RT, d_verdict);
    KERNELCHK(c, k_csr_density_verdict<IdxT>, dim3(1), dim3(1), 0, d_indptr, (long long)n_rows, (long long)n_cols, 0.3, d_verdict);
    // rows out of order: a call over every column finds them in its entry loops (a row's stretches then cover the row: an entry that
    // is not where the boundaries put it shows up outside its window); a column window asks the whole index array first -- unless the
    // matrix is a bound one, whose order was looked at when it was bound
    if (!(col_lb == 0 && col_ub == n_cols) && !c->cur_sorted_known)
        KERNELCHK(c, k_csr_sorted_check<IdxT>, dim3((unsigned)std::min<int64_t>((n_rows + 3) / 4 + 1, 8192)), dim3(256), 0, d_indices, d_indptr, (int)n_rows,
                  (int *)(d_verdict + 3));
    // windows of about 2048 genes: 72 KB of mixed cells, two workgroups per CU; equal widths
    const int n_win = (int)((W + 2047) / 2048);
    const int Wg = (int)((((W + n_win - 1) / n_win) + 63) & ~63ll);
    const int n_bnd = n_win + 1;
    u32 *bounds;
    if ((rc = scratch(c, "csrc_bounds", (size_t)n_bnd * n_rows, &bounds))) return rc;
    const size_t slab = (size_t)Wpad * 64;
    unsigned char *tables;
    if ((rc = scratch(c, "csrc_tables", slab * 4 * (size_t)(2 + n_big) + (size_t)Wpad * (16 + 8), &tables))) return rc;
    u32 *hist = (u32 *)tables, *tab = hist + slab * (size_t)(1 + n_big);
    uint4 *ginfo = (uint4 *)(tab + slab);
    double *gtot = (double *)(ginfo + Wpad);
    HIPCHK(c, hipMemsetAsync(hist, 0, slab * 4 * (size_t)(1 + n_big), c->stream));
    CsrCountsParams P;
    memset(&P, 0, sizeof P);
    P.data = d_data; P.indices = d_indices; P.indptr = d_indptr; P.perm = c->d_perm; P.pos_ptr = c->d_posptr; P.counts = c->d_counts;
    P.G = G; P.ref = (int)c->ref; P.n_cells = n_rows; P.col_lb = col_lb; P.W = (int)W; P.Wg = Wg; P.bounds = bounds; P.bstep = 1; P.n_bnd = n_bnd;
    P.tab = tab; P.ginfo = ginfo; P.gene_total = gtot; P.Wpad = Wpad; P.gene_flags = d_flags; P.verdict = d_verdict; P.unsorted = d_verdict + 3;
    P.use_continuity = (flags & ILLICO_FLAG_CONTINUITY) ? 1 : 0; P.tie_correct = (flags & ILLICO_FLAG_TIE_CORRECT) ? 1 : 0; P.alternative = alternative;
    P.out_p = o.p; P.out_u = o.u; P.out_fc = o.fc; P.out_z = o.z; P.out_ld = o.ld; P.hist = hist;
    P.chunk_p0 = c->d_csr_chunks; P.chunk_n = c->d_csr_chunks + n_chunks; P.chunk_slab = c->d_csr_chunks + 2 * n_chunks;
    P.big_groups = c->d_csr_chunks + 3 * n_chunks; P.n_big = n_big; P.abl = c->csr_counts_abl;
    {
        ProfScope ps(c, KID_SPARSE_SEG);
        const long long tot = (long long)n_rows * n_bnd;
        KERNELCHK(c, k_csr_row_bounds<IdxT>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, d_indices, d_indptr, (int)n_rows, (long long)n_cols,
                  (long long)col_lb, (long long)col_ub, Wg, n_bnd, bounds, (const u32 *)d_verdict);
    }
    {
        ProfScope ps(c, KID_FUSED_REF);
        if (n_chunks > 0) KERNELCHK(c, k_csr_hist<InT, IdxT>, dim3(n_win, n_chunks), dim3(CSRH_NT), csrh_lds_bytes(Wg), P); // the reference group (OVO), the big groups
        if (!ovr) KERNELCHK(c, k_csr_tables<false>, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, (const u32 *)hist, (long long)Wpad, (int)W, (long long)c->h_counts[c->ref], 0, tab, ginfo, gtot, (const u32 *)d_verdict);
    }
    const size_t lds = csrc_lds_bytes(Wg);
    if (ovr) {
        if ((rc = scratch(c, "csrc_dump", (size_t)G * n_win * CSRC_WPG * Wg, &P.dump))) return rc;
        {
            ProfScope ps(c, KID_CSR_COUNTS);
            KERNELCHK(c, k_csr_counts<InT, IdxT, true>, dim3(n_win, G), dim3(CSRC_NT), lds, P);
        }
        {
            ProfScope ps(c, KID_FUSED_REF);
            const int slices = std::max(1, std::min(G, (int)std::min<int64_t>(64, (1 << 20) / std::max<int64_t>(W, 1) + 1))); // ~a million threads
            const int gps = (G + slices - 1) / slices;
            KERNELCHK(c, k_csr_colhist, dim3((unsigned)((W + 255) / 256), (unsigned)((G + gps - 1) / gps)), dim3(256), 0, P, n_win, gps);
            KERNELCHK(c, k_csr_tables<true>, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, (const u32 *)hist, (long long)Wpad, (int)W, (long long)n_rows, n_big, tab, ginfo, gtot, (const u32 *)d_verdict);
        }
        ProfScope ps(c, KID_OVR_SCAN);
        KERNELCHK(c, o.z ? k_csr_ovr_sweep<true> : k_csr_ovr_sweep<false>, dim3(n_win, G), dim3(CSRC_NT), 0, P);
        if (n_big > 0) KERNELCHK(c, o.z ? k_csr_big_sweep<true, true> : k_csr_big_sweep<true>, dim3((unsigned)((W + 255) / 256), n_big), dim3(256), 0, P);
    } else {
        ProfScope ps(c, KID_CSR_COUNTS);
        KERNELCHK(c, k_csr_counts<InT, IdxT, false>, dim3(n_win, G), dim3(CSRC_NT), lds, P);
        if (n_big > 0) KERNELCHK(c, o.z ? k_csr_big_sweep<false, true> : k_csr_big_sweep<false>, dim3((unsigned)((W + 255) / 256), n_big), dim3(256), 0, P);
    }
    return ILLICO_OK;
}

// Host-resident sparse input whose stored values are counts below 255 (what a raw count matrix holds): the values travel as BYTES -- a
// quarter of a float32 array's share of the link; C3's 0.96 GB of values become 0.24 -- narrowed by host threads (on the NUMA node the array
// lives on) into two pinned 32-MB chunks, chunk k + 1 under the upload of chunk k, and widened again on the device (k_bytes_to_values) into
// the buffer the kernels read: the same values, bit for bit.  A value that is no integer in [0, 255) stops the attempt (*done = false:
// the caller uploads the array as it is).  `d_out` receives entries [k0, k1) of `data`.
#define SPB_CHUNK (32ll << 20)
// `meanwhile` runs on the calling thread while the values are narrowed and sent (the caller's upload of the index array: the link then
// carries both, the narrowing costs nothing on the clock); it runs in every case, exactly once; its status is returned first.
template <typename InT, typename Meanwhile>
static int upload_values_as_bytes(illico_ctx *c, const InT *data, int64_t k0, int64_t k1, InT *d_out, bool *done, Meanwhile &&meanwhile) {
    *done = false;
    const int64_t n = k1 - k0;
    bool look = !c->no_sparse_byte_values && n >= (4ll << 20);
    for (int64_t i = 0; i < 4096 && look; ++i) { // a look first: 4096 evenly spaced values
        uint8_t b;
        narrow_cells<InT>(data + k0 + (n - 1) * i / 4095, &b, 1);
        if (b == 255) look = false;
    }
    if (!look) return meanwhile();
    HostStage *hs = host_stage_of(c);
    for (int j = 0; j < 2; ++j) {
        if (!hs->sp_pin[j]) HIPCHK(c, hipHostMalloc(&hs->sp_pin[j], (size_t)SPB_CHUNK, hipHostMallocDefault));
        if (!hs->sp_up[j]) HIPCHK(c, hipEventCreateWithFlags(&hs->sp_up[j], hipEventDisableTiming));
    }
    int rc;
    uint8_t *d_bytes;
    if ((rc = scratch(c, "sp_bytes", (size_t)n, &d_bytes))) return rc;
    const int node = c->no_host_numa ? -1 : numa_node_of_buffer(data + k0, (size_t)n * sizeof(InT));
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(c->host_fill_threads > 0 ? c->host_fill_threads : 16, 64));
    bool bad = false;
    int hip_err = 0;
    std::thread producer([&] { // (a thread of its own: its CPU mask -- the array's NUMA node -- is inherited by the narrowing threads and ends with it)
        hipSetDevice(c->device);
        numa_confine_this_thread(node);
        int64_t chunk_no = 0;
        for (int64_t o = 0; o < n && !bad && !hip_err; o += SPB_CHUNK, ++chunk_no) {
            const int j = (int)(chunk_no & 1);
            const int64_t m = std::min<int64_t>(SPB_CHUNK, n - o);
            if (chunk_no >= 2 && hipEventSynchronize(hs->sp_up[j]) != hipSuccess) { hip_err = 1; break; }
            uint8_t *dst = (uint8_t *)hs->sp_pin[j];
            std::vector<int> flags((size_t)T, 0);
            auto piece = [&](int t) {
                const int64_t a = m * t / T, b = m * (t + 1) / T;
                narrow_cells<InT>(data + k0 + o + a, dst + a, b - a);
                int f = 0;
                for (int64_t i = a; i < b; ++i) f |= dst[i] == 255 ? 1 : 0;
                flags[(size_t)t] = f;
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < T; ++t) pool.emplace_back(piece, t);
            piece(0);
            for (auto &th : pool) th.join();
            for (int t = 0; t < T; ++t) bad = bad || flags[(size_t)t] != 0;
            if (bad) break;
            if (hipMemcpyAsync(d_bytes + o, dst, (size_t)m, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                hipEventRecord(hs->sp_up[j], c->stream) != hipSuccess) hip_err = 1;
        }
    });
    const int rc_meanwhile = meanwhile();
    producer.join();
    if (rc_meanwhile) return rc_meanwhile;
    if (hip_err) return fail(c, ILLICO_ERR_HIP, "upload of a sparse matrix's values as bytes failed");
    if (bad) { HIPCHK(c, hipStreamSynchronize(c->stream)); return ILLICO_OK; } // (the pinned chunks are free again; the caller uploads the values as they are)
    KERNELCHK(c, k_bytes_to_values<InT>, dim3(4096), dim3(256), 0, (const uint8_t *)d_bytes, (long long)n, d_out);
    c->h2d_input_bytes += n;
    *done = true;
    return ILLICO_OK;
}

// the group-major CSR pass, deferred: enqueued as a whole, its flags + verdict travel to pinned memory behind an event (resolve_pending_csc)
template <typename InT, typename IdxT>
static int run_csr_counts_deferred(const SparseCall<InT, IdxT> &S) {
    illico_ctx *c = S.c;
    const size_t bytes = (size_t)(S.W + 4) * 4;
    int rc, slot;
    u32 *d_flags;
    void *pin;
    if ((rc = scratch(c, "csrc_flags", (size_t)(S.W + 4), &d_flags))) return rc;
    if ((rc = launch_csr_counts_route(S, d_flags))) return rc;
    if ((rc = reserve_deferred_slot(c, bytes, &slot, &pin))) return rc;
    HIPCHK(c, hipMemcpyAsync(pin, d_flags, bytes, hipMemcpyDeviceToHost, c->stream));
    if ((rc = post_deferred_call(c, slot, 1, S.dtype, S.flags, S.alternative, S.n_rows, S.col_lb, S.col_ub, S.o))) return rc;
    PendingDense &q = c->pend;
    q.is_csr = true; q.sp_data = S.data; q.sp_indices = S.indices; q.sp_indptr = S.indptr; q.sorted_known = c->cur_sorted_known;
    q.idx_dtype = S.idx_dtype(); q.n_cols = S.n_cols;
    return ILLICO_OK;
}

// ---- the steps and routes of run_sparse_t, in its order.  A route sets *done when it computed the window (the call is over); left
// false, the next one is tried.  The CSC routes over column lists narrow `cols` to the genes they left instead. ----

// What the host needs of indptr: all of it for CSC (batch planning), its two ends for CSR (total stored entries).  Device arrays: on
// the context's stream (a blocking hipMemcpy runs on the null stream, which torch's side streams do not synchronise with); the sample
// of the stored values that the count-valued routes ask for rides along: one wait for both (device_probe without its own wait).
template <typename InT, typename IdxT>
static int fetch_indptr(SparseCall<InT, IdxT> &S) {
    illico_ctx *c = S.c;
    const IdxT *indptr = (const IdxT *)S.indptr;
    const int64_t n_ptr = S.n_ptr;
    IdxT ends[2] = {0, 0};
    if (S.in_dev) {
        if ((S.counts_route && S.W > 0) || S.window_route) {
            int rc = device_probe(c, S.h_sample, 4, [&](u32 *d_cnt) {
                return launch_kernel(c, k_sample_noncount_cols<InT, IdxT>, dim3((1 << 16) / 256), dim3(256), 0, S.d_data, S.d_indptr,
                                     (long long)(S.is_csr ? 0 : S.col_lb), (long long)(S.is_csr ? S.n_rows : S.col_ub), 1 << 16, S.is_csr ? FUSED_RT : CSCC_RT, d_cnt);
            }, false);
            if (rc) return rc;
            S.sampled = true;
        }
        if (S.is_csr) {
            HIPCHK(c, hipMemcpyAsync(&ends[0], indptr, sizeof(IdxT), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&ends[1], indptr + (n_ptr - 1), sizeof(IdxT), hipMemcpyDeviceToHost, c->stream));
        } else {
            S.h_indptr.resize(n_ptr);
            HIPCHK(c, hipMemcpyAsync(S.h_indptr.data(), indptr, n_ptr * sizeof(IdxT), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!S.is_csr) { ends[0] = S.h_indptr[0]; ends[1] = S.h_indptr[n_ptr - 1]; }
    } else {
        if (!S.is_csr) S.h_indptr.assign(indptr, indptr + n_ptr);
        ends[0] = indptr[0];
        ends[1] = indptr[n_ptr - 1];
    }
    S.total_nnz = (int64_t)ends[1];
    S.density = (double)S.total_nnz / ((double)std::max<int64_t>(S.n_rows, 1) * (double)std::max<int64_t>(S.n_cols, 1));
    if (ends[0] != 0) return fail(c, ILLICO_ERR_ARG, "indptr[0] must be 0");
    return ILLICO_OK;
}

// Host arrays: the device views.  CSR rows span every column: the whole matrix goes up; CSC: only the stored entries of the requested
// window.  The index array goes up on the copy stream while host threads narrow the values (count values below 255 travel as bytes: a
// quarter of their bytes over the link); the context's stream waits for it.
template <typename InT, typename IdxT>
static int upload_host_arrays(SparseCall<InT, IdxT> &S) {
    illico_ctx *c = S.c;
    int rc;
    IdxT *d_ptr, *d_idx;
    InT *d_val;
    if ((rc = scratch(c, "sp_indptr", S.n_ptr, &d_ptr))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_ptr, S.indptr, S.n_ptr * sizeof(IdxT), hipMemcpyHostToDevice, c->stream));
    S.d_indptr = d_ptr;
    const int64_t k0 = S.is_csr ? 0 : (int64_t)S.h_indptr[S.col_lb];
    const int64_t k1 = S.is_csr ? S.total_nnz : (int64_t)S.h_indptr[S.col_ub];
    const size_t cnt = (size_t)std::max<int64_t>(k1 - k0, 1);
    if ((rc = scratch(c, "sp_data", cnt, &d_val))) return rc;
    if ((rc = scratch(c, "sp_indices", cnt, &d_idx))) return rc;
    HostStage *hs = host_stage_of(c);
    if (!hs->copy) HIPCHK(c, hipStreamCreateWithFlags(&hs->copy, hipStreamNonBlocking));
    if (!hs->up[0]) HIPCHK(c, hipEventCreateWithFlags(&hs->up[0], hipEventDisableTiming));
    auto upload_indices = [&]() -> int {
        HIPCHK(c, hipMemcpyAsync(d_idx, (const IdxT *)S.indices + k0, (size_t)(k1 - k0) * sizeof(IdxT), hipMemcpyHostToDevice, hs->copy));
        HIPCHK(c, hipEventRecord(hs->up[0], hs->copy));
        HIPCHK(c, hipStreamWaitEvent(c->stream, hs->up[0], 0));
        return ILLICO_OK;
    };
    bool as_bytes = false;
    if ((rc = upload_values_as_bytes<InT>(c, (const InT *)S.data, k0, k1, d_val, &as_bytes, upload_indices))) return rc;
    if (!as_bytes) {
        HIPCHK(c, hipMemcpyAsync(d_val, (const InT *)S.data + k0, (size_t)(k1 - k0) * sizeof(InT), hipMemcpyHostToDevice, c->stream));
        c->h2d_input_bytes += (int64_t)((size_t)(k1 - k0) * sizeof(InT));
    }
    S.d_data = d_val;
    S.kshift = k0;
    S.d_indices = d_idx;
    c->h2d_input_bytes += (int64_t)(S.n_ptr * sizeof(IdxT) + (size_t)(k1 - k0) * sizeof(IdxT));
    return ILLICO_OK;
}

// `n` evenly spaced values (64k at the most) of the stored entries from k0 on: S.h_sample, for a table of `rt` values
template <typename InT, typename IdxT>
static int sample_stored_values(SparseCall<InT, IdxT> &S, int64_t k0, int64_t n, int rt) {
    const int n_samples = (int)std::min<int64_t>(n, 1 << 16);
    int rc = device_probe(S.c, S.h_sample, 2, [&](u32 *d_cnt) {
        return launch_kernel(S.c, k_sample_noncount<InT>, dim3((n_samples + 255) / 256), dim3(256), 0, S.d_data + (k0 - S.kshift), (long long)n, n_samples, rt, d_cnt);
    });
    S.h_sample[2] = (u32)n_samples;
    S.sampled = true;
    return rc;
}

// ---- CSR, count-valued, rows in order: the group-major single pass (kernels_csr_counts.h); ONE wait, for its flags + verdict.  Three
// outcomes: many genes left the pass -- the whole window again without it; some did -- those, in runs, by the exact sparse routes; the
// matrix was not for the pass -- its verdict words are the sample the dense-window route asks for, and the next route is tried ----
template <typename InT, typename IdxT, typename KeyT>
static int route_csr_counts(SparseCall<InT, IdxT> &S, bool *done) {
    if (!S.csr_counts || S.total_nnz <= 0) return ILLICO_OK;
    illico_ctx *c = S.c;
    const int64_t W = S.W;
    int rc;
    u32 *d_flags;
    if ((rc = scratch(c, "csrc_flags", (size_t)(W + 4), &d_flags))) return rc;
    if ((rc = launch_csr_counts_route(S, d_flags))) return rc;
    std::vector<u32> hf((size_t)W + 4);
    HIPCHK(c, hipMemcpyAsync(hf.data(), d_flags, (size_t)(W + 4) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (csr_counts_verdict_bad(hf.data() + W)) {
        S.h_sample[0] = hf[W]; S.h_sample[1] = hf[W + 1]; S.h_sample[2] = hf[W + 2];
        S.sampled = true;
        return ILLICO_OK;
    }
    *done = true;
    int64_t n_flagged = 0;
    for (int64_t j = 0; j < W; ++j) n_flagged += hf[j] ? 1 : 0;
    if (n_flagged * 16 > W) return S.template reenter<KeyT>(S.col_lb, S.col_ub, SparseAllow::after_csr_counts());
    // runs of flagged genes (closer than 32 genes: one run; the genes in between are recomputed, identically)
    for (int64_t j = 0; j < W;) {
        if (!hf[j]) { ++j; continue; }
        int64_t last = j;
        for (int64_t e = j + 1; e < W && e - last <= 32; ++e) if (hf[e]) last = e;
        if ((rc = S.template reenter<KeyT>(S.col_lb + j, S.col_lb + last + 1, SparseAllow::exact_window()))) return rc;
        j = last + 1;
    }
    return ILLICO_OK;
}

// ---- dense windows of a sparse call ----
// the widest window (a multiple of 64 genes) of `cell`-byte cells that the scratch cap holds
static int64_t dense_window_genes(const illico_ctx *c, int64_t n_rows, size_t cell) {
    int64_t wmax = (int64_t)((size_t)c->scratch_bytes / ((size_t)n_rows * cell)) & ~63ll;
    wmax = std::min<int64_t>(wmax, (1ll << 29));
    if (c->gene_batch > 0) wmax = std::min<int64_t>(wmax, (c->gene_batch + 63) & ~63ll);
    return wmax;
}
// the call's columns, window by window, in the "dense_window" scratch: body(w0, wn, ldD, window) fills and computes one
template <typename InT, typename IdxT, typename Body>
static int for_dense_windows(const SparseCall<InT, IdxT> &S, size_t cell, Body &&body) {
    const int64_t wmax = dense_window_genes(S.c, S.n_rows, cell);
    int rc;
    unsigned char *window;
    for (int64_t w0 = S.col_lb; w0 < S.col_ub; w0 += wmax) {
        const int64_t wn = std::min<int64_t>(wmax, S.col_ub - w0), ldD = (wn + 63) & ~63ll;
        if ((rc = scratch(S.c, "dense_window", (size_t)S.n_rows * ldD * cell, &window))) return rc;
        if ((rc = body(w0, wn, ldD, window))) return rc;
    }
    return ILLICO_OK;
}
// windows in the matrix's own type + the dense routes; densify(w0, wn, ldD, window) launches the kernel that writes one (its status)
template <typename InT, typename IdxT, typename KeyT, typename Densify>
static int run_dense_windows_own_type(const SparseCall<InT, IdxT> &S, Densify &&densify) {
    illico_ctx *c = S.c;
    return for_dense_windows(S, sizeof(InT), [&](int64_t w0, int64_t wn, int64_t ldD, void *v) -> int {
        {
            ProfScope ps(c, KID_DENSIFY);
            int rc = densify(w0, wn, ldD, (InT *)v);
            if (rc) return rc;
        }
        return run_dense_t<InT, KeyT>(c, v, S.dtype, S.n_rows, ldD, 0, wn, (S.flags | ILLICO_FLAG_INPUT_DEVICE) & ~ILLICO_FLAG_DEFER, S.alternative, S.o.shifted(w0 - S.col_lb));
    });
}

// ---- CSR, count-valued, not too sparse: dense byte windows + the fused single-pass kernels (k_csr_densify), then the exact sparse
// routes over the column window that covers the genes they left (it recomputes, identically, the good genes in between) ----
template <typename InT, typename IdxT, typename KeyT>
static int route_csr_byte_windows(SparseCall<InT, IdxT> &S, bool *done) {
    if (!S.window_route || S.density < 0.015 || S.total_nnz <= 0) return ILLICO_OK;
    illico_ctx *c = S.c;
    int rc;
    // worth it only for count-valued data: 64k evenly spaced stored values say (device-resident arrays: taken with the indptr copy)
    if (!S.sampled && (rc = sample_stored_values(S, 0, S.total_nnz, FUSED_RT))) return rc;
    // the genes this route cannot take are redone over the column window that covers them, so it needs nearly all of
    // them to fit: no non-integers, few values beyond the table
    if ((double)S.h_sample[0] > 0.02 * (double)S.h_sample[2] || (double)S.h_sample[1] > 0.005 * (double)S.h_sample[2]) return ILLICO_OK;
    *done = true;
    // byte cells (the fused kernels only take integers below 64): a quarter of the window's traffic both ways;
    // float32 cells behind "dense_window_f32"
    const bool bytes = !c->dense_window_f32;
    int64_t bad_lo = -1, bad_hi = -1;
    std::vector<u32> hf;
    rc = for_dense_windows(S, bytes ? 1 : 4, [&](int64_t w0, int64_t wn, int64_t ldD, void *v) -> int {
        {
            ProfScope ps(c, KID_SPARSE_SEG);
            const dim3 grid((unsigned)std::min<int64_t>(S.n_rows, 1 << 16));
            if (bytes)
                KERNELCHK(c, k_csr_densify<InT, IdxT, uint8_t>, grid, dim3(DENS_NT), 0, S.d_data, S.d_indices, S.d_indptr, (int)S.n_rows, (long long)w0, (int)wn,
                          (uint8_t *)v, (long long)ldD);
            else
                KERNELCHK(c, k_csr_densify<InT, IdxT, float>, grid, dim3(DENS_NT), 0, S.d_data, S.d_indices, S.d_indptr, (int)S.n_rows, (long long)w0, (int)wn,
                          (float *)v, (long long)ldD);
        }
        c->fused_tie_sparse = true; // (the window holds CSR input: the reference ranks it by its sparse path)
        const FusedCall q{v, ldD, 0, (int)wn, S.flags, S.alternative, S.o, w0 - S.col_lb};
        const int rcf = bytes ? run_fused_ovo<uint8_t>(c, q, hf) : run_fused_ovo<float>(c, q, hf);
        c->fused_tie_sparse = false;
        if (rcf) return rcf;
        for (int64_t j = 0; j < wn; ++j)
            if (hf[j] == 1u || hf[j] == 3u) { // (2 = taken by the fused route's second, wider pass)
                if (bad_lo < 0) bad_lo = w0 + j;
                bad_hi = w0 + j;
            }
        return ILLICO_OK;
    });
    if (rc || bad_lo < 0) return rc;
    return S.template reenter<KeyT>(bad_lo, bad_hi + 1, SparseAllow::exact_window());
}

// ---- float64 values that are float32 values throughout (device-resident input, nothing count-valued took it): the float32 kernels
// give the same bits and hold twice the keys per gene in LDS (C3 shape as CSR, continuous: 14 - 17 ms in float64, 6 in float32).  One
// probe over stored entries [k0, k1) (k1 > k0); the call is made again in float32 when it says so.  Not with is_log1p: the float32
// kernels form expm1 in float32, the float64 ones and the reference (utils/sparse/csr.py:282, csc.py:207) in float64.
template <typename InT, typename IdxT>
static int route_f64_as_f32(SparseCall<InT, IdxT> &S, long long k0, long long k1, bool *done) {
    if constexpr (std::is_same<InT, double>::value) {
        illico_ctx *c = S.c;
        int rc;
        float *v;
        u32 inexact = 1;
        if ((rc = device_probe(c, &inexact, 1, [&](u32 *d_inexact) {
                return launch_kernel(c, k_f64_is_f32, dim3(4096), dim3(256), 0, (const double *)S.d_data + k0, k1 - k0, d_inexact);
            }))) return rc;
        if (inexact) return ILLICO_OK;
        // (the copy covers the whole array up to k1, so that entry k of the caller's arrays stays entry k)
        if ((rc = scratch(c, "sp_f32", (size_t)k1, &v))) return rc;
        KERNELCHK(c, k_f64_to_f32, dim3(4096), dim3(256), 0, (const double *)S.d_data + k0, k1 - k0, v + k0);
        *done = true;
        return run_sparse_t<float, IdxT, u32>(c, S.is_csr, v, S.indices, S.indptr, ILLICO_F32, S.n_rows, S.n_cols, S.col_lb, S.col_ub, S.flags & ~ILLICO_FLAG_DEFER,
                                              S.alternative, S.o, S.allow.in_float32());
    }
    return ILLICO_OK;
}

// ---- CSR, any values, columns longer than the per-gene LDS kernels hold (a "sparse" matrix a fifth or more of whose cells are
// stored): a dense window in the matrix's own type + the dense routes.  The per-gene kernels behind the transposition keep a
// gene's keys in LDS (~36 000 four-byte keys, half as many eight-byte ones: long_column); longer columns fall to the general sort routes
// one by one -- C3 shape with 30 % of the cells stored and continuous values: 76 ms (OVR) / 37 ms (OVO) that way, against 12.6 ms for
// the same values handed over dense.
// OVR: the reference accumulates a sparse column's tie sum in float64 (sparse_ovr.py:49,83), the dense routes in exact integers;
// what separates them is the rounding of n0^3 (n0 zeros), 1.1e-16 of it, which reaches p as z^2 (1 - d)^3 / (6 d) x 1.1e-16 at a
// fraction d of cells stored: 6e-13 at |z| = 37 (p ~ 1e-300) for d = 0.04, the bound used here; below that the window stays with
// the sparse routes (kernels_finalize.h: tie_f64_sparse).
template <typename InT, typename IdxT, typename KeyT>
static int route_csr_dense_window(SparseCall<InT, IdxT> &S, bool *done) {
    illico_ctx *c = S.c;
    if (!(S.allow.dense_window && S.allow.transpose && !c->no_csr_densify_any && !c->tap && !c->big_n && S.n_rows < (1ll << 31) &&
          (S.many_groups || (S.density * (double)S.n_rows > long_column<KeyT>(c) && (c->ref >= 0 || S.density >= 0.04))) &&
          (size_t)S.n_rows * 64 * sizeof(InT) <= (size_t)c->scratch_bytes))
        return ILLICO_OK;
    *done = true;
    return run_dense_windows_own_type<InT, IdxT, KeyT>(S, [&](int64_t w0, int64_t wn, int64_t ldD, InT *D) {
        return launch_kernel(c, k_csr_densify<InT, IdxT, InT>, dim3((unsigned)std::min<int64_t>(S.n_rows, 1 << 16)), dim3(DENS_NT), 0, S.d_data, S.d_indices,
                             S.d_indptr, (int)S.n_rows, (long long)w0, (int)wn, D, (long long)ldD);
    });
}
// ---- CSC, the same (the columns' row indices must ascend: asked on the device; few, long parcels: the window's entries as one flat
// run, kernels_sparse.h) ----
template <typename InT, typename IdxT, typename KeyT>
static int route_csc_dense_window(SparseCall<InT, IdxT> &S, const std::vector<int64_t> &cols, bool *done) {
    illico_ctx *c = S.c;
    const int64_t W = S.W;
    if (S.allow.indices_are_codes || !S.allow.dense_window || c->no_csr_densify_any || c->tap || c->big_n || S.n_rows >= (1ll << 31) || W <= 0) return ILLICO_OK;
    const double nnz = (double)S.nnz_between(S.col_lb, S.col_ub);
    if (!(S.many_groups || ((int64_t)cols.size() == W && nnz / (double)W > long_column<KeyT>(c) && (c->ref >= 0 || nnz >= 0.04 * (double)W * (double)S.n_rows))) ||
        (size_t)S.n_rows * 64 * sizeof(InT) > (size_t)c->scratch_bytes)
        return ILLICO_OK;
    u32 h_order[2] = {0u, 0u};
    int rc = device_probe(c, h_order, 2, [&](u32 *d_bad) {
        return launch_kernel(c, k_flat_descents<IdxT>, dim3(4096), dim3(256), 0, S.d_indices, S.d_indptr + S.col_lb, (int)W, (long long)S.kshift, d_bad);
    });
    if (rc || h_order[0] != h_order[1]) return rc;
    *done = true;
    constexpr int RC = sizeof(InT) == 4 ? 128 : 64; // (33 KB tiles: four workgroups per CU)
    return run_dense_windows_own_type<InT, IdxT, KeyT>(S, [&](int64_t w0, int64_t wn, int64_t ldD, InT *D) {
        const dim3 grid((unsigned)(ldD / 64), (unsigned)((S.n_rows + RC * CDN_SUP - 1) / (RC * CDN_SUP)));
        return launch_kernel(c, k_csc_densify<InT, IdxT, RC>, grid, dim3(CDN_NT), 0, S.d_data, S.d_indices, S.d_indptr, (long long)S.kshift, (long long)w0,
                             (int)wn, (int)S.n_rows, D, (long long)ldD);
    });
}

// ---- CSR, any values: transpose the column window into CSC on the device (count, scan, gather or scatter), then the CSC routes on
// the result, whose indices are group codes ----
template <typename InT, typename IdxT, typename KeyT>
static int route_csr_transpose(SparseCall<InT, IdxT> &S, bool *done) {
    illico_ctx *c = S.c;
    if (!S.allow.transpose || c->no_csr_transpose_path || S.n_rows >= (1ll << 31)) return ILLICO_OK;
    *done = true;
    const InT *d_data = S.d_data;
    const IdxT *d_indices = S.d_indices, *d_indptr = S.d_indptr;
    const int64_t n_rows = S.n_rows, col_ub = S.col_ub;
    int rc;
    // sorted column indices (the reference's contract) allow the gather form of pass 2
    int sorted = (c->cur_sorted_known && !c->no_csr_tile_gather) ? 1 : 0; // (a bound matrix: looked at when it was bound)
    if (!sorted && !c->no_csr_tile_gather) {
        u32 bad = 0;
        if ((rc = device_probe(c, &bad, 1, [&](u32 *d_bad) {
                return launch_kernel(c, k_csr_sorted_check<IdxT>, dim3((unsigned)std::min<int64_t>((n_rows + 3) / 4 + 1, 8192)), dim3(256), 0, d_indices, d_indptr,
                                     (int)n_rows, (int *)d_bad);
            }))) return rc;
        sorted = bad ? 0 : 1;
    }
    const int cap = 8192; // LDS staging entries of k_csr_tile_gather
    int RB = 256;
    if (sorted) { // expected entries per (row block, 64-column tile) <= cap / 2
        const double per_row = std::max(S.density * TRG_COLS, 1e-9);
        RB = TRG_NT * TRG_RPT;
        while (RB > 64 && RB * per_row > cap / 2) RB >>= 1;
    }
    const int n_blocks = (int)((n_rows + RB - 1) / RB);
    // few row blocks (20 000 cells: 40): the counting pass takes a block's entries in slices, the gather form a window's tiles in stretches
    const int ny = (n_blocks >= 2048 || c->no_csr_transpose_split) ? 1 : std::min(16, (2048 + n_blocks - 1) / n_blocks);
    // the per-block column tables live in LDS: 16-bit counters in the counting pass (RB <= 512 entries per (block, column)), 32-bit
    // cursors in the scatter form of pass 2 (unsorted rows, or a (block, tile) piece beyond the gather form's staging)
    int64_t wmax = std::min<int64_t>(S.W, (sorted && RB <= 512) ? 65536 : 32768);
    for (int64_t w0 = S.col_lb; w0 < col_ub;) {
        const int64_t wn = std::min<int64_t>(wmax, col_ub - w0);
        u32 *counts, *col_total;
        if ((rc = scratch(c, "tr_counts", (size_t)n_blocks * wn, &counts))) return rc;
        if ((rc = scratch(c, "tr_cols", (size_t)(wn + 1) * 2 + 4, &col_total))) return rc;
        u32 *col_ptr = col_total + (wn + 1), *d_over = col_ptr + (wn + 1);
        u32 total = 0;
        {
            ProfScope ps(c, KID_SPARSE_SEG);
            HIPCHK(c, hipMemsetAsync(col_total + wn, 0, 4, c->stream));
            HIPCHK(c, hipMemsetAsync(d_over, 0, 4, c->stream));
            if (ny > 1) HIPCHK(c, hipMemsetAsync(counts, 0, (size_t)n_blocks * wn * 4, c->stream));
            KERNELCHK(c, k_csr_block_count<IdxT>, dim3(n_blocks, ny), dim3(TRC_NT), (size_t)((wn + 1) / 2) * 4, d_indices, d_indptr, (int)n_rows, RB, (long long)w0,
                      (int)wn, counts);
            KERNELCHK(c, k_col_block_scan, dim3((unsigned)((wn + 255) / 256)), dim3(256), 0, counts, n_blocks, (int)wn, col_total);
            KERNELCHK(c, k_gene_base_scan, dim3(1), dim3(1024), 0, (const u32 *)col_total, (int)wn + 1, col_ptr);
        }
        HIPCHK(c, hipMemcpyAsync(&total, col_ptr + wn, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // (a window whose stored entries reach 2^31 would wrap the 32-bit scan: such windows are halved before they
        //  get here -- 2^31 entries do not fit the scratch cap at 8+ bytes each)
        const size_t need = (size_t)std::max<u32>(total, 1) * (sizeof(InT) + 4);
        if ((need > (size_t)c->scratch_bytes || (double)S.total_nnz * (double)wn / (double)std::max<int64_t>(S.n_cols, 1) > 1.5e9) && wn > 64) {
            wmax = std::max<int64_t>(64, wn / 2);
            continue;
        }
        InT *t_data;
        int *t_rows;
        if ((rc = scratch(c, "tr_data", (size_t)std::max<u32>(total, 1), &t_data))) return rc;
        if ((rc = scratch(c, "tr_rows", (size_t)std::max<u32>(total, 1), &t_rows))) return rc;
        bool gathered = false;
        if (sorted) {
            ProfScope ps(c, KID_CSR_TILE_GATHER);
            const size_t lds = (size_t)cap * (sizeof(InT) + 4 + 1);
            KERNELCHK(c, k_csr_tile_gather<InT, IdxT>, dim3(n_blocks, ny), dim3(TRG_NT), lds, d_data, d_indices, d_indptr, (int)n_rows, RB, (long long)w0, (int)wn,
                      (const u32 *)counts, (const u32 *)col_total, (const u32 *)col_ptr, cap, (const int *)c->d_codes, t_data, t_rows, d_over);
            u32 over = 0;
            HIPCHK(c, hipMemcpyAsync(&over, d_over, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            gathered = over == 0; // a (block, tile) piece larger than the LDS staging: redo the window with the scatter form
        }
        if (!gathered && wn > 32768) { // (the scatter form keeps 32-bit cursors per column in LDS: narrower windows)
            wmax = 32768;
            continue;
        }
        if (!gathered) {
            ProfScope ps(c, KID_CSR_BLOCK_SCATTER);
            KERNELCHK(c, k_csr_block_scatter<InT, IdxT>, dim3(n_blocks), dim3(TR_NT), (size_t)wn * 4, d_data, d_indices, d_indptr, (int)n_rows, RB, (long long)w0,
                      (int)wn, (const u32 *)counts, (const u32 *)col_ptr, (const int *)c->d_codes, t_data, t_rows);
        }
        if ((rc = run_sparse_t<InT, int32_t, KeyT>(c, false, t_data, t_rows, col_ptr, S.dtype, n_rows, wn, 0, wn, S.flags | ILLICO_FLAG_INPUT_DEVICE, S.alternative,
                                                   S.o.shifted(w0 - S.col_lb), SparseAllow::transposed_codes())))
            return rc;
        w0 += wn;
    }
    return ILLICO_OK;
}

// per-gene stored-entry counts of the requested window
template <typename InT, typename IdxT>
static int count_gene_nnz(const SparseCall<InT, IdxT> &S, std::vector<int64_t> &gene_nnz) {
    illico_ctx *c = S.c;
    const int64_t W = S.W;
    gene_nnz.resize(W);
    if (!S.is_csr) {
        for (int64_t j = 0; j < W; ++j) gene_nnz[j] = S.nnz_between(S.col_lb + j, S.col_lb + j + 1);
        return ILLICO_OK;
    }
    int rc;
    u32 *d_cc;
    if ((rc = scratch(c, "sp_colcnt", std::max<size_t>(W, 1), &d_cc))) return rc;
    HIPCHK(c, hipMemsetAsync(d_cc, 0, W * 4, c->stream));
    {
        ProfScope ps(c, KID_SPARSE_SEG);
        KERNELCHK(c, k_csr_col_nnz<IdxT>, dim3(2048), dim3(256), 0, S.d_indices, (long long)S.total_nnz, (long long)S.col_lb, (long long)S.col_ub, d_cc);
    }
    std::vector<u32> h_cc(W);
    HIPCHK(c, hipMemcpyAsync(h_cc.data(), d_cc, W * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t j = 0; j < W; ++j) gene_nnz[j] = h_cc[j];
    return ILLICO_OK;
}

// ---- CSC, count-valued, small groups: k_csc_counts over the genes in `cols`, when a sample of the window's stored values says they
// are counts at all (large integers only take their own genes out: a column list) ----
template <typename InT, typename IdxT>
static int route_csc_counts(SparseCall<InT, IdxT> &S, std::vector<int64_t> &cols) {
    if (!S.counts_route) return ILLICO_OK;
    const int64_t k0 = (int64_t)S.h_indptr[S.col_lb], nnz = S.nnz_between(S.col_lb, S.col_ub);
    if (nnz <= 0) return ILLICO_OK;
    int rc;
    if (!S.sampled && (rc = sample_stored_values(S, k0, nnz, CSCC_RT))) return rc; // (device-resident arrays: taken with the indptr copy)
    if ((double)S.h_sample[0] > 0.02 * (double)S.h_sample[2]) return ILLICO_OK;
    return run_csc_counts_route(S, cols);
}

// ---- two-kernel route: regroup into HBM, then rank ----
template <typename KeyT>
struct TwoKernelBatch {
    int nb;                   // genes
    int64_t g0, g1, max_gene; // first column, one past the last (CSR windows are contiguous: cols[i] = col_lb + i), largest per-gene nnz
    KeyT *Xs;                 // the regrouped keys
    u32 *seg;                 // [nb][G + 1] where each (gene, group) run starts
    void *kb = nullptr;       // ping-pong buffers of the sorts (OVR, or OVO through the global sort)
    u32 *va = nullptr, *vb = nullptr, *gflags = nullptr; // (gflags: per gene, not count-valued -- where the histogram route is allowed)
    StatsPlanes st;
    const int *d_cols = nullptr; const u32 *d_base = nullptr; // CSC: column list of the batch, where each gene's keys start in Xs
};

// CSC: LDS-staged regroup first (coalesced stores, one read of every entry); genes too large for it are redone by k_csc_segment, which
// handles any size
template <typename InT, typename IdxT, typename KeyT>
static int regroup_csc_batch(const SparseCall<InT, IdxT> &S, const TwoKernelBatch<KeyT> &B) {
    illico_ctx *c = S.c;
    const int G = S.G, nb = B.nb;
    int rc;
    ProfScope ps(c, KID_SPARSE_SEG);
    const size_t fixed = (size_t)((G + 1 + 3) & ~3) * 4 + (size_t)CSCG_NT * 4;
    const int key_cap = fixed + 4096 < kMaxLds ? (int)std::min<size_t>((kMaxLds - fixed) / sizeof(KeyT), (size_t)CSCG_NT * CSCR_CACHE) : 0;
    u32 *d_fb = nullptr;
    if (!c->no_csc_regroup_lds && key_cap >= 4096) {
        if ((rc = scratch(c, "sp_fb", (size_t)nb, &d_fb))) return rc;
        HIPCHK(c, hipMemsetAsync(d_fb, 0, (size_t)nb * 4, c->stream));
        CscRegroupParams R;
        R.data = S.d_data; R.indices = S.d_indices; R.indptr = S.d_indptr; R.kshift = S.kshift; R.col0 = B.g0; R.gene_cols = B.d_cols;
        R.gene_base = B.d_base; R.nb = nb; R.codes = S.d_codes; R.G = G; R.key_cap = key_cap; R.count_limit = ovo_counts_limit(c); R.Xs = B.Xs;
        R.vals = B.va; R.seg_ptr = B.seg; R.gene_flags = B.gflags; R.fallback = d_fb;
        KERNELCHK(c, k_csc_regroup<InT, IdxT, KeyT>, dim3(nb), dim3(CSCG_NT), fixed + (size_t)key_cap * sizeof(KeyT), R);
    }
    return launch_kernel(c, k_csc_segment<InT, IdxT, KeyT>, dim3(nb), dim3(SEG_NT), seg_lds_bytes(G), S.d_data, S.d_indices, S.d_indptr, (long long)B.g0, nb,
                         S.d_codes, G, B.Xs, B.va, B.seg, B.gflags, ovo_counts_limit(c), B.d_cols, B.d_base, (long long)S.kshift, (const u32 *)d_fb);
}
// CSR: count per (gene, group), scan, scatter (global atomics)
template <typename InT, typename IdxT, typename KeyT>
static int regroup_csr_batch(const SparseCall<InT, IdxT> &S, const TwoKernelBatch<KeyT> &B) {
    illico_ctx *c = S.c;
    const int G = S.G, nb = B.nb;
    int rc;
    u32 *cursor;
    if ((rc = scratch(c, "sp_cursor", (size_t)nb * (G + 1) + (size_t)nb * 2, &cursor))) return rc;
    u32 *gene_tot = cursor + (size_t)nb * (G + 1);
    u32 *gene_base = gene_tot + nb;
    HIPCHK(c, hipMemsetAsync(B.seg, 0, (size_t)nb * (G + 1) * 4, c->stream));
    ProfScope ps(c, KID_SPARSE_SEG);
    const int rows_grid = (int)std::min<int64_t>((S.n_rows + 3) / 4, 8192);
    KERNELCHK(c, k_csr_count<InT, IdxT>, dim3(rows_grid), dim3(256), 0, S.d_data, S.d_indices, S.d_indptr, (int)S.n_rows, (long long)B.g0, (long long)B.g1,
              (const int *)c->d_codes, G, B.seg);
    KERNELCHK(c, k_seg_scan, dim3(nb), dim3(SEG_NT), seg_lds_bytes(G), B.seg, G, nb, gene_tot);
    KERNELCHK(c, k_gene_base_scan, dim3(1), dim3(1024), 0, (const u32 *)gene_tot, nb, gene_base);
    long long tot = (long long)nb * (G + 1);
    KERNELCHK(c, k_seg_add_base, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, B.seg, cursor, (const u32 *)gene_base, G, nb);
    return launch_kernel(c, k_csr_scatter<InT, IdxT, KeyT>, dim3(rows_grid), dim3(256), 0, S.d_data, S.d_indices, S.d_indptr, (int)S.n_rows, (long long)B.g0,
                         (long long)B.g1, (const int *)c->d_codes, G, cursor, B.Xs, B.va, B.gflags, ovo_counts_limit(c));
}
// Groups of hundreds / thousands of cells: the regrouped runs in the packed layout's terms, runs above 256 keys dealt into value
// buckets, then k_ovo_rank_compact (look-ups in the bucketed reference, pieces of 256 keys); what it leaves -- tie-heavy reference
// runs, *route -- and the count-valued genes (gflags == 0: k_ovo_counts) go on to launch_ovo
template <typename KeyT>
static int rank_packed_batch(illico_ctx *c, const TwoKernelBatch<KeyT> &B, const u32 *route_flags, u32 **route_out) {
    const int G = (int)c->n_groups, nb = B.nb;
    int rc;
    u16 *pk_nnz;
    u32 *pk_gofs;
    if ((rc = scratch(c, "sp_pk_nnz", (size_t)nb * G + (size_t)nb + 32, &pk_nnz))) return rc;
    u16 *ref_nnz = pk_nnz + (((size_t)nb * G + 7) & ~(size_t)7);
    if ((rc = scratch(c, "sp_pk_gofs", (size_t)nb * G + (size_t)nb, &pk_gofs))) return rc;
    u32 *route = pk_gofs + (size_t)nb * G;
    HIPCHK(c, hipMemsetAsync(route, 0, (size_t)nb * 4, c->stream));
    BigRunFn<KeyT> *big_fn = nullptr;
    {
        ProfScope ps(c, KID_GROUP_COMPACT);
        KERNELCHK(c, k_seg_to_packed, dim3((unsigned)(((size_t)nb * G + 255) / 256)), dim3(256), 0, (const u32 *)B.seg, G, nb, (int)c->ref, pk_nnz, pk_gofs,
                  ref_nnz, route, (const int *)nullptr, (u32 *)nullptr, 0); // (groups of at most 65535 cells here: 16-bit run lengths hold)
        if (c->pk_nbig > 0) {
            if ((rc = scratch(c, "packed_big_fn", (size_t)nb * c->pk_nbig, &big_fn))) return rc;
            const int64_t longest = std::min<int64_t>(c->max_nonref, B.max_gene);
            int cap = (int)std::min<int64_t>(srt_cap<KeyT>(), (longest + 63) & ~63ll);
            if (c->big_runs_cap > 0) cap = std::min(cap, std::max(c->big_runs_cap, 512) & ~63);
            // (runs beyond the LDS slots are dealt through the global sort's second key buffer)
            if ((rc = launch_bucket_big_runs<KeyT>(c, (void *)B.Xs, c->no_big_runs_global ? nullptr : B.kb, 0ll, pk_nnz, pk_gofs, nb, G, cap, big_fn, route, longest, nullptr, nullptr))) return rc;
        }
    }
    OvoCompactParams C;
    memset(&C, 0, sizeof C);
    C.Xs = B.Xs; C.gene_stride = 0; C.nnz = pk_nnz; C.gofs = pk_gofs; C.ref_out = 0; C.seg_nnz = ref_nnz; C.seg_sum = nullptr; C.out_sum = nullptr; C.nseg = 1;
    C.route = route; C.ref_by_gofs = 1; C.gene_flags = route_flags; C.big_fn = big_fn; C.big_tmp = B.kb; C.run_cuts = nullptr;
    // (a reference run longer than the kernel's key slots is taken in value-range parts; k_ovo_counts writes the count-valued genes' statistics afterwards)
    bool parts;
    *route_out = route;
    return launch_packed_rank<KeyT, false>(c, C, nb, std::min<int64_t>(c->h_counts[c->ref], std::max<int64_t>(B.max_gene, 1)), B.st.s2u, B.st.stie, &parts);
}

// one batch: genes cols[i0 .. i0 + nb) (list_nnz: their stored entries)
template <typename InT, typename IdxT, typename KeyT>
static int run_two_kernel_batch(const SparseCall<InT, IdxT> &S, const SparseBatch &b, const std::vector<int64_t> &cols, const std::vector<int64_t> &list_nnz) {
    illico_ctx *c = S.c;
    const int G = S.G;
    const bool ovr = S.ovr, is_csr = S.is_csr;
    int rc;
    TwoKernelBatch<KeyT> B;
    const int nb = B.nb = (int)(b.g1 - b.g0);
    const int64_t i0 = b.g0;
    B.g0 = cols[i0];
    B.g1 = cols[i0 + nb - 1] + 1;
    B.max_gene = b.max_gene;
    const size_t nnz = (size_t)std::max<int64_t>(b.nnz, 1);
    if ((rc = scratch(c, "xt", nnz, &B.Xs))) return rc;
    if ((rc = scratch(c, "sp_seg", (size_t)nb * (G + 1), &B.seg))) return rc;
    const int64_t ref_cap_b = ovr ? 0 : std::min<int64_t>(c->h_counts[c->ref], b.max_gene);
    const int64_t grp_cap_b = std::min<int64_t>(c->max_nonref, b.max_gene);
    const bool need_glob = !ovr && !ovo_sort_route_fits<KeyT>(ref_cap_b, grp_cap_b);
    if (ovr || need_glob) {
        KeyT *kb;
        if ((rc = scratch(c, "ovr_kb", nnz, &kb))) return rc;
        B.kb = kb;
        if ((rc = scratch(c, "ovr_va", nnz, &B.va))) return rc;
        if ((rc = scratch(c, "ovr_vb", nnz, &B.vb))) return rc;
    }
    const bool with_flags = counts_path_allowed(c, S.flags);
    if ((rc = carve_stats(c, nb, G, with_flags, &B.st))) return rc;
    B.gflags = B.st.flags;
    if (with_flags) HIPCHK(c, hipMemsetAsync(B.gflags, 0, (size_t)nb * 4, c->stream));
    if (!is_csr) {
        std::vector<int> h_cols(nb);
        std::vector<u32> h_base(nb);
        u32 run = 0;
        for (int j = 0; j < nb; ++j) {
            h_cols[j] = (int)cols[i0 + j];
            h_base[j] = run;
            run += (u32)list_nnz[i0 + j];
        }
        int *d_cols; // [nb] the columns, then [nb] where each gene's keys start
        if ((rc = scratch(c, "sp_cols", (size_t)nb * 2, &d_cols))) return rc;
        HIPCHK(c, hipMemcpyAsync(d_cols, h_cols.data(), (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_cols + nb, h_base.data(), (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // the host vectors go out of scope
        B.d_cols = d_cols;
        B.d_base = (const u32 *)(d_cols + nb);
    }
    const int64_t fin_off = is_csr ? B.g0 - S.col_lb : -S.col_lb; // CSC: col_map holds absolute columns
    if ((rc = is_csr ? regroup_csr_batch<InT, IdxT, KeyT>(S, B) : regroup_csc_batch<InT, IdxT, KeyT>(S, B))) return rc;
    // value sums first (the sorts permute Xs), exact whatever order the regroup left the runs in; the rank kernels then leave out_sum alone
    // (CSC: straight from the CSC arrays, accumulators in LDS -- the per-segment kernel spends a wavefront on every (gene, group)
    //  segment, a handful of entries each once there are thousands of groups: 9.4 ms against ~1.5 at C3 shape with 6000 groups)
    if (!is_csr) { if ((rc = launch_csc_value_sums(S, B.g0, B.d_cols, nb, B.st.ssum))) return rc; }
    else if ((rc = launch_seg_value_sums<KeyT>(c, B.Xs, B.seg, nb, S.dtype, S.flags, B.st.ssum))) return rc;
    if (ovr) {
        OvrParams P;
        P.keys_a = B.Xs; P.keys_b = B.kb; P.vals_a = B.va; P.vals_b = B.vb; P.code_by_pos = nullptr; P.seg_ptr = B.seg;
        P.stride = 0; P.pos_ptr = nullptr; P.counts = c->d_counts; P.G = G; P.n_genes = nb; P.dt = S.dtype;
        P.is_log1p = S.is_log1p() ? 1 : 0; P.n_cells = S.n_rows; P.ref = -1; P.gene_flags = nullptr;
        P.out_2u = B.st.s2u; P.out_tie = B.st.stie; P.out_sum = nullptr; P.tie_f64 = 1;
        if ((rc = launch_ovr_gene<KeyT, true>(c, P))) return rc;
        if ((rc = launch_gene_totals(c, B.st.ssum, G, nb, B.st.gtot))) return rc;
        return launch_finalize(c, B.st.s2u, B.st.stie, B.st.ssum, B.st.gtot, nb, S.flags, S.alternative, S.o, fin_off, B.d_cols, false, true);
    }
    OvoParams P;
    P.Xs = B.Xs; P.gene_stride = 0; P.pos_ptr = c->d_posptr; P.seg_ptr = B.seg; P.counts = c->d_counts;
    P.G = G; P.ref = (int)c->ref; P.n_genes = nb; P.dt = S.dtype; P.is_log1p = S.is_log1p() ? 1 : 0;
    P.ref_cap = 0; P.out_2u = B.st.s2u; P.out_tie = B.st.stie; P.out_sum = nullptr;
    const OvoGlobalBufs gb{B.kb, B.va, B.vb};
    // When the in-LDS sort route holds this batch it serves every gene (its lane-per-group form makes the
    // short runs of a sparse layout cheap for any key type); the histogram route is kept for the sizes it
    // alone can take without the global-sort fallback.
    const u32 *route_flags = need_glob ? B.gflags : nullptr;
    u32 *route = nullptr;
    if (sparse_packed_rank_fits(c, sizeof(KeyT) == 8 && !c->no_sparse_packed_small) && ovo_sort_route_fits<KeyT>(std::min<int64_t>(c->h_counts[c->ref], b.max_gene), 1024) &&
        (rc = rank_packed_batch<KeyT>(c, B, route_flags, &route))) return rc;
    if ((rc = launch_ovo<KeyT>(c, P, ref_cap_b, grp_cap_b, route_flags, &gb, true, route))) return rc;
    return launch_finalize(c, B.st.s2u, B.st.stie, B.st.ssum, nullptr, nb, S.flags, S.alternative, S.o, fin_off, B.d_cols);
}

// `cols`: the columns still to compute.  CSC batches are arbitrary column LISTS (the stragglers of the single-kernel routes are
// batched together); CSR batches are contiguous windows.
template <typename InT, typename IdxT, typename KeyT>
static int run_two_kernel_route(const SparseCall<InT, IdxT> &S, const std::vector<int64_t> &cols, const std::vector<int64_t> &gene_nnz) {
    illico_ctx *c = S.c;
    const bool may_glob = !S.ovr && !ovo_sort_route_fits<KeyT>(c->h_counts[c->ref], c->max_nonref);
    const size_t per_nnz = sizeof(KeyT) * ((S.ovr || may_glob) ? 2 : 1) + ((S.ovr || may_glob) ? 8 : 0);
    const size_t per_gene = (size_t)(S.G + 1) * 4 * (S.is_csr ? 2 : 1) + (size_t)S.G * 24 + 64;
    std::vector<int64_t> list_nnz(cols.size());
    for (size_t j = 0; j < cols.size(); ++j) list_nnz[j] = gene_nnz[cols[j] - S.col_lb];
    int rc;
    for (const SparseBatch &b : plan_batches(list_nnz, 0, per_nnz, per_gene, c->gene_batch, (size_t)c->scratch_bytes)) // (g0 / g1 index `cols`)
        if ((rc = run_two_kernel_batch<InT, IdxT, KeyT>(S, b, cols, list_nnz))) return rc;
    return ILLICO_OK;
}

// ---- the sparse half of DESIGN.md's route table, in its order ----
template <typename InT, typename IdxT, typename KeyT>
int run_sparse_t(illico_ctx *c, bool is_csr, const void *data, const void *indices, const void *indptr, int dtype,
                 int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, int alternative,
                 const OutPlanes &o, SparseAllow allow) {
    SparseCall<InT, IdxT> S = describe_sparse_call<InT, IdxT>(c, is_csr, data, indices, indptr, dtype, n_rows, n_cols, col_lb, col_ub, flags, alternative, o, allow);
    const int64_t W = S.W;
    int rc;
    bool done = false;
    // 1. the count passes of a deferred call, enqueued as a whole: no host wait
    if (S.deferrable() && S.counts_route && W > 0 && !allow.indices_are_codes && c->d_codes16 && !c->tap) return run_csc_counts_deferred(S);
    if (S.deferrable() && S.csr_counts) return run_csr_counts_deferred(S);
    // 2. / 3. indptr on the host (a value sample riding along), host arrays on the device
    if ((rc = fetch_indptr(S))) return rc;
    if (!S.in_dev && (rc = upload_host_arrays(S))) return rc;
    if (is_csr) {
        // 4. the group-major pass; 5. byte windows + the fused kernels
        if ((rc = route_csr_counts<InT, IdxT, KeyT>(S, &done)) || done) return rc;
        if ((rc = route_csr_byte_windows<InT, IdxT, KeyT>(S, &done)) || done) return rc;
        // 6. float64 that is float32 throughout (a call that no re-entry has narrowed yet)
        if (S.may_narrow() && allow.transpose && allow.csr_counts && S.total_nnz > 0 &&
            ((rc = route_f64_as_f32(S, 0, (long long)S.total_nnz, &done)) || done)) return rc;
        // 7. long columns: dense windows in the matrix's own type
        if ((rc = route_csr_dense_window<InT, IdxT, KeyT>(S, &done)) || done) return rc;
        if (S.many_groups) return fail(c, ILLICO_ERR_UNSUPPORTED, "CSR input with %d groups: beyond the regrouping kernels' LDS histogram, and the dense window was not available here", S.G);
        // 8. transposition to CSC on the device, then the CSC routes on the result
        if ((rc = route_csr_transpose<InT, IdxT, KeyT>(S, &done)) || done) return rc;
    }
    // 9. per-gene stored-entry counts; `cols`: the genes still to compute, narrowed by every route below (never empty here: run_with_outputs, core.hip, returns for an empty window before any driver runs, and no re-entry makes one)
    std::vector<int64_t> gene_nnz, cols(W);
    if ((rc = count_gene_nnz(S, gene_nnz))) return rc;
    for (int64_t j = 0; j < W; ++j) cols[j] = col_lb + j;
    if (!is_csr) {
        // 10. k_csc_counts ...
        if ((rc = route_csc_counts(S, cols)) || cols.empty()) return rc;
        // (6. and 7. for CSC, behind the histogram route: while it left every gene)
        if (S.may_narrow() && (int64_t)cols.size() == W && W > 0 && S.nnz_between(col_lb, col_ub) > 0 &&
            ((rc = route_f64_as_f32(S, (long long)S.h_indptr[col_lb], (long long)S.h_indptr[col_ub], &done)) || done)) return rc;
        if ((rc = route_csc_dense_window<InT, IdxT, KeyT>(S, cols, &done)) || done) return rc;
        if (S.many_groups) return fail(c, ILLICO_ERR_UNSUPPORTED, "CSC input with %d groups: beyond the regrouping kernels' LDS histogram, and the dense window was not available here (row indices out of order?)", S.G);
        // ... k_csc_gene (runs of more than 128 keys leave it, runs of 32 .. 128 are slow in it: the packed rank kernel then), k_csc_ovr_gene
        if (!S.ovr && !c->no_csc_gene_path && !sparse_packed_rank_fits(c) && ((rc = run_csc_gene_route<InT, IdxT, KeyT>(S, cols, gene_nnz)) || cols.empty())) return rc;
        if (S.ovr && !c->no_csc_ovr_gene_path) {
            int64_t max_nnz = 0;
            for (int64_t cc : cols) max_nnz = std::max(max_nnz, gene_nnz[cc - col_lb]);
            if ((rc = run_csc_ovr_route<InT, IdxT, KeyT>(S, max_nnz, cols)) || cols.empty()) return rc;
        }
    }
    // 11. the two-kernel route on what is left
    return run_two_kernel_route<InT, IdxT, KeyT>(S, cols, gene_nnz);
}
