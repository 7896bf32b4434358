// illico_pairwise_ranked_{dense,csc}: the Wilcoxon rank-sum test of every ordered pair of selected groups for genes of ANY float32 /
// int32 values, from one sorted walk per gene (kernels_pairwise_ranked.h).  A translation unit of its own, the
// sibling of pairwise.hip: per gene batch the transposition (k_transpose_permute*), the value-range partition (k_ovr_partition<u32>) --
// both instantiated here, as the dense one-versus-rest route launches them -- then k_pw_rank_pairs and k_pw_rank_emit.  CSC input is
// written out dense on the device batch by batch (k_csc_densify) and takes the same steps.
#include "pair_pass.h"
#include "../../include/illico_hip_ranked.h"
#include "kernels_pairwise_ranked.h"

namespace {

struct RankedArgs {
    const int64_t *sel; int64_t n_sel;
    const double *sums; int64_t sums_ld;
    int flags, alternative;
    double *out[4]; int64_t out_ld;
    uint32_t *out_left;
};

template <typename InT>
int pwr_transpose(illico_ctx *c, const void *X, int64_t ld, int64_t col0, int ncols, int N, u32 *Xt, int64_t stride) {
    ProfScope ps(c, KID_TRANSPOSE);
    dim3 grid((N + 63) / 64, (ncols + 63) / 64);
    constexpr int VEC = 16 / (int)sizeof(InT);
    const bool aligned = ((uintptr_t)X % 16 == 0) && (ld % VEC == 0) && (col0 % VEC == 0) && ((uintptr_t)Xt % 16 == 0) && (stride % 64 == 0);
    if (aligned)
        return launch_kernel(c, k_transpose_permute_vec<InT, u32, VEC>, grid, dim3(256), 0, (const InT *)X, (long long)ld, (long long)col0, ncols, (const int *)c->d_perm, N, Xt,
                             (long long)stride, (u32 *)nullptr, 0);
    return launch_kernel(c, k_transpose_permute<InT, u32>, grid, dim3(256), 0, (const InT *)X, (long long)ld, (long long)col0, ncols, (const int *)c->d_perm, N, Xt,
                         (long long)stride, (u32 *)nullptr, 0);
}

template <typename InT, typename IdxT>
int pwr_densify(illico_ctx *c, const SparseOnDevice &sp, int64_t c0, int wn, int64_t n_rows, InT *D, int64_t ldD) {
    constexpr int RC = 128; // (33 KB tiles of 4-byte values)
    ProfScope ps(c, KID_DENSIFY);
    const dim3 grid((unsigned)(ldD / 64), (unsigned)((n_rows + RC * CDN_SUP - 1) / (RC * CDN_SUP)));
    return launch_kernel(c, k_csc_densify<InT, IdxT, RC>, grid, dim3(CDN_NT), 0, (const InT *)sp.data, (const IdxT *)sp.indices, (const IdxT *)sp.indptr,
                         (long long)sp.kshift, (long long)c0, wn, (int)n_rows, D, (long long)ldD);
}
template <typename IdxT>
int pwr_csc_in_order(illico_ctx *c, const SparseOnDevice &sp, int64_t c0, int64_t W, bool *in_order) {
    u32 h_order[2] = {0u, 0u};
    int rc = device_probe(c, h_order, 2, [&](u32 *d_bad) {
        return launch_kernel(c, k_flat_descents<IdxT>, dim3(1024), dim3(256), 0, (const IdxT *)sp.indices, (const IdxT *)sp.indptr + c0, (int)W, (long long)sp.kshift, d_bad);
    });
    *in_order = h_order[0] == h_order[1];
    return rc;
}

template <typename InT>
int pwr_run(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, const RankedArgs &a, const PairSelection &S) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = resolve_pending(c);
    if (rc) return rc;
    const int64_t W = col_ub - col_lb, G = c->n_groups, N = in.n_rows, K = (int64_t)S.sel.size(), KK = K * K;
    const bool in_dev = in.on_dev, out_dev = a.flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const int n_out = a.out[3] ? 4 : 3;
    const int64_t stride = (N + 63) & ~63ll;
    int cap = pwr_record_cap((int)K, kMaxLds);
    if (c->pair_rank_cap > 0) cap = (int)std::min<int64_t>(cap, std::max<int64_t>(1024, c->pair_rank_cap & ~1023ll)); // tests: many small parts
    // ---- what stays for the whole call ----
    const size_t plane = (size_t)KK * W * 8, s_bytes = in_dev ? 0 : (size_t)G * W * 8;
    const size_t fixed = (out_dev ? 0 : plane * n_out + (size_t)W * 4) + s_bytes + (size_t)G * 4 + (size_t)K * 12 + 256;
    const bool stage_x = in.sparse || !in_dev; // a dense window of the batch in device scratch
    const size_t per_gene = (size_t)stride * 10 + (OVRP_PMAX + 1) * 4 + 16 + (size_t)KK * 16 + (stage_x ? (size_t)N * 4 : 0);
    const size_t budget = (size_t)std::max<int64_t>(c->scratch_bytes, 1);
    if (fixed + 64 * per_gene > budget)
        return fail(c, ILLICO_ERR_OOM, "illico_pairwise_ranked needs %zu bytes of device scratch for one batch of 64 genes, the budget (\"scratch_bytes\") is %lld",
                    fixed + 64 * per_gene, (long long)c->scratch_bytes);
    const int64_t batch = std::min<int64_t>({(W + 63) & ~63ll, (int64_t)((budget - fixed) / per_gene) & ~63ll, (int64_t)1 << 16});
    unsigned char *small_block;
    if ((rc = scratch(c, "pwr_small", (size_t)G * 4 + (size_t)K * 12 + 64, &small_block))) return rc;
    long long *d_n = (long long *)small_block;
    int *d_sel = (int *)(d_n + K), *d_slot = d_sel + K;
    std::vector<int> h_slot((size_t)G, -1);
    for (int64_t k = 0; k < K; ++k) h_slot[S.sel[k]] = (int)k;
    if ((rc = upload_pair_selection(c, S, d_n, d_sel))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_slot, h_slot.data(), (size_t)G * 4, hipMemcpyHostToDevice, c->stream));
    const double *d_sums = a.sums;
    int64_t d_sums_ld = a.sums_ld;
    if (!in_dev) {
        double *sums_stage;
        if ((rc = scratch(c, "pwr_sums", s_bytes / 8, &sums_stage))) return rc;
        if ((rc = stage_pair_sums(c, a.sums, a.sums_ld, G, W, sums_stage, &d_sums, &d_sums_ld))) return rc;
    }
    unsigned char *stage_out = nullptr;
    if (!out_dev && (rc = scratch(c, "pwr_stage_out", plane * n_out + (size_t)W * 4, &stage_out))) return rc;
    PlaneStage st(c, stage_out, 0, W);
    double *d_out[4];
    for (int k = 0; k < 4; ++k) d_out[k] = st.out(a.out[k], a.out_ld, KK, out_dev, true); // preloaded: the columns of genes that leave come back as they were
    u32 *d_left = st.out(a.out_left, W, 1, out_dev, false);
    if (st.rc) return st.rc;
    SparseOnDevice sp{};
    int64_t sp_c0 = 0; // column col_lb in sp.indptr
    if (in.sparse) {
        if ((rc = stage_sparse_input(c, in, col_lb, col_ub, "pwr_upload", &sp))) return rc;
        sp_c0 = col_lb - sp.ptr_col0;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the host vectors and the staged arrays came from pageable host memory)
    if (in.sparse) {
        bool in_order = false;
        rc = in.idx_dtype == ILLICO_IDX_I32 ? pwr_csc_in_order<int32_t>(c, sp, sp_c0, W, &in_order) : pwr_csc_in_order<int64_t>(c, sp, sp_c0, W, &in_order);
        if (rc) return rc;
        if (!in_order) return fail(c, ILLICO_ERR_UNSORTED, "the row indices of a CSC column do not ascend: sort them (scipy: sort_indices())");
    }
    // ---- per batch ----
    u32 *Xt, *pkeys, *part_start;
    u16 *pcodes;
    long long *s2;
    if ((rc = scratch(c, "pwr_xt", (size_t)batch * stride, &Xt))) return rc;
    if ((rc = scratch(c, "pwr_pkeys", (size_t)batch * stride, &pkeys))) return rc;
    if ((rc = scratch(c, "pwr_pcodes", (size_t)batch * stride, &pcodes))) return rc;
    if ((rc = scratch(c, "pwr_meta", (size_t)batch * ((OVRP_PMAX + 1) + 4) + 16, &part_start))) return rc;
    u32 *gene_info = part_start + (size_t)batch * (OVRP_PMAX + 1), *gene_ctr = gene_info + (size_t)batch * 4;
    if ((rc = scratch(c, "pwr_stats", (size_t)batch * KK * 2, &s2))) return rc;
    u64 *tie = (u64 *)(s2 + (size_t)batch * KK);
    InT *xwin = nullptr;
    if (stage_x && (rc = scratch(c, "pwr_xwin", (size_t)N * batch, &xwin))) return rc;
    int n_cu = 256;
    hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
    const size_t lds = pwr_lds_bytes((int)K, cap);
    for (int64_t b0 = 0; b0 < W; b0 += batch) {
        const int nb = (int)std::min<int64_t>(batch, W - b0);
        const int64_t ldw = (nb + 63) & ~63ll;
        DenseWindow xw{xwin, ldw, 0}; // (CSC: the batch written out dense)
        if (!in.sparse) rc = stage_dense_window(c, in, col_lb + b0, nb, ldw, xwin, &xw);
        else if (in.idx_dtype == ILLICO_IDX_I32) rc = pwr_densify<InT, int32_t>(c, sp, sp_c0 + b0, nb, N, xwin, ldw);
        else rc = pwr_densify<InT, int64_t>(c, sp, sp_c0 + b0, nb, N, xwin, ldw);
        if (rc) return rc;
        if ((rc = pwr_transpose<InT>(c, xw.X, xw.ld, xw.col0, nb, (int)N, Xt, stride))) return rc;
        {
            OvrPartParams Q;
            Q.Xt = Xt; Q.stride = stride; Q.n_genes = nb; Q.n_cells = (int)N; Q.code_by_pos = c->d_code_by_pos; Q.cap = cap;
            Q.out_keys = pkeys; Q.out_codes = pcodes; Q.part_start = part_start; Q.gene_info = gene_info;
            ProfScope ps(c, KID_OVR_PART);
            KERNELCHK(c, k_ovr_partition<u32>, dim3(nb), dim3(OVRP_NT), ovrp_lds_bytes(), Q);
        }
        HIPCHK(c, hipMemsetAsync(gene_ctr, 0, 4, c->stream));
        {
            PwRankParams P;
            P.pkeys = pkeys; P.pcodes = pcodes; P.pstride = stride; P.part_start = part_start; P.gene_info = gene_info; P.slot_of = d_slot; P.n = d_n;
            P.gene_counter = gene_ctr; P.nb = nb; P.K = (int)K; P.cap = cap; P.is_float = in.dtype == ILLICO_F32 ? 1 : 0;
            P.out_s2 = s2; P.out_tie = tie; P.left = d_left + b0;
            ProfScope ps(c, KID_PW_RANK_PAIRS);
            KERNELCHK(c, k_pw_rank_pairs, dim3((unsigned)std::min(nb, std::max(n_cu, 1))), dim3(PWR_NT), lds, P); // one resident workgroup per CU (LDS)
        }
        {
            PwRankEmitParams E;
            E.s2 = s2; E.tie = tie; E.left = d_left + b0; E.n = d_n; E.sel = d_sel; E.sums = d_sums; E.sums_ld = d_sums_ld; E.K = (int)K; E.nb = nb;
            E.col_off = b0; E.use_continuity = (a.flags & ILLICO_FLAG_CONTINUITY) ? 1 : 0; E.tie_correct = (a.flags & ILLICO_FLAG_TIE_CORRECT) ? 1 : 0;
            E.alternative = a.alternative;
            E.out_p = d_out[0]; E.out_u = d_out[1]; E.out_fc = d_out[2]; E.out_z = d_out[3]; E.out_ld = st.pitch(a.out_ld, out_dev);
            const dim3 grid((unsigned)((nb + 63) / 64), (unsigned)((KK + PWE_PAIRS - 1) / PWE_PAIRS));
            ProfScope ps(c, KID_PW_RANK_EMIT);
            if (d_out[3]) KERNELCHK(c, k_pw_rank_emit<true>, grid, dim3(PWE_NT), 0, E);
            else KERNELCHK(c, k_pw_rank_emit<false>, grid, dim3(PWE_NT), 0, E);
        }
    }
    if ((rc = st.finish())) return rc;
    if (out_dev && !in_dev) HIPCHK(c, hipStreamSynchronize(c->stream));
    return ILLICO_OK;
}

int pwr_entry(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, const RankedArgs &a) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    int rc = check_alternative(c, a.alternative);
    if (rc || (rc = check_matrix_input(c, in, col_lb, col_ub))) return rc;
    if (in.dtype != ILLICO_F32 && in.dtype != ILLICO_I32)
        return fail(c, ILLICO_ERR_UNSUPPORTED, "illico_pairwise_ranked takes float32 / int32 values (an 8-byte key does not pack into its 8-byte record)");
    if ((rc = check_matrix_arrays(c, in))) return rc;
    const int64_t G = c->n_groups, W = col_ub - col_lb, K = a.sel ? a.n_sel : G;
    if (K < 2) return fail(c, ILLICO_ERR_ARG, "%lld groups selected: a pair needs two", (long long)K);
    if (K > PWR_KMAX) return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld groups selected: the ranked pair route takes up to %d", (long long)K, PWR_KMAX);
    if (G > 65535) return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld groups: the ranked pair route takes up to 65535", (long long)G);
    if (in.n_rows >= (1ll << 31) - 64) return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld cells: the ranked pair route takes fewer than 2^31", (long long)in.n_rows);
    PairSelection S;
    if ((rc = select_pair_groups(c, G, a.sel, K, [&](int64_t g) { return (long long)c->h_counts[g]; }, &S))) return rc;
    if (a.out_ld < W) return fail(c, ILLICO_ERR_ARG, "out_ld smaller than the window");
    if (a.sums_ld < W) return fail(c, ILLICO_ERR_ARG, "sums_ld smaller than the window");
    if (W == 0) return ILLICO_OK;
    if (!a.sums || !a.out[0] || !a.out[1] || !a.out[2] || !a.out_left) return fail(c, ILLICO_ERR_ARG, "null sums, output plane or out_left");
    if (W > (int64_t)1 << 21) return fail(c, ILLICO_ERR_OOM, "a window of %lld genes: pass narrower gene windows", (long long)W);
    if (!in.sparse && (uint64_t)in.ld * 4 > 0xFFFFFFFFull) return fail(c, ILLICO_ERR_UNSUPPORTED, "a row pitch of 4 GiB or more");
    if (in.dtype == ILLICO_F32) return pwr_run<float>(c, in, col_lb, col_ub, a, S);
    return pwr_run<int32_t>(c, in, col_lb, col_ub, a, S);
}

} // namespace

extern "C" int illico_pairwise_ranked_dense(illico_ctx *c, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t col_lb, int64_t col_ub,
                                            const int64_t *sel, int64_t n_sel, const double *sums, int64_t sums_ld, int flags, int alternative, double *out_p,
                                            double *out_u, double *out_fc, double *out_z, int64_t out_ld, uint32_t *out_left) {
    return pwr_entry(c, dense_input(X, dtype, n_rows, n_cols, ld, flags), col_lb, col_ub,
                     RankedArgs{sel, n_sel, sums, sums_ld, flags, alternative, {out_p, out_u, out_fc, out_z}, out_ld, out_left});
}
extern "C" int illico_pairwise_ranked_csc(illico_ctx *c, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                                          int64_t n_cols, int64_t col_lb, int64_t col_ub, const int64_t *sel, int64_t n_sel, const double *sums, int64_t sums_ld,
                                          int flags, int alternative, double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld,
                                          uint32_t *out_left) {
    return pwr_entry(c, sparse_input(false, data, dtype, indices, indptr, idx_dtype, n_rows, n_cols, flags), col_lb, col_ub,
                     RankedArgs{sel, n_sel, sums, sums_ld, flags, alternative, {out_p, out_u, out_fc, out_z}, out_ld, out_left});
}
