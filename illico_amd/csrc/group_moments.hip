// illico_group_moments_{dense,csc,csr,bound}: per-(group, gene) exact sums of the values and of their squares, and the same over
// every other cell (kernels_group_moments.h); illico_ttest_from_moments / illico_student_t_pvalues: Welch's t-test from those
// planes (kernels_ttest.h).  A translation unit of its own: the kernels depend on nothing the other routes use; the host scaffolding
// (input description, common checks, sparse upload, type dispatch) is shared with the other group passes (group_pass.h).
#include "group_pass.h"
#include "kernels_group_moments.h"
#include "kernels_ttest.h"

namespace {

struct GmOutputs {
    double *sum, *sumsq, *sum_rest, *sumsq_rest;
    int64_t ld;
};

int gm_check(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, int flags, const GmOutputs &o) {
    int rc = check_matrix_input(c, in, col_lb, col_ub);
    if (rc) return rc;
    if (flags & ILLICO_FLAG_LOG1P)
        return fail(c, ILLICO_ERR_ARG, "ILLICO_FLAG_LOG1P: the moments are those of the values as given (the t-test is a test on the log values)");
    if (!o.sum && !o.sumsq && !o.sum_rest && !o.sumsq_rest) return fail(c, ILLICO_ERR_ARG, "all four output planes are null: nothing to compute");
    if (o.ld < col_ub - col_lb) return fail(c, ILLICO_ERR_ARG, "out_ld smaller than the chunk width");
    for (int64_t g = 0; g < c->n_groups; ++g)
        if (c->h_counts[g] > 2097151)
            return fail(c, ILLICO_ERR_UNSUPPORTED, "group %lld holds %d cells: the exact per-group sums hold up to 2097151", (long long)g, c->h_counts[g]);
    return ILLICO_OK;
}

template <typename InT>
int gm_dense_window(illico_ctx *c, const InT *X, int64_t ld, int64_t N, int wn, const GmChunk *d_ch, int n_ch, const GmPlanes &P) {
    {
        ProfScope ps(c, KID_GM_VMAX);
        const int gx = (wn + GM_NT - 1) / GM_NT;
        const int gy = (int)std::max<int64_t>(1, std::min<int64_t>((N + 63) / 64, (4096 + gx - 1) / gx));
        KERNELCHK(c, k_gm_dense_vmax<InT>, dim3(gx, gy), dim3(GM_NT), 0, X, (long long)ld, (long long)N, wn, P.vmax, P.vmaxq, P.nonfin);
    }
    if (n_ch) {
        ProfScope ps(c, KID_GM_DENSE);
        KERNELCHK(c, k_gm_dense<InT>, dim3(n_ch, (wn + GM_TILE - 1) / GM_TILE), dim3(GM_NT), 0, X, (long long)ld, wn, c->d_perm, d_ch, P);
    }
    return ILLICO_OK;
}

template <typename InT, typename IdxT>
int gm_sparse_window(illico_ctx *c, bool is_csr, const void *data, const void *indices, const void *indptr, long long kshift, long long col0, int64_t N,
                     int wn, int dt, const GmChunk *d_ch, int n_ch, const GmPlanes &P) {
    const int G = (int)c->n_groups;
    if (!is_csr) {
        const bool ldsg = G <= GM_CSC_LDS_G;
        GmCscParams C{data, indices, indptr, kshift, col0, c->d_codes, c->d_codes16, wn, G, dt};
        const size_t lds = gm_csc_lds_bytes(G, ldsg);
        ProfScope ps(c, KID_GM_CSC);
        const dim3 grid((unsigned)std::min<int64_t>(wn, 1 << 20));
        return launch_kernel(c, ldsg ? k_gm_csc<InT, IdxT, true> : k_gm_csc<InT, IdxT, false>, grid, dim3(GM_NT), lds, C, P);
    }
    {
        ProfScope ps(c, KID_GM_VMAX);
        const int gy = (wn + GM_VMAX_CW - 1) / GM_VMAX_CW;
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((N + 15) / 16, (2048 + gy - 1) / gy));
        KERNELCHK(c, k_gm_csr_vmax<InT, IdxT>, dim3(gx, gy), dim3(GM_NT), 0, (const InT *)data, (const IdxT *)indices, (const IdxT *)indptr, kshift, (long long)N, col0, wn, P.vmax, P.vmaxq, P.nonfin);
    }
    if (n_ch) {
        ProfScope ps(c, KID_GM_CSR);
        KERNELCHK(c, k_gm_csr<InT, IdxT>, dim3(n_ch, (wn + GM_CSR_CW - 1) / GM_CSR_CW), dim3(GM_NT), 0, (const InT *)data, (const IdxT *)indices, (const IdxT *)indptr, kshift, col0, wn, c->d_perm, d_ch, P);
    }
    return ILLICO_OK;
}

int gm_run(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, int flags, const GmOutputs &o) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = resolve_pending(c); // a plane written under ILLICO_FLAG_DEFER is complete only after its leftover genes
    if (rc) return rc;
    const int64_t W = col_ub - col_lb, G = c->n_groups, N = in.n_rows;
    if (W == 0) return ILLICO_OK;
    const bool out_dev = flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const int dt = in.dtype;
    const size_t esz = dtype_size(dt);

    // chunks of the groups' positions (dense, CSR)
    std::vector<GmChunk> hch;
    group_chunks(c, GM_CHUNK, hch);
    const int n_ch = (int)hch.size();
    GmChunk *d_ch = nullptr;
    if (n_ch) {
        if ((rc = scratch(c, "gm_chunks", hch.size(), &d_ch))) return rc;
        HIPCHK(c, hipMemcpyAsync(d_ch, hch.data(), hch.size() * sizeof(GmChunk), hipMemcpyHostToDevice, c->stream));
    }

    SparseOnDevice sp{}; // host-resident sparse input goes up once: CSC the entries of [col_lb, col_ub), CSR every row
    if (in.sparse && (rc = stage_sparse_input(c, in, col_lb, col_ub, "gm_upload", &sp))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the chunk list and the staged arrays came from pageable host memory)

    // column windows: the six [G][wn] planes (+ staged host outputs, + the staged rows of a host dense matrix) fit the scratch cap
    double *const outs[4] = {o.sum, o.sumsq, o.sum_rest, o.sumsq_rest};
    int n_out = 0;
    for (double *p : outs) n_out += p ? 1 : 0;
    const size_t per_col = (size_t)G * 48 + 64 + (out_dev ? 0 : (size_t)G * 8 * n_out) + ((!in.sparse && !in.on_dev) ? (size_t)N * esz : 0);
    const int64_t WW = std::max<int64_t>(1, std::min<int64_t>({W, (int64_t)((size_t)std::max<int64_t>(c->scratch_bytes, 1) / per_col), (int64_t)1 << 24}));
    const int n_part = (int)std::min<int64_t>(G, 32);
    unsigned char *base;
    if ((rc = scratch(c, "gm_planes", (size_t)WW * per_col + (size_t)n_part * WW * sizeof(GmTotal) + 256, &base))) return rc;
    const size_t GW = (size_t)G * WW;
    GmPlanes P;
    P.L0 = (long long *)base;
    P.L1 = P.L0 + GW;
    P.Q0 = P.L1 + GW;
    P.Q1 = P.Q0 + GW;
    P.cat = (u64 *)(P.Q1 + GW);
    P.ovf = P.cat + GW;
    P.vmax = P.ovf + GW;
    P.vmaxq = P.vmax + WW;
    P.nonfin = (int *)(P.vmaxq + WW);
    GmTotal *part = (GmTotal *)(((uintptr_t)(P.nonfin + WW) + 255) & ~(uintptr_t)255);
    unsigned char *stage = (unsigned char *)(part + (size_t)n_part * WW); // the staged host outputs, then the window's rows of a host dense matrix

    for (int64_t w0 = col_lb; w0 < col_ub; w0 += WW) {
        const int wn = (int)std::min<int64_t>(WW, col_ub - w0);
        P.W = wn;
        PlaneStage st(c, stage, w0 - col_lb, wn);
        GmOut O;
        O.sum = st.out(o.sum, o.ld, G, out_dev, false); O.sumsq = st.out(o.sumsq, o.ld, G, out_dev, false);
        O.sum_rest = st.out(o.sum_rest, o.ld, G, out_dev, false); O.sumsq_rest = st.out(o.sumsq_rest, o.ld, G, out_dev, false);
        O.ld = st.pitch(o.ld, out_dev);
        if (st.rc) return st.rc;
        void *xwin = st.rest(); // host dense: [N][wn] in the matrix's own type
        // the six planes, the two magnitude rows and the flags lie back to back: one clear (a narrower last window clears a little more than it uses)
        HIPCHK(c, hipMemsetAsync(P.L0, 0, GW * 48 + (size_t)WW * 20, c->stream));
        if (!in.sparse) {
            DenseWindow xw;
            if ((rc = stage_dense_window(c, in, w0, wn, wn, xwin, &xw))) return rc;
            rc = dispatch_value_type(dt, [&](auto t) {
                using InT = typename decltype(t)::type;
                return gm_dense_window<InT>(c, (const InT *)xw.X + xw.col0, xw.ld, N, wn, d_ch, n_ch, P);
            });
        } else {
            const long long col0 = w0 - sp.ptr_col0;
            rc = dispatch_value_index_type(dt, in.idx_dtype, [&](auto t, auto i) {
                return gm_sparse_window<typename decltype(t)::type, typename decltype(i)::type>(c, in.is_csr, sp.data, sp.indices, sp.indptr, sp.kshift, col0, N, wn,
                                                                                                 dt, d_ch, n_ch, P);
            });
        }
        if (rc) return rc;
        const int gx = (wn + GM_NT - 1) / GM_NT;
        {
            ProfScope ps(c, KID_GM_TOTALS);
            KERNELCHK(c, k_gm_totals, dim3(gx, n_part), dim3(GM_NT), 0, P, (int)G, wn, part);
        }
        {
            ProfScope ps(c, KID_GM_FINALIZE);
            const int gy = (int)std::max<int64_t>(1, std::min<int64_t>(G, (8192 + gx - 1) / gx));
            KERNELCHK(c, k_gm_finalize, dim3(gx, gy), dim3(GM_NT), 0, P, (int)G, wn, part, n_part, O);
        }
        if ((rc = st.finish())) return rc;
    }
    return ILLICO_OK;
}

int gm_entry(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, int flags, const GmOutputs &o) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    int rc = gm_check(c, in, col_lb, col_ub, flags, o);
    if (rc) return rc;
    if ((rc = check_matrix_arrays(c, in))) return rc;
    return gm_run(c, in, col_lb, col_ub, flags, o);
}

} // namespace

extern "C" int illico_group_moments_dense(illico_ctx *c, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t col_lb, int64_t col_ub,
                                          int flags, double *out_sum, double *out_sumsq, double *out_sum_rest, double *out_sumsq_rest, int64_t out_ld) {
    return gm_entry(c, dense_input(X, dtype, n_rows, n_cols, ld, flags), col_lb, col_ub, flags, {out_sum, out_sumsq, out_sum_rest, out_sumsq_rest, out_ld});
}
extern "C" int illico_group_moments_csc(illico_ctx *c, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                                        int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, double *out_sum, double *out_sumsq, double *out_sum_rest,
                                        double *out_sumsq_rest, int64_t out_ld) {
    return gm_entry(c, sparse_input(false, data, dtype, indices, indptr, idx_dtype, n_rows, n_cols, flags), col_lb, col_ub, flags,
                    {out_sum, out_sumsq, out_sum_rest, out_sumsq_rest, out_ld});
}
extern "C" int illico_group_moments_csr(illico_ctx *c, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                                        int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, double *out_sum, double *out_sumsq, double *out_sum_rest,
                                        double *out_sumsq_rest, int64_t out_ld) {
    return gm_entry(c, sparse_input(true, data, dtype, indices, indptr, idx_dtype, n_rows, n_cols, flags), col_lb, col_ub, flags,
                    {out_sum, out_sumsq, out_sum_rest, out_sumsq_rest, out_ld});
}
extern "C" int illico_group_moments_bound(illico_ctx *c, const illico_matrix *m, int64_t col_lb, int64_t col_ub, int flags, double *out_sum, double *out_sumsq,
                                          double *out_sum_rest, double *out_sumsq_rest, int64_t out_ld) {
    if (!c || !m) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    int rc = check_bound_matrix(c, m);
    if (rc) return rc;
    flags = bound_matrix_flags(flags);
    return gm_entry(c, sparse_input(m->is_csr, m->d_data, m->dtype, m->d_indices, m->d_indptr, m->idx_dtype, m->n_rows, m->n_cols, flags), col_lb, col_ub, flags,
                    {out_sum, out_sumsq, out_sum_rest, out_sumsq_rest, out_ld});
}

// ---- the t-test from moment planes -------------------------------------------------------------------------------------------------
extern "C" int illico_ttest_from_moments(illico_ctx *c, const double *sum, const double *sumsq, const double *sum_rest, const double *sumsq_rest, int64_t n_cols,
                                         int64_t in_ld, int variant, int alternative, int flags, double *out_p, double *out_t, double *out_df, double *out_mean,
                                         double *out_var, double *out_mean_ref, double *out_var_ref, int64_t out_ld) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    if (!c->has_groups) return fail(c, ILLICO_ERR_NO_GROUPS, "illico_set_groups has not been called");
    if (variant != ILLICO_TT_WELCH && variant != ILLICO_TT_OVERESTIM_VAR) return fail(c, ILLICO_ERR_ARG, "unknown t-test variant code %d", variant);
    int rc = check_alternative(c, alternative);
    if (rc) return rc;
    const bool ovr = c->ref < 0;
    if (!sum || !sumsq) return fail(c, ILLICO_ERR_ARG, "null sum / sumsq plane");
    if (ovr && (!sum_rest || !sumsq_rest)) return fail(c, ILLICO_ERR_ARG, "one-versus-rest needs the sum_rest and sumsq_rest planes");
    double *const outs[TT_N_OUT] = {out_p, out_t, out_df, out_mean, out_var, out_mean_ref, out_var_ref};
    int n_out = 0;
    for (double *p : outs) n_out += p ? 1 : 0;
    if (!n_out) return fail(c, ILLICO_ERR_ARG, "all output planes are null: nothing to compute");
    if (n_cols < 0 || in_ld < n_cols || out_ld < n_cols) return fail(c, ILLICO_ERR_ARG, "a pitch is smaller than the width (or the width is negative)");
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = resolve_pending(c))) return rc;
    const int64_t G = c->n_groups, W = n_cols;
    if (W == 0 || G == 0) return ILLICO_OK;
    const bool in_dev = flags & ILLICO_FLAG_INPUT_DEVICE, out_dev = flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const double *const ins[4] = {sum, sumsq, ovr ? sum_rest : nullptr, ovr ? sumsq_rest : nullptr};
    const int n_in = ovr ? 4 : 2;
    // column windows under the scratch cap (host planes are staged)
    StageWindows sw;
    if ((rc = plan_stage_windows(c, W, (in_dev ? 0 : (size_t)G * 8 * n_in) + (out_dev ? 0 : (size_t)G * 8 * n_out), kNoWindowCap, "tt_stage", &sw))) return rc;
    for (int64_t w0 = 0; w0 < W; w0 += sw.WW) {
        const int wn = (int)std::min<int64_t>(sw.WW, W - w0);
        PlaneStage st(c, sw.block, w0, wn);
        TtParams T;
        T.G = (int)G; T.W = wn; T.ref = (int)c->ref; T.n_cells = (long long)c->n_cells; T.counts = c->d_counts;
        T.variant = variant; T.alternative = alternative;
        T.S = st.in(ins[0], in_ld, G, in_dev); T.Q = st.in(ins[1], in_ld, G, in_dev);
        T.SR = st.in(ins[2], in_ld, G, in_dev); T.QR = st.in(ins[3], in_ld, G, in_dev);
        T.in_ld = st.pitch(in_ld, in_dev);
        for (int k = 0; k < TT_N_OUT; ++k) T.out[k] = st.out(outs[k], out_ld, G, out_dev, false);
        T.out_ld = st.pitch(out_ld, out_dev);
        if (st.rc) return st.rc;
        {
            ProfScope ps(c, KID_TTEST);
            const int gx = (wn + TT_NT - 1) / TT_NT;
            KERNELCHK(c, k_ttest_from_moments, dim3(gx, (unsigned)std::min<int64_t>(G, 65535)), dim3(TT_NT), 0, T);
        }
        if ((rc = st.finish())) return rc;
    }
    return ILLICO_OK;
}

extern "C" int illico_student_t_pvalues(illico_ctx *c, const double *t, const double *df, int64_t n, int alternative, int flags, double *out_p) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    int rc = check_alternative(c, alternative);
    if (rc) return rc;
    if (n < 0 || (n && (!t || !df || !out_p))) return fail(c, ILLICO_ERR_ARG, "null array or negative length");
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = resolve_pending(c))) return rc;
    if (n == 0) return ILLICO_OK;
    const bool in_dev = flags & ILLICO_FLAG_INPUT_DEVICE, out_dev = flags & ILLICO_FLAG_OUTPUT_DEVICE;
    StageWindows sw; // the one-row case: t and df in, p out
    if ((rc = plan_stage_windows(c, n, (in_dev ? 0 : 16) + (out_dev ? 0 : 8), (int64_t)1 << 24, "tt_stage", &sw))) return rc;
    for (int64_t i0 = 0; i0 < n; i0 += sw.WW) {
        const int64_t m = std::min(sw.WW, n - i0);
        PlaneStage st(c, sw.block, i0, m);
        const double *kt = st.in(t, n, 1, in_dev), *kd = st.in(df, n, 1, in_dev);
        double *kp = st.out(out_p, n, 1, out_dev, false);
        if (st.rc) return st.rc;
        {
            ProfScope ps(c, KID_TTEST);
            KERNELCHK(c, k_student_t_pvalues, dim3((unsigned)((m + TT_NT - 1) / TT_NT)), dim3(TT_NT), 0, kt, kd, (long long)m, alternative, kp);
        }
        if ((rc = st.finish())) return rc;
    }
    return ILLICO_OK;
}
