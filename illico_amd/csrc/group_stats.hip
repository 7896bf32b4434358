// illico_group_stats_{dense,csc,csr,bound}: per-(group, gene) non-zero counts and exact value sums, and the same over every other
// cell (kernels_group_stats.h).  A translation unit of its own: the kernels depend on nothing the Wilcoxon routes use; the host
// scaffolding (input description, common checks, sparse upload, type dispatch) is shared with the other group passes (group_pass.h).
#include "group_pass.h"
#include "kernels_group_stats.h"

namespace {

struct GsOutputs {
    int64_t *nnz, *nnz_rest;
    double *sum, *sum_rest;
    int64_t ld;
};

int gs_check(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, const GsOutputs &o) {
    int rc = check_matrix_input(c, in, col_lb, col_ub);
    if (rc) return rc;
    if (!o.nnz && !o.sum && !o.nnz_rest && !o.sum_rest) return fail(c, ILLICO_ERR_ARG, "all four output planes are null: nothing to compute");
    if (o.ld < col_ub - col_lb) return fail(c, ILLICO_ERR_ARG, "out_ld smaller than the chunk width");
    for (int64_t g = 0; g < c->n_groups; ++g)
        if (c->h_counts[g] > 2097151)
            return fail(c, ILLICO_ERR_UNSUPPORTED, "group %lld holds %d cells: the exact per-group sums hold up to 2097151", (long long)g, c->h_counts[g]);
    return ILLICO_OK;
}

template <typename InT>
int gs_dense_window(illico_ctx *c, const InT *X, int64_t ld, int64_t N, int wn, int dt, int log1p, const GsChunk *d_ch, int n_ch, const GsPlanes &P) {
    {
        ProfScope ps(c, KID_GS_VMAX);
        const int gx = (wn + GS_NT - 1) / GS_NT;
        const int gy = (int)std::max<int64_t>(1, std::min<int64_t>((N + 63) / 64, (4096 + gx - 1) / gx));
        KERNELCHK(c, k_gs_dense_vmax<InT>, dim3(gx, gy), dim3(GS_NT), 0, X, (long long)ld, (long long)N, wn, dt, log1p, P.vmax, P.nonfin);
    }
    if (n_ch) {
        ProfScope ps(c, KID_GS_DENSE);
        KERNELCHK(c, k_gs_dense<InT>, dim3(n_ch, (wn + GS_TILE - 1) / GS_TILE), dim3(GS_NT), 0, X, (long long)ld, wn, c->d_perm, d_ch, dt, log1p, P);
    }
    return ILLICO_OK;
}

template <typename InT, typename IdxT>
int gs_sparse_window(illico_ctx *c, bool is_csr, const void *data, const void *indices, const void *indptr, long long kshift, long long col0, int64_t N,
                     int wn, int dt, int log1p, const GsChunk *d_ch, int n_ch, const GsPlanes &P) {
    const int G = (int)c->n_groups;
    if (!is_csr) {
        const bool ldsg = G <= GS_CSC_LDS_G;
        GsCscParams C{data, indices, indptr, kshift, col0, c->d_codes, c->d_codes16, wn, G, dt, log1p};
        const size_t lds = gs_csc_lds_bytes(G, ldsg);
        ProfScope ps(c, KID_GS_CSC);
        const dim3 grid((unsigned)std::min<int64_t>(wn, 1 << 20));
        return launch_kernel(c, ldsg ? k_gs_csc<InT, IdxT, true> : k_gs_csc<InT, IdxT, false>, grid, dim3(GS_NT), lds, C, P);
    }
    {
        ProfScope ps(c, KID_GS_VMAX);
        const int gy = (wn + GS_VMAX_CW - 1) / GS_VMAX_CW;
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((N + 15) / 16, (2048 + gy - 1) / gy));
        KERNELCHK(c, k_gs_csr_vmax<InT, IdxT>, dim3(gx, gy), dim3(GS_NT), 0, (const InT *)data, (const IdxT *)indices, (const IdxT *)indptr, kshift, (long long)N, col0, wn, dt, log1p, P.vmax, P.nonfin);
    }
    if (n_ch) {
        ProfScope ps(c, KID_GS_CSR);
        KERNELCHK(c, k_gs_csr<InT, IdxT>, dim3(n_ch, (wn + GS_CSR_CW - 1) / GS_CSR_CW), dim3(GS_NT), 0, (const InT *)data, (const IdxT *)indices, (const IdxT *)indptr, kshift, col0, wn, c->d_perm, d_ch, dt, log1p, P);
    }
    return ILLICO_OK;
}

int gs_run(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, int flags, const GsOutputs &o) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = resolve_pending(c); // a plane written under ILLICO_FLAG_DEFER is complete only after its leftover genes
    if (rc) return rc;
    const int64_t W = col_ub - col_lb, G = c->n_groups, N = in.n_rows;
    if (W == 0) return ILLICO_OK;
    const bool out_dev = flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const int log1p = (flags & ILLICO_FLAG_LOG1P) ? 1 : 0, dt = in.dtype;
    const size_t esz = dtype_size(dt);

    // chunks of the groups' positions (dense, CSR)
    std::vector<GsChunk> hch;
    group_chunks(c, GS_CHUNK, hch);
    const int n_ch = (int)hch.size();
    GsChunk *d_ch = nullptr;
    if (n_ch) {
        if ((rc = scratch(c, "gs_chunks", hch.size(), &d_ch))) return rc;
        HIPCHK(c, hipMemcpyAsync(d_ch, hch.data(), hch.size() * sizeof(GsChunk), hipMemcpyHostToDevice, c->stream));
    }

    SparseOnDevice sp{}; // host-resident sparse input goes up once: CSC the entries of [col_lb, col_ub), CSR every row
    if (in.sparse && (rc = stage_sparse_input(c, in, col_lb, col_ub, "gs_upload", &sp))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the chunk list and the staged arrays came from pageable host memory)

    // column windows: the [G][wn] planes (+ staged host outputs, + the staged rows of a host dense matrix) fit the scratch cap
    const int n_out = (o.nnz ? 1 : 0) + (o.sum ? 1 : 0) + (o.nnz_rest ? 1 : 0) + (o.sum_rest ? 1 : 0);
    const size_t per_col = (size_t)G * 32 + 64 + (out_dev ? 0 : (size_t)G * 8 * n_out) + ((!in.sparse && !in.on_dev) ? (size_t)N * esz : 0);
    const int64_t WW = std::max<int64_t>(1, std::min<int64_t>({W, (int64_t)((size_t)std::max<int64_t>(c->scratch_bytes, 1) / per_col), (int64_t)1 << 24}));
    const int n_part = (int)std::min<int64_t>(G, 32);
    unsigned char *base;
    if ((rc = scratch(c, "gs_planes", (size_t)WW * per_col + (size_t)n_part * WW * sizeof(GsTotal) + 256, &base))) return rc;
    GsPlanes P;
    P.L0 = (long long *)base;
    P.L1 = P.L0 + (size_t)G * WW;
    P.cnt = P.L1 + (size_t)G * WW;
    P.cat = (u64 *)(P.cnt + (size_t)G * WW);
    P.vmax = P.cat + (size_t)G * WW;
    P.nonfin = (int *)(P.vmax + WW);
    GsTotal *part = (GsTotal *)(((uintptr_t)(P.nonfin + WW) + 255) & ~(uintptr_t)255);
    unsigned char *stage = (unsigned char *)(part + (size_t)n_part * WW); // the staged host outputs, then the window's rows of a host dense matrix

    for (int64_t w0 = col_lb; w0 < col_ub; w0 += WW) {
        const int wn = (int)std::min<int64_t>(WW, col_ub - w0);
        P.W = wn;
        PlaneStage st(c, stage, w0 - col_lb, wn);
        GsOut O;
        O.nnz = (long long *)st.out(o.nnz, o.ld, G, out_dev, false); O.sum = st.out(o.sum, o.ld, G, out_dev, false);
        O.nnz_rest = (long long *)st.out(o.nnz_rest, o.ld, G, out_dev, false); O.sum_rest = st.out(o.sum_rest, o.ld, G, out_dev, false);
        O.ld = st.pitch(o.ld, out_dev);
        if (st.rc) return st.rc;
        void *xwin = st.rest(); // host dense: [N][wn] in the matrix's own type
        HIPCHK(c, hipMemsetAsync(P.L0, 0, (size_t)G * wn * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(P.L1, 0, (size_t)G * wn * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(P.cnt, 0, (size_t)G * wn * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(P.cat, 0, (size_t)G * wn * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(P.vmax, 0, (size_t)wn * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(P.nonfin, 0, (size_t)wn * 4, c->stream));
        if (!in.sparse) {
            DenseWindow xw;
            if ((rc = stage_dense_window(c, in, w0, wn, wn, xwin, &xw))) return rc;
            rc = dispatch_value_type(dt, [&](auto t) {
                using InT = typename decltype(t)::type;
                return gs_dense_window<InT>(c, (const InT *)xw.X + xw.col0, xw.ld, N, wn, dt, log1p, d_ch, n_ch, P);
            });
        } else {
            const long long col0 = w0 - sp.ptr_col0;
            rc = dispatch_value_index_type(dt, in.idx_dtype, [&](auto t, auto i) {
                return gs_sparse_window<typename decltype(t)::type, typename decltype(i)::type>(c, in.is_csr, sp.data, sp.indices, sp.indptr, sp.kshift, col0, N, wn,
                                                                                                 dt, log1p, d_ch, n_ch, P);
            });
        }
        if (rc) return rc;
        const int gx = (wn + GS_NT - 1) / GS_NT;
        {
            ProfScope ps(c, KID_GS_TOTALS);
            KERNELCHK(c, k_gs_totals, dim3(gx, n_part), dim3(GS_NT), 0, P, (int)G, wn, part);
        }
        {
            ProfScope ps(c, KID_GS_FINALIZE);
            const int gy = (int)std::max<int64_t>(1, std::min<int64_t>(G, (8192 + gx - 1) / gx));
            KERNELCHK(c, k_gs_finalize, dim3(gx, gy), dim3(GS_NT), 0, P, (int)G, wn, part, n_part, O);
        }
        if ((rc = st.finish())) return rc;
    }
    return ILLICO_OK;
}

int gs_entry(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, int flags, const GsOutputs &o) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    int rc = gs_check(c, in, col_lb, col_ub, o);
    if (rc) return rc;
    if ((rc = check_matrix_arrays(c, in))) return rc;
    return gs_run(c, in, col_lb, col_ub, flags, o);
}

} // namespace

extern "C" int illico_group_stats_dense(illico_ctx *c, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t col_lb, int64_t col_ub,
                                        int flags, int64_t *out_nnz, double *out_sum, int64_t *out_nnz_rest, double *out_sum_rest, int64_t out_ld) {
    return gs_entry(c, dense_input(X, dtype, n_rows, n_cols, ld, flags), col_lb, col_ub, flags, {out_nnz, out_nnz_rest, out_sum, out_sum_rest, out_ld});
}
extern "C" int illico_group_stats_csc(illico_ctx *c, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                                      int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, int64_t *out_nnz, double *out_sum, int64_t *out_nnz_rest,
                                      double *out_sum_rest, int64_t out_ld) {
    return gs_entry(c, sparse_input(false, data, dtype, indices, indptr, idx_dtype, n_rows, n_cols, flags), col_lb, col_ub, flags,
                    {out_nnz, out_nnz_rest, out_sum, out_sum_rest, out_ld});
}
extern "C" int illico_group_stats_csr(illico_ctx *c, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                                      int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, int64_t *out_nnz, double *out_sum, int64_t *out_nnz_rest,
                                      double *out_sum_rest, int64_t out_ld) {
    return gs_entry(c, sparse_input(true, data, dtype, indices, indptr, idx_dtype, n_rows, n_cols, flags), col_lb, col_ub, flags,
                    {out_nnz, out_nnz_rest, out_sum, out_sum_rest, out_ld});
}
extern "C" int illico_group_stats_bound(illico_ctx *c, const illico_matrix *m, int64_t col_lb, int64_t col_ub, int flags, int64_t *out_nnz, double *out_sum,
                                        int64_t *out_nnz_rest, double *out_sum_rest, int64_t out_ld) {
    if (!c || !m) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    int rc = check_bound_matrix(c, m);
    if (rc) return rc;
    flags = bound_matrix_flags(flags);
    return gs_entry(c, sparse_input(m->is_csr, m->d_data, m->dtype, m->d_indices, m->d_indptr, m->idx_dtype, m->n_rows, m->n_cols, flags), col_lb, col_ub, flags,
                    {out_nnz, out_nnz_rest, out_sum, out_sum_rest, out_ld});
}
