// illico_group_value_hists_{dense,csc,csr}: per-(group, gene) histograms of the values 0 .. 255 from one pass over the matrix;
// illico_pairwise_from_hists: the Wilcoxon rank-sum test of every ordered pair of groups from those histograms (kernels_pairwise.h).
// A translation unit of its own: siblings of the one-versus-reference routes, which it does not touch; the host scaffolding of the
// histogram pass (input description, common checks, input staging, type dispatch) is shared with the other group passes (group_pass.h),
// the pair selection and the staging of the pair planes with the ranked pair route (pair_pass.h).
#include "pair_pass.h"
#include "kernels_pairwise.h"

namespace {

int pw_check(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, const uint32_t *H, const uint32_t *fl) {
    int rc = check_matrix_input(c, in, col_lb, col_ub);
    if (rc) return rc;
    if (col_ub > col_lb && (!H || !fl)) return fail(c, ILLICO_ERR_ARG, "null out_H / out_flags");
    return ILLICO_OK;
}

template <typename InT>
int pw_dense(illico_ctx *c, const void *X, int64_t ld, int64_t col0, int wn, int tiles, u32 *T, u32 *d_flags) {
    FusedParams P{};
    P.X = X; P.ld = ld; P.col0 = col0; P.ncols = wn;
    P.perm = c->d_perm; P.pos_ptr = c->d_posptr; P.counts = c->d_counts;
    P.G = (int)c->n_groups; P.ref = -1; P.n_cells = c->n_cells;
    P.gene_flags = d_flags;
    constexpr int NWH = GH_NT / 64;
    // positions per wavefront: ~2048 workgroups, at most 4096 positions (16-bit cells in LDS)
    const int wave_rows = (int)std::min<int64_t>(4096, std::max<int64_t>(256, (c->n_cells * tiles / (2048 * NWH) + 31) & ~31ll));
    const int64_t chunks = (c->n_cells + (int64_t)NWH * wave_rows - 1) / ((int64_t)NWH * wave_rows);
    if (chunks > 65535) return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld cells are more row stretches than one launch holds", (long long)c->n_cells);
    ProfScope ps(c, KID_PW_HIST_DENSE);
    KERNELCHK(c, k_group_value_hists<InT, PW_RT>, dim3(tiles, (unsigned)chunks), dim3(GH_NT), 0, P, T, wave_rows);
    return ILLICO_OK;
}

template <typename InT, typename IdxT>
int pw_sparse(illico_ctx *c, bool is_csr, const void *data, const void *indices, const void *indptr, long long kshift, long long col0, int wn, u32 *H,
              u32 *d_flags) {
    const int G = (int)c->n_groups;
    const long long N = c->n_cells;
    if (!is_csr) {
        const int gw = std::min(G, 128);
        const size_t lds = (size_t)gw * PW_RT * 4;
        ProfScope ps(c, KID_PW_HIST_CSC);
        return launch_kernel(c, k_pw_hists_csc<InT, IdxT>, dim3((unsigned)std::min(wn, 1 << 20)), dim3(PW_NT), lds, (const InT *)data, (const IdxT *)indices,
                             (const IdxT *)indptr, kshift, col0, c->d_codes, c->d_counts, N, G, wn, gw, H, d_flags);
    }
    HIPCHK(c, hipMemsetAsync(H, 0, (size_t)G * wn * PW_RT * 4, c->stream));
    {
        ProfScope ps(c, KID_PW_HIST_CSR);
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((N + 3) / 4, 1 << 16));
        KERNELCHK(c, k_pw_hists_csr<InT, IdxT>, dim3(gx), dim3(PW_NT), 0, (const InT *)data, (const IdxT *)indices, (const IdxT *)indptr, kshift, col0, c->d_codes, N, G,
                  wn, H, d_flags);
    }
    {
        ProfScope ps(c, KID_PW_HIST_FINISH);
        const long long rows = (long long)G * wn;
        KERNELCHK(c, k_pw_hists_bin0, dim3((unsigned)std::max<long long>(1, std::min<long long>((rows + 3) / 4, 1 << 16))), dim3(PW_NT), 0, H, c->d_counts, rows, wn);
    }
    return ILLICO_OK;
}

int pw_budget(illico_ctx *c, size_t need, const char *what) {
    if (need > (size_t)std::max<int64_t>(c->scratch_bytes, 1))
        return fail(c, ILLICO_ERR_OOM, "%s needs %zu bytes of device scratch, the budget (\"scratch_bytes\") is %lld: pass a narrower gene window", what, need,
                    (long long)c->scratch_bytes);
    return ILLICO_OK;
}

int pw_hists_run(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, int flags, uint32_t *out_H, uint32_t *out_flags) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = resolve_pending(c);
    if (rc) return rc;
    const int64_t W = col_ub - col_lb, G = c->n_groups, N = in.n_rows;
    if (W == 0) return ILLICO_OK;
    if (W > (int64_t)1 << 21) return fail(c, ILLICO_ERR_OOM, "a window of %lld genes: pass narrower gene windows", (long long)W);
    if (G > 65535) return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld groups: the histogram passes take up to 65535", (long long)G);
    const bool out_dev = flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const int dt = in.dtype, wn = (int)W, tiles = (wn + 63) / 64;
    const size_t esz = dtype_size(dt);
    const size_t h_bytes = (size_t)G * W * PW_RT * 4, t_bytes = in.sparse ? 0 : (size_t)G * tiles * PW_TILE_WORDS * 4;
    const size_t x_bytes = (!in.sparse && !in.on_dev) ? (size_t)N * W * esz : 0;
    if ((rc = pw_budget(c, (out_dev ? 0 : h_bytes + (size_t)W * 4) + t_bytes + x_bytes, "illico_group_value_hists"))) return rc;
    if (!in.sparse && (uint64_t)in.ld * esz > 0xFFFFFFFFull) return fail(c, ILLICO_ERR_UNSUPPORTED, "a row pitch of 4 GiB or more");
    u32 *d_H = out_H, *d_flags = out_flags;
    if (!out_dev) {
        if ((rc = scratch(c, "pw_hist_out", h_bytes / 4 + (size_t)W, &d_H))) return rc;
        d_flags = d_H + (size_t)G * W * PW_RT;
    }
    HIPCHK(c, hipMemsetAsync(d_flags, 0, (size_t)W * 4, c->stream));
    if (!in.sparse) {
        u32 *T;
        if ((rc = scratch(c, "pw_tiled", t_bytes / 4, &T))) return rc;
        HIPCHK(c, hipMemsetAsync(T, 0, t_bytes, c->stream));
        DenseWindow xw;
        unsigned char *xwin = nullptr;
        if (!in.on_dev && (rc = scratch(c, "pw_xwin", x_bytes, &xwin))) return rc;
        if ((rc = stage_dense_window(c, in, col_lb, W, W, xwin, &xw))) return rc;
        rc = dispatch_value_type(dt, [&](auto t) { return pw_dense<typename decltype(t)::type>(c, xw.X, xw.ld, xw.col0, wn, tiles, T, d_flags); });
        if (rc) return rc;
        ProfScope ps(c, KID_PW_HIST_FINISH);
        KERNELCHK(c, k_pw_transpose<true>, dim3(tiles, (unsigned)G), dim3(PW_NT), 0, d_H, T, (const int *)nullptr, wn, tiles);
    } else {
        SparseOnDevice sp; // host-resident sparse input goes up once: CSC the entries of [col_lb, col_ub), CSR every row
        if ((rc = stage_sparse_input(c, in, col_lb, col_ub, "pw_upload", &sp))) return rc;
        if (!in.on_dev) HIPCHK(c, hipStreamSynchronize(c->stream)); // (the arrays came from pageable host memory)
        // CSC: indptr is indexed by column (shifted by what was uploaded); CSR: by row, and col0 is the window's first column
        const long long col0 = in.is_csr ? col_lb : col_lb - sp.ptr_col0;
        rc = dispatch_value_index_type(dt, in.idx_dtype, [&](auto t, auto i) {
            return pw_sparse<typename decltype(t)::type, typename decltype(i)::type>(c, in.is_csr, sp.data, sp.indices, sp.indptr, sp.kshift, col0, wn, d_H, d_flags);
        });
        if (rc) return rc;
    }
    if (!out_dev) {
        HIPCHK(c, hipMemcpyAsync(out_H, d_H, h_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out_flags, d_flags, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return ILLICO_OK;
}

int pw_hists_entry(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, int flags, uint32_t *out_H, uint32_t *out_flags) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    int rc = pw_check(c, in, col_lb, col_ub, out_H, out_flags);
    if (rc) return rc;
    if ((rc = check_matrix_arrays(c, in))) return rc;
    return pw_hists_run(c, in, col_lb, col_ub, flags, out_H, out_flags);
}

} // namespace

extern "C" int illico_group_value_hists_dense(illico_ctx *c, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t col_lb,
                                              int64_t col_ub, int flags, uint32_t *out_H, uint32_t *out_flags) {
    return pw_hists_entry(c, dense_input(X, dtype, n_rows, n_cols, ld, flags), col_lb, col_ub, flags, out_H, out_flags);
}
extern "C" int illico_group_value_hists_csc(illico_ctx *c, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                                            int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, uint32_t *out_H, uint32_t *out_flags) {
    return pw_hists_entry(c, sparse_input(false, data, dtype, indices, indptr, idx_dtype, n_rows, n_cols, flags), col_lb, col_ub, flags, out_H, out_flags);
}
extern "C" int illico_group_value_hists_csr(illico_ctx *c, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                                            int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, uint32_t *out_H, uint32_t *out_flags) {
    return pw_hists_entry(c, sparse_input(true, data, dtype, indices, indptr, idx_dtype, n_rows, n_cols, flags), col_lb, col_ub, flags, out_H, out_flags);
}

extern "C" int illico_pairwise_from_hists(illico_ctx *c, const uint32_t *H, const uint32_t *gene_flags, const int64_t *counts, int64_t n_groups, int64_t n_cols,
                                          const int64_t *sel, int64_t n_sel, const double *sums, int64_t sums_ld, int flags, int alternative, double *out_p,
                                          double *out_u, double *out_fc, double *out_z, int64_t out_ld) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    int rc = check_alternative(c, alternative);
    if (rc) return rc;
    if (!counts || n_groups <= 0 || n_groups > 0x7FFFFFFF) return fail(c, ILLICO_ERR_ARG, "null counts or bad n_groups");
    const int64_t G = n_groups, W = n_cols, K = sel ? n_sel : G;
    if (K < 2) return fail(c, ILLICO_ERR_ARG, "%lld groups selected: a pair needs two", (long long)K);
    if (K > 46340) return fail(c, ILLICO_ERR_ARG, "%lld groups selected: more pairs than a launch holds", (long long)K);
    PairSelection S;
    if ((rc = select_pair_groups(c, G, sel, K, [&](int64_t g) { return (long long)counts[g]; }, &S))) return rc;
    if (W < 0 || out_ld < W) return fail(c, ILLICO_ERR_ARG, "out_ld smaller than n_cols (or n_cols negative)");
    if (sums && sums_ld < W) return fail(c, ILLICO_ERR_ARG, "sums_ld smaller than n_cols");
    if (W == 0) return ILLICO_OK;
    if (!H || !gene_flags || !out_p || !out_u || !out_fc) return fail(c, ILLICO_ERR_ARG, "null H, gene_flags or output plane");
    if (W > (int64_t)1 << 21) return fail(c, ILLICO_ERR_OOM, "a window of %lld genes: pass narrower gene windows", (long long)W);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = resolve_pending(c))) return rc;
    const bool in_dev = flags & ILLICO_FLAG_INPUT_DEVICE, out_dev = flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const int wn = (int)W, tiles = (wn + 63) / 64, n_out = out_z ? 4 : 3;
    const size_t t_bytes = (size_t)K * tiles * PW_TILE_WORDS * 4, h_bytes = (size_t)G * W * PW_RT * 4, s_bytes = sums ? (size_t)G * W * 8 : 0;
    const size_t plane = (size_t)K * K * W * 8;
    if ((rc = pw_budget(c, t_bytes + (in_dev ? 0 : h_bytes + (size_t)W * 4 + s_bytes) + (out_dev ? 0 : plane * n_out), "illico_pairwise_from_hists"))) return rc;
    unsigned char *pairs_block;
    if ((rc = scratch(c, "pw_pairs", t_bytes + (size_t)K * 16 + 64, &pairs_block))) return rc;
    u32 *T = (u32 *)pairs_block;
    long long *d_n = (long long *)(pairs_block + t_bytes);
    int *d_sel = (int *)(d_n + K);
    if ((rc = upload_pair_selection(c, S, d_n, d_sel))) return rc;
    const u32 *d_H = H, *d_flags = gene_flags;
    const double *d_sums = sums;
    int64_t d_sums_ld = sums_ld;
    if (!in_dev) {
        unsigned char *u;
        if ((rc = scratch(c, "pw_stage_in", h_bytes + (size_t)W * 4 + s_bytes + 64, &u))) return rc;
        if (sums) {
            if ((rc = stage_pair_sums(c, sums, sums_ld, G, W, u, &d_sums, &d_sums_ld))) return rc;
            u += s_bytes;
        }
        HIPCHK(c, hipMemcpyAsync(u, H, h_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(u + h_bytes, gene_flags, (size_t)W * 4, hipMemcpyHostToDevice, c->stream));
        d_H = (const u32 *)u; d_flags = (const u32 *)(u + h_bytes);
    }
    double *const outs[4] = {out_p, out_u, out_fc, out_z};
    double *stage_out = nullptr, *d_out[4];
    if (!out_dev && (rc = scratch(c, "pw_stage_out", plane / 8 * n_out + 8, &stage_out))) return rc;
    PlaneStage st(c, stage_out, 0, W);
    for (int k = 0; k < 4; ++k) d_out[k] = st.out(outs[k], out_ld, K * K, out_dev, true); // preloaded: the columns of flagged genes come back as they were
    if (st.rc) return st.rc;
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the selection and the staged arrays came from pageable host memory)
    PwParams P;
    P.T = T; P.gene_flags = d_flags; P.n = d_n; P.sel = d_sel; P.sums = d_sums; P.sums_ld = d_sums_ld;
    P.K = (int)K; P.W = wn; P.tiles = tiles; P.nrb = ((int)K + PW_RB - 1) / PW_RB;
    P.use_continuity = (flags & ILLICO_FLAG_CONTINUITY) ? 1 : 0;
    P.tie_correct = (flags & ILLICO_FLAG_TIE_CORRECT) ? 1 : 0;
    P.alternative = alternative;
    P.out_p = d_out[0]; P.out_u = d_out[1]; P.out_fc = d_out[2]; P.out_z = d_out[3]; P.out_ld = st.pitch(out_ld, out_dev);
    {
        ProfScope ps(c, KID_PW_PAIRS);
        KERNELCHK(c, k_pw_transpose<false>, dim3(tiles, (unsigned)K), dim3(PW_NT), 0, const_cast<u32 *>(d_H), T, (const int *)d_sel, wn, tiles);
        const dim3 grid((unsigned)((K * P.nrb + PW_NT / 64 - 1) / (PW_NT / 64)), (unsigned)tiles);
        if (out_z) KERNELCHK(c, k_pw_pairs<true>, grid, dim3(PW_NT), 0, P);
        else KERNELCHK(c, k_pw_pairs<false>, grid, dim3(PW_NT), 0, P);
    }
    return st.finish();
}
