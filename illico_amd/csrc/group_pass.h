// Host scaffolding of the units that read the matrix once per group family -- group_stats.hip, group_moments.hip, and through
// pair_pass.h pairwise.hip and pairwise_ranked.hip: the description of the input, the checks every entry point makes, the upload of
// host-resident sparse arrays and dense windows, the dispatch on the index type, and the groups' positions in chunks.  It brings in
// plane_stage.h, the staging of host planes, which is all that pair_ttest.hip and blocked.hip take from here (markers.hip includes
// that header alone).  Everything is local to the including unit (all are linked into one library).  The kernels, the planes, the
// column windows, the outputs and the points at which the stream is synchronised are each family's own.
#pragma once
#include "engine.h"
#include "plane_stage.h"

namespace {

struct MatrixInput {
    bool sparse = false, is_csr = false, on_dev = false;
    const void *X = nullptr; // dense
    int64_t ld = 0;
    const void *data = nullptr, *indices = nullptr, *indptr = nullptr; // sparse
    int idx_dtype = 0;
    int dtype = 0;
    int64_t n_rows = 0, n_cols = 0;
};
inline MatrixInput dense_input(const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld, int flags) {
    MatrixInput in;
    in.X = X; in.dtype = dtype; in.n_rows = n_rows; in.n_cols = n_cols; in.ld = ld; in.on_dev = flags & ILLICO_FLAG_INPUT_DEVICE;
    return in;
}
inline MatrixInput sparse_input(bool is_csr, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                                int64_t n_cols, int flags) {
    MatrixInput in;
    in.sparse = true; in.is_csr = is_csr; in.data = data; in.indices = indices; in.indptr = indptr; in.idx_dtype = idx_dtype; in.dtype = dtype;
    in.n_rows = n_rows; in.n_cols = n_cols; in.on_dev = flags & ILLICO_FLAG_INPUT_DEVICE;
    return in;
}

// what every entry point checks first, in this order; a family's own checks follow
inline int check_matrix_input(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub) {
    if (!c->has_groups) return fail(c, ILLICO_ERR_NO_GROUPS, "illico_set_groups has not been called");
    if (in.n_rows != c->n_cells)
        return fail(c, ILLICO_ERR_NO_GROUPS, "X has %lld rows but the groups describe %lld cells", (long long)in.n_rows, (long long)c->n_cells);
    if (col_lb < 0 || col_ub > in.n_cols || col_lb > col_ub)
        return fail(c, ILLICO_ERR_BOUNDS, "Invalid chunk bounds: (%lld, %lld) for data with %lld columns.", (long long)col_lb, (long long)col_ub, (long long)in.n_cols);
    if (in.dtype < 0 || in.dtype > 3) return fail(c, ILLICO_ERR_DTYPE, "unsupported dtype code %d", in.dtype);
    if (in.sparse && in.idx_dtype != ILLICO_IDX_I32 && in.idx_dtype != ILLICO_IDX_I64)
        return fail(c, ILLICO_ERR_DTYPE, "unsupported index dtype code %d", in.idx_dtype);
    return ILLICO_OK;
}

// the matrix's arrays; each family makes these checks at its own point among its own
inline int check_matrix_arrays(illico_ctx *c, const MatrixInput &in) {
    if (in.sparse) return in.data && in.indices && in.indptr ? ILLICO_OK : fail(c, ILLICO_ERR_ARG, "null sparse array");
    if (!in.X) return fail(c, ILLICO_ERR_ARG, "null X");
    if (in.ld < in.n_cols) return fail(c, ILLICO_ERR_ARG, "ld smaller than n_cols");
    return ILLICO_OK;
}

// the flags a bound matrix passes on: its arrays are on the device whatever the caller says
inline int bound_matrix_flags(int flags) { return (flags & (ILLICO_FLAG_LOG1P | ILLICO_FLAG_OUTPUT_DEVICE)) | ILLICO_FLAG_INPUT_DEVICE; }

inline int64_t idx_at(const void *p, int idx_dtype, int64_t i) { return idx_dtype == ILLICO_IDX_I32 ? (int64_t)((const int32_t *)p)[i] : ((const int64_t *)p)[i]; }

// the sparse arrays as the kernels see them: entry k at data[k - kshift]; column (CSC) or row (CSR) q at indptr[q - ptr_col0]
struct SparseOnDevice {
    const void *data, *indices, *indptr;
    long long kshift, ptr_col0;
};
// host-resident sparse input goes up once, into the scratch buffer `scratch_name`: CSC the entries of [col_lb, col_ub), CSR every row;
// device-resident input is passed through.  The copies are enqueued, not awaited: the arrays come from pageable host memory, and the
// caller synchronises the stream before it returns.
inline int stage_sparse_input(illico_ctx *c, const MatrixInput &in, int64_t col_lb, int64_t col_ub, const char *scratch_name, SparseOnDevice *out) {
    *out = SparseOnDevice{in.data, in.indices, in.indptr, 0, 0};
    if (in.on_dev) return ILLICO_OK;
    const size_t esz = dtype_size(in.dtype), isz = in.idx_dtype == ILLICO_IDX_I32 ? 4 : 8;
    const int64_t a = in.is_csr ? 0 : col_lb, b = in.is_csr ? in.n_rows : col_ub;
    const int64_t k0 = idx_at(in.indptr, in.idx_dtype, a), k1 = idx_at(in.indptr, in.idx_dtype, b);
    if (k0 < 0 || k1 < k0) return fail(c, ILLICO_ERR_ARG, "indptr is not non-decreasing");
    const size_t nnz = (size_t)(k1 - k0), nptr = (size_t)(b - a + 1);
    unsigned char *u;
    int rc = scratch(c, scratch_name, std::max<size_t>(nnz, 1) * (esz + isz) + nptr * isz + 64, &u);
    if (rc) return rc;
    void *dd = u, *di = u + ((nnz * esz + 15) & ~(size_t)15), *dp = (unsigned char *)di + ((nnz * isz + 15) & ~(size_t)15);
    HIPCHK(c, hipMemcpyAsync(dd, (const unsigned char *)in.data + (size_t)k0 * esz, nnz * esz, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(di, (const unsigned char *)in.indices + (size_t)k0 * isz, nnz * isz, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dp, (const unsigned char *)in.indptr + (size_t)a * isz, nptr * isz, hipMemcpyHostToDevice, c->stream));
    c->h2d_input_bytes += (int64_t)(nnz * (esz + isz) + nptr * isz);
    *out = SparseOnDevice{dd, di, dp, k0, a};
    return ILLICO_OK;
}

// columns [col0, col0 + wn) of a dense matrix as the kernels read them: a device matrix as it is (column col0 of X); a host matrix
// copied into `xwin`, [n_rows][wn] at `pitch` elements a row (column 0 of xwin), the bytes counted.  Enqueued, not awaited.
struct DenseWindow {
    const void *X;
    int64_t ld, col0;
};
inline int stage_dense_window(illico_ctx *c, const MatrixInput &in, int64_t col0, int64_t wn, int64_t pitch, void *xwin, DenseWindow *out) {
    *out = DenseWindow{in.X, in.ld, col0};
    if (in.on_dev) return ILLICO_OK;
    const size_t esz = dtype_size(in.dtype);
    HIPCHK(c, hipMemcpy2DAsync(xwin, (size_t)pitch * esz, (const unsigned char *)in.X + (size_t)col0 * esz, (size_t)in.ld * esz, (size_t)wn * esz,
                               (size_t)in.n_rows, hipMemcpyHostToDevice, c->stream));
    c->h2d_input_bytes += (int64_t)((size_t)in.n_rows * wn * esz);
    *out = DenseWindow{xwin, pitch, 0};
    return ILLICO_OK;
}

// f(Tag<value type>{}, Tag<index type>{}) for checked dtype codes: as dispatch_value_type (engine.h), every build instantiates f for
// all four value types and both index types
template <typename F> int dispatch_value_index_type(int dt, int idx_dtype, F &&f) {
    return dispatch_value_type(dt, [&](auto v) {
        if (idx_dtype == ILLICO_IDX_I32) return f(v, Tag<int32_t>{});
        return f(v, Tag<int64_t>{});
    });
}

// the groups' positions in chunks of at most chunk_len (a group of 100 000 cells is spread over ~100 workgroups of 1024)
template <typename Chunk> void group_chunks(const illico_ctx *c, int chunk_len, std::vector<Chunk> &out) {
    out.clear();
    int pos = 0;
    for (int64_t g = 0; g < c->n_groups; ++g) {
        const int n = c->h_counts[g];
        for (int p = 0; p < n; p += chunk_len) out.push_back({(int)g, pos + p, pos + std::min(n, p + chunk_len), n <= chunk_len ? 1 : 0});
        pos += n;
    }
}

} // namespace
