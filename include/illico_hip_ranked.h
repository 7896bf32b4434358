/* libillico_hip: the ranked pair route -- the Wilcoxon rank-sum test of every ordered pair of groups for genes of any float32 / int32
 * values, from one sorted walk per gene.  A header of its own beside illico_hip.h (whose types, flags and error codes it uses): the
 * two entry points below are exported by the same library.  Python: illico_amd._lib.RANKED_SIGNATURES, Engine.pairwise_ranked,
 * Engine.pairwise_ranked_sparse.  Design: DESIGN.md section 20. */
#ifndef ILLICO_HIP_RANKED_H
#define ILLICO_HIP_RANKED_H
#include "illico_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Every ordered pair of the K = n_sel groups sel[0 .. K) (sel null: all groups of illico_set_groups, in order; their codes, counts and
 * group-contiguous order are used, the reference / one-versus-rest mode is ignored) for each column j of [col_lb, col_ub),
 * W = col_ub - col_lb, whatever its values: negative, fractional, beyond 255.  Over the distinct values v of a column in ascending order
 * (zero among them, -0.0 tied with 0.0; a stored zero of sparse input is a zero), t_k(v) the cells of group k that hold v and
 * c_k(v) = sum_{v' < v} t_k(v'):
 *     S2  = sum_v t_g(v) (2 c_r(v) + t_r(v))                 U = 0.5 (double)(2 n_r n_g - S2)
 *     tie = (double) sum_v (t^3 - t), t = t_g(v) + t_r(v)    (0.0 without ILLICO_FLAG_TIE_CORRECT)
 * exact integers; p, z and the fold change follow as in illico_pairwise_from_hists, so plane slab r is the [K, W] plane set of a
 * one-versus-reference call with reference sel[r].  sums: REQUIRED float64 [n_groups][sums_ld >= W], the per-group value sums of the
 * fold change (illico_group_stats_*; under log1p its expm1 sums), column j - col_lb for column j.
 * Input: float32 / int32 values; dense row-major, or CSC with i32 / i64 indices whose row indices ascend strictly within a column
 * (ILLICO_ERR_UNSORTED otherwise); host arrays or, with ILLICO_FLAG_INPUT_DEVICE, device arrays (sums goes with the matrix).
 * Outputs: float64 [K][K][out_ld >= W] indexed [r][g][j - col_lb]; out_z may be null; out_left uint32 [W]: 0, or why the column left
 * the route (1: its non-zeros could not be split into value-range parts, 2: more different values than the record slots hold crowd into
 * one coarse value bucket, 3: it holds a NaN) -- the columns of such genes are left untouched in every plane, and a caller completes them
 * with one-versus-reference calls.  Host arrays, complete on return, or with ILLICO_FLAG_OUTPUT_DEVICE device arrays (planes and
 * out_left), ordered on the context's stream.  Diagonal: p = 1, U = n^2 / 2, z = 0.  Other flags: ILLICO_FLAG_CONTINUITY,
 * ILLICO_FLAG_TIE_CORRECT (ILLICO_FLAG_LOG1P is accepted and has no effect).  The window is taken in gene batches sized to
 * "scratch_bytes" (about 10 bytes x n_rows per gene, and the batch's dense window for host or CSC input); ILLICO_ERR_OOM only when a
 * batch of 64 genes does not fit.  Option "pair_rank_cap" (tests): records per value-range part at most, at least 1024.
 * Refused before anything is written: a value type other than float32 / int32, K > 64, more than 65535 groups, 2^31 cells or more, two
 * selected groups with n_g + n_r >= 2^21 (ILLICO_ERR_UNSUPPORTED); K < 2, ids of sel outside the groups or repeated, null sums / planes /
 * out_left, a pitch below the window (ILLICO_ERR_ARG); ILLICO_ERR_ALTERNATIVE, ILLICO_ERR_NO_GROUPS, ILLICO_ERR_BOUNDS, ILLICO_ERR_DTYPE. */
int illico_pairwise_ranked_dense(illico_ctx *ctx, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                                 int64_t col_lb, int64_t col_ub, const int64_t *sel, int64_t n_sel, const double *sums, int64_t sums_ld,
                                 int flags, int alternative, double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld,
                                 uint32_t *out_left);
int illico_pairwise_ranked_csc(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                               int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, const int64_t *sel, int64_t n_sel,
                               const double *sums, int64_t sums_ld, int flags, int alternative, double *out_p, double *out_u,
                               double *out_fc, double *out_z, int64_t out_ld, uint32_t *out_left);

#ifdef __cplusplus
}
#endif
#endif /* ILLICO_HIP_RANKED_H */
