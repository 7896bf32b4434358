/* libillico_hip: Welch's t-test of every ordered pair of groups from the per-group moment planes of illico_group_moments_*.  A header of
 * its own beside illico_hip.h (whose types, flags, error codes and ILLICO_TT_* variants it uses): the entry point below is exported by
 * the same library.  Python: illico_amd._lib.PAIR_TTEST_SIGNATURES, Engine.pair_ttest_from_moments, illico_amd.pairwise_ttest,
 * illico_amd.pairwise_markers(method="t-test").  Design: DESIGN.md section 28. */
#ifndef ILLICO_HIP_PAIR_TTEST_H
#define ILLICO_HIP_PAIR_TTEST_H
#include "illico_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * sum, sumsq: float64 [G][in_ld >= n_cols], the per-group sums of the values and of their squares as illico_group_moments_* write them,
 * G the groups of illico_set_groups (only their sizes are used: the reference / one-versus-rest mode of the context plays no part).
 * fsum: the sums the fold change is formed from (under log1p the expm1 sums of illico_group_stats_* with ILLICO_FLAG_LOG1P), the layout
 * of sum; null: sum itself.  sel: the K >= 2 group ids to compare, strictly ascending, on the host.
 *
 * Outputs: up to five float64 planes [K][K][out_ld >= n_cols] indexed [r][g][j] -- group sel[g] against reference sel[r] in column j,
 * the layout illico_combine_pairs reads -- each written only if its pointer is not null, at least one of them:
 *   out_p, out_t, out_df   the bits illico_ttest_from_moments writes for group sel[g], column j, under a reference group sel[r]
 *                          (illico_hip.h states the formula: every step one IEEE float64 operation; `variant`, `alternative` as there);
 *                          the diagonal is its reference row: (t, p) = (0, 1), df what the formula gives for a group against itself
 *   out_fc                 (F1 / n1) / (F2 / n2), inf where F2 / n2 == 0   (F = fsum, or sum)
 *   out_d                  Cohen's d with the two variances averaged: (m1 - m2) / sqrt(0.5 * (v1 + v2)), each step one float64
 *                          operation; NaN -> 0, +-inf kept, 0 on the diagonal
 * ILLICO_TT_WELCH evaluates Student's t tail once per unordered pair and writes both cells from it (the mirrored cell is the bits of
 * a direct evaluation); ILLICO_TT_OVERESTIM_VAR is not symmetric and evaluates every ordered pair.
 *
 * Host arrays, complete on return -- staged in column windows sized to "scratch_bytes" -- or with ILLICO_FLAG_INPUT_DEVICE (sum, sumsq,
 * fsum) / ILLICO_FLAG_OUTPUT_DEVICE (the planes) device arrays, ordered on the context's stream.
 * ILLICO_ERR_NO_GROUPS without groups.  ILLICO_ERR_ARG: K < 2, sel null, not strictly ascending or out of range, null sum / sumsq, no
 * output plane, in_ld or out_ld below n_cols, n_cols < 0, an unknown variant; ILLICO_ERR_ALTERNATIVE.  ILLICO_ERR_UNSUPPORTED: more
 * than 2880 selected groups (the tile pairs of one launch).
 */
int illico_pair_ttest_from_moments(illico_ctx *ctx, const double *sum, const double *sumsq, const double *fsum, int64_t n_cols,
                                   int64_t in_ld, const int32_t *sel, int64_t K, int variant, int alternative, int flags,
                                   double *out_p, double *out_t, double *out_df, double *out_fc, double *out_d, int64_t out_ld);

#ifdef __cplusplus
}
#endif
#endif /* ILLICO_HIP_PAIR_TTEST_H */
