/* libillico_hip: per-group marker statistics -- the K - 1 tests of a group against every other group combined into one p-value per
 * (group, gene), on the device.  A header of its own beside illico_hip.h (whose types, flags and error codes it uses): the entry point
 * below is exported by the same library.  Python: illico_amd._lib.MARKER_SIGNATURES, Engine.combine_pairs,
 * illico_amd.pairwise_markers.  Design: DESIGN.md section 26. */
#ifndef ILLICO_HIP_MARKERS_H
#define ILLICO_HIP_MARKERS_H
#include "illico_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ILLICO_COMBINE_ALL 0   /* intersection-union: the largest p */
#define ILLICO_COMBINE_ANY 1   /* Simes */
#define ILLICO_COMBINE_SOME 2  /* Holm's adjusted p of rank rank_j ("middle") */
#define ILLICO_COMBINE_MAX_GROUPS 256
#define ILLICO_COMBINE_MAX_EFFECTS 4

/*
 * p: float64 [K][K][in_ld >= W] indexed [r][g][j], the p-value of group g against reference r for column j, as the pair routes write
 * them (illico_pairwise_from_hists, illico_pairwise_ranked_*).  For a group g and a column j take the n = K - 1 values
 * p_r = p[r][g][j], r != g (the diagonal entry is never read, whatever it holds), and their stable rank
 *     rank(r) = 1 + #{r' != g : p_r' < p_r, or p_r' == p_r and r' < r};        p_(i): the p of the reference of rank i.
 * In IEEE float64, in the order written, the integers converted to double first:
 *     ILLICO_COMBINE_ALL    out_p = p_(n)                                                        representative rank i* = n
 *     ILLICO_COMBINE_ANY    out_p = min_i ( p_(i) * (double)n / (double)i )                      i* = 1
 *     ILLICO_COMBINE_SOME   out_p = min(1.0, max_{i <= rank_j} ( p_(i) * ((double)n - (double)i + 1.0) ))    i* = rank_j, in [1, n]
 * out_rep[g][j] (int32): the reference whose stable rank is i*, an index into the K groups.  For each effect plane e0 .. e3 that is
 * not null (float64, the layout and pitch of p: U, fold change, z ...) the matching output o0 .. o3 receives e[rep][g][j]: a selection,
 * no arithmetic; an effect plane is read at the representative only.  (rank_j is ignored by the other two methods.)
 * skip: uint32 [W] or null, on the side of p; a non-zero entry means the column is neither validated nor written in any output
 * (the `flags` of illico_group_value_hists_*, the `out_left` of illico_pairwise_ranked_*: their untouched columns hold anything).
 * Outputs: [K][out_ld >= W], out_ld independent of in_ld (out_rep has the same pitch, in its own elements).
 * Host arrays, complete on return -- staged in gene batches sized to "scratch_bytes" -- or with ILLICO_FLAG_INPUT_DEVICE /
 * ILLICO_FLAG_OUTPUT_DEVICE device arrays, ordered on the context's stream.
 * ILLICO_ERR_ARG naming (reference, group, column) and the value: an off-diagonal p of a column that is not skipped which is NaN or
 * outside [0, 1].  Device input is validated whole before anything is written; host input batch by batch as it arrives (a plane set
 * larger than one batch may then have earlier batches written).
 * Refused before anything is written: K < 2, null p / out_p / out_rep, an effect plane without its output, a method or rank_j outside
 * its range, a pitch below W, W < 0 (ILLICO_ERR_ARG); K > 256 (ILLICO_ERR_UNSUPPORTED).
 */
int illico_combine_pairs(illico_ctx *ctx, const double *p, const double *e0, const double *e1, const double *e2, const double *e3,
                         int64_t K, int64_t W, int64_t in_ld, const uint32_t *skip, int method, int64_t rank_j, int flags,
                         double *out_p, int32_t *out_rep, double *o0, double *o1, double *o2, double *o3, int64_t out_ld);

#ifdef __cplusplus
}
#endif
#endif /* ILLICO_HIP_MARKERS_H */
