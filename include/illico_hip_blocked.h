/* libillico_hip: blocked Wilcoxon rank-sum tests -- a test spread over B blocks (batches, donors, plates), each group compared with
 * the reference cells of the same block and the per-block tests combined on the device (scran's `block=` of pairwiseWilcox, with
 * Stouffer's weighted z).  A header of its own beside illico_hip.h (whose types, flags and error codes it uses): the entry points
 * below are exported by the same library.  Python: illico_amd._lib.BLOCKED_SIGNATURES, Engine.blocked_from_hists,
 * Engine.blocked_from_planes, illico_amd.blocked_wilcoxon.  Design: DESIGN.md section 27. */
#ifndef ILLICO_HIP_BLOCKED_H
#define ILLICO_HIP_BLOCKED_H
#include "illico_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Definition.  G groups g, B blocks b in ascending order, compound sizes counts[g * B + b] (int64, host memory, always).  The
 * reference of a test is the group `ref`, or with ref = -1 the rest of the block.  For a test (g, column j) block b is USED when it
 * holds n_g > 0 cells of g and n_r > 0 reference cells (those of ref in b, or those of b that are not g).  In a used block, with
 * gc = group_const(n_r, n_g, n_r + n_g) (kernels_finalize.h):
 *     U_b    the reference's U of the block's two samples, as every route reports it
 *     tie_b  their tie sum, 0.0 without ILLICO_FLAG_TIE_CORRECT
 *     z_b  = zscore_device_pre(gc.nnn, gc.var0, tie_b, U_b, gc.mu): never continuity-corrected, 0.0 for a constant block
 *     w_b  = (double)(n_g n_r)
 * and over the used blocks in ascending b, in IEEE float64, in the order written:
 *     z         = (sum_b w_b z_b) / sqrt(sum_b w_b w_b)        -- over one used block: z_b itself (the same number, not rounded twice)
 *     p         = erfc(|z| / sqrt 2) two-sided, 0.5 erfc(-z / sqrt 2) greater, 0.5 erfc(z / sqrt 2) less
 *     statistic = sum_b U_b
 *     fold      = (sum_b S_gb / sum_b n_gb) / (sum_b S_rb / sum_b n_rb), +inf where the reference's pooled mean is 0
 * with S the value sums.  A test without a used block has NaN in all four planes.  The row of the group `ref` itself is p = 1,
 * statistic = -1, z = 0.  There is no continuity correction: the z planes carry none.
 * Outputs: float64 [G][out_ld >= n_cols] planes out_p, out_u (statistic), out_fc, out_z; columns beyond n_cols are not touched.
 * Arrays are host arrays, complete on return, or with ILLICO_FLAG_INPUT_DEVICE / ILLICO_FLAG_OUTPUT_DEVICE device arrays, ordered on
 * the context's stream (counts and row_map are host arrays in either case).
 * Refused before anything is written: B < 1, G < 1 (G < 2 with a reference), ref outside [-1, G), a negative size, a null array,
 * a pitch below n_cols, n_cols < 0 (ILLICO_ERR_ARG); an alternative code that is none (ILLICO_ERR_ALTERNATIVE); a used block whose
 * two samples hold 2097152 cells or more, more than 65535 compound groups (ILLICO_ERR_UNSUPPORTED); a working set beyond the option
 * "scratch_bytes" (ILLICO_ERR_OOM: pass a narrower gene window).
 *
 * illico_blocked_from_hists: the per-block statistics from value histograms.  H: uint32 [G * B][n_cols][256] and gene_flags: uint32
 * [n_cols], as illico_group_value_hists_* write them for the compound group coding k = g * B + b; the columns of flagged genes are
 * left untouched in every plane.  sums: optional float64 [G * B][sums_ld >= n_cols] compound value sums for the fold change (under
 * log1p the expm1 sums of illico_group_stats_*); null: the sums of the histograms.
 */
int illico_blocked_from_hists(illico_ctx *ctx, const uint32_t *H, const uint32_t *gene_flags, const int64_t *counts, int64_t n_groups,
                              int64_t n_blocks, int64_t n_cols, int64_t ref, const double *sums, int64_t sums_ld, int flags, int alternative,
                              double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld);

/*
 * illico_blocked_from_planes: z_b and U_b read from planes.  z, U: float64 [B][G][in_ld >= n_cols], the z and U planes of B
 * one-versus-reference (or one-versus-rest) calls without continuity correction, each on the rows of one block.  row_map: int32
 * [B][G] (host memory), the row of group g in block b's plane set, or -1 where g has no cells in b (the block is then not used for
 * g); an entry below -1 or beyond G - 1 is refused (ILLICO_ERR_ARG).  sums as above, but without it there is no fold change: out_fc
 * must then be null (and may be null with it).
 */
int illico_blocked_from_planes(illico_ctx *ctx, const double *z, const double *U, int64_t in_ld, const int32_t *row_map, const int64_t *counts,
                               int64_t n_groups, int64_t n_blocks, int64_t n_cols, int64_t ref, const double *sums, int64_t sums_ld, int flags,
                               int alternative, double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld);

#ifdef __cplusplus
}
#endif
#endif /* ILLICO_HIP_BLOCKED_H */
