/*
 * illico_hip.h -- C-ABI of libillico_hip.so, the MI355X (gfx950) engine for illico's asymptotic
 * Wilcoxon rank-sum hot path.
 *
 * The reference (remydubois/illico v0.2.0) has no FFI: its seam is the Python operator
 *   dispatcher(X, chunk_lb, chunk_ub, grpc, is_log1p, use_continuity, tie_correct, alternative)
 *       -> (pvalues, statistics, fold_change)          each float64 [n_groups, chunk_ub-chunk_lb]
 * (illico/asymptotic_wilcoxon.py:59-67; Numba signature illico/utils/compile.py:35-47), one
 * implementation per (Test, KernelDataFormat) key (illico/utils/registry.py:15-43).  The entry
 * points below are what a binding for that seam binds: plain pointers and sizes, `int` status
 * returns (0 = ok, negative = error mapped by the host onto the reference's exception types),
 * nothing thrown across the boundary.  INTEGRATION.md shows the ctypes stub.
 *
 * Ownership: the caller owns X, the group arrays and the three output planes; the library owns
 * only device scratch inside the context and never writes to X (the reference's tests assert the
 * input is not mutated, tests/test_asymptotic_wilcoxon.py:187-194).
 * Threading: one context = one HIP stream.  Every entry point that takes a context locks it for the
 * duration of the call, so host threads sharing ONE context (the reference's joblib threads share one
 * dispatcher, illico/asymptotic_wilcoxon.py:236-241) are serialised, never raced; illico_last_error
 * returns the calling thread's own last message.  Threads that want overlap use one context each.
 * illico_ctx_destroy must not race with other calls on the same context.
 */
#ifndef ILLICO_HIP_H
#define ILLICO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct illico_ctx illico_ctx;

/* status codes; the Python host maps them onto the reference's exceptions */
enum {
    ILLICO_OK = 0,
    ILLICO_ERR_ARG = -1,          /* null pointer / nonsensical size                          -> ValueError */
    ILLICO_ERR_BOUNDS = -2,       /* bad chunk bounds (asymptotic_wilcoxon.py:49-50, csc.py:158-159, csr.py:161-162) -> ValueError */
    ILLICO_ERR_ALTERNATIVE = -3,  /* unknown alternative (utils/math.py:116)                  -> ValueError */
    ILLICO_ERR_DTYPE = -4,        /* unsupported element / index dtype (registry.py:54-58)    -> KeyError   */
    ILLICO_ERR_NO_GROUPS = -5,    /* illico_set_groups not called / inconsistent with n_rows  -> ValueError */
    ILLICO_ERR_UNSORTED = -6,     /* CSR indices not sorted (asymptotic_wilcoxon.py:186-193)  -> ValueError */
    ILLICO_ERR_HIP = -10,         /* a HIP runtime call failed (see illico_last_error)        -> RuntimeError */
    ILLICO_ERR_OOM = -11,         /* device allocation failed                                 -> MemoryError */
    ILLICO_ERR_UNSUPPORTED = -12  /* shape outside what this build handles (see last_error)   -> NotImplementedError */
};

/* element dtypes of X / data */
enum { ILLICO_F32 = 0, ILLICO_F64 = 1, ILLICO_I32 = 2, ILLICO_I64 = 3 };
/* index dtypes of sparse indices/indptr (scipy uses one dtype for both) */
enum { ILLICO_IDX_I32 = 0, ILLICO_IDX_I64 = 1 };
/* alternative hypothesis (utils/math.py:99-116) */
enum { ILLICO_ALT_TWO_SIDED = 0, ILLICO_ALT_LESS = 1, ILLICO_ALT_GREATER = 2 };
/* flags */
enum {
    ILLICO_FLAG_LOG1P = 1,          /* is_log1p        (utils/math.py:212)        */
    ILLICO_FLAG_CONTINUITY = 2,     /* use_continuity  (ovo/dense_ovo.py:58)      */
    ILLICO_FLAG_TIE_CORRECT = 4,    /* tie_correct     (ovo/dense_ovo.py:54)      */
    ILLICO_FLAG_INPUT_DEVICE = 8,   /* X / data / indices / indptr are device pointers on ctx's device */
    ILLICO_FLAG_OUTPUT_DEVICE = 16, /* out_p / out_u / out_fc are device pointers                       */
    /* illico_run_dense with device-resident input AND device planes: enqueue the fused single-pass route and return without
     * waiting for it.  The few genes that route cannot take (values outside its table) are recomputed when their flags have
     * arrived -- by the next call on the context or by illico_ctx_synchronize, after which the planes are complete.  X and
     * the planes must stay valid until then.  A following deferred call that writes OTHER planes is enqueued before the
     * earlier one is completed, so back-to-back passes run without a host round trip in between.
     * illico_run_csc / illico_run_bound on device-resident CSC arrays with device planes honour it too: the count-valued pass
     * (whether the window holds counts at all is decided on the device, from a sample of its stored values) is enqueued and the
     * columns it cannot take are recomputed the same way, later.  Ignored elsewhere (host arrays, host planes, CSR). */
    ILLICO_FLAG_DEFER = 32
};

/* ---- context ---------------------------------------------------------------------------- */
int illico_ctx_create(int device_id, illico_ctx **out_ctx);
int illico_ctx_destroy(illico_ctx *ctx);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the context's own. */
int illico_ctx_set_stream(illico_ctx *ctx, void *hip_stream);
/* Tunables: "gene_batch" (genes per device pass, 0 = auto), "scratch_bytes" (cap of device scratch; default: 64 GiB or a
 * quarter of the device's memory, whichever is less),
 * "profile" (1 = bracket kernel launches with HIP events on the context's stream), "profile_only" (kernel id: time
 * that kernel only, -1 = all), "fused_groups_per_wg" / "ovr_hist_groups_per_wg" (launch geometry, 0 = auto).
 * Route switches, all 0 by default; every route produces the same integers, the switches exist so that tests and
 * A/B measurements can force each one: "no_fused_path", "no_counts_path" (dense / segmented histogram routes),
 * "no_ovr_one_pass" (dense OVR in two passes over X; "ovr_full_dump" = 1: its one pass writes every word of every group histogram
 * instead of the leading non-zero ones), "no_csc_counts_path" (count-valued CSC on LDS histograms;
 * "no_csc_counts_mixed" = 1: its 8-bit cell form only; "no_csc_counts_wide" = 1: never its 16-bit-cell form, i.e. the route is off when
 * more than 8 ranked groups exceed 255 cells; "no_csc_counts_windows" = 1: never in windows of groups, i.e. off when the groups' tables
 * do not fit LDS at once; "csc_counts_max_windows" > 0: nor in more windows of groups than this),
 * "no_packed_dense" (dense two-pass routes: group-wise packing of the non-zero keys + look-ups in a counted bitmap of the reference
 * for OVO, the transposition with the group sums folded in for OVR; 1 = the plain transposition and the kernels behind it;
 * "no_ovr_packed_partition" = 1: dense OVR splits the padded key rows -- every key -- instead of the packed ones;
 * "packed_eq_buckets": the packed OVO kernel's value buckets follow the reference's distribution, 1 = always, 0 = never,
 * -1 = for references of more than 16384 cells, the default; "no_ovo_parts" = 1: a reference whose non-zero keys outgrow the kernel's
 * LDS slots is never taken in value-range parts -- such genes go to the general sort routes; "no_big_runs_global" = 1: a ranked
 * group's run of more keys than LDS holds is not dealt into value buckets through HBM -- its gene goes to the general sort routes;
 * "no_packed_small_wg" = 1: the packed OVO kernel never takes its 256-thread form for small references with few groups;
 * "no_coop_runs" = 1: it walks a long run with one wavefront instead of all of the workgroup's; "no_deal_runs" = 1: in value-range
 * parts it never deals the short runs by part first -- every part then looks every key up, masked; "packed_ref_cap" / "big_runs_cap"
 * > 0: cap the kernel's LDS key slots for the reference / k_bucket_big_runs' LDS key slots, so that tests reach the value-range
 * parts / the route through HBM at small sizes; "no_sparse_packed_small" = 1: sparse OVO genes with eight-byte keys beyond
 * k_csc_gene's LDS go to k_ovo_rank or the dense windows instead of the packed kernel; "debug_routes" = 1: stderr says what the
 * packed OVO kernel left to the general routes, and why),
 * "no_compact_narrow" (k_group_compact never takes its 32-gene tiles for few, long blocks; "compact_narrow_rows": rows of the longest
 * block from which it does, default 8192; "compact_narrow_wgs": and only while the launch would have fewer 64-gene workgroups than
 * this, default 2048; a value of 0 or less restores either default), "no_compact_order" (k_group_compact numbers its workgroups in
 * grid order whatever the blocks' lengths instead of starting the longest block first), "no_big_runs_wide" (runs above 8192 keys get no 1024-thread launch of their own),
 * "big_runs_slice_bytes" (> 0: LDS bytes of k_bucket_big_runs_global's slice buffer), "no_ovr_packed_big" (dense OVR with a group above
 * 65535 cells partitions the padded rows, as before), "no_ovr_part_coop" (the packed partition walks every block with one wavefront),
 * "ovr_rank_whole" (dense OVR rank kernel: one 1024-thread workgroup per CU with all of its LDS instead of two of 512 threads),
 * "no_group_hist_route" (count-valued dense input with few large groups, or OVR / OVO with a group above 65535 cells: the fused kernels
 * instead of the (group, gene) value histograms of kernels_group_hists.h; "group_hist_min_cells": cells from which the route is
 * taken, default 32768; "group_hist_max_wgs": and only while the fused launch would have fewer workgroups than this, default 1024;
 * a value of 0 or less restores either default), "no_csr_transpose_split" (CSR -> CSC on the device: one workgroup per row block whatever their number),
 * "no_csc_ovr_small_lds" (k_csc_ovr_gene takes a CU's whole LDS per workgroup whatever the columns' lengths),
 * "no_ovo_ref_buckets" (OVO sort route: reference column in value buckets instead of sorted), "no_ovr_parts_path" (dense OVR, any values: value-range parts ranked in LDS; "ovr_parts_cap" > 0 caps the keys per part), "no_csc_gene_path" (CSC OVO single-kernel route), "no_csc_ovr_gene_path" (CSC OVR single-kernel route; "csc_ovr_sorted_form" = 1 makes it sort every
 * gene in LDS, the form tie-heavy columns take, instead of bucketing the keys), "no_csc_regroup_lds" (two-kernel CSC route: regroup with scattered
 * stores only),
 * "no_fused_wide" (the 256-value second stage of the fused routes), "no_wide_gather" (that stage always over the window as it lies, never
 * on the gathered columns), "no_leftover_gather" (the genes the fused passes leave are recomputed as column runs of the input instead
 * of being gathered into a narrow matrix),
 * "no_dense_window_path" (CSR through dense windows; "dense_window_f32" = 1: float32 cells instead of bytes), "no_csr_transpose_path" / "no_csr_tile_gather"
 * (CSR -> CSC transposition on the device / its gather form for sorted rows), "no_csr_counts_path" (count-valued CSR by the byte windows
 * instead of the group-major pass), "no_csr_densify_any" (sparse windows with columns of more than 32 768 stored entries stay with the
 * sparse routes instead of being written out dense), "no_f64_narrowing" (float64 sparse values that are all float32 values stay with the
 * float64 kernels).
 * Not route switches: "host_narrow" (-1 automatic / 1 / 0: host-resident count matrices go up as bytes), "bound_ahead_genes" (0 = off:
 * a call for fewer genes of a bound CSR matrix computes the aligned window of that many genes around them once and later calls inside
 * the window are slices of it -- for bindings that keep the reference's 256-gene chunk loop),
 * "fused_mem_policy" (cache policy of the fused dense OVO pass, same bits whatever the value: 0 = the engine's choice -- non-temporal loads for 4- and 8-byte values, default loads for byte windows, 8-byte stores; loads of X 1 = default policy, 2 = non-temporal; plus result stores 4 = 8 bytes per lane, 8 = 16 bytes per lane, 12 = 16 bytes write-through),
 * "host_fill_threads" (> 0: host threads that fill the pinned slots of the host-window pipelines; default 12 for float32 and 16 for
 * byte windows), "no_host_numa" (1 = those threads are not confined to the NUMA node the caller's matrix lives on),
 * "no_sparse_byte_values" (1 = the stored values of host-resident sparse input always go up in their own type; count values go up as
 * bytes otherwise), "prewarm_host_window_bytes" (an action, not a setting: a value > 0 pins the three host slots and allocates the
 * three device windows of the host-window pipelines at that many bytes each now, instead of in the context's first call on a
 * host-resident dense matrix; 0 does nothing), "pair_rank_cap" (> 0: records per part at most in the ranked pair route, never below
 * 1024 -- tests force many small parts with it), "csr_counts_abl" (a timing experiment: bits that leave out stages of k_csr_counts,
 * whose results are then wrong; 0 = the whole kernel), "no_ovr_library_sort" (accepted and ignored: there is no library sort any more).
 * Unknown keys return ILLICO_ERR_ARG. */
int illico_ctx_set_option(illico_ctx *ctx, const char *key, int64_t value);
const char *illico_last_error(const illico_ctx *ctx);
int illico_ctx_synchronize(illico_ctx *ctx);

/* ---- groups: GroupContainer of illico/utils/groups.py:6-15, all int64 host arrays ------- */
/* encoded_groups[n_cells], counts[n_groups], indices[n_cells] (cells ordered by group),
 * indptr[n_groups+1]; encoded_ref_group == -1 selects OVR (asymptotic_wilcoxon.py:41-44). */
int illico_set_groups(illico_ctx *ctx, const int64_t *encoded_groups, const int64_t *counts,
                      const int64_t *indices, const int64_t *indptr, int64_t n_cells, int64_t n_groups,
                      int64_t encoded_ref_group);

/* ---- the six (Test x KernelDataFormat) dispatchers of registry.py:26-43 -------------------
 * Each computes columns [col_lb, col_ub) and writes three row-major float64 planes
 * out_*[g * out_ld + (j - col_lb)], g < n_groups.  The reference-group row of an OVO call is
 * written as (p = 1.0, U = -1.0) in every format (sparse_ovo.py:140-143).
 */
/* replaces dense_ovo_mwu_kernel_over_contiguous_col_chunk (ovo/dense_ovo.py:65-137) and
 * dense_ovr_mwu_kernel_over_contiguous_col_chunk (ovr/dense_ovr.py:15-80); X is row-major
 * [n_rows, >=n_cols] with leading dimension ld elements (registry.py:105-108). */
int illico_run_dense(illico_ctx *ctx, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                     int64_t col_lb, int64_t col_ub, int flags, int alternative, double *out_p, double *out_u,
                     double *out_fc, int64_t out_ld);
/* replaces csc_ovo_mwu_kernel_over_contiguous_col_chunk (ovo/sparse_ovo.py:163-210) and
 * csc_ovr_mwu_kernel_over_contiguous_col_chunk (ovr/sparse_ovr.py:100-155); CSCMatrix(data, indices,
 * indptr, shape) of utils/sparse/csc.py:10. */
int illico_run_csc(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr,
                   int idx_dtype, int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags,
                   int alternative, double *out_p, double *out_u, double *out_fc, int64_t out_ld);
/* replaces csr_ovo_mwu_kernel_over_contiguous_col_chunk (ovo/sparse_ovo.py:214-260) and
 * csr_ovr_mwu_kernel_over_contiguous_col_chunk (ovr/sparse_ovr.py:158-208); CSRMatrix of
 * utils/sparse/csr.py:16.  Indices must be sorted per row (checked by illico_csr_indices_sorted). */
int illico_run_csr(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr,
                   int idx_dtype, int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags,
                   int alternative, double *out_p, double *out_u, double *out_fc, int64_t out_ld);
/* The same three with a fourth plane: out_z receives the z-score of every test, (mu - U) / sigma with mu = n_ref n_tgt / 2 and sigma
 * formed exactly as the p-value forms it (tie-corrected under ILLICO_FLAG_TIE_CORRECT, never continuity-corrected, whatever the
 * alternative): positive when the group ranks above its reference -- scanpy's "scores".  0.0 on a constant column (where p is 1 through
 * the tie correction) and on the reference group's row of an OVO call.  out_z may be null (the calls above are these with null); it
 * shares out_ld and the residency flags with the other planes, and the p, U and fold-change planes are the same bytes either way. */
int illico_run_dense_ex(illico_ctx *ctx, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                        int64_t col_lb, int64_t col_ub, int flags, int alternative, double *out_p, double *out_u,
                        double *out_fc, double *out_z, int64_t out_ld);
int illico_run_csc_ex(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr,
                      int idx_dtype, int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags,
                      int alternative, double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld);
int illico_run_csr_ex(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr,
                      int idx_dtype, int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags,
                      int alternative, double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld);
/* ---- a sparse matrix bound once, computed chunk by chunk -------------------------------------
 * The reference's driver calls a dispatcher once per gene chunk with the SAME matrix (illico/asymptotic_wilcoxon.py:236-241:
 * 32 calls at 8000 genes and batch_size 256); CSR rows span every gene, so illico_run_csr on HOST arrays has to move the whole
 * matrix to the device in every call.  illico_csr_bind / illico_csc_bind upload the arrays ONCE (or, with
 * ILLICO_FLAG_INPUT_DEVICE, adopt device arrays without copying) and return a handle; illico_run_bound then computes any
 * column chunk of it like illico_run_csr / illico_run_csc on device-resident arrays (flags: LOG1P / CONTINUITY / TIE_CORRECT /
 * OUTPUT_DEVICE / DEFER).  The caller may free or modify its host arrays as soon as bind returns.  A handle belongs to the
 * context that made it; illico_matrix_release frees the device copy (illico_ctx_destroy releases what is left).  An explicit
 * handle, not a cache keyed on pointers: nothing about a matrix is remembered behind the caller's back. */
typedef struct illico_matrix illico_matrix;
int illico_csr_bind(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                    int64_t n_rows, int64_t n_cols, int flags, illico_matrix **out_matrix);
int illico_csc_bind(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                    int64_t n_rows, int64_t n_cols, int flags, illico_matrix **out_matrix);
int illico_run_bound(illico_ctx *ctx, const illico_matrix *matrix, int64_t col_lb, int64_t col_ub, int flags, int alternative,
                     double *out_p, double *out_u, double *out_fc, int64_t out_ld);
/* with the z-score plane (see the _ex calls above).  A call with out_z != null computes its chunk directly, whatever
 * "bound_ahead_genes" says: the windows computed ahead hold three planes; they are neither used nor replaced by it. */
int illico_run_bound_ex(illico_ctx *ctx, const illico_matrix *matrix, int64_t col_lb, int64_t col_ub, int flags, int alternative,
                        double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld);
int illico_matrix_release(illico_ctx *ctx, illico_matrix *matrix);
/* Adopted device arrays (ILLICO_FLAG_INPUT_DEVICE) stay the caller's: they must not change while a call on them is in flight, and what
 * the context remembers about a bound matrix -- whether its CSR rows are in order (looked at once, at bind time) and, with the option
 * "bound_ahead_genes", result windows computed ahead of the chunk calls -- describes the arrays as they were.  A caller that rewrites
 * adopted arrays in place (normalise, log1p_) calls illico_matrix_touch afterwards: windows of the matrix are dropped, the row order is
 * looked at again.  (Uploaded matrices are the library's own copy and never need it.) */
int illico_matrix_touch(illico_ctx *ctx, illico_matrix *matrix);

/* replaces check_indices_sorted_per_parcel (utils/ranking.py:245-273); *out_sorted = 1/0. */
int illico_csr_indices_sorted(illico_ctx *ctx, const void *indices, const void *indptr, int idx_dtype,
                              int64_t n_rows, int flags, int *out_sorted);

/* ---- the ranking primitives, before finalisation -----------------------------------------
 * Device counterpart of rank_sum_and_ties_from_sorted (utils/ranking.py:52-158; OVO) and
 * _accumulate_group_ranksums_from_argsort (utils/ranking.py:7-49; OVR) for the dense columns [col_lb, col_ub): the integer
 * statistics the dispatchers feed to compute_pval, as the reference's own primitive tests look at them
 * (tests/utils/test_ranking.py:13-56).  Host arrays [col_ub - col_lb][n_groups]:
 *   out_two_u[j][g]     2 * U1,  U1 = n_ref n_tgt + n_tgt (n_tgt + 1) / 2 - ranksum_g   (dense_ovo.py:48, dense_ovr.py:57-61;
 *                       n_ref = reference-group size, or every other cell for OVR) -- ranksum_g follows exactly;
 *   out_tie_sum[j][g]   sum over tie blocks of t^3 - t  (of reference + group g for OVO, of the whole column for OVR);
 *   out_value_sum[j][g] the group's value sum (expm1'd under ILLICO_FLAG_LOG1P).
 * The reference group's own entries are unspecified in OVO.  Runs the two-pass routes (the fused single-pass kernels
 * never materialise these numbers).  flags: ILLICO_FLAG_LOG1P, ILLICO_FLAG_INPUT_DEVICE. */
int illico_rank_statistics(illico_ctx *ctx, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                           int64_t col_lb, int64_t col_ub, int flags, int64_t *out_two_u, uint64_t *out_tie_sum,
                           double *out_value_sum);

/* ---- multi-GPU ----------------------------------------------------------------------------
 * Gene sharding is host-side: one context per GPU and process, each computing its own column range with the entry points
 * above (no input is exchanged); the one collective of the path -- the gather of the planes to rank 0 -- is issued by the
 * host over RCCL (illico_amd/distributed.py: torch.distributed.gather on device planes, backend "nccl").  The C-ABI has no
 * illico_gather entry: a binding that wants several GPUs brings its own process group, as the Python host does.
 *
 * What the C-ABI does offer the gathering rank: the way its planes reach host memory.  Three gathered device planes [n_groups][n_cols]
 * (dense, row pitch n_cols) are copied into the caller's host planes (row pitch out_ld >= n_cols) through the context's two pinned
 * buffers -- block i travels at the link's rate while block i - 1 is scattered by a few host threads -- i.e. the path the results of
 * an ordinary call with host planes take (asymptotic_wilcoxon.py:242-244 copies each chunk's planes into `results`).  Needs groups
 * (n_groups).  */
int illico_planes_to_host(illico_ctx *ctx, const double *dev_p, const double *dev_u, const double *dev_fc, int64_t n_cols,
                          double *out_p, double *out_u, double *out_fc, int64_t out_ld);

/* ---- multiple-testing correction of a p-value plane ---------------------------------------
 * p: float64 [n_rows][n_cols], row pitch in_ld >= n_cols: one row per group, one column per gene (the out_p plane of the calls
 * above).  Each row is adjusted on its own, m = n_cols:
 *   ILLICO_ADJ_BH          Benjamini-Hochberg: adj_(i) = min_{k >= i} p_(k) * (m / k), clipped to 1 -- bit for bit what scipy's
 *                          stats.false_discovery_control(p, axis=1, method="bh") returns;
 *   ILLICO_ADJ_BY          Benjamini-Yekutieli: the same with an extra factor c_m = sum_{i <= m} 1 / i, formed on the host in the
 *                          order numpy's pairwise sum takes (blocks of 8192, its default buffer): scipy's method="by" within a
 *                          relative 1e-14 -- bit for bit as long as numpy sums that way;
 *   ILLICO_ADJ_BONFERRONI  min(p * m, 1).
 * m == 1 returns p unchanged; zeros come out as +0.0.  out_adj: float64 [n_rows][out_ld >= n_cols], or null (top-n only); it may be p
 * itself (in place, out_ld == in_ld).  n_top > 0: out_top int64 [n_rows][top_ld >= n_top] receives the first n_top columns of the row
 * sorted ascending by p, ties by ascending column -- numpy's argsort(p + 0.0, kind="stable")[:, :n_top]; n_top == 0: none.
 * flags: ILLICO_FLAG_INPUT_DEVICE (p on the device), ILLICO_FLAG_OUTPUT_DEVICE (out_adj / out_top on the device).  Host outputs are
 * complete on return, device outputs are ordered on the context's stream.  A deferred call (ILLICO_FLAG_DEFER) is completed first.
 * ILLICO_ERR_ARG: null pointers, a pitch below the width, n_top > n_cols, an unknown method, or a p that is NaN or outside [0, 1]
 * (illico_last_error names the first such (row, column); nothing is written -- except, for a host plane larger than the
 * "scratch_bytes" cap, the batches of rows before the offending one).  Rows of up to ILLICO_ADJ_LDS_COLS p-values are sorted by one
 * workgroup in LDS; longer rows through device scratch (the "scratch_bytes" cap; rows are processed in batches). */
enum { ILLICO_ADJ_BH = 0, ILLICO_ADJ_BY = 1, ILLICO_ADJ_BONFERRONI = 2 };
enum { ILLICO_ADJ_LDS_COLS = 8192 };
int illico_adjust_pvalues(illico_ctx *ctx, const double *p, int64_t n_rows, int64_t n_cols, int64_t in_ld,
                          int method, int flags, double *out_adj, int64_t out_ld,
                          int64_t n_top, int64_t *out_top, int64_t top_ld);
/* Top columns by score: for each row of x (float64 [n_rows][in_ld >= n_cols], a z-score plane), out_top int64 [n_rows][top_ld >= n_top]
 * receives the first n_top columns sorted DESCENDING by x, ties by ascending column -- numpy's
 * argsort(-(x + 0.0), kind="stable")[:, :n_top] (-0.0 and +0.0 tie; +inf first, -inf last).  1 <= n_top <= n_cols.  The sort and merge
 * kernels of the adjustment above, on the order-preserving key of -x + 0.0.  ILLICO_ERR_ARG for a NaN, naming the first (row, column),
 * before anything is written.  flags, residency, batches and a deferred call: as for the adjustment. */
int illico_top_by_score(illico_ctx *ctx, const double *x, int64_t n_rows, int64_t n_cols, int64_t in_ld, int flags,
                        int64_t n_top, int64_t *out_top, int64_t top_ld);

/* ---- per-group expression statistics --------------------------------------------------------
 * For each group g of illico_set_groups and each column j of [col_lb, col_ub) (plane column j - col_lb):
 *   out_nnz[g][j]       int64: cells of g whose value is non-zero (v != 0: -0.0 and stored explicit zeros do not count, NaN does);
 *                       sparse input counts stored non-zero ENTRIES, so a duplicate (row, column) entry counts once per entry, as the
 *                       Wilcoxon routes rank duplicates as separate values;
 *   out_sum[g][j]       float64: the sum of g's values; under ILLICO_FLAG_LOG1P the sum of expm1(v), the quantity the fold change
 *                       divides (one-versus-one: (sum[g] / n_g) / (sum[ref] / n_ref) is fold_change[g]);
 *   out_nnz_rest[g][j], out_sum_rest[g][j]: the same over every cell NOT in g (what one-versus-rest compares against).
 * Sums are exact-limb sums (kernels_group_stats.h): the correctly rounded sum of the values, whatever the input format or the order
 * of the stored entries -- byte-identical across dense / CSC / CSR / bound and from run to run; the rest sums are formed exactly
 * (integer totals minus the group's own), not as a float64 difference.  Values smaller than 2^-83 of the column's largest finite
 * magnitude are truncated at that unit.  NaN / +inf / -inf (or an expm1 that overflows) make the affected sums NaN / +inf / -inf as
 * numpy's sum would (+inf and -inf together: NaN); nothing faults.
 * Planes: row-major [G][out_ld], out_ld >= col_ub - col_lb.  Any of the four pointers may be null (that plane is not produced); at
 * least one must be given.  flags: ILLICO_FLAG_LOG1P, ILLICO_FLAG_INPUT_DEVICE (X / the sparse arrays on the device),
 * ILLICO_FLAG_OUTPUT_DEVICE (all four planes on the device, ordered on the context's stream; host planes are complete on return);
 * other flags are ignored.  Dtypes: the four of ILLICO_F32.., index dtypes ILLICO_IDX_I32 / I64.  CSR rows need not have sorted
 * column indices.  Host dense input is staged column window by column window (the "scratch_bytes" cap), host CSC uploads the
 * entries of [col_lb, col_ub) once, host CSR the whole matrix once.  A deferred call (ILLICO_FLAG_DEFER) is completed first.
 * Errors: ILLICO_ERR_NO_GROUPS (no groups / n_rows mismatch), ILLICO_ERR_BOUNDS, ILLICO_ERR_DTYPE, ILLICO_ERR_ARG (null input,
 * all outputs null, out_ld or ld too small), ILLICO_ERR_UNSUPPORTED (a group of more than 2097151 cells), ILLICO_ERR_OOM. */
int illico_group_stats_dense(illico_ctx *ctx, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                             int64_t col_lb, int64_t col_ub, int flags,
                             int64_t *out_nnz, double *out_sum, int64_t *out_nnz_rest, double *out_sum_rest, int64_t out_ld);
int illico_group_stats_csc(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                           int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags,
                           int64_t *out_nnz, double *out_sum, int64_t *out_nnz_rest, double *out_sum_rest, int64_t out_ld);
int illico_group_stats_csr(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                           int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags,
                           int64_t *out_nnz, double *out_sum, int64_t *out_nnz_rest, double *out_sum_rest, int64_t out_ld);
/* a matrix bound with illico_csr_bind / illico_csc_bind; flags: ILLICO_FLAG_LOG1P, ILLICO_FLAG_OUTPUT_DEVICE */
int illico_group_stats_bound(illico_ctx *ctx, const illico_matrix *matrix, int64_t col_lb, int64_t col_ub, int flags,
                             int64_t *out_nnz, double *out_sum, int64_t *out_nnz_rest, double *out_sum_rest, int64_t out_ld);

/* ---- per-group first and second moments, Welch's t-test ---------------------------------------
 * illico_group_moments_*: for each group g of illico_set_groups and each column j of [col_lb, col_ub) (plane column j - col_lb), float64:
 *   out_sum[g][j]         the sum of g's values x (taken as double);
 *   out_sumsq[g][j]       the sum of fl(x * x);
 *   out_sum_rest[g][j], out_sumsq_rest[g][j]: the same over every cell NOT in g.
 * Arguments, windowing under "scratch_bytes", host / device input and output, bound matrices and the completion of a deferred call are
 * those of illico_group_stats_*.  The pass always works on the values as given: ILLICO_FLAG_LOG1P is ILLICO_ERR_ARG (the t-test is a
 * test on the log values).  It reads the input as often as illico_group_stats_* does.
 * Both sums are exact-limb sums (kernels_group_moments.h): 128-bit totals, rest = total - own in integers, each sum rounded to float64
 * once -- byte-identical across dense / CSC / CSR / bound, host / device input, and from run to run.  The 84 limb bits hold a value
 * exactly while it is within 2^-30 (float32 values: 2^-59) of the column's largest finite magnitude, and the 48-bit square of a float32
 * value while it is within 2^-35 of the column's largest square; smaller ones are truncated toward zero at 2^-83 of the largest.  The
 * squares' scale is fl(v * v), v the column's largest |x| whose square is finite.
 * Non-finite: sum is NaN / +inf / -inf as numpy's would be.  A square that is not finite (NaN, +-inf, |x| beyond about 1.3e154) is kept
 * out of the limbs: sumsq is NaN with a NaN among the values, else +inf with such a square.
 * Any of the four pointers may be null; at least one must be given.  Errors: as illico_group_stats_* (the 2097151-cell group limit is
 * ILLICO_ERR_UNSUPPORTED), plus ILLICO_ERR_ARG for ILLICO_FLAG_LOG1P. */
int illico_group_moments_dense(illico_ctx *ctx, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                               int64_t col_lb, int64_t col_ub, int flags,
                               double *out_sum, double *out_sumsq, double *out_sum_rest, double *out_sumsq_rest, int64_t out_ld);
int illico_group_moments_csc(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                             int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags,
                             double *out_sum, double *out_sumsq, double *out_sum_rest, double *out_sumsq_rest, int64_t out_ld);
int illico_group_moments_csr(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                             int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags,
                             double *out_sum, double *out_sumsq, double *out_sum_rest, double *out_sumsq_rest, int64_t out_ld);
/* a matrix bound with illico_csr_bind / illico_csc_bind; flags: ILLICO_FLAG_OUTPUT_DEVICE */
int illico_group_moments_bound(illico_ctx *ctx, const illico_matrix *matrix, int64_t col_lb, int64_t col_ub, int flags,
                               double *out_sum, double *out_sumsq, double *out_sum_rest, double *out_sumsq_rest, int64_t out_ld);

/* Welch's unequal-variance t-test of every (group, column) from moment planes (float64 [G][in_ld >= n_cols], all on the host, or all on
 * the device with ILLICO_FLAG_INPUT_DEVICE).  The context's groups give the sizes and the test: with a reference group the reference is
 * that group's row of sum / sumsq (the rest planes are not read), otherwise it is the rest planes, which are then required
 * (ILLICO_ERR_ARG).  With n1, S1, Q1 the group's and n2, S2, Q2 the reference's size, sum and sum of squares, every step is one IEEE
 * float64 operation, in this order:
 *     m1 = S1 / n1                  m2 = S2 / n2
 *     q1 = Q1 - S1 * m1             q2 = Q2 - S2 * m2        (q < 0 -> 0; NaN stays NaN)
 *     v1 = q1 / (n1 - 1)            v2 = q2 / (n2 - 1)        (n = 1: 0 / 0 -> NaN)
 *     n2' = n1 for ILLICO_TT_OVERESTIM_VAR (scanpy's "t-test_overestim_var"), else n2
 *     a = v1 / n1                   b = v2 / n2'
 *     t  = (m1 - m2) / sqrt(a + b)
 *     df = ((a + b) * (a + b)) / (a * a / (n1 - 1) + b * b / (n2' - 1));   NaN -> 1   (as scipy)
 * (scanpy's float64 form: the variance carries a relative error of about 2^-52 (1 + mean^2 / var); no exact integer form is offered.)
 * p: two-sided 2 sf(|t|, df), ILLICO_ALT_GREATER sf(t, df), ILLICO_ALT_LESS sf(-t, df), sf Student's t tail in float64 -- what
 * scipy.stats.ttest_ind_from_stats(..., equal_var=False, alternative=...) gives with the group first; p stays a normal number down to
 * 1e-300.  A NaN t (0 / 0, n = 1, NaN input) gives (t, p) = (0, 1); t = +-inf (no variance on either side, different means) is kept and p
 * follows from it; the reference row of a one-versus-reference call gets (0, 1).
 * Outputs: float64 [G][out_ld >= n_cols], each may be null (at least one given): p, t, df, the group's mean m1 and variance v1, the
 * reference's m2 and v2; on the device with ILLICO_FLAG_OUTPUT_DEVICE (ordered on the context's stream), else complete on return.
 * Errors: ILLICO_ERR_NO_GROUPS, ILLICO_ERR_ALTERNATIVE, ILLICO_ERR_ARG (unknown variant, null sum / sumsq, missing rest planes, all
 * outputs null, a pitch below the width). */
enum { ILLICO_TT_WELCH = 0, ILLICO_TT_OVERESTIM_VAR = 1 };
int illico_ttest_from_moments(illico_ctx *ctx, const double *sum, const double *sumsq, const double *sum_rest, const double *sumsq_rest,
                              int64_t n_cols, int64_t in_ld, int variant, int alternative, int flags,
                              double *out_p, double *out_t, double *out_df, double *out_mean, double *out_var,
                              double *out_mean_ref, double *out_var_ref, int64_t out_ld);
/* The same tail, elementwise: out_p[i] from (t[i], df[i]), df > 0 and finite (1 .. about 4e6 is what the test forms), i < n.  NaN for a
 * NaN t, and for an evaluation whose continued fraction did not converge within its step limit.  flags: ILLICO_FLAG_INPUT_DEVICE (t and
 * df), ILLICO_FLAG_OUTPUT_DEVICE (out_p). */
int illico_student_t_pvalues(illico_ctx *ctx, const double *t, const double *df, int64_t n, int alternative, int flags, double *out_p);

/* ---- all-pairs Wilcoxon rank-sum tests from value histograms ----------------------------------
 * Stage 1, illico_group_value_hists_*: for each group g of illico_set_groups (codes, counts and the group-contiguous order are used;
 * the reference / one-versus-rest mode is ignored) and each column j of [col_lb, col_ub), W = col_ub - col_lb:
 *   out_H[(g * W + (j - col_lb)) * 256 + c]   uint32: the cells of g whose value in column j is the integer c, c in 0 .. 255;
 *   out_flags[j - col_lb]                     uint32: non-zero when column j holds a value that is not an integer in [0, 255] (negative,
 *                                             fractional, larger, NaN); out_H of such a column is unspecified.
 * Sparse input gives the dense answer: a stored zero counts in bin 0, the cells that are not stored too (counts[g] minus the stored
 * entries of g); CSR rows need not be sorted.  Input: as illico_group_stats_* (f32 / f64 / i32 / i64 values, i32 / i64 indices, host
 * arrays or, with ILLICO_FLAG_INPUT_DEVICE, device arrays).  Output: host arrays, complete on return, or device arrays with
 * ILLICO_FLAG_OUTPUT_DEVICE (ordered on the context's stream).  The whole window is held in device scratch (G * W KB, twice for dense
 * input): a window beyond "scratch_bytes" is ILLICO_ERR_OOM before any work -- pass narrower windows.  A pending deferred call is
 * completed first.  Errors: ILLICO_ERR_NO_GROUPS, ILLICO_ERR_BOUNDS, ILLICO_ERR_DTYPE, ILLICO_ERR_ARG, ILLICO_ERR_OOM, and
 * ILLICO_ERR_UNSUPPORTED for a dense row pitch of 4 GiB or more. */
int illico_group_value_hists_dense(illico_ctx *ctx, const void *X, int dtype, int64_t n_rows, int64_t n_cols, int64_t ld,
                                   int64_t col_lb, int64_t col_ub, int flags, uint32_t *out_H, uint32_t *out_flags);
int illico_group_value_hists_csc(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                                 int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, uint32_t *out_H, uint32_t *out_flags);
int illico_group_value_hists_csr(illico_ctx *ctx, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype,
                                 int64_t n_rows, int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, uint32_t *out_H, uint32_t *out_flags);
/* Stage 2: every ordered pair of the K = n_sel groups sel[0 .. K) (sel null: all n_groups, in order) from H [n_groups][n_cols][256] and
 * gene_flags [n_cols] as stage 1 writes them (both on the host, or both on the device with ILLICO_FLAG_INPUT_DEVICE; sums goes with
 * them).  counts [n_groups] and sel are HOST arrays; the context's groups are not used.  With h_g, h_r the histograms of group sel[g]
 * and of the reference sel[r], n_g, n_r their sizes, cum_r[c] = sum_{c' < c} h_r[c']:
 *     S2  = sum_c h_g[c] (cum_r[c] + cum_r[c + 1])           U = 0.5 (double)(2 n_r n_g - S2)
 *     tie = (double) sum_c (t^3 - t), t = h_g[c] + h_r[c]    (0.0 without ILLICO_FLAG_TIE_CORRECT)
 * p and z follow as in illico_run_*_ex from U, tie and the sizes (n = n_g + n_r): the same integers and functions as a one-versus-
 * reference call, so plane slab r is that call's [K, n_cols] plane set with reference sel[r].  fold change: (S_g / n_g) / (S_r / n_r),
 * +inf where the reference's mean is 0, S = sums[sel[.]][j] (float64 [n_groups][sums_ld]) or, sums null, sum_c c h[c] (exact).
 * Outputs: float64 [K][K][out_ld >= n_cols] indexed [r][g][j]; out_z may be null.  Diagonal: p = 1, U = n^2 / 2, z = 0.  Columns with a
 * non-zero flag are left untouched in every plane.  flags: ILLICO_FLAG_CONTINUITY, ILLICO_FLAG_TIE_CORRECT, ILLICO_FLAG_INPUT_DEVICE,
 * ILLICO_FLAG_OUTPUT_DEVICE (ILLICO_FLAG_LOG1P is accepted and has no effect: pass the expm1 sums as sums).
 * Refused before anything is written: K < 2, ids of sel outside [0, n_groups) or repeated (ILLICO_ERR_ARG); two selected groups with
 * n_g + n_r >= 2^21 (ILLICO_ERR_UNSUPPORTED: the integer sums hold below that); ILLICO_ERR_ALTERNATIVE; a working set beyond
 * "scratch_bytes" (ILLICO_ERR_OOM). */
int illico_pairwise_from_hists(illico_ctx *ctx, const uint32_t *H, const uint32_t *gene_flags, const int64_t *counts, int64_t n_groups,
                               int64_t n_cols, const int64_t *sel, int64_t n_sel, const double *sums, int64_t sums_ld, int flags,
                               int alternative, double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld);

/* ---- all-pairs Wilcoxon rank-sum tests for any values of a 4-byte type: one sorted walk per gene -----------
 * The illico_pairwise_ranked_* entry points (dense and CSC input) are declared and documented in illico_hip_ranked.h, which includes
 * this header. */

/* ---- measurement hooks (bench.py roofline leg) ------------------------------------------- */
int illico_profile_num_kernels(void);
const char *illico_profile_kernel_name(int kernel_id);
/* Sums HIP-event durations of kernel `kernel_id` since the last reset (synchronises the stream). */
int illico_profile_get(illico_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
int illico_profile_reset(illico_ctx *ctx);
/* Bytes of INPUT (matrix values / indices / index pointers) copied host -> device since the context was created: what a test
 * of "one upload per matrix" looks at. */
int illico_profile_input_bytes(illico_ctx *ctx, int64_t *h2d_bytes);

const char *illico_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ILLICO_HIP_H */
