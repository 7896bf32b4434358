// The context's options: the fields with their defaults (EngineOptions, which illico_ctx derives from), and the one table that
// pairs every name illico_ctx_set_option accepts with what it stores (kEngineOptions, set_engine_option).  A new option is one field,
// one table line and one clause in the comment of include/illico_hip.h (tests/test_host_logic.py compares the two).  Host-only, no HIP.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/illico_hip.h"
#include "kernel_ids.h"

struct EngineOptions {
    int64_t gene_batch = 0;
    int64_t scratch_bytes = 24ll << 30; // (illico_ctx_create: min(64 GiB, a quarter of the device's memory))
    bool no_counts_path = false;
    bool no_fused_path = false;
    bool no_ovr_packed_partition = false; // 1: dense OVR partitions the padded rows (every key) instead of the packed ones
    bool no_packed_dense = false;      // 1: dense OVO on continuous values takes the transpose + k_ovo_rank route (no group-wise packing)
    bool no_sparse_packed_small = false; // sparse OVO, eight-byte keys: genes beyond k_csc_gene's LDS go to k_ovo_rank / the dense window (as before round 5), not to the packed rank kernel
    int csc_counts_max_windows = 0;    // > 0: count-valued CSC with more windows of groups than this leaves the histogram route (8: as before round 5)
    bool no_sparse_byte_values = false; // host-resident sparse input: the stored values always go up in their own type (count values: as bytes otherwise)
    bool no_host_numa = false;         // host-window pipelines: do not confine the fill threads to the NUMA node the caller's matrix lives on
    int host_fill_threads = 0;         // > 0: host threads that fill the pinned slots of the host-window pipelines (default: 12 float32 / 16 byte windows)
    bool debug_routes = false;         // stderr: what the packed OVO rank kernel left to the general routes, and why
    int packed_ref_cap = 0;            // > 0: caps the packed rank kernel's key slots for the reference (tests: value-range parts at small sizes)
    int big_runs_cap = 0;              // > 0: caps k_bucket_big_runs' LDS key slots (tests: the route through HBM at small sizes)
    int big_runs_slice_bytes = 0;      // > 0: the LDS bytes of k_bucket_big_runs_global's slice buffer (default: what the CU's LDS leaves beside the counters)
    bool no_big_runs_wide = false;     // k_bucket_big_runs: 256 threads whatever the runs' length
    bool no_big_runs_global = false;   // packed routes: a (gene, group) run beyond k_bucket_big_runs' LDS slots sends its gene to the general route (as before round 5)
    bool no_compact_order = false;     // k_group_compact: workgroups in grid order whatever the blocks' lengths
    bool no_compact_narrow = false;    // k_group_compact: never the 32-gene tiles for few, long blocks
    int64_t compact_narrow_wgs = 2048;  // ... and the launch would have fewer 64-gene workgroups than this (8 per compute unit)
    int64_t compact_narrow_rows = 8192; // ... from this many rows in the longest block
    bool no_ovr_part_coop = false;     // k_ovr_partition_packed: one wavefront per block whatever the blocks' lengths
    bool no_ovr_packed_big = false;    // dense OVR: groups above 65535 cells take the padded rows (every key, zeros included), as before
    bool no_group_hist_route = false;  // count-valued dense input with few, large groups: the fused kernels (a wavefront per group), as before
    int64_t group_hist_max_wgs = 1024;  // ... while the fused launch would have fewer workgroups than this
    int64_t group_hist_min_cells = 32768; // ... from this many cells (tests lower it)
    bool no_csr_transpose_split = false; // CSR -> CSC on the device: one workgroup per row block whatever their number
    bool no_csc_ovr_small_lds = false; // k_csc_ovr_gene: a CU's whole LDS per workgroup whatever the columns' lengths
    bool no_coop_runs = false;         // packed rank kernel: a long run is walked by one wavefront (as before) instead of all of the workgroup's
    bool no_deal_runs = false;         // packed rank kernel in parts: never deal the short runs by part first (every part then looks every key up, masked)
    bool no_packed_small_wg = false;   // packed rank kernel: never the 256-thread form for small references with few groups
    bool no_ovo_parts = false;         // packed rank kernel: never take a reference in value-range parts (genes beyond the LDS slots go to the general routes, as before round 5)
    int packed_eq_buckets = -1;        // packed rank kernel: distribution-following bucket function; -1 = for references above 16384 cells
    bool no_csc_counts_windows = false; // 1: count-valued CSC with more groups than LDS holds tables for never takes k_csc_counts (windows of groups)
    bool no_csc_counts_wide = false;   // 1: count-valued CSC with more than 8 groups above 255 cells never takes k_csc_counts (16-bit cells)
    bool ovr_full_dump = false;        // 1: the one-pass OVR route dumps whole group histograms (A/B of the shortened dump)
    bool no_wide_gather = false;       // 1: the 256-value stage always runs over the window as it lies (never left to the host's gather)
    bool no_leftover_gather = false;   // 1: the genes the fused passes leave are recomputed as column runs of the input (no gather into a narrow matrix)
    bool no_fused_wide = false;        // 1: no second, 256-value pass of the fused OVO route (genes beyond 63 go to the two-pass routes)
    bool no_csc_regroup_lds = false;   // 1: the two-kernel CSC route regroups with k_csc_segment only
    bool no_csc_gene_path = false;
    bool ovr_rank_whole = false;       // dense OVR rank kernel: one 1024-thread workgroup per CU with all of the LDS (as before round 5) instead of two of 512
    int64_t ovr_parts_cap = 0;         // > 0: keys per part at most in the value-range parts route (tests: many small parts)
    int64_t pair_rank_cap = 0;         // > 0: records per part at most in the ranked pair route (tests: many small parts)
    bool no_ovo_ref_buckets = false;   // 1: the OVO sort route always sorts the reference column (no value-bucket form)
    bool no_ovr_parts_path = false;    // 1: dense OVR (any values) never takes the value-range parts route (k_ovr_partition + k_ovr_rank_gene_parts)
    bool no_csc_ovr_gene_path = false; // 1: CSC OVR never takes the single-kernel LDS-sort route (k_csc_ovr_gene)
    bool csc_ovr_sorted_form = false;  // 1: k_csc_ovr_gene sorts every gene's keys in LDS (the form tie-heavy columns take) instead of bucketing them
    bool no_csc_counts_path = false;   // 1: count-valued CSC genes do not take the LDS-histogram kernel (k_csc_counts)
    bool no_csc_counts_mixed = false;  // 1: k_csc_counts with 8-bit cells for every value only (the form 4-bit overflows fall back to)
    bool no_ovr_one_pass = false;      // 1: dense OVR reads X twice (column histogram, then rank sums) instead of once
    bool no_csr_tile_gather = false;    // 1: CSR -> CSC always by the scatter form (k_csr_block_scatter), as for unsorted rows
    bool no_f64_narrowing = false;      // 1: float64 sparse values that are all float32 values stay with the float64 kernels (A/B)
    bool no_csr_densify_any = false;    // 1: CSR windows with long columns of any values are never handed to the dense routes (A/B)
    bool no_csr_transpose_path = false; // 1: CSR is regrouped by (gene, group) with global atomics instead of being transposed to CSC
    bool dense_window_f32 = false;      // 1: CSR dense windows hold float32 cells instead of bytes
    int host_narrow = 0;               // host-resident count matrices as byte windows: 0 = when a value sample says counts, 1 = always, -1 = never
    bool no_csr_counts_path = false;   // 1: count-valued CSR never takes the group-major single pass (k_csr_counts)
    int csr_counts_abl = 0;            // timing experiments (CsrCountsParams::abl)
    bool no_dense_window_path = false; // 1: CSR never goes through dense float32 windows + the fused kernels
    int fused_groups_per_wg = 0; // 0 = auto
    int fused_mem_policy = 0;    // first OVO pass of the fused route: loads 0 = default / 1 = plain / 2 = non-temporal, + stores 4 = 8 B / 8 = 16 B / 12 = 16 B write-through
    int ovr_hist_groups_per_wg = 0; // k_ovr_from_hists; 0 = auto
    bool profile = false;
    int profile_only = -1;        // >= 0: time this kernel id only (the others run without events around them)
    // "bound_ahead_genes" > 0: a call for FEWER genes of a bound CSR matrix computes the aligned window of that many genes around them
    // into planes of the context's own and hands out slices -- the reference's driver asks for ~256 genes at a time
    // (asymptotic_wilcoxon.py:213-241), and a CSR call walks every row whatever the width of its window (core.hip: run_bound_ahead)
    int64_t bound_ahead_genes = 0;
};

// One option: its name and what a value does to the fields.  A setter that refuses the value says why and returns false.
struct EngineOption {
    const char *name;
    bool (*set)(EngineOptions &, int64_t, std::string *why);
};

// The table's lines.  The name is spelled once per line: it is the key and the field, so a line for a field that does not exist
// does not compile.
#define OPT_VALUE(name, expr) {#name, [](EngineOptions &o, int64_t v, std::string *) { o.name = (expr); return true; }}
#define OPT_FLAG(name) OPT_VALUE(name, v != 0)
#define OPT_INT(name) OPT_VALUE(name, (int)v)
#define OPT_INT64(name) OPT_VALUE(name, v)
#define OPT_POSITIVE(name) OPT_VALUE(name, v > 0 ? v : EngineOptions{}.name) // positive, else the default
#define OPT_AT_LEAST_0(name) OPT_VALUE(name, (int)(v < 0 ? 0 : v))
#define OPT_NO_FIELD(name) {#name, [](EngineOptions &, int64_t, std::string *) { return true; }}
#define OPT_CHECKED(name, fn) {#name, fn}

inline bool set_fused_mem_policy(EngineOptions &o, int64_t v, std::string *why) {
    const bool ok = v >= 0 && v <= 15 && (v & 3) != 3;
    if (ok) o.fused_mem_policy = (int)v;
    else *why = "fused_mem_policy: loads 0 / 1 / 2 plus stores 0 / 4 / 8 / 12, not " + std::to_string((long long)v);
    return ok;
}

inline constexpr EngineOption kEngineOptions[] = {
    OPT_INT64(gene_batch),
    OPT_INT64(scratch_bytes),
    OPT_FLAG(profile),
    OPT_VALUE(profile_only, (v >= 0 && v < KID_COUNT) ? (int)v : -1),
    OPT_FLAG(no_counts_path),
    OPT_FLAG(no_fused_path),
    OPT_FLAG(no_fused_wide),
    OPT_FLAG(no_leftover_gather),
    OPT_FLAG(no_wide_gather),
    OPT_VALUE(bound_ahead_genes, v < 0 ? 0 : v),
    OPT_FLAG(no_csc_counts_windows),
    OPT_FLAG(no_csc_counts_wide),
    OPT_FLAG(ovr_full_dump),
    OPT_FLAG(no_packed_dense),
    OPT_INT(packed_eq_buckets),
    OPT_FLAG(no_ovo_parts),
    OPT_FLAG(no_packed_small_wg),
    OPT_FLAG(no_deal_runs),
    OPT_FLAG(no_coop_runs),
    OPT_FLAG(no_csc_ovr_small_lds),
    OPT_FLAG(no_csr_transpose_split),
    OPT_FLAG(no_group_hist_route),
    OPT_POSITIVE(group_hist_max_wgs),
    OPT_POSITIVE(group_hist_min_cells),
    OPT_FLAG(no_ovr_part_coop),
    OPT_FLAG(no_ovr_packed_big),
    OPT_INT(big_runs_slice_bytes),
    OPT_FLAG(no_big_runs_wide),
    OPT_FLAG(no_compact_order),
    OPT_FLAG(no_compact_narrow),
    OPT_POSITIVE(compact_narrow_wgs),
    OPT_POSITIVE(compact_narrow_rows),
    OPT_FLAG(no_big_runs_global),
    OPT_INT(packed_ref_cap),
    OPT_FLAG(debug_routes),
    OPT_INT(host_fill_threads),
    OPT_NO_FIELD(prewarm_host_window_bytes), // an action of the context, not a field (core.hip: prewarm_host_windows, before the table)
    OPT_FLAG(no_host_numa),
    OPT_FLAG(no_sparse_byte_values),
    OPT_INT(csc_counts_max_windows),
    OPT_FLAG(no_sparse_packed_small),
    OPT_INT(big_runs_cap),
    OPT_FLAG(no_ovr_packed_partition),
    OPT_FLAG(no_csc_counts_path),
    OPT_FLAG(no_csc_counts_mixed),
    OPT_FLAG(no_csc_regroup_lds),
    OPT_FLAG(no_csc_gene_path),
    OPT_INT64(ovr_parts_cap),
    OPT_VALUE(pair_rank_cap, v > 0 ? (v < 1024 ? 1024 : v) : 0), // when positive, at least 1024
    OPT_FLAG(ovr_rank_whole),
    OPT_FLAG(no_ovo_ref_buckets),
    OPT_FLAG(no_ovr_parts_path),
    OPT_FLAG(no_csc_ovr_gene_path),
    OPT_FLAG(csc_ovr_sorted_form),
    OPT_FLAG(no_ovr_one_pass),
    OPT_NO_FIELD(no_ovr_library_sort), // accepted and ignored: there is no library sort any more
    OPT_FLAG(no_csr_tile_gather),
    OPT_FLAG(no_csr_transpose_path),
    OPT_FLAG(no_csr_densify_any),
    OPT_FLAG(no_f64_narrowing),
    OPT_FLAG(dense_window_f32),
    OPT_VALUE(host_narrow, v > 0 ? 1 : (v < 0 ? -1 : 0)), // the sign of the value
    OPT_FLAG(no_csr_counts_path),
    OPT_INT(csr_counts_abl),
    OPT_FLAG(no_dense_window_path),
    OPT_AT_LEAST_0(ovr_hist_groups_per_wg),
    OPT_AT_LEAST_0(fused_groups_per_wg),
    OPT_CHECKED(fused_mem_policy, set_fused_mem_policy),
};

#undef OPT_VALUE
#undef OPT_FLAG
#undef OPT_INT
#undef OPT_INT64
#undef OPT_POSITIVE
#undef OPT_AT_LEAST_0
#undef OPT_NO_FIELD
#undef OPT_CHECKED

enum { ENGINE_OPTION_UNKNOWN = 1 }; // set_engine_option: the table does not hold the key (no status code: the caller words the error)

// Stores `value` under `key`: ILLICO_OK, ILLICO_ERR_ARG with the reason in *why, or ENGINE_OPTION_UNKNOWN.
inline int set_engine_option(EngineOptions &o, const char *key, int64_t value, std::string *why) {
    for (const EngineOption &e : kEngineOptions)
        if (!strcmp(key, e.name)) return e.set(o, value, why) ? ILLICO_OK : ILLICO_ERR_ARG;
    return ENGINE_OPTION_UNKNOWN;
}
