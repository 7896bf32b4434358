// Host-side shared definitions of libillico_hip: the context, its helpers, the dispatch on the value / index types, and the
// declarations that tie the translation units together.  core.hip holds the context / C-ABI / deferred-call protocol; keyed_*.hip
// the launchers that depend on the key type only; dense_*.hip / sparse_*.hip one value type each (explicit instantiations of
// dense_driver.h / sparse_driver.h); group_stats / group_moments / pairwise.hip the per-group passes (group_pass.h).
#pragma once
#include <cstring>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/illico_hip.h"
#include "common.h"
#include "options.h" // EngineOptions; with kernel_ids.h: the KID_* ids and kKernelNames
#include "kernels_finalize.h"
#include "kernels_ovo.h"
#include "kernels_ovo_compact.h"
#include "kernels_ovo_counts.h"
#include "kernels_ovo_fused.h"
#include "kernels_group_hists.h"
#include "kernels_ovr.h"
#include "kernels_sparse.h"
#include "kernels_csc_gene.h"
#include "kernels_csc_counts.h"
#include "kernels_ovr_rank.h"
#include "kernels_csc_ovr.h"
#include "kernels_ovr_partition.h"
#include "kernels_ovr_parts.h"
#include "kernels_sums.h"
#include "kernels_leftover.h"
#include "kernels_csr_counts.h"

struct OutPlanes {
    double *p, *u, *fc; // device
    int64_t ld;
    bool staged;
    double *z = nullptr; // device z-score plane (the *_ex entry points), null = none
    OutPlanes shifted(int64_t j) const { return {p + j, u + j, fc + j, ld, staged, z ? z + j : nullptr}; } // column j on
};

// A call made with ILLICO_FLAG_DEFER whose single pass is in flight: which genes it could not take is known only once
// its route flags have reached the host; they are then recomputed by the ordinary routes (resolve_pending).
struct PendingDense {
    bool on = false;
    int kind = 0;                 // 0: dense (X, ld), 1: CSC (sp_*: the count-valued CSC pass, sparse_driver.h)
    const void *sp_data = nullptr, *sp_indices = nullptr, *sp_indptr = nullptr;
    int idx_dtype = 0;
    int64_t n_cols = 0;
    const void *X = nullptr;
    int dtype = 0, flags = 0, alternative = 0, slot = 0;
    bool is_csr = false;          // kind 1: the arrays are CSR (the group-major count pass, kernels_csr_counts.h)
    bool sorted_known = false;    // kind 1, CSR: the matrix was bound and its rows found in order (illico_ctx::cur_sorted_known when the call was made)
    int64_t N = 0, ld = 0, col_lb = 0, col_ub = 0, out_ld = 0;
    double *p = nullptr, *u = nullptr, *fc = nullptr;
    double *z = nullptr;          // the call's z-score plane (null: none): complete exactly when p is
    OutPlanes planes() const { return {p, u, fc, out_ld, false, z}; }
};

// a sparse matrix bound to a context (illico_csr_bind / illico_csc_bind): device arrays, owned or adopted
struct illico_matrix {
    illico_ctx *owner = nullptr;
    bool is_csr = false, owns = false;
    int dtype = 0, idx_dtype = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    void *d_data = nullptr, *d_indices = nullptr, *d_indptr = nullptr;
    int sorted = -1;              // CSR: 1 = every row's column indices ascend (looked at once, when the matrix is bound), 0 = not, -1 = not looked at
};

struct ProfEvent {
    int kid;
    hipEvent_t a, b;
};

// (the option fields -- c->no_fused_path, c->profile, c->scratch_bytes ... -- are EngineOptions': options.h)
struct illico_ctx : EngineOptions {
    // Every entry point that takes the context holds this lock for the whole call: two host threads driving ONE context
    // (the reference's joblib threads share one dispatcher, asymptotic_wilcoxon.py:236-241) are serialised, not raced.
    std::recursive_mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // groups
    bool has_groups = false;
    int64_t n_cells = 0, n_groups = 0, ref = -1;
    std::vector<int> h_counts;
    int64_t max_nonref = 0;
    bool big_n = false;           // OVR over more than 2^21 - 1 cells: sparse input only, on the routes whose arithmetic does not wrap
    int *d_codes = nullptr;       // [N] group code of each cell
    int *d_perm = nullptr;        // [N] cell index at group-contiguous position p
    int *d_posptr = nullptr;      // [G+1]
    int *d_pk_blk = nullptr;      // packed dense layout (kernels_ovo_compact.h): [pk_nblk+1] first group of each block, then [pk_nblk] first key slot
    int pk_nblk = 0, pk_ref_out = 0;
    int *d_pk_code = nullptr;     // padded dense layout (dense OVR): group code of every key slot (holes: 0, they hold zero keys)
    int64_t pk_stride = 0;        // keys per gene in the packed layout
    int *d_pk_big = nullptr;      // [pk_nbig] the groups (never the reference) of more than 256 cells: their packed runs may need k_bucket_big_runs;
                                  // then [G]: a group's place in that list, or -1
    int pk_nbig = 0;
    int64_t pk_max_block_rows = 0; // rows of the longest block
    int *d_pk_order = nullptr;    // [pk_nblk] the blocks by falling row count, or null when their lengths are alike (k_group_compact starts the longest first)
    int pk_nlong = 0;             // blocks of more than OVRP_LONG_ROWS rows and at most 64 groups (k_ovr_partition_packed deals their units over all wavefronts)
    int *d_pk_long = nullptr;     // [pk_nlong] those blocks
    unsigned char *d_pk_islong = nullptr; // [pk_nblk]
    int64_t pk_len = 0;           // ... of which the blocks take the first pk_len (the padded dense layout's row length)
    int *d_counts = nullptr;      // [G]
    GroupConst *d_gconst = nullptr; // [G] per-group constants of the p-value / fold change for this ref (kernels_finalize.h)
    int *d_code_by_pos = nullptr; // [N] group code at position p
    u32 *d_hist_off = nullptr;    // [G+1] OVR one-pass histograms: words per lane before group g (16 per group of <= 255 cells, else 32)
    size_t hist_words = 0;        // d_hist_off[G]
    u16 *d_codes16 = nullptr;     // [N] d_codes as 16-bit values when G <= 65535 (half the cache lines per codes[row] gather), else null
    // the group-major CSR pass (kernels_csr_counts.h): row chunks of its histogram pre-pass -- slab 0 = the reference group's rows (OVO; OVR:
    // the column histograms come out of the count pass itself), slab 1 + k = the k-th group of more than 255 cells -- as [3][csr_n_chunks] {p0, rows, slab}, then [csr_n_big] group numbers
    int *d_csr_chunks = nullptr;
    int csr_n_chunks = 0, csr_n_big = 0; // csr_n_big < 0: more big groups than the route takes
    bool cur_sorted_known = false;       // the running call is on a bound CSR matrix whose rows were found in order when it was bound
    bool fused_tie_sparse = false;       // the fused OVR kernels run on a window of CSR input: tie sums as the reference's SPARSE path forms them
    bool hold_csr_counts = false;        // set while a deferred call's leftover genes are recomputed (they must not come back to the route)
    PendingDense pend;            // deferred dense call (ILLICO_FLAG_DEFER), see resolve_pending
    void *pend_pinned[2] = {nullptr, nullptr}; // its route flags arrive here (two buffers: the next call may be enqueued first)
    size_t pend_pinned_bytes[2] = {0, 0};
    hipEvent_t pend_event[2] = {nullptr, nullptr};
    int pend_next = 0;
    void *out_pin[2] = {nullptr, nullptr}; // pinned buffers + events of end_outputs (host planes)
    size_t out_pin_bytes = 0;
    hipEvent_t out_ev[2] = {nullptr, nullptr};
    void *pinned = nullptr;       // pinned host staging for small device -> host results
    size_t pinned_bytes = 0;
    int64_t h2d_input_bytes = 0;  // matrix bytes copied host -> device (illico_profile_input_bytes)
    std::vector<illico_matrix *> bound; // matrices bound to this context and not yet released
    uint64_t groups_gen = 0;      // counts illico_set_groups calls (the windows below belong to one set of groups)
    struct AheadWindow {
        const illico_matrix *m = nullptr;
        uint64_t gen = 0, stamp = 0;
        int flags = 0, alternative = 0;
        int64_t lb = 0, ub = 0;
        double *planes = nullptr;   // device, [3][G][ub - lb]
        size_t cap = 0;             // bytes
    } ahead[2];
    uint64_t ahead_clock = 0;
    struct HostStage *host_stage = nullptr; // pinned slots / copy stream of the host-window pipeline (dense driver)
    std::vector<ProfEvent> events;
    std::vector<hipEvent_t> event_pool;
    double prof_ms[KID_COUNT] = {0};
    int64_t prof_n[KID_COUNT] = {0};
    // grow-only scratch
    std::map<std::string, std::pair<void *, size_t>> scratch;
    // illico_rank_statistics: host arrays that receive the integer rank statistics of the two-pass routes instead of the
    // finalisation ([W][G] each, W = the call's column window)
    struct StatsTap { long long *two_u; u64 *tie; double *sum; } *tap = nullptr;
};

#define CTX_LOCK(c) std::lock_guard<std::recursive_mutex> ctx_lock__((c)->mu)

int fail(illico_ctx *c, int code, const char *fmt, ...);

#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            return fail(ctx, e__ == hipErrorOutOfMemory ? ILLICO_ERR_OOM : ILLICO_ERR_HIP, "%s failed: %s (%s:%d)", \
                        #call, hipGetErrorString(e__), __FILE__, __LINE__);                            \
    } while (0)

int get_scratch(illico_ctx *c, const char *name, size_t bytes, void **out);
// `count` elements of T from the grow-only scratch block `name`.  A block that is carved into several arrays is
// asked for as bytes (T = unsigned char) or in units of its first array, and carved by the caller.
template <typename T> int scratch(illico_ctx *c, const char *name, size_t count, T **out) {
    void *v;
    int rc = get_scratch(c, name, count * sizeof(T), &v);
    *out = (T *)v;
    return rc;
}

// A kernel's dynamic-LDS limit on `device` raised to `lds`, unless it has been raised that far already: the limit is the kernel's, not a
// context's, so what has been set is kept once for the process (a context that set a smaller one later would lower it under the others).
// The runtime call made before every launch showed in the steady per-step time of the dense OVO pass.
inline hipError_t raise_lds_limit(int device, const void *kern, size_t lds) {
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> raised;
    std::lock_guard<std::mutex> g(mu);
    size_t &have = raised[{device, kern}];
    if (lds <= have) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) have = lds;
    return e;
}
// One kernel launch on the context's stream, checked where it is made: with dynamic LDS the kernel's limit is
// raised to `lds` first.  No ProfScope: the caller places it, often around several launches.  launch_kernel(c, kern, grid, block, lds,
// args...) returns ILLICO_OK or the code of fail(); KERNELCHK(...) returns from the calling function on failure, as HIPCHK does.
template <typename... KArgs, typename... Args>
int launch_kernel_at(illico_ctx *c, const char *file, int line, const char *what, void (*kern)(KArgs...), dim3 grid, dim3 block, size_t lds, Args &&...args) {
    hipError_t e = lds > 0 ? raise_lds_limit(c->device, (const void *)kern, lds) : hipSuccess;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kern, grid, block, lds, c->stream, std::forward<Args>(args)...);
        e = hipGetLastError();
    }
    if (e == hipSuccess) return ILLICO_OK;
    return fail(c, e == hipErrorOutOfMemory ? ILLICO_ERR_OOM : ILLICO_ERR_HIP, "launch_kernel(%s) failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
}
#define launch_kernel(ctx, ...) launch_kernel_at(ctx, __FILE__, __LINE__, #__VA_ARGS__, __VA_ARGS__)
#define KERNELCHK(ctx, ...)                                \
    do {                                                   \
        int rc__ = launch_kernel(ctx, __VA_ARGS__);        \
        if (rc__) return rc__;                             \
    } while (0)

hipEvent_t take_event(illico_ctx *c);

struct ProfScope {
    illico_ctx *c;
    int kid;
    hipEvent_t a = nullptr, b = nullptr;
    bool on;
    ProfScope(illico_ctx *c_, int kid_) : c(c_), kid(kid_), on(c_->profile && (c_->profile_only < 0 || c_->profile_only == kid_)) {
        if (on) {
            a = take_event(c);
            b = take_event(c);
            hipEventRecord(a, c->stream);
        }
    }
    ~ProfScope() {
        if (on) {
            hipEventRecord(b, c->stream);
            c->events.push_back({kid, a, b});
        }
    }
};

// ---- small host idioms shared by the drivers ----
// Ask the device up to four words.  clear_flag_words: the "flag" scratch, zeroed, on the context's stream.  device_probe: that, then
// `launch(words)` (the caller's kernel launches, through launch_kernel: it returns their status), the first `n` words copied to `out`
// -- and the wait for them, unless `wait` is false (the caller then waits itself, with further copies behind the same wait).  The
// scratch is shared by name: a probe's words are read before the next probe is enqueued.
static inline int clear_flag_words(illico_ctx *c, u32 **words) {
    int rc = scratch(c, "flag", 4, words);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(*words, 0, 16, c->stream));
    return ILLICO_OK;
}
template <typename Launch> static int device_probe(illico_ctx *c, u32 *out, int n, Launch &&launch, bool wait = true) {
    u32 *words;
    int rc = clear_flag_words(c, &words);
    if (rc) return rc;
    if ((rc = launch(words))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, words, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (wait) HIPCHK(c, hipStreamSynchronize(c->stream));
    return ILLICO_OK;
}
// the context's pinned staging for small device -> host results, grown to `bytes`
static inline int ensure_pinned(illico_ctx *c, size_t bytes) {
    if (c->pinned_bytes >= bytes) return ILLICO_OK;
    if (c->pinned) hipHostFree(c->pinned);
    c->pinned = nullptr;
    c->pinned_bytes = 0;
    HIPCHK(c, hipHostMalloc(&c->pinned, bytes + 4096, hipHostMallocDefault));
    c->pinned_bytes = bytes + 4096;
    return ILLICO_OK;
}
// the per-gene words a kernel left for `nb` genes, on the host (the context's pinned staging): one wait
static inline int read_gene_flags(illico_ctx *c, const u32 *d_flags, int nb, const u32 **h_flags) {
    int rc = ensure_pinned(c, (size_t)nb * 4);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->pinned, d_flags, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *h_flags = (const u32 *)c->pinned;
    return ILLICO_OK;
}
// The "stats" scratch of the two-pass routes carved for `nb` genes: doubled rank sums, tie sums, value sums ([nb][G] each), gene
// totals ([nb]); with_flags: the per-gene words of "gene_flags" too (else null).  stats_batch_genes: how many genes of `n` one carving
// takes (4 GB of statistics at the most).
struct StatsPlanes { long long *s2u; u64 *stie; double *ssum, *gtot; u32 *flags; };
static inline int64_t stats_batch_genes(int64_t n, int G) {
    return std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)((size_t)(4ll << 30) / ((size_t)G * 24 + 16))));
}
static inline int carve_stats(illico_ctx *c, int64_t nb, int G, bool with_flags, StatsPlanes *s) {
    unsigned char *v;
    int rc = scratch(c, "stats", (size_t)nb * G * 24 + (size_t)nb * 8, &v);
    if (rc) return rc;
    s->s2u = (long long *)v;
    s->stie = (u64 *)(s->s2u + (size_t)nb * G);
    s->ssum = (double *)(s->stie + (size_t)nb * G);
    s->gtot = s->ssum + (size_t)nb * G;
    s->flags = nullptr;
    if (with_flags && (rc = scratch(c, "gene_flags", (size_t)nb, &s->flags))) return rc;
    return ILLICO_OK;
}

void drain_events(illico_ctx *c);
// ---- deferred calls (core.hip) ----
int resolve_pending(illico_ctx *c); // completes the deferred call in flight, if any
// A route that defers: reserve_deferred_slot (pinned room for `bytes` of route flags, the slot's event), then its own device-to-host
// copies into `pin` on the context's stream, then post_deferred_call (records the event, installs c->pend from the common fields);
// what is the route's own -- X / ld, or sp_* / idx_dtype / n_cols / is_csr / sorted_known -- it sets in c->pend afterwards.
int reserve_deferred_slot(illico_ctx *c, size_t bytes, int *slot, void **pin);
int post_deferred_call(illico_ctx *c, int slot, int kind, int dtype, int flags, int alternative, int64_t N, int64_t col_lb, int64_t col_ub,
                       const OutPlanes &o);
// a handle of illico_csr_bind / illico_csc_bind, under the context's lock (held by the caller for the whole call: illico_matrix_release on
// another thread cannot free the arrays under it).  The list is searched first: a released handle is not read.
int check_bound_matrix(illico_ctx *c, const illico_matrix *m);

#define FUSED_RT 64 // table size of the fused single-pass routes (values 0 .. 63)
static const size_t kMaxLds = 160 * 1024;
static const int kOvoThreads = 512;

static inline size_t dtype_size(int dt) { return (dt == ILLICO_F32 || dt == ILLICO_I32) ? 4 : 8; }

// pinned slots / copy stream of the host-window pipeline (dense_driver.h: host_windows_pipeline); one per context, freed with it
#define HS_SLOTS 3
struct HostStage {
    void *pin[HS_SLOTS] = {nullptr, nullptr, nullptr};
    size_t pin_bytes = 0;
    int *lists = nullptr;        // pinned: column lists of the flagged genes, window after window (gathered leftovers)
    size_t lists_ints = 0;
    hipStream_t copy = nullptr;
    hipEvent_t up[HS_SLOTS] = {nullptr, nullptr, nullptr}, done[HS_SLOTS] = {nullptr, nullptr, nullptr};
    void *sp_pin[2] = {nullptr, nullptr}; // pinned byte chunks of a sparse matrix's count values on their way up (sparse_driver.h)
    hipEvent_t sp_up[2] = {nullptr, nullptr};
};
HostStage *host_stage_of(illico_ctx *c);
void free_host_stage(illico_ctx *c);

// ---- dispatch on the value / index types ----
// f(Tag<value type>{}) for a checked dtype code: every build instantiates f for all four value types (the per-group passes)
template <typename T> struct Tag { using type = T; };
template <typename F> int dispatch_value_type(int dt, F &&f) {
    switch (dt) {
    case ILLICO_F32: return f(Tag<float>{});
    case ILLICO_F64: return f(Tag<double>{});
    case ILLICO_I32: return f(Tag<int32_t>{});
    default: return f(Tag<int64_t>{});
    }
}
// Run-time flags as template arguments: dispatch_flags(f, a, b) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}) -- a generic
// lambda that reads them as `decltype(x)::value` / x.value.  dispatch_int<64, 32>(v, f): f(std::integral_constant<int, V>{}) for the
// listed value that v equals, the last one otherwise.  f is instantiated for every combination: where a kernel exists for some of them
// only, the lambda guards the others with `if constexpr`.
template <typename F> int dispatch_flags(F &&f) { return f(); }
template <typename F, typename... Bs> int dispatch_flags(F &&f, bool b, Bs... rest) {
    return b ? dispatch_flags([&](auto... cs) { return f(std::true_type{}, cs...); }, rest...)
             : dispatch_flags([&](auto... cs) { return f(std::false_type{}, cs...); }, rest...);
}
template <int V0, int... Vs, typename F> int dispatch_int(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
    else return v == V0 ? f(std::integral_constant<int, V0>{}) : dispatch_int<Vs...>(v, f);
}
// The Wilcoxon drivers: f(Tag<InT>{}, Tag<KeyT>{}), or with an index dtype code f(Tag<InT>{}, Tag<IdxT>{}, Tag<KeyT>{}) -- for the
// types the build holds.  A development build (ILLICO_DEV_F32_ONLY=1 python build.py: 4x faster) compiles the float32 / int32-index
// drivers only, and f is instantiated for nothing else.
#ifndef ILLICO_DEV_F32_ONLY
template <typename F> int dispatch_driver_types(illico_ctx *, int dt, F &&f) {
    return dispatch_value_type(dt, [&](auto v) { return f(v, Tag<std::conditional_t<sizeof(typename decltype(v)::type) == 4, u32, u64>>{}); });
}
template <typename F> int dispatch_driver_types(illico_ctx *c, int dt, int idx_dtype, F &&f) {
    return dispatch_driver_types(c, dt, [&](auto v, auto k) { return idx_dtype == ILLICO_IDX_I32 ? f(v, Tag<int32_t>{}, k) : f(v, Tag<int64_t>{}, k); });
}
#else
template <typename F> int dispatch_driver_types(illico_ctx *c, int dt, F &&f) {
    return dt == ILLICO_F32 ? f(Tag<float>{}, Tag<u32>{}) : fail(c, ILLICO_ERR_DTYPE, "this development build holds the float32 kernels only");
}
template <typename F> int dispatch_driver_types(illico_ctx *c, int dt, int idx_dtype, F &&f) {
    return dt == ILLICO_F32 && idx_dtype == ILLICO_IDX_I32 ? f(Tag<float>{}, Tag<int32_t>{}, Tag<u32>{})
                                                            : fail(c, ILLICO_ERR_DTYPE, "this development build holds the float32 / int32-index kernels only");
}
#endif

// ---- non-template host helpers (core.hip) ----
int ovo_counts_limit(const illico_ctx *c);           // table size of the two-pass histogram route (k_ovo_counts)
bool counts_path_allowed(const illico_ctx *c, int flags);
bool fused_path_allowed(const illico_ctx *c, int flags);
int launch_finalize(illico_ctx *c, const long long *s2u, const u64 *stie, const double *ssum, const double *gene_total, int nb, int flags,
                    int alternative, const OutPlanes &o, int64_t col_off, const int *col_map = nullptr, bool packed = false, bool tie_f64 = false);
int launch_gene_totals(illico_ctx *c, const double *ssum, int G, int nb, double *gtot);
void flagged_runs(const u32 *hf, int64_t wn, int64_t w0, std::vector<std::pair<int64_t, int64_t>> &runs);

// ---- per-value-type entry points (dense_driver.h / sparse_driver.h; one explicit instantiation per type, in its own translation unit) ----
template <typename InT, typename KeyT>
int run_dense_t(illico_ctx *c, const void *X, int dtype, int64_t N, int64_t ld, int64_t col_lb, int64_t col_ub, int flags, int alternative,
                const OutPlanes &o);
template <typename InT, typename KeyT>
int run_leftovers(illico_ctx *c, const void *X, int dtype, int64_t N, int64_t ld, int64_t col_lb, int64_t col_ub, int flags, int alternative,
                  const OutPlanes &o, const u32 *hf, bool wide_skipped = false, const int *outer = nullptr);
// One call of the fused single pass (run_fused_ovo, dense_driver.h): genes [b0, b0 + nb) of X, whose column j is
// column col_off + j of the planes.  defer_slot >= 0: the route flags go to that deferred slot and nobody waits; probe: find the
// count-valued genes on the device first (OVR); max_gather > 0: the device may leave the 256-value stage to the host when at most
// that many genes are flagged; init_flags (host, [nb]): the 256-value stage alone, for the genes marked 1.
struct FusedCall {
    const void *X;
    int64_t ld, b0;
    int nb, flags, alternative;
    OutPlanes o;
    int64_t col_off;
    int defer_slot = -1; bool probe = false; int64_t max_gather = 0; const u32 *init_flags = nullptr;
};
template <typename InT> int run_fused_ovo(illico_ctx *c, const FusedCall &q, std::vector<u32> &h_flags);
// Which routes a (re-)entry of run_sparse_t may still take.  `indices_are_codes`: CSC whose `indices` hold the
// group code of each stored entry's cell (what the device CSR -> CSC transposition writes: the per-entry lookup codes[row] is an
// uncoalesced gather the CSC kernels then skip).
struct SparseAllow {
    bool dense_window, transpose, indices_are_codes, csr_counts;
    static SparseAllow everything() { return {true, true, false, true}; }           // the entry from core.hip
    static SparseAllow after_csr_counts() { return {true, true, false, false}; }    // the whole window again, without the group-major pass
    static SparseAllow exact_window() { return {false, true, false, false}; }       // the exact sparse routes over a window of left-over genes
    static SparseAllow transposed_codes() { return {false, false, true, false}; }   // the CSC the device transposition wrote
    SparseAllow in_float32() const { return {dense_window, transpose, indices_are_codes, false}; } // the same call, values narrowed
};
template <typename InT, typename IdxT, typename KeyT>
int run_sparse_t(illico_ctx *c, bool is_csr, const void *data, const void *indices, const void *indptr, int dtype, int64_t n_rows, int64_t n_cols,
                 int64_t col_lb, int64_t col_ub, int flags, int alternative, const OutPlanes &o, SparseAllow allow);
// the run_sparse_t of a type given by its codes (core.hip; what a deferred CSC pass's leftovers and the drivers' own re-entries call)
int run_sparse_inner(illico_ctx *c, bool is_csr, const void *data, int dtype, const void *indices, const void *indptr, int idx_dtype, int64_t n_rows,
                     int64_t n_cols, int64_t col_lb, int64_t col_ub, int flags, int alternative, const OutPlanes &o);

// the alternative code, as the t-test and the pair entry points check it
static inline int check_alternative(illico_ctx *c, int alternative) {
    if (alternative != ILLICO_ALT_TWO_SIDED && alternative != ILLICO_ALT_LESS && alternative != ILLICO_ALT_GREATER)
        return fail(c, ILLICO_ERR_ALTERNATIVE, "Unsupported alternative hypothesis code: %d", alternative);
    return ILLICO_OK;
}
