// illico_combine_pairs: the [K, K, W] p-value plane of the pair routes combined into one p-value, one representative reference and
// the effects against it per (group, gene) (kernels_markers.h; include/illico_hip_markers.h).  A translation unit
// of its own: the kernels depend on nothing the Wilcoxon routes use.  They have no profiled kernel id: callers time the call with
// stream events.
#include "plane_stage.h"
#include "../../include/illico_hip_markers.h"
#include "kernels_markers.h"

namespace {

constexpr int kMaxEffects = ILLICO_COMBINE_MAX_EFFECTS;

struct CombineArgs {
    const double *p;
    const double *e[kMaxEffects];
    int64_t K, W, in_ld;
    const uint32_t *skip;
    int method;
    int64_t rank_j;
    int flags;
    double *out_p;
    int32_t *out_rep;
    double *o[kMaxEffects];
    int64_t out_ld;
};

// the first invalid p of the wb columns at dp (column 0 there is column col0 of the call): ILLICO_ERR_ARG naming it, or OK
int mk_validate(illico_ctx *c, const CombineArgs &a, const double *dp, int64_t dld, int64_t wb, const u32 *dskip, int64_t col0, bool staged, u64 *d_err) {
    HIPCHK(c, hipMemsetAsync(d_err, 0xFF, 8, c->stream));
    const unsigned gx = (unsigned)std::min<int64_t>((wb + 255) / 256, 64);
    KERNELCHK(c, k_mk_validate, dim3(gx, (unsigned)a.K, (unsigned)a.K), dim3(256), 0, dp, (long long)dld, (int)a.K, (long long)wb, dskip, d_err);
    u64 err = 0;
    HIPCHK(c, hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (err == ~0ull) return ILLICO_OK;
    const int64_t rk = (int64_t)(err / (u64)wb), col = (int64_t)(err % (u64)wb);
    double v = 0.0;
    if (staged) v = a.p[rk * a.in_ld + col0 + col];
    else HIPCHK(c, hipMemcpy(&v, dp + rk * dld + col, 8, hipMemcpyDeviceToHost));
    return fail(c, ILLICO_ERR_ARG, "p-value at (reference %lld, group %lld, column %lld) is %.17g: p-values must lie in [0, 1]", (long long)(rk / a.K),
                (long long)(rk % a.K), (long long)(col0 + col), v);
}

int mk_launch(illico_ctx *c, const MkParams &P, int method) {
    const dim3 grid((unsigned)((P.W + MK_NT - 1) / MK_NT), (unsigned)P.K);
    const size_t lds = mk_lds_bytes(P.K, method);
    if (method == ILLICO_COMBINE_ALL) return launch_kernel(c, k_mk_combine<ILLICO_COMBINE_ALL>, grid, dim3(MK_NT), lds, P);
    if (method == ILLICO_COMBINE_ANY) return launch_kernel(c, k_mk_combine<ILLICO_COMBINE_ANY>, grid, dim3(MK_NT), lds, P);
    return launch_kernel(c, k_mk_combine<ILLICO_COMBINE_SOME>, grid, dim3(MK_NT), lds, P);
}

int mk_run(illico_ctx *c, const CombineArgs &a) {
    const int64_t K = a.K, W = a.W, KK = K * K;
    const bool in_dev = a.flags & ILLICO_FLAG_INPUT_DEVICE, out_dev = a.flags & ILLICO_FLAG_OUTPUT_DEVICE;
    int ne = 0;
    for (int k = 0; k < kMaxEffects; ++k) ne += a.e[k] ? 1 : 0;
    // device bytes per column of a batch: the staged planes of host input, the staged outputs of host planes
    const size_t b_in = in_dev ? 0 : (size_t)(1 + ne) * KK * 8, b_skip = (in_dev || !a.skip) ? 0 : 4;
    const size_t b_out = out_dev ? 0 : (size_t)(1 + ne) * K * 8, b_rep = out_dev ? 0 : (size_t)K * 4;
    int rc;
    u64 *d_err;
    if ((rc = scratch(c, "mk_err", 2, &d_err))) return rc;
    StageWindows sw;
    if ((rc = plan_stage_windows(c, W, b_in + b_out + b_rep + b_skip, kNoWindowCap, "mk_work", &sw))) return rc;

    // device input is looked at whole before anything is written; host input batch by batch, as it arrives
    if (in_dev && (rc = mk_validate(c, a, a.p, a.in_ld, W, a.skip, 0, false, d_err))) return rc;
    const bool preload = a.skip != nullptr; // with skipped columns the caller's planes go up first: those columns come back as they were
    for (int64_t b0 = 0; b0 < W; b0 += sw.WW) {
        const int64_t wb = std::min<int64_t>(sw.WW, W - b0);
        PlaneStage st(c, sw.block, b0, wb);
        MkParams P{};
        P.K = (int)K;
        P.W = wb;
        P.rank_j = (int)a.rank_j;
        P.p = st.in(a.p, a.in_ld, KK, in_dev);
        for (int k = 0; k < kMaxEffects; ++k) P.e[k] = st.in(a.e[k], a.in_ld, KK, in_dev);
        P.in_ld = st.pitch(a.in_ld, in_dev);
        P.skip = st.in(a.skip, W, 1, in_dev);
        if (st.rc) return st.rc;
        if (!in_dev && (rc = mk_validate(c, a, P.p, P.in_ld, wb, P.skip, b0, true, d_err))) return rc;
        P.out_p = st.out(a.out_p, a.out_ld, K, out_dev, preload);
        for (int k = 0; k < kMaxEffects; ++k) P.o[k] = st.out(a.e[k] ? a.o[k] : nullptr, a.out_ld, K, out_dev, preload);
        P.out_rep = st.out(a.out_rep, a.out_ld, K, out_dev, preload);
        P.out_ld = st.pitch(a.out_ld, out_dev);
        if (st.rc) return st.rc;
        if ((rc = mk_launch(c, P, a.method))) return rc;
        if ((rc = st.finish())) return rc;
    }
    return ILLICO_OK;
}

} // namespace

extern "C" int illico_combine_pairs(illico_ctx *c, const double *p, const double *e0, const double *e1, const double *e2, const double *e3, int64_t K, int64_t W,
                                    int64_t in_ld, const uint32_t *skip, int method, int64_t rank_j, int flags, double *out_p, int32_t *out_rep, double *o0,
                                    double *o1, double *o2, double *o3, int64_t out_ld) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    const CombineArgs a{p, {e0, e1, e2, e3}, K, W, in_ld, skip, method, rank_j, flags, out_p, out_rep, {o0, o1, o2, o3}, out_ld};
    if (K < 2) return fail(c, ILLICO_ERR_ARG, "%lld groups: a pair needs two", (long long)K);
    if (K > ILLICO_COMBINE_MAX_GROUPS)
        return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld groups: illico_combine_pairs takes up to %d", (long long)K, ILLICO_COMBINE_MAX_GROUPS);
    if (W < 0) return fail(c, ILLICO_ERR_ARG, "negative number of columns %lld", (long long)W);
    if (method != ILLICO_COMBINE_ALL && method != ILLICO_COMBINE_ANY && method != ILLICO_COMBINE_SOME)
        return fail(c, ILLICO_ERR_ARG, "unknown combination method %d", method);
    if (method == ILLICO_COMBINE_SOME && (rank_j < 1 || rank_j > K - 1))
        return fail(c, ILLICO_ERR_ARG, "rank_j %lld outside [1, K - 1 = %lld]", (long long)rank_j, (long long)(K - 1));
    if (in_ld < W) return fail(c, ILLICO_ERR_ARG, "in_ld %lld smaller than the %lld columns", (long long)in_ld, (long long)W);
    if (out_ld < W) return fail(c, ILLICO_ERR_ARG, "out_ld %lld smaller than the %lld columns", (long long)out_ld, (long long)W);
    if (!p || !out_p || !out_rep) return fail(c, ILLICO_ERR_ARG, "null p, out_p or out_rep");
    for (int k = 0; k < kMaxEffects; ++k)
        if (a.e[k] && !a.o[k]) return fail(c, ILLICO_ERR_ARG, "effect plane %d has no output plane", k);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = resolve_pending(c); // a plane written under ILLICO_FLAG_DEFER is complete only after its leftover genes
    if (rc) return rc;
    if (W == 0) return ILLICO_OK;
    return mk_run(c, a);
}
