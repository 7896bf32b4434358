// illico_pair_ttest_from_moments: Welch's t-test of every ordered pair of the selected groups from the moment planes of
// illico_group_moments_* (kernels_pair_ttest.h; include/illico_hip_pair_ttest.h).  A translation unit of its own:
// a sibling of illico_ttest_from_moments (group_moments.hip), whose tail it reuses and whose kernel it does not touch.  Like
// illico_combine_pairs the kernel has no profiled kernel id (the pinned list of kernel_ids.h stays as it is): callers time the call
// with stream events.
#include "group_pass.h"
#include "../../include/illico_hip_pair_ttest.h"
#include "kernels_pair_ttest.h"

namespace {

// gridDim.z: the pairs of a workgroup's tile pair dealt over `split` workgroups, until the launch holds about four wavefronts per SIMD
int pt_split(illico_ctx *c, int64_t gene_tiles, int64_t tile_pairs) {
    int cus = 256;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    const int64_t want = (int64_t)std::max(cus, 1) * 16, have = gene_tiles * tile_pairs * (PT_NT / 64);
    return (int)std::max<int64_t>(1, std::min<int64_t>(PT_MAX_SPLIT, (want + have - 1) / have));
}

} // namespace

extern "C" int illico_pair_ttest_from_moments(illico_ctx *c, const double *sum, const double *sumsq, const double *fsum, int64_t n_cols, int64_t in_ld,
                                              const int32_t *sel, int64_t K, int variant, int alternative, int flags, double *out_p, double *out_t,
                                              double *out_df, double *out_fc, double *out_d, int64_t out_ld) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    if (!c->has_groups) return fail(c, ILLICO_ERR_NO_GROUPS, "illico_set_groups has not been called");
    if (variant != ILLICO_TT_WELCH && variant != ILLICO_TT_OVERESTIM_VAR) return fail(c, ILLICO_ERR_ARG, "unknown t-test variant code %d", variant);
    int rc = check_alternative(c, alternative);
    if (rc) return rc;
    const int64_t G = c->n_groups, W = n_cols;
    if (K < 2) return fail(c, ILLICO_ERR_ARG, "%lld groups selected: a pair needs two", (long long)K);
    if (!sel) return fail(c, ILLICO_ERR_ARG, "null sel");
    for (int64_t k = 0; k < K; ++k) {
        if (sel[k] < 0 || sel[k] >= G) return fail(c, ILLICO_ERR_ARG, "sel[%lld] = %d is no group id (0 .. %lld)", (long long)k, sel[k], (long long)G - 1);
        if (k && sel[k] <= sel[k - 1]) return fail(c, ILLICO_ERR_ARG, "sel must ascend strictly: sel[%lld] = %d after %d", (long long)k, sel[k], sel[k - 1]);
    }
    if (!sum || !sumsq) return fail(c, ILLICO_ERR_ARG, "null sum / sumsq plane");
    double *const outs[PT_N_OUT] = {out_p, out_t, out_df, out_fc, out_d};
    int n_out = 0;
    for (double *p : outs) n_out += p ? 1 : 0;
    if (!n_out) return fail(c, ILLICO_ERR_ARG, "all output planes are null: nothing to compute");
    if (W < 0 || in_ld < W || out_ld < W) return fail(c, ILLICO_ERR_ARG, "a pitch is smaller than the width (or the width is negative)");
    const int64_t n_tiles = (K + PT_GT - 1) / PT_GT, tile_pairs = n_tiles * (n_tiles + 1) / 2;
    if (tile_pairs > 65535) return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld groups selected: illico_pair_ttest_from_moments takes up to 2880", (long long)K);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = resolve_pending(c))) return rc; // a plane written under ILLICO_FLAG_DEFER is complete only after its leftover genes
    if (W == 0) return ILLICO_OK;
    const bool in_dev = flags & ILLICO_FLAG_INPUT_DEVICE, out_dev = flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const int n_in = fsum ? 3 : 2;
    const int64_t KK = K * K;

    int *d_sel;
    if ((rc = scratch(c, "pt_sel", (size_t)K, &d_sel))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_sel, sel, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    // column windows under the scratch cap (host planes are staged)
    StageWindows sw;
    if ((rc = plan_stage_windows(c, W, (in_dev ? 0 : (size_t)G * 8 * n_in) + (out_dev ? 0 : (size_t)KK * 8 * n_out), (int64_t)1 << 24, "pt_stage", &sw))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the selection came from pageable host memory)
    for (int64_t w0 = 0; w0 < W; w0 += sw.WW) {
        const int wn = (int)std::min<int64_t>(sw.WW, W - w0);
        PlaneStage st(c, sw.block, w0, wn);
        PtParams T;
        T.K = (int)K; T.W = wn; T.n_tiles = (int)n_tiles; T.variant = variant; T.alternative = alternative;
        T.counts = c->d_counts; T.sel = d_sel;
        T.S = st.in(sum, in_ld, G, in_dev); T.Q = st.in(sumsq, in_ld, G, in_dev); T.F = st.in(fsum, in_ld, G, in_dev);
        T.in_ld = st.pitch(in_ld, in_dev);
        for (int k = 0; k < PT_N_OUT; ++k) T.out[k] = st.out(outs[k], out_ld, KK, out_dev, false);
        T.out_ld = st.pitch(out_ld, out_dev);
        if (st.rc) return st.rc;
        const int64_t gx = (wn + PT_TILE - 1) / PT_TILE;
        KERNELCHK(c, k_pair_ttest, dim3((unsigned)gx, (unsigned)tile_pairs, (unsigned)pt_split(c, gx, tile_pairs)), dim3(PT_NT), 0, T);
        if ((rc = st.finish())) return rc;
    }
    return ILLICO_OK;
}
