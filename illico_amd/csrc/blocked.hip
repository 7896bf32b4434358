// illico_blocked_from_hists / illico_blocked_from_planes: Wilcoxon rank-sum tests spread over B blocks, the per-block tests combined on
// the device (kernels_blocked.h; include/illico_hip_blocked.h states the definition).  A translation unit of its
// own, a sibling of pairwise.hip and markers.hip: it shares the plane staging of plane_stage.h (through group_pass.h) and the histogram layouts of
// kernels_pairwise.h, and touches no other route.  Its kernels have no profiled kernel id: callers time the calls with stream events.
#include "group_pass.h"
#include "../../include/illico_hip_blocked.h"
#include "kernels_blocked.h"

namespace {

struct BlkCall {
    const int64_t *counts;
    int64_t G, B, W, ref;
    const double *sums;
    int64_t sums_ld;
    int flags, alternative;
    double *out[4]; // p, statistic, fold change, z
    int64_t out_ld;
    const int32_t *row_map = nullptr; // illico_blocked_from_planes
};
struct BlkSizes {
    std::vector<long long> n, ntot; // [G][B], [B]
};

// what both entry points refuse, before anything is written; the compound sizes and the block totals
int blk_check(illico_ctx *c, const BlkCall &a, BlkSizes *S) {
    int rc = check_alternative(c, a.alternative);
    if (rc) return rc;
    if (a.B < 1) return fail(c, ILLICO_ERR_ARG, "%lld blocks: a blocked test needs one", (long long)a.B);
    if (a.G < 1 || (a.ref >= 0 && a.G < 2)) return fail(c, ILLICO_ERR_ARG, "%lld groups: a test against %s needs %d", (long long)a.G, a.ref >= 0 ? "a reference group" : "the rest", a.ref >= 0 ? 2 : 1);
    if (a.ref < -1 || a.ref >= a.G) return fail(c, ILLICO_ERR_ARG, "reference %lld is no group id (0 .. %lld, or -1 for the rest)", (long long)a.ref, (long long)a.G - 1);
    if (a.G > 65535 || a.B > 65535 || a.G * a.B > 65535) return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld x %lld compound groups: the blocked tests take up to 65535", (long long)a.G, (long long)a.B);
    if (!a.counts) return fail(c, ILLICO_ERR_ARG, "null counts");
    if (a.W < 0 || a.out_ld < a.W) return fail(c, ILLICO_ERR_ARG, "out_ld smaller than n_cols (or n_cols negative)");
    if (a.sums && a.sums_ld < a.W) return fail(c, ILLICO_ERR_ARG, "sums_ld smaller than n_cols");
    if (a.W > (int64_t)1 << 21) return fail(c, ILLICO_ERR_OOM, "a window of %lld genes: pass narrower gene windows", (long long)a.W);
    S->n.resize((size_t)(a.G * a.B));
    S->ntot.assign((size_t)a.B, 0);
    for (int64_t k = 0; k < a.G * a.B; ++k) {
        if (a.counts[k] < 0) return fail(c, ILLICO_ERR_ARG, "counts[%lld] is negative", (long long)k);
        if (a.counts[k] >= 2097152ll) return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld cells of one group in one block: the integer rank and tie sums hold below 2097152 cells per test", (long long)a.counts[k]);
        S->n[k] = a.counts[k];
        S->ntot[k % a.B] += a.counts[k];
    }
    for (int64_t g = 0; g < a.G; ++g)
        for (int64_t b = 0; b < a.B; ++b) {
            const long long n_g = S->n[g * a.B + b], n_r = a.ref >= 0 ? S->n[a.ref * a.B + b] : S->ntot[b] - n_g;
            if (n_g > 0 && n_r > 0 && n_g + n_r >= 2097152ll)
                return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld cells in the test of group %lld in block %lld: the integer rank and tie sums hold below 2097152 cells per test",
                            n_g + n_r, (long long)g, (long long)b);
        }
    if (a.row_map)
        for (int64_t k = 0; k < a.G * a.B; ++k)
            if (a.row_map[k] < -1 || a.row_map[k] >= a.G)
                return fail(c, ILLICO_ERR_ARG, "row_map[%lld][%lld] = %d is no row of a plane set of %lld rows (or -1)", (long long)(k / a.G), (long long)(k % a.G), (int)a.row_map[k], (long long)a.G);
    return ILLICO_OK;
}

// one scratch block carved into 256-byte aligned arrays: sized in a first pass (base null), carved in a second
struct Carver {
    unsigned char *base = nullptr;
    size_t used = 0;
    template <typename T> T *take(size_t count) {
        const size_t at = used;
        used = (used + count * sizeof(T) + 255) & ~(size_t)255;
        return base ? (T *)(base + at) : nullptr;
    }
};

// The work arrays of one call, and the block a host caller's planes are staged in.  blk_plan runs twice over the same requests.
struct BlkDevice {
    long long *n, *ntot;
    int *row_map;
    u32 *T, *TOT;
    double *stot;
    unsigned char *stage;
};
void blk_plan(Carver &cv, const BlkCall &a, bool hists, size_t staged, BlkDevice *d) {
    const size_t GB = (size_t)(a.G * a.B), W = (size_t)a.W, tiles = (W + 63) / 64;
    d->n = cv.take<long long>(GB);
    d->ntot = cv.take<long long>((size_t)a.B);
    d->row_map = a.row_map ? cv.take<int>(GB) : nullptr;
    d->T = hists ? cv.take<u32>(GB * tiles * PW_TILE_WORDS) : nullptr;
    d->TOT = hists && a.ref < 0 ? cv.take<u32>((size_t)a.B * tiles * PW_TILE_WORDS) : nullptr;
    d->stot = a.sums && a.ref < 0 ? cv.take<double>((size_t)a.B * W) : nullptr;
    d->stage = staged ? cv.take<unsigned char>(staged) : nullptr;
}

int blk_run(illico_ctx *c, const BlkCall &a, const BlkSizes &S, const u32 *H, const u32 *gene_flags, const double *z, const double *U, int64_t in_ld) {
    const bool hists = H != nullptr, in_dev = a.flags & ILLICO_FLAG_INPUT_DEVICE, out_dev = a.flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const int64_t G = a.G, B = a.B, W = a.W, GB = G * B;
    const int wn = (int)W, tiles = (wn + 63) / 64;
    // one window; a host caller's planes are staged: the sums, the histograms and the gene flags or z and U, the outputs
    const size_t GBW = (size_t)GB * W;
    int n_out = 0;
    for (double *p : a.out) n_out += p ? 1 : 0;
    const size_t staged = (in_dev ? 0 : (a.sums ? GBW * 8 : 0) + (hists ? GBW * PW_RT * 4 + (size_t)W * 4 + 8 : GBW * 16)) + (out_dev ? 0 : (size_t)n_out * G * W * 8);
    BlkDevice d;
    Carver cv;
    blk_plan(cv, a, hists, staged, &d);
    if (cv.used > (size_t)std::max<int64_t>(c->scratch_bytes, 1))
        return fail(c, ILLICO_ERR_OOM, "%s needs %zu bytes of device scratch, the budget (\"scratch_bytes\") is %lld: pass a narrower gene window",
                    hists ? "illico_blocked_from_hists" : "illico_blocked_from_planes", cv.used, (long long)c->scratch_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = resolve_pending(c); // a plane written under ILLICO_FLAG_DEFER is complete only after its leftover genes
    if (rc) return rc;
    const size_t need = cv.used;
    cv = Carver{};
    if ((rc = scratch(c, "blk_work", need, &cv.base))) return rc;
    blk_plan(cv, a, hists, staged, &d);

    HIPCHK(c, hipMemcpyAsync(d.n, S.n.data(), (size_t)GB * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.ntot, S.ntot.data(), (size_t)B * 8, hipMemcpyHostToDevice, c->stream));
    if (a.row_map) HIPCHK(c, hipMemcpyAsync(d.row_map, a.row_map, (size_t)GB * 4, hipMemcpyHostToDevice, c->stream));
    BlkParams P{};
    P.n = d.n; P.ntot = d.ntot; P.row_map = d.row_map;
    P.G = (int)G; P.B = (int)B; P.W = wn; P.ref = (int)a.ref; P.alternative = a.alternative;
    P.tiles = tiles; P.tie_correct = (a.flags & ILLICO_FLAG_TIE_CORRECT) ? 1 : 0;
    PlaneStage sh(c, d.stage, 0, (int64_t)GBW * PW_RT); // the histograms [GB][W][PW_RT] go up as one row
    const u32 *d_H = sh.in(H, 0, 1, in_dev);
    if (sh.rc) return sh.rc;
    PlaneStage st(c, sh.rest(), 0, W);
    P.sums = st.in(a.sums, a.sums_ld, GB, in_dev); P.sums_ld = st.pitch(a.sums_ld, in_dev);
    P.gene_flags = st.in(gene_flags, W, 1, in_dev);
    P.z = st.in(z, in_ld, GB, in_dev); P.U = st.in(U, in_ld, GB, in_dev); P.in_ld = st.pitch(in_ld, in_dev);
    // from histograms a host caller's planes go up first: the columns of flagged genes come back as they were
    P.out_p = st.out(a.out[0], a.out_ld, G, out_dev, hists); P.out_u = st.out(a.out[1], a.out_ld, G, out_dev, hists);
    P.out_fc = st.out(a.out[2], a.out_ld, G, out_dev, hists); P.out_z = st.out(a.out[3], a.out_ld, G, out_dev, hists);
    P.out_ld = st.pitch(a.out_ld, out_dev);
    if (st.rc) return st.rc;
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the sizes and the staged arrays came from pageable host memory)

    if (d.stot) {
        KERNELCHK(c, k_blk_sum_totals, dim3((unsigned)((wn + 255) / 256), (unsigned)B), dim3(256), 0, P.sums, (long long)P.sums_ld, d.stot, (int)G, (int)B, wn);
        P.stot = d.stot;
    }
    if (hists) {
        KERNELCHK(c, k_pw_transpose<false>, dim3(tiles, (unsigned)GB), dim3(PW_NT), 0, const_cast<u32 *>(d_H), d.T, (const int *)nullptr, wn, tiles);
        P.T = d.T;
        if (d.TOT) {
            KERNELCHK(c, k_blk_block_totals, dim3(tiles, (unsigned)B), dim3(PW_NT), 0, (const u32 *)d.T, d.TOT, (int)G, (int)B, tiles);
            P.TOT = d.TOT;
        }
        KERNELCHK(c, k_blk_from_hists, dim3((unsigned)((G + PW_NT / 64 - 1) / (PW_NT / 64)), (unsigned)tiles), dim3(PW_NT), 0, P);
    } else {
        KERNELCHK(c, k_blk_from_planes, dim3((unsigned)((wn + 255) / 256), (unsigned)G), dim3(256), 0, P);
    }
    return st.finish();
}

} // namespace

extern "C" int illico_blocked_from_hists(illico_ctx *c, const uint32_t *H, const uint32_t *gene_flags, const int64_t *counts, int64_t n_groups, int64_t n_blocks,
                                         int64_t n_cols, int64_t ref, const double *sums, int64_t sums_ld, int flags, int alternative, double *out_p,
                                         double *out_u, double *out_fc, double *out_z, int64_t out_ld) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    const BlkCall a{counts, n_groups, n_blocks, n_cols, ref, sums, sums_ld, flags, alternative, {out_p, out_u, out_fc, out_z}, out_ld};
    BlkSizes S;
    int rc = blk_check(c, a, &S);
    if (rc) return rc;
    if (n_cols == 0) return ILLICO_OK;
    if (!H || !gene_flags || !out_p || !out_u || !out_fc || !out_z) return fail(c, ILLICO_ERR_ARG, "null H, gene_flags or output plane");
    return blk_run(c, a, S, H, gene_flags, nullptr, nullptr, 0);
}

extern "C" int illico_blocked_from_planes(illico_ctx *c, const double *z, const double *U, int64_t in_ld, const int32_t *row_map, const int64_t *counts,
                                          int64_t n_groups, int64_t n_blocks, int64_t n_cols, int64_t ref, const double *sums, int64_t sums_ld, int flags,
                                          int alternative, double *out_p, double *out_u, double *out_fc, double *out_z, int64_t out_ld) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    BlkCall a{counts, n_groups, n_blocks, n_cols, ref, sums, sums_ld, flags, alternative, {out_p, out_u, out_fc, out_z}, out_ld};
    if (!row_map) return fail(c, ILLICO_ERR_ARG, "null row_map");
    a.row_map = row_map;
    BlkSizes S;
    int rc = blk_check(c, a, &S);
    if (rc) return rc;
    if (in_ld < n_cols) return fail(c, ILLICO_ERR_ARG, "in_ld %lld smaller than the %lld columns", (long long)in_ld, (long long)n_cols);
    if (out_fc && !sums) return fail(c, ILLICO_ERR_ARG, "a fold-change plane needs the sums plane");
    if (n_cols == 0) return ILLICO_OK;
    if (!z || !U || !out_p || !out_u || !out_z) return fail(c, ILLICO_ERR_ARG, "null z, U or output plane");
    return blk_run(c, a, S, nullptr, nullptr, z, U, in_ld);
}
