// Dense-input drivers, templated on the value type: instantiated in dense_<type>.hip.
#pragma once
#include "keyed_driver.h"
#include "host_narrow.h"
#ifndef ILLICO_DENSE_U8_UNIT // the fused kernels on byte windows are instantiated in dense_u8.hip only
extern template int run_fused_ovo<uint8_t>(illico_ctx *, const FusedCall &, std::vector<u32> &);
#endif

// k_group_compact over one gene batch; pack = false: the padded dense layout (every key kept, sums only)
template <typename InT, typename KeyT>
static int launch_group_compact(illico_ctx *c, GroupCompactParams Q, int nb, int flags, bool pack) {
    constexpr int VEC = 16 / (int)sizeof(InT);
    const bool aligned = ((uintptr_t)Q.X % 16 == 0) && (Q.ld % VEC == 0) && (Q.col0 % VEC == 0);
    const bool lg = flags & ILLICO_FLAG_LOG1P;
    // few, long blocks (cluster-sized groups): a workgroup's chain of 64-row chunks is what the launch waits for -- tiles of 32 genes
    // (128-byte row pieces) put twice the workgroups on the same rows
    Q.blk_order = (c->no_compact_order || Q.nblk != c->pk_nblk) ? nullptr : c->d_pk_order; // (null unless the blocks' lengths differ much: set_groups)
    const bool narrow = !c->no_compact_narrow && c->pk_max_block_rows >= c->compact_narrow_rows && (long long)Q.nblk * ((nb + 63) / 64) < c->compact_narrow_wgs;
    const int tw = narrow ? 32 : 64;
    const dim3 grid(((Q.nseg + 7) & ~7) + Q.nblk, (nb + tw - 1) / tw);
    ProfScope ps(c, KID_GROUP_COMPACT);
    return dispatch_flags([&](auto vec, auto log1p, auto packed) {
        return dispatch_int<32, 64>(tw, [&](auto tile) {
            return launch_kernel(c, k_group_compact<InT, KeyT, decltype(vec)::value, decltype(log1p)::value, decltype(packed)::value, decltype(tile)::value>, grid,
                                 dim3(GCMP_NT), 0, Q);
        });
    }, aligned, lg, pack);
}

template <typename InT, typename KeyT>
static int run_ovo_packed(illico_ctx *c, const void *X, int64_t ld, int64_t col0, int nb, int N, KeyT *Xt, int64_t stride, int dtype, int flags,
                          long long *s2u, u64 *stie, double *ssum, std::vector<int> *redo /* genes of the batch the route left (groups above 1024 cells) */) {
    const int G = (int)c->n_groups, ref = (int)c->ref;
    const int64_t n_ref = c->h_counts[ref];
    const int nseg = gcmp_ref_segments(n_ref);
    int rc;
    unsigned char *nnz_block, *seg_sum_block;
    if ((rc = scratch(c, "packed_nnz", (size_t)nb * G * 2 + (size_t)nb * nseg * 2 + 64, &nnz_block))) return rc;
    u16 *nnz = (u16 *)nnz_block;
    u16 *seg_nnz = nnz + (((size_t)nb * G + 7) & ~(size_t)7);
    if ((rc = scratch(c, "packed_seg_sum", (size_t)nb * nseg * 8 + (size_t)nb * 4 + (size_t)nb * G * 4, &seg_sum_block))) return rc;
    double *seg_sum = (double *)seg_sum_block;
    u32 *route = (u32 *)(seg_sum + (size_t)nb * nseg);
    u32 *gofs = route + nb;
    HIPCHK(c, hipMemsetAsync(route, 0, (size_t)nb * 4, c->stream));
    const int is_log1p = (flags & ILLICO_FLAG_LOG1P) ? 1 : 0;
    u32 *run_n = nullptr;
    {
        GroupCompactParams Q;
        Q.X = X; Q.ld = ld; Q.col0 = col0; Q.ncols = nb; Q.perm = c->d_perm; Q.pos_ptr = c->d_posptr; Q.G = G; Q.ref = ref; Q.nseg = nseg;
        Q.blk_g0 = c->d_pk_blk; Q.blk_g1 = c->d_pk_blk + c->pk_nblk; Q.blk_out = c->d_pk_blk + 2 * c->pk_nblk; Q.nblk = c->pk_nblk; Q.ref_out = c->pk_ref_out;
        Q.Xt = Xt; Q.xt_stride = stride; Q.nnz = nnz; Q.gofs = gofs; Q.blk_cnt = nullptr; Q.out_sum = ssum; Q.seg_nnz = seg_nnz; Q.seg_sum = seg_sum;
        Q.cand_of = nullptr; Q.run_n = nullptr; Q.n_cand = c->pk_nbig;
        if (c->pk_nbig > 0 && c->max_nonref >= 65535) { // a (gene, group) run can outgrow the 16-bit lengths: exact ones beside them
            if ((rc = scratch(c, "packed_run_n", (size_t)nb * c->pk_nbig, &run_n))) return rc;
            Q.cand_of = c->d_pk_big + c->pk_nbig; Q.run_n = run_n;
        }
        if ((rc = launch_group_compact<InT, KeyT>(c, Q, nb, flags, true))) return rc;
    }
    bool parts = false;
    BigRunFn<KeyT> *big_fn = nullptr;
    u32 *run_cuts = nullptr;
    KeyT *big_tmp = nullptr; // groups with more cells than k_bucket_big_runs' LDS slots: a second key buffer, into which such runs are dealt
    if (c->pk_nbig > 0) { // runs of more than 256 non-zero keys are dealt into value buckets in place: the rank kernel walks them in pieces
        if ((rc = scratch(c, "packed_big_fn", (size_t)nb * c->pk_nbig, &big_fn))) return rc;
        ProfScope ps(c, KID_GROUP_COMPACT);
        int cap = (int)std::min<int64_t>(srt_cap<KeyT>(), (c->max_nonref + 63) & ~63ll); // (a run holds at most its group's cells)
        if (c->big_runs_cap > 0) cap = std::min(cap, std::max(c->big_runs_cap, 512) & ~63);
        if (c->max_nonref > cap && !c->no_big_runs_global && scratch(c, "packed_big_tmp", (size_t)nb * (size_t)stride, &big_tmp) != ILLICO_OK) big_tmp = nullptr;
        if (c->max_nonref > OCR_COOP_MIN && !c->no_coop_runs) { // runs long enough for the rank kernel to walk them with all its wavefronts: the bucket kernels leave cuts
            if ((rc = scratch(c, "packed_run_cuts", (size_t)nb * c->pk_nbig * OCR_CUTS, &run_cuts))) return rc;
        }
        if ((rc = launch_bucket_big_runs<KeyT>(c, (void *)Xt, big_tmp, (long long)stride, nnz, gofs, nb, G, cap, big_fn, route, c->max_nonref, run_n, run_cuts))) return rc;
    }
    {
        OvoCompactParams C;
        C.Xs = Xt; C.gene_stride = stride; C.nnz = nnz; C.gofs = gofs; C.ref_out = c->pk_ref_out; C.seg_nnz = seg_nnz; C.seg_sum = seg_sum;
        C.out_sum = ssum; C.nseg = nseg; C.route = route; C.ref_by_gofs = 0; C.gene_flags = nullptr; C.big_fn = big_fn; C.big_tmp = big_tmp;
        C.run_cuts = run_cuts; C.run_n = run_n;
        if ((rc = launch_packed_rank<KeyT, true>(c, C, nb, n_ref, s2u, stie, &parts))) return rc;
    }
    // What the packed kernels left.  The plain kernel's genes (route word 1: a tie-heavy reference column, the reference's segments moved
    // together) go to k_ovo_rank over the packed layout when its LDS holds the reference and the groups (<= 1024 keys); everything else --
    // the PARTS kernel's genes (a reason in the word's high bits: their segments lie where they were), a run beyond every bucket kernel
    // (route 2), or sizes k_ovo_rank does not take -- is handed back to the caller: transposition + the general sort route.
    const bool sort_fits = packed_leftovers_fit_sort_route<KeyT>(c);
    if (parts || !sort_fits || c->pk_nbig > 0) { // (runs above 256 keys: a gene with a value bucket above 256 keys leaves the rank kernel late, its segments unmoved)
        std::vector<u32> hr((size_t)nb);
        HIPCHK(c, hipMemcpyAsync(hr.data(), route, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bool any_sort = false;
        for (int j = 0; j < nb; ++j) {
            if (hr[j] && (!sort_fits || hr[j] > 255u || (hr[j] & 255u) == 2u)) redo->push_back(j);
            else if (hr[j]) any_sort = true;
        }
        if (c->debug_routes) { // why (PARTS: 1 = more parts than the launch has, 2 = a part beyond the slots, 3 = walks of overfull table words
            // would dominate, 5 = a run above 256 keys not dealt)
            int why[8] = {0, 0, 0, 0, 0, 0, 0, 0}, r2 = 0;
            for (int j = 0; j < nb; ++j) { if ((hr[j] & 255u) == 2u) ++r2; else if (hr[j]) ++why[(hr[j] >> 8) & 7u]; }
            fprintf(stderr, "[illico] packed OVO: %d genes, parts %d, left %zu to the general route (route 2: %d; reasons 0..5: %d %d %d %d %d %d)\n", nb, parts ? 1 : 0,
                    redo->size(), r2, why[0], why[1], why[2], why[3], why[4], why[5]);
        }
        if (!any_sort) return ILLICO_OK;
    }
    // the genes the packed kernel left (tie-heavy reference column, a group of more than 256 non-zeros): k_ovo_rank over the
    // packed layout; its workgroups return at once for every other gene
    OvoParams P;
    P.Xs = Xt; P.gene_stride = stride; P.pos_ptr = c->d_posptr; P.seg_ptr = nullptr; P.counts = c->d_counts;
    P.G = G; P.ref = ref; P.n_genes = nb; P.dt = dtype; P.is_log1p = is_log1p;
    P.ref_cap = 0; P.out_2u = s2u; P.out_tie = stie; P.out_sum = nullptr; P.nnz = nnz; P.gofs = gofs; P.only = route;
    return launch_ovo<KeyT>(c, P, n_ref, c->max_nonref, nullptr, nullptr, false);
}

template <typename InT, typename KeyT>
static int launch_transpose(illico_ctx *c, const void *X, int64_t ld, int64_t col0, int ncols, int N, KeyT *Xt, int64_t stride, u32 *flags,
                            int limit) { // flags[gene] != 0: a value that is no integer in [0, limit)
    ProfScope ps(c, KID_TRANSPOSE);
    dim3 grid((N + 63) / 64, (ncols + 63) / 64);
    constexpr int VEC = 16 / (int)sizeof(InT);
    const bool aligned = ((uintptr_t)X % 16 == 0) && (ld % VEC == 0) && (col0 % VEC == 0) && ((uintptr_t)Xt % 16 == 0) && (stride % 64 == 0);
    return launch_kernel(c, aligned ? k_transpose_permute_vec<InT, KeyT, VEC> : k_transpose_permute<InT, KeyT>, grid, dim3(256), 0, (const InT *)X, (long long)ld,
                         (long long)col0, ncols, (const int *)c->d_perm, N, Xt, (long long)stride, flags, limit);
}


// The first-pass OVO kernel for a cell width, with or without the z plane, under a memory policy (FUSED_MP_* bits, kernels_ovo_fused.h).
// What "fused_mem_policy" = 0 stands for: non-temporal loads and 8-byte stores, i.e. 6 (same-process A/B at C2, profiles/NOTES_r06.md:
// 1.815 -> 1.711 ms; the 16-byte write-through stores on top of it, 14, are worth 0.3 % more and did not clear the round's rule).
#define FUSED_DEFAULT_NT_LOADS 1
#define FUSED_DEFAULT_STORES 4
typedef void (*fused_main_fn)(FusedParams);
template <typename InT, int RT, int CB, bool Z> static fused_main_fn fused_ovo_main_z(int mp) {
    switch (mp) {
    case FUSED_MP_NT: return k_ovo_fused<InT, RT, false, CB, FUSED_U, false, Z, FUSED_MP_NT>;
    case FUSED_MP_ST16: return k_ovo_fused<InT, RT, false, CB, FUSED_U, false, Z, FUSED_MP_ST16>;
    case FUSED_MP_ST16 | FUSED_MP_NT: return k_ovo_fused<InT, RT, false, CB, FUSED_U, false, Z, FUSED_MP_ST16 | FUSED_MP_NT>;
    case FUSED_MP_ST16WT: return k_ovo_fused<InT, RT, false, CB, FUSED_U, false, Z, FUSED_MP_ST16WT>;
    case FUSED_MP_ST16WT | FUSED_MP_NT: return k_ovo_fused<InT, RT, false, CB, FUSED_U, false, Z, FUSED_MP_ST16WT | FUSED_MP_NT>;
    default: return k_ovo_fused<InT, RT, false, CB, FUSED_U, false, Z, 0>;
    }
}
template <typename InT, int RT, int CB> static fused_main_fn fused_ovo_main_fn(bool zp, int mp) {
    return zp ? fused_ovo_main_z<InT, RT, CB, true>(mp) : fused_ovo_main_z<InT, RT, CB, false>(mp);
}
// ---- the fused single pass: run_fused_ovo is the order of the steps below, each over one FusedState ----
// Writes final planes for every gene of the call it can take and sets h_flags[j] != 0 for the others (1 / 3: left to the two-pass
// routes; 2: done by the 256-value stage).  h_flags[nb] (also word nb of the deferred call's pinned flags) != 0: the 256-value stage
// was left to the host (k_wide_decide; only with max_gather > 0).  init_flags (host, [nb]): the 256-value stage ALONE, for the genes
// marked 1 there (run_leftovers: a narrow matrix of gathered columns).
struct FusedState {
    FusedParams P;     // the first pass's parameters; a 256-value stage copies them and swaps the tables (carve_ref_tables)
    int nb, tiles;     // tiles of 64 genes; nb64 = 64 * tiles: the cumulative tables are stored per tile
    size_t nb64;
    bool zp, ovr, wide_only; // zp: the z-score plane (the kernels' Z = true instantiations); wide_only: FusedCall::init_flags given
    u32 *skipw;        // one word: the 256-value stage is left to the host (k_wide_decide)
    dim3 main_grid;
};
// ref_TA [nb], ref_sum [nb], ref_cum [nb64][rt + 1] at the head of a table allocation: their bytes, and what follows them
static size_t ref_tables_bytes(const FusedState &S, int rt) { return S.nb64 * (rt + 1) * 4 + (size_t)S.nb * 8 * 2; }
static u32 *carve_ref_tables(FusedParams &P, unsigned char *v, const FusedState &S, int rt) {
    P.ref_TA = (u64 *)v; P.ref_sum = P.ref_TA + S.nb; P.ref_cum = (u32 *)(P.ref_sum + S.nb);
    return P.ref_cum + S.nb64 * (rt + 1);
}
static int fused_groups_per_wg(const illico_ctx *c, int tiles, bool ovr) {
    int gpw = c->fused_groups_per_wg;
    if (gpw <= 0) { // 8 groups per workgroup (two per wavefront) measured best at C2 (4: +2 %, 16: +1 %, 32: +3 %: shorter
        // workgroups leave a shorter tail at the end of the launch); keep >= ~2048 workgroups on smaller problems
        // OVR (k_ovr_group_hists): a workgroup ends by adding its share of the column histogram to the global one -- same-process A/B
        // at C4 (tools/ab.py): 8 / 16 / 32 groups per workgroup 2.601 / 2.589 / 2.614 ms; 4: +36 %
        gpw = ovr ? 16 : 8;
        while (gpw > 4 && (int64_t)tiles * ((c->n_groups + gpw - 1) / gpw) < 2048) gpw >>= 1;
    }
    return std::min(gpw, 128); // (k_ovr_group_hists packs a workgroup's cells into 16-bit fields: 128 x 255 < 2^16)
}
// The first pass's tables out of "fused_tables" with the route flags cleared (or set from init_flags), and everything of FusedParams that
// the call and the context give
static int carve_fused_tables(illico_ctx *c, const FusedCall &q, FusedState &S) {
    constexpr int RT = FUSED_RT;
    const OutPlanes &o = q.o;
    FusedParams &P = S.P;
    S.nb = q.nb; S.tiles = (q.nb + 63) / 64; S.nb64 = (size_t)S.tiles * 64;
    S.ovr = c->ref < 0; S.zp = o.z != nullptr; S.wide_only = q.init_flags != nullptr;
    unsigned char *v;
    int rc;
    if ((rc = scratch(c, "fused_tables", ref_tables_bytes(S, RT) + (size_t)q.nb * 4 + (size_t)q.nb * RT * 4 + 64, &v))) return rc;
    P.X = q.X; P.ld = q.ld; P.col0 = q.b0; P.ncols = q.nb; P.perm = c->d_perm; P.pos_ptr = c->d_posptr; P.counts = c->d_counts; P.gconst = c->d_gconst;
    P.G = (int)c->n_groups; P.ref = (int)c->ref;
    P.gene_flags = carve_ref_tables(P, v, S, RT);
    P.hist_all = P.gene_flags + q.nb; // OVR: the column histograms; OVO: the reference group's
    P.group_hist = P.wide_tiles = P.wide_bad = nullptr; P.hist_off = nullptr; P.hist_words = nullptr;
    P.tie_mode = S.ovr ? (c->fused_tie_sparse ? 2 : 1) : 0; // (the reference's float64 tie accumulation: dense order, or a CSR window's sparse order)
    P.hist_full = c->ovr_full_dump ? 1 : 0;
    P.hist_total = (long long)c->hist_words;
    P.wide_skip = S.skipw = P.hist_all + (size_t)q.nb * RT; // (inside the 64 spare bytes of the allocation)
    P.n_cells = c->n_cells;
    P.rows_per_wg = (int)std::max<int64_t>(1024, (c->n_cells + 31) / 32);
    P.use_continuity = (q.flags & ILLICO_FLAG_CONTINUITY) ? 1 : 0;
    P.tie_correct = (q.flags & ILLICO_FLAG_TIE_CORRECT) ? 1 : 0;
    P.alternative = q.alternative;
    P.out_p = o.p + q.col_off; P.out_u = o.u + q.col_off; P.out_fc = o.fc + q.col_off; P.out_ld = o.ld;
    P.out_z = o.z ? o.z + q.col_off : nullptr;
    P.groups_per_wg = fused_groups_per_wg(c, S.tiles, S.ovr);
    S.main_grid = dim3(S.tiles, ((int)c->n_groups + P.groups_per_wg - 1) / P.groups_per_wg);
    HIPCHK(c, hipMemsetAsync(S.skipw, 0, 4, c->stream));
    if (S.wide_only) HIPCHK(c, hipMemcpyAsync(P.gene_flags, q.init_flags, (size_t)S.nb * 4, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(P.gene_flags, 0, (size_t)S.nb * 4, c->stream));
    return ILLICO_OK;
}
// few, large groups (clusters of an atlas): the (group, gene) value histograms first, rows split over as many wavefronts as the launch
// needs, then the same integers from the histograms (kernels_group_hists.h) -- the fused kernels give a wavefront one GROUP at a time
static bool takes_group_hist_route(const illico_ctx *c, const FusedState &S) {
    const size_t gh_bytes = (size_t)c->n_groups * (size_t)S.tiles * FUSED_RT * 64 * 4;
    const bool gh_few = (int64_t)S.tiles * ((c->n_groups + 3) / 4) < c->group_hist_max_wgs && gh_bytes <= ((size_t)256 << 20);
    // ... and OVR with a group beyond the 16-bit cells of the one-pass form (an atlas whose control group has 66 667 cells): the histograms
    // here are 32 bits wide, one read of X instead of the two-pass form's two (2 000 000 x 1200 x 2000 groups: 6.9 ms)
    // (OVO with a ranked group beyond 65535 cells: the fused kernel's 32-bit multiplicities take 82 KB of LDS -- one workgroup, four wavefronts, per CU)
    const bool gh_ovr_big = c->max_nonref > 65535 && gh_bytes <= ((size_t)1 << 30);
    // ... and groups of very different sizes (clusters from fifty to tens of thousands of cells): the largest group alone is more than twice
    // an average wavefront's share of the fused launch -- its wavefront is what that launch waits for (100 000 cells x 8192 genes x 30
    // clusters: 0.84 ms with equal groups, 1.56 with a Dirichlet draw of sizes)
    const bool gh_ragged = gh_bytes <= ((size_t)256 << 20) && c->max_nonref > 2 * (c->n_cells * (int64_t)S.tiles / 4096) && c->max_nonref >= 4096;
    return !S.wide_only && !c->no_group_hist_route && (gh_few || gh_ovr_big || gh_ragged) && c->n_cells >= c->group_hist_min_cells && c->n_cells <= (1ll << 21);
}
// OVR on device-resident input, and the histogram route: which genes are count-valued at all is found on the device (the OVO pass has
// k_fused_ref, which reads every reference row first)
template <typename InT> static int fused_probe(illico_ctx *c, const FusedState &S) {
    ProfScope ps(c, KID_FUSED_REF);
    return launch_kernel(c, k_fused_probe<InT, FUSED_RT>, dim3(S.tiles), dim3(FUSED_PROBE_NT), 0, S.P);
}
// k_fused_tables_all over the first pass's tables (inside the caller's KID_FUSED_REF scope)
static int launch_fused_tables_all(illico_ctx *c, const FusedState &S) {
    return launch_kernel(c, k_fused_tables_all<FUSED_RT>, dim3((S.nb + 255) / 256), dim3(256), 0, S.P);
}
template <typename InT> static int fused_hist_route(illico_ctx *c, const FusedState &S) {
    constexpr int RT = FUSED_RT;
    const FusedParams &P = S.P;
    const int tiles = S.tiles;
    u32 *H;
    int rc;
    const size_t h_bytes = (size_t)c->n_groups * tiles * RT * 64 * 4;
    if ((rc = scratch(c, "group_value_hists", h_bytes / 4, &H))) return rc;
    HIPCHK(c, hipMemsetAsync(H, 0, h_bytes, c->stream));
    constexpr int NWH = GH_NT / 64;
    // positions per wavefront: ~2048 workgroups, at most 4096 positions (16-bit cells)
    int wave_rows = (int)std::min<int64_t>(4096, std::max<int64_t>(256, (c->n_cells * tiles / (2048 * NWH) + 31) & ~31ll));
    const int chunks = (int)((c->n_cells + (int64_t)NWH * wave_rows - 1) / ((int64_t)NWH * wave_rows));
    {
        ProfScope ps(c, KID_GROUP_HISTS);
        KERNELCHK(c, k_group_value_hists<InT, RT>, dim3(tiles, chunks), dim3(GH_NT), 0, P, H, wave_rows);
    }
    ProfScope ps(c, KID_FUSED_REF);
    if (S.ovr) {
        HIPCHK(c, hipMemsetAsync(P.hist_all, 0, (size_t)S.nb * RT * 4, c->stream));
        KERNELCHK(c, k_group_hists_to_column<RT, true>, dim3(tiles, ((int)c->n_groups + 63) / 64), dim3(256), 0, P, (const u32 *)H);
    } else KERNELCHK(c, k_group_hists_to_column<RT, false>, dim3(tiles), dim3(256), 0, P, (const u32 *)H);
    if ((rc = launch_fused_tables_all(c, S))) return rc;
    const dim3 ge(tiles, ((int)c->n_groups + 3) / 4);
    auto emit = S.ovr ? (S.zp ? k_emit_from_group_hists<RT, true, true> : k_emit_from_group_hists<RT, true>)
                      : (S.zp ? k_emit_from_group_hists<RT, false, true> : k_emit_from_group_hists<RT, false>);
    return launch_kernel(c, emit, ge, dim3(256), 0, P, (const u32 *)H);
}
// OVO: the reference group's tables
template <typename InT> static int fused_ovo_reference(illico_ctx *c, FusedState &S) {
    constexpr int RT = FUSED_RT;
    FusedParams &P = S.P;
    ProfScope ps(c, KID_FUSED_REF);
    if (S.tiles >= 100) { // one 1024-thread workgroup per tile builds the tables (C2: 125 tiles, 0.074 ms)
        return launch_kernel(c, S.zp ? k_fused_ref<InT, RT, false, true> : k_fused_ref<InT, RT>, dim3(S.tiles), dim3(FUSED_REF_NT), fused_ref_lds_bytes(RT), P);
    } else { // few tiles (a C5 shard: 59): the reference rows split over (tiles, row chunks), then one thread per gene for
        // the tables -- 0.20 -> 0.11 ms there, 0.074 -> 0.083 ms at C2, hence the switch
        HIPCHK(c, hipMemsetAsync(P.hist_all, 0, (size_t)S.nb * RT * 4, c->stream));
        const int64_t n_ref = c->h_counts[c->ref];
        const int want_chunks = std::max(1, 768 / std::max(S.tiles, 1)); // enough workgroups for 256 CUs, few enough flushes
        P.rows_per_wg = (int)std::max<int64_t>(FUSED_REF_ROWS, (n_ref + want_chunks - 1) / want_chunks); // (kept for the passes that follow)
        const int chunks = (int)std::max<int64_t>(1, (n_ref + P.rows_per_wg - 1) / P.rows_per_wg);
        KERNELCHK(c, k_fused_ref_hist<InT, RT>, dim3(S.tiles, chunks), dim3(FUSED_NT), 0, P);
        return launch_fused_tables_all(c, S);
    }
}
template <typename InT> static int fused_ovo_main(illico_ctx *c, const FusedState &S) {
    constexpr int RT = FUSED_RT;
    const FusedParams &P = S.P;
    // memory policy of the pass ("fused_mem_policy"): 16-byte stores only where every pair of a plane in use is 16-byte aligned.
    // Left to the engine, the loads are non-temporal where a wavefront's row segment is whole 128-byte lines (4- and 8-byte
    // values); a byte window's 64-byte segments share each line between two tiles, so it is not read once (and not measured).
    const int pol = c->fused_mem_policy;
    int mp = ((pol & 3) == 2 || ((pol & 3) == 0 && FUSED_DEFAULT_NT_LOADS && sizeof(InT) >= 4)) ? FUSED_MP_NT : 0;
    const int st = (pol & 12) ? (pol & 12) : FUSED_DEFAULT_STORES;
    auto aligned16 = [](const double *q) { return ((uintptr_t)q & 15) == 0; };
    if (st != 4 && (P.out_ld & 1) == 0 && aligned16(P.out_p) && aligned16(P.out_u) && aligned16(P.out_fc) && (!S.zp || aligned16(P.out_z)))
        mp |= st == 12 ? FUSED_MP_ST16WT : FUSED_MP_ST16;
    ProfScope ps(c, (mp & (FUSED_MP_ST16 | FUSED_MP_ST16WT)) ? KID_OVO_FUSED_ST16 : KID_OVO_FUSED); // (a name of its own: tests tell the forms apart)
    // 8-bit running multiplicities: 34 KB of LDS per workgroup instead of 50 KB; clusters of more than 65535 cells: 32-bit ones (82 KB:
    // one workgroup per CU)
    return dispatch_int<8, 16, 32>(c->max_nonref <= 255 ? 8 : c->max_nonref <= 65535 ? 16 : 32, [&](auto cb) {
        constexpr int CB = decltype(cb)::value;
        return launch_kernel(c, fused_ovo_main_fn<InT, RT, CB>(S.zp, mp), S.main_grid, dim3(FUSED_NT), fused_main_lds_bytes<RT, false, CB>(), P);
    });
}
// is the 256-value stage left to the host?  (decided on the device, after the first pass: nothing waits for it here)
static int wide_decide(illico_ctx *c, const FusedCall &q, const FusedState &S) {
    if (S.wide_only || q.max_gather <= 0 || c->no_wide_gather) return ILLICO_OK;
    ProfScope ps(c, KID_FUSED_REF);
    return launch_kernel(c, k_wide_decide, dim3(1), dim3(1024), 0, (const u32 *)S.P.gene_flags, S.nb, (int)std::min<int64_t>(q.max_gather, 0x7FFFFFFF), S.skipw);
}
// A 256-value kernel as resident workgroups, per_cu of them on every CU, working through the tiles that Q.wide_tiles lists
static int launch_resident_wide(illico_ctx *c, fused_main_fn kern, size_t lds, int per_cu, const FusedParams &Q) {
    ProfScope ps(c, KID_OVO_FUSED_WIDE);
    int n_cu = 256;
    hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
    return launch_kernel(c, kern, dim3((unsigned)std::max(per_cu * n_cu, 1)), dim3(FUSED_NT), lds, Q);
}
// OVO second pass, 256-value tables, over the tiles that hold genes the first pass flagged (counts of 64 .. 255: highly
// expressed genes of real count matrices): same kernels, one workgroup per CU (130 KB of LDS), resident workgroups
// working through the list of such tiles that k_fused_ref<WIDE> builds on the device -- an empty list costs two
// near-empty launches (0.005 ms at C2).  Flags after it: 1 = the host's two-pass routes, 0 / 2 = done.
template <typename InT> static int fused_ovo_wide_stage(illico_ctx *c, const FusedCall &q, const FusedState &S) {
    constexpr int WRT = FUSED_WIDE_RT;
    if (c->max_nonref > 255 || c->no_fused_wide) return ILLICO_OK;
    unsigned char *v;
    int rc;
    if ((rc = wide_decide(c, q, S))) return rc;
    if ((rc = scratch(c, "fused_tables_wide", ref_tables_bytes(S, WRT) + (size_t)(S.tiles + 1) * 4 + 64, &v))) return rc;
    FusedParams Q = S.P;
    Q.wide_tiles = carve_ref_tables(Q, v, S, WRT);
    HIPCHK(c, hipMemsetAsync(Q.wide_tiles, 0, 4, c->stream));
    {
        ProfScope ps(c, KID_FUSED_REF);
        KERNELCHK(c, S.zp ? k_fused_ref<InT, WRT, true, true> : k_fused_ref<InT, WRT, true>, dim3(S.tiles), dim3(FUSED_REF_NT), fused_ref_lds_bytes(WRT), Q);
    }
    fused_main_fn kern = S.zp ? k_ovo_fused<InT, WRT, false, 8, FUSED_U, true, true> : k_ovo_fused<InT, WRT, false, 8, FUSED_U, true>;
    return launch_resident_wide(c, kern, fused_main_lds_bytes<WRT, false, 8>(), 1, Q);
}
// OVR, one pass over X: per-(group, gene) histograms that fit the scratch cap (64 or 128 bytes each), then the rank sums from them.
// `*done` stays false where the form does not apply (fused_ovr_two_pass follows).
template <typename InT> static int fused_ovr_one_pass(illico_ctx *c, FusedState &S, bool *done) {
    constexpr int RT = FUSED_RT;
    FusedParams &P = S.P;
    const int tiles = S.tiles;
    int rc;
    // 8-bit cells when no group is larger than 255 cells, else the width per group (0): a few large groups do not double
    // the histogram bytes of all the small ones
    const int cbits = c->max_nonref <= 255 ? 8 : 0;
    const size_t hist_bytes = cbits ? (size_t)c->n_groups * tiles * (RT * cbits / 32) * 64 * 4 : (size_t)c->hist_words * tiles * 64 * 4;
    if (c->no_ovr_one_pass || c->max_nonref > 65535 || hist_bytes > (size_t)c->scratch_bytes) return ILLICO_OK; // (16-bit cells: no group beyond 65535 cells)
    *done = true;
    if ((rc = scratch(c, "group_hist", hist_bytes / 4, &P.group_hist))) return rc;
    if ((rc = scratch(c, "group_hist_words", (size_t)c->n_groups * tiles, &P.hist_words))) return rc;
    P.hist_off = c->d_hist_off;
    {
        ProfScope ps(c, KID_OVR_FUSED);
        KERNELCHK(c, cbits == 8 ? k_ovr_group_hists<InT, RT, 8> : k_ovr_group_hists<InT, RT, 0>, S.main_grid, dim3(FUSED_NT), 0, P);
    }
    ProfScope ps(c, KID_FUSED_REF);
    if ((rc = launch_fused_tables_all(c, S))) return rc;
    // the rank-sum kernel keeps a 64-entry table per lane in registers: more groups per workgroup amortise its fill
    FusedParams P2 = P;
    P2.groups_per_wg = c->ovr_hist_groups_per_wg > 0 ? c->ovr_hist_groups_per_wg : 32;
    while (P2.groups_per_wg > 8 && (int64_t)tiles * ((c->n_groups + P2.groups_per_wg - 1) / P2.groups_per_wg) < 2048) P2.groups_per_wg >>= 1;
    const dim3 grid2(tiles, ((int)c->n_groups + P2.groups_per_wg - 1) / P2.groups_per_wg);
    return dispatch_flags([&](auto cells8, auto np3, auto zp) { // (np3: s < 2^24, three byte planes)
        return launch_kernel(c, k_ovr_from_hists<RT, decltype(cells8)::value ? 8 : 0, decltype(np3)::value ? 3 : 4, decltype(zp)::value>, grid2, dim3(FUSED_NT), 0, P2);
    }, cbits == 8, c->n_cells < (1ll << 23), S.zp);
}
// OVR, two passes over X: the column histograms and their tables, then k_ovo_fused<OVR>
template <typename InT> static int fused_ovr_two_pass(illico_ctx *c, const FusedState &S) {
    constexpr int RT = FUSED_RT;
    const FusedParams &P = S.P;
    {
        ProfScope ps(c, KID_FUSED_REF);
        const int chunks = (int)((c->n_cells + P.rows_per_wg - 1) / P.rows_per_wg);
        KERNELCHK(c, k_fused_hist_all<InT, RT>, dim3(S.tiles, chunks), dim3(FUSED_NT), fused_ref_lds_bytes(RT), P);
        int rc = launch_fused_tables_all(c, S);
        if (rc) return rc;
    }
    ProfScope ps(c, KID_OVR_FUSED);
    return launch_kernel(c, S.zp ? k_ovo_fused<InT, RT, true, 16, FUSED_U, false, true> : k_ovo_fused<InT, RT, true, 16>, S.main_grid, dim3(FUSED_NT),
                         fused_main_lds_bytes<RT, true, 16>(), P);
}
template <typename InT> static int fused_ovr_first_pass(illico_ctx *c, FusedState &S) {
    int rc;
    bool done = false;
    HIPCHK(c, hipMemsetAsync(S.P.hist_all, 0, (size_t)S.nb * FUSED_RT * 4, c->stream));
    if ((rc = fused_ovr_one_pass<InT>(c, S, &done)) || done) return rc;
    return fused_ovr_two_pass<InT>(c, S);
}
// OVR second stage, 256-value tables, over the tiles that hold genes the 64-value pass flagged (counts of 64 .. 255): the
// two-pass form -- column histograms of those tiles (k_fused_hist_all<WIDE>: every row, so a candidate is known to fit),
// tables, then k_ovo_fused<OVR, WIDE> with resident workgroups over the listed tiles.  No per-group state: 67 KB of LDS.
// C4 shape with gene means up to 40: 97 ms (those genes through the general sort route) -> see DESIGN.md.
template <typename InT> static int fused_ovr_wide_stage(illico_ctx *c, const FusedCall &q, const FusedState &S) {
    constexpr int WRT = FUSED_WIDE_RT;
    if (c->no_fused_wide) return ILLICO_OK;
    const int nb = S.nb, tiles = S.tiles;
    unsigned char *v;
    int rc;
    if ((rc = wide_decide(c, q, S))) return rc;
    if ((rc = scratch(c, "fused_tables_wide", ref_tables_bytes(S, WRT) + (size_t)nb * WRT * 4 + (size_t)(nb + tiles) * 4 + (size_t)(tiles + 1) * 4 + 64, &v))) return rc;
    FusedParams Q = S.P;
    Q.hist_all = carve_ref_tables(Q, v, S, WRT);
    Q.wide_bad = Q.hist_all + (size_t)nb * WRT;          // [nb] + [tiles] tile marks
    Q.wide_tiles = Q.wide_bad + nb + tiles;
    HIPCHK(c, hipMemsetAsync(Q.hist_all, 0, ((size_t)nb * WRT + nb + tiles + 1) * 4, c->stream));
    {
        ProfScope ps(c, KID_FUSED_REF);
        const int chunks = (int)((c->n_cells + S.P.rows_per_wg - 1) / S.P.rows_per_wg);
        KERNELCHK(c, k_fused_hist_all<InT, WRT, true>, dim3(tiles, chunks), dim3(FUSED_NT), fused_ref_lds_bytes(WRT), Q);
        KERNELCHK(c, k_fused_tables_all<WRT, true>, dim3((nb + 255) / 256), dim3(256), 0, Q);
    }
    fused_main_fn kern = S.zp ? k_ovo_fused<InT, WRT, true, 16, FUSED_U, true, true> : k_ovo_fused<InT, WRT, true, 16, FUSED_U, true>;
    return launch_resident_wide(c, kern, fused_main_lds_bytes<WRT, true, 16>(), 2, Q);
}
// The route flags and the skip word, through a pinned staging buffer (a pageable destination makes the copy a blocking, staged one).
// Deferred: the copies are enqueued into the slot the caller named, the caller's event marks them, nobody waits here (resolve_pending does).
static int return_fused_flags(illico_ctx *c, const FusedCall &q, const FusedState &S, std::vector<u32> &h_flags) {
    const size_t nb = (size_t)S.nb;
    int rc, slot = q.defer_slot;
    void *pin;
    if (slot >= 0) {
        if ((rc = reserve_deferred_slot(c, nb * 4 + 4, &slot, &pin))) return rc; // (the slot the caller named, which posts the call)
    } else {
        if ((rc = ensure_pinned(c, nb * 4 + 4))) return rc;
        pin = c->pinned;
    }
    HIPCHK(c, hipMemcpyAsync(pin, S.P.gene_flags, nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync((u32 *)pin + nb, S.skipw, 4, hipMemcpyDeviceToHost, c->stream));
    if (q.defer_slot >= 0) return ILLICO_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    h_flags.assign((const u32 *)pin, (const u32 *)pin + nb + 1);
    return ILLICO_OK;
}
template <typename InT> int run_fused_ovo(illico_ctx *c, const FusedCall &q, std::vector<u32> &h_flags) {
    FusedState S;
    int rc;
    if ((rc = carve_fused_tables(c, q, S))) return rc;
    const bool hist_route = takes_group_hist_route(c, S), first_pass = !hist_route && !S.wide_only;
    if ((q.probe || hist_route) && !S.wide_only && (rc = fused_probe<InT>(c, S))) return rc;
    if (hist_route && (rc = fused_hist_route<InT>(c, S))) return rc;
    if (S.ovr) {
        if (first_pass && (rc = fused_ovr_first_pass<InT>(c, S))) return rc;
        if ((rc = fused_ovr_wide_stage<InT>(c, q, S))) return rc;
    } else if (!hist_route) {
        if (first_pass && ((rc = fused_ovo_reference<InT>(c, S)) || (rc = fused_ovo_main<InT>(c, S)))) return rc;
        if ((rc = fused_ovo_wide_stage<InT>(c, q, S))) return rc;
    }
    return return_fused_flags(c, q, S, h_flags);
}
// Of 64k evenly spaced cells of a HOST matrix window: is it count-valued at all?  (The fused route over a host matrix copies
// the window up; on normalised data that copy would be made twice, once for nothing.)
template <typename InT> static bool host_window_is_count_valued(const InT *X, int64_t ld, int64_t col_lb, int64_t N, int64_t W, bool *light_tails = nullptr) {
    const int64_t n_samples = std::min<int64_t>(N * W, 1 << 16);
    int64_t bad = 0, big = 0;
    for (int64_t i = 0; i < n_samples; ++i) {
        const int64_t k = (int64_t)((double)i * (double)(N * W) / (double)n_samples);
        const int64_t r = k / W, j = k - r * W;
        const InT v = X[r * ld + col_lb + j];
        if (!(v >= (InT)0 && v < (InT)(1 << 24) && (InT)(int)v == v)) ++bad;
        else if (v >= (InT)255) ++big;
    }
    // light tails: (nearly) no sampled cell of 255 or more -- the byte windows (ByteWindows) then hold (nearly) every
    // gene; a heavy-tailed count matrix keeps the float32 windows, whose flagged genes are gathered on the device instead of going up again
    if (light_tails) *light_tails = (double)(bad + big) * 2048.0 <= (double)n_samples;
    return (double)bad <= 0.02 * (double)n_samples;
}
// ---- host-resident dense input: a three-stage pipeline over column windows ----------------------------------------------
// A pageable 2-D copy of the whole window (what this path did before) moves 9.6 GB at ~43 GB/s through the driver's own
// staging and nothing overlaps it.  Here: (1) HS_THREADS host threads copy window k + 1's row pieces out of the caller's
// matrix into a PINNED slot, (2) the copy stream moves window k's slot to the device at the link's rate, (3) the context's
// stream runs the fused pass on window k - 1 -- all three at once, three slots deep.  Slot j serves the windows k = j mod 3: its
// pinned half is free once its upload has completed, its device half once the pass over it has (events both ways).
#define HS_THREADS 12
#define HS_THREADS_NARROW 16 // (the byte pipeline: the fill -- 9.6 GB of host reads at C2 -- is what must keep up with a quarter-size upload)
struct HostLeftovers { // the flagged genes' columns, gathered on the device while their window is still there
    void *xl = nullptr;    // [N][cap] values
    int64_t cap = 0, n = 0;
    int *d_dst = nullptr;  // [n] output column (relative to the call's planes) of gathered column j
};
// What the pipeline's two forms differ in: the cell type and row pitch of a slot, the fill of one row, the default number of fill
// threads, how "gene_batch" bounds a window, and what becomes of the genes a window's pass flagged.
template <typename InT> struct OwnTypeWindows { // windows in the matrix's own type
    typedef InT Cell;
    static constexpr int fill_threads = HS_THREADS;
    static constexpr int pad = 1; // a window's row pitch, and "gene_batch" as a window's width, are rounded up to it
    static const char *name() { return "own-type"; }
    static void fill_row(const InT *src, InT *dst, int64_t wn, int64_t) { memcpy(dst, src, (size_t)wn * sizeof(InT)); }
    HostLeftovers left;
    int *d_src = nullptr; // [left.cap] column of its window of gathered column j

    // room for the genes the fused pass flags (a count matrix: few): they are gathered out of their window while it is on the device,
    // so that no window travels twice
    int prepare(illico_ctx *c, HostStage *hs, int64_t N, int64_t W) {
        int rc;
        left.cap = c->no_leftover_gather ? 0 : std::min<int64_t>((W / 4 + 63) & ~63ll, (int64_t)((size_t)c->scratch_bytes / 4 / ((size_t)N * sizeof(InT))) & ~63ll);
        if (left.cap < 64) { left.cap = 0; return ILLICO_OK; }
        InT *xl;
        if ((rc = scratch(c, "xleft", (size_t)N * (size_t)left.cap, &xl))) return rc;
        left.xl = xl;
        HIPCHK(c, hipMemsetAsync(left.xl, 0, (size_t)N * (size_t)left.cap * sizeof(InT), c->stream));
        if ((rc = scratch(c, "xleft_cols", (size_t)left.cap * 2, &d_src))) return rc;
        left.d_dst = d_src + left.cap;
        if (hs->lists_ints < (size_t)left.cap * 2) {
            if (hs->lists) hipHostFree(hs->lists);
            hs->lists = nullptr; hs->lists_ints = 0;
            HIPCHK(c, hipHostMalloc((void **)&hs->lists, (size_t)left.cap * 8, hipHostMallocDefault));
            hs->lists_ints = (size_t)left.cap * 2;
        }
        return ILLICO_OK;
    }
    // this window's flagged genes: out of the device window into the leftover matrix (else: column runs, uploaded again later)
    int after_pass(illico_ctx *c, HostStage *hs, const InT *win, int64_t N, int64_t wn, int64_t w0, int64_t col_lb, const std::vector<u32> &hf,
                   std::vector<std::pair<int64_t, int64_t>> &runs) {
        int cnt = 0, rc = ILLICO_OK;
        for (int64_t q = 0; q < wn; ++q) cnt += (hf[q] == 1u || hf[q] == 3u) ? 1 : 0;
        if (!cnt) return ILLICO_OK;
        if (left.n + cnt > left.cap) { flagged_runs(hf.data(), wn, w0, runs); return ILLICO_OK; }
        int *ls = hs->lists + left.n, *ld_ = hs->lists + left.cap + left.n;
        int e = 0;
        for (int64_t q = 0; q < wn; ++q)
            if (hf[q] == 1u || hf[q] == 3u) { ls[e] = (int)q; ld_[e] = (int)(w0 - col_lb + q); ++e; }
        if (hipMemcpyAsync(d_src + left.n, ls, (size_t)cnt * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(left.d_dst + left.n, ld_, (size_t)cnt * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            rc = fail(c, ILLICO_ERR_HIP, "uploading a column list failed");
        if (!rc) {
            ProfScope ps(c, KID_GATHER_COLS);
            rc = launch_kernel(c, k_gather_columns<InT>, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, win, (long long)wn, (int)N, (const int *)(d_src + left.n), cnt, cnt,
                               (InT *)left.xl, (long long)left.cap, (long long)left.n);
        }
        left.n += cnt;
        return rc;
    }
};
// BYTE windows (host_narrow.h): a count matrix in host memory goes up as a quarter of its float32 bytes.  The threads that fill a
// pinned slot convert as they copy (cell = the value when it is an integer in [0, 255), else 255); the copy stream moves N x pitch
// bytes (pitch: the window's width rounded up to 64, the pad zeroed); the context's stream runs the fused kernels on the byte window
// -- k_ovo_fused<uint8_t> / k_ovr_group_hists<uint8_t>, the forms count-valued CSR windows take, 64-value pass and 256-value second
// pass alike.  A gene they flag (a 255 cell: a value of 255 or more, a fraction, a negative) comes back as a column run and goes up
// again, in its own type, through the two-pass routes (run_dense_twopass on the host matrix): few genes on count data.  Windows are
// four times as wide as the float32 pipeline's for the same pinned memory: each row piece is a longer contiguous read of the
// caller's matrix.
template <typename InT> struct ByteWindows {
    typedef uint8_t Cell;
    static constexpr int fill_threads = HS_THREADS_NARROW;
    static constexpr int pad = 64;
    static const char *name() { return "byte"; }
    static void fill_row(const InT *src, uint8_t *dst, int64_t wn, int64_t pitch) {
        narrow_cells<InT>(src, dst, wn);
        if (pitch > wn) memset(dst + wn, 0, (size_t)(pitch - wn));
    }
    int prepare(illico_ctx *, HostStage *, int64_t, int64_t) { return ILLICO_OK; }
    int after_pass(illico_ctx *, HostStage *, const uint8_t *, int64_t, int64_t wn, int64_t w0, int64_t, const std::vector<u32> &hf,
                   std::vector<std::pair<int64_t, int64_t>> &runs) {
        flagged_runs(hf.data(), wn, w0, runs); // these genes go up again in the matrix's own type (the two-pass routes)
        return ILLICO_OK;
    }
};
struct HostWindowQueue { // what the producer and the consumer of host_windows_pipeline share
    int64_t N, col_lb, col_ub, wmax, n_win;
    std::mutex mu;
    std::condition_variable cv;
    int64_t ready = 0, consumed = 0; // windows whose upload is enqueued / whose pass is
    int err = 0;                     // a failure on either side: both stop
    double t_fill = 0.0, t_wait = 0.0; // (ILLICO_HS_DEBUG=1 prints them: seconds the producer spent filling slots / the consumer waiting for one)
    int64_t w0(int64_t k) const { return col_lb + k * wmax; }
    int64_t wn(int64_t k) const { return std::min<int64_t>(wmax, col_ub - w0(k)); }
};
// the copy stream, the events and the pinned halves of the slots
static int prepare_host_stage(illico_ctx *c, HostStage *hs, size_t slot_bytes) {
    if (!hs->copy) HIPCHK(c, hipStreamCreateWithFlags(&hs->copy, hipStreamNonBlocking));
    for (int j = 0; j < HS_SLOTS; ++j) {
        if (!hs->up[j]) HIPCHK(c, hipEventCreateWithFlags(&hs->up[j], hipEventDisableTiming));
        if (!hs->done[j]) HIPCHK(c, hipEventCreateWithFlags(&hs->done[j], hipEventDisableTiming));
    }
    if (hs->pin_bytes < slot_bytes) {
        for (int j = 0; j < HS_SLOTS; ++j) { if (hs->pin[j]) hipHostFree(hs->pin[j]); hs->pin[j] = nullptr; }
        hs->pin_bytes = 0;
        for (int j = 0; j < HS_SLOTS; ++j) HIPCHK(c, hipHostMalloc(&hs->pin[j], slot_bytes, hipHostMallocDefault));
        hs->pin_bytes = slot_bytes;
    }
    return ILLICO_OK;
}
// producer: fills and uploads the slots; the calling thread consumes them
template <typename InT, typename Pol> static void produce_host_windows(illico_ctx *c, HostStage *hs, HostWindowQueue &Q, const InT *X, int64_t ld, int x_node, typename Pol::Cell *const *dev) {
    typedef typename Pol::Cell Cell;
    const int64_t N = Q.N;
    hipSetDevice(c->device);
    numa_confine_this_thread(x_node); // (the fill threads started below inherit the mask; this thread ends with the call)
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(c->host_fill_threads > 0 ? c->host_fill_threads : Pol::fill_threads, N / 4096 + 1));
    for (int64_t k = 0; k < Q.n_win; ++k) {
        const int j = (int)(k % HS_SLOTS);
        const int64_t w0 = Q.w0(k), wn = Q.wn(k), pitch = (wn + Pol::pad - 1) & ~(int64_t)(Pol::pad - 1);
        if (k >= HS_SLOTS) { // slot j still belongs to window k - HS_SLOTS until the pass over it is done
            std::unique_lock<std::mutex> lk(Q.mu);
            Q.cv.wait(lk, [&] { return Q.consumed > k - HS_SLOTS || Q.err; });
            if (Q.err) return;
            lk.unlock();
            if (hipEventSynchronize(hs->done[j]) != hipSuccess) { std::lock_guard<std::mutex> g(Q.mu); Q.err = 1; Q.cv.notify_all(); return; }
        }
        Cell *dst = (Cell *)hs->pin[j];
        const auto t_a = std::chrono::steady_clock::now();
        auto rows = [=](int64_t r0, int64_t r1) {
            for (int64_t r = r0; r < r1; ++r) {
                // a row piece is a few KB, the next one a whole matrix row further on: the hardware prefetchers do not follow; ask for
                // the piece eight rows ahead by hand (a thread is otherwise held to its handful of outstanding cache misses)
                if (r + 8 < r1) {
                    const char *pf = (const char *)(X + (size_t)(r + 8) * ld + w0);
                    for (size_t b = 0; b < (size_t)wn * sizeof(InT); b += 64) __builtin_prefetch(pf + b, 0, 1);
                }
                Pol::fill_row(X + (size_t)r * ld + w0, dst + (size_t)r * pitch, wn, pitch);
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back(rows, N * t / T, N * (t + 1) / T);
        rows(0, N / T);
        for (auto &th : pool) th.join();
        Q.t_fill += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_a).count();
        hipError_t e = hipMemcpyAsync(dev[j], dst, (size_t)pitch * sizeof(Cell) * (size_t)N, hipMemcpyHostToDevice, hs->copy);
        if (e == hipSuccess) e = hipEventRecord(hs->up[j], hs->copy);
        std::lock_guard<std::mutex> g(Q.mu);
        if (e != hipSuccess) Q.err = 1;
        Q.ready = k + 1;
        Q.cv.notify_all();
        if (Q.err) return;
    }
}
// One pipeline for both forms: pol says what they differ in; runs receives the column ranges that must go up again.
template <typename InT, typename Pol> static int host_windows_pipeline(illico_ctx *c, const InT *X, int64_t ld, int64_t N, int64_t col_lb, int64_t col_ub, int flags, int alternative,
                                 const OutPlanes &o, std::vector<std::pair<int64_t, int64_t>> &runs, Pol &pol) {
    typedef typename Pol::Cell Cell;
    int rc;
    // windows of ~256 MB (a multiple of 64 genes): long enough for the link's rate, short enough that the first pass starts early
    // (wmax is a multiple of 64 unless "gene_batch" says otherwise: every window's row pitch fits its slot)
    int64_t wmax = std::max<int64_t>(64, (int64_t)(((size_t)256 << 20) / ((size_t)N * sizeof(Cell))) & ~63ll);
    wmax = std::min<int64_t>(wmax, std::max<int64_t>(64, (int64_t)((size_t)c->scratch_bytes / HS_SLOTS / ((size_t)N * sizeof(Cell))) & ~63ll));
    if (c->gene_batch > 0) wmax = std::min<int64_t>(wmax, (std::max<int64_t>(1, c->gene_batch) + Pol::pad - 1) & ~(int64_t)(Pol::pad - 1));
    const size_t slot_bytes = (size_t)wmax * (size_t)N * sizeof(Cell);
    HostStage *hs = host_stage_of(c);
    if ((rc = prepare_host_stage(c, hs, slot_bytes)) || (rc = pol.prepare(c, hs, N, col_ub - col_lb))) return rc;
    Cell *dev[HS_SLOTS];
    static const char *names[HS_SLOTS] = {"xin0", "xin1", "xin2"};
    for (int j = 0; j < HS_SLOTS; ++j)
        if ((rc = scratch(c, names[j], (size_t)wmax * (size_t)N, &dev[j]))) return rc;
    HostWindowQueue Q;
    Q.N = N; Q.col_lb = col_lb; Q.col_ub = col_ub; Q.wmax = wmax; Q.n_win = (col_ub - col_lb + wmax - 1) / wmax;
    const int x_node = c->no_host_numa ? -1 : numa_node_of_buffer(X, (size_t)N * (size_t)ld * sizeof(InT));
    std::thread producer([&] { produce_host_windows<InT, Pol>(c, hs, Q, X, ld, x_node, dev); });
    std::vector<u32> hf;
    rc = ILLICO_OK;
    for (int64_t k = 0; k < Q.n_win && !rc; ++k) {
        const int j = (int)(k % HS_SLOTS);
        const int64_t w0 = Q.w0(k), wn = Q.wn(k), pitch = (wn + Pol::pad - 1) & ~(int64_t)(Pol::pad - 1);
        {
            const auto t_a = std::chrono::steady_clock::now();
            std::unique_lock<std::mutex> lk(Q.mu);
            Q.cv.wait(lk, [&] { return Q.ready > k || Q.err; });
            Q.t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_a).count();
            if (Q.err) { rc = fail(c, ILLICO_ERR_HIP, "staging a host window failed"); break; }
        }
        if (hipStreamWaitEvent(c->stream, hs->up[j], 0) != hipSuccess) { rc = fail(c, ILLICO_ERR_HIP, "hipStreamWaitEvent failed"); break; }
        rc = run_fused_ovo<Cell>(c, {dev[j], pitch, 0, (int)wn, flags, alternative, o, w0 - col_lb}, hf);
        if (!rc) rc = pol.after_pass(c, hs, dev[j], N, wn, w0, col_lb, hf, runs);
        if (!rc && hipEventRecord(hs->done[j], c->stream) != hipSuccess) rc = fail(c, ILLICO_ERR_HIP, "hipEventRecord failed");
        c->h2d_input_bytes += (int64_t)((size_t)pitch * sizeof(Cell) * (size_t)N);
        std::lock_guard<std::mutex> g(Q.mu);
        Q.consumed = k + 1;
        if (rc) Q.err = 1;
        Q.cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> g(Q.mu);
        if (rc) Q.err = 1;
        Q.consumed = Q.n_win + HS_SLOTS;
        Q.cv.notify_all();
    }
    producer.join();
    hipStreamSynchronize(hs->copy);
    if (getenv("ILLICO_HS_DEBUG"))
        fprintf(stderr, "[illico] host %s windows: %lld x %lld genes, slot fill %.1f ms, consumer waited %.1f ms for uploads, matrix on NUMA node %d\n",
                Pol::name(), (long long)Q.n_win, (long long)wmax, Q.t_fill * 1e3, Q.t_wait * 1e3, x_node);
    return rc;
}
// ---- gathered columns: a few scattered genes of a device-resident window as a narrow matrix of their own (kernels_leftover.h) ----
// How many columns of N cells a gather may take (0: none): the narrow matrix fits "scratch_bytes" and the column numbers 32 bits.
// Also the bound under which the device may leave the 256-value stage to run_leftovers (k_wide_decide).
template <typename InT> static int64_t max_gather_columns(const illico_ctx *c, int64_t N, int64_t col_ub) {
    if (c->no_leftover_gather || col_ub > 0x7FFFFFFFll) return 0;
    return (int64_t)((size_t)c->scratch_bytes / std::max<size_t>(1, (size_t)N * sizeof(InT))) & ~63ll;
}
// n of a window's W columns (fewer than half), padded to 64: device input, and nobody taps the statistics by window column
template <typename InT> static bool can_gather_columns(const illico_ctx *c, int flags, int64_t N, int64_t n, int64_t W, int64_t col_ub) {
    return (flags & ILLICO_FLAG_INPUT_DEVICE) && !c->tap && n * 2 <= W && ((n + 63) & ~63ll) <= max_gather_columns<InT>(c, N, col_ub);
}
// Columns src of X into *xl [N][n_pad] (scratch x_name); the list goes up through scratch list_name, with dst (output columns, if
// given) behind it as *d_dst.  Waits: the host lists may go out of scope.
template <typename InT> static int gather_columns_narrow(illico_ctx *c, const void *X, int64_t ld, int64_t N, const std::vector<int> &src, const std::vector<int> *dst,
                                 const char *x_name, const char *list_name, InT **xl, int **d_dst = nullptr) {
    const int64_t n = (int64_t)src.size(), n_pad = (n + 63) & ~63ll;
    int rc;
    int *d_src;
    if ((rc = scratch(c, x_name, (size_t)N * (size_t)n_pad, xl))) return rc;
    if ((rc = scratch(c, list_name, (size_t)n * (dst ? 2 : 1), &d_src))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_src, src.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (dst) {
        *d_dst = d_src + n;
        HIPCHK(c, hipMemcpyAsync(*d_dst, dst->data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
    {
        ProfScope ps(c, KID_GATHER_COLS);
        KERNELCHK(c, k_gather_columns<InT>, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, (const InT *)X, (long long)ld, (int)N, (const int *)d_src, (int)n, (int)n_pad,
                  *xl, (long long)n_pad, 0ll);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ILLICO_OK;
}
template <typename InT, typename KeyT> static int run_dense_twopass(illico_ctx *c, const void *X, int dtype, int64_t N, int64_t ld, int64_t col_lb, int64_t col_ub, int flags,
                             int alternative, const OutPlanes &o, std::vector<std::pair<int64_t, int64_t>> runs, const int *col_map = nullptr,
                             bool prefer_counts = false, bool allow_packed = true);
// A narrow device matrix xl [N][n_pad] of n flagged genes (gathered by run_leftovers) computed as one window: init[j] = 1: the 256-value stage first (wide_skipped: it was left to us), 3: not worth it;
// dst[j]: gene j's column of the caller's planes.
template <typename InT, typename KeyT> static int leftovers_on_narrow(illico_ctx *c, InT *xl, int dtype, int64_t N, int64_t n, int64_t n_pad, int flags, int alternative, const OutPlanes &o,
                               const std::vector<u32> &init, const std::vector<int> &dst, bool wide_skipped, bool is_outer) {
    const int G = (int)c->n_groups;
    int rc;
    int *d_dst;
    if ((rc = scratch(c, is_outer ? "xleft2_cols" : "xleft_cols", (size_t)n * 2, &d_dst))) return rc;
    u32 *d_flags2 = (u32 *)(d_dst + n);
    HIPCHK(c, hipMemcpyAsync(d_dst, dst.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the host list may go out of scope)
    const int lflags = (flags | ILLICO_FLAG_INPUT_DEVICE) & ~ILLICO_FLAG_DEFER;
    if (wide_skipped) {
        std::vector<u32> hf2;
        bool any = false;
        for (int64_t j = 0; j < n; ++j) any = any || init[j] == 1u;
        if (any) {
            double *tp;
            if ((rc = scratch(c, "wide_tmp", (size_t)(o.z ? 4 : 3) * G * (size_t)n_pad, &tp))) return rc;
            const OutPlanes ot{tp, tp + (size_t)G * n_pad, tp + (size_t)2 * G * n_pad, n_pad, false, o.z ? tp + (size_t)3 * G * n_pad : nullptr};
            if ((rc = run_fused_ovo<InT>(c, {xl, n_pad, 0, (int)n, lflags, alternative, ot, 0, -1, false, 0, init.data()}, hf2))) return rc;
            HIPCHK(c, hipMemcpyAsync(d_flags2, hf2.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
            {
                ProfScope ps(c, KID_GATHER_COLS);
                const dim3 grid((unsigned)((n + 255) / 256), (unsigned)std::min(G, 1024));
                KERNELCHK(c, k_scatter_planes, grid, dim3(256), 0, (const double *)ot.p, (const double *)ot.u, (const double *)ot.fc, (long long)n_pad, (const int *)d_dst,
                          (const u32 *)d_flags2, 2u, (int)n, G, o.p, o.u, o.fc, (long long)o.ld);
                if (o.z) KERNELCHK(c, k_scatter_plane, grid, dim3(256), 0, (const double *)ot.z, (long long)n_pad, (const int *)d_dst, (const u32 *)d_flags2, 2u, (int)n, G,
                                   o.z, (long long)o.ld);
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::vector<u32> hf3((size_t)n);
            for (int64_t j = 0; j < n; ++j) hf3[j] = hf2[j] == 2u ? 0u : 1u;
            return run_leftovers<InT, KeyT>(c, xl, dtype, N, n_pad, 0, n, lflags, alternative, o, hf3.data(), false, dst.data());
        }
    }
    std::vector<std::pair<int64_t, int64_t>> runs{{0, n}};
    return run_dense_twopass<InT, KeyT>(c, xl, dtype, N, n_pad, 0, n, lflags, alternative, o, runs, d_dst, true);
}
// The genes the fused passes of a DEVICE-resident window [col_lb, col_ub) left behind (hf[j] = 1 / 3).  Few and scattered (a count
// matrix's highly expressed genes): gathered into a narrow matrix of their own and computed as ONE window whose results
// k_finalize scatters back through a column map (kernels_leftover.h).  Many (normalised data: every gene): the column runs, as before.
// wide_skipped: the device left the 256-value stage to us (k_wide_decide): it runs on the narrow matrix first (the genes flagged 1),
// its finished columns are copied into the caller's planes, and what it leaves is gathered once more out of the narrow matrix.
// outer (host, [W]): the window is itself such a narrow matrix -- column j of it is column outer[j] of the caller's planes.
template <typename InT, typename KeyT> int run_leftovers(illico_ctx *c, const void *X, int dtype, int64_t N, int64_t ld, int64_t col_lb, int64_t col_ub, int flags, int alternative,
                  const OutPlanes &o, const u32 *hf, bool wide_skipped, const int *outer) {
    const int64_t W = col_ub - col_lb;
    int rc;
    std::vector<int> src, dst;
    for (int64_t j = 0; j < W; ++j)
        if (hf[j] == 1u || hf[j] == 3u) { src.push_back((int)(col_lb + j)); dst.push_back(outer ? outer[j] : (int)j); }
    if (src.empty()) return ILLICO_OK;
    const int64_t n = (int64_t)src.size(), n_pad = (n + 63) & ~63ll;
    if (!can_gather_columns<InT>(c, flags, N, n, W, col_ub)) {
        std::vector<u32> merged(hf, hf + W);
        if (wide_skipped) { // (k_wide_decide only leaves the stage to us when the gather is possible; an option changed in between)
            std::vector<u32> init((size_t)W), hf2;
            for (int64_t j = 0; j < W; ++j) init[j] = hf[j] == 1u ? 1u : 3u;
            if ((rc = run_fused_ovo<InT>(c, {X, ld, col_lb, (int)W, flags & ~ILLICO_FLAG_DEFER, alternative, o, 0, -1, false, 0, init.data()}, hf2))) return rc;
            for (int64_t j = 0; j < W; ++j) merged[j] = ((hf[j] == 1u || hf[j] == 3u) && hf2[j] != 2u) ? 1u : 0u;
        }
        if (outer) { // a narrow matrix whose leftovers cannot be gathered again: all of it as one window, through the map
            int *v;
            if ((rc = scratch(c, "xleft_outer", (size_t)W, &v))) return rc;
            HIPCHK(c, hipMemcpyAsync(v, outer, (size_t)W * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::vector<std::pair<int64_t, int64_t>> all{{col_lb, col_ub}};
            return run_dense_twopass<InT, KeyT>(c, X, dtype, N, ld, col_lb, col_ub, flags, alternative, o, all, v, true);
        }
        std::vector<std::pair<int64_t, int64_t>> runs;
        flagged_runs(merged.data(), W, col_lb, runs);
        return run_dense_twopass<InT, KeyT>(c, X, dtype, N, ld, col_lb, col_ub, flags, alternative, o, runs);
    }
    InT *xl;
    if ((rc = gather_columns_narrow<InT>(c, X, ld, N, src, nullptr, outer ? "xleft2" : "xleft", outer ? "xleft2_src" : "xleft_src", &xl))) return rc;
    std::vector<u32> init((size_t)n);
    for (int64_t j = 0; j < n; ++j) init[j] = hf[src[j] - col_lb] == 1u ? 1u : 3u;
    return leftovers_on_narrow<InT, KeyT>(c, xl, dtype, N, n, n_pad, flags, alternative, o, init, dst, wide_skipped, outer != nullptr);
}
// ---- a dense call as a list of routes.  int route(D, bool *done): *done = true: the call is over ----
template <typename InT> struct DenseCall {
    illico_ctx *c;
    const InT *X;
    int dtype, flags, alternative;
    int64_t N, ld, col_lb, col_ub;
    const OutPlanes &o;
    bool in_dev, try_fused;                         // try_fused: the fused single pass may run, and there is something to run it on
    bool windowed = false;                          // a host route took the window: runs holds what it left
    std::vector<std::pair<int64_t, int64_t>> runs;  // column ranges still to be computed by the two-pass routes
    int64_t W() const { return col_ub - col_lb; }
};
// Route 1 (dense, count-valued genes), device input: the fused single pass; run_leftovers takes the genes it reports.
// Which genes are count-valued is found by the kernels themselves (k_fused_ref reads the reference rows first, k_fused_probe
// a few hundred rows of every gene): flagged tiles are skipped on the device, so there is no host-side route decision, no
// sampling round trip and nothing cached between calls.
template <typename InT, typename KeyT> static int route_fused_device(DenseCall<InT> &D, bool *done) {
    illico_ctx *c = D.c;
    if (!D.in_dev || !D.try_fused) return ILLICO_OK;
    *done = true;
    int rc;
    std::vector<u32> hf;
    FusedCall q{D.X, D.ld, D.col_lb, (int)D.W(), D.flags, D.alternative, D.o, 0};
    q.probe = c->ref < 0;
    q.max_gather = max_gather_columns<InT>(c, D.N, D.col_ub);
    // ILLICO_FLAG_DEFER (device planes only): enqueue and return; the flags are looked at by resolve_pending
    if ((D.flags & ILLICO_FLAG_DEFER) && (D.flags & ILLICO_FLAG_OUTPUT_DEVICE) && !D.o.staged) {
        q.defer_slot = c->pend_next;
        if ((rc = run_fused_ovo<InT>(c, q, hf))) return rc;
        if ((rc = post_deferred_call(c, q.defer_slot, 0, D.dtype, D.flags, D.alternative, D.N, D.col_lb, D.col_ub, D.o))) return rc;
        c->pend.X = D.X; c->pend.ld = D.ld;
        return ILLICO_OK;
    }
    if ((rc = run_fused_ovo<InT>(c, q, hf))) return rc;
    return run_leftovers<InT, KeyT>(c, D.X, D.dtype, D.N, D.ld, D.col_lb, D.col_ub, D.flags, D.alternative, D.o, hf.data(), hf[D.W()] != 0u);
}
// host matrix of counts with light tails: byte windows ("host_narrow": 1 forces them, -1 forbids them)
template <typename InT> static int route_host_byte_windows(DenseCall<InT> &D, bool *done) {
    illico_ctx *c = D.c;
    bool light = false;
    if (D.in_dev || !D.try_fused || c->host_narrow < 0 || c->max_nonref > 65535) return ILLICO_OK;
    if (c->host_narrow == 0 && !(host_window_is_count_valued<InT>(D.X, D.ld, D.col_lb, D.N, D.W(), &light) && light)) return ILLICO_OK;
    D.windowed = true;
    ByteWindows<InT> pol;
    const int rc = host_windows_pipeline<InT>(c, D.X, D.ld, D.N, D.col_lb, D.col_ub, D.flags, D.alternative, D.o, D.runs, pol);
    *done = !rc && D.runs.empty();
    return rc;
}
// host matrix of counts: column windows travel through pinned staging slots in the matrix's own type and take the same fused pass;
// the gathered leftovers are one window of a device matrix, their results scattered through the column map
template <typename InT, typename KeyT> static int route_host_windows(DenseCall<InT> &D, bool *done) {
    illico_ctx *c = D.c;
    if (D.windowed || D.in_dev || !D.try_fused || !host_window_is_count_valued<InT>(D.X, D.ld, D.col_lb, D.N, D.W())) return ILLICO_OK;
    D.windowed = true;
    int rc;
    OwnTypeWindows<InT> pol;
    if ((rc = host_windows_pipeline<InT>(c, D.X, D.ld, D.N, D.col_lb, D.col_ub, D.flags, D.alternative, D.o, D.runs, pol))) return rc;
    const HostLeftovers &left = pol.left;
    if (left.n > 0) {
        std::vector<std::pair<int64_t, int64_t>> lr{{0, left.n}};
        if ((rc = run_dense_twopass<InT, KeyT>(c, left.xl, D.dtype, D.N, left.cap, 0, left.n, D.flags | ILLICO_FLAG_INPUT_DEVICE, D.alternative, D.o, lr,
                                               left.d_dst, true))) return rc;
    }
    *done = D.runs.empty();
    return ILLICO_OK;
}
template <typename InT, typename KeyT> int run_dense_t(illico_ctx *c, const void *X, int dtype, int64_t N, int64_t ld, int64_t col_lb, int64_t col_ub, int flags,
                int alternative, const OutPlanes &o) {
    // the fused kernels: a row pitch within 32-bit byte offsets; they go from values to p-values without leaving statistics behind (no tap)
    const bool try_fused = fused_path_allowed(c, flags) && (uint64_t)ld * sizeof(InT) < (1ull << 32) && !c->tap && N > 0 && col_ub > col_lb;
    DenseCall<InT> D{c, (const InT *)X, dtype, flags, alternative, N, ld, col_lb, col_ub, o, (flags & ILLICO_FLAG_INPUT_DEVICE) != 0, try_fused};
    int rc;
    bool done = false;
    if ((rc = route_fused_device<InT, KeyT>(D, &done)) || done) return rc;
    if ((rc = route_host_byte_windows<InT>(D, &done)) || done) return rc;
    if ((rc = route_host_windows<InT, KeyT>(D, &done)) || done) return rc;
    if (!D.windowed) D.runs.push_back({col_lb, col_ub});
    return run_dense_twopass<InT, KeyT>(c, X, dtype, N, ld, col_lb, col_ub, flags, alternative, o, D.runs);
}
// ---- routes 2-4 over the column runs the fused route left (or over everything): the transposition and the per-gene rank kernels, in
// gene batches bounded by the scratch cap.  One TwoPassPlan per call; a batch takes one of four routes over it ----
template <typename InT, typename KeyT> struct TwoPassPlan {
    illico_ctx *c;
    const void *X;
    int64_t ld, N, col_lb, col_ub;
    int flags, alternative, dtype;
    const OutPlanes &o;
    const int *cmap;        // (finalize: output column of batch gene j = cmap[b0 - col_lb + j]; null: the window's own columns)
    bool prefer_counts, in_dev, packed, padded, ovr_counts, ovr_packed;
    int64_t stride, nb_max;
    KeyT *Xt; StatsPlanes st; u32 *gflags; OvoGlobalBufs gb; // a batch's scratch
    InT *xin;               // host input: a batch's columns on the device
};
struct BatchInput { const void *X; int64_t ld, col0; }; // where a batch's columns lie on the device
// Flagged genes scattered through the window would make one tiny launch sequence each: runs closer than 32 genes
// are merged (the good genes in between are recomputed, identically, by the two-pass routes).
static void merge_close_runs(std::vector<std::pair<int64_t, int64_t>> &runs) {
    if (runs.size() <= 1) return;
    std::vector<std::pair<int64_t, int64_t>> merged;
    for (auto &r : runs) {
        if (!merged.empty() && r.first - merged.back().second < 32) merged.back().second = r.second;
        else merged.push_back(r);
    }
    runs.swap(merged);
}
// prefer_counts: the genes are count-like (gathered leftovers of a count matrix) -- the plain transposition with per-gene histogram
// routes (k_ovo_counts / k_ovr_counts) first, the routes for continuous values only for what they leave.
template <typename InT, typename KeyT> static int plan_twopass(TwoPassPlan<InT, KeyT> &p, const std::vector<std::pair<int64_t, int64_t>> &runs, bool allow_packed) {
    illico_ctx *c = p.c;
    const int G = (int)c->n_groups;
    const bool ovr = c->ref < 0;
    const int64_t N = p.N;
    p.in_dev = p.flags & ILLICO_FLAG_INPUT_DEVICE;
    p.prefer_counts = p.prefer_counts && !(p.flags & ILLICO_FLAG_LOG1P) && !c->no_counts_path && (ovr || counts_path_allowed(c, p.flags));
    // dense OVO: group-wise packing + look-ups (kernels_ovo_compact.h) whenever the sizes allow; it has no histogram side path
    // (count-valued genes reach this function only when the fused route is off, or as gathered leftovers: prefer_counts) and holds
    // ties exactly
    p.packed = !ovr && !p.prefer_counts && allow_packed && packed_route_fits<KeyT>(c);
    // dense OVR: the transposition with the group sums folded in (k_group_compact keeping every key: padded dense layout)
    // (any group sizes: only the PACKED rows below count a (gene, group)'s non-zeros in 16 bits)
    p.padded = ovr && !p.prefer_counts && !c->no_packed_dense && c->pk_nblk > 0 && c->pk_stride < (1ll << 31);
    // (groups of any size: a group of 65535 cells and more is the last of its block, whose 16-bit length the partition never looks at)
    p.ovr_packed = p.padded && !c->no_ovr_packed_partition && !c->no_ovr_parts_path && G <= 65535 && (c->max_nonref <= 65535 || !c->no_ovr_packed_big);
    p.ovr_counts = ovr && p.prefer_counts && N < (1ll << 31);
    p.stride = (p.packed || p.padded) ? c->pk_stride : ((N + 63) & ~63ll);
    int64_t widest = 0;
    for (auto &r : runs) widest = std::max(widest, r.second - r.first);
    const bool need_glob = !ovr && !ovo_sort_route_fits<KeyT>(c->h_counts[c->ref], c->max_nonref);
    const bool pingpong = ovr || need_glob;
    size_t per_gene = (size_t)p.stride * sizeof(KeyT) * (pingpong ? 2 : 1) + (pingpong ? (size_t)p.stride * 4 * 2 : 0) +
                      (p.in_dev ? 0 : (size_t)N * sizeof(InT)) + (size_t)G * 24 + 64;
    int64_t nb_max = c->gene_batch > 0 ? c->gene_batch : std::max<int64_t>(64, (int64_t)(c->scratch_bytes / per_gene));
    nb_max = std::min<int64_t>(nb_max, widest);
    if (nb_max > 64) nb_max &= ~63ll;
    p.nb_max = nb_max = std::max<int64_t>(nb_max, 1);
    int rc;
    if ((rc = scratch(c, "xt", (size_t)nb_max * p.stride, &p.Xt))) return rc;
    if ((rc = carve_stats(c, nb_max, G, false, &p.st))) return rc;
    p.gflags = nullptr;
    if (((counts_path_allowed(c, p.flags) && !p.packed && !ovr) || p.ovr_counts) && (rc = scratch(c, "gene_flags", (size_t)nb_max, &p.gflags))) return rc;
    if (need_glob) {
        KeyT *kb;
        if ((rc = scratch(c, "ovr_kb", (size_t)nb_max * p.stride, &kb))) return rc;
        p.gb.kb = kb;
        if ((rc = scratch(c, "ovr_va", (size_t)nb_max * p.stride, &p.gb.va))) return rc;
        if ((rc = scratch(c, "ovr_vb", (size_t)nb_max * p.stride, &p.gb.vb))) return rc;
    }
    p.xin = nullptr;
    if (!p.in_dev && (rc = scratch(c, "xin", (size_t)nb_max * N, &p.xin))) return rc;
    return ILLICO_OK;
}
// host input: the batch's columns go up into xin
template <typename InT, typename KeyT> static int stage_batch_input(const TwoPassPlan<InT, KeyT> &p, int64_t b0, int nb, BatchInput *in) {
    *in = {p.X, p.ld, b0};
    if (p.in_dev) return ILLICO_OK;
    HIPCHK(p.c, hipMemcpy2DAsync(p.xin, (size_t)nb * sizeof(InT), (const InT *)p.X + b0, (size_t)p.ld * sizeof(InT),
                                 (size_t)nb * sizeof(InT), (size_t)p.N, hipMemcpyHostToDevice, p.c->stream));
    *in = {p.xin, nb, 0};
    return ILLICO_OK;
}
template <typename InT, typename KeyT> static int finalize_batch(const TwoPassPlan<InT, KeyT> &p, int64_t b0, int nb, const double *gtot) {
    const int64_t j0 = b0 - p.col_lb;
    return launch_finalize(p.c, p.st.s2u, p.st.stie, p.st.ssum, gtot, nb, p.flags, p.alternative, p.o, p.cmap ? 0 : j0, p.cmap ? p.cmap + j0 : nullptr);
}
// A batch's statistics: to the tap (illico_rank_statistics), or through k_finalize into the planes
template <typename InT, typename KeyT> static int emit_batch(const TwoPassPlan<InT, KeyT> &p, int64_t b0, int nb, const double *gtot) {
    illico_ctx *c = p.c;
    if (!c->tap) return finalize_batch(p, b0, nb, gtot);
    const size_t off = (size_t)(b0 - p.col_lb) * c->n_groups, cnt = (size_t)nb * c->n_groups;
    HIPCHK(c, hipMemcpyAsync(c->tap->two_u + off, p.st.s2u, cnt * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->tap->tie + off, p.st.stie, cnt * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->tap->sum + off, p.st.ssum, cnt * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ILLICO_OK;
}
// the plain transposition of a batch; gflags (where the plan has them): the genes the histogram kernels cannot take
template <typename InT, typename KeyT> static int transpose_batch(const TwoPassPlan<InT, KeyT> &p, const BatchInput &in, int nb) {
    illico_ctx *c = p.c;
    if (p.gflags) HIPCHK(c, hipMemsetAsync(p.gflags, 0, (size_t)nb * 4, c->stream));
    return launch_transpose<InT, KeyT>(c, in.X, in.ld, in.col0, nb, (int)p.N, p.Xt, p.stride, p.gflags, p.ovr_counts ? OVRC_R : ovo_counts_limit(c));
}
// OVO, packed layout; redo_runs receives the genes the route left while groups above 1024 cells rule k_ovo_rank out
template <typename InT, typename KeyT>
static int twopass_ovo_packed_batch(const TwoPassPlan<InT, KeyT> &p, const BatchInput &in, int64_t b0, int nb, std::vector<std::pair<int64_t, int64_t>> &redo_runs) {
    int rc;
    std::vector<int> redo;
    if ((rc = run_ovo_packed<InT, KeyT>(p.c, in.X, in.ld, in.col0, nb, (int)p.N, p.Xt, p.stride, p.dtype, p.flags, p.st.s2u, p.st.stie, p.st.ssum, &redo))) return rc;
    for (int j : redo) {
        if (!redo_runs.empty() && redo_runs.back().second == b0 + j) redo_runs.back().second = b0 + j + 1;
        else redo_runs.push_back({b0 + j, b0 + j + 1});
    }
    return emit_batch(p, b0, nb, nullptr);
}
// OVO: transposition, then k_ovo_counts (flagged-free genes) and the sort routes (launch_ovo)
template <typename InT, typename KeyT> static int twopass_ovo_batch(TwoPassPlan<InT, KeyT> &p, const BatchInput &in, int64_t b0, int nb) {
    illico_ctx *c = p.c;
    int rc;
    if ((rc = transpose_batch(p, in, nb))) return rc;
    OvoParams P;
    P.Xs = p.Xt; P.gene_stride = p.stride; P.pos_ptr = c->d_posptr; P.seg_ptr = nullptr; P.counts = c->d_counts;
    P.G = (int)c->n_groups; P.ref = (int)c->ref; P.n_genes = nb; P.dt = p.dtype; P.is_log1p = (p.flags & ILLICO_FLAG_LOG1P) ? 1 : 0;
    P.ref_cap = 0; P.out_2u = p.st.s2u; P.out_tie = p.st.stie; P.out_sum = p.st.ssum;
    if ((rc = launch_ovo<KeyT>(c, P, c->h_counts[c->ref], c->max_nonref, p.gflags, &p.gb, false))) return rc;
    return emit_batch(p, b0, nb, nullptr);
}
// OVR, count-like leftovers: the column-histogram kernel takes every integer gene below OVRC_R; the value-range parts /
// the general route only see the runs of genes it flags.  No tap here: prefer_counts is only asked for gathered columns, which
// a tapped call never has (can_gather_columns), and for host windows, which it never takes (run_dense_t).
template <typename InT, typename KeyT> static int twopass_ovr_counts_batch(const TwoPassPlan<InT, KeyT> &p, const BatchInput &in, int64_t b0, int nb) {
    illico_ctx *c = p.c;
    const int G = (int)c->n_groups, N = (int)p.N;
    const int64_t stride = p.stride;
    const StatsPlanes &st = p.st;
    int rc;
    if ((rc = transpose_batch(p, in, nb))) return rc;
    {
        OvrCountsParams Q;
        Q.Xt = p.Xt; Q.stride = stride; Q.pos_ptr = c->d_posptr; Q.counts = c->d_counts; Q.G = G; Q.n_genes = nb; Q.dt = p.dtype; Q.n_cells = p.N;
        Q.gene_flags = p.gflags; Q.out_2u = st.s2u; Q.out_tie = st.stie; Q.out_sum = st.ssum; Q.gene_total = st.gtot;
        ProfScope ps(c, KID_OVR_COUNTS);
        KERNELCHK(c, k_ovr_counts<KeyT>, dim3(nb), dim3(OVRC_NT), OVRC_R * 4, Q);
    }
    std::vector<u32> hg(nb);
    HIPCHK(c, hipMemcpyAsync(hg.data(), p.gflags, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int j = 0; j < nb;) {
        if (!hg[j]) { ++j; continue; }
        int e = j;
        while (e < nb && hg[e]) ++e;
        const int sub = e - j;
        bool done = false;
        if ((rc = run_ovr_dense_parts<KeyT>(c, p.Xt + (size_t)j * stride, stride, sub, N, p.dtype, p.flags, st.s2u + (size_t)j * G, st.stie + (size_t)j * G,
                                            st.ssum + (size_t)j * G, st.gtot + j, &done, false, nullptr))) return rc;
        if (!done && (rc = run_ovr_dense_batch<KeyT>(c, p.Xt + (size_t)j * stride, stride, sub, N, p.dtype, p.flags, st.s2u + (size_t)j * G,
                                                     st.stie + (size_t)j * G, st.ssum + (size_t)j * G, st.gtot + j, false))) return rc;
        j = e;
    }
    return finalize_batch(p, b0, nb, st.gtot);
}
// OVR: k_group_compact into the padded (or, for the partition, packed) layout -- or the plain transposition -- then the value-range
// parts; sizes they do not take go the general route, over padded rows
template <typename InT, typename KeyT> static int twopass_ovr_batch(const TwoPassPlan<InT, KeyT> &p, const BatchInput &in, int64_t b0, int nb) {
    illico_ctx *c = p.c;
    const int G = (int)c->n_groups, flags = p.flags;
    const int64_t stride = p.stride;
    const StatsPlanes &st = p.st;
    KeyT *Xt = p.Xt;
    int rc;
    OvrPackedInput pki;
    if (p.padded) {
        GroupCompactParams Q;
        memset(&Q, 0, sizeof Q);
        Q.X = in.X; Q.ld = in.ld; Q.col0 = in.col0; Q.ncols = nb; Q.perm = c->d_perm; Q.pos_ptr = c->d_posptr; Q.G = G; Q.ref = -1; Q.nseg = 0;
        Q.blk_g0 = c->d_pk_blk; Q.blk_g1 = c->d_pk_blk + c->pk_nblk; Q.blk_out = c->d_pk_blk + 2 * c->pk_nblk; Q.nblk = c->pk_nblk;
        Q.Xt = Xt; Q.xt_stride = stride; Q.out_sum = st.ssum;
        if (p.ovr_packed) { // packed rows (non-zero keys only) for the partition; flagged genes are written again, padded, below
            if ((rc = scratch(c, "packed_nnz", (size_t)nb * G + 32, &Q.nnz))) return rc;
            if ((rc = scratch(c, "packed_seg_sum", (size_t)nb * G + (size_t)nb * c->pk_nblk + 16, &Q.gofs))) return rc;
            Q.blk_cnt = Q.gofs + (size_t)nb * G;
            pki.nnz = Q.nnz; pki.blk_cnt = Q.blk_cnt;
            const GroupCompactParams Q0 = Q;
            pki.repad = [c, Q0, Xt, stride, flags, G](int first, int sub) -> int {
                GroupCompactParams R = Q0;
                R.col0 = Q0.col0 + first; R.ncols = sub; R.Xt = (KeyT *)Xt + (size_t)first * stride;
                R.out_sum = Q0.out_sum + (size_t)first * G; R.nnz = nullptr; R.gofs = nullptr; R.blk_cnt = nullptr;
                return launch_group_compact<InT, KeyT>(c, R, sub, flags, false);
            };
        }
        if ((rc = launch_group_compact<InT, KeyT>(c, Q, nb, flags, p.ovr_packed))) return rc;
    } else if ((rc = transpose_batch(p, in, nb))) return rc;
    bool done = false;
    if ((rc = run_ovr_dense_parts<KeyT>(c, Xt, stride, nb, (int)p.N, p.dtype, flags, st.s2u, st.stie, st.ssum, st.gtot, &done, p.padded, p.ovr_packed ? &pki : nullptr))) return rc;
    if (!done) {
        if (p.ovr_packed && (rc = pki.repad(0, nb))) return rc;
        if ((rc = run_ovr_dense_batch<KeyT>(c, Xt, stride, nb, (int)p.N, p.dtype, flags, st.s2u, st.stie, st.ssum, st.gtot, p.padded))) return rc;
    }
    return emit_batch(p, b0, nb, st.gtot);
}
// The genes the packed route left (tie-heavy columns of a matrix with groups above 1024 cells): transposition + the general sort route.
// Few genes scattered over the window (each a run of its own: one transposition, one single-workgroup sort after the other --
// nine genes of a two-million-cell matrix: 480 ms): gathered into a narrow matrix and computed as ONE batch, side by side.
template <typename InT, typename KeyT> static int redo_as_one_batch(const TwoPassPlan<InT, KeyT> &p, const std::vector<std::pair<int64_t, int64_t>> &redo_runs) {
    illico_ctx *c = p.c;
    int64_t n = 0;
    for (auto &r : redo_runs) n += r.second - r.first;
    if (redo_runs.size() > 1 && !p.cmap && can_gather_columns<InT>(c, p.flags, p.N, n, p.col_ub - p.col_lb, p.col_ub)) {
        std::vector<int> src, dst;
        for (auto &r : redo_runs)
            for (int64_t j = r.first; j < r.second; ++j) { src.push_back((int)j); dst.push_back((int)(j - p.col_lb)); }
        int rc;
        InT *xl;
        int *d_dst;
        if ((rc = gather_columns_narrow<InT>(c, p.X, p.ld, p.N, src, &dst, "xredo", "xredo_cols", &xl, &d_dst))) return rc;
        std::vector<std::pair<int64_t, int64_t>> all{{0, n}};
        return run_dense_twopass<InT, KeyT>(c, xl, p.dtype, p.N, (n + 63) & ~63ll, 0, n, p.flags, p.alternative, p.o, all, d_dst, p.prefer_counts, false);
    }
    return run_dense_twopass<InT, KeyT>(c, p.X, p.dtype, p.N, p.ld, p.col_lb, p.col_ub, p.flags, p.alternative, p.o, redo_runs, p.cmap, p.prefer_counts, false);
}
// col_map (device, one entry per column of X's window): the output column of each gene, relative to the planes (the gathered
// leftover columns of a count matrix, kernels_leftover.h)
template <typename InT, typename KeyT> static int run_dense_twopass(illico_ctx *c, const void *X, int dtype, int64_t N, int64_t ld, int64_t col_lb, int64_t col_ub, int flags,
                             int alternative, const OutPlanes &o, std::vector<std::pair<int64_t, int64_t>> runs, const int *col_map,
                             bool prefer_counts, bool allow_packed) {
    TwoPassPlan<InT, KeyT> p{c, X, ld, N, col_lb, col_ub, flags, alternative, dtype, o, col_map, prefer_counts};
    const bool ovr = c->ref < 0;
    int rc;
    merge_close_runs(runs);
    if ((rc = plan_twopass(p, runs, allow_packed))) return rc;
    std::vector<std::pair<int64_t, int64_t>> redo_runs;
    for (auto &run : runs)
        for (int64_t b0 = run.first; b0 < run.second; b0 += p.nb_max) {
            const int nb = (int)std::min<int64_t>(p.nb_max, run.second - b0);
            BatchInput in;
            if ((rc = stage_batch_input(p, b0, nb, &in))) return rc;
            rc = p.packed ? twopass_ovo_packed_batch(p, in, b0, nb, redo_runs) : !ovr ? twopass_ovo_batch(p, in, b0, nb)
               : p.ovr_counts ? twopass_ovr_counts_batch(p, in, b0, nb) : twopass_ovr_batch(p, in, b0, nb);
            if (rc) return rc;
        }
    return redo_runs.empty() ? ILLICO_OK : redo_as_one_batch(p, redo_runs);
}
