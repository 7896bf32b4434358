// CSC, count-valued genes, small groups: one pass over a gene's stored entries builds the per-group value histograms in
// LDS -- h[group][value] -- with ONE non-returning LDS atomic per entry; a sweep with one thread per group then turns
// histograms into the statistics:
//   OVO:  S2 = sum_{c>=1} tB[c] (2 zA + 2 cumA[c] + tA[c]) + zB zA,      tie = T_A + sum_{c>=1} tB (3 tA (tA+tB) + tB^2 - 1) + (t0^3 - t0)
//   OVR:  r2 = sum_{c>=1} tB[c] (2 n0 + 2 cum[c] + t[c] + 1) + zB (n0 + 1),  tie = sum_{c>=1} (t^3 - t) + (n0^3 - n0)
// Per value c the group-independent part is formed once per gene (wave 0, into wtab; tS = t[c] or tA[c], z = n0 or zA):
//   A[c] = 2 z + 2 cum[c] + tS (+ 1: OVR),  B[c] = 3 tS^2 - 1,  C[c] = 3 tS
// so that a cell of tB entries adds tB A[c] to S2 / r2 and (OVO) tB (B[c] + tB (C[c] + tB)) = tB (3 tS (tS + tB) + tB^2 - 1) to the tie sum.
// (zA, zB, n0 = implicit zeros of the reference / the group / the column, t0 = zA + zB) -- the same integers the sort-based
// CSC kernels produce (kernels_csc_gene.h, kernels_ovr.h; sparse_ovo.py:58-85, sparse_ovr.py:70-83), without sorting,
// regrouping or searching anything.  Nothing but the CSC arrays is read from HBM: 1.9 GB at C3.
//
// Takes a gene only if every stored value is an integer in [1, RT) (stored zeros are dropped: they are zeros) and
// -- host-checked -- at most CSCC_MAX_BIG ranked groups have more than 255 cells (those get 32-bit cells); other genes set
// fallback[gene] = 1 and go to the general CSC routes.
//
// Three cell layouts, each stated once in CsccLayout below (word-major: word w of group g = h[w * G + g], so lanes = consecutive
// groups read consecutive words in the sweep and the increments of random groups spread over all banks):
//  * CSCC_MIXED: 8 bits for the values 1 .. 7, 4 bits for 8 .. 63 -> 36 bytes per group, 72 KB for 2000 groups, so that TWO
//    workgroups fit a CU and one gene's entry loop overlaps the other's zeroing / sweep / stores.  A 4-bit cell that
//    overflows (16 or more cells of one group with the same value >= 8) carries into its neighbour: the cells of the gene then
//    add up to fewer entries than were counted (a carry can only lose entries), the gene sets fallback[gene] = 2 and the host
//    sends it through the 8-bit form.  words 0, 1: the 8-bit cells of values 0 .. 7; words 2 .. 8: eight 4-bit cells each.
//  * CSCC_8BIT: 8-bit cells for every value: RT bytes per group (128 KB for 2000 groups at RT = 64: one workgroup per CU).
//  * CSCC_16BIT: 16-bit cells for every group (RT / 2 words per group): what the route takes when more than CSCC_MAX_BIG ranked groups
//    exceed 255 cells -- a few hundred groups of a thousand cells each still fit LDS (300 groups x 128 bytes), and every term of the
//    sweep is 64-bit.
//
// What bounds the entry loop is the texture addresser: one codes[row] gather per entry.  A column's rows ascend, so the 64
// gathers of a wavefront fall into a few cache lines -- half as many with 16-bit codes (codes16): 0.80 -> 0.65 ms at C3.
// History at C3 (tools/micro/cscc_bench.hip, nnz 2.4e8): 8-bit cells, 1024 threads, sweep fully unrolled (43 spilled VGPRs)
// 1.51 ms -> sweep rolled, no spills 1.05 -> 16 entries per thread in flight 1.01 -> mixed cells, 2 x 512 threads per CU 0.79
// -> 16-bit codes 0.65 ms.  Phases of the 1.01 ms form: zeroing + launch 0.15, entry loop 0.64, sweep + stores 0.2.
// A branch-free entry (one redirected atomic per entry, whatever its value): 0.58 -> 0.60 ms, the branches skip more than they cost.
// (The variants these were timed against -- ablation builds, 1024 threads, per-cell sweep terms, that entry -- lived in the tree up to the parent commit.)
//
// Where the layouts, the formulas, the LDS size and each template parameter are stated: DESIGN.md section 25.
#pragma once
#include "common.h"
#include "kernels_finalize.h"

#define CSCC_NT 512
#ifndef CSCC_UL
#define CSCC_UL 16 // entries per thread and round
#endif
#define CSCC_RT 64 // widest table (values 1 .. 63); the 32-value form is used when 64 bytes per group do not fit LDS
#define CSCC_MAX_BIG 8

struct CscCountsParams {
    const void *data, *indices, *indptr; // CSC arrays (device); stored entry k lives at data[k - kshift], indices[k - kshift]
    long long kshift;
    long long col0;                      // first gene of the batch (contiguous batches)
    const int *gene_cols;                // or: the batch's genes as a column list (absolute indices); nullptr = contiguous
    int nb;
    const u16 *codes16;                  // [n_cells] group code per cell as 16-bit values (C16); else `indices` already holds group codes
    const int *counts;                   // [G]
    int G, ref;                          // ref == -1: OVR.  G: the groups THIS launch holds tables for (a window of the groups, below)
    int g_lo, G_total;                   // groups [g_lo, g_lo + G) of G_total: more groups than LDS holds tables for are taken window by window,
                                         // one launch each (entries of other groups only feed the selected histogram); codes, counts, big_slot,
                                         // ref and the statistics are indexed by the group's number among all G_total
    long long n_cells;
    const signed char *big_slot;         // [G] -1, or the row of the group in the 32-bit table (groups of more than 255 cells)
    u32 *fallback;                       // [nb] set to 1 for genes this kernel cannot take
    long long *out_2u;
    u64 *out_tie;
    double *out_sum;
    double *gene_total;                  // OVR: [nb] the column's value sum (what k_gene_totals would add up from out_sum), or nullptr
    int pack16;                          // statistics as 16 bytes per test: out_2u = value sum << 40 | 2U (40 bits, two's complement: -2 = the OVO
                                         // reference row), out_tie; out_sum unused.  Host-checked: no group beyond 255 cells (sums < 2^24, 2U < 2^39)
    int tie_f64;                         // OVR: out_tie = the bits of the float64 tie sum of the reference's sparse path (tie_f64_sparse)
    const u32 *verdict;                  // deferred calls: {non-integers, -, samples} of k_sample_noncount_cols, looked at on the device
                                         // (more than 2 % non-integers: not a count matrix, every gene is left to the general routes); or nullptr
};

// ---- the cell layout: stated here, once, for the host's LDS size, the entry's atomic and the sweep's unpacking ----
// A group's cells are one or two runs of equally wide cells: the values below `split` in `lo_bits` bits each from word 0 on, the values
// from `split` on in 4 bits each behind them.
enum { CSCC_MIXED = 0, CSCC_8BIT = 1, CSCC_16BIT = 2 };
constexpr int cscc_split(int cells, int rt) { return cells == CSCC_MIXED ? 8 : rt; }
constexpr int cscc_lo_bits(int cells) { return cells == CSCC_16BIT ? 16 : 8; }
constexpr int cscc_run_words(int n_values, int bits) { return n_values * bits / 32; }
constexpr int cscc_wpg(int cells, int rt) { // words per group: 9 (mixed, rt = 64), rt / 4, rt / 2
    return cscc_run_words(cscc_split(cells, rt), cscc_lo_bits(cells)) + cscc_run_words(rt - cscc_split(cells, rt), 4);
}
// dynamic LDS of a launch: the cells + one slot byte per group (the 16-bit form knows no side table)
static inline size_t cscc_lds_bytes(int G, int cells, int rt) {
    return (size_t)G * cscc_wpg(cells, rt) * 4 + (cells == CSCC_16BIT ? 16 : (((size_t)G + 15) & ~(size_t)15));
}

// a run: the values V0, V0 + 1, .. in BITS bits each, from word W0 of the group on.  Value c lives in word(c) at shift(c) (the entry's
// side); cell k = 0 .. PER - 1 of word i = w holds count(w, k) entries of the value value(i, k) (the sweep's side): one formula, both ways.
template <int V0, int W0, int BITS> struct CsccRun {
    static constexpr int PER = 32 / BITS, LOG = PER == 2 ? 1 : PER == 4 ? 2 : 3, FIRST = W0;
    static __device__ __forceinline__ int word(int c) { return W0 + ((c - V0) >> LOG); }
    static __device__ __forceinline__ int shift(int c) { return ((c - V0) & (PER - 1)) * BITS; }
    static __device__ __forceinline__ int value(int i, int k) { return V0 + ((i - W0) << LOG) + k; }
    static __device__ __forceinline__ u32 count(u32 w, int k) { return (w >> (k * BITS)) & ((1u << BITS) - 1u); }
};
template <int CELLS, int RT> struct CsccLayout {
    static_assert(CELLS != CSCC_MIXED || RT == 64, "the mixed layout holds the values 1 .. 63");
    static constexpr int SPLIT = cscc_split(CELLS, RT), WPG = cscc_wpg(CELLS, RT);
    typedef CsccRun<0, 0, cscc_lo_bits(CELLS)> Lo;
    typedef CsccRun<SPLIT, cscc_run_words(SPLIT, cscc_lo_bits(CELLS)), 4> Hi; // (no value reaches it unless SPLIT < RT)
    // the entry's side: what one entry of value c adds, and to which word of its group
    static __device__ __forceinline__ int word(int c) { return (SPLIT < RT && c >= SPLIT) ? Hi::word(c) : Lo::word(c); }
    static __device__ __forceinline__ u32 inc(int c) { return 1u << ((SPLIT < RT && c >= SPLIT) ? Hi::shift(c) : Lo::shift(c)); }
};

// CELLS: the layout, chosen by the host per call (CscCountsLayout in sparse_driver.h).  RT: the table's values, 64 or 32 (LDS).
// HAS_BIG: some groups have 32-bit cells of their own (at most CSCC_MAX_BIG groups above 255 cells; never with 16-bit cells).
// C16: group codes come from codes16[row] (the host's case whenever a code table exists: sparse input is limited to fewer than
// 65 536 groups); else `indices` already holds the codes (the device CSR -> CSC transposition writes them).
// WIN: this launch holds tables for the groups [g_lo, g_lo + G) only (CscCountsParams::g_lo).
template <typename InT, typename IdxT, bool OVR, int RT, bool HAS_BIG, int CELLS, bool C16, bool WIN>
__global__ __launch_bounds__(CSCC_NT, CELLS == CSCC_MIXED ? 4 : 2) void k_csc_counts(CscCountsParams P) { // (waves per SIMD: two workgroups per CU for the mixed form)
    typedef CsccLayout<CELLS, RT> Cells;
    constexpr bool MIXED = CELLS == CSCC_MIXED, W16 = CELLS == CSCC_16BIT;
    static_assert(!W16 || !HAS_BIG, "16-bit cells: one plain layout for every group");
    constexpr int NT = CSCC_NT, UL = (HAS_BIG && MIXED) ? CSCC_UL / 2 : CSCC_UL, WPG = Cells::WPG; // (UL halved where 16 entries in flight would spill)
    extern __shared__ __align__(16) u32 cscc_h[];             // [WPG][G] words
    __shared__ u32 hsel[RT];   // OVO: histogram of the reference group's stored values; OVR: of the whole column
    __shared__ u32 hbig[HAS_BIG ? CSCC_MAX_BIG * RT : 1]; // 32-bit cells of the few groups with more than 255 cells
    signed char *slot = (signed char *)(cscc_h + (size_t)WPG * P.G); // [G] copy of big_slot (HAS_BIG)
    __shared__ u32 cum[RT + 1]; // cum[c] = # selected stored values < c (c >= 1); read by cell64 only (HAS_BIG || W16).  (cum[RT] is padding:
                                // without it the tables behind it move by 16 bytes and the HAS_BIG instances take up to 5 VGPRs more)
    __shared__ uint4 wtab[RT]; // per value c: {A, B, C, -}: 2 rank(c) term, 3 tS^2 - 1, 3 tS (B, C: OVO tie term)
    __shared__ u64 s_T, s_sum;
    __shared__ u32 s_nnz, s_entries, s_cells;
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63;
    const int G = P.G, ref = P.ref, g_lo = P.g_lo;
    const InT *data = (const InT *)P.data;
    const IdxT *indices = (const IdxT *)P.indices, *indptr = (const IdxT *)P.indptr;

    if (P.verdict && (double)P.verdict[0] > 0.02 * (double)P.verdict[2]) { // uniform: decided from a value sample, without the host
        for (int gene = blockIdx.x; gene < P.nb; gene += gridDim.x)
            if (tid == 0) P.fallback[gene] = 1u;
        return;
    }
    for (int gene = blockIdx.x; gene < P.nb; gene += gridDim.x) {
        const long long col = P.gene_cols ? (long long)P.gene_cols[gene] : P.col0 + gene;
        const long long k0 = (long long)indptr[col] - P.kshift, k1 = (long long)indptr[col + 1] - P.kshift;
        bool bad = false;
        u32 n_ent = 0; // MIXED: entries this thread put into the packed group tables
        // one stored entry (value v, group code cd) into the tables: ONE non-returning LDS atomic (two for the selected group)
        auto put = [&](InT v, int cd) {
            if (v != (InT)0) {
                const int c = (v > (InT)0 && v < (InT)RT) ? (int)v : 0;
                if (c == 0 || (InT)c != v) bad = true; // negative, fractional, NaN or beyond the table
                else {
                    const int cl = WIN ? cd - g_lo : cd; // the group's place in this launch's window (WIN: a window of the groups)
                    if (!WIN || (unsigned)cl < (unsigned)G) {
                        const int bs = HAS_BIG ? (int)slot[cl] : -1;
                        if (bs >= 0) atomicAdd(&hbig[bs * RT + c], 1u);
                        else if (OVR || cd != ref) {
                            atomicAdd(&cscc_h[Cells::word(c) * G + cl], Cells::inc(c)); // (16-bit cells: a group holds fewer than 65 536 cells)
                            if (MIXED) ++n_ent;
                        }
                    }
                    if (OVR || cd == ref) atomicAdd(&hsel[c], 1u);
                }
            }
        };
        auto zero_tables = [&]() {
            uint4 *h4 = (uint4 *)cscc_h;
            const int n4 = (G * WPG) >> 2;
            for (int i = tid; i < n4; i += NT) h4[i] = make_uint4(0u, 0u, 0u, 0u);
            for (int i = (n4 << 2) + tid; i < G * WPG; i += NT) cscc_h[i] = 0;
            if (tid < RT) hsel[tid] = 0;
            if (HAS_BIG) {
                for (int i = tid; i < CSCC_MAX_BIG * RT; i += NT) hbig[i] = 0;
                for (int i = tid; i < G; i += NT) slot[i] = P.big_slot[g_lo + i];
            }
            if (tid == 0) { s_bad = 0; s_entries = 0; s_cells = 0; }
        };
        // A two-stage pipeline with a straight-line body.  A wavefront owns UL * 64 consecutive entries of a
        // round: every round but a column's last is FULL, and its 2 UL requests are one 32-bit lane offset + immediate
        // offsets off a scalar base -- no per-lane bound, no branch, no 64-bit address per request.  The last round clamps
        // its entry numbers to the column's last entry (requests stay unconditional) and drops the surplus lanes when it
        // counts.
        typedef const __attribute__((address_space(1))) char *gchar_p;
        typedef const __attribute__((address_space(1))) InT *gval_p;
        typedef const __attribute__((address_space(1))) IdxT *gidx_p;
        typedef const __attribute__((address_space(1))) u16 *gu16_p;
        constexpr u32 span = (u32)NT * UL;
        const u32 n = (u32)(k1 - k0); // (a column holds fewer than 2^31 stored entries: at most one per row)
        const u32 R = (n + span - 1) / span;
        const gchar_p dbase = (gchar_p)(data + k0), ibase = (gchar_p)(indices + k0), cbase = (gchar_p)P.codes16;
        const u32 e_w = (u32)(tid >> 6) * (UL * 64) + (u32)lane;
        const u32 last = n - 1u;
        InT vn[UL];
        IdxT in[UL];
        auto load_full = [&](u32 r) { // one lane offset, immediate offsets
            const u32 e0 = r * span + e_w;
            const gchar_p pv = dbase + (size_t)(e0 * (u32)sizeof(InT)), pi = ibase + (size_t)(e0 * (u32)sizeof(IdxT));
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                vn[u] = *(gval_p)(pv + u * 64 * (int)sizeof(InT));
                in[u] = *(gidx_p)(pi + u * 64 * (int)sizeof(IdxT));
            }
        };
        auto load_clamped = [&](u32 r) { // the column's last, partial round
            const u32 e0 = r * span + e_w;
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const u32 e = min(e0 + u * 64u, last);
                vn[u] = *(gval_p)(dbase + (size_t)(e * (u32)sizeof(InT)));
                in[u] = *(gidx_p)(ibase + (size_t)(e * (u32)sizeof(IdxT)));
            }
        };
        // round r: its group codes are requested, then (PF) the next round's values / row indices, then it is counted.
        // Three copies of the body -- next round full / partial / none -- so that neither kind of request sits under a
        // condition inside the loop (the compiler merges two conditional request groups into one with 2 UL computed 64-bit
        // addresses).
        auto round = [&](u32 r, auto pf, auto partial) {
            InT v[UL];
            u32 cd[UL];
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                v[u] = vn[u];
                cd[u] = C16 ? (u32)*(gu16_p)(cbase + (size_t)((u32)in[u] * 2u)) : (u32)in[u]; // (n_cells < 2^30: host-checked)
            }
            if constexpr (decltype(pf)::value == 1) load_full(r + 1);
            if constexpr (decltype(pf)::value == 2) load_clamped(r + 1);
            const u32 e0 = r * span + e_w;
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const bool live = !decltype(partial)::value || e0 + u * 64u <= last;
                put(live ? v[u] : (InT)0, (int)cd[u]);
            }
        };
        typedef std::integral_constant<int, 0> I0;
        typedef std::integral_constant<int, 1> I1;
        typedef std::integral_constant<int, 2> I2;
        const u32 Rf = n / span; // full rounds; R - Rf = 0 or 1 partial round behind them
        if (Rf > 0) load_full(0);
        else if (R > 0) load_clamped(0);
        zero_tables();
        __syncthreads();
        for (u32 r = 0; r + 1 < Rf; ++r) round(r, I1(), I0());
        if (Rf > 0) {
            if (R > Rf) round(Rf - 1, I2(), I0());
            else round(Rf - 1, I0(), I0());
        }
        if (R > Rf) round(Rf, I0(), I1());
        if (MIXED) {
            n_ent = (u32)wave_sum((int)n_ent);
            if (lane == 0 && n_ent) atomicAdd(&s_entries, n_ent);
        }
        if (bad) s_bad = 1;
        __syncthreads();
        if (s_bad) { // uniform: this gene takes the general routes
            if (tid == 0) P.fallback[gene] = 1u;
            __syncthreads();
            continue;
        }
        { // wave 0: prefix counts, tie term and value sum of the selected histogram by lane = value; the weight words
            if (tid < 64) {
                const int c = tid;
                const u32 t = (c >= 1 && c < RT) ? hsel[c] : 0u;
                u32 inc = t; // inclusive scan over the values
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const u32 o = (u32)__shfl_up((int)inc, d);
                    if (lane >= d) inc += o;
                }
                const u32 lo = inc - t, run = (u32)__shfl((int)inc, 63);
                const u64 t64 = t;
                const u64 T = wave_sum<u64>(t64 * t64 * t64 - t64), sum = wave_sum<u64>(t64 * (u64)c);
                const long long n_sel = OVR ? P.n_cells : (long long)P.counts[OVR ? 0 : ref];
                const u32 z2 = 2u * (u32)(n_sel - (long long)run); // 2 zA (OVO) or 2 n0 (OVR)
                if (c < RT) {
                    wtab[c] = make_uint4(z2 + 2u * lo + t + (OVR ? 1u : 0u), 3u * t * t - 1u, 3u * t, 0u);
                    if (HAS_BIG || W16) cum[c] = lo;
                }
                if (c == 0) {
                    s_nnz = run; s_T = T; s_sum = sum;
                    if (OVR && P.gene_total) P.gene_total[gene] = (double)sum; // integer sums: exact whatever the order of addition
                }
            }
        }
        __syncthreads();
        const u64 nnz_sel = s_nnz, T_sel = s_T;
        const long long n_ref = OVR ? 0 : P.counts[OVR ? 0 : ref];
        const u64 zsel = (u64)((OVR ? P.n_cells : n_ref) - (long long)nnz_sel); // zA (OVO) or n0 (OVR)
        u32 cells_seen = 0;
        auto emit = [&](int g, long long two_u, u64 tie_sum, u64 sum_g) { // (integer value sums: counts)
            const size_t o = (size_t)gene * P.G_total + g; // (g: the group's number among all)
            if (P.pack16) { // (uniform) 16 bytes per test: a third less for this kernel to write and for k_finalize to read
                P.out_2u[o] = (long long)(((u64)sum_g << 40) | ((u64)two_u & 0xFFFFFFFFFFull));
                P.out_tie[o] = tie_sum;
            } else { P.out_2u[o] = two_u; P.out_tie[o] = tie_sum; P.out_sum[o] = (double)sum_g; }
        };
        for (int g = tid; g < G; g += NT) {
            const int gg = g_lo + g; // the group's number among all
            if (!OVR && gg == ref) {
                emit(gg, -2, 0, s_sum);
                continue;
            }
            // 32-bit inner terms (host-checked: n_ref < 30000 for OVO, n_cells < 2^30), one 32 x 32 -> 64 multiply-add each;
            // a word whose cells are empty for every lane of the wavefront is skipped.  The word loop stays rolled: unrolled,
            // the compiler hoists all 2 RT table reads into registers and spills 43 of them.
            u64 acc = 0, tie = 0;
            u32 nnz_g = 0, vsum = 0;
            const int bs = HAS_BIG ? (int)slot[g] : -1;
            auto cell = [&](int c, u32 tB) {
                nnz_g += tB;
                vsum += tB * (u32)c;
                { // A = 2 zsel + 2 cum[c] + tS (+ 1), B = 3 tS^2 - 1, C = 3 tS: tB (3 tS (tS + tB) + tB^2 - 1) = tB (B + tB (C + tB))
                    const uint4 w = wtab[c];
                    acc += (u64)tB * w.x;
                    if (!OVR) tie += (u64)tB * (u32)(w.y + tB * (w.z + tB));
                }
            };
            auto cell64 = [&](int c, u64 tB) { // a cell of a group of any size: 64-bit terms (3 tS (tS + tB) + tB^2 leaves 32 bits)
                const u64 tS = hsel[c], lo = cum[c];
                nnz_g += (u32)tB;
                vsum += (u32)tB * (u32)c;
                if (OVR) acc += tB * (2ull * zsel + 2ull * lo + tS + 1ull);
                else {
                    acc += tB * (2ull * zsel + 2ull * lo + tS);
                    tie += tB * (3ull * tS * (tS + tB) + tB * tB - 1ull);
                }
            };
            if (HAS_BIG && bs >= 0) { // 32-bit cells of their own
#pragma unroll 1
                for (int c = 1; c < RT; ++c) cell64(c, (u64)hbig[bs * RT + c]);
            }
            const bool packed = !HAS_BIG || bs < 0;
            // The words of the group, cell by cell (CsccRun: the values and counts of a word).  A word whose cells are empty for every
            // lane of the wavefront is skipped.  The word loops stay rolled (but for the two words of the mixed layout's 8-bit cells):
            // unrolled, the compiler hoists all 2 RT table reads into registers and spills 43 of them.
            typedef typename Cells::Lo Lo;
            typedef typename Cells::Hi Hi;
            if (MIXED) {
#pragma unroll
                for (int i = 0; i < Hi::FIRST; ++i) {
                    const u32 w = packed ? cscc_h[i * G + g] : 0u;
                    if (__ballot(w != 0) == 0ull) continue;
#pragma unroll
                    for (int k = 0; k < Lo::PER; ++k) cell(Lo::value(i, k), Lo::count(w, k));
                }
#pragma unroll 1
                for (int i = Hi::FIRST; i < WPG; ++i) {
                    const u32 w = packed ? cscc_h[i * G + g] : 0u;
                    if (__ballot(w != 0) == 0ull) continue;
#pragma unroll
                    for (int k = 0; k < Hi::PER; ++k) cell(Hi::value(i, k), Hi::count(w, k));
                }
                if (packed) cells_seen += nnz_g;
            } else {
#pragma unroll 1
                for (int i = 0; i < WPG; ++i) {
                    const u32 w = packed ? cscc_h[i * G + g] : 0u;
                    if (__ballot(w != 0) == 0ull) continue;
#pragma unroll
                    for (int k = 0; k < Lo::PER; ++k) {
                        const u32 tB = Lo::count(w, k);
                        if (!W16) cell(Lo::value(i, k), tB);
                        else if (tB) cell64(Lo::value(i, k), (u64)tB);
                    }
                }
            }
            const long long n_g = P.counts[gg];
            const u64 zB = (u64)(n_g - (long long)nnz_g);
            if (OVR) {
                acc += zB * (zsel + 1ull);
                emit(gg, 2ll * (P.n_cells - n_g) * n_g + n_g * (n_g + 1) - (long long)acc, P.tie_f64 ? tie_f64_sparse(T_sel, (long long)zsel) : T_sel + (zsel * zsel * zsel - zsel), (u64)vsum);
            } else {
                acc += zB * zsel;
                const u64 t0 = zsel + zB;
                emit(gg, 2ll * n_ref * n_g - (long long)acc, T_sel + tie + (t0 * t0 * t0 - t0), (u64)vsum);
            }
        }
        if (MIXED) {
            cells_seen = (u32)wave_sum((int)cells_seen);
            if (lane == 0 && cells_seen) atomicAdd(&s_cells, cells_seen);
            __syncthreads();
            if (tid == 0 && s_cells != s_entries) P.fallback[gene] = 2u; // a 4-bit cell overflowed: the 8-bit form redoes this gene
        }
        __syncthreads();
    }
}
