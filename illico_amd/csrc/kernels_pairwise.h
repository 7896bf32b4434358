// All-pairs Wilcoxon rank-sum tests from per-(group, gene) value histograms -- illico_group_value_hists_* and
// illico_pairwise_from_hists (pairwise.hip).
//
// For count-valued data U, the tie term and the value sum of a test are functions of the two groups' value histograms alone
// (kernels_group_hists.h).  With h_g[c], h_r[c] the counts of value c in group g and in the reference r, cum_r[c] = sum_{c' < c} h_r[c']:
//     S2   = sum_c h_g[c] (cum_r[c] + cum_r[c + 1])
//     U    = 0.5 (double)(2 n_r n_g - S2)                  the reference's U, as every OVO route reports it
//     tie  = (double) sum_c (t^3 - t),  t = h_g[c] + h_r[c]   (the same integer as T_A + 3 TT of k_emit_from_group_hists)
//     S    = sum_c c h[c]                                  the value sums of the fold change
// and p, z follow from pval_device_pre / zscore_device_pre with group_const(n_r, n_g, n_r + n_g) (kernels_finalize.h): the same
// integers and the same functions as the OVO routes, so bit for bit their planes.  One read of X gives the histograms of all groups;
// every ordered pair (g, r) follows from them.  The integer sums fit 64 bits while n_g + n_r < 2^21.
//
// Layouts.  The caller sees H as uint32 [G][W][PW_RT] (a gene's table is 1 KB, contiguous).  The kernels whose lane is a gene
// (k_group_value_hists, k_pw_pairs) work on [g][tile][value][lane], tile = 64 consecutive genes: k_pw_transpose goes between the two.
#pragma once
#include "kernels_group_hists.h"

#define PW_NT 256
#define PW_RT 256 // values 0 .. 255
#define PW_RB 4   // references per wavefront of k_pw_pairs
#define PW_TILE_WORDS (PW_RT * 64)

// [k][tile][value][lane] <-> [g][gene][value]; grid (tiles, K), g = sel ? sel[k] : k.  64 x 64 words at a time through LDS: both
// sides move whole 256-byte segments.
template <bool TO_PUBLIC>
static __global__ __launch_bounds__(PW_NT) void k_pw_transpose(u32 *__restrict__ pub, u32 *__restrict__ tiled, const int *__restrict__ sel, int W, int tiles) {
    __shared__ u32 t[64][65]; // [value][lane]
    const int tile = blockIdx.x, k = blockIdx.y, g = sel ? sel[k] : k;
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6; // hi 0..3
    u32 *tb = tiled + ((size_t)k * tiles + tile) * PW_TILE_WORDS;
    u32 *pb = pub + ((size_t)g * W + (size_t)tile * 64) * PW_RT;
    const int ngene = min(64, W - tile * 64);
    for (int q = 0; q < PW_RT / 64; ++q) {
        if (TO_PUBLIC) {
            for (int v = hi; v < 64; v += 4) t[v][lo] = tb[(q * 64 + v) * 64 + lo];
        } else {
            for (int l = hi; l < 64; l += 4) t[lo][l] = l < ngene ? pb[(size_t)l * PW_RT + q * 64 + lo] : 0u;
        }
        __syncthreads();
        if (TO_PUBLIC) {
            for (int l = hi; l < ngene; l += 4) pb[(size_t)l * PW_RT + q * 64 + lo] = t[lo][l];
        } else {
            for (int v = hi; v < 64; v += 4) tb[(q * 64 + v) * 64 + lo] = t[v][lo];
        }
        __syncthreads();
    }
}

// ---- sparse input: the dense answer (a stored zero counts in bin 0, the cells that are not stored too) ----

// CSC: one workgroup per gene.  Counts go to an LDS table [gw groups][256 values] (dynamic LDS: gw KB), group window after group
// window (each window walks the column again); a window's tables leave as whole 1 KB rows of H.  A stored value that is no integer in
// [0, 255], or a row index outside the matrix, flags the gene.
template <typename InT, typename IdxT>
static __global__ __launch_bounds__(PW_NT) void k_pw_hists_csc(const InT *__restrict__ data, const IdxT *__restrict__ indices, const IdxT *__restrict__ indptr,
                                                               long long kshift, long long col0, const int *__restrict__ codes, const int *__restrict__ counts,
                                                               long long N, int G, int W, int gw, u32 *__restrict__ H, u32 *__restrict__ flags) {
    extern __shared__ u32 pw_tab[]; // [gw][PW_RT]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = blockIdx.x; j < W; j += gridDim.x) {
        const long long k0 = (long long)indptr[col0 + j], k1 = (long long)indptr[col0 + j + 1];
        bool bad = false;
        for (int g0 = 0; g0 < G; g0 += gw) {
            const int ng = min(gw, G - g0);
            for (int i = tid; i < ng * PW_RT; i += PW_NT) pw_tab[i] = 0u;
            __syncthreads();
            for (long long k = k0 + tid; k < k1; k += PW_NT) {
                const long long row = (long long)indices[k - kshift];
                if ((unsigned long long)row >= (unsigned long long)N) { bad = true; continue; }
                const int g = codes[row] - g0;
                if ((unsigned)g >= (unsigned)ng) continue;
                bool exact;
                const u32 c = clamp_count<InT, PW_RT>(data[k - kshift], exact);
                if (!exact) bad = true;
                atomicAdd(&pw_tab[g * PW_RT + (int)c], 1u);
            }
            __syncthreads();
            for (int g = wave; g < ng; g += PW_NT / 64) { // a wavefront per group: its row of H, bin 0 completed by the cells not stored
                u32 v[PW_RT / 64], stored = 0;
#pragma unroll
                for (int i = 0; i < PW_RT / 64; ++i) { v[i] = pw_tab[g * PW_RT + i * 64 + lane]; stored += v[i]; }
                for (int o = 32; o; o >>= 1) stored += __shfl_xor(stored, o, 64);
                if (lane == 0) v[0] += (u32)counts[g0 + g] - stored;
                u32 *h = H + ((size_t)(g0 + g) * W + j) * PW_RT + lane;
#pragma unroll
                for (int i = 0; i < PW_RT / 64; ++i) h[i * 64] = v[i];
            }
            __syncthreads();
        }
        if (__syncthreads_or(bad ? 1 : 0) && tid == 0) flags[j] = 1u;
    }
}

// CSR: a wavefront per row, rows in any order, entries filtered to the gene window; counts go to H (zeroed by the host) with
// returnless global atomics.  k_pw_hists_bin0 then completes bin 0.
template <typename InT, typename IdxT>
static __global__ __launch_bounds__(PW_NT) void k_pw_hists_csr(const InT *__restrict__ data, const IdxT *__restrict__ indices, const IdxT *__restrict__ indptr,
                                                               long long kshift, long long col0, const int *__restrict__ codes, long long N, int G, int W,
                                                               u32 *__restrict__ H, u32 *__restrict__ flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long row = (long long)blockIdx.x * (PW_NT / 64) + wave; row < N; row += (long long)gridDim.x * (PW_NT / 64)) {
        const int g = codes[row];
        if ((unsigned)g >= (unsigned)G) continue;
        const long long k0 = (long long)indptr[row], k1 = (long long)indptr[row + 1];
        for (long long k = k0 + lane; k < k1; k += 64) {
            const long long col = (long long)indices[k - kshift] - col0;
            if ((unsigned long long)col >= (unsigned long long)W) continue;
            bool exact;
            const u32 c = clamp_count<InT, PW_RT>(data[k - kshift], exact);
            if (!exact) flags[col] = 1u;
            else atomicAdd(&H[((size_t)g * W + (size_t)col) * PW_RT + c], 1u);
        }
    }
}
// bin 0 of every (group, gene) row of H += counts[g] - (the row's sum): a wavefront per row
static __global__ __launch_bounds__(PW_NT) void k_pw_hists_bin0(u32 *__restrict__ H, const int *__restrict__ counts, long long rows, int W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long r = (long long)blockIdx.x * (PW_NT / 64) + wave; r < rows; r += (long long)gridDim.x * (PW_NT / 64)) {
        u32 *h = H + (size_t)r * PW_RT;
        u32 stored = 0;
#pragma unroll
        for (int i = 0; i < PW_RT / 64; ++i) stored += h[i * 64 + lane];
        for (int o = 32; o; o >>= 1) stored += __shfl_xor(stored, o, 64);
        if (lane == 0) h[0] += (u32)counts[r / W] - stored;
    }
}

// ---- the pairs ----
struct PwParams {
    const u32 *T;          // [K][tiles][PW_RT][64] histograms of the selected groups
    const u32 *gene_flags; // [W] non-zero: the gene's planes are left untouched
    const long long *n;    // [K] sizes of the selected groups
    const int *sel;        // [K] their group ids (rows of sums)
    const double *sums;    // optional [G][sums_ld] value sums of the fold change; null: sum_c c h[c]
    long long sums_ld;
    int K, W, tiles, nrb;  // nrb = ceil(K / PW_RB)
    int use_continuity, tie_correct, alternative;
    double *out_p, *out_u, *out_fc, *out_z; // [K][K][out_ld]: [r][g][gene], group sel[g] against reference sel[r]
    long long out_ld;
};

// grid (ceil(K nrb / 4), tiles): the workgroups of one tile are neighbours in launch order, so the tile's K x 64 KB of histograms are
// read from HBM once and served from L2 after that.  A wavefront takes one group g and PW_RB references: it walks the 256 values once,
// lane = gene, with S2, the tie sum, the reference's running cumulative count and value sum of each pair in registers, then writes its
// PW_RB x (3 or 4) output segments of 512 bytes.
template <bool Z>
static __global__ __launch_bounds__(PW_NT) void k_pw_pairs(PwParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.y, unit = (int)blockIdx.x * (PW_NT / 64) + wave;
    if (unit >= P.K * P.nrb) return;
    const int g = unit / P.nrb, r0 = (unit % P.nrb) * PW_RB;
    const int gene = tile * 64 + lane;
    if (gene >= P.W || P.gene_flags[gene] != 0u) return;
    const u32 *hg = P.T + ((size_t)g * P.tiles + tile) * PW_TILE_WORDS + lane;
    const u32 *hr[PW_RB];
#pragma unroll
    for (int j = 0; j < PW_RB; ++j) hr[j] = P.T + ((size_t)min(r0 + j, P.K - 1) * P.tiles + tile) * PW_TILE_WORDS + lane;
    u64 S2[PW_RB], TT[PW_RB], SR[PW_RB], SG = 0;
    u32 cum[PW_RB];
#pragma unroll
    for (int j = 0; j < PW_RB; ++j) { S2[j] = 0; TT[j] = 0; SR[j] = 0; cum[j] = 0; }
#pragma unroll 4
    for (int c = 0; c < PW_RT; ++c) {
        const u32 a = hg[c * 64];
        SG += (u64)a * (u32)c;
#pragma unroll
        for (int j = 0; j < PW_RB; ++j) {
            const u32 b = hr[j][c * 64];
            const u32 lo = cum[j], hi = lo + b;
            cum[j] = hi;
            S2[j] += (u64)a * (u64)(lo + hi);
            const u64 t = (u64)a + (u64)b;
            TT[j] += t * t * t - t;
            SR[j] += (u64)b * (u32)c;
        }
    }
    const double cc = P.use_continuity ? 0.5 : 0.0;
    const long long n_g = P.n[g];
    const double sum_g = P.sums ? P.sums[(size_t)P.sel[g] * P.sums_ld + gene] : (double)SG;
#pragma unroll
    for (int j = 0; j < PW_RB; ++j) {
        const int r = r0 + j;
        if (r >= P.K) break;
        const long long n_r = P.n[r];
        const GroupConst gc = group_const(n_r, n_g, n_r + n_g);
        const long long two_u = 2ll * n_r * n_g - (long long)S2[j];
        const double U = 0.5 * (double)two_u;
        const double tie = P.tie_correct ? (double)TT[j] : 0.0;
        double pv = 1.0, z = 0.0;
        if (r != g) {
            pv = pval_device_pre(gc.nnn, gc.var0, gc.n12, tie, U, gc.mu, cc, P.alternative);
            if constexpr (Z) z = zscore_device_pre(gc.nnn, gc.var0, tie, U, gc.mu);
        }
        const double sum_r = P.sums ? P.sums[(size_t)P.sel[r] * P.sums_ld + gene] : (double)SR[j];
        const size_t o = ((size_t)r * P.K + g) * P.out_ld + gene;
        P.out_p[o] = pv;
        P.out_u[o] = U;
        P.out_fc[o] = fold_change_device(sum_g, sum_r, gc);
        if constexpr (Z) P.out_z[o] = z;
    }
}
