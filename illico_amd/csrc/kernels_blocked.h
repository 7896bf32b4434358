// Blocked Wilcoxon rank-sum tests: a test spread over B blocks (batches, donors, plates), the per-block tests combined by a weighted
// Stouffer sum on the device -- illico_blocked_from_hists / illico_blocked_from_planes (blocked.hip; include/illico_hip_blocked.h states
// the definition).
//
// Compound groups k = g * B + b.  In a block b that holds n_g > 0 cells of g and n_r > 0 reference cells (those of the group ref, or
// with ref < 0 the cells of b that are not g) the block is USED, and with gc = group_const(n_r, n_g, n_r + n_g)
//     U_b, tie_b   as kernels_pairwise.h forms them from the two histograms        z_b = zscore_device_pre(gc.nnn, gc.var0, tie_b, U_b, gc.mu)
//     w_b = (double)(n_g n_r)
// blk_fold adds a used block to the accumulators, in ascending b; blk_finish turns them into the four plane values.  The two feeders
// -- k_blk_from_hists (the statistics of a block from its histograms) and k_blk_from_planes (z_b, U_b read from the planes of B engine
// calls) -- share both, so they cannot drift apart.  Lane = gene in both: every plane access is a whole 512-byte segment.
#pragma once
#include "kernels_pairwise.h"

struct BlkAcc {
    double wz = 0.0, ww = 0.0, u = 0.0, w = 0.0, sg = 0.0, sr = 0.0, z1 = 0.0;
    long long ng = 0, nr = 0;
    int nb = 0;
};
struct BlkOut { double p, stat, fc, z; };

__device__ __forceinline__ void blk_fold(BlkAcc &a, double z_b, double w_b, double U_b, long long n_g, long long n_r, double S_g, double S_r) {
    if (a.nb == 0) a.z1 = z_b;
    a.wz += w_b * z_b;
    a.ww += w_b * w_b;
    a.u += U_b;
    a.w += w_b;
    a.sg += S_g;
    a.sr += S_r;
    a.ng += n_g;
    a.nr += n_r;
    a.nb += 1;
}
// Z = (sum w z) / sqrt(sum w^2); over ONE used block that is z_b itself, and z_b is returned rather than the rounded (w z) / w: the
// row of a single block is the row of the unblocked call, bit for bit.  No used block: NaN in every plane.
__device__ __forceinline__ BlkOut blk_finish(const BlkAcc &a, int alternative) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (a.nb == 0) return {nan, nan, nan, nan};
    const double Z = a.nb == 1 ? a.z1 : a.wz / sqrt(a.ww);
    double p;
    if (alternative == 0) p = erfc(fabs(Z) / sqrt(2.0));
    else if (alternative == 2) p = 0.5 * erfc(-Z / sqrt(2.0));
    else p = 0.5 * erfc(Z / sqrt(2.0));
    const double mu_g = a.sg / (double)a.ng, mu_r = a.sr / (double)a.nr;
    return {p, a.u, (mu_r == 0.0) ? __longlong_as_double(0x7FF0000000000000ll) : mu_g / mu_r, Z};
}
// the reference group's own row, as k_finalize writes it
__device__ __forceinline__ BlkOut blk_reference_row(BlkOut o) { return {1.0, -1.0, o.fc, 0.0}; }

struct BlkParams {
    const long long *n;     // [G][B] compound sizes
    const long long *ntot;  // [B] cells of each block
    const double *sums;     // optional [G * B][sums_ld] compound value sums
    const double *stot;     // [B][W] their totals per block: ref < 0 with sums, else null
    long long sums_ld;
    int G, B, W, ref;       // ref < 0: the rest of the block
    int alternative;
    double *out_p, *out_u, *out_fc, *out_z; // [G][out_ld]; out_fc may be null (k_blk_from_planes without sums)
    long long out_ld;
    // k_blk_from_hists
    const u32 *T;           // [G * B][tiles][PW_RT][64] tiled histograms of the compound groups
    const u32 *TOT;         // [B][tiles][PW_RT][64] their sums over the groups of a block: ref < 0, else null
    const u32 *gene_flags;  // [W] non-zero: the gene's planes are left untouched
    int tiles, tie_correct;
    // k_blk_from_planes
    const double *z, *U;    // [B][G][in_ld]
    const int *row_map;     // [B][G] the row of group g in block b's plane set, or -1
    long long in_ld;
};

// TOT[b][tile] = sum_g T[g * B + b][tile], word by word; grid (tiles, B)
static __global__ __launch_bounds__(PW_NT) void k_blk_block_totals(const u32 *__restrict__ T, u32 *__restrict__ TOT, int G, int B, int tiles) {
    const int tile = blockIdx.x, b = blockIdx.y;
    u32 *dst = TOT + ((size_t)b * tiles + tile) * PW_TILE_WORDS;
    for (int i = threadIdx.x; i < PW_TILE_WORDS; i += PW_NT) {
        u32 t = 0;
        for (int g = 0; g < G; ++g) t += T[(((size_t)g * B + b) * tiles + tile) * PW_TILE_WORDS + i];
        dst[i] = t;
    }
}
// stot[b][gene] = sum_g sums[g * B + b][gene], in group order; one thread per (b, gene)
static __global__ __launch_bounds__(256) void k_blk_sum_totals(const double *__restrict__ sums, long long sums_ld, double *__restrict__ stot, int G, int B, int W) {
    const int gene = (int)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (gene >= W) return;
    double t = 0.0;
    for (int g = 0; g < G; ++g) t += sums[((size_t)g * B + b) * (size_t)sums_ld + gene];
    stot[(size_t)b * W + gene] = t;
}

// the sizes of test (g, block b): false when the block is not used
__device__ __forceinline__ bool blk_sizes(const BlkParams &P, int g, int b, long long &n_g, long long &n_r) {
    n_g = P.n[(size_t)g * P.B + b];
    n_r = P.ref >= 0 ? P.n[(size_t)P.ref * P.B + b] : P.ntot[b] - n_g;
    return n_g > 0 && n_r > 0;
}
// the value sums of test (g, block b) from the sums plane
__device__ __forceinline__ void blk_plane_sums(const BlkParams &P, int g, int b, int gene, double &S_g, double &S_r) {
    S_g = P.sums[((size_t)g * P.B + b) * (size_t)P.sums_ld + gene];
    S_r = P.ref >= 0 ? P.sums[((size_t)P.ref * P.B + b) * (size_t)P.sums_ld + gene] : P.stot[(size_t)b * P.W + gene] - S_g;
}
__device__ __forceinline__ void blk_store(const BlkParams &P, int g, int gene, BlkOut o) {
    if (g == P.ref) o = blk_reference_row(o);
    const size_t at = (size_t)g * (size_t)P.out_ld + gene;
    P.out_p[at] = o.p;
    P.out_u[at] = o.stat;
    if (P.out_fc) P.out_fc[at] = o.fc;
    P.out_z[at] = o.z;
}

// grid (ceil(G / 4), tiles): the wavefronts of one tile are neighbours in launch order, so the reference's B tables of the tile (or the
// B tables of block totals) come from HBM once and from L2 after that.  A wavefront takes one test g, lane = gene, and walks its used
// blocks; in each it walks the 256 values once with S2, the tie sum, the reference's running count and the two value sums in registers.
static __global__ __launch_bounds__(PW_NT) void k_blk_from_hists(const BlkParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.y, g = (int)blockIdx.x * (PW_NT / 64) + wave;
    if (g >= P.G) return;
    const int gene = tile * 64 + lane;
    if (gene >= P.W || P.gene_flags[gene] != 0u) return;
    const bool rest = P.ref < 0;
    BlkAcc acc;
    for (int b = 0; b < P.B; ++b) {
        long long n_g, n_r;
        if (!blk_sizes(P, g, b, n_g, n_r)) continue;
        const u32 *hg = P.T + (((size_t)g * P.B + b) * P.tiles + tile) * PW_TILE_WORDS + lane;
        const u32 *hr = rest ? P.TOT + ((size_t)b * P.tiles + tile) * PW_TILE_WORDS + lane
                             : P.T + (((size_t)P.ref * P.B + b) * P.tiles + tile) * PW_TILE_WORDS + lane;
        u64 S2 = 0, TT = 0, SG = 0, SR = 0;
        u32 cum = 0;
#pragma unroll 8
        for (int c = 0; c < PW_RT; ++c) {
            const u32 a = hg[c * 64], q = hr[c * 64];
            const u32 r = rest ? q - a : q;
            const u32 lo = cum, hi = lo + r;
            cum = hi;
            S2 += (u64)a * (u64)(lo + hi);
            const u64 t = (u64)a + (u64)r;
            TT += t * t * t - t;
            SG += (u64)a * (u32)c;
            SR += (u64)r * (u32)c;
        }
        const GroupConst gc = group_const(n_r, n_g, n_r + n_g);
        const double U = 0.5 * (double)(2ll * n_r * n_g - (long long)S2);
        const double tie = P.tie_correct ? (double)TT : 0.0;
        double S_g = (double)SG, S_r = (double)SR;
        if (P.sums) blk_plane_sums(P, g, b, gene, S_g, S_r);
        blk_fold(acc, zscore_device_pre(gc.nnn, gc.var0, tie, U, gc.mu), (double)(n_r * n_g), U, n_g, n_r, S_g, S_r);
    }
    blk_store(P, g, gene, blk_finish(acc, P.alternative));
}

// grid (ceil(W / 256), G): one thread per (test, gene); reads and writes are coalesced along genes
static __global__ __launch_bounds__(256) void k_blk_from_planes(const BlkParams P) {
    const int gene = (int)blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    if (gene >= P.W) return;
    BlkAcc acc;
    for (int b = 0; b < P.B; ++b) {
        long long n_g, n_r;
        const int row = P.row_map[(size_t)b * P.G + g];
        if (!blk_sizes(P, g, b, n_g, n_r) || row < 0) continue;
        const size_t at = ((size_t)b * P.G + row) * (size_t)P.in_ld + gene;
        double S_g = 0.0, S_r = 0.0;
        if (P.sums) blk_plane_sums(P, g, b, gene, S_g, S_r);
        blk_fold(acc, P.z[at], (double)(n_r * n_g), P.U[at], n_g, n_r, S_g, S_r);
    }
    blk_store(P, g, gene, blk_finish(acc, P.alternative));
}
