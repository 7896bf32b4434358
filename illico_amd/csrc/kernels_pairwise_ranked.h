// All-pairs Wilcoxon rank-sum tests for ANY values of a 4-byte type from one sorted walk per gene -- illico_pairwise_ranked_*
// (pairwise_ranked.hip).  The histogram pair route (kernels_pairwise.h) takes the genes whose values are the
// integers 0 .. 255; this one takes the others.
//
// For one gene and the selected groups k = 0 .. K - 1 of sizes n_k, over the distinct values v in ascending order (zero among them,
// -0.0 tied with it as key_of folds it), t_k(v) the cells of k that hold v, c_k(v) = sum_{v' < v} t_k(v'):
//     L[g][r] = sum_v t_g(v) c_r(v)            the pairs with x_r < x_g
//     T[k]    = sum_v (t_k^3 - t_k)
//     X[g][r] = sum_v t_g t_r (t_g + t_r)      symmetric
//     S2[g][r]  = n_g n_r + L[g][r] - L[r][g]  ( = sum_v t_g (2 c_r + t_r), the S2 of kernels_pairwise.h)
//     tie[g][r] = T[g] + T[r] + 3 X[g][r]      ( = sum_v ((t_g + t_r)^3 - (t_g + t_r)))
// all of them integers that fit 64 bits while n_g + n_r < 2^21.  The zeros are never records: with neg_k / pos_k the negative / positive
// cells of k and z_k = n_k - neg_k - pos_k, at the end L[g][r] += pos_g z_r + z_g neg_r, T[k] += z_k^3 - z_k, X[g][r] += z_g z_r (z_g + z_r).
//
// k_pw_rank_pairs walks the value-range parts k_ovr_partition wrote (kernels_ovr_partition.h: (key, group code) records of the non-zeros, part
// after part in value order, a part at most `cap` records): one workgroup per gene, drawn from a queue, its parts one after the other.
// A part's records of selected groups go to LDS as u64 (key << 32 | slot) and are sorted there (block_sort_hybrid).  The sixteen
// wavefronts split the sorted part into stretches cut at key changes; a small histogram per stretch gives each wavefront the counts
// c[] its stretch starts from.  In the walk lane = reference slot r: c[r] is a register, frozen inside a tie block while a pending
// vector collects the block's counts; a record of group g is ONE LDS add, K lanes wide at consecutive addresses: L[g][r] += c[r].  At a
// key change the pending vector is committed (c += pending) and, if the block held more than one record, T and -- for the groups
// present -- X are updated.  A part beyond the record slots is a crowded coarse bucket that got a part of its own
// (ovrp_assign_parts_skewed): one value is counted per group and taken as one tie block, different values send the gene away.
// k_pw_rank_emit turns the [gene][K * K] integers into the planes with the functions of kernels_finalize.h -- the same integers and the
// same functions as the one-versus-reference routes and the histogram pair route.
#pragma once
#include "common.h"
#include "kernels_ovr_partition.h"
#include "kernels_finalize.h"

#define PWR_NT 1024
#define PWR_KMAX 64   // selected groups at most: lane = reference slot, and L / X take K * K * 16 bytes of LDS
#define PWR_SORT_K 16 // keys per lane of the register sort phases: 1024-record chunks
// why a gene left the route (out_left)
#define PWR_LEFT_PARTITION 1u // the partition could not split it (gene_info flag)
#define PWR_LEFT_PART 2u      // a part beyond the record slots holds different values
#define PWR_LEFT_NAN 3u       // it holds a NaN

struct PwRankParams {
    const u32 *pkeys;      // [nb][pstride] non-zero keys, part after part
    const u16 *pcodes;     // [nb][pstride] their group codes
    long long pstride;
    const u32 *part_start; // [nb][OVRP_PMAX + 1]
    const u32 *gene_info;  // [nb][4] non-zeros, negatives, parts, flag
    const int *slot_of;    // [G] slot of a group code among the selected ones, or -1
    const long long *n;    // [K] sizes of the selected groups
    u32 *gene_counter;     // queue head (zeroed by the host)
    int nb, K, cap;        // cap: record slots, a multiple of 1024
    int is_float;          // float32 keys: a key beyond +-inf is a NaN
    long long *out_s2;     // [nb][K * K]: S2 of group g against reference r at r * K + g
    u64 *out_tie;          // [nb][K * K]
    u32 *left;             // [nb] 0, or why the gene left
};

// bytes beside L, X and the records: T [64] | carry, neg [64] each | per-wavefront counts [16][64] | stretch starts | words
#define PWR_FIXED_LDS (512 + 256 + 256 + (PWR_NT / 64) * 256 + 128 + 64)
static inline int pwr_record_cap(int K, size_t lds_max) {
    return (int)(((lds_max - (size_t)K * K * 16 - PWR_FIXED_LDS) / 8) & ~(size_t)1023);
}
static inline size_t pwr_lds_bytes(int K, int cap) { return (size_t)K * K * 16 + PWR_FIXED_LDS + (size_t)cap * 8; }

// the end of a tie block of `blen` records whose per-group counts are `pend` (lane = slot): T, X for the groups present, c += pend
__device__ __forceinline__ void pwr_commit(u32 &c, u32 &pend, u32 &blen, u64 *T, u64 *X, int K, int lane) {
    if (blen > 1u) { // (uniform)
        const u64 p = pend;
        if (pend > 1u) atomicAdd(&T[lane], p * p * p - p);
        u64 m = __ballot(pend > 0u);
        if (m & (m - 1ull)) {
            while (m) {
                const int g = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                m &= m - 1ull;
                const u64 tg = (u32)__builtin_amdgcn_readlane((int)pend, g);
                if (pend > 0u && lane != g) atomicAdd(&X[g * K + lane], tg * p * (tg + p));
            }
        }
    }
    c += pend;
    pend = 0u;
    blen = 0u;
}

__global__ __launch_bounds__(PWR_NT) void k_pw_rank_pairs(PwRankParams P) {
    constexpr int NT = PWR_NT, NW = NT / 64;
    constexpr u32 ZEROK = KeyInfo<u32>::ZEROK;
    extern __shared__ __align__(16) unsigned char smem[];
    const int K = P.K, KK = K * K;
    u64 *L = (u64 *)smem;               // [K][K]
    u64 *X = L + KK;                    // [K][K]
    u64 *T = X + KK;                    // [64]
    u32 *carry = (u32 *)(T + 64);       // [64] records of each slot in the parts walked so far
    u32 *negc = carry + 64;             // [64] ... of them below zero
    u32 *wcnt = negc + 64;              // [NW][64] records of each slot in a wavefront's stretch
    int *wstart = (int *)(wcnt + NW * 64); // [NW + 1]
    u32 *s_misc = (u32 *)(wstart + 32); // [0] records taken  [1] NaN seen  [2] queue slot  [4], [5] smallest / largest key of a long part
    u64 *A = (u64 *)(smem + (size_t)KK * 16 + PWR_FIXED_LDS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 nan_hi = 0xFF800000u, nan_lo = 0x007FFFFFu; // key_of(+inf), key_of(-inf)

    for (;;) {
        if (tid == 0) s_misc[2] = atomicAdd(P.gene_counter, 1u);
        __syncthreads();
        const int gene = (int)s_misc[2];
        __syncthreads();
        if (gene >= P.nb) break;
        const u32 *gi = P.gene_info + (size_t)gene * 4;
        if (gi[3] != 0u) { // (uniform)
            if (tid == 0) P.left[gene] = PWR_LEFT_PARTITION;
            __syncthreads(); // (thread 0 stays with the workgroup: without it the compiler lets the other lanes run on to the queue's barrier)
            continue;
        }
        const int n_parts = (int)gi[2];
        const u32 *ps = P.part_start + (size_t)gene * (OVRP_PMAX + 1);
        for (int i = tid; i < 2 * KK; i += NT) L[i] = 0ull; // L and X
        if (tid < 64) { T[tid] = 0ull; carry[tid] = 0u; negc[tid] = 0u; }
        __syncthreads();
        u32 bad = 0u;
        for (int part = 0; part < n_parts; ++part) {
            const u32 base = ps[part];
            const int n = (int)(ps[part + 1] - base);
            if (n == 0) continue;
            const long long k0 = (long long)gene * P.pstride + base;
            if (n > P.cap) { // (uniform) a crowded coarse bucket with a part of its own
                if (tid == 0) { s_misc[4] = 0xFFFFFFFFu; s_misc[5] = 0u; }
                if (tid < 64) wcnt[tid] = 0u;
                __syncthreads();
                u32 tmin = 0xFFFFFFFFu, tmax = 0u;
                for (int i = tid; i < n; i += NT) {
                    const u32 key = P.pkeys[k0 + i];
                    tmin = min(tmin, key);
                    tmax = max(tmax, key);
                }
                tmin = wave_min_key(tmin);
                tmax = wave_max_key(tmax);
                if (lane == 0) { atomicMin(&s_misc[4], tmin); atomicMax(&s_misc[5], tmax); }
                __syncthreads();
                const u32 q = s_misc[4];
                if (s_misc[5] != q) { bad = PWR_LEFT_PART; break; }
                if (P.is_float && (q > nan_hi || q < nan_lo)) { bad = PWR_LEFT_NAN; break; }
                for (int i = tid; i < n; i += NT) {
                    const int s = P.slot_of[P.pcodes[k0 + i]];
                    if (s >= 0) atomicAdd(&wcnt[s], 1u);
                }
                __syncthreads();
                if (wave == 0) { // one tie block: every record of g stands above c[r] records of r
                    u32 pend = wcnt[lane], c = carry[lane], blen = 0u;
                    u64 m = __ballot(pend > 0u);
                    while (m) {
                        const int g = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                        m &= m - 1ull;
                        const u32 tg = (u32)__builtin_amdgcn_readlane((int)pend, g);
                        blen += tg;
                        if (lane < K && c) atomicAdd(&L[g * K + lane], (u64)tg * (u64)c);
                    }
                    if (q < ZEROK) negc[lane] += pend;
                    pwr_commit(c, pend, blen, T, X, K, lane);
                    carry[lane] = c;
                }
                __syncthreads();
                continue;
            }
            // ---- the part's records of selected groups -> LDS ----
            const int ncap = (n + 1023) & ~1023;
            for (int i = tid; i < NW * 64; i += NT) wcnt[i] = 0u;
            if (tid == 0) { s_misc[0] = 0u; s_misc[1] = 0u; }
            __syncthreads();
            {
                u32 taken = 0u;
                bool nan = false;
                for (int i = tid; i < ncap; i += NT) {
                    u64 rec = ~0ull; // sorts behind every record
                    if (i < n) {
                        const u32 key = P.pkeys[k0 + i];
                        const int s = P.slot_of[P.pcodes[k0 + i]];
                        nan |= P.is_float && (key > nan_hi || key < nan_lo);
                        if (s >= 0) { rec = ((u64)key << 32) | (u32)s; ++taken; }
                    }
                    A[i] = rec;
                }
                taken = (u32)wave_sum((int)taken);
                if (lane == 0 && taken) atomicAdd(&s_misc[0], taken);
                if (__any(nan) && lane == 0) s_misc[1] = 1u;
            }
            __syncthreads();
            if (s_misc[1]) { bad = PWR_LEFT_NAN; break; } // (uniform)
            const int nv = (int)s_misc[0];
            block_sort_hybrid<u64, NT, PWR_SORT_K>(A, ncap, tid);
            // ---- stretches: the wavefront's even share, moved on to the next key change ----
            {
                const int per = (nv + NW - 1) / NW;
                int p = min(wave * per, nv);
                while (p > 0 && p < nv) { // (uniform per wavefront)
                    const int i = p + lane;
                    const bool head = i < nv && (u32)(A[i] >> 32) != (u32)(A[i - 1] >> 32);
                    const u64 m = __ballot(head);
                    if (m) { p += __ffsll((long long)m) - 1; break; }
                    p = min(p + 64, nv);
                }
                if (lane == 0) wstart[wave] = p;
                if (tid == 0) wstart[NW] = nv;
            }
            __syncthreads();
            const int s0 = __builtin_amdgcn_readfirstlane(wstart[wave]), e0 = __builtin_amdgcn_readfirstlane(wstart[wave + 1]);
            for (int i = s0 + lane; i < e0; i += 64) {
                const u64 rec = A[i];
                const u32 slot = (u32)rec & 63u;
                atomicAdd(&wcnt[wave * 64 + slot], 1u);
                if ((u32)(rec >> 32) < ZEROK) atomicAdd(&negc[slot], 1u);
            }
            __syncthreads();
            // ---- the walk ----
            {
                u32 c = carry[lane];
                for (int w = 0; w < wave; ++w) c += wcnt[w * 64 + lane];
                u32 pend = 0u, blen = 0u, cur = 0u;
                for (int i0 = s0; i0 < e0; i0 += 64) {
                    const int i = i0 + lane;
                    const u64 rec = i < e0 ? A[i] : 0ull;
                    const int rk = (int)(u32)(rec >> 32), rs = (int)(u32)rec;
                    const int cnt = min(64, e0 - i0);
                    for (int j = 0; j < cnt; ++j) {
                        const u32 key = (u32)__builtin_amdgcn_readlane(rk, j);
                        const int g = __builtin_amdgcn_readlane(rs, j) & 63;
                        if (blen && key != cur) pwr_commit(c, pend, blen, T, X, K, lane);
                        cur = key;
                        if (lane < K && c) atomicAdd(&L[g * K + lane], (u64)c);
                        pend += lane == g ? 1u : 0u;
                        ++blen;
                    }
                }
                if (blen) pwr_commit(c, pend, blen, T, X, K, lane);
            }
            __syncthreads();
            if (tid < 64) {
                u32 tot = 0u;
                for (int w = 0; w < NW; ++w) tot += wcnt[w * 64 + tid];
                carry[tid] += tot;
            }
            __syncthreads();
        }
        __syncthreads();
        if (bad) { // (uniform)
            if (tid == 0) P.left[gene] = bad;
            __syncthreads(); // (as above)
            continue;
        }
        // ---- the zeros, and the statistics of every ordered pair ----
        u32 *s_pos = wcnt, *s_z = wcnt + 64;
        if (tid < 64) {
            u32 pos = 0u, z = 0u;
            if (tid < K) {
                pos = carry[tid] - negc[tid];
                z = (u32)(P.n[tid] - (long long)carry[tid]);
                const u64 zz = z;
                T[tid] += zz * zz * zz - zz;
            }
            s_pos[tid] = pos;
            s_z[tid] = z;
        }
        __syncthreads();
        for (int idx = tid; idx < KK; idx += NT) {
            const int r = idx / K, g = idx - r * K;
            const u64 zg = s_z[g], zr = s_z[r];
            const u64 Lgr = L[g * K + r] + (u64)s_pos[g] * zr + zg * (u64)negc[r];
            const u64 Lrg = L[r * K + g] + (u64)s_pos[r] * zg + zr * (u64)negc[g];
            const size_t o = (size_t)gene * KK + idx;
            P.out_s2[o] = P.n[g] * P.n[r] + (long long)Lgr - (long long)Lrg;
            P.out_tie[o] = T[g] + T[r] + 3ull * (X[g * K + r] + zg * zr * (zg + zr));
        }
        if (tid == 0) P.left[gene] = 0u;
        __syncthreads();
    }
}

struct PwRankEmitParams {
    const long long *s2;   // [nb][K * K]
    const u64 *tie;
    const u32 *left;       // [nb]
    const long long *n;    // [K]
    const int *sel;        // [K] group ids (rows of sums)
    const double *sums;    // [G][sums_ld]
    long long sums_ld;
    int K, nb;
    long long col_off;     // column of the batch's first gene in sums and in the planes
    int use_continuity, tie_correct, alternative;
    double *out_p, *out_u, *out_fc, *out_z; // [K][K][out_ld]: [r][g][gene]
    long long out_ld;
};

#define PWE_NT 256
#define PWE_PAIRS 32 // ordered pairs per workgroup
// grid (ceil(nb / 64), ceil(K K / 32)): 64 genes x 32 pairs of statistics through an LDS tile (read as 256-byte runs of a gene's
// row), then lane = gene: a wavefront writes a pair's 512-byte segment of each plane.  Columns of genes that left stay untouched.
template <bool Z>
__global__ __launch_bounds__(PWE_NT) void k_pw_rank_emit(PwRankEmitParams P) {
    __shared__ long long t_s2[PWE_PAIRS][65];
    __shared__ u64 t_tie[PWE_PAIRS][65];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = P.K, KK = K * K;
    const int gene0 = blockIdx.x * 64, pair0 = blockIdx.y * PWE_PAIRS;
    {
        const int pl = tid & (PWE_PAIRS - 1), gl0 = tid / PWE_PAIRS;
        for (int gl = gl0; gl < 64; gl += PWE_NT / PWE_PAIRS) {
            const int gene = gene0 + gl, pair = pair0 + pl;
            const bool ok = gene < P.nb && pair < KK;
            const size_t o = (size_t)gene * KK + pair;
            t_s2[pl][gl] = ok ? P.s2[o] : 0ll;
            t_tie[pl][gl] = ok ? P.tie[o] : 0ull;
        }
    }
    __syncthreads();
    const int gene = gene0 + lane;
    if (gene >= P.nb || P.left[gene] != 0u) return;
    const long long col = P.col_off + gene;
    const double cc = P.use_continuity ? 0.5 : 0.0;
    for (int pl = wave; pl < PWE_PAIRS; pl += PWE_NT / 64) {
        const int pair = pair0 + pl;
        if (pair >= KK) break;
        const int r = pair / K, g = pair - r * K;
        const long long n_r = P.n[r], n_g = P.n[g];
        const GroupConst gc = group_const(n_r, n_g, n_r + n_g);
        const double sum_g = P.sums[(size_t)P.sel[g] * P.sums_ld + col], sum_r = P.sums[(size_t)P.sel[r] * P.sums_ld + col];
        const size_t o = (size_t)pair * P.out_ld + col;
        double U, pv = 1.0, z = 0.0;
        if (r != g) {
            const long long two_u = 2ll * n_r * n_g - t_s2[pl][lane];
            U = 0.5 * (double)two_u;
            const double tie = P.tie_correct ? (double)t_tie[pl][lane] : 0.0;
            pv = pval_device_pre(gc.nnn, gc.var0, gc.n12, tie, U, gc.mu, cc, P.alternative);
            if constexpr (Z) z = zscore_device_pre(gc.nnn, gc.var0, tie, U, gc.mu);
        } else {
            U = 0.5 * (double)(n_r * n_g);
        }
        P.out_p[o] = pv;
        P.out_u[o] = U;
        P.out_fc[o] = fold_change_device(sum_g, sum_r, gc);
        if constexpr (Z) P.out_z[o] = z;
    }
}
