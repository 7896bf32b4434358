// Per-group marker statistics: the K - 1 p-values of a group against every other group combined into one (illico_combine_pairs,
// markers.hip; include/illico_hip_markers.h states the three formulas).
//
// Lane = gene.  A wavefront takes one group g and 64 consecutive columns j: every load of p[r][g][j0 .. j0 + 63] is one 512-byte
// line, and each (r, g, j) is loaded by exactly one lane, once.  No lane reads what another wrote, so there is no barrier.
//
//   k_mk_validate   finds the first off-diagonal p of a live column that is NaN or outside [0, 1] (atomicMin on one word);
//   k_mk_combine    ALL: a running maximum in registers, the last index winning ties (the representative has rank n).
//                   ANY / SOME: the lane's n values are staged in LDS as [reference slot][lane] -- 64 consecutive doubles per slot,
//                   conflict-free -- and the stable rank of each is formed by counting: MK_RB values are held in registers per walk
//                   over the column, so one LDS read serves MK_RB comparisons.  The term of the formula is taken at that rank and
//                   folded with min / max: over non-NaN terms the result does not depend on the order, so it equals the sorted
//                   form bit for bit.  The effect planes are read at the representative only.
//
// LDS: 512 (K - 1) bytes per workgroup -- 127.5 KiB at K = 256, which is why a workgroup is one wavefront.
#pragma once
#include "../../include/illico_hip_markers.h"
#include "common.h"

#define MK_NT 64  // lanes (columns) per workgroup
#define MK_RB 8   // values ranked per walk over the staged column

struct MkParams {
    const double *p;      // [K][K][in_ld]
    const double *e[ILLICO_COMBINE_MAX_EFFECTS];
    long long in_ld;
    const u32 *skip;      // [W] or null
    int K;
    long long W;
    int rank_j;           // SOME
    double *out_p;        // [K][out_ld]
    int *out_rep;
    double *o[ILLICO_COMBINE_MAX_EFFECTS];
    long long out_ld;
};

static inline size_t mk_lds_bytes(int K, int method) { return method == ILLICO_COMBINE_ALL ? 0 : (size_t)(K - 1) * MK_NT * sizeof(double); }

// grid (column blocks, K groups, K references); err: the first invalid position (r * K + g) * W + column
__global__ __launch_bounds__(256) void k_mk_validate(const double *__restrict__ p, long long ld, int K, long long W, const u32 *__restrict__ skip,
                                                     u64 *__restrict__ err) {
    const int r = blockIdx.z, g = blockIdx.y;
    if (r == g) return;
    const double *row = p + ((size_t)r * K + g) * (size_t)ld;
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < W; c += (long long)gridDim.x * 256) {
        if (skip && skip[c]) continue;
        const double v = row[c];
        if (!(v >= 0.0 && v <= 1.0)) atomicMin(err, ((u64)r * (u64)K + (u64)g) * (u64)W + (u64)c);
    }
}

// grid (column blocks of MK_NT, K groups), MK_NT threads; dynamic LDS mk_lds_bytes(K, METHOD)
template <int METHOD>
__global__ __launch_bounds__(MK_NT) void k_mk_combine(const MkParams P) {
    extern __shared__ __align__(16) unsigned char mk_lds[];
    const int lane = threadIdx.x, g = blockIdx.y, K = P.K, n = K - 1;
    const long long j = (long long)blockIdx.x * MK_NT + lane;
    if (j >= P.W || (P.skip && P.skip[j])) return;
    const size_t slab = (size_t)K * (size_t)P.in_ld; // elements from one reference to the next
    const double *src = P.p + (size_t)g * (size_t)P.in_ld + j;
    double best;
    int rep = 0;
    if constexpr (METHOD == ILLICO_COMBINE_ALL) {
        best = -1.0; // (below every valid p)
#pragma unroll 8
        for (int r = 0; r < g; ++r) {
            const double v = src[(size_t)r * slab];
            if (v >= best) best = v, rep = r;
        }
#pragma unroll 8
        for (int r = g + 1; r < K; ++r) {
            const double v = src[(size_t)r * slab];
            if (v >= best) best = v, rep = r;
        }
    } else {
        double *col = (double *)mk_lds + lane; // slot s (reference s + (s >= g)) at col[s * MK_NT]
#pragma unroll 8
        for (int s = 0; s < g; ++s) col[s * MK_NT] = src[(size_t)s * slab];
#pragma unroll 8
        for (int s = g; s < n; ++s) col[s * MK_NT] = src[(size_t)(s + 1) * slab];
        const double dn = (double)n;
        best = METHOD == ILLICO_COMBINE_ANY ? __longlong_as_double(0x7FF0000000000000ll) : -1.0;
        for (int s0 = 0; s0 < n; s0 += MK_RB) {
            double v[MK_RB];
            int below[MK_RB];
#pragma unroll
            for (int b = 0; b < MK_RB; ++b) {
                v[b] = col[min(s0 + b, n - 1) * MK_NT];
                below[b] = 0;
            }
            const int s1 = min(s0 + MK_RB, n);
#pragma unroll 4
            for (int t = 0; t < s0; ++t) { // earlier slots: an equal p ranks below
                const double q = col[t * MK_NT];
#pragma unroll
                for (int b = 0; b < MK_RB; ++b) below[b] += q <= v[b] ? 1 : 0;
            }
            for (int t = s0; t < s1; ++t) {
                const double q = col[t * MK_NT];
#pragma unroll
                for (int b = 0; b < MK_RB; ++b) below[b] += (q < v[b] || (q == v[b] && t < s0 + b)) ? 1 : 0;
            }
#pragma unroll 4
            for (int t = s1; t < n; ++t) { // later slots: only a smaller p ranks below
                const double q = col[t * MK_NT];
#pragma unroll
                for (int b = 0; b < MK_RB; ++b) below[b] += q < v[b] ? 1 : 0;
            }
#pragma unroll
            for (int b = 0; b < MK_RB; ++b) {
                const int s = s0 + b, rank = below[b] + 1;
                if (s >= n) break;
                if constexpr (METHOD == ILLICO_COMBINE_ANY) {
                    best = fmin(best, v[b] * dn / (double)rank);
                    if (rank == 1) rep = s + (s >= g ? 1 : 0);
                } else {
                    if (rank <= P.rank_j) best = fmax(best, v[b] * (dn - (double)rank + 1.0));
                    if (rank == P.rank_j) rep = s + (s >= g ? 1 : 0);
                }
            }
        }
        if constexpr (METHOD == ILLICO_COMBINE_SOME) best = fmin(1.0, best);
    }
    const size_t o = (size_t)g * (size_t)P.out_ld + j;
    P.out_p[o] = best;
    P.out_rep[o] = rep;
#pragma unroll
    for (int k = 0; k < ILLICO_COMBINE_MAX_EFFECTS; ++k)
        if (P.e[k]) P.o[k][o] = P.e[k][((size_t)rep * K + g) * (size_t)P.in_ld + j];
}
