// Multiple-testing correction of a p-value plane, one row per group (illico_adjust_pvalues, adjust.hip).
//
// Every row is sorted ascending by p, ties broken by ascending column index (a total, deterministic order).  The sort key is the
// bit pattern of p + 0.0 read as a u64: valid p are non-negative doubles (-0.0 becomes +0.0), whose bit patterns order like their
// values, and 1.0 is 0x3FF0000000000000 -- anything above that (NaN, a sign bit, a value beyond 1) is an invalid p.
//
//   k_adj_validate    finds the first invalid p (row-major position, atomicMin on one word) before anything is written;
//   k_adj_sort_lds    one workgroup sorts up to ADJ_LDS_COLS (key, column) pairs in LDS (bitonic network on the composite key, so
//                     the order of equal keys is fixed by the column).  FINAL: the row fits, and the same workgroup then forms the
//                     Benjamini-Hochberg / -Yekutieli values (suffix minimum of p_(k) * (m / k) [* c_m]), clips them to 1 and
//                     scatters them back to their columns, and writes the first n_top columns of the order.  Otherwise it sorts
//                     one ADJ_LDS_COLS-wide segment of a longer row into a run in HBM;
//   k_adj_merge       merges pairs of sorted runs of a longer row, one element per thread: an element of the left run moves by
//                     the number of right-run keys below it, one of the right run by the number of left-run keys at or below it
//                     (the left run holds the lower columns, so equal keys keep their column order);
//   k_adj_scan        one workgroup per longer row: the suffix minimum over its sorted run, back to front in tiles, scatter, top-n;
//   k_adj_bonferroni  min(p * m, 1), elementwise.
//
// The arithmetic is scipy's (stats.false_discovery_control): m / k is one float64 division, then multiplied in; BY multiplies by
// c_m = sum_{i <= m} 1 / i afterwards (formed on the host in the order of numpy's pairwise sum, adjust.hip: harmonic; the contract
// is a relative 1e-14, since numpy's summation order is its own; BH and Bonferroni bit for bit).  Zeros come out as +0.0.
#pragma once
#include "../../include/illico_hip.h"
#include "common.h"

#define ADJ_LDS_COLS ILLICO_ADJ_LDS_COLS   // longest row one workgroup sorts in LDS (12 B per slot: 96 KiB + the wave totals)
#define ADJ_KEY_MAX 0x3FF0000000000000ull  // the key of 1.0
#define ADJ_SCAN_NT 1024
#define ADJ_SCAN_E 4                       // k_adj_scan: contiguous slots per thread and tile

enum { ADJ_M_BH = 0, ADJ_M_BY = 1, ADJ_M_NONE = 2 }; // what the sort kernels form besides the order (NONE: top-n only)

__device__ __forceinline__ u64 adj_key(double p) { return (u64)__double_as_longlong(p + 0.0); }
// illico_top_by_score: the order-preserving u64 of -x + 0.0 (sign bit set: all bits flipped, else the sign bit set), so that keys ascend as
// x descends; -0.0 and +0.0 share a key, +inf sorts first, -inf last -- at 0xFFF0000000000000, still below the padding key ~0.  (NaN is
// refused before: k_top_validate.)
__device__ __forceinline__ u64 score_key(double x) {
    const u64 b = (u64)__double_as_longlong(-x + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct AdjParams {
    const double *p;        // first row of the batch
    long long in_ld;
    int m;                  // columns per row
    int n2;                 // k_adj_sort_lds: power-of-two LDS slots
    int method;             // ADJ_M_*
    double cm;              // BY: sum_{i <= m} 1 / i
    double *out;            // null: no adjusted plane
    long long out_ld;
    long long *top;         // null: no top-n
    long long top_ld;
    int n_top;
    u64 *skey;              // long rows: sorted runs [row][m] (keys, then columns)
    u32 *sidx;
};

// the value of sorted position k (0-based) before the suffix minimum
__device__ __forceinline__ double adj_value(u64 key, int k, const AdjParams &P) {
    double v = __longlong_as_double((long long)key) * ((double)P.m / (double)(k + 1));
    if (P.method == ADJ_M_BY) v *= P.cm;
    return v;
}

// Exclusive suffix minimum over the threads of the workgroup (min of x over the threads above this one) and, in `total`, the minimum
// over all of them.  wtot: blockDim.x / 64 doubles of LDS; the caller synchronises before wtot is written again.
__device__ __forceinline__ double adj_suffix_excl(double x, double *wtot, double &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double inc = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_down(inc, off);
        if (lane + off < 64) inc = fmin(inc, y);
    }
    double ex = __shfl_down(inc, 1);
    if (lane == 63) ex = __builtin_inf();
    if (lane == 0) wtot[w] = inc;
    __syncthreads();
    double after = __builtin_inf(), tot = __builtin_inf();
    for (int v = 0; v < nw; ++v) {
        const double t = wtot[v];
        tot = fmin(tot, t);
        if (v > w) after = fmin(after, t);
    }
    total = tot;
    return fmin(ex, after);
}

// grid (column blocks, rows); err: first invalid position row * m + column (rows counted from row0)
__global__ __launch_bounds__(256) void k_adj_validate(const double *__restrict__ p, long long ld, int m, long long row0, u64 *__restrict__ err) {
    const double *row = p + (size_t)blockIdx.y * ld;
    for (int c = blockIdx.x * 256 + (int)threadIdx.x; c < m; c += gridDim.x * 256)
        if (adj_key(row[c]) > ADJ_KEY_MAX) atomicMin(err, (u64)(row0 + blockIdx.y) * (u64)m + (u64)c);
}

// illico_top_by_score: the first NaN, as k_adj_validate
__global__ __launch_bounds__(256) void k_top_validate(const double *__restrict__ x, long long ld, int m, long long row0, u64 *__restrict__ err) {
    const double *row = x + (size_t)blockIdx.y * ld;
    for (int c = blockIdx.x * 256 + (int)threadIdx.x; c < m; c += gridDim.x * 256)
        if (isnan(row[c])) atomicMin(err, (u64)(row0 + blockIdx.y) * (u64)m + (u64)c);
}

// grid (column blocks, rows)
__global__ __launch_bounds__(256) void k_adj_bonferroni(const double *__restrict__ p, long long ld, int m, double *__restrict__ out,
                                                        long long out_ld) {
    const double *row = p + (size_t)blockIdx.y * ld;
    double *orow = out + (size_t)blockIdx.y * out_ld;
    for (int c = blockIdx.x * 256 + (int)threadIdx.x; c < m; c += gridDim.x * 256) orow[c] = fmin((row[c] + 0.0) * (double)m, 1.0);
}

// grid (segments, rows), blockDim = min(1024, n2 / 2) (n2 a power of two, at least 128); dynamic LDS 12 * n2 + 8 * 16 bytes.
// FINAL: grid.x == 1 and m <= n2.  Otherwise segment s holds columns [s * n2, min((s + 1) * n2, m)) and is written, sorted, to skey / sidx.
// SCORE (k_top_sort_lds): the keys of illico_top_by_score; only the order and the top-n are formed (method ADJ_M_NONE).
template <bool FINAL, bool SCORE>
__device__ __forceinline__ void adj_sort_lds_body(const AdjParams &P) {
    extern __shared__ __align__(16) unsigned char adj_lds[];
    const int n2 = P.n2, nt = blockDim.x, tid = threadIdx.x;
    u64 *key = (u64 *)adj_lds;
    u32 *idx = (u32 *)(adj_lds + (size_t)n2 * 8);
    double *wtot = (double *)(adj_lds + (size_t)n2 * 12);
    const long long row = blockIdx.y;
    const int c0 = FINAL ? 0 : (int)blockIdx.x * n2;
    const int valid = min(n2, P.m - c0);
    const double *prow = P.p + row * P.in_ld + c0;
    for (int i = tid; i < n2; i += nt) {
        key[i] = i < valid ? (SCORE ? score_key(prow[i]) : adj_key(prow[i])) : ~0ull; // padding sorts last (every valid key is below ~0)
        idx[i] = i < valid ? (u32)(c0 + i) : 0xFFFFFFFFu;
    }
    __syncthreads();
    // bitonic network on (key, column): pair q of a stage compares slots i and i + j, i = q with a zero bit inserted at log2(j)
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = tid; q < (n2 >> 1); q += nt) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i + j;
                const u64 a = key[i], b = key[l];
                const u32 ia = idx[i], ib = idx[l];
                const bool gt = a > b || (a == b && ia > ib);
                if (gt == ((i & k) == 0)) {
                    key[i] = b; key[l] = a;
                    idx[i] = ib; idx[l] = ia;
                }
            }
            __syncthreads();
        }
    if (!FINAL) {
        const size_t base = (size_t)row * P.m + c0;
        for (int i = tid; i < valid; i += nt) {
            P.skey[base + i] = key[i];
            P.sidx[base + i] = idx[i];
        }
        return;
    }
    long long *trow = P.top ? P.top + row * P.top_ld : nullptr;
    if (P.method == ADJ_M_NONE) {
        for (int i = tid; i < P.n_top; i += nt) trow[i] = idx[i];
        return;
    }
    // this thread's slots [tid * e, tid * e + e): their suffix minimum in place (as doubles, over the keys), then the threads above
    const int e = n2 / nt, k0 = tid * e;
    double s = __builtin_inf();
    for (int u = e - 1; u >= 0; --u) {
        const int k = k0 + u;
        if (k < P.m) s = fmin(s, adj_value(key[k], k, P));
        key[k] = (u64)__double_as_longlong(s);
    }
    double total;
    const double after = adj_suffix_excl(s, wtot, total);
    double *orow = P.out + row * P.out_ld;
    for (int u = 0; u < e; ++u) {
        const int k = k0 + u;
        if (k < P.m) {
            orow[idx[k]] = fmin(fmin(__longlong_as_double((long long)key[k]), after), 1.0);
            if (k < P.n_top) trow[k] = idx[k];
        }
    }
}
template <bool FINAL>
__global__ __launch_bounds__(1024) void k_adj_sort_lds(AdjParams P) { adj_sort_lds_body<FINAL, false>(P); }
template <bool FINAL>
__global__ __launch_bounds__(1024) void k_top_sort_lds(AdjParams P) { adj_sort_lds_body<FINAL, true>(P); }

// grid (ceil(m / 256), rows): runs of w sorted slots -> runs of 2w
__global__ __launch_bounds__(256) void k_adj_merge(const u64 *__restrict__ sk, const u32 *__restrict__ si, u64 *__restrict__ dk,
                                                   u32 *__restrict__ di, int m, int w) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const size_t rb = (size_t)blockIdx.y * m;
    const u64 *K = sk + rb;
    const long long run = e / w, base = (run & ~1ll) * w;
    const u64 x = K[e];
    long long dest;
    if (!(run & 1)) { // left run: moves past the right-run keys below it
        const long long lo = min(base + w, (long long)m), hi = min(base + 2ll * w, (long long)m);
        long long a = lo, b = hi;
        while (a < b) {
            const long long mid = (a + b) >> 1;
            if (K[mid] < x) a = mid + 1; else b = mid;
        }
        dest = e + (a - lo);
    } else { // right run: moves back before the left-run keys above it
        const long long lo = base, hi = base + w;
        long long a = lo, b = hi;
        while (a < b) {
            const long long mid = (a + b) >> 1;
            if (K[mid] <= x) a = mid + 1; else b = mid;
        }
        dest = e - w + (a - lo);
    }
    dk[rb + dest] = x;
    di[rb + dest] = si[rb + e];
}

// grid (1, rows), ADJ_SCAN_NT threads: the sorted run of each row, back to front in tiles of ADJ_SCAN_NT * ADJ_SCAN_E slots
__global__ __launch_bounds__(ADJ_SCAN_NT) void k_adj_scan(AdjParams P) {
    __shared__ double wtot[2][ADJ_SCAN_NT / 64];
    const size_t rb = (size_t)blockIdx.y * P.m;
    const u64 *K = P.skey + rb;
    const u32 *I = P.sidx + rb;
    double *orow = P.out ? P.out + (size_t)blockIdx.y * P.out_ld : nullptr;
    long long *trow = P.top ? P.top + (size_t)blockIdx.y * P.top_ld : nullptr;
    const int tile = ADJ_SCAN_NT * ADJ_SCAN_E;
    if (P.method == ADJ_M_NONE) {
        for (int i = threadIdx.x; i < P.n_top; i += ADJ_SCAN_NT) trow[i] = I[i];
        return;
    }
    double carry = __builtin_inf(); // minimum over the tiles already done (the later positions)
    int buf = 0;
    for (long long t0 = (long long)(P.m - 1) / tile * tile; t0 >= 0; t0 -= tile, buf ^= 1) {
        const int k0 = (int)t0 + (int)threadIdx.x * ADJ_SCAN_E;
        double v[ADJ_SCAN_E];
        double s = __builtin_inf();
#pragma unroll
        for (int u = ADJ_SCAN_E - 1; u >= 0; --u) {
            const int k = k0 + u;
            if (k < P.m) s = fmin(s, adj_value(K[k], k, P));
            v[u] = s;
        }
        double total;
        const double after = fmin(adj_suffix_excl(s, wtot[buf], total), carry);
#pragma unroll
        for (int u = 0; u < ADJ_SCAN_E; ++u) {
            const int k = k0 + u;
            if (k < P.m) {
                const u32 col = I[k];
                orow[col] = fmin(fmin(v[u], after), 1.0);
                if (k < P.n_top) trow[k] = col;
            }
        }
        carry = fmin(carry, total); // (wtot[buf] is next written two tiles on, after the barrier of the next tile)
    }
}
