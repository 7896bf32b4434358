// Per-(group, gene) first and second moments -- illico_group_moments_* (group_moments.hip): the sum of a group's values, the sum
// of their squares, and both over every cell NOT in the group.  What Welch's t-test needs (kernels_ttest.h).
//
// Sibling kernels of kernels_group_stats.h (which stays as it is): the same exact limb sums (kernels_sums.h), twice per value.
// A value x (taken as double) is split into two 42-bit limbs at the scale of the gene's largest finite |x|; its square fl(x * x)
// is split the same way at the scale of fl(v * v), v the gene's largest |x| whose square is finite (v is the largest |x| itself
// unless a square overflows, so the scale costs no further read of the input).  Limbs are added as 64-bit integers in any order;
// the gene's totals over all groups are 128-bit, the rest of a group is total - own in integers, and every sum is rounded to
// float64 once.  No non-zero count is kept: n of a moment is the group's size, zeros count.
//
// Exactness: the 84 limb bits hold a value exactly while it is within 2^-30 (float64; float32: 2^-59) of the gene's largest
// magnitude, and the 48-bit square of a float32 value while it is within 2^-35 of the gene's largest square; smaller ones are
// truncated toward zero at 2^-83 of the respective largest.
//
// Non-finite: NaN / +inf / -inf values are counted per (group, gene) in the packed word `cat` (21 bits each) and kept out of both
// sums' limbs; a finite x whose square overflows (|x| beyond about 1.3e154) adds to the limbs of x and is counted in `ovf`.
// sum is NaN / +inf / -inf as numpy's would be; sumsq is NaN with a NaN, else +inf with an infinity or an overflowing square.
//
// Planes (device scratch, row-major [G][W]): L0 / L1 limbs of x, Q0 / Q1 limbs of x * x, cat, ovf; vmax[W] / vmaxq[W] the bits of
// the two magnitudes above, nonfin[W] a gene that met a non-finite value or an overflowing square.
#pragma once
#include "common.h"
#include "kernels_sums.h"

#define GM_NT 256
#define GM_TILE 256          // dense: genes per workgroup (4 per lane)
#define GM_CHUNK 1024        // dense / CSR: positions (cells) of one group per workgroup at most
#define GM_CSR_CW 2048       // CSR: columns per workgroup: 4 limb planes of 8 bytes = 64 KB of LDS, two workgroups per CU
#define GM_CSC_LDS_G 2048    // CSC: groups held in LDS (32 bytes each, 64 KB: two workgroups per CU); more go through global atomics
#define GM_VMAX_CW 4096      // CSR max pass: columns per LDS window

struct GmPlanes {
    long long *L0, *L1, *Q0, *Q1;
    u64 *cat, *ovf;
    u64 *vmax, *vmaxq;
    int *nonfin;
    long long W; // pitch of the planes (= the window's width)
};

// a chunk of one group's positions: [p0, p1) of d_perm, all of group g; single = the group's only chunk
struct GmChunk { int g, p0, p1, single; };

__device__ __forceinline__ double gm_from_bits(u64 b) { return __longlong_as_double((long long)b); }
// the two scales of a gene from its vmax / vmaxq words
__device__ __forceinline__ ExsScale gm_scale_x(u64 vb) { return exs_scale(vb ? gm_from_bits(vb) : 1.0); }
__device__ __forceinline__ ExsScale gm_scale_q(u64 vqb) {
    const double v = gm_from_bits(vqb), q = v * v;
    return exs_scale(q > 0.0 ? q : 1.0); // (a square that underflows to zero adds nothing)
}
// a value's part in the two magnitudes
__device__ __forceinline__ void gm_track(double x, u64 &m, u64 &mq, bool &nf) {
    if (exs_finite(x)) {
        const u64 b = exs_absbits(x);
        m = umax_t(m, b);
        if (exs_finite(x * x)) mq = umax_t(mq, b); else nf = true;
    } else nf = true;
}

// one value into a lane's limb accumulators of x (a0, a1) and of x * x (b0, b1)
template <typename InT>
__device__ __forceinline__ void gm_add(InT v, const ExsScale &S, const ExsScale &SQ, long long &a0, long long &a1, long long &b0, long long &b1, u64 *catp,
                                       u64 *ovfp) {
    if (!(v != (InT)0)) return;
    const double x = (double)v;
    if (exs_finite(x)) {
        long long l0, l1;
        exs_split(x, S, l0, l1);
        a0 += l0; a1 += l1;
        const double q = x * x;
        if (exs_finite(q)) {
            exs_split(q, SQ, l0, l1);
            b0 += l0; b1 += l1;
        } else atomicAdd(ovfp, 1ull);
    } else atomicAdd(catp, exs_cat_of(x));
}

// ---- dense: the genes' magnitudes ------------------------------------------------------------------------------------------------
// grid (ceil(W / 256), row slices); thread = one gene, rows of its slice in natural order
template <typename InT>
__global__ __launch_bounds__(GM_NT) void k_gm_dense_vmax(const InT *__restrict__ X, long long ld, long long N, int W, u64 *__restrict__ vmax,
                                                        u64 *__restrict__ vmaxq, int *__restrict__ nonfin) {
    const int j = blockIdx.x * GM_NT + threadIdx.x;
    if (j >= W) return;
    const long long rs = (N + gridDim.y - 1) / gridDim.y, r0 = (long long)blockIdx.y * rs, r1 = r0 + rs < N ? r0 + rs : N;
    u64 m = 0, mq = 0;
    bool nf = false;
    long long r = r0;
    for (; r + 4 <= r1; r += 4) {
        InT v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = X[(size_t)(r + u) * ld + j];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v[u] != (InT)0) gm_track((double)v[u], m, mq, nf);
    }
    for (; r < r1; ++r) {
        const InT v = X[(size_t)r * ld + j];
        if (v != (InT)0) gm_track((double)v, m, mq, nf);
    }
    if (m) atomicMax(&vmax[j], m);
    if (mq) atomicMax(&vmaxq[j], mq);
    if (nf) atomicOr(&nonfin[j], 1);
}

// ---- dense: limb sums ----------------------------------------------------------------------------------------------------------
// grid (chunks, ceil(W / GM_TILE)); wavefront w takes positions p0 + w, p0 + w + 4, ... of the chunk; lane l holds genes
// tile + l + 64 u (u < 4).  The four wavefronts' integer partials meet in LDS (32 KB); the chunk's totals are stored (the group's only
// chunk) or added with 64-bit atomics.
template <typename InT>
__global__ __launch_bounds__(GM_NT) void k_gm_dense(const InT *__restrict__ X, long long ld, int W, const int *__restrict__ perm,
                                                   const GmChunk *__restrict__ chunks, GmPlanes P) {
    constexpr int U = GM_TILE / 64;
    __shared__ long long s[4][4][GM_TILE]; // [limb plane][wavefront][gene]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GmChunk ch = chunks[blockIdx.x];
    const int tile0 = blockIdx.y * GM_TILE;
    ExsScale S[U], SQ[U];
    long long a0[U], a1[U], b0[U], b1[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = tile0 + lane + 64 * u;
        ok[u] = j < W;
        S[u] = gm_scale_x(ok[u] ? P.vmax[j] : 0ull);
        SQ[u] = gm_scale_q(ok[u] ? P.vmaxq[j] : 0ull);
        a0[u] = a1[u] = b0[u] = b1[u] = 0;
    }
    const size_t rowo = (size_t)ch.g * P.W + tile0 + lane;
    u64 *catrow = P.cat + rowo, *ovfrow = P.ovf + rowo;
    int p = ch.p0 + wave;
    for (; p + 4 < ch.p1; p += 8) { // two rows in flight per wavefront
        const InT *r0 = X + (size_t)perm[p] * ld + tile0 + lane, *r1 = X + (size_t)perm[p + 4] * ld + tile0 + lane;
        InT v0[U], v1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { v0[u] = ok[u] ? r0[64 * u] : (InT)0; v1[u] = ok[u] ? r1[64 * u] : (InT)0; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            gm_add(v0[u], S[u], SQ[u], a0[u], a1[u], b0[u], b1[u], catrow + 64 * u, ovfrow + 64 * u);
            gm_add(v1[u], S[u], SQ[u], a0[u], a1[u], b0[u], b1[u], catrow + 64 * u, ovfrow + 64 * u);
        }
    }
    if (p < ch.p1) {
        const InT *r0 = X + (size_t)perm[p] * ld + tile0 + lane;
#pragma unroll
        for (int u = 0; u < U; ++u) gm_add(ok[u] ? r0[64 * u] : (InT)0, S[u], SQ[u], a0[u], a1[u], b0[u], b1[u], catrow + 64 * u, ovfrow + 64 * u);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        s[0][wave][lane + 64 * u] = a0[u]; s[1][wave][lane + 64 * u] = a1[u];
        s[2][wave][lane + 64 * u] = b0[u]; s[3][wave][lane + 64 * u] = b1[u];
    }
    __syncthreads();
    const int j = tile0 + tid;
    if (j < W) {
        const size_t o = (size_t)ch.g * P.W + j;
        long long *const planes[4] = {P.L0, P.L1, P.Q0, P.Q1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long t = s[k][0][tid] + s[k][1][tid] + s[k][2][tid] + s[k][3][tid];
            if (ch.single) planes[k][o] = t;
            else if (t) atomicAdd((u64 *)&planes[k][o], (u64)t);
        }
    }
}

// ---- CSC: one workgroup per gene --------------------------------------------------------------------------------------------------
// Pass 1 finds the gene's two magnitudes, pass 2 (the column again, from cache) adds each stored non-zero into its group's limbs:
// LDS atomics for up to GM_CSC_LDS_G groups (flushed to the planes at the end), 64-bit global atomics on the planes beyond.
struct GmCscParams {
    const void *data, *indices, *indptr; // stored entry k at data[k - kshift]
    long long kshift, col0;              // first column of the window
    const int *codes;
    const u16 *codes16;
    int W, G, dt;
};
template <typename InT, typename IdxT, bool LDSG>
__global__ __launch_bounds__(GM_NT) void k_gm_csc(GmCscParams C, GmPlanes P) {
    constexpr int NT = GM_NT, NW = NT / 64;
    extern __shared__ __align__(16) unsigned char smem[];
    u64 *s_red = (u64 *)smem;                     // [2 NW]
    long long *L0 = (long long *)(smem + 64);     // [G] each (LDSG)
    long long *L1 = L0 + (LDSG ? C.G : 0), *Q0 = L1 + (LDSG ? C.G : 0), *Q1 = Q0 + (LDSG ? C.G : 0);
    __shared__ int s_nf[NW];
    const int tid = threadIdx.x, G = C.G;
    const InT *data = (const InT *)C.data;
    const IdxT *indices = (const IdxT *)C.indices, *indptr = (const IdxT *)C.indptr;
    for (int gene = blockIdx.x; gene < C.W; gene += gridDim.x) {
        const long long col = C.col0 + gene;
        const long long k0 = (long long)indptr[col] - C.kshift, k1 = (long long)indptr[col + 1] - C.kshift;
        if (LDSG) for (int g = tid; g < G; g += NT) { L0[g] = 0; L1[g] = 0; Q0[g] = 0; Q1[g] = 0; }
        u64 m = 0, mq = 0;
        bool nf = false;
        for (long long k = k0 + tid; k < k1; k += NT) {
            const InT v = data[k];
            if (v != (InT)0) gm_track((double)v, m, mq, nf);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            m = umax_t(m, (u64)__shfl_xor((long long)m, d));
            mq = umax_t(mq, (u64)__shfl_xor((long long)mq, d));
        }
        const int wnf = __any(nf ? 1 : 0);
        __syncthreads();
        if ((tid & 63) == 0) { s_red[tid >> 6] = m; s_red[NW + (tid >> 6)] = mq; s_nf[tid >> 6] = wnf; }
        __syncthreads();
        m = s_red[0]; mq = s_red[NW];
        bool any_nf = s_nf[0] != 0;
        for (int w = 1; w < NW; ++w) { m = umax_t(m, s_red[w]); mq = umax_t(mq, s_red[NW + w]); any_nf = any_nf || s_nf[w] != 0; }
        if (tid == 0) { P.vmax[gene] = m; P.vmaxq[gene] = mq; P.nonfin[gene] = any_nf ? 1 : 0; }
        const ExsScale S = gm_scale_x(m), SQ = gm_scale_q(mq);
        for (long long k = k0 + tid; k < k1; k += NT) {
            const InT v = data[k];
            if (!(v != (InT)0)) continue;
            const long long row = (long long)indices[k];
            const int g = C.codes16 ? (int)C.codes16[row] : C.codes[row];
            const size_t o = (size_t)g * P.W + gene;
            const double x = (double)v;
            long long l0 = 0, l1 = 0, q0 = 0, q1 = 0;
            if (exs_finite(x)) {
                exs_split(x, S, l0, l1);
                const double q = x * x;
                if (exs_finite(q)) exs_split(q, SQ, q0, q1);
                else atomicAdd(&P.ovf[o], 1ull);
            } else atomicAdd(&P.cat[o], exs_cat_of(x));
            if constexpr (LDSG) {
                if (l0) atomicAdd((u64 *)&L0[g], (u64)l0);
                if (l1) atomicAdd((u64 *)&L1[g], (u64)l1);
                if (q0) atomicAdd((u64 *)&Q0[g], (u64)q0);
                if (q1) atomicAdd((u64 *)&Q1[g], (u64)q1);
            } else {
                if (l0) atomicAdd((u64 *)&P.L0[o], (u64)l0);
                if (l1) atomicAdd((u64 *)&P.L1[o], (u64)l1);
                if (q0) atomicAdd((u64 *)&P.Q0[o], (u64)q0);
                if (q1) atomicAdd((u64 *)&P.Q1[o], (u64)q1);
            }
        }
        if constexpr (LDSG) {
            __syncthreads();
            for (int g = tid; g < G; g += NT) {
                const size_t o = (size_t)g * P.W + gene;
                P.L0[o] = L0[g]; P.L1[o] = L1[g]; P.Q0[o] = Q0[g]; P.Q1[o] = Q1[g];
            }
        }
        __syncthreads();
    }
}
static inline size_t gm_csc_lds_bytes(int G, bool ldsg) { return 64 + (ldsg ? (size_t)G * 32 : 0); }

// ---- CSR: the genes' magnitudes (every stored entry of the window's columns) --------------------------------------------------------
// grid (row blocks, ceil(W / GM_VMAX_CW)); a wavefront per row, LDS maxima per column window, flushed with global atomicMax.  The LDS
// word holds the largest |x| whose square is finite; the rare finite x beyond that goes to vmax in HBM directly.
template <typename InT, typename IdxT>
__global__ __launch_bounds__(GM_NT) void k_gm_csr_vmax(const InT *__restrict__ data, const IdxT *__restrict__ indices, const IdxT *__restrict__ indptr,
                                                      long long kshift, long long n_rows, long long col0, int W, u64 *__restrict__ vmax,
                                                      u64 *__restrict__ vmaxq, int *__restrict__ nonfin) {
    __shared__ u64 sm[GM_VMAX_CW];
    __shared__ int snf[GM_VMAX_CW / 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long wo = (long long)blockIdx.y * GM_VMAX_CW;
    const long long c0 = col0 + wo;
    const int cw = (int)(W - wo < GM_VMAX_CW ? W - wo : GM_VMAX_CW);
    for (int i = tid; i < cw; i += GM_NT) sm[i] = 0;
    for (int i = tid; i < GM_VMAX_CW / 32; i += GM_NT) snf[i] = 0;
    __syncthreads();
    const long long rb = (n_rows + gridDim.x - 1) / gridDim.x, r0 = (long long)blockIdx.x * rb, r1 = r0 + rb < n_rows ? r0 + rb : n_rows;
    for (long long r = r0 + wave; r < r1; r += GM_NT / 64) {
        const long long k0 = (long long)indptr[r] - kshift, k1 = (long long)indptr[r + 1] - kshift;
        for (long long k = k0 + lane; k < k1; k += 64) {
            const long long c = (long long)indices[k] - c0;
            if (c < 0 || c >= cw) continue;
            const InT v = data[k];
            if (!(v != (InT)0)) continue;
            const double x = (double)v;
            bool nf = true;
            if (exs_finite(x)) {
                const u64 b = exs_absbits(x);
                nf = !exs_finite(x * x);
                if (nf) atomicMax(&vmax[wo + c], b);
                else if (b) atomicMax(&sm[c], b);
            }
            if (nf) atomicOr(&snf[c >> 5], 1 << (c & 31));
        }
    }
    __syncthreads();
    for (int i = tid; i < cw; i += GM_NT) {
        if (sm[i]) { atomicMax(&vmax[wo + i], sm[i]); atomicMax(&vmaxq[wo + i], sm[i]); }
        if ((snf[i >> 5] >> (i & 31)) & 1) atomicOr(&nonfin[wo + i], 1);
    }
}

// ---- CSR: limb sums, group-major ---------------------------------------------------------------------------------------------------
// grid (chunks, ceil(W / GM_CSR_CW)): the workgroup walks its chunk's rows through d_perm (a wavefront per row, lanes over the row's
// stored entries in any order) and adds the entries of its column window into LDS limbs; the chunk's totals are stored (the group's
// only chunk) or added with 64-bit atomics
template <typename InT, typename IdxT>
__global__ __launch_bounds__(GM_NT) void k_gm_csr(const InT *__restrict__ data, const IdxT *__restrict__ indices, const IdxT *__restrict__ indptr,
                                                 long long kshift, long long col0, int W, const int *__restrict__ perm, const GmChunk *__restrict__ chunks,
                                                 GmPlanes P) {
    __shared__ long long L[4][GM_CSR_CW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GmChunk ch = chunks[blockIdx.x];
    const int w0 = blockIdx.y * GM_CSR_CW, cw = W - w0 < GM_CSR_CW ? W - w0 : GM_CSR_CW;
    const long long c0 = col0 + w0;
    for (int i = tid; i < cw; i += GM_NT) { L[0][i] = 0; L[1][i] = 0; L[2][i] = 0; L[3][i] = 0; }
    __syncthreads();
    for (int p = ch.p0 + wave; p < ch.p1; p += GM_NT / 64) {
        const long long r = perm[p];
        const long long k0 = (long long)indptr[r] - kshift, k1 = (long long)indptr[r + 1] - kshift;
        for (long long k = k0 + lane; k < k1; k += 64) {
            const long long c = (long long)indices[k] - c0;
            if (c < 0 || c >= cw) continue;
            const InT v = data[k];
            if (!(v != (InT)0)) continue;
            const double x = (double)v;
            const size_t o = (size_t)ch.g * P.W + w0 + c;
            if (exs_finite(x)) {
                long long l0, l1;
                exs_split(x, gm_scale_x(P.vmax[w0 + c]), l0, l1);
                if (l0) atomicAdd((u64 *)&L[0][c], (u64)l0);
                if (l1) atomicAdd((u64 *)&L[1][c], (u64)l1);
                const double q = x * x;
                if (exs_finite(q)) {
                    exs_split(q, gm_scale_q(P.vmaxq[w0 + c]), l0, l1);
                    if (l0) atomicAdd((u64 *)&L[2][c], (u64)l0);
                    if (l1) atomicAdd((u64 *)&L[3][c], (u64)l1);
                } else atomicAdd(&P.ovf[o], 1ull);
            } else atomicAdd(&P.cat[o], exs_cat_of(x));
        }
    }
    __syncthreads();
    long long *const planes[4] = {P.L0, P.L1, P.Q0, P.Q1};
    for (int i = tid; i < cw; i += GM_NT) {
        const size_t o = (size_t)ch.g * P.W + w0 + i;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (ch.single) planes[k][o] = L[k][i];
            else if (L[k][i]) atomicAdd((u64 *)&planes[k][o], (u64)L[k][i]);
        }
    }
}

// ---- totals over the groups and the output planes ---------------------------------------------------------------------------------
struct GmTotal {
    __int128 T, TQ;      // sums over groups of L1 * 2^42 + L0 and of Q1 * 2^42 + Q0
    long long nan, pinf, ninf, ovf;
};
__device__ __forceinline__ __int128 gm_pair(long long l0, long long l1) { return (__int128)l1 * ((__int128)1 << EXS_LIMB) + (__int128)l0; }
// partial totals of slice blockIdx.y of the groups: part[s][W]
static __global__ __launch_bounds__(GM_NT) void k_gm_totals(GmPlanes P, int G, int W, GmTotal *__restrict__ part) {
    const int j = blockIdx.x * GM_NT + threadIdx.x;
    if (j >= W) return;
    const int gs = (G + gridDim.y - 1) / gridDim.y, g0 = blockIdx.y * gs, g1 = g0 + gs < G ? g0 + gs : G;
    const bool nf = P.nonfin[j] != 0;
    GmTotal t;
    t.T = 0; t.TQ = 0; t.nan = t.pinf = t.ninf = t.ovf = 0;
    for (int g = g0; g < g1; ++g) {
        const size_t o = (size_t)g * P.W + j;
        t.T += gm_pair(P.L0[o], P.L1[o]);
        t.TQ += gm_pair(P.Q0[o], P.Q1[o]);
        if (nf) {
            const u64 c = P.cat[o];
            t.nan += (long long)(c & EXS_M21); t.pinf += (long long)((c >> 21) & EXS_M21); t.ninf += (long long)(c >> 42);
            t.ovf += (long long)P.ovf[o];
        }
    }
    part[(size_t)blockIdx.y * W + j] = t;
}

__device__ __forceinline__ double gm_sumsq_value(__int128 TQ, long long nan, long long inf, const ExsScale &SQ) {
    if (nan) return __longlong_as_double(0x7FF8000000000000ll);
    if (inf) return __longlong_as_double(0x7FF0000000000000ll);
    return exs_combine128(TQ, SQ);
}

struct GmOut {
    double *sum, *sumsq, *sum_rest, *sumsq_rest;
    long long ld;        // row pitch of the four planes
};
// grid (ceil(W / 256), group slices): thread = one gene of the slice's groups
static __global__ __launch_bounds__(GM_NT) void k_gm_finalize(GmPlanes P, int G, int W, const GmTotal *__restrict__ part, int n_part, GmOut O) {
    const int j = blockIdx.x * GM_NT + threadIdx.x;
    if (j >= W) return;
    GmTotal t = part[j];
    for (int s = 1; s < n_part; ++s) {
        const GmTotal q = part[(size_t)s * W + j];
        t.T += q.T; t.TQ += q.TQ; t.nan += q.nan; t.pinf += q.pinf; t.ninf += q.ninf; t.ovf += q.ovf;
    }
    const bool nf = P.nonfin[j] != 0;
    const ExsScale S = gm_scale_x(P.vmax[j]), SQ = gm_scale_q(P.vmaxq[j]);
    const int gs = (G + gridDim.y - 1) / gridDim.y, g0 = blockIdx.y * gs, g1 = g0 + gs < G ? g0 + gs : G;
    for (int g = g0; g < g1; ++g) {
        const size_t o = (size_t)g * P.W + j, q = (size_t)g * O.ld + j;
        long long a = 0, b = 0, c = 0, v = 0;
        if (nf) {
            const u64 w = P.cat[o];
            a = (long long)(w & EXS_M21); b = (long long)((w >> 21) & EXS_M21); c = (long long)(w >> 42);
            v = (long long)P.ovf[o];
        }
        if (O.sum || O.sum_rest) {
            const __int128 own = gm_pair(P.L0[o], P.L1[o]);
            if (O.sum) O.sum[q] = exs_sum_value(own, a, b, c, S);
            if (O.sum_rest) O.sum_rest[q] = exs_sum_value(t.T - own, t.nan - a, t.pinf - b, t.ninf - c, S);
        }
        if (O.sumsq || O.sumsq_rest) {
            const __int128 own = gm_pair(P.Q0[o], P.Q1[o]);
            if (O.sumsq) O.sumsq[q] = gm_sumsq_value(own, a, b + c + v, SQ);
            if (O.sumsq_rest) O.sumsq_rest[q] = gm_sumsq_value(t.TQ - own, t.nan - a, (t.pinf - b) + (t.ninf - c) + (t.ovf - v), SQ);
        }
    }
}
