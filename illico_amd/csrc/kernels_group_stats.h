// Per-(group, gene) expression statistics -- illico_group_stats_* (group_stats.hip): the number of a group's cells whose value is
// non-zero, the sum of its values (expm1'd under ILLICO_FLAG_LOG1P: the quantity the fold change divides), and both over every
// cell NOT in the group (the "rest" of one-versus-rest).
//
// Arithmetic: the exact limb sums of kernels_sums.h.  A gene's largest finite magnitude fixes its scale; every finite value is
// split into two 42-bit integer limbs (exs_split) and the limbs are added as 64-bit integers, in any order (LDS atomics, global
// atomics, register sums: integer addition is associative).  A (group, gene) sum holds at most 2^21 - 1 values (the group size
// limit the entry points check), so its limb totals cannot wrap.  The gene's total over all groups is formed in 128-bit
// integers; the rest of group g is total - own, EXACT integer arithmetic, and every sum is rounded to float64 once.  The result
// is the correctly rounded sum whatever the input format, the launch shape or the order of arrival (values below 2^-83 of the
// gene's largest magnitude are truncated there, see kernels_sums.h).
//
// Non-finite values (NaN, +inf, -inf, or an expm1 that overflows) are kept out of the limbs and counted per (group, gene) in one
// packed word (EXS_NAN / EXS_PINF / EXS_NINF, 21 bits each); a sum that meets one is NaN, +inf or -inf as numpy's would be.
//
// Planes (device scratch, row-major [G][W], W = the window's width): L0 / L1 limb sums, cnt non-zero counts, cat non-finite
// counts; vmax[W] the bits of each gene's largest finite |x| (u64 atomicMax: non-negative doubles order as their bit patterns),
// nonfin[W] a gene that met a non-finite value.
#pragma once
#include "common.h"
#include "kernels_sums.h"

#define GS_NT 256
#define GS_TILE 256          // dense: genes per workgroup (4 per lane, each wavefront covers the whole tile)
#define GS_CHUNK 1024        // dense / CSR: positions (cells) of one group per workgroup at most: large groups are split
#define GS_CSR_CW 2048       // CSR: columns per workgroup (LDS counters + limbs)
#define GS_CSC_LDS_G 4096    // CSC: groups held in LDS; more go through global atomics on the planes
#define GS_VMAX_CW 8192      // CSR max pass: columns per LDS window

struct GsPlanes {
    long long *L0, *L1, *cnt;
    u64 *cat;
    u64 *vmax;
    int *nonfin;
    long long W; // pitch of the planes (= the window's width)
};

// a chunk of one group's positions: [p0, p1) of d_perm, all of group g; single = the group's only chunk
struct GsChunk { int g, p0, p1, single; };


// one value into a lane's (l0, l1, n) accumulators; a non-finite x goes straight to the packed counter word of its (group, gene)
template <typename InT>
__device__ __forceinline__ void gs_add(InT v, int dt, int is_log1p, const ExsScale &S, long long &a0, long long &a1, int &n, u64 *catp) {
    if (!(v != (InT)0)) return;
    ++n;
    const double x = sums_value(v, dt, is_log1p);
    if (exs_finite(x)) {
        long long l0, l1;
        exs_split(x, S, l0, l1);
        a0 += l0; a1 += l1;
    } else atomicAdd(catp, exs_cat_of(x));
}

// ---- dense: the genes' largest finite magnitudes -------------------------------------------------------------------------------
// grid (ceil(W / 256), row slices); thread = one gene, rows of its slice in natural order
template <typename InT>
__global__ __launch_bounds__(GS_NT) void k_gs_dense_vmax(const InT *__restrict__ X, long long ld, long long N, int W, int dt, int is_log1p,
                                                        u64 *__restrict__ vmax, int *__restrict__ nonfin) {
    const int j = blockIdx.x * GS_NT + threadIdx.x;
    if (j >= W) return;
    const long long rs = (N + gridDim.y - 1) / gridDim.y, r0 = (long long)blockIdx.y * rs, r1 = r0 + rs < N ? r0 + rs : N;
    u64 m = 0;
    bool nf = false;
    long long r = r0;
    for (; r + 4 <= r1; r += 4) {
        InT v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = X[(size_t)(r + u) * ld + j];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v[u] != (InT)0) {
                const double x = sums_value(v[u], dt, is_log1p);
                if (exs_finite(x)) m = umax_t(m, exs_absbits(x)); else nf = true;
            }
    }
    for (; r < r1; ++r) {
        const InT v = X[(size_t)r * ld + j];
        if (v != (InT)0) {
            const double x = sums_value(v, dt, is_log1p);
            if (exs_finite(x)) m = umax_t(m, exs_absbits(x)); else nf = true;
        }
    }
    if (m) atomicMax(&vmax[j], m);
    if (nf) atomicOr(&nonfin[j], 1);
}

// ---- dense: counts and limb sums -----------------------------------------------------------------------------------------------
// grid (chunks, ceil(W / GS_TILE)); wavefront w takes positions p0 + w, p0 + w + 4, ... of the chunk; lane l holds genes
// tile + l + 64 u (u < 4): every load instruction of a wavefront reads 64 consecutive values of one row.  The four wavefronts'
// integer partials meet in LDS; the chunk's totals are stored (the group's only chunk) or added with 64-bit atomics.
template <typename InT>
__global__ __launch_bounds__(GS_NT) void k_gs_dense(const InT *__restrict__ X, long long ld, int W, const int *__restrict__ perm,
                                                   const GsChunk *__restrict__ chunks, int dt, int is_log1p, GsPlanes P) {
    constexpr int U = GS_TILE / 64;
    __shared__ long long s0[4][GS_TILE], s1[4][GS_TILE];
    __shared__ int sn[4][GS_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GsChunk ch = chunks[blockIdx.x];
    const int tile0 = blockIdx.y * GS_TILE;
    ExsScale S[U];
    long long a0[U], a1[U];
    int n[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = tile0 + lane + 64 * u;
        ok[u] = j < W;
        S[u] = exs_scale(ok[u] && P.vmax[j] ? __longlong_as_double((long long)P.vmax[j]) : 1.0);
        a0[u] = a1[u] = 0;
        n[u] = 0;
    }
    u64 *catrow = P.cat + (size_t)ch.g * P.W + tile0 + lane;
    int p = ch.p0 + wave;
    for (; p + 4 < ch.p1; p += 8) { // two rows in flight per wavefront
        const InT *r0 = X + (size_t)perm[p] * ld + tile0 + lane, *r1 = X + (size_t)perm[p + 4] * ld + tile0 + lane;
        InT v0[U], v1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { v0[u] = ok[u] ? r0[64 * u] : (InT)0; v1[u] = ok[u] ? r1[64 * u] : (InT)0; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            gs_add(v0[u], dt, is_log1p, S[u], a0[u], a1[u], n[u], catrow + 64 * u);
            gs_add(v1[u], dt, is_log1p, S[u], a0[u], a1[u], n[u], catrow + 64 * u);
        }
    }
    if (p < ch.p1) {
        const InT *r0 = X + (size_t)perm[p] * ld + tile0 + lane;
#pragma unroll
        for (int u = 0; u < U; ++u) gs_add(ok[u] ? r0[64 * u] : (InT)0, dt, is_log1p, S[u], a0[u], a1[u], n[u], catrow + 64 * u);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { s0[wave][lane + 64 * u] = a0[u]; s1[wave][lane + 64 * u] = a1[u]; sn[wave][lane + 64 * u] = n[u]; }
    __syncthreads();
    const int j = tile0 + tid;
    if (j < W) {
        const long long t0 = s0[0][tid] + s0[1][tid] + s0[2][tid] + s0[3][tid];
        const long long t1 = s1[0][tid] + s1[1][tid] + s1[2][tid] + s1[3][tid];
        const long long tn = (long long)sn[0][tid] + sn[1][tid] + sn[2][tid] + sn[3][tid];
        const size_t o = (size_t)ch.g * P.W + j;
        if (ch.single) { P.L0[o] = t0; P.L1[o] = t1; P.cnt[o] = tn; }
        else {
            if (t0) atomicAdd((u64 *)&P.L0[o], (u64)t0);
            if (t1) atomicAdd((u64 *)&P.L1[o], (u64)t1);
            if (tn) atomicAdd((u64 *)&P.cnt[o], (u64)tn);
        }
    }
}

// ---- CSC: one workgroup per gene --------------------------------------------------------------------------------------------------
// Pass 1 finds the gene's largest finite magnitude, pass 2 (the column again, from cache) adds each stored non-zero into its group's
// counters: LDS atomics for up to GS_CSC_LDS_G groups (flushed to the planes at the end), 64-bit global atomics on the planes beyond.
struct GsCscParams {
    const void *data, *indices, *indptr; // stored entry k at data[k - kshift]
    long long kshift, col0;              // first column of the window
    const int *codes;
    const u16 *codes16;
    int W, G, dt, is_log1p;
};
template <typename InT, typename IdxT, bool LDSG>
__global__ __launch_bounds__(GS_NT) void k_gs_csc(GsCscParams C, GsPlanes P) {
    constexpr int NT = GS_NT, NW = NT / 64;
    extern __shared__ __align__(16) unsigned char smem[];
    u64 *s_red = (u64 *)smem;                     // [NW]
    long long *L0 = (long long *)(smem + 64);     // [G] (LDSG)
    long long *L1 = L0 + (LDSG ? C.G : 0);
    int *CN = (int *)(L1 + (LDSG ? C.G : 0));
    __shared__ int s_nf[NW];
    const int tid = threadIdx.x, G = C.G;
    const InT *data = (const InT *)C.data;
    const IdxT *indices = (const IdxT *)C.indices, *indptr = (const IdxT *)C.indptr;
    for (int gene = blockIdx.x; gene < C.W; gene += gridDim.x) {
        const long long col = C.col0 + gene;
        const long long k0 = (long long)indptr[col] - C.kshift, k1 = (long long)indptr[col + 1] - C.kshift;
        if (LDSG) for (int g = tid; g < G; g += NT) { L0[g] = 0; L1[g] = 0; CN[g] = 0; }
        u64 m = 0;
        bool nf = false;
        for (long long k = k0 + tid; k < k1; k += NT) {
            const InT v = data[k];
            if (v != (InT)0) {
                const double x = sums_value(v, C.dt, C.is_log1p);
                if (exs_finite(x)) m = umax_t(m, exs_absbits(x)); else nf = true;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) m = umax_t(m, (u64)__shfl_xor((long long)m, d));
        const int wnf = __any(nf ? 1 : 0);
        __syncthreads();
        if ((tid & 63) == 0) { s_red[tid >> 6] = m; s_nf[tid >> 6] = wnf; }
        __syncthreads();
        m = s_red[0];
        bool any_nf = s_nf[0] != 0;
        for (int w = 1; w < NW; ++w) { m = umax_t(m, s_red[w]); any_nf = any_nf || s_nf[w] != 0; }
        if (tid == 0) { P.vmax[gene] = m; P.nonfin[gene] = any_nf ? 1 : 0; }
        const ExsScale S = exs_scale(m ? __longlong_as_double((long long)m) : 1.0);
        for (long long k = k0 + tid; k < k1; k += NT) {
            const InT v = data[k];
            if (!(v != (InT)0)) continue;
            const long long row = (long long)indices[k];
            const int g = C.codes16 ? (int)C.codes16[row] : C.codes[row];
            const size_t o = (size_t)g * P.W + gene;
            const double x = sums_value(v, C.dt, C.is_log1p);
            long long l0 = 0, l1 = 0;
            const bool fin = exs_finite(x);
            if (fin) exs_split(x, S, l0, l1);
            else atomicAdd(&P.cat[o], exs_cat_of(x));
            if constexpr (LDSG) {
                atomicAdd(&CN[g], 1);
                if (l0) atomicAdd((u64 *)&L0[g], (u64)l0);
                if (l1) atomicAdd((u64 *)&L1[g], (u64)l1);
            } else {
                atomicAdd((u64 *)&P.cnt[o], 1ull);
                if (l0) atomicAdd((u64 *)&P.L0[o], (u64)l0);
                if (l1) atomicAdd((u64 *)&P.L1[o], (u64)l1);
            }
        }
        if constexpr (LDSG) {
            __syncthreads();
            for (int g = tid; g < G; g += NT) {
                const size_t o = (size_t)g * P.W + gene;
                P.L0[o] = L0[g]; P.L1[o] = L1[g]; P.cnt[o] = CN[g];
            }
        }
        __syncthreads();
    }
}
static inline size_t gs_csc_lds_bytes(int G, bool ldsg) { return 64 + (ldsg ? (size_t)G * 20 : 0); }

// ---- CSR: the genes' largest finite magnitudes (every stored entry of the window's columns) --------------------------------------
// grid (row blocks, ceil(W / GS_VMAX_CW)); a wavefront per row, LDS maxima per column window, flushed with global atomicMax
template <typename InT, typename IdxT>
__global__ __launch_bounds__(GS_NT) void k_gs_csr_vmax(const InT *__restrict__ data, const IdxT *__restrict__ indices, const IdxT *__restrict__ indptr,
                                                      long long kshift, long long n_rows, long long col0, int W, int dt, int is_log1p, u64 *__restrict__ vmax,
                                                      int *__restrict__ nonfin) {
    __shared__ u64 sm[GS_VMAX_CW];
    __shared__ int snf[GS_VMAX_CW / 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c0 = col0 + (long long)blockIdx.y * GS_VMAX_CW;
    const int cw = (int)(W - (long long)blockIdx.y * GS_VMAX_CW < GS_VMAX_CW ? W - (long long)blockIdx.y * GS_VMAX_CW : GS_VMAX_CW);
    for (int i = tid; i < cw; i += GS_NT) sm[i] = 0;
    for (int i = tid; i < GS_VMAX_CW / 32; i += GS_NT) snf[i] = 0;
    __syncthreads();
    const long long rb = (n_rows + gridDim.x - 1) / gridDim.x, r0 = (long long)blockIdx.x * rb, r1 = r0 + rb < n_rows ? r0 + rb : n_rows;
    for (long long r = r0 + wave; r < r1; r += GS_NT / 64) {
        const long long k0 = (long long)indptr[r] - kshift, k1 = (long long)indptr[r + 1] - kshift;
        for (long long k = k0 + lane; k < k1; k += 64) {
            const long long c = (long long)indices[k] - c0;
            if (c < 0 || c >= cw) continue;
            const InT v = data[k];
            if (!(v != (InT)0)) continue;
            const double x = sums_value(v, dt, is_log1p);
            if (exs_finite(x)) { const u64 b = exs_absbits(x); if (b) atomicMax(&sm[c], b); }
            else atomicOr(&snf[c >> 5], 1 << (c & 31));
        }
    }
    __syncthreads();
    const long long o = (long long)blockIdx.y * GS_VMAX_CW;
    for (int i = tid; i < cw; i += GS_NT) {
        if (sm[i]) atomicMax(&vmax[o + i], sm[i]);
        if ((snf[i >> 5] >> (i & 31)) & 1) atomicOr(&nonfin[o + i], 1);
    }
}

// ---- CSR: counts and limb sums, group-major --------------------------------------------------------------------------------------
// Stored entry k at data[k - kshift].  grid (chunks, ceil(W / GS_CSR_CW)): the workgroup walks its chunk's rows through d_perm (a wavefront per row, lanes over the
// row's stored entries in any order) and adds the entries of its column window into LDS counters; the chunk's totals are stored
// (the group's only chunk) or added with 64-bit atomics
template <typename InT, typename IdxT>
__global__ __launch_bounds__(GS_NT) void k_gs_csr(const InT *__restrict__ data, const IdxT *__restrict__ indices, const IdxT *__restrict__ indptr,
                                                 long long kshift, long long col0, int W, const int *__restrict__ perm, const GsChunk *__restrict__ chunks, int dt,
                                                 int is_log1p, GsPlanes P) {
    __shared__ long long L0[GS_CSR_CW], L1[GS_CSR_CW];
    __shared__ int CN[GS_CSR_CW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GsChunk ch = chunks[blockIdx.x];
    const int w0 = blockIdx.y * GS_CSR_CW, cw = W - w0 < GS_CSR_CW ? W - w0 : GS_CSR_CW;
    const long long c0 = col0 + w0;
    for (int i = tid; i < cw; i += GS_NT) { L0[i] = 0; L1[i] = 0; CN[i] = 0; }
    __syncthreads();
    for (int p = ch.p0 + wave; p < ch.p1; p += GS_NT / 64) {
        const long long r = perm[p];
        const long long k0 = (long long)indptr[r] - kshift, k1 = (long long)indptr[r + 1] - kshift;
        for (long long k = k0 + lane; k < k1; k += 64) {
            const long long c = (long long)indices[k] - c0;
            if (c < 0 || c >= cw) continue;
            const InT v = data[k];
            if (!(v != (InT)0)) continue;
            atomicAdd(&CN[c], 1);
            const double x = sums_value(v, dt, is_log1p);
            if (exs_finite(x)) {
                const u64 vb = P.vmax[w0 + c];
                const ExsScale S = exs_scale(vb ? __longlong_as_double((long long)vb) : 1.0);
                long long l0, l1;
                exs_split(x, S, l0, l1);
                if (l0) atomicAdd((u64 *)&L0[c], (u64)l0);
                if (l1) atomicAdd((u64 *)&L1[c], (u64)l1);
            } else atomicAdd(&P.cat[(size_t)ch.g * P.W + w0 + c], exs_cat_of(x));
        }
    }
    __syncthreads();
    for (int i = tid; i < cw; i += GS_NT) {
        const size_t o = (size_t)ch.g * P.W + w0 + i;
        if (ch.single) { P.L0[o] = L0[i]; P.L1[o] = L1[i]; P.cnt[o] = CN[i]; }
        else {
            if (L0[i]) atomicAdd((u64 *)&P.L0[o], (u64)L0[i]);
            if (L1[i]) atomicAdd((u64 *)&P.L1[o], (u64)L1[i]);
            if (CN[i]) atomicAdd((u64 *)&P.cnt[o], (u64)CN[i]);
        }
    }
}

// ---- totals over the groups and the output planes ---------------------------------------------------------------------------------
struct GsTotal {
    __int128 T;          // sum over groups of L1 * 2^42 + L0
    long long n, nan, pinf, ninf;
};
// partial totals of slice blockIdx.y of the groups: part[s][W]
__global__ __launch_bounds__(GS_NT) void k_gs_totals(GsPlanes P, int G, int W, GsTotal *__restrict__ part) {
    const int j = blockIdx.x * GS_NT + threadIdx.x;
    if (j >= W) return;
    const int gs = (G + gridDim.y - 1) / gridDim.y, g0 = blockIdx.y * gs, g1 = g0 + gs < G ? g0 + gs : G;
    const bool nf = P.nonfin[j] != 0;
    GsTotal t;
    t.T = 0; t.n = t.nan = t.pinf = t.ninf = 0;
    for (int g = g0; g < g1; ++g) {
        const size_t o = (size_t)g * P.W + j;
        t.T += (__int128)P.L1[o] * ((__int128)1 << EXS_LIMB) + (__int128)P.L0[o];
        t.n += P.cnt[o];
        if (nf) { const u64 c = P.cat[o]; t.nan += (long long)(c & EXS_M21); t.pinf += (long long)((c >> 21) & EXS_M21); t.ninf += (long long)(c >> 42); }
    }
    part[(size_t)blockIdx.y * W + j] = t;
}


struct GsOut {
    long long *nnz, *nnz_rest;
    double *sum, *sum_rest;
    long long ld;        // row pitch of the four planes
};
// grid (ceil(W / 256), group slices): thread = one gene of the slice's groups
__global__ __launch_bounds__(GS_NT) void k_gs_finalize(GsPlanes P, int G, int W, const GsTotal *__restrict__ part, int n_part, GsOut O) {
    const int j = blockIdx.x * GS_NT + threadIdx.x;
    if (j >= W) return;
    GsTotal t = part[j];
    for (int s = 1; s < n_part; ++s) {
        const GsTotal q = part[(size_t)s * W + j];
        t.T += q.T; t.n += q.n; t.nan += q.nan; t.pinf += q.pinf; t.ninf += q.ninf;
    }
    const bool nf = P.nonfin[j] != 0;
    const u64 vb = P.vmax[j];
    const ExsScale S = exs_scale(vb ? __longlong_as_double((long long)vb) : 1.0);
    const int gs = (G + gridDim.y - 1) / gridDim.y, g0 = blockIdx.y * gs, g1 = g0 + gs < G ? g0 + gs : G;
    for (int g = g0; g < g1; ++g) {
        const size_t o = (size_t)g * P.W + j, q = (size_t)g * O.ld + j;
        const long long n = P.cnt[o];
        if (O.nnz) O.nnz[q] = n;
        if (O.nnz_rest) O.nnz_rest[q] = t.n - n;
        if (O.sum || O.sum_rest) {
            const __int128 own = (__int128)P.L1[o] * ((__int128)1 << EXS_LIMB) + (__int128)P.L0[o];
            long long a = 0, b = 0, c = 0;
            if (nf) { const u64 w = P.cat[o]; a = (long long)(w & EXS_M21); b = (long long)((w >> 21) & EXS_M21); c = (long long)(w >> 42); }
            if (O.sum) O.sum[q] = exs_sum_value(own, a, b, c, S);
            if (O.sum_rest) O.sum_rest[q] = exs_sum_value(t.T - own, t.nan - a, t.pinf - b, t.ninf - c, S);
        }
    }
}
