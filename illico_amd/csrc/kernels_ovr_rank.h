// One-versus-rest ranks of a RUN of keys, in LDS and without a sort: the one body of k_csc_ovr_gene (the run = a CSC column's stored
// entries, kernels_csc_ovr.h) and of k_ovr_rank_gene_parts (the run = one value-range part of a dense column, kernels_ovr_parts.h).
// A rank needs, for every key, the tie block [s, e) its value occupies among the column's sorted keys.  ovr_rank_run, step by step:
//
//   clear       bucket table, key range, the census words
//   key range   sampled: every 8th row of NT entries -> bucket function (key - kmin) >> shift, 2^lg - 1 buckets of 16-bit counters.  Any
//               monotone bucket function ranks correctly (keys outside the sampled range are clamped into the first / last bucket); the
//               range only balances the buckets
//   count       one LDS atomic per key; a CSC column's census of stored zeros and negatives rides in the same walk
//   crowd test  no bucket above CSCO_MAX_BUCKET keys, the average key shares its bucket with at most CSCO_MAX_AVG: else the sorted form
//   scan        exclusive offsets (three barriers: 16 counters per thread, a wavefront scan, the wavefronts' totals)
//   scatter     one returning LDS atomic + one LDS store per key: the keys, bucket after bucket
//   walk        per key: its bucket's bounds (two neighbouring table entries), the first four keys of the bucket in straight-line code
//               (average bucket: two keys), the rare longer bucket in a loop; s = base + lo + #smaller, e = s + #equal,
//               acc[group] += 2 s + t + 1 (+ 2 n0 for positive keys), tie += t^2 - 1: over a tie block that is t^3 - t
//
// Runs whose values crowd into few buckets (heavy ties, an outlier stretching the range) take the sorted form: the keys are sorted in
// LDS as bare keys (block_sort_hybrid) and every entry looks its value up with two binary searches.
// Measured and not kept (profiles/NOTES_r03.md): a part's records held in registers across the phases (28 - 64 per thread, fully
// unrolled): the kernel becomes instruction-fetch bound (every instruction runs once per part) -- 12.8 ms against 8.3 ms.
//
// The zeros stay implicit (illico/ovr/sparse_ovr.py:70-83): the n0 zeros of a column tie at rank n_neg + (n0 + 1) / 2 and shift every
// positive key by n0; ovr_close_gene adds them per group from the group's count of ranked keys.
#pragma once
#include "common.h"
#include "kernels_finalize.h"
#include "kernels_sparse.h"

#define CSCO_NT 1024
#define CSCO_K 16        // keys per lane of the register sort phases (sorted form): 1024-key chunks
#define CSCO_MAX_BUCKET 192 // bucket form only while no bucket holds more keys than this ...
#define CSCO_MAX_AVG 64     // ... and the average entry shares its bucket with at most this many
#define CSCO_CNT_SHIFT 40   // acc word: doubled rank sum below, ranked keys of the group above
#define CSCO_TAIL_BYTES 256 // s_red | s_k | s_misc: a multiple of 16

// Dynamic LDS of both kernels:  acc [G] 64-bit words (with ACCG: the groups that keep theirs in LDS) | tab [2^lg] 16-bit bucket counters /
// offsets | the tail | A [key_cap + 4] keys.  Everything in front of the keys:
__host__ __device__ static inline size_t csco_acc_bytes(int G) { return (size_t)((G + 1) & ~1) * 8; }
__host__ __device__ static inline size_t csco_fixed_lds_bytes(int G, int lg_buckets) { return csco_acc_bytes(G) + ((size_t)2 << lg_buckets) + CSCO_TAIL_BYTES; }
static inline int csco_key_cap(int G, int lg_buckets, size_t key_size, size_t lds_max, bool accg = false) {
    const size_t fixed = csco_fixed_lds_bytes(accg ? 0 : G, lg_buckets);
    if (fixed + (size_t)CSCO_NT * 4 + 64 > lds_max) return 0; // the scan borrows NT words of the key buffer
    // bucket offsets are 16-bit; 4 slots stay free behind the keys (the bucket walk reads 4 keys at a time)
    return (int)std::min<size_t>((lds_max - fixed) / key_size - 4, 65535 - 4);
}
enum { OVR_N_ZERO = 0, OVR_N_NEG = 1, OVR_FULLEST = 2, OVR_CALLER = 3 }; // s_misc: stored zeros; negatives; largest bucket; the caller's word
template <typename KeyT> struct OvrRankLds { // the kernels' pointers into that layout (nw: wavefronts of the workgroup)
    u64 *acc, *s_red; u32 *tab, *s_misc; u16 *tab16; KeyT *s_k, *A; int nbkt;
    __device__ __forceinline__ OvrRankLds(unsigned char *smem, int G_lds, int lg_buckets, int nw) {
        nbkt = 1 << lg_buckets;
        acc = (u64 *)smem;                                           // [G_lds] doubled rank sum | ranked keys << CSCO_CNT_SHIFT
        tab = (u32 *)(smem + csco_acc_bytes(G_lds));                 // [nbkt / 2] two 16-bit counters / offsets per word
        tab16 = (u16 *)tab;
        s_red = (u64 *)(tab + nbkt / 2);                             // [nw]
        s_k = (KeyT *)(s_red + nw);                                  // [2] smallest / largest sampled key
        s_misc = (u32 *)(s_red + nw + 2);                            // [4] OVR_N_ZERO ..
        A = (KeyT *)(smem + csco_fixed_lds_bytes(G_lds, lg_buckets));
    }
};
static_assert(CSCO_NT / 64 * 8 + 2 * 8 + 4 * 4 <= CSCO_TAIL_BYTES, "s_red, s_k and s_misc of the largest workgroup fit the tail");

// exclusive scan of the 16-bit counters arr[0..n) in place; n = NT * per, per a multiple of 2; totals below 2^16.  tmp: [NT / 64] words.
template <int NT> __device__ __forceinline__ void block_excl_scan_u16_waves(u16 *arr, int n, u32 *tmp, int tid) {
    const int per = n / NT, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = NT / 64;
    u32 *w = (u32 *)arr + (size_t)tid * (per / 2);
    u32 s = 0;
    for (int i = 0; i < per / 2; ++i) { const u32 x = w[i]; s += (x & 0xFFFFu) + (x >> 16); }
    const u32 incl = (u32)wave_incl_scan_add((int)s);
    if (lane == 63) tmp[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const u32 t = lane < NW ? tmp[lane] : 0u;
        const u32 ti = (u32)wave_incl_scan_add((int)t);
        if (lane < NW) tmp[lane] = ti - t;
    }
    __syncthreads();
    u32 run = tmp[wave] + incl - s;
    for (int i = 0; i < per / 2; ++i) {
        const u32 x = w[i];
        const u32 lo = run;
        run += x & 0xFFFFu;
        const u32 hi = run;
        run += x >> 16;
        w[i] = (lo & 0xFFFFu) | (hi << 16);
    }
    __syncthreads();
}

// One source entry: CSC stored entry k of the column, or record k of the part.  Raw loads (value / row index or group
// code) are split from what is derived from them (key; group code through the codes[row] gather) so that the entry
// loops can request round i + 1's raw loads before round i's gather and LDS work.
template <typename InT, typename IdxT, typename KeyT, bool PARTS_> struct OvrSource {
    static constexpr bool PARTS = PARTS_;
    typedef typename std::conditional<PARTS, KeyT, InT>::type RawV;
    typedef typename std::conditional<PARTS, u16, IdxT>::type RawI;
    const InT *data;
    const IdxT *indices;
    const int *codes;
    const u16 *codes16;
    const KeyT *pkeys;
    const u16 *pcodes;
    __device__ __forceinline__ RawV raw_v(long long k, bool in) const {
        if constexpr (PARTS) return in ? pkeys[k] : (KeyT)0;
        else return in ? data[k] : (InT)0;
    }
    __device__ __forceinline__ RawI raw_i(long long k, bool in) const {
        if constexpr (PARTS) return in ? pcodes[k] : (u16)0;
        else return in ? indices[k] : (IdxT)0;
    }
    // key of an entry; nz = it takes part in the ranking (a stored zero is an implicit zero)
    __device__ __forceinline__ KeyT key_from(RawV v, bool in, bool &nz) const {
        if constexpr (PARTS) { nz = in; return v; }
        else { nz = v != (InT)0; return key_of(v); }
    }
    __device__ __forceinline__ int code_from(RawI i) const {
        if constexpr (PARTS) return (int)i;
        else return codes16 ? (int)codes16[(long long)i] : (codes ? codes[(long long)i] : (int)i); // (entries past the end carry row 0: a valid, ignored look-up)
    }
};

// for every entry k in [k0, k1), UL per thread and round: body(u, k, key, nz, code).  Two-stage pipeline: the raw loads of the next
// round are issued before this round's code gather and bodies.  No load sits under a per-lane condition (hipcc gives each such load a
// basic block of its own: `s_and_saveexec` + branch): a round's requests are clamped to the column's last entry, full rounds run
// their bodies unconditionally, only the last, partial round checks each entry.
template <bool WANT_CODE, int NT, int UL, typename Src, typename KeyT, typename Body>
__device__ __forceinline__ void ovr_for_entries(const Src &src, long long k0, long long k1, int tid, Body &&body) {
    constexpr int PER = NT * UL;
    const int n = (int)(k1 - k0); // (a column / a part: at most key_cap entries)
    if (n <= 0) return;
    typename Src::RawV vn[UL];
    typename Src::RawI in[UL];
    auto request = [&](int base) {
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const long long k = k0 + min(base + u * NT + tid, n - 1);
            vn[u] = src.raw_v(k, true);
            if (WANT_CODE) in[u] = src.raw_i(k, true);
        }
    };
    request(0);
    for (int base = 0; base < n; base += PER) {
        KeyT key[UL];
        bool nz[UL];
        int cd[UL];
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            key[u] = src.key_from(vn[u], true, nz[u]);
            cd[u] = WANT_CODE ? src.code_from(in[u]) : 0;
        }
        if (base + PER < n) request(base + PER); // uniform
        if (base + PER <= n) { // uniform: a full round
#pragma unroll
            for (int u = 0; u < UL; ++u) body(u, k0 + base + u * NT + tid, key[u], nz[u], cd[u]);
        } else {
#pragma unroll
            for (int u = 0; u < UL; ++u)
                if (base + u * NT + tid < n) body(u, k0 + base + u * NT + tid, key[u], nz[u], cd[u]);
        }
    }
}

// ---- the steps ----------------------------------------------------------------------------------------------------------------------
constexpr int OVR_UL = 8; // independent entries per thread in flight

// The value-bucket function over a key range kr[0] .. kr[1] (MAXK, 0: no key was seen -- one bucket): (key - kmin) >> shift, clamped
// to 0 .. last.  The rank kernels' table has 2^lg - 1 buckets (last = 2^lg - 2), the partition's histogram 2^lg (last = 2^lg - 1).
template <typename KeyT> struct OvrBuckets {
    KeyT kmin, last;
    int shift;
    __device__ __forceinline__ OvrBuckets(const KeyT *kr, int lg, KeyT last_) : last(last_) {
        const bool have_range = kr[1] >= kr[0];
        const KeyT kmax = have_range ? kr[1] : (KeyT)0;
        kmin = have_range ? kr[0] : (KeyT)0;
        shift = max(0, key_range_bits((KeyT)(kmax - kmin)) - lg);
    }
    __device__ __forceinline__ u32 bucket(KeyT key) const {
        const KeyT d = key > kmin ? (KeyT)((KeyT)(key - kmin) >> shift) : (KeyT)0;
        return (u32)(d < last ? d : last);
    }
    // table entry of a key: 1 + its bucket.  Entry 0 stays 0, so that after the scan and the scattering pass bucket b is
    // [entry b, entry b + 1): two neighbouring 16-bit reads, no special case for the first bucket.
    __device__ __forceinline__ u32 entry(KeyT key) const { return bucket(key) + 1u; }
};

// The smallest / largest key among entries tid, tid + NT * step, .. below n into kr[0] / kr[1] (set to MAXK / 0 and a barrier before;
// a barrier before they are read).  key_at(i, key): entry i's key; false = the entry does not take part.
template <int NT, typename KeyT, typename KeyAt>
__device__ __forceinline__ void ovr_sampled_range(int n, int step, KeyT *kr, int tid, KeyAt &&key_at) {
    KeyT tmin = KeyInfo<KeyT>::MAXK, tmax = (KeyT)0;
    for (int i = tid; i < n; i += NT * step) {
        KeyT key;
        if (key_at(i, key)) { tmin = key < tmin ? key : tmin; tmax = key > tmax ? key : tmax; }
    }
    wg_key_range(tmin, tmax, kr, tid & 63);
}

template <int NT, typename KeyT> __device__ __forceinline__ void ovr_clear_run(const OvrRankLds<KeyT> &S, int tid) {
    for (int b = tid; b < S.nbkt / 2; b += NT) S.tab[b] = 0u;
    if (tid == 0) { S.s_k[0] = KeyInfo<KeyT>::MAXK; S.s_k[1] = (KeyT)0; S.s_misc[OVR_N_ZERO] = 0u; S.s_misc[OVR_N_NEG] = 0u; S.s_misc[OVR_FULLEST] = 0u; }
}

// Bucket sizes (COUNT).  A CSC column's stored zeros and negatives are counted in the same walk, with or without COUNT: one pass.
template <int NT, typename KeyT, typename Src>
__device__ __forceinline__ void ovr_count_keys(const OvrRankLds<KeyT> &S, const Src &src, long long k0, long long k1, const OvrBuckets<KeyT> &vb, bool count, int tid) {
    u32 my_zero = 0, my_neg = 0;
    ovr_for_entries<false, NT, OVR_UL, Src, KeyT>(src, k0, k1, tid, [&](int, long long, KeyT key, bool nz, int) {
        if (nz) {
            if constexpr (!Src::PARTS) my_neg += key < KeyInfo<KeyT>::ZEROK ? 1u : 0u;
            if (count) {
                const u32 e = vb.entry(key);
                atomicAdd(&S.tab[e >> 1], (e & 1u) ? 0x10000u : 1u); // no carry: a counter stays below 2^16
            }
        } else ++my_zero; // a stored zero is an implicit zero
    });
    if constexpr (!Src::PARTS) {
        my_zero = (u32)wave_sum((int)my_zero);
        my_neg = (u32)wave_sum((int)my_neg);
        if ((tid & 63) == 0) {
            if (my_zero) atomicAdd(&S.s_misc[OVR_N_ZERO], my_zero);
            if (my_neg) atomicAdd(&S.s_misc[OVR_N_NEG], my_neg);
        }
    }
}

// How crowded are the buckets?  true: the run of n keys takes the sorted form (uniform).  Two barriers; s_red is free again after them.
template <int NT, typename KeyT> __device__ __forceinline__ bool ovr_buckets_crowded(const OvrRankLds<KeyT> &S, int n, int tid) {
    u64 sq = 0;
    u32 mx = 0;
    for (int b = tid; b < S.nbkt / 2; b += NT) {
        const u32 x = S.tab[b], c0 = x & 0xFFFFu, c1 = x >> 16;
        sq += (u64)c0 * c0 + (u64)c1 * c1;
        mx = max(mx, max(c0, c1));
    }
    sq = wave_sum(sq);
    mx = (u32)wave_incl_scan_max((int)mx);
    if ((tid & 63) == 63) { S.s_red[tid >> 6] = sq; atomicMax(&S.s_misc[OVR_FULLEST], mx); }
    __syncthreads();
    u64 sumsq = 0;
    for (int w = 0; w < NT / 64; ++w) sumsq += S.s_red[w];
    const bool crowded = S.s_misc[OVR_FULLEST] > (u32)CSCO_MAX_BUCKET || sumsq > (u64)CSCO_MAX_AVG * (u64)n;
    __syncthreads();
    return crowded;
}

// Keys into their buckets (the table holds exclusive offsets) and the pad behind them; after the next barrier bucket b = [tab16[b], tab16[b + 1]).
template <int NT, typename KeyT, typename Src>
__device__ __forceinline__ void ovr_scatter(const OvrRankLds<KeyT> &S, const Src &src, long long k0, long long k1, const OvrBuckets<KeyT> &vb, int n, int tid) {
    ovr_for_entries<false, NT, OVR_UL, Src, KeyT>(src, k0, k1, tid, [&](int, long long, KeyT key, bool nz, int) {
        if (nz) {
            const u32 e = vb.entry(key);
            const u32 old = atomicAdd(&S.tab[e >> 1], (e & 1u) ? 0x10000u : 1u);
            S.A[(e & 1u) ? (old >> 16) : (old & 0xFFFFu)] = key;
        }
    });
    if (tid < 4) S.A[n + tid] = KeyInfo<KeyT>::MAXK; // the walk reads up to 3 keys past a bucket's end
}

// Every key against its bucket: the first four keys in straight-line code (the average bucket holds two); keys past a bucket's end
// belong to later buckets (larger than q) or are the MAXK pad and count for neither sum.  Returns the thread's share of the tie sum.
template <int NT, typename KeyT, typename Src, typename AccAdd>
__device__ __forceinline__ u64 ovr_bucket_walk(const OvrRankLds<KeyT> &S, const Src &src, long long k0, long long k1, const OvrBuckets<KeyT> &vb, u64 base, long long n0,
                                               int tid, AccAdd &&acc_add) {
    constexpr KeyT ZEROK = KeyInfo<KeyT>::ZEROK;
    const u64 c_neg = 2ull * base + 1ull + (1ull << CSCO_CNT_SHIFT), c_pos = c_neg + 2ull * (u64)n0;
    const KeyT *A = S.A;
    u32 tie32 = 0; // at most 64 keys per thread x 192^2
    ovr_for_entries<true, NT, OVR_UL, Src, KeyT>(src, k0, k1, tid, [&](int, long long, KeyT q, bool nz, int cd) {
        if (nz) {
            const u32 e = vb.entry(q);
            const u32 lo = S.tab16[e - 1], hi = S.tab16[e];
            const KeyT a0 = A[lo], a1 = A[lo + 1], a2 = A[lo + 2], a3 = A[lo + 3];
            u32 less = (a0 < q ? 1u : 0u) + (a1 < q ? 1u : 0u) + (a2 < q ? 1u : 0u) + (a3 < q ? 1u : 0u);
            u32 eq = (a0 == q ? 1u : 0u) + (a1 == q ? 1u : 0u) + (a2 == q ? 1u : 0u) + (a3 == q ? 1u : 0u);
            for (u32 j = lo + 4; j < hi; j += 4) { // rare
                const KeyT b0 = A[j], b1 = A[j + 1], b2 = A[j + 2], b3 = A[j + 3];
                less += (b0 < q ? 1u : 0u) + (b1 < q ? 1u : 0u) + (b2 < q ? 1u : 0u) + (b3 < q ? 1u : 0u);
                eq += (b0 == q ? 1u : 0u) + (b1 == q ? 1u : 0u) + (b2 == q ? 1u : 0u) + (b3 == q ? 1u : 0u);
            }
            eq = bucket_eq_padded(q, lo, hi, less, eq);
            acc_add(cd, ((q > ZEROK) ? c_pos : c_neg) + (u64)(2u * (lo + less) + eq));
            tie32 += eq * eq - 1u;
        }
    });
    return (u64)tie32;
}

// Sorted form: keys -> LDS (entries that take no part sort past the n keys, as the pad to whole sort chunks does), sort, tie blocks, two
// look-ups per entry.  false (uniform, nothing written): the padded run does not fit the key slots.
template <int NT, typename KeyT, typename Src, typename AccAdd>
__device__ __forceinline__ bool ovr_rank_sorted(const OvrRankLds<KeyT> &S, const Src &src, long long k0, long long k1, int n, int key_cap, u64 base, long long n0, u64 &tie,
                                                int tid, AccAdd &&acc_add) {
    constexpr int CH = 64 * CSCO_K;
    constexpr KeyT ZEROK = KeyInfo<KeyT>::ZEROK, MAXK = KeyInfo<KeyT>::MAXK;
    KeyT *A = S.A;
    const int ns = (int)(k1 - k0), ncap = (ns + CH - 1) / CH * CH;
    if (ncap > key_cap) return false;
    for (int i = ns + tid; i < ncap; i += NT) A[i] = MAXK;
    ovr_for_entries<false, NT, OVR_UL, Src, KeyT>(src, k0, k1, tid, [&](int, long long k, KeyT key, bool nz, int) { A[k - k0] = nz ? key : MAXK; });
    __syncthreads();
    block_sort_hybrid<KeyT, NT, CSCO_K>(A, ncap, tid);
    const u32 un = (u32)n, top = top_pow2(un);
    for (int i = tid; i < n; i += NT) {
        const KeyT k = A[i];
        if ((i == 0 || A[i - 1] != k) && i + 1 < n && A[i + 1] == k) {
            const u64 t = upper_bound_pow2(A, un, top, k) - (u32)i;
            tie += t * t * t - t;
        }
    }
    const u64 c_neg = 2ull * base + 1ull + (1ull << CSCO_CNT_SHIFT), c_pos = c_neg + 2ull * (u64)n0;
    ovr_for_entries<true, NT, OVR_UL, Src, KeyT>(src, k0, k1, tid, [&](int, long long, KeyT q, bool nz, int cd) {
        if (nz) {
            const u32 s = lower_bound_pow2(A, un, top, q);
            u32 e = s + 1;
            if (e < un && A[e] == q) e = upper_bound_pow2(A, un, top, q);
            acc_add(cd, ((q > ZEROK) ? c_pos : c_neg) + (u64)s + (u64)e);
        }
    });
    return true;
}

// Rank the run src[k0, k1): every key that takes part adds  2 (base + s) + t + 1 (+ 2 n0 when positive) + 1 << CSCO_CNT_SHIFT  to its
// group through acc_add(group, x); the thread's share of sum (t^3 - t) is added to tie.  base: keys of the column below the run's.
// n0: the column's zeros; a CSC column's stored zeros are added to it here, and its negatives are counted into nneg (a part's caller
// knows both).  sorted_form: take the sorted form whatever the buckets look like.  The caller has set up acc_add's accumulators (a
// barrier stands between here and the first add) and puts a barrier behind the run before LDS is used again.  false (uniform): the
// run cannot be taken -- it does not fit the key slots in its sorted form -- and nothing was added.
template <int NT, typename KeyT, typename Src, typename AccAdd>
__device__ __forceinline__ bool ovr_rank_run(const OvrRankLds<KeyT> &S, const Src &src, long long k0, long long k1, u64 base, long long &n0, long long &nneg,
                                             int lg_buckets, int key_cap, bool sorted_form, u64 &tie, int tid, AccAdd &&acc_add) {
    const int ns = (int)(k1 - k0);
    ovr_clear_run<NT>(S, tid);
    __syncthreads();
    ovr_sampled_range<NT>(ns, ns > 8 * NT ? 8 : 1, S.s_k, tid, [&](int i, KeyT &key) {
        bool nz;
        key = src.key_from(src.raw_v(k0 + i, true), true, nz);
        return nz;
    });
    __syncthreads();
    const OvrBuckets<KeyT> vb(S.s_k, lg_buckets, (KeyT)(S.nbkt - 2));
    if (!Src::PARTS || !sorted_form) ovr_count_keys<NT>(S, src, k0, k1, vb, !sorted_form, tid);
    __syncthreads();
    int n = ns; // the keys that take part
    if constexpr (!Src::PARTS) {
        n -= (int)S.s_misc[OVR_N_ZERO];
        n0 += (long long)S.s_misc[OVR_N_ZERO];
        nneg = (long long)S.s_misc[OVR_N_NEG];
    }
    if (n == 0) return true; // uniform
    if (!sorted_form) sorted_form = ovr_buckets_crowded<NT>(S, n, tid);
    if (sorted_form) return ovr_rank_sorted<NT>(S, src, k0, k1, n, key_cap, base, n0, tie, tid, acc_add);
    block_excl_scan_u16_waves<NT>(S.tab16, S.nbkt, (u32 *)S.s_red, tid); // (s_red: NW 64-bit slots, the scan wants NW words)
    ovr_scatter<NT>(S, src, k0, k1, vb, n, tid);
    __syncthreads();
    tie += ovr_bucket_walk<NT>(S, src, k0, k1, vb, base, n0, tid, acc_add);
    return true;
}

// The gene's statistics, once its runs are ranked: tie sum over the workgroup (+ the zeros' block, or the float64 form of the
// reference's sparse path), and per group the zeros at their rank (zeros_rank_sum2; z = the group's cells without a ranked key),
// 2 U of "the rest" (dense_ovr.py:57-61).  acc_of(g): group g's accumulator.  out_2u, out_tie: the gene's [G].
template <int NT, typename AccOf>
__device__ __forceinline__ void ovr_close_gene(u64 tie, u64 *s_red, bool tie_f64, long long n0, long long nneg, long long n_cells, const int *counts, int G,
                                               long long *out_2u, u64 *out_tie, int tid, AccOf &&acc_of) {
    constexpr u64 R2MASK = (1ull << CSCO_CNT_SHIFT) - 1ull;
    tie = wave_sum(tie);
    __syncthreads(); // (s_red's readers of the crowd test are done)
    if ((tid & 63) == 0) s_red[tid >> 6] = tie;
    __syncthreads();
    u64 tie_total = 0;
    for (int w = 0; w < NT / 64; ++w) tie_total += s_red[w];
    if (tie_f64) tie_total = tie_f64_sparse(tie_total, n0);
    else tie_total += (u64)n0 * (u64)n0 * (u64)n0 - (u64)n0;
    for (int g = tid; g < G; g += NT) {
        const long long n_g = counts[g];
        const u64 a = acc_of(g);
        const long long z = n_g - (long long)(a >> CSCO_CNT_SHIFT);
        const u64 r2 = (a & R2MASK) + zeros_rank_sum2(z, nneg, n0);
        out_2u[g] = 2ll * (n_cells - n_g) * n_g + n_g * (n_g + 1) - (long long)r2;
        out_tie[g] = tie_total;
    }
}
