// Dense one-versus-rest, any values: split a gene's non-zero keys by VALUE into parts of at most `cap` keys, for the kernels that rank a
// part at a time in LDS (k_ovr_rank_gene_parts, kernels_ovr_parts.h; k_pw_rank_pairs, kernels_pairwise_ranked.h).  Histogram over 8192
// value buckets, scan, part = cumulative count / quota, (key, group code) records appended per part in HBM.  Dense continuous OVR at
// C4 shape: 68 ms (segmented radix sort of (key, group) pairs in HBM) -> see DESIGN.
//
// Two kernels, one per way the keys lie in memory -- k_ovr_partition: gene-major rows of n_cells keys; k_ovr_partition_packed: the
// packed rows of k_group_compact -- each with its own two key walks (count, place).  Everything else is stated once below: the LDS
// layout (OvrpLds), the per-key count (ovrp_count_key), the plan (ovrp_plan), a record's placement (ovrp_put_record), the closing
// stores (ovrp_store_plan).  The bucket function and the sampled key range are the rank kernels' (OvrBuckets, ovr_sampled_range).
#pragma once
#include "kernels_ovr_rank.h"

#define OVRP_NT 512         // threads of the partition kernels
#define OVRP_LG 13          // their coarse buckets: (key - kmin) >> shift, 8192 of them over the gene's own key range
#define OVRP_PMAX 255       // parts per gene at most (8-bit part ids; 128 until late in round 5: a column of more cells than 128 parts hold left the route)

// The kernels' dynamic LDS, stated once for the host (ovrp_lds_bytes) and the kernels (OvrpSmem): byte offsets.
struct OvrpLds {
    static constexpr size_t NB = (size_t)1 << OVRP_LG;
    static constexpr size_t hist = 0;                                // [NB] words: counts, then exclusive offsets in value order
    static constexpr size_t tmp = hist + NB * 4;                     // [OVRP_NT] words: the scan's; the skewed plan's list of big buckets
    static constexpr size_t pstart = tmp + OVRP_NT * 4;              // [OVRP_PMAX + 1] words: first record of each part
    static constexpr size_t pfill = pstart + (OVRP_PMAX + 1) * 4;    // [OVRP_PMAX] words: records placed so far
    static constexpr size_t s_mx = pfill + OVRP_PMAX * 4;            // [2] words: largest bucket (then: the skewed plan's parts), negatives
    static constexpr size_t s_k = (s_mx + 2 * 4 + 7) & ~(size_t)7;   // [2] keys: smallest / largest sampled non-zero key
    static constexpr size_t total = s_k + 2 * 8 + NB;                // part_of [NB] bytes, part of a bucket: right behind the two keys of either size
};
static_assert(OvrpLds::s_k % 8 == 0, "eight-byte keys");
static_assert(OVRP_NT >= 2 * 128 && OVRP_NT >= OVRP_PMAX, "tmp holds the skewed plan's 2 x 128 words; one thread clears each pfill word");
static inline size_t ovrp_lds_bytes() { return OvrpLds::total; }
template <typename KeyT> struct OvrpSmem {
    u32 *hist, *tmp, *pstart, *pfill, *s_mx; KeyT *s_k; unsigned char *part_of;
    __device__ __forceinline__ OvrpSmem(unsigned char *smem)
        : hist((u32 *)(smem + OvrpLds::hist)), tmp((u32 *)(smem + OvrpLds::tmp)), pstart((u32 *)(smem + OvrpLds::pstart)), pfill((u32 *)(smem + OvrpLds::pfill)),
          s_mx((u32 *)(smem + OvrpLds::s_mx)), s_k((KeyT *)(smem + OvrpLds::s_k)), part_of((unsigned char *)(s_k + 2)) {}
};

// Parts of a gene whose coarse buckets are SKEWED (one holds more than a quarter of `cap`: heavy ties -- log1p of raw counts, counts times a
// constant -- or a crowd of values in a sliver of the range).  A bucket above cap / 2 ("big") gets a part of its own; the small buckets
// are split evenly by their own running count S (the big ones left out) with a quota of cap / 2, so a part of small buckets holds at most
// cap keys:    part(b) = S(b) / (cap / 2) + 2 B(b) + [b is big],   B(b) = big buckets before b
// -- monotone in b, ids with gaps (an unused id is an empty part: its start is the next part's).  A big bucket's part may exceed `cap`: the
// rank kernel takes it in its streaming form when all its keys are equal (one value: nothing to rank, the records are only counted per
// group) and hands the gene to the general route when they are not.  hist: exclusive bucket offsets; big_list: 2 x 128 words of scratch;
// *np_out: the parts, or 0xFFFFFFFF (more than OVRP_PMAX ids, more than 128 big buckets).  Every thread of the workgroup calls it.
// (Until late in round 5 a skewed gene left the route at once: dense OVR on log1p of raw counts ran the per-gene radix sort in HBM, 24 ms
// for 2048 genes against 5 for tie-free values.)
template <int NT>
__device__ __forceinline__ void ovrp_assign_parts_skewed(const u32 *hist, int NB, u32 n, u32 cap, unsigned char *part_of, u32 *pstart, u32 *big_list,
                                                         u32 *np_out, int tid) {
    u32 *bigb = big_list, *bigc = big_list + 128;
    const u32 half = cap / 2u;
    if (tid == 0) *np_out = 0u; // (first: the number of big buckets; then: the largest part id)
    for (int p = tid; p <= OVRP_PMAX; p += NT) pstart[p] = n;
    __syncthreads();
    for (int b = tid; b < NB; b += NT) {
        const u32 c = (b + 1 < NB ? hist[b + 1] : n) - hist[b];
        if (c > half) { const u32 i = atomicAdd(np_out, 1u); if (i < 128u) { bigb[i] = (u32)b; bigc[i] = c; } }
    }
    __syncthreads();
    const u32 nbig = *np_out;
    __syncthreads();
    if (nbig > 128u) { if (tid == 0) *np_out = 0xFFFFFFFFu; __syncthreads(); return; }
    if (tid == 0) *np_out = 0u;
    __syncthreads();
    u32 pmax = 0;
    for (int b = tid; b < NB; b += NT) {
        const u32 lo = hist[b], c = (b + 1 < NB ? hist[b + 1] : n) - lo;
        u32 B = 0, BS = 0;
        for (u32 i = 0; i < nbig; ++i) { const bool before = bigb[i] < (u32)b; B += before ? 1u : 0u; BS += before ? bigc[i] : 0u; }
        const u32 pid = (lo - BS) / half + 2u * B + (c > half ? 1u : 0u);
        part_of[b] = (unsigned char)min(pid, (u32)OVRP_PMAX - 1);
        if (c) { pmax = max(pmax, pid); if (pid < (u32)OVRP_PMAX) atomicMin(&pstart[pid], lo); }
    }
    atomicMax(np_out, pmax);
    __syncthreads();
    const u32 top = *np_out;
    __syncthreads();
    if (top >= (u32)OVRP_PMAX) { if (tid == 0) *np_out = 0xFFFFFFFFu; __syncthreads(); return; }
    if (tid == 0) { // an unused id starts where the next part does
        for (int p = (int)top - 1; p >= 0; --p) pstart[p] = min(pstart[p], pstart[p + 1]);
        pstart[top + 1] = n;
        *np_out = n ? top + 1u : 0u;
    }
    __syncthreads();
}

// ---- what the two kernels share -------------------------------------------------------------------------------------------------------
// Start of a gene (a barrier behind it).
template <typename KeyT> __device__ __forceinline__ void ovrp_clear(const OvrpSmem<KeyT> &S, int nt, int tid) {
    for (int b = tid; b < (int)OvrpLds::NB; b += nt) S.hist[b] = 0u;
    if (tid < OVRP_PMAX) S.pfill[tid] = 0u;
    if (tid == 0) { S.s_mx[0] = 0u; S.s_mx[1] = 0u; S.s_k[0] = KeyInfo<KeyT>::MAXK; S.s_k[1] = (KeyT)0; }
}
// The bucket function over the sampled key range (any monotone function partitions correctly: keys outside the sampled range are clamped
// into the first / last bucket).
template <typename KeyT> __device__ __forceinline__ OvrBuckets<KeyT> ovrp_buckets(const OvrpSmem<KeyT> &S) {
    return OvrBuckets<KeyT>(S.s_k, OVRP_LG, (KeyT)(OvrpLds::NB - 1));
}
// Count walk, per key (the zero key: no record -- a zero of the row, or the walk's "past the end" mark) and per thread at its end.
template <typename KeyT> __device__ __forceinline__ void ovrp_count_key(const OvrpSmem<KeyT> &S, const OvrBuckets<KeyT> &vb, KeyT key, u32 &neg) {
    if (key != KeyInfo<KeyT>::ZEROK) {
        atomicAdd(&S.hist[vb.bucket(key)], 1u);
        neg += key < KeyInfo<KeyT>::ZEROK ? 1u : 0u;
    }
}
template <typename KeyT> __device__ __forceinline__ void ovrp_count_done(const OvrpSmem<KeyT> &S, u32 neg, int lane) {
    neg = (u32)wave_sum((int)neg);
    if (lane == 0 && neg) atomicAdd(&S.s_mx[1], neg);
}

// The plan of a gene, once the count walk and a barrier are behind: the census' tail (largest bucket, the scan, the key and negative
// counts), quota or skew, the parts' starts (pstart) and every bucket's part (part_of).  bad (uniform): more parts than ids -- the gene
// goes to the general route, gene_info says so, nothing else is to be written.  Ends on a barrier unless bad.
struct OvrpPlan {
    u32 n, nneg, n_parts; // non-zero keys, negatives among them, parts
    int p_bits;           // bits of the values 0 .. n_parts
    bool bad;
};
template <int NT, typename KeyT> __device__ __forceinline__ OvrpPlan ovrp_plan(const OvrpSmem<KeyT> &S, int cap, u32 *gi, int tid) {
    constexpr int NB = (int)OvrpLds::NB;
    const int lane = tid & 63;
    OvrpPlan pl;
    u32 mx = 0;
    for (int b = tid; b < NB; b += NT) mx = max(mx, S.hist[b]);
    mx = (u32)wave_incl_scan_max((int)mx);
    if (lane == 63) atomicMax(&S.s_mx[0], mx);
    __syncthreads();
    mx = S.s_mx[0];
    pl.n = block_excl_scan_inplace<NT>(S.hist, NB, S.tmp, tid);
    pl.nneg = S.s_mx[1];
    // part of a bucket = keys before it / quota; no bucket is larger than a quarter of cap, so every part gets a bucket
    // boundary and holds fewer than quota + mx = cap keys
    const bool skew = (unsigned long long)mx * 4ull > (unsigned long long)cap;
    const u32 quota = skew ? 1u : (u32)cap - mx;
    pl.n_parts = pl.n ? (pl.n - 1) / quota + 1 : 0u;
    if (skew) { // (uniform) crowded buckets get parts of their own
        ovrp_assign_parts_skewed<NT>(S.hist, NB, pl.n, (u32)cap, S.part_of, S.pstart, S.tmp, &S.s_mx[0], tid);
        pl.n_parts = S.s_mx[0];
    }
    pl.bad = pl.n_parts > (u32)OVRP_PMAX;
    pl.p_bits = 0;
    if (pl.bad) { // uniform
        if (tid == 0) { gi[0] = pl.n; gi[1] = pl.nneg; gi[2] = 0u; gi[3] = 1u; }
        return pl;
    }
    if (!skew) {
        for (int b = tid; b < NB; b += NT) {
            const u32 p = S.hist[b] / quota;
            S.part_of[b] = (unsigned char)min(p, (u32)OVRP_PMAX - 1); // (empty buckets past the last key may overshoot)
            if (p < pl.n_parts && (b == 0 || S.hist[b - 1] / quota != p)) S.pstart[p] = S.hist[b];
            // the last bucket may reach into a part that no bucket starts (key n - 1 lies one part beyond the bucket's first key, and no
            // bucket follows): that part is empty -- its keys are placed with the bucket's, in part p
            if (b == NB - 1 && p + 1 < pl.n_parts) S.pstart[p + 1] = pl.n;
        }
        if (tid == 0) S.pstart[pl.n_parts] = pl.n;
    }
    pl.p_bits = 32 - __clz(pl.n_parts);
    __syncthreads();
    return pl;
}

// Place walk, per key: the record (key, code) into the next free slot of its part, out_keys / out_codes being the gene's rows.  Every
// lane of the wavefront calls it, a lane without a record with the zero key.  lt_mask: the lanes below this one.
template <typename KeyT>
__device__ __forceinline__ void ovrp_put_record(const OvrpSmem<KeyT> &S, const OvrpPlan &pl, const OvrBuckets<KeyT> &vb, KeyT key, int code, KeyT *out_keys,
                                                u16 *out_codes, int lane, u64 lt_mask) {
    const bool nz = key != KeyInfo<KeyT>::ZEROK;
    const int p = nz ? (int)S.part_of[vb.bucket(key)] : (int)pl.n_parts; // n_parts = not a record
    // lanes with the same part, without a loop over parts: match the bits of p through ballots (as many bits as
    // n_parts needs: 3 for the 6 parts of a half-empty 300 000-cell column)
    // (at least bit 0: without parts every lane carries p = 0 and the round leaves m as it is -- no zero-trip test per key)
    u64 m = ~0ull;
    int bit = 0;
    do {
        const bool on = (p >> bit) & 1;
        const u64 bl = __ballot(on);
        m &= on ? bl : ~bl;
    } while (++bit < pl.p_bits);
    if (nz) { // one LDS atomic per (wavefront, part present in it): the lowest lane of each match set
        const int leader = __ffsll((long long)m) - 1;
        u32 b0 = 0;
        if (lane == leader) b0 = atomicAdd(&S.pfill[p], (u32)__popcll(m));
        b0 = (u32)__shfl((int)b0, leader);
        const u32 slot = S.pstart[p] + b0 + (u32)__popcll(m & lt_mask);
        out_keys[slot] = key;
        out_codes[slot] = (u16)code;
    }
}

// The gene's plan for the rank kernel: part_start [OVRP_PMAX + 1], gene_info [4]: non-zeros, negatives, parts, flag.
template <typename KeyT> __device__ __forceinline__ void ovrp_store_plan(const OvrpSmem<KeyT> &S, const OvrpPlan &pl, u32 *ps_out, u32 *gi, int tid) {
    if (tid <= (int)pl.n_parts) ps_out[tid] = S.pstart[tid];
    if (tid == 0) { gi[0] = pl.n; gi[1] = pl.nneg; gi[2] = pl.n_parts; gi[3] = 0u; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Gene-major key rows, group-contiguous positions (what k_transpose_permute writes).
// ---------------------------------------------------------------------------------------------------------------------
struct OvrPartParams {
    const void *Xt;            // [n_genes][stride] keys
    long long stride;
    int n_genes, n_cells;
    const int *code_by_pos;    // [n_cells]
    int cap;                   // keys per part at most
    void *out_keys;            // [n_genes][stride]
    u16 *out_codes;            // [n_genes][stride]
    u32 *part_start;           // [n_genes][OVRP_PMAX + 1]
    u32 *gene_info;            // [n_genes][4]: non-zeros, negatives, parts, flag
};

template <typename KeyT>
__global__ __launch_bounds__(OVRP_NT) void k_ovr_partition(OvrPartParams P) {
    constexpr int NT = OVRP_NT, UL = 8;
    constexpr KeyT ZEROK = KeyInfo<KeyT>::ZEROK;
    extern __shared__ __align__(16) unsigned char smem[];
    const OvrpSmem<KeyT> S(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int N = P.n_cells;
    const u64 lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int gene = blockIdx.x; gene < P.n_genes; gene += gridDim.x) {
        const KeyT *row = (const KeyT *)P.Xt + (size_t)gene * P.stride;
        ovrp_clear(S, NT, tid);
        __syncthreads();
        ovr_sampled_range<NT>(N, 8, S.s_k, tid, [&](int i, KeyT &key) { key = row[i]; return key != ZEROK; }); // every 8th row of NT keys
        __syncthreads();
        const OvrBuckets<KeyT> vb = ovrp_buckets(S);
        u32 neg = 0;
        for (int i0 = 0; i0 < N; i0 += NT * UL) {
            KeyT k[UL];
#pragma unroll
            for (int u = 0; u < UL; ++u) { const int i = i0 + u * NT + tid; k[u] = i < N ? row[i] : ZEROK; }
#pragma unroll
            for (int u = 0; u < UL; ++u) ovrp_count_key(S, vb, k[u], neg);
        }
        ovrp_count_done(S, neg, lane);
        __syncthreads();
        u32 *gi = P.gene_info + (size_t)gene * 4;
        const OvrpPlan pl = ovrp_plan<NT>(S, P.cap, gi, tid);
        if (pl.bad) { // uniform
            __syncthreads();
            continue;
        }
        KeyT *out_keys = (KeyT *)P.out_keys + (size_t)gene * P.stride;
        u16 *out_codes = P.out_codes + (size_t)gene * P.stride;
        for (int i0 = 0; i0 < N; i0 += NT * UL) {
            KeyT k[UL];
            int cd[UL];
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const int i = i0 + u * NT + tid;
                k[u] = i < N ? row[i] : ZEROK;
                cd[u] = i < N ? P.code_by_pos[i] : 0;
            }
#pragma unroll
            for (int u = 0; u < UL; ++u) ovrp_put_record(S, pl, vb, k[u], cd[u], out_keys, out_codes, lane, lt_mask);
        }
        ovrp_store_plan(S, pl, P.part_start + (size_t)gene * (OVRP_PMAX + 1), gi, tid);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same split over the PACKED key rows of k_group_compact (kernels_ovo_compact.h): only the non-zero keys are there -- block
// after block of groups, blk_cnt[gene][block] keys from slot blk_out[block] on, a group's keys back to back with the next
// group's -- so the three walks read 45 % of a half-empty matrix instead of all of it.  One wavefront takes a block at a time;
// a key's group code is the block's first group plus the group ends (running sums of nnz[gene][group]) at or below the key's
// offset: a few compares against scalars.
// ---------------------------------------------------------------------------------------------------------------------
struct OvrPartPackedParams {
    const void *Xt;            // [n_genes][stride] packed keys
    long long stride;
    int n_genes, G, nblk;
    const u16 *nnz;            // [n_genes][G]
    const u32 *blk_cnt;        // [n_genes][nblk]
    const int *blk_g0, *blk_g1, *blk_out; // [nblk] first group, one past the last, first key slot
    int cap;
    void *out_keys;
    u16 *out_codes;
    u32 *part_start, *gene_info; // as OvrPartParams
    // the kernel's COOP form: some blocks are LONG (more than OVRP_LONG_ROWS rows and at most 64 groups: a cluster of thousands of cells, the
    // control group of a screen): their 512-key units are dealt over ALL the wavefronts (unit u of the i-th long block: wavefront (u + i) % NW)
    // instead of one wavefront walking the block alone; the other blocks stay with their wavefront
    int n_long;
    const int *long_blk;            // [n_long] the long blocks
    const unsigned char *blk_is_long; // [nblk]
};
#define OVRP_LONG_ROWS 4096

template <typename KeyT, bool COOP = false>
__global__ __launch_bounds__(OVRP_NT) void k_ovr_partition_packed(OvrPartPackedParams P) {
    constexpr int NT = OVRP_NT, NW = NT / 64;
    constexpr KeyT ZEROK = KeyInfo<KeyT>::ZEROK;
    constexpr KeyT MAXK = KeyInfo<KeyT>::MAXK;
    extern __shared__ __align__(16) unsigned char smem[];
    const OvrpSmem<KeyT> S(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u64 lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    constexpr int UL = 8; // 64-key pieces of a block in flight per wavefront (a block of ~1024 rows holds ~500 keys)
    const int gene = blockIdx.x;
    const KeyT *row = (const KeyT *)P.Xt + (size_t)gene * P.stride;
    const u32 *bcnt = P.blk_cnt + (size_t)gene * P.nblk;
    const u16 *nnz = P.nnz + (size_t)gene * P.G;
    ovrp_clear(S, NT, tid);
    __syncthreads();
    { // key range for the bucket function, from every 8th block
        KeyT tmin = MAXK, tmax = (KeyT)0;
        if (COOP) { // (and every 8th 64-key piece of the long blocks)
            for (int i8 = wave; i8 < P.n_long; i8 += NW) {
                const int b = P.long_blk[i8], n_b = (int)bcnt[b];
                const KeyT *src = row + P.blk_out[b];
                for (int i = lane; i < n_b; i += 64 * 8) { const KeyT k = src[i]; tmin = k < tmin ? k : tmin; tmax = k > tmax ? k : tmax; }
            }
        }
        for (int b = wave * 8; b < P.nblk; b += NW * 8) {
            if (COOP && P.blk_is_long[b]) continue;
            const int n_b = (int)bcnt[b];
            const KeyT *src = row + P.blk_out[b];
            for (int i = lane; i < n_b; i += 64) { const KeyT k = src[i]; tmin = k < tmin ? k : tmin; tmax = k > tmax ? k : tmax; }
        }
        wg_key_range(tmin, tmax, S.s_k, lane);
    }
    __syncthreads();
    const OvrBuckets<KeyT> vb = ovrp_buckets(S);
    static_assert((NW & (NW - 1)) == 0, "units are dealt by (u + b) % NW");
    // both walks (COOP: the wavefront's own blocks, the long ones left out, then its units of the long blocks)
    const int n_own = (P.nblk - wave + NW - 1) / NW;
    {
        u32 neg = 0;
        for (int it = 0; it < n_own + (COOP ? P.n_long : 0); ++it) {
            const bool lng = COOP && it >= n_own;
            const int b = lng ? P.long_blk[it - n_own] : wave + it * NW;
            if (COOP && !lng && P.blk_is_long[b]) continue;
            const int n_b = (int)bcnt[b];
            const KeyT *src = row + P.blk_out[b];
            const int o_first = lng ? ((wave - (it - n_own)) & (NW - 1)) * (64 * UL) : 0, o_step = lng ? NW * 64 * UL : 64 * UL;
            for (int o = o_first; o < n_b; o += o_step) {
                KeyT k[UL];
#pragma unroll
                for (int u = 0; u < UL; ++u) { const int i = o + u * 64 + lane; k[u] = i < n_b ? src[i] : ZEROK; }
#pragma unroll
                for (int u = 0; u < UL; ++u) ovrp_count_key(S, vb, k[u], neg); // (packed keys are never the zero key: it marks "past the end")
            }
        }
        ovrp_count_done(S, neg, lane);
    }
    __syncthreads();
    u32 *ginfo = P.gene_info + (size_t)gene * 4;
    const OvrpPlan pl = ovrp_plan<NT>(S, P.cap, ginfo, tid);
    if (pl.bad) return; // uniform
    KeyT *out_keys = (KeyT *)P.out_keys + (size_t)gene * P.stride;
    u16 *out_codes = P.out_codes + (size_t)gene * P.stride;
    for (int it = 0; it < n_own + (COOP ? P.n_long : 0); ++it) {
        const bool split = COOP && it >= n_own; // a long block (at most 64 groups: its group ends sit in a register): this wavefront's units of it
        const int b = split ? P.long_blk[it - n_own] : wave + it * NW;
        if (COOP && !split && P.blk_is_long[b]) continue;
        const int n_b = (int)bcnt[b];
        const KeyT *src = row + P.blk_out[b];
        int gcur = P.blk_g0[b];
        const int glast = P.blk_g1[b];
        const int o_first = split ? ((wave - (it - n_own)) & (NW - 1)) * (64 * UL) : 0, o_step = split ? NW * 64 * UL : 64 * UL;
        if (COOP && o_first >= n_b) continue;
        int gend = gcur < glast ? (int)nnz[gcur] : 0; // offset (inside the block) where group gcur's keys end
        // A block of at most 64 groups (the usual case: ~7 groups of ~150 cells per 1024 rows) keeps its group ends in ONE register,
        // lane l = the offset where group g0 + l ends: the walks below then read a lane instead of loading nnz[g] from memory -- a
        // chain of dependent loads per 64-key piece otherwise.
        const int g0 = gcur, ng = glast - g0;
        const bool ends_in_lanes = ng <= 64;
        int endv = 0, gi = 0; // gi: gcur - g0
        // (a group of 65535 cells and more is the LAST of its block -- a block closes at 1024 rows -- and a block's last end is never looked
        //  at: the 16-bit lengths may saturate there)
        if (ends_in_lanes) endv = wave_incl_scan_add(lane < ng ? (int)nnz[g0 + lane] : 0);
        for (int o = o_first; o < n_b; o += o_step) {
            if (split) gi = min(ng - 1, (int)__popcll(__ballot(lane < ng && endv <= o))); // the groups that end at or before this unit's first key
            KeyT k[UL];
#pragma unroll
            for (int u = 0; u < UL; ++u) { const int i = o + u * 64 + lane; k[u] = i < n_b ? src[i] : ZEROK; }
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                const int off = o + u * 64 + lane;
                if (o + u * 64 >= n_b) break; // uniform
                // group code: gcur + the group ends at or below this key's offset (empty groups repeat an end: skipped over)
                int cd = gcur;
                if (ends_in_lanes) { // uniform
                    const int piece_end = o + u * 64 + 64;
                    cd = g0 + gi;
                    int j = gi, e = __builtin_amdgcn_readlane(endv, __builtin_amdgcn_readfirstlane(gi));
                    while (e < piece_end && j + 1 < ng) { // uniform
                        cd += off >= e ? 1 : 0;
                        ++j;
                        e = __builtin_amdgcn_readlane(endv, __builtin_amdgcn_readfirstlane(j));
                    }
                    while (gi + 1 < ng && __builtin_amdgcn_readlane(endv, __builtin_amdgcn_readfirstlane(gi)) <= piece_end) ++gi;
                } else {
                    int g = gcur, e = gend;
                    while (e < o + u * 64 + 64 && g + 1 < glast) { // uniform
                        cd += off >= e ? 1 : 0;
                        ++g;
                        e += (int)nnz[g];
                    }
                    // the next piece starts at o + u * 64 + 64: advance past the groups that end at or before it
                    while (gend <= o + u * 64 + 64 && gcur + 1 < glast) { ++gcur; gend += (int)nnz[gcur]; }
                }
                ovrp_put_record(S, pl, vb, k[u], cd, out_keys, out_codes, lane, lt_mask);
            }
        }
    }
    __syncthreads();
    ovrp_store_plan(S, pl, P.part_start + (size_t)gene * (OVRP_PMAX + 1), ginfo, tid);
}
