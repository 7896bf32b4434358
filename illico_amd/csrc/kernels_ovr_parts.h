// Dense one-versus-rest, any values: the rank kernel over value-range parts (k_ovr_partition / k_ovr_partition_packed,
// kernels_ovr_partition.h, write the parts: (key, group code) records, part after part, each part at most key_cap records).
//
// One workgroup takes a GENE at a time (drawn from a queue) and walks its parts in value order; the per-group accumulators stay in
// LDS for the whole gene and the statistics leave once, as plain stores -- no per-part atomics into HBM, no finishing kernel.
// Per part: ovr_rank_run (kernels_ovr_rank.h: its steps, the bucket and the sorted form, are listed there) over the part's records,
// with the keys of the lower parts as rank offset -- what k_csc_ovr_gene does over a CSC column.  This file holds what is the parts'
// own: the queue, the part loop, and the streaming form of a part of one value.
//
// Device counterpart of illico/ovr/dense_ovr.py:46-75 + _accumulate_group_ranksums_from_argsort (illico/utils/ranking.py:7-49).
#pragma once
#include "kernels_ovr_partition.h"
#include "kernels_ovr_rank.h"

struct OvrRankGeneParams {
    const void *pkeys;        // [nb][pstride] non-zero keys, part after part
    const u16 *pcodes;        // [nb][pstride] their group codes
    long long pstride;
    const u32 *part_start;    // [nb][OVRP_PMAX + 1] first record of each part, relative to the gene
    const u32 *gene_info;     // [nb][4] non-zeros, negatives, parts, flag (1 = the gene left this route)
    u32 *gflag;               // [nb] set to 1 when a part cannot be ranked here
    u32 *gene_counter;        // work queue head (zeroed by the host)
    int nb, G;
    const int *counts;        // [G]
    long long n_cells;
    int key_cap, lg_buckets, force_sorted;
    long long *out_2u;        // [nb][G]
    u64 *out_tie;             // [nb][G]
};

template <typename KeyT, int NT_ = CSCO_NT>
__global__ __launch_bounds__(NT_) void k_ovr_rank_gene_parts(OvrRankGeneParams P0) {
    // The parameter block is read where it lies (the kernel's only argument, at the start of the kernel-argument segment), field by field
    // where a step uses it: read through P0, every field is loaded into scalar registers at entry and kept there (kernels_ovo_compact.h).
    const OvrRankGeneParams &P = *(const OvrRankGeneParams *)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int NT = NT_;
    constexpr KeyT ZEROK = KeyInfo<KeyT>::ZEROK;
    constexpr KeyT MAXK = KeyInfo<KeyT>::MAXK;
    extern __shared__ __align__(16) unsigned char smem[];
    const int G = P.G;
    const OvrRankLds<KeyT> S(smem, G, P.lg_buckets, NT / 64);
    const int tid = threadIdx.x;
    typedef OvrSource<KeyT, int, KeyT, true> Src;
    Src src;
    src.pkeys = (const KeyT *)P.pkeys; src.pcodes = P.pcodes;
    auto acc_add = [&](int g, u64 x) { atomicAdd(&S.acc[g], x); };

    for (;;) {
        if (tid == 0) S.s_misc[OVR_CALLER] = atomicAdd(P.gene_counter, 1u);
        __syncthreads();
        const int gene = (int)S.s_misc[OVR_CALLER];
        __syncthreads();
        if (gene >= P.nb) break; // every wavefront leaves here
        const u32 *gi = P.gene_info + (size_t)gene * 4;
        if (gi[3] != 0u) continue; // uniform: the partition sent this gene to the general route
        const int n_parts = (int)gi[2];
        long long n0 = P.n_cells - (long long)gi[0], nneg = gi[1]; // (the partition counted both: ovr_rank_run leaves them as they are)
        const u32 *ps = P.part_start + (size_t)gene * (OVRP_PMAX + 1);
        for (int g = tid; g < G; g += NT) S.acc[g] = 0ull;
        u64 tie = 0;
        bool bad = false;
        for (int part = 0; part < n_parts; ++part) {
            const u32 base = ps[part];
            const int n = (int)(ps[part + 1] - base);
            if (n == 0) continue;
            const long long k0 = (long long)gene * P.pstride + base, k1 = k0 + n;
            if (n > (P.key_cap & ~1023)) { // (uniform; the sorted form rounds a part up to 1024 keys) a part beyond the key slots: a crowded coarse bucket that the partition gave a part of its own
                // (ovrp_assign_parts_skewed).  ONE value -- the ties of log1p'd or scaled counts -- needs no ranking: every record stands
                // at base .. base + n - 1 with n equals; the records are only counted per group.  Different values: the general route's gene.
                if (tid == 0) { S.s_k[0] = MAXK; S.s_k[1] = (KeyT)0; }
                __syncthreads();
                ovr_sampled_range<NT>(n, 1, S.s_k, tid, [&](int i, KeyT &key) { key = src.pkeys[k0 + i]; return true; });
                __syncthreads();
                const KeyT q = S.s_k[0];
                const bool one_value = S.s_k[1] == q;
                __syncthreads();
                if (!one_value) { bad = true; break; }
                const u64 add = 2ull * (u64)base + 1ull + (1ull << CSCO_CNT_SHIFT) + ((q > ZEROK) ? 2ull * (u64)n0 : 0ull) + (u64)n;
                for (long long k = k0 + tid; k < k1; k += NT) acc_add(src.pcodes[k], add);
                if (tid == 0) tie += (u64)n * ((u64)n * (u64)n - 1ull);
                __syncthreads();
                continue;
            }
            if (!ovr_rank_run<NT>(S, src, k0, k1, (u64)base, n0, nneg, P.lg_buckets, P.key_cap, P.force_sorted != 0, tie, tid, acc_add)) { bad = true; break; } // uniform
            __syncthreads(); // the table and the key buffer are free for the next part
        }
        if (bad) { // uniform
            if (tid == 0) P.gflag[gene] = 1u;
            __syncthreads();
            continue;
        }
        ovr_close_gene<NT>(tie, S.s_red, false, n0, nneg, P.n_cells, P.counts, G, P.out_2u + (size_t)gene * G, P.out_tie + (size_t)gene * G, tid, [&](int g) { return S.acc[g]; });
        __syncthreads();
    }
}
