// CSC one-versus-rest for ANY values in ONE kernel per gene, without a sort.  A rank needs, for every stored entry, the
// tie block [s, e) its value occupies in the sorted column.  The gene's stored non-zeros are dealt into LDS buckets by
// value ((key - kmin) >> shift, 8192 or 16384 buckets with 16-bit offsets: a counting pass, a scan, a scattering pass), and every entry then
// counts the smaller and the equal keys INSIDE ITS OWN BUCKET (a few keys): s = bucket start + #smaller, e = s + #equal,
// 2 * avg_rank = s + e + 1 goes to its group's LDS accumulator and e - s (the tie block length t) gives the tie term as
// sum over entries of (t^2 - 1) = sum over blocks of (t^3 - t).  Nothing but the CSC arrays is read and nothing but the
// [gene][G] statistics is written; the general route it replaces regroups the entries in HBM (k_csc_regroup), sorts
// (key, group) pairs with a segmented radix sort in HBM and sweeps them (k_ovr_gene).
//
// Columns whose values crowd into few buckets (heavy ties, an outlier stretching the range) take the second form in the
// same kernel: the keys are sorted in LDS as bare keys (block_sort_hybrid) and every entry looks its value up with two
// binary searches.  Both forms, step by step, are ovr_rank_run (kernels_ovr_rank.h) over the column's stored entries; this
// file holds what is the CSC column's own: where its entries are, the accumulators that may live in HBM, the fallback flag.
//
// Device counterpart of sparse_ovr_mwu_kernel + its CSC entry (illico/ovr/sparse_ovr.py:23-97, :100-155) and
// _accumulate_group_ranksums_from_argsort (utils/ranking.py:7-49) for one gene at a time; the zeros stay implicit
// (sparse_ovr.py:70-83): n0 = N - nnz cells tie at rank n_neg + (n0 + 1) / 2 and shift every positive entry by n0.
//
// A gene with more stored entries than the LDS key buffer sets fallback[gene]; the host sends those genes through the
// general route.
//
// DENSE columns (and whatever else exceeds the LDS key buffer) take the same ranking in pieces: k_ovr_partition
// (kernels_ovr_partition.h) splits a gene's non-zero keys by VALUE into parts of at most key_cap keys, k_ovr_rank_gene_parts
// (kernels_ovr_parts.h) ranks each part in LDS exactly as a CSC column is ranked here -- a key's rank is the number of keys in lower
// parts plus its rank inside its own part.
#pragma once
#include "kernels_ovr_rank.h"

struct CscOvrParams {
    // CSC source
    const void *data, *indices, *indptr; // CSC arrays (device); stored entry k lives at data[k - kshift], indices[k - kshift]
    long long kshift;
    long long col0;                      // first gene of the batch (contiguous batches)
    const int *gene_cols;                // or: the batch's genes as a column list (absolute indices); nullptr = contiguous
    const int *codes;                    // [n_cells] group code per cell; nullptr: `indices` already holds group codes
    const u16 *codes16;                  // the same as 16-bit values (fewer cache lines per gather), or nullptr
    int nb;
    const int *counts;                   // [G]
    int G, dt, is_log1p;
    long long n_cells;
    int key_cap;                         // LDS key slots
    int lg_buckets;                      // log2 of the bucket count
    int force_sorted;                    // 1: every gene takes the sorted form (tests / A-B)
    u32 *fallback;                       // [nb] set to 1 for genes this kernel cannot take
    long long *out_2u;                   // [nb][G] 2 U (U of "the rest", dense_ovr.py:57-61)
    u64 *out_tie;                        // [nb][G] sum (t^3 - t), the same for every group of a gene
    int tie_f64;                         // out_tie = the bits of the float64 tie sum of the reference's sparse path (tie_f64_sparse)
    u64 *acc_global;                     // ACCG: [nb][G] the accumulators in HBM (zeroed by the host), for more groups than LDS holds beside the keys
    int g_lds;                           // ACCG: the groups [0, g_lds) keep theirs in LDS all the same (what is left beside the keys)
    // (per-group value sums are not formed here: they would be order-dependent float64 atomics.  The host launches
    //  k_csc_value_sums / k_group_sums_rows, kernels_sums.h, whose results do not depend on the order of arrival.)
};

// ACCG: the per-group accumulators in HBM (global atomics, read back at L2) instead of LDS: with thousands of groups acc[G] would
// take the key buffer's place (6000 groups: 48 KB; the C3 gene's 30 000 keys then no longer fit and the gene fell to the HBM sort).
template <typename InT, typename IdxT, typename KeyT, bool ACCG = false>
__global__ __launch_bounds__(CSCO_NT) void k_csc_ovr_gene(CscOvrParams P0) {
    // The parameter block is read where it lies (the kernel's only argument, at the start of the kernel-argument segment), field by field
    // where a step uses it: read through P0, every field is loaded into scalar registers at entry and kept there (kernels_ovo_compact.h).
    const CscOvrParams &P = *(const CscOvrParams *)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int NT = CSCO_NT;
    extern __shared__ __align__(16) unsigned char smem[];
    const int G = P.G;
    const int G_lds = ACCG ? P.g_lds : G; // groups whose accumulators are in LDS
    const OvrRankLds<KeyT> S(smem, G_lds, P.lg_buckets, NT / 64);
    const int tid = threadIdx.x;
    const IdxT *indptr = (const IdxT *)P.indptr;
    OvrSource<InT, IdxT, KeyT, false> src;
    src.data = (const InT *)P.data; src.indices = (const IdxT *)P.indices; src.codes = P.codes; src.codes16 = P.codes16;
    // one gene per workgroup
    for (int gene = blockIdx.x; gene < P.nb; gene += gridDim.x) {
        const long long col = P.gene_cols ? (long long)P.gene_cols[gene] : P.col0 + gene;
        const long long k0 = (long long)indptr[col] - P.kshift, k1 = (long long)indptr[col + 1] - P.kshift;
        if (k1 - k0 > (long long)P.key_cap) { // uniform: this gene takes the general route
            if (tid == 0) P.fallback[gene] = 1u;
            continue;
        }
        u64 *acc_hbm = ACCG ? P.acc_global + (size_t)gene * G : nullptr;
        for (int g = tid; g < G_lds; g += NT) S.acc[g] = 0ull;
        long long n0 = P.n_cells - (k1 - k0), nneg = 0; // zeros of the column: the cells without a stored entry, then the stored zeros
        u64 tie = 0;
        const bool taken = ovr_rank_run<NT>(S, src, k0, k1, 0ull, n0, nneg, P.lg_buckets, P.key_cap, P.force_sorted != 0, tie, tid, [&](int g, u64 x) {
            // one atomic per entry: LDS for the groups that fit there, HBM (L2) for the others
            if (!ACCG || g < G_lds) atomicAdd(&S.acc[g], x);
            else atomicAdd(&acc_hbm[g], x);
        });
        if (!taken) { // uniform
            if (tid == 0) P.fallback[gene] = 1u;
            __syncthreads();
            continue;
        }
        ovr_close_gene<NT>(tie, S.s_red, P.tie_f64 != 0, n0, nneg, P.n_cells, P.counts, G, P.out_2u + (size_t)gene * G, P.out_tie + (size_t)gene * G, tid, [&](int g) {
            return (ACCG && g >= G_lds) ? atomicAdd(&acc_hbm[g], 0ull) : S.acc[g]; // (HBM accumulators: read at L2, where the atomics landed)
        });
        __syncthreads();
    }
}
