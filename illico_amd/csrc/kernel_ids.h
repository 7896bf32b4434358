// The profiled kernels, listed once: X(id, name).  The KID_* enum (here) and kKernelNames (core.hip) are both expanded from this list, so an id and
// its name cannot drift apart.  The order is the id ("profile_only" selects by it, illico_profile_get indexes by it) and the name keys
// profiles/traffic.json: append new kernels at the end.  Host-only, no HIP.
#pragma once

#define ILLICO_KERNELS(X) \
    X(KID_TRANSPOSE, "k_transpose_permute") \
    X(KID_OVO_RANK, "k_ovo_rank") \
    X(KID_OVO_COUNTS, "k_ovo_counts") \
    X(KID_OVO_FUSED, "k_ovo_fused") \
    X(KID_OVR_FUSED, "k_ovr_fused") \
    X(KID_FUSED_REF, "k_fused_tables") \
    X(KID_FINALIZE, "k_finalize") \
    X(KID_OVR_SCAN, "k_ovr_gene") \
    X(KID_SPARSE_SEG, "k_sparse_seg") \
    X(KID_CSC_GENE, "k_csc_gene") \
    X(KID_GENE_TOTALS, "k_gene_totals") \
    X(KID_CSC_COUNTS, "k_csc_counts") \
    X(KID_CSC_OVR, "k_csc_ovr_gene") \
    X(KID_OVR_PART, "k_ovr_partition") \
    X(KID_OVR_RANK_PARTS, "k_ovr_rank_parts") \
    X(KID_VALUE_SUMS, "k_value_sums") \
    X(KID_OVO_FUSED_WIDE, "k_ovo_fused_wide") \
    X(KID_GROUP_COMPACT, "k_group_compact") \
    X(KID_OVO_RANK_COMPACT, "k_ovo_rank_compact") \
    X(KID_OVR_COUNTS, "k_ovr_counts") \
    X(KID_GATHER_COLS, "k_gather_columns") \
    X(KID_CSR_COUNTS, "k_csr_counts") \
    X(KID_DENSIFY, "k_densify") \
    X(KID_GROUP_HISTS, "k_group_value_hists") \
    X(KID_ADJ_VALIDATE, "k_adj_validate") /* illico_adjust_pvalues (kernels_adjust.h) */ \
    X(KID_ADJ_SORT, "k_adj_sort_lds") \
    X(KID_ADJ_MERGE, "k_adj_merge") \
    X(KID_ADJ_SCAN, "k_adj_scan") \
    X(KID_ADJ_BONF, "k_adj_bonferroni") \
    X(KID_GS_VMAX, "k_gs_vmax") /* illico_group_stats_* (kernels_group_stats.h) */ \
    X(KID_GS_DENSE, "k_gs_dense") \
    X(KID_GS_CSC, "k_gs_csc") \
    X(KID_GS_CSR, "k_gs_csr") \
    X(KID_GS_TOTALS, "k_gs_totals") \
    X(KID_GS_FINALIZE, "k_gs_finalize") \
    X(KID_FINALIZE_Z, "k_finalize_z") /* k_finalize<true>: with the z-score plane */ \
    X(KID_TOP_VALIDATE, "k_top_validate") /* illico_top_by_score (kernels_adjust.h) */ \
    X(KID_TOP_SORT, "k_top_sort") \
    X(KID_TOP_MERGE, "k_top_merge") \
    X(KID_TOP_SCAN, "k_top_scan") \
    X(KID_GM_VMAX, "k_gm_vmax") /* illico_group_moments_* (kernels_group_moments.h) */ \
    X(KID_GM_DENSE, "k_gm_dense") \
    X(KID_GM_CSC, "k_gm_csc") \
    X(KID_GM_CSR, "k_gm_csr") \
    X(KID_GM_TOTALS, "k_gm_totals") \
    X(KID_GM_FINALIZE, "k_gm_finalize") \
    X(KID_TTEST, "k_ttest") /* illico_ttest_from_moments / illico_student_t_pvalues (kernels_ttest.h) */ \
    X(KID_PW_HIST_DENSE, "k_pw_hists_dense") /* illico_group_value_hists_* (kernels_pairwise.h) */ \
    X(KID_PW_HIST_CSC, "k_pw_hists_csc") \
    X(KID_PW_HIST_CSR, "k_pw_hists_csr") \
    X(KID_PW_HIST_FINISH, "k_pw_hists_finish") \
    X(KID_PW_PAIRS, "k_pw_pairs") /* illico_pairwise_from_hists */ \
    X(KID_OVO_FUSED_ST16, "k_ovo_fused_st16") /* k_ovo_fused's first pass in a 16-byte-store form ("fused_mem_policy" 8 / 12 where the planes allow it) */ \
    X(KID_PW_RANK_PAIRS, "k_pw_rank_pairs") /* illico_pairwise_ranked_* (kernels_pairwise_ranked.h) */ \
    X(KID_PW_RANK_EMIT, "k_pw_rank_emit") \
    X(KID_CSR_TILE_GATHER, "k_csr_tile_gather") /* pass 2 of the CSR -> CSC transposition (route_csr_transpose): the gather form ... */ \
    X(KID_CSR_BLOCK_SCATTER, "k_csr_block_scatter") /* ... and the scatter form; the counting pass stays under k_sparse_seg */

#define ILLICO_KERNEL_ID(id, name) id,
#define ILLICO_KERNEL_NAME(id, name) name,
enum { ILLICO_KERNELS(ILLICO_KERNEL_ID) KID_COUNT };
extern const char *const kKernelNames[KID_COUNT]; // = {ILLICO_KERNELS(ILLICO_KERNEL_NAME)}, in core.hip
