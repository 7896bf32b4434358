"""illico_amd -- MI355X-native engine for illico's asymptotic Wilcoxon rank-sum hot path.

``from illico_amd import asymptotic_wilcoxon`` is a drop-in for ``illico.asymptotic_wilcoxon``; ``adjust_pvalues`` and
``differential_expression`` add the per-group multiple-testing correction and top-gene ranking that follow it; ``top_by_score``
ranks a z-score plane; ``welch_ttest`` is Welch's t-test in the same frame; ``pairwise_wilcoxon`` compares every group with every
other group from one pass over the matrix, ``pairwise_ttest`` does so with Welch's t-test; ``pairwise_markers`` combines the tests of
either into one row per (group, gene);
``blocked_wilcoxon`` tests each group against the reference cells of the same block (batch, donor, plate) and combines the blocks.
"""
from illico_amd.anndata_lite import AnnDataLite
from illico_amd.adjust import adjust_pvalues, differential_expression, top_by_score
from illico_amd.asymptotic_wilcoxon import asymptotic_wilcoxon
from illico_amd.blocked import blocked_wilcoxon
from illico_amd.group_stats import group_statistics
from illico_amd.pairwise import pairwise_markers, pairwise_wilcoxon
from illico_amd.pairwise_ttest import pairwise_ttest
from illico_amd.ttest import welch_ttest

__all__ = ["asymptotic_wilcoxon", "AnnDataLite", "adjust_pvalues", "blocked_wilcoxon", "differential_expression", "group_statistics", "pairwise_markers",
           "pairwise_ttest", "pairwise_wilcoxon", "top_by_score", "welch_ttest"]
__version__ = "0.1.0"
