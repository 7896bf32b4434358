"""Multiple-testing correction and top-gene ranking of the engine's p-value planes, on the device.

``adjust_pvalues`` corrects a ``[G, M]`` plane of p-values within each row (group) -- Benjamini-Hochberg as scipy's
``stats.false_discovery_control(p, axis=1)`` computes it, Benjamini-Yekutieli, Bonferroni -- and optionally returns each row's
``n_top`` columns by ascending p.  ``differential_expression`` is ``asymptotic_wilcoxon`` followed by that step: the same
DataFrame plus a ``p_value_adj`` column, optionally cut to each group's top genes.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from illico_amd import _lib
from illico_amd._passes import METHODS, _method, adjust_and_cut, check_bool, check_corr_method, check_n_genes, cut_rows  # noqa: F401
from illico_amd.asymptotic_wilcoxon import _planes_frame, _wilcoxon_planes

__all__ = ["adjust_pvalues", "differential_expression", "top_by_score"]

#: what ``differential_expression`` can order each group's rows by for its ``n_genes`` cut
RANK_BY = ("p_value", "z_score")
#: ... with a t-test method: the statistic column (t) is the score
RANK_BY_TTEST = ("p_value", "statistic")
#: the tests ``differential_expression`` runs (scanpy's names) -> the variant of ``welch_ttest``, None for the Wilcoxon engine
DE_METHODS = {"wilcoxon": None, "t-test": "welch", "t-test_overestim_var": "overestim_var"}

def adjust_pvalues(p, method: str = "benjamini-hochberg", *, n_top: int = 0):
    """Adjust each row of a p-value plane for multiple testing.

    ``p``: float64 ``[G, M]`` numpy array or CUDA tensor with unit column stride (a view of a wider plane is fine), every value in
    [0, 1].  ``method``: ``"bh"`` / ``"benjamini-hochberg"``, ``"by"`` / ``"benjamini-yekutieli"`` or ``"bonferroni"``.  The result
    lives where ``p`` lives: ``adj`` float64 ``[G, M]``, or ``(adj, top)`` with ``top`` int64 ``[G, n_top]`` -- each row's first
    ``n_top`` columns sorted by ascending p, ties by column (``np.argsort(p + 0.0, axis=1, kind="stable")[:, :n_top]``) -- when
    ``n_top > 0``.  Raises ``ValueError`` for a NaN or a value outside [0, 1], naming its position, as scipy does.
    """
    code = _method(method)
    _check_plane(p)
    _lib._adjust_n_top(n_top, int(p.shape[1]))
    device = p.device.index if _lib._is_torch_tensor(p) else None
    return _lib.get_engine(device).adjust_pvalues(p, code, n_top=n_top)


def top_by_score(z, n_top: int):
    """Each row's first ``n_top`` columns by descending score, ties by column: ``np.argsort(-(z + 0.0), axis=1, kind="stable")[:, :n_top]``.

    ``z``: float64 ``[G, M]`` numpy array or CUDA tensor with unit column stride -- a z-score plane (``Engine.run_dense(scores=True)``).
    Returns int64 ``[G, n_top]`` where ``z`` lives.  ``-0.0`` and ``+0.0`` tie, ``+inf`` comes first, ``-inf`` last; a NaN raises
    ``ValueError`` naming its position."""
    _check_plane(z, "z")
    n_top = _lib._adjust_n_top(n_top, int(z.shape[1]))
    device = z.device.index if _lib._is_torch_tensor(z) else None
    return _lib.get_engine(device).top_by_score(z, n_top)


def _check_plane(p, what="p"):
    """The dtype / rank / residency checks of Engine.adjust_pvalues, before any engine exists."""
    if _lib._is_torch_tensor(p):
        import torch
        if not p.is_cuda:
            raise ValueError(f"{what} must be a numpy array or a CUDA tensor (got a CPU tensor)")
        if p.dtype != torch.float64 or p.dim() != 2:
            raise ValueError(f"{what} must be a float64 2-D tensor, got {p.dtype} with {p.dim()} dimensions")
    elif not isinstance(p, np.ndarray):
        raise ValueError(f"{what} must be a numpy array or a CUDA tensor, got {type(p).__name__}")
    elif p.dtype != np.float64 or p.ndim != 2:
        raise ValueError(f"{what} must be a float64 2-D array, got {p.dtype} with {p.ndim} dimensions")


def differential_expression(adata, is_log1p: bool, group_keys: str, reference: str | None = None, *,
                            corr_method: str = "benjamini-hochberg", n_genes: int | None = None, pts: bool = False,
                            scores: bool = False, rank_by: str = "p_value", method: str = "wilcoxon", **kw) -> pd.DataFrame:
    """``asymptotic_wilcoxon`` plus the multiple-testing correction that follows it in a DE workflow.

    ``kw`` takes the other arguments of ``asymptotic_wilcoxon`` (``batch_size``, ``alternative``, ``layer``, ...).  Returns its
    DataFrame -- the same ``p_value``, ``statistic`` and ``fold_change`` -- plus a float64 ``p_value_adj`` column: ``corr_method``
    applied within each group across all genes of the call.  With ``n_genes``, each group keeps only its ``n_genes`` rows of smallest
    p (ties by gene order), in that order; the groups keep their order.  The reference group's row of a one-versus-one call stays,
    as ``asymptotic_wilcoxon`` keeps it (its p are 1.0, so are their adjusted values).  ``pts=True`` adds the four columns of
    ``group_statistics`` (``pct_group``, ``pct_reference``, ``mean_group``, ``mean_reference``) before the ``n_genes`` cut, so they
    stay on their rows; an in-RAM CSR matrix is uploaded once for both passes.  ``scores=True`` adds a float64 ``z_score`` column: the
    test's z, positive when the group ranks above its reference (scanpy's ``scores``; include/illico_hip.h: illico_run_dense_ex).
    ``rank_by="z_score"`` orders each group's rows by descending z for the ``n_genes`` cut -- scanpy's order, and the one that still
    separates genes whose p has underflowed to 0 -- and implies ``scores=True``; ``rank_by="p_value"`` (the default) orders by p.

    ``method``: ``"wilcoxon"`` (the default: everything above), ``"t-test"`` or ``"t-test_overestim_var"`` -- scanpy's names for Welch's
    t-test and its variant (``illico_amd.welch_ttest``).  With a t-test ``p_value``, ``statistic`` (t) and ``fold_change`` are
    ``welch_ttest``'s; ``p_value_adj``, ``n_genes`` and ``pts`` work as above; ``rank_by="statistic"`` orders each group's rows by
    descending t (valid with a t-test only).  The statistic column is the score, so ``scores=True`` and ``rank_by="z_score"`` raise
    ``ValueError``; ``use_continuity`` / ``tie_correct`` mean nothing to a t-test and raise ``TypeError``; ``n_threads``,
    ``batch_size`` and ``precompile`` are accepted and ignored.
    """
    code = check_corr_method(corr_method)
    if not isinstance(method, str) or method not in DE_METHODS:
        raise ValueError(f"method must be one of {tuple(DE_METHODS)}, got {method!r}")
    variant = DE_METHODS[method]
    check_bool("pts", pts)
    check_bool("scores", scores)
    if variant is not None and scores:
        raise ValueError("scores=True belongs to method='wilcoxon': a t-test's statistic column is its score")
    ranks, where = (RANK_BY, "") if variant is None else (RANK_BY_TTEST, " with a t-test method")
    if not isinstance(rank_by, str) or rank_by not in ranks:
        raise ValueError(f"rank_by must be one of {ranks}{where}, got {rank_by!r}")
    check_n_genes(n_genes)
    wilcoxon_only = {"use_continuity", "tie_correct"}
    if variant is not None and set(kw) & wilcoxon_only:
        raise TypeError(f"differential_expression(method='t-test...') got Wilcoxon-only keyword arguments {sorted(set(kw) & wilcoxon_only)}")
    unknown = set(kw) - {"n_threads", "batch_size", "alternative", "layer", "precompile"} - wilcoxon_only
    if unknown:
        raise TypeError(f"differential_expression() got unexpected keyword arguments {sorted(unknown)}")
    by_score = rank_by != "p_value"
    if variant is None:
        scores = bool(scores) or by_score
        args = dict(n_threads=1, batch_size="auto", alternative="two-sided", use_continuity=True, tie_correct=True, layer=None)
        args.update({k: v for k, v in kw.items() if k != "precompile"})
        inputs: list = []
        planes, index = _wilcoxon_planes(adata, is_log1p, group_keys, reference, **args, inputs=inputs, scores=scores)
        score, extra = planes[3] if by_score else None, {"z_score": planes[3]} if scores else {}
        planes, inputs = planes[:3], inputs[0] if pts else None
    else:
        from illico_amd import ttest
        alternative, layer = kw.get("alternative", "two-sided"), kw.get("layer")
        ttest._check_arguments(is_log1p, variant, alternative)
        planes, index, inputs = ttest._ttest_frame_inputs(adata, is_log1p, group_keys, reference, variant, alternative, layer)
        score, extra = planes[1] if by_score else None, {}
    adj, top = adjust_and_cut(planes[0], code, n_genes, score)
    if pts:
        from illico_amd.group_stats import stat_planes
        X, handler, group_container = inputs
        extra.update(stat_planes(X, handler, group_container, bool(is_log1p)))
    df = _planes_frame(planes, index, p_value_adj=adj, **extra)
    return df if top is None else cut_rows(df, top, planes.shape[2])
