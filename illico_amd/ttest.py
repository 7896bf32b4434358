"""Welch's unequal-variance t-test per (group, gene) -- scanpy's ``rank_genes_groups(method="t-test")`` and ``"t-test_overestim_var"``.

``welch_ttest`` returns the ``(pert, feature)`` frame of ``asymptotic_wilcoxon`` with ``p_value``, ``statistic`` (t) and
``fold_change``.  The test runs on the values as given (the log values of a log1p matrix).  Each group's exact sum and sum of squares
-- and, one-versus-rest, the same over every other cell -- are formed on the device in one pass over the matrix
(include/illico_hip.h: illico_group_moments_*); t, the Welch-Satterthwaite degrees of freedom and Student's t tail follow on the
device from those planes (illico_ttest_from_moments).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from illico_amd import _lib
from illico_amd._passes import VARIANTS, _input, _product_index, check_alternative, check_bool, check_variant, chunks, device_handler
from illico_amd.utils.groups import encode_and_count_groups
from illico_amd.utils.registry import data_handler_registry

__all__ = ["welch_ttest", "VARIANTS"]


def _check_arguments(is_log1p, variant, alternative):
    check_bool("is_log1p", is_log1p)
    check_variant(variant)
    check_alternative(alternative)


def fold_change_planes(sum_g: np.ndarray, sum_ref: np.ndarray, counts: np.ndarray, n_cells: int, ref: int) -> np.ndarray:
    """``fold_change`` as ``asymptotic_wilcoxon`` forms it: (sum_g / n_g) / (reference sum / reference size), inf where the reference's
    mean is 0.  ``sum_ref``: the rest sums [G, M] (one-versus-rest) or the reference group's row [M]."""
    n_g = counts.astype(np.float64)[:, None]
    n_ref = (float(n_cells) - n_g) if ref < 0 else float(counts[ref])
    with np.errstate(divide="ignore", invalid="ignore"):
        mu_ref = sum_ref / n_ref
        fc = (sum_g / n_g) / mu_ref
    return np.where(np.broadcast_to(mu_ref == 0.0, fc.shape), np.inf, fc)


def ttest_planes(X, handler, group_container, is_log1p: bool, variant: str, alternative: str) -> np.ndarray:
    """float64 [3, G, n_genes]: p_value, t, fold_change for the groups of ``group_container`` (engine groups are set here).  The matrix
    is read by the moments pass alone, plus one ``group_stats`` pass for the expm1 sums of the fold change under ``is_log1p``."""
    import torch
    eng = _lib.get_engine()
    eng.set_groups(group_container)
    counts = np.asarray(group_container.counts, dtype=np.int64)
    G, M, N = int(counts.size), int(X.shape[1]), int(X.shape[0])
    ref = int(group_container.encoded_ref_group)
    ovr = ref < 0
    planes = np.empty((3, G, M), dtype=np.float64)
    dev = torch.device("cuda", eng.device)
    for chunk in chunks(X, handler):
        w, lb, ub = chunk.width, chunk.lb, chunk.lb + chunk.width
        mom = tuple(torch.empty((G, w), dtype=torch.float64, device=dev) for _ in range(4 if ovr else 2))
        fsum = tuple(np.empty((G, w), dtype=np.float64) for _ in range(2 if ovr else 1)) if is_log1p else None
        chunk.group_moments(eng, 0, w, rest=ovr, out=mom)
        if is_log1p:
            chunk.group_stats(eng, 0, w, is_log1p=True, rest=ovr, out=(None, fsum[0]) + ((None, fsum[1]) if ovr else ()))
        p, t = eng.ttest_from_moments(*mom, variant=variant, alternative=alternative, want=("p", "t"))
        planes[0][:, lb:ub] = p.cpu().numpy()
        planes[1][:, lb:ub] = t.cpu().numpy()
        if is_log1p:
            s_g, s_ref = fsum[0], (fsum[1] if ovr else fsum[0][ref])
        else:
            s_g = mom[0].cpu().numpy()
            s_ref = mom[2].cpu().numpy() if ovr else s_g[ref]
        planes[2][:, lb:ub] = fold_change_planes(s_g, s_ref, counts, N, ref)
    return planes


def _ttest_frame_inputs(adata, is_log1p, group_keys, reference, variant, alternative, layer):
    """(planes [3, G, M], index, (X, handler, GroupContainer)) of one t-test call."""
    X = _input(adata, layer)
    handler = device_handler(X, data_handler_registry.get(X))
    unique_raw_groups, group_container = encode_and_count_groups(groups=adata.obs[group_keys], ref_group=reference)
    planes = ttest_planes(X, handler, group_container, bool(is_log1p), variant, alternative)
    index = _product_index(pd.Series(unique_raw_groups, name="pert", dtype=str), pd.Series(np.asarray(adata.var_names), name="feature", dtype=str))
    return planes, index, (X, handler, group_container)


def welch_ttest(adata, is_log1p: bool, group_keys: str, reference: str | None = None, *, variant: str = "welch",
                alternative: str = "two-sided", layer: str | None = None) -> pd.DataFrame:
    """Welch's t-test per (group, gene) on one MI355X.

    ``adata``, ``group_keys``, ``reference`` and ``layer`` as in ``asymptotic_wilcoxon`` (``reference=None``: one-versus-rest); every
    container it accepts is accepted, streamed (backed) containers are read gene chunk by gene chunk.  ``variant``: ``"welch"``
    (scanpy's ``"t-test"``; ``scipy.stats.ttest_ind(group, reference, equal_var=False)``) or ``"overestim_var"`` (scanpy's
    ``"t-test_overestim_var"``: the reference's variance is divided by the group's size).  ``alternative``: ``"two-sided"``,
    ``"greater"`` (the group's mean is larger) or ``"less"``.

    Returns the DataFrame of ``asymptotic_wilcoxon`` -- MultiIndex ``(pert, feature)``, group-major rows -- with float64 columns
    ``p_value``, ``statistic`` (t) and ``fold_change`` (formed as ``asymptotic_wilcoxon`` forms it: from the values, or from
    ``expm1`` of them under ``is_log1p``).  The test itself always runs on the values as given.  A test without variance on either
    side and equal means, or with a one-cell side, gives (t, p) = (0, 1), as scanpy does; the reference group's row of a
    one-versus-one call is (0, 1) too.  Groups of more than 2097151 cells raise ``NotImplementedError``.
    """
    _check_arguments(is_log1p, variant, alternative)
    planes, index, _ = _ttest_frame_inputs(adata, is_log1p, group_keys, reference, variant, alternative, layer)
    from illico_amd.asymptotic_wilcoxon import _planes_frame
    return _planes_frame(planes, index)
