"""Per-group expression fractions and mean expression -- the ``pts`` / ``pct.1`` / ``pct.2`` and mean columns of a marker-gene table.

``group_statistics`` returns, for every (group, gene) row of ``asymptotic_wilcoxon`` (same index, same order), the fraction of the
group's cells that express the gene (value != 0), the same fraction over the reference, and both mean values.  The reference is the
reference group in one-versus-one, every other cell in one-versus-rest.  Under ``is_log1p`` the means are means of ``expm1(x)``, so
that ``mean_group / mean_reference`` is the fold change of ``asymptotic_wilcoxon`` (one-versus-one).  The counts and exact sums are
formed on the device (include/illico_hip.h: illico_group_stats_*).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from illico_amd import _lib
from illico_amd._passes import _input, _product_index, check_bool, chunks
from illico_amd.utils.groups import encode_and_count_groups
from illico_amd.utils.registry import data_handler_registry

__all__ = ["group_statistics"]

#: the columns group_statistics adds, in order
STAT_COLUMNS = ("pct_group", "pct_reference", "mean_group", "mean_reference")


def stat_planes(X, handler, group_container, is_log1p: bool) -> dict[str, np.ndarray]:
    """The four float64 [G, n_genes] planes of STAT_COLUMNS for the groups of ``group_container`` (engine groups are set here)."""
    eng = _lib.get_engine()
    eng.set_groups(group_container)
    counts = np.asarray(group_container.counts, dtype=np.int64)
    G, M, N = int(counts.size), int(X.shape[1]), int(X.shape[0])
    ref = int(group_container.encoded_ref_group)
    ovr = ref < 0
    nnz = np.zeros((2 if ovr else 1, G, M), dtype=np.int64)
    sums = np.zeros((2 if ovr else 1, G, M), dtype=np.float64)
    for chunk in chunks(X, handler):
        lb, ub = chunk.lb, chunk.lb + chunk.width
        out = (nnz[0][:, lb:ub], sums[0][:, lb:ub]) + ((nnz[1][:, lb:ub], sums[1][:, lb:ub]) if ovr else ())
        chunk.group_stats(eng, 0, chunk.width, is_log1p=is_log1p, rest=ovr, out=out)
    n_grp = counts.astype(np.float64)[:, None]
    n_ref = (N - n_grp) if ovr else np.full_like(n_grp, float(counts[ref]))
    with np.errstate(divide="ignore", invalid="ignore"):
        planes = {"pct_group": nnz[0] / n_grp, "mean_group": sums[0] / n_grp}
        if ovr:
            planes["pct_reference"] = nnz[1] / n_ref
            planes["mean_reference"] = sums[1] / n_ref
        else:
            planes["pct_reference"] = np.broadcast_to(nnz[0][ref] / n_ref[0, 0], (G, M)).copy()
            planes["mean_reference"] = np.broadcast_to(sums[0][ref] / n_ref[0, 0], (G, M)).copy()
    return {k: planes[k] for k in STAT_COLUMNS}


def group_statistics(adata, group_keys: str, reference: str | None = None, *, is_log1p: bool, layer: str | None = None) -> pd.DataFrame:
    """Expression fraction and mean per (group, gene), on the device.

    Returns a DataFrame with the ``(pert, feature)`` index and row order of ``asymptotic_wilcoxon`` and float64 columns
    ``pct_group`` (fraction of the group's cells whose value is non-zero), ``pct_reference`` (the same over the reference),
    ``mean_group`` and ``mean_reference`` (mean value; of ``expm1(x)`` under ``is_log1p``).  ``reference=None``: one-versus-rest,
    the reference of a group is every other cell (NaN when there is none: a single group).  Accepts every container
    ``asymptotic_wilcoxon`` accepts; streamed (backed) containers are read gene chunk by gene chunk.  Sparse input counts stored
    non-zero entries (a duplicate entry counts once per entry).
    """
    check_bool("is_log1p", is_log1p)
    X = _input(adata, layer)
    handler = data_handler_registry.get(X)
    unique_raw_groups, group_container = encode_and_count_groups(groups=adata.obs[group_keys], ref_group=reference)
    planes = stat_planes(X, handler, group_container, bool(is_log1p))
    index = _product_index(pd.Series(unique_raw_groups, name="pert", dtype=str), pd.Series(np.asarray(adata.var_names), name="feature", dtype=str))
    return pd.DataFrame({k: v.reshape(-1) for k, v in planes.items()}, index=index, copy=False)
