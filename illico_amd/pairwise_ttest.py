"""All-pairs Welch t-tests: every group against every other group, from one moments pass over the matrix.

``pairwise_ttest`` is scran's ``pairwiseTTests``: row ``(g, r, gene)`` of its frame is row ``(g, gene)`` of
``welch_ttest(..., reference=r)``, byte for byte.  The moments of a group do not depend on the reference: the exact per-group sums and
sums of squares are formed once per gene window (include/illico_hip.h: illico_group_moments_*), and every ordered pair follows from
them on the device (include/illico_hip_pair_ttest.h: illico_pair_ttest_from_moments) -- Welch's form with one evaluation of Student's t
tail per unordered pair.  ``pairwise_markers(..., method="t-test")`` (pairwise.py) hands the same blocks to ``Engine.combine_pairs``.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from illico_amd import _lib
from illico_amd import pairwise as pairwise_mod
from illico_amd._passes import (HostPlanes, _input, _select, check_alternative, check_bool, check_corr_method, check_max_result_bytes,
                                check_variant, device_handler, pair_frame, walk)
from illico_amd.utils.groups import encode_and_count_groups

__all__ = ["pairwise_ttest"]

#: the planes of the frame, and of the marker frame (p first, then the four effect planes of ``combine_pairs``)
FRAME_PLANES = ("p", "t", "fold_change")
MARKER_PLANES = ("p", "t", "fold_change", "df", "cohen_d")


def pair_ttest_blocks(X, handler, group_container, sel: np.ndarray, is_log1p: bool, variant: str, alternative: str, want, sink) -> None:
    """The planes ``want`` (names of ``_lib.PAIR_TT_OUTPUTS``) of the groups ``sel``, block of columns by block: ``sink(cols, planes,
    None)`` receives the int64 gene numbers of a block's w columns and its float64 CUDA tensors ``[K, K, w]`` indexed ``[r, g, gene]``,
    the contract of ``pairwise_planes``' sink.  Per chunk of the handler and per gene window -- sized so that the moments and the planes
    stay under ``pairwise.PAIR_WINDOW_BYTES``, halved when the engine's scratch budget refuses it -- one ``group_moments``, one
    ``group_stats(is_log1p=True)`` under ``is_log1p``, one pair call."""
    import torch
    eng = _lib.get_engine()
    dev = torch.device("cuda", eng.device)
    handler = device_handler(X, handler)  # an in-RAM CSR matrix goes up once
    eng.set_groups(group_container._replace(encoded_ref_group=-1))  # the moments pass uses codes, counts and order only
    G, K = int(np.asarray(group_container.counts).size), int(sel.size)
    per_gene = (3 if is_log1p else 2) * G * 8 + len(want) * K * K * 8

    def window(chunk, o0, o1):
        w = o1 - o0
        mom = tuple(torch.empty((G, w), dtype=torch.float64, device=dev) for _ in range(2))
        fsum = torch.empty((G, w), dtype=torch.float64, device=dev) if is_log1p else None
        chunk.group_moments(eng, o0, o1, out=mom)
        if is_log1p:
            chunk.group_stats(eng, o0, o1, is_log1p=True, out=(None, fsum))
        got = eng.pair_ttest_from_moments(*mom, sel=sel, fsum=fsum, variant=variant, alternative=alternative, want=want)
        sink(np.arange(chunk.lb + o0, chunk.lb + o1, dtype=np.int64), tuple(got), None)

    walk(X, handler, per_gene, pairwise_mod.PAIR_WINDOW_BYTES, window)


def pairwise_ttest(adata, is_log1p: bool, group_keys: str, *, groups=None, variant: str = "welch", alternative: str = "two-sided",
                   layer: str | None = None, corr_method: str | None = None, max_result_bytes: int = 8 << 30) -> pd.DataFrame:
    """Welch's t-test of every group against every other group, on one MI355X (scran's ``pairwiseTTests``).

    ``adata``, ``is_log1p``, ``group_keys``, ``variant``, ``alternative`` and ``layer`` as in ``welch_ttest``; every container it
    accepts is accepted, backed containers are streamed chunk by chunk, an in-RAM CSR matrix is uploaded once.  ``groups``: a sequence
    of labels that restricts both sides of the comparison (default: all groups); whatever its order, groups appear in the order
    ``welch_ttest`` gives them.

    Returns a DataFrame with MultiIndex ``(pert, reference, feature)`` -- reference-major, then pert, then gene, as
    ``pairwise_wilcoxon``; a group is not compared with itself -- and float64 columns ``p_value``, ``statistic`` (t) and
    ``fold_change``; ``p_value_adj`` with ``corr_method`` (``"benjamini-hochberg"`` / ``"bh"``, ``"benjamini-yekutieli"`` / ``"by"``,
    ``"bonferroni"``): each (pert, reference) pair adjusted across its genes.  Row ``(g, r, gene)`` is row ``(g, gene)`` of
    ``welch_ttest(..., reference=r)``, byte for byte.  The matrix is read by one moments pass (and one ``group_stats`` pass under
    ``is_log1p``), whatever the number of groups.

    ``ValueError``: a label of ``groups`` that is not present or named twice, fewer than two groups, a bad ``variant`` or
    ``alternative``, a non-bool ``is_log1p``, and a result of more than ``max_result_bytes`` bytes (K (K - 1) x genes x 8 bytes x
    columns), raised before any device work.  ``NotImplementedError``: a group of more than 2097151 cells."""
    check_bool("is_log1p", is_log1p)
    check_variant(variant)
    check_alternative(alternative)
    check_max_result_bytes(max_result_bytes)
    code = check_corr_method(corr_method, optional=True)
    X = _input(adata, layer)
    unique_raw_groups, group_container = encode_and_count_groups(groups=adata.obs[group_keys], ref_group=None)
    sel = _select(np.asarray(unique_raw_groups), groups)

    def compute():
        from illico_amd.utils.registry import data_handler_registry
        to_host = HostPlanes(len(FRAME_PLANES), int(sel.size), int(X.shape[1]))
        pair_ttest_blocks(X, data_handler_registry.get(X), group_container, sel, bool(is_log1p), variant, alternative, FRAME_PLANES, to_host)
        return to_host.planes, {}

    return pair_frame(("p_value", "statistic", "fold_change"), np.asarray(unique_raw_groups)[sel], np.asarray(adata.var_names), code,
                      max_result_bytes, compute)
