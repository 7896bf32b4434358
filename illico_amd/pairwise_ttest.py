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

from illico_amd import pairwise as pairwise_mod
from illico_amd.pairwise import _pair_index, _select, _windows
from illico_amd.ttest import ALTERNATIVES, VARIANTS
from illico_amd.utils.groups import encode_and_count_groups

__all__ = ["pairwise_ttest"]

#: the planes of the frame, and of the marker frame (p first, then the four effect planes of ``combine_pairs``)
FRAME_PLANES = ("p", "t", "fold_change")
MARKER_PLANES = ("p", "t", "fold_change", "df", "cohen_d")


def _check_arguments(is_log1p, variant, alternative, corr_method, max_result_bytes):
    if not isinstance(is_log1p, (bool, np.bool_)):
        raise ValueError(f"is_log1p must be a bool, got {is_log1p!r}")
    if not isinstance(variant, str) or variant not in VARIANTS:
        raise ValueError(f"variant must be one of {VARIANTS}, got {variant!r}")
    if not isinstance(alternative, str) or alternative not in ALTERNATIVES:
        raise ValueError(f"Unsupported alternative hypothesis: {alternative}")
    if isinstance(max_result_bytes, bool) or not isinstance(max_result_bytes, (int, np.integer)) or max_result_bytes < 0:
        raise ValueError(f"max_result_bytes must be a non-negative integer, got {max_result_bytes!r}")
    if corr_method is None:
        return None
    from illico_amd.adjust import _method
    return _method(corr_method)


def pair_ttest_blocks(X, handler, group_container, sel: np.ndarray, is_log1p: bool, variant: str, alternative: str, want, sink) -> None:
    """The planes ``want`` (names of ``_lib.PAIR_TT_OUTPUTS``) of the groups ``sel``, block of columns by block: ``sink(cols, planes,
    None)`` receives the int64 gene numbers of a block's w columns and its float64 CUDA tensors ``[K, K, w]`` indexed ``[r, g, gene]``,
    the contract of ``pairwise_planes``' sink.  Per chunk of the handler and per gene window -- sized so that the moments and the planes
    stay under ``pairwise.PAIR_WINDOW_BYTES``, halved when the engine's scratch budget refuses it -- one ``group_moments``, one
    ``group_stats(is_log1p=True)`` under ``is_log1p``, one pair call."""
    import torch
    from illico_amd import _lib
    from illico_amd.group_stats import _chunks
    from illico_amd.ttest import device_handler
    eng = _lib.get_engine()
    dev = torch.device("cuda", eng.device)
    handler = device_handler(X, handler)  # an in-RAM CSR matrix goes up once
    eng.set_groups(group_container._replace(encoded_ref_group=-1))  # the moments pass uses codes, counts and order only
    G, K = int(np.asarray(group_container.counts).size), int(sel.size)
    per_gene = (3 if is_log1p else 2) * G * 8 + len(want) * K * K * 8
    width = max(64, (pairwise_mod.PAIR_WINDOW_BYTES // per_gene) // 64 * 64)
    for lb, ub in _chunks(X, handler):
        fetched, (a, b) = handler.fetch(lb, ub)
        Xc = handler.to_nb(fetched)
        sparse_in = hasattr(Xc, "indptr")
        fmt = ("csr" if handler.fmt.name == "CSR" else "csc") if sparse_in else None
        todo = _windows(0, ub - lb, width)
        while todo:
            o0, o1 = todo.pop(0)
            w = o1 - o0
            try:
                mom = tuple(torch.empty((G, w), dtype=torch.float64, device=dev) for _ in range(2))
                fsum = torch.empty((G, w), dtype=torch.float64, device=dev) if is_log1p else None
                if sparse_in:
                    eng.group_moments_sparse(fmt, Xc.data, Xc.indices, Xc.indptr, Xc.shape, a + o0, a + o1, out=mom)
                    if is_log1p:
                        eng.group_stats_sparse(fmt, Xc.data, Xc.indices, Xc.indptr, Xc.shape, a + o0, a + o1, is_log1p=True, out=(None, fsum))
                else:
                    eng.group_moments(Xc, a + o0, a + o1, out=mom)
                    if is_log1p:
                        eng.group_stats(Xc, a + o0, a + o1, is_log1p=True, out=(None, fsum))
                got = eng.pair_ttest_from_moments(*mom, sel=sel, fsum=fsum, variant=variant, alternative=alternative, want=want)
            except (MemoryError, torch.cuda.OutOfMemoryError):
                if w <= 64:
                    raise
                half = max(64, (w // 2 + 63) // 64 * 64)
                todo = _windows(o0, o1, half) + todo
                mom = fsum = None
                continue
            sink(np.arange(lb + o0, lb + o1, dtype=np.int64), tuple(got), None)


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
    code = _check_arguments(is_log1p, variant, alternative, corr_method, max_result_bytes)
    from illico_amd.group_stats import _input
    X = _input(adata, layer)
    unique_raw_groups, group_container = encode_and_count_groups(groups=adata.obs[group_keys], ref_group=None)
    sel = _select(np.asarray(unique_raw_groups), groups)
    K, M = int(sel.size), int(X.shape[1])
    n_cols = 3 + int(code is not None)
    need = K * (K - 1) * M * 8 * n_cols
    if need > max_result_bytes:
        raise ValueError(f"the result of {K} x {K - 1} pairs over {M} genes with {n_cols} columns takes {need} bytes, more than "
                         f"max_result_bytes = {int(max_result_bytes)}: restrict `groups`, or raise max_result_bytes")
    from illico_amd.utils.registry import data_handler_registry
    handler = data_handler_registry.get(X)
    planes = np.empty((len(FRAME_PLANES), K, K, M), dtype=np.float64)

    def to_host(cols, block, skip):
        for k, q in enumerate(block):
            planes[k][:, :, cols] = q.cpu().numpy()

    pair_ttest_blocks(X, handler, group_container, sel, bool(is_log1p), variant, alternative, FRAME_PLANES, to_host)
    r_idx, g_idx = np.divmod(np.arange(K * K), K)
    rows = np.flatnonzero(r_idx != g_idx)
    cols = {name: planes[k].reshape(K * K, M)[rows].reshape(-1) for k, name in enumerate(("p_value", "statistic", "fold_change"))}
    if code is not None:
        from illico_amd import _lib
        adj = _lib.get_engine().adjust_pvalues(np.ascontiguousarray(planes[0].reshape(K * K, M)[rows]), code)
        cols["p_value_adj"] = np.asarray(adj).reshape(-1)
    labels = np.asarray(unique_raw_groups)[sel]
    index = _pair_index(labels, np.asarray(adata.var_names), r_idx[rows], g_idx[rows])
    return pd.DataFrame(cols, index=index, copy=False)
