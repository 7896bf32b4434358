"""What the Python front ends share (pairwise.py, pairwise_ttest.py, blocked.py, ttest.py, group_stats.py, adjust.py): the argument
checks, the matrix hand-off to the engine (``Matrix``), the walk over gene chunks and windows with its halving rule (``chunks``,
``walk_windows``, ``walk``), the collector of flagged genes (``FlaggedGenes``) and the tails of the frames (``pair_frame``,
``adjust_and_cut``, ``cut_rows``).  The front ends import from here and not from each other; this module rests on ``_lib``, ``utils`` and
``asymptotic_wilcoxon`` alone.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
from scipy import sparse

from illico_amd import _lib
from illico_amd.asymptotic_wilcoxon import _product_index  # noqa: F401  (the (pert, feature) index of the front ends' frames)

ALTERNATIVES = ("two-sided", "less", "greater")
#: the variants of the t-tests: Welch's, and scanpy's "overestim_var" (the reference's variance is divided by the GROUP's size)
VARIANTS = ("welch", "overestim_var")
#: correction method names -> the engine's codes (include/illico_hip.h: ILLICO_ADJ_*)
METHODS = {"bh": "bh", "benjamini-hochberg": "bh", "by": "by", "benjamini-yekutieli": "by", "bonferroni": "bonferroni"}


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def check_bool(name: str, v) -> None:
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be a bool, got {v!r}")


def check_alternative(alternative) -> None:
    if not isinstance(alternative, str) or alternative not in ALTERNATIVES:
        raise ValueError(f"Unsupported alternative hypothesis: {alternative}")


def check_variant(variant) -> None:
    if not isinstance(variant, str) or variant not in VARIANTS:
        raise ValueError(f"variant must be one of {VARIANTS}, got {variant!r}")


def check_n_genes(n_genes) -> None:
    if n_genes is not None and (isinstance(n_genes, bool) or not isinstance(n_genes, (int, np.integer)) or n_genes < 1):
        raise ValueError(f"n_genes must be a positive integer or None, got {n_genes!r}")


def check_max_result_bytes(max_result_bytes) -> None:
    if isinstance(max_result_bytes, bool) or not isinstance(max_result_bytes, (int, np.integer)) or max_result_bytes < 0:
        raise ValueError(f"max_result_bytes must be a non-negative integer, got {max_result_bytes!r}")


def _method(name) -> str:
    try:
        return METHODS[name.lower()]
    except (KeyError, AttributeError):
        raise ValueError(f"Unknown p-value correction method {name!r}: one of {sorted(METHODS)}") from None


def check_corr_method(corr_method, optional: bool = False):
    """The engine's code of ``corr_method``; with ``optional``, None stands for no correction and gives None."""
    return None if optional and corr_method is None else _method(corr_method)


def _select(unique_groups: np.ndarray, groups) -> np.ndarray:
    """The selected group ids, ascending: all of them, or those of the labels in ``groups``."""
    G = int(len(unique_groups))
    if groups is None:
        sel = np.arange(G, dtype=np.int64)
    else:
        if isinstance(groups, (str, bytes)):
            raise ValueError(f"groups must be a sequence of labels, got the single label {groups!r}")
        labels = [str(x) for x in groups]
        known = {str(x): k for k, x in enumerate(unique_groups)}
        unknown = [x for x in labels if x not in known]
        if unknown:
            raise ValueError(f"groups names labels that are not present: {unknown}")
        if len(set(labels)) != len(labels):
            raise ValueError(f"groups names a label twice: {labels}")
        sel = np.array(sorted(known[x] for x in labels), dtype=np.int64)
    if sel.size < 2:
        raise ValueError(f"pairwise tests need at least two groups, got {sel.size}")
    return sel


# ---- the input ------------------------------------------------------------------------------------------------------------------------
def _input(adata, layer):
    X = adata.layers[layer] if layer is not None else adata.X
    if len(getattr(X, "shape", ())) != 2:
        raise ValueError(f"the expression matrix must be 2-D, got shape {getattr(X, 'shape', None)}")
    return X


def _is_ram_csr(X) -> bool:
    return isinstance(X, sparse.csr_matrix) or (hasattr(sparse, "csr_array") and isinstance(X, sparse.csr_array))


def device_handler(X, handler):
    """The handler the passes of one call read: an in-RAM CSR matrix goes up once (every pass walks all of its rows)."""
    if _is_ram_csr(X):
        from illico_amd.asymptotic_wilcoxon import _csr_to_device
        return _csr_to_device(X, handler, check=False)[1]
    return handler


def _chunks(X, handler) -> list[tuple[int, int]]:
    """The gene ranges of one call: the whole range in RAM, chunks of about STREAM_CHUNK_BYTES for streamed containers."""
    from illico_amd.asymptotic_wilcoxon import STREAM_CHUNK_BYTES
    n_genes = int(X.shape[1])
    if not getattr(handler, "streams", False) or n_genes == 0:
        return [(0, n_genes)] if n_genes else []
    per_gene = max(1, int(X.shape[0]) * getattr(getattr(X, "dtype", None), "itemsize", 4))
    w = int(max(1, min(n_genes, STREAM_CHUNK_BYTES // per_gene)))
    b = list(range(0, n_genes, w)) + [n_genes]
    return list(zip(b[:-1], b[1:]))


# ---- the matrix hand-off --------------------------------------------------------------------------------------------------------------
class Matrix:
    """One matrix on its way to the engine -- a fetched chunk or gathered genes: dense numpy, a CUDA tensor, or the arrays of a CSC /
    CSR matrix (``fmt``: "csc" / "csr", None for dense).  Each pass over the columns [lb, ub) forwards to the public ``Engine`` method
    of its name, or to that method's ``_sparse`` twin, looked up on the engine when the call is made; keywords pass through.

    A chunk of the walk carries its place as well: ``lb`` the global number of its first gene, ``width`` its genes, ``base`` where
    they begin inside ``X``, ``fetched`` the container as the handler read it, ``streams`` whether it was read from storage.  The
    column ranges of the passes count from ``base``."""

    def __init__(self, X, fmt: str = "csc", *, lb: int = 0, width: int | None = None, base: int = 0, fetched=None, streams: bool = False):
        self.X, self.fmt = X, (fmt if hasattr(X, "indptr") else None)
        self.lb, self.width, self.base, self.fetched, self.streams = lb, int(X.shape[1]) if width is None else width, base, fetched, streams

    def _call(self, eng, dense: str, sparse_: str, lb: int, ub: int, kw: dict):
        X, lb, ub = self.X, self.base + lb, self.base + ub
        if self.fmt is None:
            return getattr(eng, dense)(X, lb, ub, **kw)
        return getattr(eng, sparse_)(self.fmt, X.data, X.indices, X.indptr, X.shape, lb, ub, **kw)

    def group_stats(self, eng, lb, ub, **kw):
        return self._call(eng, "group_stats", "group_stats_sparse", lb, ub, kw)

    def group_moments(self, eng, lb, ub, **kw):
        return self._call(eng, "group_moments", "group_moments_sparse", lb, ub, kw)

    def group_value_hists(self, eng, lb, ub, **kw):
        return self._call(eng, "group_value_hists", "group_value_hists_sparse", lb, ub, kw)

    def run(self, eng, lb, ub, **kw):
        return self._call(eng, "run_dense", "run_sparse", lb, ub, kw)

    def pairwise_ranked(self, eng, lb, ub, **kw):
        return self._call(eng, "pairwise_ranked", "pairwise_ranked_sparse", lb, ub, kw)


# ---- the walk -------------------------------------------------------------------------------------------------------------------------
def _windows(lb: int, ub: int, w: int):
    return [(a, min(ub, a + w)) for a in range(lb, ub, w)]


def chunks(X, handler):
    """The chunks of ``_chunks(X, handler)``, each fetched when it is asked for and handed over as a ``Matrix``."""
    fmt = "csr" if handler.fmt.name == "CSR" else "csc"
    for lb, ub in _chunks(X, handler):
        fetched, (a, b) = handler.fetch(lb, ub)
        yield Matrix(handler.to_nb(fetched), fmt, lb=lb, width=ub - lb, base=a, fetched=fetched, streams=getattr(handler, "streams", False))


def walk_windows(chunk: Matrix, per_gene: int, budget: int, body) -> None:
    """``body(chunk, o0, o1)`` over the windows [o0, o1) of one chunk, offsets counted from the chunk's first gene.  A window is
    ``max(64, (budget // per_gene) // 64 * 64)`` genes wide.  One that the body refuses with ``MemoryError`` or
    ``torch.cuda.OutOfMemoryError`` is redone as windows of ``max(64, (w // 2 + 63) // 64 * 64)`` genes, in order, before the rest; a
    refused window of 64 genes or fewer raises.  What the refused body allocated is gone before the retry: its frame dies with the
    exception, and the retry starts outside the ``except`` block."""
    import torch
    todo = _windows(0, chunk.width, max(64, (budget // per_gene) // 64 * 64))
    while todo:
        o0, o1 = todo.pop(0)
        try:
            body(chunk, o0, o1)
            continue
        except (MemoryError, torch.cuda.OutOfMemoryError):
            if o1 - o0 <= 64:
                raise
        todo = _windows(o0, o1, max(64, ((o1 - o0) // 2 + 63) // 64 * 64)) + todo


def walk(X, handler, per_gene: int, budget: int, body) -> None:
    """``body(chunk, o0, o1)`` over every window (``walk_windows``) of every chunk (``chunks``) of ``X``, in order.  A front end with
    work of its own per chunk -- setting groups, gathering flagged genes -- writes this loop out and calls ``walk_windows`` in it."""
    for chunk in chunks(X, handler):
        walk_windows(chunk, per_gene, budget, body)


# ---- the flagged genes ----------------------------------------------------------------------------------------------------------------
def _gather_columns(src, cols: np.ndarray):
    """The columns ``cols`` of one fetched container, in a form the one-versus-reference engine calls take: a dense matrix stays dense
    (numpy, or a CUDA tensor), a sparse one becomes a scipy CSC matrix."""
    if _lib._is_torch_tensor(src):
        import torch
        return src[:, torch.as_tensor(cols, device=src.device)].contiguous()
    if hasattr(src, "indptr"):
        return sparse.csc_matrix(src[:, cols])
    return np.ascontiguousarray(np.asarray(src)[:, cols])


def _hstack(parts):
    if len(parts) == 1:
        return parts[0]
    if _lib._is_torch_tensor(parts[0]):
        import torch
        return torch.cat(parts, dim=1)
    if hasattr(parts[0], "indptr"):
        return sparse.hstack(parts, format="csc")
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


class FlaggedGenes:
    """The flagged genes of one call, gathered chunk by chunk: from the streamed chunk, or from the container as the caller gave it in
    ``handler`` (the device copy of an in-RAM CSR matrix is not sliced by columns).  ``whole``: a chunk of which every gene of the
    matrix is flagged (a log-normalised matrix) is taken as the container itself, not a copy of it, unless it is CSR."""

    def __init__(self, handler, whole: bool = False):
        self.data, self.whole, self.parts, self.cols = handler.data, whole, [], []

    def add(self, chunk: Matrix, offsets) -> None:
        """``offsets``: the flagged genes of the chunk's windows, arrays of offsets from the chunk's first gene."""
        flagged = np.concatenate(offsets) if offsets else np.empty(0, dtype=np.int64)
        if not flagged.size:
            return
        src, off = (chunk.fetched, chunk.base) if chunk.streams else (self.data, chunk.lb)
        if self.whole and flagged.size == int(self.data.shape[1]) and chunk.fmt != "csr":
            self.parts.append(src)
        else:
            self.parts.append(_gather_columns(src, off + flagged))
        self.cols.append(chunk.lb + flagged)

    def result(self):
        """(the gathered genes side by side, their global column numbers), or (None, no numbers)."""
        if not self.parts:
            return None, np.empty(0, dtype=np.int64)
        return _hstack(self.parts), np.concatenate(self.cols)


# ---- host planes ----------------------------------------------------------------------------------------------------------------------
def _span(cols: np.ndarray):
    """``cols`` (ascending) as a slice when they are neighbours -- a block of planes is then written as a block -- else as they are."""
    n = len(cols)
    return slice(int(cols[0]), int(cols[0]) + n) if n and int(cols[-1]) - int(cols[0]) == n - 1 else cols


class HostPlanes:
    """The sink (``sink(cols, planes, skip)``, pairwise.py: ``pairwise_planes``) that keeps every block in host planes
    ``[n, K, K, n_genes]``.  ``skip`` is not looked at: a column a block does not hold is written again by the block that does."""

    def __init__(self, n: int, K: int, M: int):
        self.planes = np.empty((n, K, K, M), dtype=np.float64)

    def __call__(self, cols, planes, skip):
        where = _span(cols)
        for dst, q in zip(self.planes, planes):
            dst[:, :, where] = q.cpu().numpy()


# ---- the frame tails ------------------------------------------------------------------------------------------------------------------
def _pair_index(labels: np.ndarray, features: np.ndarray, r_idx: np.ndarray, g_idx: np.ndarray) -> pd.MultiIndex:
    """(pert, reference, feature) for the pairs (g_idx[k], r_idx[k]) in order, each over all features."""
    names = ["pert", "reference", "feature"]
    li, fi = pd.Index(pd.Series(labels, dtype=str)), pd.Index(pd.Series(features, dtype=str))
    M, P = len(fi), len(r_idx)
    if li.is_unique and fi.is_unique and not li.hasnans and not fi.hasnans and M:
        ll, lf = li.sort_values(), fi.sort_values()
        lcode, fcode = ll.get_indexer(li), lf.get_indexer(fi)
        return pd.MultiIndex(levels=[ll, ll, lf], codes=[np.repeat(lcode[g_idx], M), np.repeat(lcode[r_idx], M), np.tile(fcode, P)],
                             names=names, verify_integrity=False)
    return pd.MultiIndex.from_arrays([np.repeat(np.asarray(li)[g_idx], M), np.repeat(np.asarray(li)[r_idx], M), np.tile(np.asarray(fi), P)],
                                     names=names)


def pair_frame(columns, labels: np.ndarray, features: np.ndarray, code, max_result_bytes: int, compute) -> pd.DataFrame:
    """The ``(pert, reference, feature)`` frame of K groups ``labels`` over the genes ``features``: reference-major, then pert, then
    gene, a group not compared with itself.  A frame of more than ``max_result_bytes`` bytes is refused before ``compute()`` is called;
    it gives the host planes ``[n, K, K, M]`` indexed ``[plane, r, g, gene]`` -- the p-values first -- and the frame's ``attrs``.
    ``columns`` names the planes; ``code`` (not None) adds ``p_value_adj``, each pair adjusted across its genes."""
    K, M = len(labels), len(features)
    n_cols = len(columns) + int(code is not None)
    need = K * (K - 1) * M * 8 * n_cols
    if need > max_result_bytes:
        raise ValueError(f"the result of {K} x {K - 1} pairs over {M} genes with {n_cols} columns takes {need} bytes, more than "
                         f"max_result_bytes = {int(max_result_bytes)}: restrict `groups`, or raise max_result_bytes")
    planes, attrs = compute()
    r_idx, g_idx = np.divmod(np.arange(K * K), K)
    rows = np.flatnonzero(r_idx != g_idx)
    cols = {name: planes[k].reshape(K * K, M)[rows].reshape(-1) for k, name in enumerate(columns)}
    if code is not None:
        adj = _lib.get_engine().adjust_pvalues(np.ascontiguousarray(planes[0].reshape(K * K, M)[rows]), code)
        cols["p_value_adj"] = np.asarray(adj).reshape(-1)
    df = pd.DataFrame(cols, index=_pair_index(labels, features, r_idx[rows], g_idx[rows]), copy=False)
    df.attrs.update(attrs)
    return df


def adjust_and_cut(p, code: str, n_genes, score=None):
    """(``adj``, ``top``) of a ``[G, M]`` host plane of p-values: each row adjusted by ``code``, and -- with ``n_genes`` -- each row's
    first ``min(n_genes, M)`` columns, int64 ``[G, n_top]`` (else None): by ascending p (``Engine.adjust_pvalues(n_top=)``), or by
    descending ``score`` where a score plane is given (``Engine.top_by_score``).  A plane without rows or columns asks no engine."""
    G, M = p.shape
    n_top = min(int(n_genes), M) if n_genes is not None else 0
    if not (G and M):
        return np.empty((G, M), dtype=np.float64), None if n_genes is None else np.empty((G, 0), dtype=np.int64)
    eng = _lib.get_engine()
    if score is None:
        res = eng.adjust_pvalues(p, code, n_top=n_top)
        return res if n_top else (res, None)
    return eng.adjust_pvalues(p, code, n_top=0), eng.top_by_score(score, n_top) if n_top else None


def cut_rows(df: pd.DataFrame, top, M: int) -> pd.DataFrame:
    """The rows of a group-major ``(group, gene)`` frame over M genes that ``top`` (``adjust_and_cut``) keeps, in its order."""
    top = np.asarray(top)
    return df.iloc[(np.arange(len(top), dtype=np.int64)[:, None] * M + top).reshape(-1)]
