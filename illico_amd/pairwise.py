"""All-pairs Wilcoxon rank-sum tests: every group against every other group, from one pass over the matrix.

``pairwise_wilcoxon`` answers the marker-gene question of a clustering ("which genes separate cluster A from B, from C, ...") and of a
perturbation screen that compares perturbations with each other.  Row ``(g, r, gene)`` of its frame is row ``(g, gene)`` of
``asymptotic_wilcoxon(..., reference=r)``.

For count-valued genes (integers 0 .. 255) the statistics of a test are functions of the two groups' value histograms alone: the
histograms of all groups are formed on the device in one read of the matrix (include/illico_hip.h: illico_group_value_hists_*), and
every ordered pair follows from them (illico_pairwise_from_hists).  Genes with other values (continuous, negative, beyond 255) are
gathered once; float32 / int32 values and up to 64 groups take one sorted walk per gene that gives every pair
(illico_pairwise_ranked_*): a log-normalised float32 matrix takes that path whole.  What it cannot take -- other value types, more
groups, a gene with a NaN -- is completed by one one-versus-reference engine call per reference.

``pairwise_markers`` is the marker workflow on top of it (scran's ``combineMarkers``): each group's K - 1 tests are combined on the
device, block of columns by block (illico_combine_pairs), into one row per (group, gene); the K x K planes never reach the host.
With ``method="t-test"`` the blocks are those of the all-pairs Welch t-tests (pairwise_ttest.py: ``pair_ttest_blocks``).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from illico_amd import _lib
from illico_amd._passes import (FlaggedGenes, HostPlanes, Matrix, _gather_columns, _input, _product_index, _select, _windows, adjust_and_cut,
                                check_alternative, check_bool, check_corr_method, check_max_result_bytes, check_n_genes, chunks, cut_rows,
                                device_handler, pair_frame, walk_windows)
from illico_amd.utils.groups import encode_and_count_groups

__all__ = ["pairwise_wilcoxon", "pairwise_markers"]

#: scran's ``pval.type``: how ``pairwise_markers`` combines a group's tests against the other groups
PVAL_TYPES = ("any", "some", "all")
#: device bytes one gene window of the pair route may take (histograms in both layouts and the result planes); a window the engine's
#: scratch budget refuses is halved
PAIR_WINDOW_BYTES = 2 << 30


def _check_arguments(is_log1p, alternative, use_continuity, tie_correct, scores, corr_method, max_result_bytes):
    check_bool("is_log1p", is_log1p)
    check_alternative(alternative)
    for name, v in (("use_continuity", use_continuity), ("tie_correct", tie_correct), ("scores", scores)):
        check_bool(name, v)
    check_max_result_bytes(max_result_bytes)
    return check_corr_method(corr_method, optional=True)


def _ranked_route_takes(eng, Xf, K: int) -> bool:
    """Whether the ranked pair route takes the gathered genes ``Xf``: float32 / int32 values, at most 64 selected groups."""
    dt = Xf.data.dtype if hasattr(Xf, "indptr") else Xf.dtype
    return K <= eng.RANKED_MAX_GROUPS and str(dt).replace("torch.", "") in ("float32", "int32")


def _ranked_pairs(eng, Xf, sel: np.ndarray, planes, cols: np.ndarray, opts: dict, sink=None) -> np.ndarray:
    """The gathered genes ``Xf`` (gene j is column ``cols[j]`` of ``planes``) through ``Engine.pairwise_ranked``, window by window,
    under the engine's current groups.  Returns the genes (indices into ``Xf``'s columns) the route left: their columns are not written.
    With a ``sink`` (``planes`` is then None) each window's planes are written on the device and handed over with its ``left`` words.
    A window the engine refuses is not halved: its genes are left to the fallback."""
    import torch
    K, n_planes, nf = int(sel.size), 4 if opts["scores"] else 3, int(Xf.shape[1])
    dev = torch.device("cuda", eng.device)
    if hasattr(Xf, "indptr"):
        Xf.sort_indices()
    genes = Matrix(Xf)
    width = max(64, (PAIR_WINDOW_BYTES // (n_planes * K * K * 8)) // 64 * 64)
    left_genes = []
    for a, b in _windows(0, nf, width):
        try:
            out = None
            if sink is not None:
                out = [torch.empty((K, K, b - a), dtype=torch.float64, device=dev) for _ in range(n_planes)] + [torch.empty((b - a,), dtype=torch.int32, device=dev)]
            sums = genes.group_stats(eng, a, b, is_log1p=opts["is_log1p"])[1]
            got = genes.pairwise_ranked(eng, a, b, sums=sums, sel=sel, out=out, **opts)
        except (MemoryError, torch.cuda.OutOfMemoryError):
            left_genes.append(np.arange(a, b))
            continue
        if sink is not None:
            sink(cols[a:b], tuple(got[:n_planes]), got[-1])
            left = got[-1].cpu().numpy()
        else:
            got = [q.cpu().numpy() if hasattr(q, "cpu") else q for q in got]
            left = got[-1]
            done = np.flatnonzero(left == 0)
            for k in range(n_planes):
                planes[k][:, :, cols[a + done]] = got[k][:, :, done]
        left_genes.append(a + np.flatnonzero(left != 0))
    return np.concatenate(left_genes) if left_genes else np.empty(0, dtype=np.int64)


def _fallback_blocks(eng, Xr, group_container, sel: np.ndarray, cols: np.ndarray, opts: dict, sink) -> None:
    """The genes ``Xr`` (gene j is column ``cols[j]``) by one one-versus-reference call per reference, for a ``sink``: the K slabs of a
    window of genes are gathered into one device block ``[K, K, w]`` per plane, the window sized by ``PAIR_WINDOW_BYTES``."""
    import torch
    dev = torch.device("cuda", eng.device)
    K, G, n_planes, n = int(sel.size), int(np.asarray(group_container.counts).size), 4 if opts["scores"] else 3, int(Xr.shape[1])
    genes = Matrix(Xr)
    rows = torch.as_tensor(sel, device=dev)
    containers = [group_container._replace(encoded_ref_group=int(r)) for r in sel]
    width = max(64, (PAIR_WINDOW_BYTES // (n_planes * (K * K + G) * 8)) // 64 * 64)
    for a, b in _windows(0, n, width):
        block = tuple(torch.empty((K, K, b - a), dtype=torch.float64, device=dev) for _ in range(n_planes))
        for ri, grp in enumerate(containers):
            eng.set_groups(grp)
            got = genes.run(eng, a, b, device_out=True, **opts)
            for k in range(n_planes):
                block[k][ri] = got[k][rows]
        sink(cols[a:b], block, None)


def _fallback_planes(eng, Xr, group_container, sel: np.ndarray, cols: np.ndarray, opts: dict, planes) -> None:
    """The same genes into host ``planes``: one call per reference over all of them, what a user does by hand."""
    genes, n = Matrix(Xr), int(Xr.shape[1])
    for ri, r in enumerate(sel):
        eng.set_groups(group_container._replace(encoded_ref_group=int(r)))
        got = genes.run(eng, 0, n, **opts)
        for k in range(len(planes)):
            q = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
            planes[k][ri][:, cols] = q[sel]


def pairwise_planes(X, handler, group_container, sel: np.ndarray, is_log1p: bool, alternative: str, use_continuity: bool, tie_correct: bool,
                    scores: bool, sink=None):
    """(planes float64 [3 or 4, K, K, n_genes] indexed [plane, r, g, gene], number of flagged genes, number of them completed by the
    per-reference fallback) for the groups ``sel``.

    ``sink``: a callable ``sink(cols, planes, skip)``.  No host planes are then allocated (the first entry of the result is None):
    every finished block of columns is handed over as it stands on the device -- ``cols`` the int64 gene numbers of its w columns,
    ``planes`` the 3 or 4 float64 CUDA tensors ``[K, K, w]``, ``skip`` an int32 CUDA tensor ``[w]``, non-zero for a column the block
    does not hold (it comes in a later block), or None.  Over all blocks every gene is held exactly once.  Without one, the histogram
    route's blocks go to a sink that keeps host planes (``_passes.HostPlanes``)."""
    import torch
    eng = _lib.get_engine()
    dev = torch.device("cuda", eng.device)
    flagged = FlaggedGenes(handler)
    handler = device_handler(X, handler)  # an in-RAM CSR matrix goes up once
    counts = np.asarray(group_container.counts, dtype=np.int64)
    G, M, K = int(counts.size), int(X.shape[1]), int(sel.size)
    n_planes = 4 if scores else 3
    ovr_groups = group_container._replace(encoded_ref_group=-1)  # the histogram pass uses codes, counts and order only
    eng.set_groups(ovr_groups)
    planes = None
    if sink is None:
        hist_sink = HostPlanes(n_planes, K, M)
        planes = hist_sink.planes
    else:
        hist_sink = sink
    per_gene = 2 * G * 1024 + K * 1024 + n_planes * K * K * 8 + (G * 8 if is_log1p else 0) + 4

    def hist_window(chunk, o0, o1):
        w = o1 - o0
        H = torch.empty((G, w, eng.HIST_VALUES), dtype=torch.int32, device=dev)
        fl = torch.empty((w,), dtype=torch.int32, device=dev)
        sums = torch.empty((G, w), dtype=torch.float64, device=dev) if is_log1p else None
        chunk.group_value_hists(eng, o0, o1, out=(H, fl))
        if is_log1p:
            chunk.group_stats(eng, o0, o1, is_log1p=True, out=(None, sums))
        got = eng.pairwise_from_hists(H, fl, counts=counts, sel=sel, sums=sums, is_log1p=is_log1p, use_continuity=use_continuity,
                                      tie_correct=tie_correct, alternative=alternative, scores=scores)
        hist_sink(np.arange(chunk.lb + o0, chunk.lb + o1, dtype=np.int64), tuple(got), fl)
        chunk_flagged.append(o0 + np.flatnonzero(fl.cpu().numpy()))

    for chunk in chunks(X, handler):
        chunk_flagged = []
        walk_windows(chunk, per_gene, PAIR_WINDOW_BYTES, hist_window)
        flagged.add(chunk, chunk_flagged)
    Xf, cols = flagged.result()
    n_flagged, n_fallback = int(cols.size), 0
    if n_flagged:
        opts = dict(is_log1p=is_log1p, use_continuity=use_continuity, tie_correct=tie_correct, alternative=alternative, scores=scores)
        # any float32 / int32 values, up to 64 groups: every pair from one sorted walk per gene (illico_pairwise_ranked_*) ...
        rest = _ranked_pairs(eng, Xf, sel, planes, cols, opts, sink) if _ranked_route_takes(eng, Xf, K) else np.arange(n_flagged)
        n_fallback = int(rest.size)
        if n_fallback:
            # ... and for what it leaves, one one-versus-reference call per reference
            Xr = Xf if n_fallback == n_flagged else _gather_columns(Xf, rest)
            if sink is not None:
                _fallback_blocks(eng, Xr, group_container, sel, cols[rest], opts, sink)
            else:
                _fallback_planes(eng, Xr, group_container, sel, cols[rest], opts, planes)
    return planes, n_flagged, n_fallback


def pairwise_wilcoxon(adata, is_log1p: bool, group_keys: str, *, groups=None, alternative: str = "two-sided", use_continuity: bool = True,
                      tie_correct: bool = True, layer: str | None = None, scores: bool = False, corr_method: str | None = None,
                      max_result_bytes: int = 8 << 30) -> pd.DataFrame:
    """Asymptotic Wilcoxon rank-sum tests of every group against every other group, on one MI355X.

    ``adata``, ``is_log1p``, ``group_keys``, ``alternative``, ``use_continuity``, ``tie_correct`` and ``layer`` as in
    ``asymptotic_wilcoxon``; every container it accepts is accepted, backed containers are streamed chunk by chunk, an in-RAM CSR
    matrix is uploaded once.  ``groups``: a sequence of labels that restricts both sides of the comparison (default: all groups);
    whatever its order, groups appear in the order ``asymptotic_wilcoxon`` gives them.

    Returns a DataFrame with MultiIndex ``(pert, reference, feature)`` -- reference-major, then pert, then gene; a group is not
    compared with itself -- and float64 columns ``p_value``, ``statistic`` and ``fold_change``; ``z_score`` with ``scores=True``;
    ``p_value_adj`` with ``corr_method`` (``"benjamini-hochberg"`` / ``"bh"``, ``"benjamini-yekutieli"`` / ``"by"``,
    ``"bonferroni"``): each (pert, reference) pair adjusted across its genes.  Row ``(g, r, gene)`` is row ``(g, gene)`` of
    ``asymptotic_wilcoxon(..., reference=r)``.  ``df.attrs["n_flagged_genes"]``: the genes that hold a value which is no integer in
    [0, 255]; ``df.attrs["n_ranked_genes"]`` of them took the sorted walk that gives every pair (float32 / int32 values, up to 64
    groups), ``df.attrs["n_fallback_genes"]`` were completed by one one-versus-reference engine call per reference.

    ``ValueError``: a label of ``groups`` that is not present or named twice, fewer than two groups, a bad ``alternative``, a
    non-bool ``is_log1p``, and a result of more than ``max_result_bytes`` bytes (K (K - 1) x genes x 8 bytes x columns), raised before
    any device work.  ``NotImplementedError``: two selected groups of 2097152 cells or more together."""
    code = _check_arguments(is_log1p, alternative, use_continuity, tie_correct, scores, corr_method, max_result_bytes)
    X = _input(adata, layer)
    unique_raw_groups, group_container = encode_and_count_groups(groups=adata.obs[group_keys], ref_group=None)
    sel = _select(np.asarray(unique_raw_groups), groups)

    def compute():
        from illico_amd.utils.registry import data_handler_registry
        planes, n_flagged, n_fallback = pairwise_planes(X, data_handler_registry.get(X), group_container, sel, bool(is_log1p), alternative,
                                                        bool(use_continuity), bool(tie_correct), bool(scores))
        return planes, {"n_flagged_genes": n_flagged, "n_ranked_genes": n_flagged - n_fallback, "n_fallback_genes": n_fallback}

    columns = ("p_value", "statistic", "fold_change") + (("z_score",) if scores else ())
    return pair_frame(columns, np.asarray(unique_raw_groups)[sel], np.asarray(adata.var_names), code, max_result_bytes, compute)


class _MarkerSink:
    """The sink of ``pairwise_planes`` that combines every block on the device (``Engine.combine_pairs``) and keeps ``[K, M]`` host
    planes: the combined p, the representative reference, and the effects against it -- U, fold change and z; with a t-test method
    (``n_effects=4``) t, fold change, df and Cohen's d."""

    def __init__(self, eng, K: int, M: int, method: str, rank: int, n_effects: int = 3):
        self.eng, self.method, self.rank = eng, method, rank
        self.p = np.empty((K, M), dtype=np.float64)
        self.rep = np.empty((K, M), dtype=np.int32)
        self.effects = [np.empty((K, M), dtype=np.float64) for _ in range(n_effects)]

    def __call__(self, cols, planes, skip):
        got = self.eng.combine_pairs(planes[0], planes[1:], method=self.method, rank=self.rank, skip=skip)
        live = slice(None) if skip is None else np.flatnonzero(skip.cpu().numpy() == 0)
        for dst, q in zip([self.p, self.rep, *self.effects], got):
            dst[:, cols[live]] = q.cpu().numpy()[:, live]


#: ``pairwise_markers``' ``method`` -> the variant of ``pairwise_ttest`` (None: the Wilcoxon tests)
MARKER_METHODS = {"wilcoxon": None, "t-test": "welch", "t-test_overestim_var": "overestim_var"}


def _check_marker_arguments(pval_type, min_prop, n_genes):
    if not isinstance(pval_type, str) or pval_type not in PVAL_TYPES:
        raise ValueError(f"pval_type must be one of {PVAL_TYPES}, got {pval_type!r}")
    if isinstance(min_prop, bool) or not isinstance(min_prop, (int, float, np.integer, np.floating)) or not 0 < min_prop <= 1:
        raise ValueError(f"min_prop must be a number in (0, 1], got {min_prop!r}")
    check_n_genes(n_genes)


def pairwise_markers(adata, is_log1p: bool, group_keys: str, *, groups=None, pval_type: str = "any", min_prop: float = 0.5,
                     alternative: str = "two-sided", use_continuity: bool = True, tie_correct: bool = True, layer: str | None = None,
                     corr_method: str | None = "benjamini-hochberg", n_genes: int | None = None, method: str = "wilcoxon") -> pd.DataFrame:
    """Marker genes of every group from the all-pairs Wilcoxon tests: scran's ``pairwiseWilcox`` followed by ``combineMarkers``, on
    one MI355X, without the K (K - 1) tables per gene ever reaching the host.  ``method="t-test"`` / ``"t-test_overestim_var"``: from
    the all-pairs Welch t-tests instead (``pairwiseTTests``; scran's ``findMarkers`` default), see below.

    The tests are those of ``pairwise_wilcoxon`` (same arguments, same routes).  For each group and gene its K - 1 p-values against
    the other selected groups are combined on the device (include/illico_hip_markers.h: illico_combine_pairs): ``pval_type="all"``
    -- the gene separates the group from every other group: the largest p --, ``"any"`` -- from any of them: Simes' combination --
    or ``"some"`` -- from at least ``min_prop`` of them: Holm's adjusted p of rank ``max(1, ceil((K - 1) * min_prop))``.

    Returns a DataFrame with MultiIndex ``(pert, feature)``, K x genes rows, groups in ``asymptotic_wilcoxon``'s order: ``p_value`` the
    combined p; ``p_value_adj`` (unless ``corr_method`` is None) each group's combined p adjusted across the genes; ``reference`` the
    label of the representative comparison (categorical) -- the one of largest p for ``"all"``, of smallest p for ``"any"``, of that
    rank for ``"some"``, ties by group order --; ``statistic``, ``fold_change`` and ``z_score`` against that reference; ``auc`` =
    ``statistic / (n_group x n_reference)``.  ``n_genes`` keeps each group's rows of smallest combined p (ties by gene order), in that
    order.  ``df.attrs["n_flagged_genes"]`` / ``["n_ranked_genes"]`` / ``["n_fallback_genes"]`` as in ``pairwise_wilcoxon``.

    With a t-test method the tests are those of ``pairwise_ttest`` (``variant="welch"`` for ``"t-test"``, ``"overestim_var"`` for
    ``"t-test_overestim_var"``), combined in the same way; the frame then holds ``p_value``, ``p_value_adj``, ``reference``,
    ``statistic`` (t against the representative), ``fold_change``, ``df`` (the Welch-Satterthwaite degrees of freedom) and ``cohen_d``
    (the difference of the means over the root of the two variances' mean) -- no ``z_score`` or ``auc``, no ``attrs``.
    ``use_continuity`` and ``tie_correct`` mean nothing to a t-test: a non-default value is a ``ValueError``.

    ``ValueError``, before any device work: a bad ``pval_type``, ``min_prop`` outside (0, 1], a bad ``n_genes``, an unknown ``method``,
    and what ``pairwise_wilcoxon`` refuses (there is no ``max_result_bytes``: the result is K x genes).  ``NotImplementedError``: more
    than 256 selected groups."""
    _check_marker_arguments(pval_type, min_prop, n_genes)
    if not isinstance(method, str) or method not in MARKER_METHODS:
        raise ValueError(f"method must be one of {tuple(MARKER_METHODS)}, got {method!r}")
    ttest = method != "wilcoxon"
    if ttest:
        from illico_amd.pairwise_ttest import MARKER_PLANES, pair_ttest_blocks
        if use_continuity is not True or tie_correct is not True:
            raise ValueError("use_continuity and tie_correct belong to the Wilcoxon tests: leave them at their defaults with a t-test method")
        check_bool("is_log1p", is_log1p)
        check_alternative(alternative)
        code = check_corr_method(corr_method, optional=True)
    else:
        code = _check_arguments(is_log1p, alternative, use_continuity, tie_correct, True, corr_method, 0)
    X = _input(adata, layer)
    unique_raw_groups, group_container = encode_and_count_groups(groups=adata.obs[group_keys], ref_group=None)
    sel = _select(np.asarray(unique_raw_groups), groups)
    K, M = int(sel.size), int(X.shape[1])
    if K > _lib.COMBINE_MAX_GROUPS:
        raise NotImplementedError(f"{K} groups selected: pairwise_markers takes up to {_lib.COMBINE_MAX_GROUPS}")
    rank = _lib.combine_rank(K - 1, pval_type, None, min_prop)
    from illico_amd.utils.registry import data_handler_registry
    handler = data_handler_registry.get(X)
    eng = _lib.get_engine()
    if ttest:
        effect_names = ("statistic", "fold_change", "df", "cohen_d")
        sink = _MarkerSink(eng, K, M, pval_type, rank, n_effects=len(effect_names))
        pair_ttest_blocks(X, handler, group_container, sel, bool(is_log1p), MARKER_METHODS[method], alternative, MARKER_PLANES, sink)
    else:
        effect_names = ("statistic", "fold_change", "z_score")
        sink = _MarkerSink(eng, K, M, pval_type, rank)
        _, n_flagged, n_fallback = pairwise_planes(X, handler, group_container, sel, bool(is_log1p), alternative, bool(use_continuity),
                                                   bool(tie_correct), True, sink=sink)
    labels = np.asarray(unique_raw_groups)[sel]
    cols = {"p_value": sink.p.reshape(-1)}
    top = None
    if M and (code is not None or n_genes is not None):  # (without a correction the ranking alone is wanted: any method gives it)
        adj, top = adjust_and_cut(sink.p, code or "bh", n_genes)
        if code is not None:
            cols["p_value_adj"] = np.asarray(adj).reshape(-1)
    elif code is not None:
        cols["p_value_adj"] = np.empty(0, dtype=np.float64)
    cols["reference"] = pd.Categorical.from_codes(sink.rep.reshape(-1), categories=pd.Index(pd.Series(labels, dtype=str)))
    for name, e in zip(effect_names, sink.effects):
        cols[name] = e.reshape(-1)
    if not ttest:
        n_cells = np.asarray(group_container.counts, dtype=np.float64)[sel]
        cols["auc"] = (sink.effects[0] / (n_cells[:, None] * n_cells[sink.rep])).reshape(-1)
    index = _product_index(pd.Series(labels, dtype=str), pd.Series(np.asarray(adata.var_names), dtype=str))
    df = pd.DataFrame(cols, index=index, copy=False)
    if top is not None:
        df = cut_rows(df, top, M)
    if not ttest:
        df.attrs["n_flagged_genes"] = n_flagged
        df.attrs["n_ranked_genes"] = n_flagged - n_fallback
        df.attrs["n_fallback_genes"] = n_fallback
    return df
