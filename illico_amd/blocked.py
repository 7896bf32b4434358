"""Blocked Wilcoxon rank-sum tests: every group against the reference cells of the same block, the per-block tests combined.

A screen or an atlas is run in batches (GEM wells, donors, plates), and the test that is wanted compares a perturbation with the
control cells of the same batch, or a cluster with the rest of the same donor.  ``blocked_wilcoxon`` is scran's ``block=`` of
``pairwiseWilcox`` / ``findMarkers``: in every block that holds both samples the rank-sum test is formed, and a test's blocks are
combined by Stouffer's z weighted with ``n_group x n_reference`` (include/illico_hip_blocked.h states the definition; DESIGN.md
section 27).

For count-valued genes (integers 0 .. 255) the histograms of the compound groups (group x block) are formed on the device in one read
of the matrix (illico_group_value_hists_*) and every test follows from them (illico_blocked_from_hists).  Genes with other values are
gathered once and take one one-versus-reference (or one-versus-rest) engine call per block, on that block's rows, whose z and U planes
are combined on the device (illico_blocked_from_planes): each row is read once in total, by whichever route the engine picks for it.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from illico_amd import _lib
from illico_amd._passes import (FlaggedGenes, Matrix, _input, _product_index, _span, _windows, adjust_and_cut, check_alternative, check_bool,
                                check_corr_method, check_n_genes, chunks, cut_rows, device_handler, walk_windows)
from illico_amd.utils.groups import GroupContainer, encode_and_count_groups

__all__ = ["blocked_wilcoxon"]

#: device bytes one gene window may take (histograms in both layouts, block totals, sums and the result planes); a window the engine's
#: scratch budget refuses is halved
BLOCK_WINDOW_BYTES = 2 << 30


def _check_arguments(adata, is_log1p, block_key, alternative, tie_correct, corr_method, n_genes):
    check_bool("is_log1p", is_log1p)
    check_alternative(alternative)
    check_bool("tie_correct", tie_correct)
    check_n_genes(n_genes)
    if not isinstance(block_key, str) or block_key not in adata.obs:
        raise ValueError(f"block_key {block_key!r} is no column of adata.obs")
    return check_corr_method(corr_method)


def compound_groups(g_codes: np.ndarray, b_codes: np.ndarray, G: int, B: int) -> GroupContainer:
    """The container of the compound coding ``k = g * B + b`` over all G x B compounds (one without cells has count 0), for the
    histogram and sum passes: they use codes, counts and order only."""
    codes = np.ascontiguousarray(g_codes.astype(np.int64) * B + b_codes.astype(np.int64))
    counts = np.bincount(codes, minlength=G * B).astype(np.int64)
    return GroupContainer(codes, counts, np.argsort(codes, kind="stable").astype(np.int64),
                          np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), -1)


def _take_rows(Xf, rows: np.ndarray):
    """The rows ``rows`` of the gathered genes, in the form the engine calls take."""
    from illico_amd._lib import _is_torch_tensor
    if _is_torch_tensor(Xf):
        import torch
        return Xf[torch.as_tensor(rows, device=Xf.device)].contiguous()
    if hasattr(Xf, "indptr"):
        from scipy import sparse
        return sparse.csc_matrix(Xf[rows])
    return np.ascontiguousarray(Xf[rows])


def _plane_genes(eng, Xf, g_codes, b_codes, comp, G, B, ref, is_log1p, tie_correct, alternative, planes, cols, take_rows=_take_rows):
    """The gathered genes ``Xf`` (gene j is column ``cols[j]`` of ``planes``) through one engine call per block and
    ``Engine.blocked_from_planes``, window by window.  ``take_rows(Xf, rows)``: a block's rows of ``Xf``."""
    import torch
    dev = torch.device("cuda", eng.device)
    genes, nf = Matrix(Xf), int(Xf.shape[1])
    counts = np.asarray(comp.counts, dtype=np.int64)
    row_map = np.full((B, G), -1, dtype=np.int32)
    blocks = []  # (b, the block's rows of Xf, its group container)
    for b in range(B):
        rows = np.flatnonzero(b_codes == b)
        present = np.unique(g_codes[rows])
        if ref >= 0 and ref not in present:
            continue  # no test uses this block
        row_map[b, present] = np.arange(present.size, dtype=np.int32)
        if present.size < 2:
            continue  # one group alone: no test but the reference's own row, which reads nothing (the planes stay zero)
        local = np.searchsorted(present, g_codes[rows])
        n_local = np.bincount(local, minlength=present.size).astype(np.int64)
        grp = GroupContainer(local.astype(np.int64), n_local, np.argsort(local, kind="stable").astype(np.int64),
                             np.concatenate([[0], np.cumsum(n_local)]).astype(np.int64), int(np.searchsorted(present, ref)) if ref >= 0 else -1)
        blocks.append((b, Matrix(take_rows(Xf, rows)), grp))
    width = max(64, (BLOCK_WINDOW_BYTES // ((3 * G * B + 6 * G) * 8)) // 64 * 64)
    for a, e in _windows(0, nf, width):
        w = e - a
        zs = torch.zeros((B, G, w), dtype=torch.float64, device=dev)
        us = torch.zeros((B, G, w), dtype=torch.float64, device=dev)
        spare = [torch.empty((G, w), dtype=torch.float64, device=dev) for _ in range(2)]  # the per-block p and fold change: not used
        for b, Xb, grp in blocks:
            eng.set_groups(grp)
            k = int(grp.counts.size)
            out = (spare[0][:k], us[b, :k], spare[1][:k], zs[b, :k])
            Xb.run(eng, a, e, is_log1p=False, use_continuity=False, tie_correct=tie_correct, alternative=alternative, out=out, device_out=True,
                   scores=True)
        eng.set_groups(comp)
        sums = torch.empty((G * B, w), dtype=torch.float64, device=dev)
        genes.group_stats(eng, a, e, is_log1p=is_log1p, out=(None, sums))
        got = eng.blocked_from_planes(zs, us, row_map, counts=counts, ref=ref if ref >= 0 else None, sums=sums, alternative=alternative)
        where = _span(cols[a:e])  # (neighbouring genes -- a matrix flagged whole -- are written as a block)
        for k in range(4):
            planes[k][:, where] = got[k].cpu().numpy()


def blocked_planes(X, handler, g_codes, b_codes, G: int, B: int, ref: int, is_log1p: bool, alternative: str, tie_correct: bool,
                   take_rows=_take_rows):
    """(planes float64 [4, G, n_genes]: p, statistic, fold change, z; number of flagged genes) of the blocked tests of G groups in B
    blocks; ``ref``: the reference group id, -1 for the rest of each block.  ``take_rows(Xf, rows)``: how a block's rows are taken from
    the gathered genes (a container of the caller's own, as tools/bench_blocked.py's device CSC arrays, brings its own)."""
    import torch
    eng = _lib.get_engine()
    dev = torch.device("cuda", eng.device)
    flagged = FlaggedGenes(handler, whole=True)
    handler = device_handler(X, handler)  # an in-RAM CSR matrix goes up once
    comp = compound_groups(g_codes, b_codes, G, B)
    counts = np.asarray(comp.counts, dtype=np.int64)
    GB, M = G * B, int(X.shape[1])
    planes = np.empty((4, G, M), dtype=np.float64)
    per_gene = 2 * GB * 1024 + B * 1024 + 4 * G * 8 + (GB * 8 if is_log1p else 0) + 4

    def hist_window(chunk, o0, o1):
        w = o1 - o0
        H = torch.empty((GB, w, eng.HIST_VALUES), dtype=torch.int32, device=dev)
        fl = torch.empty((w,), dtype=torch.int32, device=dev)
        chunk.group_value_hists(eng, o0, o1, out=(H, fl))
        genes = np.flatnonzero(fl.cpu().numpy())
        if genes.size < w:  # (a window without a count-valued gene -- every window of a log-normalised matrix -- has nothing to combine)
            sums = None
            if is_log1p:
                sums = torch.empty((GB, w), dtype=torch.float64, device=dev)
                chunk.group_stats(eng, o0, o1, is_log1p=True, out=(None, sums))
            got = eng.blocked_from_hists(H, fl, counts=counts, n_blocks=B, ref=ref if ref >= 0 else None, sums=sums, tie_correct=tie_correct,
                                         alternative=alternative)
            for k in range(4):
                planes[k][:, chunk.lb + o0:chunk.lb + o1] = got[k].cpu().numpy()
        chunk_flagged.append(o0 + genes)

    for chunk in chunks(X, handler):
        eng.set_groups(comp)
        chunk_flagged = []
        walk_windows(chunk, per_gene, BLOCK_WINDOW_BYTES, hist_window)
        flagged.add(chunk, chunk_flagged)
    Xf, cols = flagged.result()
    if cols.size:
        _plane_genes(eng, Xf, g_codes, b_codes, comp, G, B, ref, is_log1p, tie_correct, alternative, planes, cols, take_rows)
    return planes, int(cols.size)


def blocked_wilcoxon(adata, is_log1p: bool, group_keys: str, block_key: str, reference: str | None = None, *, alternative: str = "two-sided",
                     tie_correct: bool = True, layer: str | None = None, corr_method: str = "bh", n_genes: int | None = None) -> pd.DataFrame:
    """Asymptotic Wilcoxon rank-sum tests within blocks, combined per (group, gene), on one MI355X.

    ``adata``, ``is_log1p``, ``group_keys``, ``reference``, ``alternative``, ``tie_correct`` and ``layer`` as in ``asymptotic_wilcoxon``;
    ``block_key``: the column of ``adata.obs`` that names each cell's block.  Each group is compared with the cells of ``reference`` --
    or, without one, with all other cells -- of the SAME block, in every block that holds both samples; a test's blocks are combined
    by Stouffer's z with the weights ``n_group x n_reference`` (scran's ``block=``).  There is no ``use_continuity``: the per-block z
    carry no continuity correction, and a half-unit shift has no meaning for a weighted sum.

    Returns a DataFrame with MultiIndex ``(pert, feature)`` in ``asymptotic_wilcoxon``'s order and the columns ``p_value``;
    ``p_value_adj``: ``corr_method`` within each group across the genes (a group without a used block has NaN rows and is left out);
    ``statistic``: the sum of the per-block U; ``fold_change``: the ratio of the means pooled over the used blocks; ``z_score``: the
    combined z, positive when the group ranks above its reference; ``auc`` = ``statistic / sum_b n_group n_reference``; ``n_blocks``:
    the blocks the test rests on.  The reference group's own rows are p = 1, statistic = -1, z = 0.  ``n_genes`` keeps each group's
    rows of smallest p (ties by gene order), in that order.  ``df.attrs``: ``n_flagged_genes`` -- the genes that hold a value which is
    no integer in [0, 255] --, ``n_plane_genes`` -- those combined from per-block engine calls (all of them) --, ``blocks``: the
    block labels, ascending.

    ``ValueError``, before any device work: an unknown ``block_key``, a ``reference`` that is no group, a bad ``alternative``,
    ``corr_method`` or ``n_genes``, a non-bool ``is_log1p``."""
    code = _check_arguments(adata, is_log1p, block_key, alternative, tie_correct, corr_method, n_genes)
    X = _input(adata, layer)
    unique_groups, group_container = encode_and_count_groups(groups=adata.obs[group_keys], ref_group=reference)
    block_labels, block_container = encode_and_count_groups(groups=adata.obs[block_key], ref_group=None)
    g_codes, b_codes = np.asarray(group_container.encoded_groups), np.asarray(block_container.encoded_groups)
    G, B, M, ref = int(len(unique_groups)), int(len(block_labels)), int(X.shape[1]), int(group_container.encoded_ref_group)
    from illico_amd.utils.registry import data_handler_registry
    handler = data_handler_registry.get(X)
    planes, n_flagged = blocked_planes(X, handler, g_codes, b_codes, G, B, ref, bool(is_log1p), alternative, bool(tie_correct))
    eng = _lib.get_engine()
    counts, _, _, _, n_blocks = eng._blocked_sizes(np.bincount(g_codes * B + b_codes, minlength=G * B), G * B, B, ref if ref >= 0 else None)
    n_r = counts[ref][None, :] if ref >= 0 else counts.sum(axis=0)[None, :] - counts
    weight = (counts * n_r * ((counts > 0) & (n_r > 0))).sum(axis=1).astype(np.float64)  # sum over the used blocks of n_g n_r
    live = np.flatnonzero(n_blocks > 0)
    # a group without a used block keeps NaN rows and, under n_genes, its first genes in gene order
    adj = np.full((G, M), np.nan)
    top = np.tile(np.arange(min(int(n_genes), M) if n_genes is not None else 0, dtype=np.int64), (G, 1))
    if M and live.size:
        adj[live], live_top = adjust_and_cut(np.ascontiguousarray(planes[0][live]), code, n_genes)
        if live_top is not None:
            top[live] = live_top
    with np.errstate(divide="ignore", invalid="ignore"):
        auc = planes[1] / weight[:, None]
    cols = {"p_value": planes[0].reshape(-1), "p_value_adj": adj.reshape(-1), "statistic": planes[1].reshape(-1),
            "fold_change": planes[2].reshape(-1), "z_score": planes[3].reshape(-1), "auc": auc.reshape(-1),
            "n_blocks": np.repeat(n_blocks, M)}
    index = _product_index(pd.Series(np.asarray(unique_groups), dtype=str), pd.Series(np.asarray(adata.var_names), dtype=str))
    df = pd.DataFrame(cols, index=index, copy=False)
    if top.shape[1]:
        df = cut_rows(df, top, M)
    df.attrs["n_flagged_genes"] = n_flagged
    df.attrs["n_plane_genes"] = n_flagged
    df.attrs["blocks"] = [str(x) for x in block_labels]
    return df
