"""The numpy restatement of illico_combine_pairs (include/illico_hip_markers.h), in the sorted form: a stable argsort of each group's
K - 1 p-values along the reference axis, then the three formulas exactly as the header writes them -- IEEE float64, in that order."""
import math

import numpy as np

METHODS = ("all", "any", "some")


def default_rank(n: int, min_prop: float = 0.5) -> int:
    return max(1, math.ceil(n * min_prop))


def combine_model(P, effects=(), *, method, rank=None, min_prop=0.5):
    """``(p [K, W], rep int32 [K, W], *selected effects)`` of the ``[K, K, W]`` plane ``P`` indexed ``[r, g, j]``; the diagonal is never
    read.  ``rank``: j* of ``method="some"`` (default ``max(1, ceil(n * min_prop))``)."""
    assert method in METHODS
    P = np.asarray(P, dtype=np.float64)
    K, W = P.shape[0], P.shape[2]
    n = K - 1
    j_star = default_rank(n, min_prop) if rank is None else int(rank)
    assert 1 <= j_star <= n
    out_p = np.empty((K, W), dtype=np.float64)
    rep = np.empty((K, W), dtype=np.int32)
    i = np.arange(1, n + 1, dtype=np.float64)[:, None]
    for g in range(K):
        refs = np.array([r for r in range(K) if r != g])
        sub = P[refs, g, :]                                   # [n, W]
        order = np.argsort(sub, axis=0, kind="stable")        # rank i - 1 -> position among refs
        ps = np.take_along_axis(sub, order, axis=0)           # p_(1) .. p_(n)
        if method == "all":
            out_p[g], i_star = ps[n - 1], n
        elif method == "any":
            out_p[g], i_star = (ps * float(n) / i).min(axis=0), 1
        else:
            out_p[g], i_star = np.minimum(1.0, (ps[:j_star] * (float(n) - i[:j_star] + 1.0)).max(axis=0)), j_star
        rep[g] = refs[order[i_star - 1]]
    cols = np.arange(W)
    selected = [np.stack([np.asarray(E)[rep[g], g, cols] for g in range(K)]) for E in effects]
    return (out_p, rep, *selected)
