"""A float64 numpy restatement of the blocked Wilcoxon definition (include/illico_hip_blocked.h), and the case
builders of tests/test_blocked_host.py, tests/test_gpu_blocked.py and their edge-case siblings (tests/test_blocked_edges_host.py,
tests/test_gpu_blocked_edges.py).

Per block the reference's U and the tie sum come from ``np.unique`` counts; z_b restates ``zscore_device_pre``; the combination is the
weighted Stouffer sum over the used blocks in ascending block order, finished with ``scipy.special.erfc``.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
from scipy.special import erfc

ALTERNATIVES = ("two-sided", "less", "greater")

#: per (group, block, gene) statistics: ``used`` bool [G, B]; sizes int64 [G, B]; the rest float64 [G, B, W]
BlockStats = namedtuple("BlockStats", "used n_g n_r U tie S_g S_r")
BlockedResult = namedtuple("BlockedResult", "p statistic fold z n_blocks auc")


def block_stats(X, g_codes, b_codes, G, B, ref=None, is_log1p=False) -> BlockStats:
    """The statistics of every test (g, gene) in every block.  ``ref``: the reference group id, None for the rest of the block."""
    X = np.asarray(X)
    N, W = X.shape
    V = np.expm1(X.astype(np.float64)) if is_log1p else X.astype(np.float64)
    used = np.zeros((G, B), dtype=bool)
    n_g = np.zeros((G, B), dtype=np.int64)
    n_r = np.zeros((G, B), dtype=np.int64)
    U, tie, S_g, S_r = (np.zeros((G, B, W)) for _ in range(4))
    for b in range(B):
        rows = np.flatnonzero(b_codes == b)
        gb = g_codes[rows]
        cnt = np.bincount(gb, minlength=G)
        for g in range(G):
            n_g[g, b] = cnt[g]
            n_r[g, b] = cnt[ref] if ref is not None else rows.size - cnt[g]
            used[g, b] = n_g[g, b] > 0 and n_r[g, b] > 0
        if not used[:, b].any():
            continue
        Sb = np.stack([V[rows[gb == g]].sum(axis=0) if cnt[g] else np.zeros(W) for g in range(G)])  # [G, W]
        for j in range(W):
            vals, inv = np.unique(X[rows, j], return_inverse=True)
            h = np.zeros((G, vals.size), dtype=np.int64)
            np.add.at(h, (gb, inv.reshape(-1)), 1)
            tot = h.sum(axis=0)
            for g in range(G):
                if not used[g, b]:
                    continue
                hg = h[g]
                hr = h[ref] if ref is not None else tot - hg
                below_g = np.cumsum(hg) - hg                       # cells of g below each value
                two_u = int((hr * (2 * below_g + hg)).sum())       # 2 x (pairs with the reference cell above + half the ties)
                t = hg + hr
                U[g, b, j] = 0.5 * float(two_u)
                tie[g, b, j] = float(int((t * t * t - t).sum()))
                S_g[g, b, j] = Sb[g, j]
                S_r[g, b, j] = Sb[ref, j] if ref is not None else Sb[:, j].sum() - Sb[g, j]
    return BlockStats(used, n_g, n_r, U, tie, S_g, S_r)


def stats_from_hists(H, counts, ref=None) -> BlockStats:
    """The statistics of every test from the value histograms ``H`` ``[G * B, W, 256]`` (compound ``g * B + b``) and the compound sizes
    ``counts`` ``[G, B]`` alone, in Python integers: S2 (twice the cells of the reference below each cell of g, plus the ties), the tie
    sum and the value sums are exact at any size; then ``U = 0.5 * float(2 n_r n_g - S2)`` and ``tie = float(TT)``, each rounded once."""
    counts = np.asarray(counts, dtype=np.int64)
    G, B = counts.shape
    H = np.asarray(H)
    W = H.shape[1]
    used = np.zeros((G, B), dtype=bool)
    n_g, n_r = counts.copy(), np.zeros((G, B), dtype=np.int64)
    U, tie, S_g, S_r = (np.zeros((G, B, W)) for _ in range(4))
    for b in range(B):
        for g in range(G):
            n_r[g, b] = counts[ref, b] if ref is not None else counts[:, b].sum() - counts[g, b]
            used[g, b] = n_g[g, b] > 0 and n_r[g, b] > 0
        for j in range(W):
            h = [[int(x) for x in H[g * B + b, j]] for g in range(G)]
            tot = [sum(col) for col in zip(*h)]
            for g in range(G):
                if not used[g, b]:
                    continue
                hg = h[g]
                hr = h[ref] if ref is not None else [t - a for t, a in zip(tot, hg)]
                below = S2 = TT = 0
                for a, r in zip(hg, hr):
                    S2 += a * (2 * below + r)
                    below += r
                    TT += (a + r) ** 3 - (a + r)
                U[g, b, j] = 0.5 * float(2 * int(n_r[g, b]) * int(n_g[g, b]) - S2)
                tie[g, b, j] = float(TT)
                S_g[g, b, j] = float(sum(c * a for c, a in enumerate(hg)))
                S_r[g, b, j] = float(sum(c * r for c, r in enumerate(hr)))
    return BlockStats(used, n_g, n_r, U, tie, S_g, S_r)


def z_block(n_g: int, n_r: int, tie: float, U: float) -> float:
    """``zscore_device_pre`` with ``group_const(n_r, n_g, n_r + n_g)`` (kernels_finalize.h), operation by operation."""
    n = n_g + n_r
    nnn = float(n * (n - 1) * (n + 1))
    var0 = float(n_r * n_g * (n + 1)) / 12.0
    mu = float(n_r * n_g) / 2.0
    tie_corr = 1.0 - tie / nnn
    if tie_corr > 1.0e-9:
        return (mu - U) / math.sqrt(var0 * tie_corr)
    return 0.0


def p_of_z(Z: float, alternative: str) -> float:
    if alternative == "two-sided":
        return float(erfc(abs(Z) / math.sqrt(2.0)))
    if alternative == "greater":
        return float(0.5 * erfc(-Z / math.sqrt(2.0)))
    return float(0.5 * erfc(Z / math.sqrt(2.0)))


def combine(st: BlockStats, ref=None, alternative="two-sided", tie_correct=True, z_blocks=None) -> BlockedResult:
    """The combined planes ``[G, W]`` from the per-block statistics.  ``z_blocks``: per-block z ``[G, B, W]`` to use instead of the
    model's own (the independent form of tests/test_blocked_host.py)."""
    G, B, W = st.U.shape
    p, stat, fold, z = (np.full((G, W), np.nan) for _ in range(4))
    n_blocks = st.used.sum(axis=1).astype(np.int64)
    auc = np.full((G, W), np.nan)
    for g in range(G):
        blocks = np.flatnonzero(st.used[g])
        if blocks.size == 0:
            continue
        ng, nr = int(st.n_g[g, blocks].sum()), int(st.n_r[g, blocks].sum())
        for j in range(W):
            wz = ww = u = w_sum = sg = sr = 0.0
            z1 = 0.0
            for k, b in enumerate(blocks):
                w = float(int(st.n_g[g, b]) * int(st.n_r[g, b]))
                zb = float(z_blocks[g, b, j]) if z_blocks is not None else \
                    z_block(int(st.n_g[g, b]), int(st.n_r[g, b]), float(st.tie[g, b, j]) if tie_correct else 0.0, float(st.U[g, b, j]))
                if k == 0:
                    z1 = zb
                wz += w * zb
                ww += w * w
                u += float(st.U[g, b, j])
                w_sum += w
                sg += float(st.S_g[g, b, j])
                sr += float(st.S_r[g, b, j])
            # over one used block the weighted form IS z_b: taken as such, not as the twice-rounded (w z) / w
            Z = z1 if blocks.size == 1 else wz / math.sqrt(ww)
            mu_r = sr / float(nr)
            z[g, j], p[g, j], stat[g, j], auc[g, j] = Z, p_of_z(Z, alternative), u, u / w_sum
            fold[g, j] = math.inf if mu_r == 0.0 else (sg / float(ng)) / mu_r
        if ref is not None and g == ref:  # the reference group's own row, as k_finalize writes it
            p[g], stat[g], z[g], auc[g] = 1.0, -1.0, 0.0, -1.0 / float(sum(int(st.n_g[g, b]) * int(st.n_r[g, b]) for b in blocks))
    return BlockedResult(p, stat, fold, z, n_blocks, auc)


def blocked_model(X, g_codes, b_codes, G, B, ref=None, alternative="two-sided", tie_correct=True, is_log1p=False) -> BlockedResult:
    return combine(block_stats(X, g_codes, b_codes, G, B, ref, is_log1p), ref, alternative, tie_correct)


def combine_planes(zs, us, row_map, counts, ref=None, alternative="two-sided"):
    """The combination alone, vectorised over genes: what a user does on the host with the z and U planes ``[B, G, W]`` of B per-block
    engine calls (``row_map`` ``[B, G]``: the row of group g in block b's planes, -1 without cells; ``counts`` ``[G, B]``).  Returns
    ``(p, statistic, z)`` ``[G, W]``; tools/bench_blocked.py times it as the baseline's host step."""
    zs, us, counts = np.asarray(zs), np.asarray(us), np.asarray(counts, dtype=np.int64)
    B, G, W = zs.shape
    n_r = counts[ref][None, :] if ref is not None else counts.sum(axis=0)[None, :] - counts
    used = (counts > 0) & (n_r > 0) & (np.asarray(row_map).T >= 0)
    w = (counts * n_r).astype(np.float64) * used
    wz, ww, stat, z1 = np.zeros((G, W)), np.zeros((G, 1)), np.zeros((G, W)), np.zeros((G, W))
    seen = np.zeros(G, dtype=bool)
    for b in range(B):
        rows = np.where(used[:, b], np.asarray(row_map)[b], 0)
        zb, ub = zs[b][rows] * used[:, b, None], us[b][rows] * used[:, b, None]
        z1 = np.where((used[:, b] & ~seen)[:, None], zb, z1)
        seen |= used[:, b]
        wz += w[:, b, None] * zb
        ww += (w[:, b] * w[:, b])[:, None]
        stat += ub
    n_blocks = used.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = np.where((n_blocks == 1)[:, None], z1, wz / np.sqrt(ww))
    if alternative == "two-sided":
        p = erfc(np.abs(Z) / math.sqrt(2.0))
    else:
        p = 0.5 * erfc((-Z if alternative == "greater" else Z) / math.sqrt(2.0))
    dead = n_blocks == 0
    p[dead], stat[dead], Z[dead] = np.nan, np.nan, np.nan
    if ref is not None:
        p[ref], stat[ref], Z[ref] = 1.0, -1.0, 0.0
    return p, stat, Z


# ---- case builders ----
Case = namedtuple("Case", "X g_codes b_codes G B")


def make_case(G: int, B: int, W: int, seed: int = 0, base: int = 7, values: str = "small") -> Case:
    """Counts 0 .. 5 (float32) for G groups in B blocks of unequal sizes: compound (g, b) holds ``base + 3 b + (g + 2 b) % 4`` cells,
    in shuffled row order.  Gene ``W // 2`` holds the values 0 and 255 only.

    ``values="full-range"``: counts 0 .. 255 instead, so that every part of the 256-value walk carries cells; gene 0 holds 248 .. 255
    only (the last unroll group), gene 1 multiples of 8 (one value in every unroll group), gene ``W // 2`` 0 and 255 as before."""
    if values not in ("small", "full-range"):
        raise ValueError(values)
    rng = np.random.RandomState(1000 * G + 100 * B + W + seed)
    g_codes, b_codes = [], []
    for g in range(G):
        for b in range(B):
            n = base + 3 * b + (g + 2 * b) % 4
            g_codes += [g] * n
            b_codes += [b] * n
    g_codes, b_codes = np.array(g_codes), np.array(b_codes)
    perm = rng.permutation(g_codes.size)
    g_codes, b_codes = g_codes[perm], b_codes[perm]
    N = g_codes.size
    if values == "full-range":
        X = rng.randint(0, 256, size=(N, W))
        X[:, 0] = rng.randint(248, 256, size=N)
        if W > 1:
            X[:, 1] = 8 * rng.randint(0, 32, size=N)
    else:
        # a shift per (group, gene) keeps the tests from being all alike; values stay within 0 .. 5
        X = rng.randint(0, 4, size=(N, W)) + (rng.rand(G, W) < 0.3)[g_codes] * rng.randint(0, 3, size=(N, W))
    X[:, W // 2] = 255 * (rng.rand(N) < 0.5)
    return Case(X.astype(np.float32), g_codes, b_codes, G, B)


def labels_of(codes, prefix: str) -> np.ndarray:
    """String labels whose ``np.unique`` order is the order of the codes."""
    return np.array([f"{prefix}{int(c):03d}" for c in codes])


def edge_case(kind: str, W: int = 5, ref: int = 0) -> Case:
    """The blocks that do not count (tests/test_gpu_blocked.py, case 4).  Group ``ref`` is the reference of the reference-mode tests:
    the cases are stated below for ``ref = 0``, and another ``ref`` rotates the roles of the groups, ``g -> (g + ref) % G``, over the
    same rows and values.

    ``group-absent``: group 2 has no cells in block 1.  ``reference-absent``: group 0 has none in block 2.  ``no-shared-block``: group 3
    lives in block 3 alone, where group 0 has no cells.  ``one-against-one``: block 1 holds one cell of group 1 and one of group 0 (and
    nothing else).  ``constant-block``: gene 1 is constant in block 0.  ``constant-gene``: gene 2 is constant everywhere.
    ``below-reference-absent``: group 3 -- after the rotation group ``ref - 1``, the one just below the reference -- has no cells in
    block 1, where the reference has: in that block the reference's row among the groups present is not ``ref``."""
    rng = np.random.RandomState(sum(map(ord, kind)))
    G, B = 4, 4
    sizes = np.array([[6 + (g + 2 * b) % 5 for b in range(B)] for g in range(G)])
    if kind == "group-absent":
        sizes[2, 1] = 0
    elif kind == "reference-absent":
        sizes[0, 2] = 0
    elif kind == "no-shared-block":
        sizes[3, :3] = 0
        sizes[0, 3] = 0
    elif kind == "one-against-one":
        sizes[:, 1] = 0
        sizes[0, 1] = sizes[1, 1] = 1
    elif kind == "below-reference-absent":
        sizes[3, 1] = 0
    elif kind not in ("constant-block", "constant-gene"):
        raise ValueError(kind)
    if not 0 <= ref < G:
        raise ValueError(ref)
    g_codes = np.repeat(np.repeat(np.arange(G), B), sizes.reshape(-1))
    b_codes = np.repeat(np.tile(np.arange(B), G), sizes.reshape(-1))
    perm = rng.permutation(g_codes.size)
    g_codes, b_codes = g_codes[perm], b_codes[perm]
    X = rng.randint(0, 6, size=(g_codes.size, W))
    if kind == "constant-block":
        X[b_codes == 0, 1] = 3
    if kind == "constant-gene":
        X[:, 2] = 2
    return Case(X.astype(np.float32), (g_codes + ref) % G, b_codes, G, B)


LIMIT_CELLS = 2097151  # the largest test illico_blocked_from_hists accepts (n_g + n_r of one block)


def limit_case(mode: str):
    """``(H uint32 [6, 4, 256], flags uint32 [4], counts int64 [3, 2], ref)``: synthetic histograms of G = 3 groups in B = 2 blocks whose
    largest test holds ``LIMIT_CELLS`` cells, for the C entry points -- no matrix of that size is needed.

    ``"reference"``: ref = 1 and the test of group 0 in block 0 has 1048576 + 1048575 cells.  ``"rest"``: ref = None and block 0 holds
    1048576 + 1048570 + 5 cells.  Every compound's histogram row sums to its count.  In block 0 gene 0 has all cells in bin 255 (the
    largest tie sum there is, n^3 - n < 2^63, and z_b = 0); gene 1 bins 0 and 255 only, group 0 with n / 2 + 3000 cells in bin 255 and
    every other group split evenly (the odd cell in bin 0): z_b of about 4; gene 2 a multinomial draw over the 256 bins per compound.
    Block 1 holds 7, 9 and 11 cells: gene 0 constant (bin 0), genes 1 and 2 drawn over the whole range.  Gene 3 is flagged and its
    words are 0xFFFFFFFF: nothing may read them."""
    if mode == "reference":
        counts, ref = np.array([[1048576, 7], [1048575, 9], [5, 11]], dtype=np.int64), 1
    elif mode == "rest":
        counts, ref = np.array([[1048576, 7], [1048570, 9], [5, 11]], dtype=np.int64), None
    else:
        raise ValueError(mode)
    G, B, W = 3, 2, 4
    rng = np.random.RandomState(0)
    H = np.zeros((G * B, W, 256), dtype=np.uint32)
    for g in range(G):
        for b in range(B):
            n, row = int(counts[g, b]), H[g * B + b]
            if b == 0:
                row[0, 255] = n
                row[1, 255] = n // 2 + (3000 if g == 0 else 0)
                row[1, 0] = n - int(row[1, 255])
            else:
                row[0, 0] = n
                row[1] = rng.multinomial(n, [1.0 / 256] * 256)
            row[2] = rng.multinomial(n, [1.0 / 256] * 256)
            row[3] = 0xFFFFFFFF
    return H, np.array([0, 0, 0, 1], dtype=np.uint32), counts, ref
