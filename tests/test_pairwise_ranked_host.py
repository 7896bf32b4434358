"""All-pairs Wilcoxon tests for any values from one sorted walk per gene (illico_pairwise_ranked_*): the L / T / X definition of
include/illico_hip_ranked.h and DESIGN.md section 20 restated in numpy integers -- the zeros handled by the correction at the end, as the
device does -- and held to the CPU oracle run once per reference.  The integers are finalised by pairs_exact of test_pairwise_host
(no copy of the p-value formula here).  tests/test_gpu_pairwise_ranked.py imports the cases and the restatement."""
import functools

import numpy as np

import oracle
from test_pairwise_host import exact_planes, groups_of, hists_numpy, offdiag, pair_ints, pairs_numpy

RANKED_SIZES = (1, 2, 63, 64, 65, 300, 1024, 1141)
#: the constructed genes of ranked_case("f32")
KINDS = ("negatives", "70 % zeros", "log1p of small counts", "constant non-zero", "all zero", "one non-zero", "-0.0", "+-inf", "denormal",
         "one ulp apart")
TIE_HEAVY = 2


@functools.lru_cache(maxsize=None)
def ranked_case(name):
    """(X [2660, M], codes int64, counts int64).  "f32": 130 float32 genes, the first ten as KINDS names them; "i32": 20 int32 genes with
    negatives and values beyond 255.  Shared: do not write to them."""
    rng = np.random.RandomState(171)
    N = sum(RANKED_SIZES)
    codes = rng.permutation(np.repeat(np.arange(len(RANKED_SIZES)), RANKED_SIZES))
    if name == "i32":
        X = rng.poisson(2.0, size=(N, 20)).astype(np.int32)
        X[rng.rand(N, 20) < 0.6] = 0
        X[:, 1] -= 3                                                  # negatives, zeros among them
        X[:, 2] = rng.randint(-100000, 100000, size=N)                # far beyond 255, nearly tie-free
        X[::5, 3] = 1000 + rng.randint(0, 3, size=X[::5, 3].size)
        X[0, 4], X[1, 4] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
        X[:, 5] = 7
    else:
        M = 130
        X = np.zeros((N, M), dtype=np.float32)
        for j in range(M):
            kind = j % 3
            if kind == 0:    # log-normalised counts: tie-heavy, mostly zero
                X[:, j] = np.log1p(rng.poisson(rng.uniform(0.2, 3.0), size=N)).astype(np.float32)
            elif kind == 1:  # continuous, 70 % zeros
                X[:, j] = rng.lognormal(size=N).astype(np.float32) * (rng.rand(N) < 0.3)
            else:            # continuous, both signs, no zero
                X[:, j] = rng.normal(size=N).astype(np.float32)
        X[:, 0] = -np.abs(rng.normal(size=N)).astype(np.float32) * (rng.rand(N) < 0.5)
        X[:, 1] = rng.lognormal(size=N).astype(np.float32) * (rng.rand(N) < 0.3)
        X[:, 2] = np.log1p(rng.poisson(1.0, size=N)).astype(np.float32)
        X[:, 3] = 2.5
        X[:, 4] = 0.0
        X[:, 5] = 0.0
        X[np.flatnonzero(codes == 5)[7], 5] = 3.25
        X[:, 6] = rng.poisson(0.7, size=N).astype(np.float32) * 0.5
        X[::4, 6] = -0.0
        X[:, 7] = rng.normal(size=N).astype(np.float32)
        X[np.flatnonzero(codes == 6)[:3], 7] = np.inf
        X[np.flatnonzero(codes == 7)[:2], 7] = -np.inf
        X[:, 8] = rng.poisson(0.3, size=N).astype(np.float32)
        X[np.flatnonzero(codes == 5)[:9], 8] = np.nextafter(np.float32(0), np.float32(1))
        X[np.flatnonzero(codes == 6)[:4], 8] = -np.nextafter(np.float32(0), np.float32(1))
        X[:, 9] = np.where(rng.rand(N) < 0.5, np.float32(1.0), np.nextafter(np.float32(1), np.float32(2)))
    for a in (X, codes):
        a.setflags(write=False)
    return X, codes.astype(np.int64), np.asarray(RANKED_SIZES, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def ranked_oracle_slabs(name, is_log1p=False, use_continuity=True, tie_correct=True, alternative="two-sided"):
    """(p, U, fc) float64 [G, G, M]: slab r = oracle.run with reference r"""
    X, codes, counts = ranked_case(name)
    out = [oracle.run(np.ascontiguousarray(X), groups_of(codes, r), is_log1p=is_log1p, use_continuity=use_continuity, tie_correct=tie_correct,
                      alternative=alternative) for r in range(counts.size)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def recode(x):
    """(codes int64 [N] in 0 .. d - 1, d): the values of one gene recoded order-preservingly; -0.0 and 0.0 share a code"""
    u, inv = np.unique(np.asarray(x, dtype=np.float64) + 0.0, return_inverse=True)
    return inv.astype(np.int64), int(u.size)


def ltx_numpy(x, codes, counts, sel):
    """(S2, tie) Python-int object arrays [K, K] indexed [r][g] of one gene: the walk over the NON-ZERO values alone, the zeros added at
    the end -- the definition as the device evaluates it."""
    v = np.asarray(x, dtype=np.float64)
    K = len(sel)
    n = [int(counts[s]) for s in sel]
    nz = v != 0
    vals, inv = np.unique(v[nz], return_inverse=True)
    t = np.zeros((K, vals.size), dtype=np.int64)
    slot = np.full(int(counts.size), -1)
    slot[np.asarray(sel)] = np.arange(K)
    s = slot[codes[nz]]
    np.add.at(t, (s[s >= 0], inv[s >= 0]), 1)
    t = t.astype(object)
    c = np.concatenate([np.zeros((K, 1), dtype=object), np.cumsum(t, axis=1)[:, :-1]], axis=1) if vals.size else t
    L = t @ c.T                                                    # L[g][r] = sum_v t_g(v) c_r(v)
    T = (t ** 3 - t).sum(axis=1) if vals.size else np.zeros(K, dtype=object)
    X = np.array([[(t[g] * t[r] * (t[g] + t[r])).sum() if vals.size else 0 for r in range(K)] for g in range(K)], dtype=object)
    neg = np.array([int(t[k][vals < 0].sum()) for k in range(K)], dtype=object)
    pos = np.array([int(t[k][vals > 0].sum()) for k in range(K)], dtype=object)
    z = np.array(n, dtype=object) - neg - pos
    L = L + np.outer(pos, z) + np.outer(z, neg)
    T = T + z ** 3 - z
    X = X + np.array([[z[g] * z[r] * (z[g] + z[r]) for r in range(K)] for g in range(K)], dtype=object)
    S2 = np.empty((K, K), dtype=object)
    tie = np.empty((K, K), dtype=object)
    for r in range(K):
        for g in range(K):
            S2[r, g] = n[g] * n[r] + L[g, r] - L[r, g]
            tie[r, g] = T[g] + T[r] + 3 * X[g, r]
    return S2, tie


def ints_of(S2, tie, n_r, n_g):
    """the record pairs_exact finalises (test_pairwise_host.pair_ints), from the walk's integers; the value sums play no part"""
    n = n_g + n_r
    return dict(S2=int(S2), two_u=2 * n_r * n_g - int(S2), tie=int(tie), nnn=n * (n - 1) * (n + 1), var12=n_r * n_g * (n + 1), n12=n_r * n_g,
                n_g=n_g, n_r=n_r, S_g=0, S_r=0)


def ranked_planes_numpy(X, codes, counts, sel=None, *, use_continuity=True, tie_correct=True, alternative="two-sided"):
    """dict of float64 [K, K, M] planes U, p, z, tie_corr indexed [r, g, gene] (test_pairwise_host.exact_planes of the walk's integers)
    and fc from float64 sums of the values"""
    sel = list(range(counts.size)) if sel is None else [int(s) for s in sel]
    K, M = len(sel), X.shape[1]
    n = [int(counts[s]) for s in sel]
    ints = {}
    for j in range(M):
        S2, tie = ltx_numpy(X[:, j], codes, counts, sel)
        for r in range(K):
            for g in range(K):
                ints[r, g, j] = ints_of(S2[r, g], tie[r, g], n[r], n[g])
    out = dict(exact_planes(np.zeros((K, M, 1), dtype=np.int64), np.asarray(n), use_continuity=use_continuity, tie_correct=tie_correct,
                            alternative=alternative, ints=ints))
    sums = np.stack([np.asarray(X, dtype=np.float64)[codes == s].sum(axis=0) for s in sel])
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = sums / np.asarray(n, dtype=np.float64)[:, None]
        out["fc"] = np.where(mean[:, None, :] == 0.0, np.inf, mean[None, :, :] / mean[:, None, :])
    return out


@functools.lru_cache(maxsize=None)
def ranked_exact(name, genes=None, **opts):
    X, codes, counts = ranked_case(name)
    return ranked_planes_numpy(X if genes is None else X[:, list(genes)], codes, counts, **opts)


def test_walk_restatement_matches_the_oracle_for_every_reference():
    X, codes, counts = ranked_case("f32")
    genes = tuple(range(len(KINDS))) + (10, 11, 12)
    # the case holds what it names
    assert (X[:, 0] < 0).any() and np.mean(X[:, 1] == 0) > 0.6 and np.unique(X[:, 2]).size < 12 and np.unique(X[:, 3]).tolist() == [2.5]
    assert not X[:, 4].any() and np.count_nonzero(X[:, 5]) == 1 and np.signbit(X[::4, 6]).all() and np.isinf(X[:, 7]).sum() == 5
    assert 0 < np.abs(X[:, 8][X[:, 8] != 0]).min() < 1e-44 and np.unique(X[:, 9]).size == 2 and np.diff(np.unique(X[:, 9]).view(np.int32)) == 1
    got = ranked_exact("f32", genes)
    wp, wU, wfc = (a[:, :, list(genes)] for a in ranked_oracle_slabs("f32"))
    keep = np.broadcast_to(offdiag(counts.size)[:, :, None], wU.shape)
    np.testing.assert_array_equal(got["U"][keep], wU[keep])
    np.testing.assert_allclose(got["p"][keep], wp[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got["fc"][keep], wfc[keep], rtol=1e-12, atol=0.0, equal_nan=True)
    sat = np.mean((wp[keep] == 0.0) | (wp[keep] == 1.0))
    print(f"{sat:.4f} of {keep.sum()} compared p-values are exactly 0 or 1")
    assert sat <= 0.35   # (the constant and the all-zero gene are 2 of 13, the single non-zero nearly so)


def test_walk_restatement_matches_the_oracle_on_integers():
    X, codes, counts = ranked_case("i32")
    assert X.min() < 0 and X.max() > 255
    genes = (0, 1, 2, 3, 4, 5)
    got = ranked_exact("i32", genes)
    wp, wU, wfc = (a[:, :, list(genes)] for a in ranked_oracle_slabs("i32"))
    keep = np.broadcast_to(offdiag(counts.size)[:, :, None], wU.shape)
    np.testing.assert_array_equal(got["U"][keep], wU[keep])
    np.testing.assert_allclose(got["p"][keep], wp[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got["fc"][keep], wfc[keep], rtol=1e-12, atol=0.0, equal_nan=True)


def test_a_gene_of_few_values_gives_the_integers_of_its_histograms():
    """the bridge to the histogram pair route: recoded to 0 .. d - 1, the walk's S2 and tie are those of pair_ints / pairs_numpy"""
    X, codes, counts = ranked_case("f32")
    G = counts.size
    for gene in (TIE_HEAVY, 6, 9, 4):
        rc, d = recode(X[:, gene])
        assert d <= 256
        H, flags = hists_numpy(rc[:, None].astype(np.float64), codes, G)
        assert not flags.any()
        S2, tie = ltx_numpy(X[:, gene], codes, counts, list(range(G)))
        Hl = H.tolist()
        for r in range(G):
            for g in range(G):
                q = pair_ints(Hl, counts, r, g, 0)
                assert (S2[r, g], tie[r, g]) == (q["S2"], q["tie"]), (gene, r, g)
        # and so the statistic of pairs_numpy, bit for bit
        U = pairs_numpy(H, counts)[1][:, :, 0]
        want = np.array([[0.5 * float(2 * int(counts[r]) * int(counts[g]) - S2[r, g]) for g in range(G)] for r in range(G)])
        assert np.array_equal(U, want)


def test_a_subset_of_groups_in_any_order_is_the_same_definition():
    X, codes, counts = ranked_case("f32")
    full = ltx_numpy(X[:, 1], codes, counts, list(range(counts.size)))
    sel = [6, 2, 5]
    sub = ltx_numpy(X[:, 1], codes, counts, sel)
    for a, r in enumerate(sel):
        for b, g in enumerate(sel):
            assert sub[0][a, b] == full[0][r, g] and sub[1][a, b] == full[1][r, g]


def test_the_ranked_entry_points_are_declared_exported_and_built():
    from pathlib import Path
    from illico_amd import _lib
    from illico_amd.csrc import build
    root = Path(__file__).resolve().parent.parent
    header = (root / "include" / "illico_hip_ranked.h").read_text()
    for name in ("illico_pairwise_ranked_dense", "illico_pairwise_ranked_csc"):
        assert name in _lib.RANKED_SIGNATURES and f"int {name}(" in header
        assert hasattr(_lib.load(), name), f"{name} is not exported by the library"
    assert "pairwise_ranked" in build.UNITS and "pairwise_ranked" in build.DEV_UNITS
    assert (root / "illico_amd" / "csrc" / "pairwise_ranked.hip").exists() and (root / "illico_amd" / "csrc" / "kernels_pairwise_ranked.h").exists()
    assert hasattr(_lib.Engine, "pairwise_ranked") and hasattr(_lib.Engine, "pairwise_ranked_sparse")
