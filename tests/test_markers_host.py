"""CPU-only tests of the marker combination: the numpy model (tests/markers_model.py) on hand-computed cases, the build and export of
illico_combine_pairs, and the argument errors of pairwise_markers, raised before any device work."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from markers_model import METHODS, combine_model, default_rank

ROOT = Path(__file__).resolve().parent.parent


def _plane(K, cols):
    """[K, K, W] from {(r, g): [p per column]}; everything else (the diagonal included) NaN: reading it would poison the result."""
    W = len(next(iter(cols.values())))
    P = np.full((K, K, W), np.nan)
    for (r, g), v in cols.items():
        P[r, g] = v
    return P


# ---- the model, by hand ----
def test_two_groups_return_the_single_p():
    P = _plane(2, {(1, 0): [0.25, 0.0, 1.0], (0, 1): [0.5, 1e-300, 5e-324]})
    E = np.arange(12, dtype=np.float64).reshape(2, 2, 3)
    for method in METHODS:
        p, rep, e = combine_model(P, (E,), method=method)
        assert np.array_equal(p, [[0.25, 0.0, 1.0], [0.5, 1e-300, 5e-324]])
        assert np.array_equal(rep, [[1, 1, 1], [0, 0, 0]]) and rep.dtype == np.int32
        assert np.array_equal(e, [E[1, 0], E[0, 1]])


def test_three_groups_by_hand():
    # group 0 against references 1 and 2: p = (0.04, 0.01); group 1 against 0 and 2: a tie (0.5, 0.5); group 2: (0.3, 0.9)
    P = _plane(3, {(1, 0): [0.04], (2, 0): [0.01], (0, 1): [0.5], (2, 1): [0.5], (0, 2): [0.3], (1, 2): [0.9]})
    p, rep = combine_model(P, method="all")
    assert np.array_equal(p[:, 0], [0.04, 0.5, 0.9]) and np.array_equal(rep[:, 0], [1, 2, 1])   # the tie: the later reference has rank n
    p, rep = combine_model(P, method="any")
    assert np.array_equal(p[:, 0], [min(0.01 * 2.0 / 1.0, 0.04 * 2.0 / 2.0), 0.5, min(0.3 * 2.0, 0.9)])
    assert np.array_equal(rep[:, 0], [2, 0, 0])                                                # the tie: the earlier reference has rank 1
    p, rep = combine_model(P, method="some", rank=1)
    assert np.array_equal(p[:, 0], [0.02, 1.0, 0.6]) and np.array_equal(rep[:, 0], [2, 0, 0])
    p, rep = combine_model(P, method="some", rank=2)
    assert np.array_equal(p[:, 0], [max(0.02, 0.04), 1.0, 0.9]) and np.array_equal(rep[:, 0], [1, 2, 1])
    assert default_rank(2) == 1 and default_rank(3) == 2 and default_rank(63) == 32 and default_rank(5, 1.0) == 5 and default_rank(9, 0.01) == 1


def test_the_diagonal_is_never_read_and_effects_are_selected():
    rng = np.random.default_rng(0)
    K, W = 5, 9
    P = rng.random((K, K, W))
    E = rng.normal(size=(K, K, W))
    Q = P.copy()
    Q[np.arange(K), np.arange(K)] = np.nan
    for method in METHODS:
        a, b = combine_model(P, (E,), method=method), combine_model(Q, (E,), method=method)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        p, rep, e = a
        g, j = np.meshgrid(np.arange(K), np.arange(W), indexing="ij")
        assert (rep != g).all() and np.array_equal(e, E[rep, g, j])


@pytest.mark.parametrize("K", [3, 4, 7, 33])
def test_some_at_its_two_ends_and_simes_bounds(K):
    rng = np.random.default_rng(K)
    n, W = K - 1, 40
    P = rng.random((K, K, W)) ** 3
    P[:, :, :8] = rng.choice([0.0, 5e-324, 1e-300, 0.5, 1.0], size=(K, K, 8))
    off = ~np.eye(K, dtype=bool)
    srt = np.stack([np.sort(P[off[:, g], g, :], axis=0) for g in range(K)])        # [g, i, j]
    p1 = srt[:, 0, :]
    p, _ = combine_model(P, method="some", rank=1)
    assert np.array_equal(p, np.minimum(1.0, float(n) * p1))
    p, rep = combine_model(P, method="some", rank=n)
    holm = np.minimum(1.0, (srt * (float(n) - np.arange(1, n + 1, dtype=np.float64)[None, :, None] + 1.0)).max(axis=1))
    assert np.array_equal(p, holm)
    assert np.array_equal(rep, combine_model(P, method="all")[1])                   # rank n: the same representative
    p, _ = combine_model(P, method="any")
    assert (p >= p1).all() and (p <= float(n) * p1).all()
    p, _ = combine_model(P, method="all")
    assert np.array_equal(p, srt[:, n - 1, :])


def test_the_rank_counting_form_gives_the_same_bits():
    """What the kernel does: the term at each reference's stable rank, folded with min / max in reference order."""
    rng = np.random.default_rng(5)
    for K in (2, 3, 6, 17):
        n = K - 1
        P = rng.choice([0.0, 5e-324, 1e-300, 0.5, 1.0, 0.3, 1e-9], size=(K, K, 30))
        j_star = default_rank(n)
        want_any, want_some = combine_model(P, method="any")[0], combine_model(P, method="some", rank=j_star)[0]
        for g in range(K):
            refs = [r for r in range(K) if r != g]
            for j in range(P.shape[2]):
                v = [P[r, g, j] for r in refs]
                rank = [1 + sum(1 for t in range(n) if v[t] < v[s] or (v[t] == v[s] and t < s)) for s in range(n)]
                assert min(v[s] * float(n) / float(rank[s]) for s in range(n)) == want_any[g, j]
                assert min(1.0, max(v[s] * (float(n) - float(rank[s]) + 1.0) for s in range(n) if rank[s] <= j_star)) == want_some[g, j]


# ---- build and export ----
def test_the_entry_point_is_declared_exported_and_built():
    from illico_amd import _lib
    from illico_amd.csrc import build
    header = (ROOT / "include" / "illico_hip_markers.h").read_text()
    assert "int illico_combine_pairs(" in header
    assert "illico_combine_pairs" not in (ROOT / "include" / "illico_hip.h").read_text()
    assert "illico_combine_pairs" in _lib.MARKER_SIGNATURES and "illico_combine_pairs" not in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "illico_combine_pairs") and lib.illico_combine_pairs.argtypes == _lib.MARKER_SIGNATURES["illico_combine_pairs"][0]
    assert "markers" in build.UNITS and "markers" in build.DEV_UNITS
    assert (ROOT / "illico_amd" / "csrc" / "markers.hip").exists() and (ROOT / "illico_amd" / "csrc" / "kernels_markers.h").exists()
    import illico_amd
    assert "pairwise_markers" in illico_amd.__all__
    assert _lib.COMBINE_METHODS == {"all": 0, "any": 1, "some": 2}
    for name, code in (("ILLICO_COMBINE_ALL", 0), ("ILLICO_COMBINE_ANY", 1), ("ILLICO_COMBINE_SOME", 2), ("ILLICO_COMBINE_MAX_GROUPS", 256)):
        assert f"#define {name} {code}" in header


def test_the_rank_handed_to_the_library():
    from illico_amd._lib import combine_rank
    assert combine_rank(63, "some", None, 0.5) == 32 and combine_rank(2, "some", None, 0.5) == 1 and combine_rank(4, "some", None, 1) == 4
    assert combine_rank(63, "some", 7, 0.5) == 7 and combine_rank(63, "any", 7, 0.5) == 1 and combine_rank(63, "all", None, 0.5) == 1
    assert [combine_rank(n, "some", None, 0.5) for n in range(1, 9)] == [default_rank(n) for n in range(1, 9)]
    for bad in (dict(method="top"), dict(method=None), dict(min_prop=0), dict(min_prop=1.5), dict(min_prop="half"), dict(min_prop=True),
                dict(rank=1.5), dict(rank=True)):
        kw = dict(method="some", rank=None, min_prop=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            combine_rank(5, kw["method"], kw["rank"], kw["min_prop"])


# ---- argument validation of pairwise_markers: raised before any device work ----
def _adata():
    from illico_amd import AnnDataLite
    X = np.arange(24, dtype=np.float32).reshape(6, 4) % 5
    return AnnDataLite(X, obs=pd.DataFrame({"g": ["a", "a", "b", "b", "c", "c"]}))


@pytest.mark.parametrize("kw, match", [
    (dict(pval_type="top"), "pval_type"),
    (dict(pval_type=None), "pval_type"),
    (dict(min_prop=0), "min_prop"),
    (dict(min_prop=1.01), "min_prop"),
    (dict(min_prop="0.5"), "min_prop"),
    (dict(n_genes=0), "n_genes"),
    (dict(n_genes=2.0), "n_genes"),
    (dict(groups=["a", "zz"]), "not present"),
    (dict(groups=["a"]), "at least two"),
    (dict(groups=["a", "a", "b"]), "twice"),
    (dict(groups="ab"), "sequence of labels"),
    (dict(alternative="both"), "Unsupported alternative"),
    (dict(use_continuity=1), "use_continuity must be a bool"),
    (dict(corr_method="holm"), "correction method"),
])
def test_pairwise_markers_refuses_bad_arguments(kw, match):
    from illico_amd import pairwise_markers
    with pytest.raises(ValueError, match=match):
        pairwise_markers(_adata(), False, "g", **kw)


def test_pairwise_markers_refuses_a_non_bool_is_log1p():
    from illico_amd import pairwise_markers
    with pytest.raises(ValueError, match="is_log1p must be a bool"):
        pairwise_markers(_adata(), 1, "g")
