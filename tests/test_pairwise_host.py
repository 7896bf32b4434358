"""All-pairs Wilcoxon tests from per-(group, gene) value histograms: the arithmetic of include/illico_hip.h
(illico_pairwise_from_hists) restated in float64 numpy and held to the CPU oracle run once per reference, plus the argument
validation of pairwise_wilcoxon that needs no device.  tests/test_gpu_pairwise.py imports the cases and the restatement."""
import functools

import numpy as np
import pandas as pd
import pytest
from scipy import special

import oracle
from conftest import make_counts

HIST_VALUES = 256
#: genes of case A that hold a value which is no integer in [0, 255]
CASE_A_FLAGGED = (7, 9, 11)


def _codes(sizes, seed):
    return np.random.RandomState(seed).permutation(np.repeat(np.arange(len(sizes)), sizes))


@functools.lru_cache(maxsize=None)
def case(name):
    """(X float32 [N, M], codes int64 [N], counts int64 [G]).  The arrays are shared: do not write to them."""
    if name == "A":  # every cell width and tile edge: sizes around 64 and 256, two full gene tiles and a ragged one
        sizes = (1, 2, 63, 255, 256, 257, 1024, 742)
        codes = _codes(sizes, 131)
        X, rng = make_counts(31, 2600, 130, 0.7)
        X[:, 3] = 0                                                  # constant: p = 1, z = 0
        X[:, 5] = rng.randint(253, 256, size=2600)                   # the table's last values ...
        X[codes == 4, 5] = 255                                       # ... and a multiplicity equal to the group's size (256)
        X[:, 7] = rng.randint(254, 257, size=2600)                   # 256: flagged
        X[::7, 9] += 0.5                                             # fractional: flagged
        X[::11, 11] = -1                                             # negative: flagged
    elif name == "B":  # one histogram cell passes 65535
        sizes = (66000, 300, 5)
        codes = _codes(sizes, 132)
        X = np.random.RandomState(32).poisson(3.0, size=(sum(sizes), 4)).astype(np.float32)
        X[codes == 0, 0] = 2
    elif name == "C":  # group counts beyond 64 and 128, a ragged last block of references
        sizes = (10,) * 130
        codes = _codes(sizes, 133)
        X, _ = make_counts(9, 1300, 70, 0.7)
    else:
        raise KeyError(name)
    for a in (X, codes):
        a.setflags(write=False)
    return X, codes.astype(np.int64), np.asarray(sizes, dtype=np.int64)


def labels_of(codes):
    """string labels whose np.unique order is the order of the codes"""
    return np.array([f"g{c:03d}" for c in codes])


def groups_of(codes, ref=None):
    lab = labels_of(codes)
    return oracle.encode_and_count_groups(lab, None if ref is None else f"g{ref:03d}")[1]


@functools.lru_cache(maxsize=None)
def oracle_slabs(name, is_log1p=False, use_continuity=True, tie_correct=True, alternative="two-sided"):
    """(p, U, fc) float64 [G, G, M]: slab r = oracle.run with reference r"""
    X, codes, counts = case(name)
    out = [oracle.run(np.ascontiguousarray(X), groups_of(codes, r), is_log1p=is_log1p, use_continuity=use_continuity, tie_correct=tie_correct,
                      alternative=alternative) for r in range(counts.size)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def hists_numpy(X, codes, G):
    """(H int64 [G, M, 256], flags bool [M]): np.add.at counts of the values 0 .. 255; H of a flagged gene counts its valid values only"""
    V = np.asarray(X, dtype=np.float64)
    N, M = V.shape
    ok = (V == np.floor(V)) & (V >= 0) & (V <= HIST_VALUES - 1)
    H = np.zeros((G, M, HIST_VALUES), dtype=np.int64)
    r, c = np.nonzero(ok)
    np.add.at(H, (codes[r], c, V[r, c].astype(np.int64)), 1)
    return H, ~ok.all(axis=0)


def pairs_numpy(H, counts, *, use_continuity=True, tie_correct=True, alternative="two-sided"):
    """(p, U, fc, z) float64 [G, G, M] indexed [r, g, gene], from the histograms alone: the block of include/illico_hip.h."""
    H = np.asarray(H, dtype=np.int64)
    G, M, R = H.shape
    n = np.asarray(counts, dtype=np.int64)
    cum = np.concatenate([np.zeros((G, M, 1), dtype=np.int64), np.cumsum(H, axis=2)], axis=2)
    S = (H * np.arange(R, dtype=np.int64)).sum(axis=2)                       # exact value sums
    p, U, fc, z = (np.empty((G, G, M), dtype=np.float64) for _ in range(4))
    cc = 0.5 if use_continuity else 0.0
    for r in range(G):
        n_r, n_g = n[r], n[:, None]
        S2 = (H * (cum[r, :, :-1] + cum[r, :, 1:])[None]).sum(axis=2)        # [G, M]
        u = 0.5 * (2 * n_r * n_g - S2).astype(np.float64)
        t = H + H[r][None]
        tie = (t ** 3 - t).sum(axis=2).astype(np.float64) if tie_correct else np.zeros((G, M))
        nn = n_r + n_g
        nnn = (nn * (nn - 1) * (nn + 1)).astype(np.float64)
        var0 = (n_r * n_g * (nn + 1)).astype(np.float64) / 12.0
        n12 = (n_r * n_g).astype(np.float64)
        mu = n12 / 2.0
        tie_corr = 1.0 - tie / nnn
        live = tie_corr > 1.0e-9
        with np.errstate(invalid="ignore", divide="ignore"):
            sigma = np.sqrt(var0 * tie_corr)
            if alternative == "two-sided":
                delta = np.minimum(u, n12 - u) - mu
                pv = special.erfc(((np.abs(delta) + np.sign(delta) * cc) / sigma) / np.sqrt(2.0))
            elif alternative == "greater":
                pv = 0.5 * special.erfc((((u - mu) - cc) / sigma) / np.sqrt(2.0))
            elif alternative == "less":
                pv = 0.5 * special.erfc(-(((u - mu) + cc) / sigma) / np.sqrt(2.0))
            else:
                raise ValueError(alternative)
            zz = (mu - u) / sigma
            mu_ref = S[r].astype(np.float64) / float(n_r)
            f = (S.astype(np.float64) / n_g.astype(np.float64)) / mu_ref[None]
        p[r] = np.where(live, pv, 1.0)
        z[r] = np.where(live, zz, 0.0)
        U[r] = u
        fc[r] = np.where(mu_ref[None] == 0.0, np.inf, f)
        p[r, r], z[r, r] = 1.0, 0.0
    return p, U, fc, z


def offdiag(G):
    return ~np.eye(G, dtype=bool)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_restatement_matches_the_oracle_for_every_reference(name):
    X, codes, counts = case(name)
    G = counts.size
    H, flags = hists_numpy(X, codes, G)
    assert np.array_equal(np.flatnonzero(flags), CASE_A_FLAGGED if name == "A" else [])
    p, U, fc, z = pairs_numpy(H, counts)
    wp, wU, wfc = oracle_slabs(name)
    keep = offdiag(G)[:, :, None] & ~flags[None, None, :]
    np.testing.assert_array_equal(U[keep], wU[keep])
    np.testing.assert_allclose(p[keep], wp[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(fc[keep], wfc[keep], rtol=1e-12, atol=0.0)
    # the inputs' own condition: the p-values are mostly informative, not saturated at 0 or 1
    sat = np.mean((wp[keep] == 0.0) | (wp[keep] == 1.0))
    print(f"case {name}: {sat:.4f} of {keep.sum()} compared p-values are exactly 0 or 1")
    assert sat <= 0.20
    # antisymmetry of the definition itself
    U, z = U[:, :, ~flags], z[:, :, ~flags]
    nn = counts[:, None] * counts[None, :]
    assert np.array_equal(U + U.transpose(1, 0, 2), np.broadcast_to(nn[:, :, None].astype(np.float64), U.shape))
    assert np.array_equal(z, -z.transpose(1, 0, 2))
    assert np.array_equal(np.diagonal(U, axis1=0, axis2=1).T, np.broadcast_to((counts ** 2 / 2.0)[:, None], U.shape[1:]))


def test_restatement_less_and_greater_mirror_each_other():
    X, codes, counts = case("A")
    H, flags = hists_numpy(X, codes, counts.size)
    less = pairs_numpy(H, counts, alternative="less")[0]
    greater = pairs_numpy(H, counts, alternative="greater")[0]
    keep = offdiag(counts.size)[:, :, None] & ~flags[None, None, :]
    assert np.array_equal(less[keep], greater.transpose(1, 0, 2)[keep])


# ---- argument validation of pairwise_wilcoxon: raised before any device work ----
def _adata():
    from illico_amd import AnnDataLite
    X = np.arange(24, dtype=np.float32).reshape(6, 4) % 5
    return AnnDataLite(X, obs=pd.DataFrame({"g": ["a", "a", "b", "b", "c", "c"]}))


@pytest.mark.parametrize("kw, match", [
    (dict(groups=["a", "zz"]), "not present"),
    (dict(groups=["a"]), "at least two"),
    (dict(groups=["a", "a", "b"]), "twice"),
    (dict(groups="ab"), "sequence of labels"),
    (dict(alternative="both"), "Unsupported alternative"),
    (dict(scores=1), "scores must be a bool"),
    (dict(corr_method="holm"), "correction method"),
    (dict(max_result_bytes=-1), "max_result_bytes"),
])
def test_pairwise_wilcoxon_refuses_bad_arguments(kw, match):
    from illico_amd import pairwise_wilcoxon
    with pytest.raises(ValueError, match=match):
        pairwise_wilcoxon(_adata(), False, "g", **kw)


def test_pairwise_wilcoxon_refuses_a_non_bool_is_log1p():
    from illico_amd import pairwise_wilcoxon
    with pytest.raises(ValueError, match="is_log1p must be a bool"):
        pairwise_wilcoxon(_adata(), 1, "g")


def test_pairwise_wilcoxon_refuses_a_result_beyond_max_result_bytes():
    from illico_amd import pairwise_wilcoxon
    with pytest.raises(ValueError, match=r"max_result_bytes = 1\b"):
        pairwise_wilcoxon(_adata(), False, "g", max_result_bytes=1)
    # 3 x 2 pairs x 4 genes x 8 bytes x 3 columns = 576 bytes; a fourth column with scores
    with pytest.raises(ValueError, match="768 bytes"):
        pairwise_wilcoxon(_adata(), False, "g", scores=True, max_result_bytes=767)


def test_the_entry_points_are_declared_exported_and_built():
    from pathlib import Path
    from illico_amd import _lib
    from illico_amd.csrc import build
    root = Path(__file__).resolve().parent.parent
    header = (root / "include" / "illico_hip.h").read_text()
    for name in ("illico_group_value_hists_dense", "illico_group_value_hists_csc", "illico_group_value_hists_csr", "illico_pairwise_from_hists"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    assert "pairwise" in build.UNITS and "pairwise" in build.DEV_UNITS
    assert (root / "illico_amd" / "csrc" / "pairwise.hip").exists()
