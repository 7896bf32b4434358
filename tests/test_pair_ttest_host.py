"""All-pairs Welch t-tests, host side: the numpy model of every ordered pair (tests/pair_ttest_model.py) agrees with scipy when it is
fed exact sums, has the special cases and the symmetry the device relies on, argument errors raise before any engine (or GPU) is
touched, and the C-ABI exports the new entry."""
import sys

import numpy as np
import pandas as pd
import pytest
from scipy import stats

import illico_amd
from illico_amd import AnnDataLite, pairwise_markers, pairwise_ttest
from illico_amd import _lib
from illico_amd import pairwise as pairwise_mod
from pair_ttest_model import pair_model
from test_ttest_host import fsum_moments, lognorm_nb

pt_mod = sys.modules["illico_amd.pairwise_ttest"]   # (the package's attribute of that name is the function)


def _exact_planes(seed=5, n_cells=400, n_genes=24, G=5):
    X, rng = lognorm_nb(seed, n_cells, n_genes)
    codes = rng.integers(0, G, n_cells)
    V = X.astype(np.float64)
    S, Q = (np.stack(a) for a in zip(*[fsum_moments(V, codes == g) for g in range(G)]))
    return V, codes, S, Q, np.bincount(codes, minlength=G)


def test_model_from_exact_sums_matches_scipy():
    """t and df against scipy's Welch formula on the same exact moments (rtol 1e-13: a square root and its square apart); p by
    scipy's tail at the model's (t, df); Cohen's d and the fold change against the data's own means and variances."""
    V, codes, S, Q, counts = _exact_planes()
    G = len(counts)
    M = pair_model(S, Q, counts)
    n = counts[:, None].astype(np.float64)
    mean = S / n
    std = np.sqrt((Q - S * mean) / (n - 1.0))
    eps = np.finfo(np.float64).eps
    for r in range(G):
        for g in range(G):
            if r == g:
                continue
            want = stats.ttest_ind_from_stats(mean[g], std[g], counts[g], mean[r], std[r], counts[r], equal_var=False)
            a, b = V[codes == g], V[codes == r]
            direct = stats.ttest_ind(a, b, axis=0, equal_var=False)
            np.testing.assert_allclose(M["t"][r, g], want.statistic, rtol=1e-13, atol=0.0)
            np.testing.assert_allclose(M["df"][r, g], direct.df, rtol=1e-13, atol=0.0)
            np.testing.assert_allclose(2.0 * stats.t.sf(np.abs(M["t"][r, g]), M["df"][r, g]), want.pvalue, rtol=1e-12, atol=0.0)
            # the data's own (pairwise-summed) means carry a few eps each: the difference of two means that much absolutely
            sd = np.sqrt(0.5 * (a.var(axis=0, ddof=1) + b.var(axis=0, ddof=1)))
            d = (a.mean(axis=0) - b.mean(axis=0)) / sd
            assert (np.abs(M["cohen_d"][r, g] - d) <= 1e-12 * np.abs(d) + 64 * eps * (np.abs(mean[g]) + np.abs(mean[r])) / sd).all()
            np.testing.assert_allclose(M["fold_change"][r, g], a.mean(axis=0) / b.mean(axis=0), rtol=1e-13)


def test_model_special_cases():
    # groups: 0 = one cell (2); 1 = four cells, constant 2; 2 = five cells, constant 2; 3 = five cells, constant 1; 4 = {1, 2, 3}
    counts = np.array([1, 4, 5, 5, 3])
    S = np.array([[2.0], [8.0], [10.0], [5.0], [6.0]])
    Q = np.array([[4.0], [16.0], [20.0], [5.0], [14.0]])
    M = pair_model(S, Q, counts)
    t, raw, df = M["t"][:, :, 0], M["t_raw"][:, :, 0], M["df"][:, :, 0]
    assert np.isnan(raw[0, :]).all() and np.isnan(raw[:, 0]).all() and (t[0, :] == 0).all() and (t[:, 0] == 0).all()   # a one-cell side
    assert np.isnan(raw[1, 2]) and t[1, 2] == 0.0 and df[1, 2] == 1.0          # no variance on either side, equal means: (0, 1)
    assert raw[3, 2] == np.inf and raw[2, 3] == -np.inf and t[3, 2] == np.inf  # ... different means: +-inf, kept
    assert df[3, 2] == 1.0
    assert (np.diagonal(t) == 0).all() and (np.diagonal(M["cohen_d"][:, :, 0]) == 0).all()
    assert np.isfinite(raw[4, 1]) and raw[4, 1] == 0.0                         # equal means, variance on one side: a true zero
    assert M["cohen_d"][1, 2, 0] == 0.0 and M["cohen_d"][3, 2, 0] == np.inf    # NaN -> 0, inf kept
    assert M["fold_change"][3, 2, 0] == 2.0
    Z = pair_model(np.array([[0.0], [3.0]]), np.array([[0.0], [5.0]]), np.array([2, 3]))
    assert Z["fold_change"][0, 1, 0] == np.inf and Z["fold_change"][0, 0, 0] == np.inf and Z["fold_change"][1, 0, 0] == 0.0
    F = pair_model(S, Q, counts, fsum=2.0 * S)
    assert np.array_equal(F["fold_change"], M["fold_change"]) and np.array_equal(F["t"], M["t"])
    # the selection: a subset's planes are the sub-planes
    sub = pair_model(S, Q, counts, sel=[1, 3, 4])
    assert np.array_equal(sub["t"], M["t"][np.ix_([1, 3, 4], [1, 3, 4])])


def test_welch_is_antisymmetric_in_t_and_symmetric_in_df_bit_for_bit():
    """What lets the device evaluate the tail once per unordered pair; overestim_var has neither property."""
    _, _, S, Q, counts = _exact_planes(seed=9, n_genes=64)
    S[:, 3], Q[:, 3] = counts * 2.0, counts * 4.0      # a constant gene
    M = pair_model(S, Q, counts)
    tr, sw = M["t_raw"], np.swapaxes(M["t_raw"], 0, 1)
    assert np.array_equal(np.isnan(tr), np.isnan(sw)) and np.isnan(tr[:, :, 3]).all()
    nz = ~np.isnan(tr) & (tr != 0)
    assert nz.sum() > 1000 and np.array_equal((-tr)[nz].view(np.uint64), sw[nz].view(np.uint64))
    assert (sw[tr == 0] == 0).all()                     # equal means: +0 on both sides (x - x is +0), not -0
    assert np.array_equal(M["df"].view(np.uint64), np.swapaxes(M["df"], 0, 1).view(np.uint64))
    assert np.array_equal(M["cohen_d"][nz].view(np.uint64), (-np.swapaxes(M["cohen_d"], 0, 1))[nz].view(np.uint64))
    O = pair_model(S, Q, counts, overestim=True)
    assert not np.array_equal(O["df"], np.swapaxes(O["df"], 0, 1))


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "get_engine", boom)
    monkeypatch.setattr(pt_mod, "pair_ttest_blocks", boom)
    monkeypatch.setattr(pairwise_mod, "pairwise_planes", boom)


def _adata():
    return AnnDataLite(np.zeros((6, 3), np.float32), obs=pd.DataFrame({"pert": ["a", "b", "c", "a", "b", "c"]}))


@pytest.mark.parametrize("bad", [
    dict(variant="student"), dict(variant=None), dict(alternative="both"), dict(alternative=None), dict(corr_method="holm"),
    dict(groups=["a"]), dict(groups=["a", "z"]), dict(groups=["a", "a", "b"]), dict(groups="a"), dict(max_result_bytes=-1),
    dict(max_result_bytes=True), dict(max_result_bytes=100),
])
def test_pairwise_ttest_bad_arguments(no_engine, bad):
    with pytest.raises(ValueError):
        pairwise_ttest(_adata(), False, "pert", **bad)


@pytest.mark.parametrize("is_log1p", [0, 1, None, "yes"])
def test_pairwise_ttest_is_log1p_must_be_bool(no_engine, is_log1p):
    with pytest.raises(ValueError):
        pairwise_ttest(_adata(), is_log1p, "pert")


def test_pairwise_ttest_refuses_wilcoxon_keywords(no_engine):
    for bad in (dict(use_continuity=True), dict(tie_correct=False), dict(scores=True)):
        with pytest.raises(TypeError):
            pairwise_ttest(_adata(), False, "pert", **bad)


@pytest.mark.parametrize("bad", [
    dict(method="ttest"), dict(method=None), dict(method="t-test_overestim"), dict(method="welch"),
    dict(method="t-test", use_continuity=False), dict(method="t-test", tie_correct=False), dict(method="t-test_overestim_var", use_continuity=False),
    dict(method="t-test", pval_type="most"), dict(method="t-test", min_prop=0.0), dict(method="t-test", n_genes=0),
    dict(method="t-test", alternative="both"), dict(method="t-test", corr_method="holm"), dict(method="t-test", groups=["a"]),
])
def test_pairwise_markers_bad_method_arguments(no_engine, bad):
    with pytest.raises(ValueError):
        pairwise_markers(_adata(), False, "pert", **bad)


def test_engine_argument_checks_before_the_library():
    eng = _lib.Engine.__new__(_lib.Engine)   # (no context: these checks are host logic)
    eng.n_groups = 3
    S = np.zeros((3, 4))
    for bad in (dict(variant="pooled"), dict(alternative="both"), dict(want=("p", "z")), dict(want=()), dict(want=("p", "p")),
                dict(sel=[0]), dict(sel=[]), dict(sel=[1, 0]), dict(sel=[0, 0]), dict(sel=[0, 3]), dict(sel=[-1, 1]), dict(sel=[0.0, 1.0]),
                dict(fsum=np.zeros((3, 5))), dict(out=(np.zeros((3, 3, 4)),)), dict(want=("p",), out=(np.zeros((3, 3, 5)),)),
                dict(want=("p",), out=(np.zeros((2, 2, 4)),)), dict(want=("p",), out=(np.zeros((3, 3, 4), np.float32),)),
                dict(want=("p",), sel=[0, 2], out=(np.zeros((3, 3, 4)),))):
        with pytest.raises(ValueError):
            eng.pair_ttest_from_moments(S, S, **bad)
    with pytest.raises(ValueError):
        eng.pair_ttest_from_moments(S, None)
    with pytest.raises(ValueError):
        eng.pair_ttest_from_moments(S, np.zeros((3, 5)))
    with pytest.raises(ValueError):
        eng.pair_ttest_from_moments(np.zeros((4, 4)), np.zeros((4, 4)))      # rows != groups
    ro = np.zeros((3, 3, 4))
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        eng.pair_ttest_from_moments(S, S, want=("p",), out=(ro,))


def test_new_symbols_are_exported():
    from conftest import ROOT
    header = (ROOT / "include" / "illico_hip_pair_ttest.h").read_text()
    name = "illico_pair_ttest_from_moments"
    assert f"int {name}(" in header and name in _lib.PAIR_TTEST_SIGNATURES and name not in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.PAIR_TTEST_SIGNATURES[name][0]
    assert len(_lib.PAIR_TTEST_SIGNATURES[name][0]) == 17
    assert _lib.PAIR_TT_OUTPUTS == ("p", "t", "df", "fold_change", "cohen_d")
    kernel = (ROOT / "illico_amd" / "csrc" / "kernels_pair_ttest.h").read_text()
    assert f"#define PT_TILE {_lib.PAIR_TT_GENE_TILE} " in kernel and f"#define PT_GT {_lib.PAIR_TT_GROUP_TILE} " in kernel
    assert "pairwise_ttest" in illico_amd.__all__ and "pairwise_markers" in illico_amd.__all__
    assert set(pairwise_mod.MARKER_METHODS) == {"wilcoxon", "t-test", "t-test_overestim_var"}
    from illico_amd.csrc import build
    assert "pair_ttest" in build.UNITS and "pair_ttest" in build.DEV_UNITS
