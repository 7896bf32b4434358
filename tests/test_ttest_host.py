"""Welch's t-test, host side: argument errors raise before any engine (or GPU) is touched, the C-ABI exports the new entries, and the
float64 formula the device evaluates (restated here in numpy, one IEEE operation per step) agrees with scipy when it is fed exact sums."""
import math

import numpy as np
import pandas as pd
import pytest
from scipy import stats

import illico_amd
from illico_amd import AnnDataLite, differential_expression, welch_ttest
from illico_amd import _lib
from illico_amd import adjust as adjust_mod
from illico_amd import ttest as ttest_mod


def welch_numpy(n1, S1, Q1, n2, S2, Q2, overestim=False):
    """(t, df, m1, v1, m2, v2) as include/illico_hip.h: illico_ttest_from_moments states them -- every step one float64 operation, in
    that order; t is left NaN where the device then writes (0, 1).  n1 / n2 broadcast against the planes."""
    n1, n2 = np.asarray(n1, dtype=np.float64), np.asarray(n2, dtype=np.float64)
    S1, Q1, S2, Q2 = (np.asarray(a, dtype=np.float64) for a in (S1, Q1, S2, Q2))
    with np.errstate(all="ignore"):
        m1, m2 = S1 / n1, S2 / n2
        q1, q2 = Q1 - S1 * m1, Q2 - S2 * m2
        q1, q2 = np.where(q1 < 0, 0.0, q1), np.where(q2 < 0, 0.0, q2)
        v1, v2 = q1 / (n1 - 1), q2 / (n2 - 1)
        n2p = n1 if overestim else n2
        a, b = v1 / n1, v2 / n2p
        t = (m1 - m2) / np.sqrt(a + b)
        df = ((a + b) * (a + b)) / (a * a / (n1 - 1) + b * b / (n2p - 1))
        df = np.where(np.isnan(df), 1.0, df)
    return t, df, m1, v1, m2, v2


def fsum_moments(V, member):
    """(sum, sum of squares) of the float64 values V[member] per column, correctly rounded."""
    A = V[member]
    return (np.array([math.fsum(A[:, j]) for j in range(V.shape[1])]),
            np.array([math.fsum(A[:, j] * A[:, j]) for j in range(V.shape[1])]))


def lognorm_nb(seed, n_cells, n_genes):
    """log-normalised negative-binomial counts, float32"""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.3, 20.0, n_genes)
    C = rng.negative_binomial(2.0, 2.0 / (2.0 + mu), size=(n_cells, n_genes)).astype(np.float64)
    C = C / np.maximum(C.sum(axis=1, keepdims=True), 1.0) * 1e3
    return np.log1p(C).astype(np.float32), rng


@pytest.mark.parametrize("ref", [None, 0])
def test_formula_from_exact_sums_matches_scipy(ref):
    X, rng = lognorm_nb(3, 600, 48)
    codes = rng.integers(0, 5, 600)
    V = X.astype(np.float64)
    n_nan = 0
    for g in range(5):
        if g == ref:
            continue
        own, other = codes == g, (codes != g if ref is None else codes == ref)
        S1, Q1 = fsum_moments(V, own)
        S2, Q2 = fsum_moments(V, other)
        t, df, *_ = welch_numpy(own.sum(), S1, Q1, other.sum(), S2, Q2)
        want = stats.ttest_ind(V[own], V[other], axis=0, equal_var=False)
        ok = ~np.isnan(want.statistic)
        n_nan += int((~ok).sum())
        np.testing.assert_allclose(t[ok], want.statistic[ok], rtol=1e-12, atol=0.0)
        np.testing.assert_allclose(df[ok], want.df[ok], rtol=1e-12, atol=0.0)
    assert n_nan == 0


def test_formula_special_cases():
    # n = 1: 0 / 0; equal constants: 0 / 0; different constants: +-inf; df NaN -> 1
    t, df, *_ = welch_numpy(np.array([1.0, 4.0, 4.0]), np.array([2.0, 8.0, 8.0]), np.array([4.0, 16.0, 16.0]),
                            np.array([5.0, 5.0, 5.0]), np.array([10.0, 10.0, 5.0]), np.array([30.0, 20.0, 5.0]))
    assert np.isnan(t[0]) and np.isnan(t[1]) and t[2] == np.inf
    assert df[1] == 1.0 and df[2] == 1.0
    t, df, *_ = welch_numpy(3.0, 6.0, 14.0, 4.0, 8.0, 30.0, overestim=True)   # {1,2,3} vs sum 8, sumsq 30 of 4 values
    want = stats.ttest_ind_from_stats(2.0, 1.0, 3, 2.0, math.sqrt(14.0 / 3.0), 3, equal_var=False)
    assert t == 0.0 and want.statistic == 0.0
    a, b = 1.0 / 3.0, (14.0 / 3.0) / 3.0                                      # the reference's variance over the GROUP's size
    np.testing.assert_allclose(df, (a + b) ** 2 / (a * a / 2.0 + b * b / 2.0), rtol=1e-14)


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "get_engine", boom)
    monkeypatch.setattr(adjust_mod, "_wilcoxon_planes", boom)
    monkeypatch.setattr(ttest_mod, "ttest_planes", boom)


def _adata():
    return AnnDataLite(np.zeros((4, 3), np.float32), obs=pd.DataFrame({"pert": ["a", "b", "a", "b"]}))


@pytest.mark.parametrize("bad", [
    dict(variant="student"), dict(variant=None), dict(variant=0), dict(alternative="both"), dict(alternative=None),
])
def test_welch_ttest_bad_arguments(no_engine, bad):
    with pytest.raises(ValueError):
        welch_ttest(_adata(), False, "pert", **bad)


@pytest.mark.parametrize("is_log1p", [0, 1, None, "yes"])
def test_welch_ttest_is_log1p_must_be_bool(no_engine, is_log1p):
    with pytest.raises(ValueError):
        welch_ttest(_adata(), is_log1p, "pert")


@pytest.mark.parametrize("bad", [
    dict(method="ttest"), dict(method=None), dict(method="t-test_overestim"), dict(method="t-test", scores=True),
    dict(method="t-test", rank_by="z_score"), dict(method="t-test_overestim_var", rank_by="z_score"), dict(method="t-test", rank_by="t"),
    dict(method="wilcoxon", rank_by="statistic"), dict(rank_by="statistic"), dict(method="t-test", alternative="both"),
    dict(method="t-test", n_genes=0), dict(method="t-test", pts=1), dict(method="t-test", corr_method="holm"),
])
def test_differential_expression_bad_method_arguments(no_engine, bad):
    with pytest.raises(ValueError):
        differential_expression(_adata(), False, "pert", **bad)


@pytest.mark.parametrize("bad", [
    dict(use_continuity=True), dict(use_continuity=False), dict(tie_correct=True), dict(tie_correct=False, use_continuity=True), dict(foo=1),
])
def test_differential_expression_ttest_refuses_wilcoxon_keywords(no_engine, bad):
    with pytest.raises(TypeError):
        differential_expression(_adata(), False, "pert", method="t-test", **bad)


def test_engine_argument_checks_before_the_library():
    eng = _lib.Engine.__new__(_lib.Engine)   # (no context: these checks are host logic)
    eng.n_groups = 2
    S = np.zeros((2, 3))
    with pytest.raises(ValueError):
        eng.ttest_from_moments(S, S, variant="pooled")
    with pytest.raises(ValueError):
        eng.ttest_from_moments(S, S, alternative="both")
    with pytest.raises(ValueError):
        eng.ttest_from_moments(S, S, want=("p", "z"))
    with pytest.raises(ValueError):
        eng.ttest_from_moments(S, S, want=())
    with pytest.raises(ValueError):
        eng.ttest_from_moments(S, None)
    with pytest.raises(ValueError):
        eng.ttest_from_moments(S, np.zeros((2, 4)))
    with pytest.raises(ValueError):
        eng.ttest_from_moments(np.zeros((3, 3)), np.zeros((3, 3)))       # rows != groups
    with pytest.raises(ValueError):
        eng.ttest_from_moments(S, S, out=(np.zeros((2, 3)),))            # two planes wanted, one given
    with pytest.raises(ValueError):
        eng.student_t_pvalues(np.zeros(3), np.ones(4))
    with pytest.raises(ValueError):
        eng.student_t_pvalues(np.zeros(3), np.ones(3), alternative="both")
    with pytest.raises(ValueError):
        eng._gs_outputs((np.zeros((2, 3)),) * 3, 2, 3, True, False, eng._GM_KINDS, eng._GM_NAMES)
    with pytest.raises(ValueError):
        eng._gs_outputs((np.zeros((2, 3), np.int64), np.zeros((2, 3))), 2, 3, False, False, eng._GM_KINDS, eng._GM_NAMES)


def test_new_symbols_are_exported():
    from conftest import ROOT
    header = (ROOT / "include" / "illico_hip.h").read_text()
    for name in ("illico_group_moments_dense", "illico_group_moments_csc", "illico_group_moments_csr", "illico_group_moments_bound",
                 "illico_ttest_from_moments", "illico_student_t_pvalues"):
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert hasattr(_lib.load(), name)
    assert "ILLICO_TT_WELCH = 0" in header and "ILLICO_TT_OVERESTIM_VAR = 1" in header
    assert (_lib.TT_WELCH, _lib.TT_OVERESTIM_VAR) == (0, 1)
    assert "welch_ttest" in illico_amd.__all__
    assert adjust_mod.RANK_BY_TTEST == ("p_value", "statistic") and set(adjust_mod.DE_METHODS) == {"wilcoxon", "t-test", "t-test_overestim_var"}
    from illico_amd.csrc import build
    assert "group_moments" in build.UNITS and "group_moments" in build.DEV_UNITS
