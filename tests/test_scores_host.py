"""z-score plane / top_by_score: argument errors raise before any engine (or GPU) is touched; the C-ABI exports the new entries."""
import numpy as np
import pandas as pd
import pytest

import illico_amd
from illico_amd import AnnDataLite, differential_expression, top_by_score
from illico_amd import _lib
from illico_amd import adjust as adjust_mod


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "get_engine", boom)
    monkeypatch.setattr(adjust_mod, "_wilcoxon_planes", boom)


@pytest.mark.parametrize("bad", [
    dict(rank_by="foo"), dict(rank_by=None), dict(rank_by="z"), dict(scores=1), dict(scores="yes"), dict(scores=None),
])
def test_differential_expression_bad_score_arguments(no_engine, bad):
    adata = AnnDataLite(np.zeros((4, 3), np.float32), obs=pd.DataFrame({"pert": ["a", "b", "a", "b"]}))
    with pytest.raises(ValueError):
        differential_expression(adata, False, "pert", **bad)


@pytest.mark.parametrize("x,n", [
    (np.zeros((3, 10), np.float32), 2), (np.zeros(10), 2), (np.zeros((2, 3, 4)), 1), ([[0.5, 0.5]], 1),
    (np.zeros((3, 10)), 11), (np.zeros((3, 10)), -1), (np.zeros((3, 10)), 2.0), (np.zeros((3, 10)), True),
])
def test_top_by_score_bad_arguments(no_engine, x, n):
    with pytest.raises(ValueError):
        top_by_score(x, n)


def test_engine_refuses_a_bad_plane_count_before_the_library():
    eng = _lib.Engine.__new__(_lib.Engine)   # (no context: _outputs is host logic)
    with pytest.raises(ValueError):
        eng._outputs((np.zeros((2, 3)),) * 2, 2, 3, False)
    with pytest.raises(ValueError):
        eng._outputs((np.zeros((2, 3)),) * 3, 2, 3, False, scores=True)
    with pytest.raises(ValueError):
        eng._outputs(None, 2, 3, False, scores="yes")
    planes = eng._outputs(None, 2, 3, False, scores=True)[0]
    assert len(planes) == 4 and all(p.shape == (2, 3) and p.dtype == np.float64 for p in planes)


def test_new_symbols_are_exported():
    from conftest import ROOT
    header = (ROOT / "include" / "illico_hip.h").read_text()
    for name in ("illico_run_dense_ex", "illico_run_csc_ex", "illico_run_csr_ex", "illico_run_bound_ex", "illico_top_by_score"):
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert hasattr(_lib.load(), name)
    assert "top_by_score" in illico_amd.__all__
    assert adjust_mod.RANK_BY == ("p_value", "z_score")
