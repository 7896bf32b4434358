"""adjust_pvalues / differential_expression: argument errors raise before any engine (or GPU) is touched."""
import numpy as np
import pandas as pd
import pytest

import illico_amd
from illico_amd import AnnDataLite, adjust_pvalues, differential_expression
from illico_amd import _lib
from illico_amd import adjust as adjust_mod


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "get_engine", boom)
    monkeypatch.setattr(adjust_mod, "_wilcoxon_planes", boom)


@pytest.mark.parametrize("bad", [
    dict(method="holm"), dict(method=None), dict(method=3), dict(n_top=-1), dict(n_top=11), dict(n_top=2.0), dict(n_top=True),
])
def test_adjust_pvalues_bad_arguments(no_engine, bad):
    p = np.full((3, 10), 0.5)
    with pytest.raises(ValueError):
        adjust_pvalues(p, **bad)


@pytest.mark.parametrize("p", [
    np.full((3, 10), 0.5, dtype=np.float32), np.full(10, 0.5), np.full((2, 3, 4), 0.5), [[0.5, 0.5]], np.full((3, 10), 1, dtype=np.int64),
])
def test_adjust_pvalues_bad_planes(no_engine, p):
    with pytest.raises(ValueError):
        adjust_pvalues(p)


def test_adjust_pvalues_method_names_are_known():
    assert {adjust_mod._method(n) for n in ("bh", "benjamini-hochberg", "BH")} == {"bh"}
    assert {adjust_mod._method(n) for n in ("by", "benjamini-yekutieli")} == {"by"}
    assert adjust_mod._method("bonferroni") == "bonferroni"
    assert set(adjust_mod.METHODS.values()) == set(_lib.ADJUST_METHODS)
    assert "adjust_pvalues" in illico_amd.__all__ and "differential_expression" in illico_amd.__all__


@pytest.mark.parametrize("bad", [
    dict(corr_method="holm"), dict(n_genes=0), dict(n_genes=-3), dict(n_genes=2.5), dict(n_genes=True),
])
def test_differential_expression_bad_arguments(no_engine, bad):
    adata = AnnDataLite(np.zeros((4, 3), np.float32), obs=pd.DataFrame({"pert": ["a", "b", "a", "b"]}))
    with pytest.raises(ValueError):
        differential_expression(adata, False, "pert", **bad)


def test_differential_expression_unknown_keyword(no_engine):
    adata = AnnDataLite(np.zeros((4, 3), np.float32), obs=pd.DataFrame({"pert": ["a", "b", "a", "b"]}))
    with pytest.raises(TypeError):
        differential_expression(adata, False, "pert", no_such_argument=1)


def test_c_header_and_binding_agree_on_the_adjustment_constants():
    from conftest import ROOT
    header = (ROOT / "include" / "illico_hip.h").read_text()
    assert f"ILLICO_ADJ_LDS_COLS = {_lib.ADJUST_LDS_COLS}" in header
    assert "ILLICO_ADJ_BH = 0, ILLICO_ADJ_BY = 1, ILLICO_ADJ_BONFERRONI = 2" in header
    assert (_lib.ADJ_BH, _lib.ADJ_BY, _lib.ADJ_BONFERRONI) == (0, 1, 2)
    assert "illico_adjust_pvalues" in _lib.SYMBOLS
