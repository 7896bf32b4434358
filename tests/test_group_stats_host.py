"""group_statistics / differential_expression(pts=...) / the illico_group_stats_* bindings: argument errors raise before any engine
(or GPU) is touched."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import illico_amd
from illico_amd import AnnDataLite, differential_expression, group_statistics
from illico_amd import _lib
from illico_amd import adjust as adjust_mod
from illico_amd import group_stats as gs_mod

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["illico_group_stats_dense", "illico_group_stats_csc", "illico_group_stats_csr", "illico_group_stats_bound"]


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "get_engine", boom)
    monkeypatch.setattr(adjust_mod, "_wilcoxon_planes", boom)
    monkeypatch.setattr(gs_mod, "stat_planes", boom)


def _adata(X=None, **layers):
    X = np.zeros((4, 3), np.float32) if X is None else X
    return AnnDataLite(X, obs=pd.DataFrame({"pert": ["a", "b", "a", "b"]}), layers=layers or None)


@pytest.mark.parametrize("pts", [1, "yes", None, 0.0])
def test_bad_pts_type(no_engine, pts):
    with pytest.raises(ValueError, match="pts"):
        differential_expression(_adata(), False, "pert", pts=pts)


def test_unknown_keyword(no_engine):
    with pytest.raises(TypeError):
        differential_expression(_adata(), False, "pert", pts=True, no_such_argument=1)
    with pytest.raises(TypeError):
        group_statistics(_adata(), "pert", is_log1p=False, no_such_argument=1)


def test_is_log1p_is_required_and_a_bool(no_engine):
    with pytest.raises(TypeError):
        group_statistics(_adata(), "pert")
    with pytest.raises(ValueError):
        group_statistics(_adata(), "pert", is_log1p="no")


def test_bad_layer(no_engine):
    with pytest.raises(KeyError):
        group_statistics(_adata(), "pert", is_log1p=False, layer="no_such_layer")


@pytest.mark.parametrize("X", [np.zeros(4, np.float32), np.zeros((4, 3, 2), np.float32)])
def test_non_2d_input(no_engine, X):
    adata = _adata()
    adata.X = X
    with pytest.raises(ValueError, match="2-D"):
        group_statistics(adata, "pert", is_log1p=False)


def test_exported():
    assert "group_statistics" in illico_amd.__all__
    assert illico_amd.group_statistics is group_statistics
    assert gs_mod.STAT_COLUMNS == ("pct_group", "pct_reference", "mean_group", "mean_reference")


def test_header_declares_the_entry_points_the_binding_loads():
    header = (ROOT / "include" / "illico_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SYMBOLS


def test_null_context_is_an_argument_error():
    lib = _lib.load()  # (the library is built before the suite runs; no device is needed for these calls)
    out = (ctypes.c_int64 * 4)()
    rc = [lib.illico_group_stats_dense(None, out, 0, 2, 2, 2, 0, 2, 0, out, None, None, None, 2),
          lib.illico_group_stats_csc(None, out, 0, out, out, 0, 2, 2, 0, 2, 0, out, None, None, None, 2),
          lib.illico_group_stats_csr(None, out, 0, out, out, 0, 2, 2, 0, 2, 0, out, None, None, None, 2),
          lib.illico_group_stats_bound(None, None, 0, 2, 0, out, None, None, None, 2)]
    assert rc == [_lib.ERR_ARG] * 4
    with pytest.raises(ValueError):
        _lib._raise(_lib.ERR_ARG, "x")
    with pytest.raises(ValueError):
        _lib._raise(_lib.ERR_BOUNDS, "x")
    with pytest.raises(ValueError):
        _lib._raise(_lib.ERR_NO_GROUPS, "x")
    with pytest.raises(KeyError):
        _lib._raise(_lib.ERR_DTYPE, "x")
    with pytest.raises(NotImplementedError):
        _lib._raise(_lib.ERR_UNSUPPORTED, "x")


def _bare_engine():
    eng = _lib.Engine.__new__(_lib.Engine)  # (no context: _gs_outputs validates planes on the host)
    eng.device = 0
    return eng


@pytest.mark.parametrize("out", [
    (None, None),
    (None, None, None, None),
    (np.zeros((3, 5), np.int64),),
    (np.zeros((3, 5), np.float64), np.zeros((3, 5), np.float64)),      # nnz must be int64
    (np.zeros((3, 5), np.int64), np.zeros((3, 5), np.float32)),         # sum must be float64
    (np.zeros((3, 4), np.int64), np.zeros((3, 5), np.float64)),         # shape
    (np.zeros((3, 10), np.int64)[:, ::2], np.zeros((3, 5), np.float64)),  # column stride
    (np.zeros((3, 6), np.int64)[:, :5], np.zeros((3, 5), np.float64)),    # row strides differ
])
def test_bad_output_planes(out):
    with pytest.raises(ValueError):
        _bare_engine()._gs_outputs(out, 3, 5, False, False)


def test_output_planes_may_be_null():
    nnz = np.zeros((3, 8), np.int64)[:, 1:6]
    s = np.zeros((3, 8), np.float64)[:, 2:7]
    planes, ptrs, flag, ld = _bare_engine()._gs_outputs((nnz, None, None, s), 3, 5, True, False)
    assert ptrs[1] is None and ptrs[2] is None and ptrs[0] == nnz.ctypes.data and ptrs[3] == s.ctypes.data
    assert flag == 0 and ld == 8
