"""The plane helpers of illico_amd._lib (_plane, _plane_set, _pair_selection, _pair_planes, Engine._outputs) and its signature table, on numpy arrays and CPU
tensors: they need neither the library nor a device."""
import ctypes
import re

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import as_strided

from conftest import ROOT
from illico_amd import _lib


def _strided(kind):
    """A [3, 5] float64 view the C side cannot walk, and the values it shows."""
    if kind == "every_other_column":
        return np.arange(30, dtype=np.float64).reshape(3, 10)[:, ::2]
    if kind == "rows_reversed":
        return np.arange(15, dtype=np.float64).reshape(3, 5)[::-1]
    if kind == "zero_stride_rows":
        return np.broadcast_to(np.arange(5, dtype=np.float64), (3, 5))
    return as_strided(np.arange(7, dtype=np.float64), shape=(3, 5), strides=(8, 8))  # rows one element apart


STRIDED = ["every_other_column", "rows_reversed", "zero_stride_rows", "overlapping_rows"]


def test_contiguous_plane():
    A = np.zeros((3, 5))
    q = _lib._plane(A, "A")
    assert q.array is A and q == (A, A.ctypes.data, 3, 5, 5, False)


def test_column_window_is_not_copied():
    B = np.zeros((3, 8))
    A = B[:, 2:7]
    q = _lib._plane(A, "A", shape=(3, 5), writeable=True)
    assert q.array is A and (q.ptr, q.rows, q.cols, q.pitch, q.on_device) == (B.ctypes.data + 16, 3, 5, 8, False)


def test_one_row_and_one_column():
    B = np.zeros((3, 8), np.int64)
    row, col = B[1:2, 2:7], B[:, 3:4]
    q = _lib._plane(row, "row", dtype=np.int64)
    assert q.array is row and (q.ptr, q.rows, q.cols, q.pitch) == (B.ctypes.data + 8 * 10, 1, 5, 5)
    q = _lib._plane(col, "col", dtype=np.int64)
    assert q.array is col and (q.ptr, q.rows, q.cols, q.pitch) == (B.ctypes.data + 8 * 3, 3, 1, 8)
    q = _lib._plane(B[:, ::4][:, :1], "col", dtype=np.int64)   # a single column has no column stride to speak of
    assert (q.cols, q.pitch) == (1, 8)


@pytest.mark.parametrize("x,kw", [
    (np.zeros((3, 5), np.float32), {}),
    (np.zeros((3, 5), np.float64), dict(dtype=np.int64)),
    (np.zeros((3, 5), np.dtype(np.float64).newbyteorder()), {}),
    (np.zeros((3, 5), np.dtype(np.int64).newbyteorder()), dict(dtype=np.int64)),
    (np.zeros(5), {}),
    (np.zeros((3, 5, 2)), {}),
    (np.zeros((3, 5)), dict(shape=(4, 5))),
    (np.zeros((3, 5)), dict(shape=(3, 4))),
    (torch.zeros((3, 5), dtype=torch.float64), {}),
    (torch.zeros((3, 5), dtype=torch.float64), dict(copy_ok=True)),
    ([[0.0, 1.0], [2.0, 3.0]], {}),
    (None, {}),
], ids=["float32", "not_int64", "float64_byte_swapped", "int64_byte_swapped", "1-D", "3-D", "rows", "cols", "cpu_tensor", "cpu_tensor_copy_ok", "list", "none"])
def test_refused(x, kw):
    with pytest.raises(ValueError):
        _lib._plane(x, "x", **kw)


@pytest.mark.parametrize("kind", STRIDED)
def test_strides_the_library_cannot_walk(kind):
    X = _strided(kind)
    assert X.shape == (3, 5)
    with pytest.raises(ValueError):
        _lib._plane(X, "X")
    q = _lib._plane(X, "X", copy_ok=True)
    assert q.array is not X and q.array.flags.c_contiguous and q.ptr == q.array.ctypes.data
    assert (q.rows, q.cols, q.pitch, q.on_device) == (3, 5, 5, False)
    np.testing.assert_array_equal(q.array, X)


def test_row_stride_of_half_an_element():
    X = as_strided(np.zeros(17), shape=(3, 5), strides=(44, 8))   # (the last element ends at byte 2 * 44 + 5 * 8 = 128 of 136)
    with pytest.raises(ValueError):
        _lib._plane(X, "X")
    assert _lib._plane(X, "X", copy_ok=True).pitch == 5


def test_read_only():
    A = np.zeros((3, 5))
    A.flags.writeable = False
    assert _lib._plane(A, "A").array is A
    with pytest.raises(ValueError):
        _lib._plane(A, "A", writeable=True)


def test_plane_set():
    B = [np.zeros((3, 8)) for _ in range(3)]
    a, b = (_lib._plane(x[:, 1:6], "x") for x in B[:2])
    ptrs, flag, pitch = _lib._plane_set([a, None, b, None], "planes")
    assert ptrs == [B[0].ctypes.data + 8, None, B[1].ctypes.data + 8, None] and (flag, pitch) == (0, 8)
    with pytest.raises(ValueError):
        _lib._plane_set([a, _lib._plane(np.zeros((3, 5)), "x")], "planes")      # pitches 8 and 5
    dev = a._replace(on_device=True)   # (a record as a CUDA tensor would give it: the rule needs no device)
    assert _lib._plane_set([dev, None], "planes")[1:] == (_lib.FLAG_OUTPUT_DEVICE, 8)
    with pytest.raises(ValueError):
        _lib._plane_set([a, dev], "planes")
    assert _lib._plane_set([None, None], "planes") == ([None, None], 0, None)


def _bare_engine():
    eng = _lib.Engine.__new__(_lib.Engine)   # (no context: _outputs is host logic)
    eng.device = 0
    return eng


def test_outputs():
    G, W = 2, 6
    B = [np.zeros((G, 9)) for _ in range(4)]
    out = tuple(b[:, 1:7] for b in B)
    planes, ptrs, flag, ld = _bare_engine()._outputs(out, G, W, False)
    assert all(p is q for p, q in zip(planes, out)) and ptrs == [b.ctypes.data + 8 for b in B] and (flag, ld) == (0, 9)
    planes, ptrs, flag, ld = _bare_engine()._outputs(out[:3], G, W, True)    # (given planes decide the side)
    assert len(planes) == len(ptrs) == 3 and (flag, ld) == (0, 9)
    planes, ptrs, flag, ld = _bare_engine()._outputs(None, G, W, False)
    assert ptrs == [p.ctypes.data for p in planes] and (flag, ld) == (0, W)


def _read_only(shape):
    A = np.zeros(shape)
    A.flags.writeable = False
    return A


@pytest.mark.parametrize("bad", [
    lambda: _read_only((2, 6)),
    lambda: torch.zeros((2, 6), dtype=torch.float64),
    lambda: np.zeros((3, 6)),
    lambda: np.zeros((2, 6), np.float32),
    lambda: np.zeros((2, 6), np.dtype(np.float64).newbyteorder()),
    lambda: np.zeros((2, 8))[:, 1:7],           # another pitch than the other two
    lambda: np.zeros((2, 12))[:, ::2],
], ids=["read_only", "cpu_tensor", "one_row_more", "float32", "byte_swapped", "pitch", "column_stride"])
def test_outputs_refuses(bad):
    for k in range(3):
        out = [np.zeros((2, 6)) for _ in range(3)]
        out[k] = bad()
        with pytest.raises(ValueError):
            _bare_engine()._outputs(tuple(out), 2, 6, False)


def test_block_takes_exactly_the_named_dtypes():
    H = np.zeros((2, 6, 256), np.uint32)
    assert _lib._block(H, "H", (np.uint32,), H.shape, writeable=True) == (H.ctypes.data, False)
    for bad in (H.astype(np.int32), H.astype(H.dtype.newbyteorder()), H[:, ::2], H.tolist(), torch.zeros(H.shape, dtype=torch.int32)):
        with pytest.raises(ValueError):
            _lib._block(bad, "H", (np.uint32,), H.shape)
    assert _lib._block(H.astype(np.int32), "H", (np.int32, np.uint32), H.shape)[1] is False
    with pytest.raises(ValueError):
        _lib._block(H, "H", (np.uint32,), H.shape, on_device=True)


def test_pair_selection():
    assert _lib._pair_selection(None, 5) == (5, None, None)
    K, keep, ptr = _lib._pair_selection([3, 0, 4], 5)
    assert K == 3 and keep.dtype == np.int64 and keep.tolist() == [3, 0, 4] and ptr == keep.ctypes.data


@pytest.mark.parametrize("with_left", [False, True])
def test_pair_planes(with_left):
    K, W = 2, 3
    given = [np.zeros((K, K, W)) for _ in range(4)] + ([np.zeros(W, np.uint32)] if with_left else [])
    planes, left, ptrs, left_ptr, on_dev = _lib._pair_planes(given, 4, K, W, False, None, with_left)
    assert all(p is q for p, q in zip(planes, given)) and ptrs == [q.ctypes.data for q in given[:4]] and on_dev is False
    assert (left is given[4] and left_ptr == left.ctypes.data) if with_left else (left is None and left_ptr is None)
    planes, left, ptrs, left_ptr, on_dev = _lib._pair_planes(None, 3, K, W, False, "cuda:0", with_left)   # (host input: host planes)
    assert len(planes) == 3 and all(p.shape == (K, K, W) and p.dtype == np.float64 for p in planes) and on_dev is False
    assert (left.shape == (W,) and left.dtype == np.uint32) if with_left else left is None
    tail = given[4:]
    for n, bad, text in [(3, given, "out must hold 3 planes (p, U, fold change)"),                    # one plane too many
                         (4, given[:3] + tail, "out must hold 4 planes (p, U, fold change, z)"),      # one too few
                         (4, [np.zeros((K, K, W + 1))] + given[1:], "array of shape (2, 2, 3)"),      # wrong shape
                         (4, given[:3] + [np.zeros((K * K, W))] + tail, "array of shape (2, 2, 3)"),
                         (4, given[:3] + [torch.zeros((K, K, W), dtype=torch.float64)] + tail, "numpy array or a CUDA tensor")]:
        with pytest.raises(ValueError, match=re.escape(text)) as e:
            _lib._pair_planes(bad, n, K, W, False, None, with_left)
        assert ("and left" in str(e.value)) == (with_left and "out must hold" in text)
    if with_left:   # the side is that of left: a CPU tensor is neither, and host planes behind host left are host planes whatever the input
        with pytest.raises(ValueError, match="left must be a numpy array or a CUDA tensor"):
            _lib._pair_planes(given[:4] + [torch.zeros(W, dtype=torch.int32)], 4, K, W, False, None, True)
        assert _lib._pair_planes(given, 4, K, W, True, "cuda:0", True)[4] is False
        with pytest.raises(ValueError, match="left must be a writeable contiguous host uint32"):
            _lib._pair_planes(given[:4] + [np.zeros(W, np.int32)], 4, K, W, False, None, True)
    else:           # mixed sides: host planes where the input, and with it the planes, are on the device
        with pytest.raises(ValueError, match="an output plane must be a writeable contiguous CUDA float64 array"):
            _lib._pair_planes(given, 4, K, W, True, "cuda:0", False)


def test_outputs_of_an_empty_chunk():
    out = tuple(np.zeros((2, 0)) for _ in range(3))
    planes, ptrs, flag, ld = _bare_engine()._outputs(out, 2, 0, False)
    assert all(p is q for p, q in zip(planes, out)) and (ptrs, flag, ld) == (None, 0, 1)
    planes, ptrs, flag, ld = _bare_engine()._outputs(None, 2, 0, False, scores=True)
    assert len(planes) == 4 and all(p.shape == (2, 0) for p in planes) and (ptrs, flag, ld) == (None, 0, 1)


def test_signature_table_names_what_the_header_declares():
    header = (ROOT / "include" / "illico_hip.h").read_text()
    declared = set(re.findall(r"\b(illico_\w+)\s*\(", header))
    assert len(_lib.SIGNATURES) == 44 and set(_lib.SIGNATURES) == declared
    assert _lib.SYMBOLS == list(_lib.SIGNATURES)
    for name, (_, restype) in _lib.SIGNATURES.items():
        returns_text = re.search(rf"const char \*\s*{name}\s*\(", header) is not None
        assert restype is (ctypes.c_char_p if returns_text else ctypes.c_int), name


@pytest.mark.parametrize("plain", ["illico_run_dense", "illico_run_csc", "illico_run_csr", "illico_run_bound"])
def test_ex_signature_is_the_plain_one_with_one_more_plane(plain):
    args, restype = _lib.SIGNATURES[plain]
    assert _lib.SIGNATURES[plain + "_ex"] == (args[:-1] + [ctypes.c_void_p] + args[-1:], restype)

