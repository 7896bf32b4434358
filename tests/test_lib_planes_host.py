"""The plane helpers of illico_amd._lib (_plane, _plane_set, _pair_selection, _pair_planes, Engine._outputs; _stacked_rows, _hists_input,
_moment_planes, _sums_arg) and its signature table, on numpy arrays and CPU tensors: they need neither the library nor a device."""
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



# ---- the checks the plane-to-plane entry points share ----
def test_stacked_rows_is_a_view_of_the_block_and_of_its_first_columns():
    block = np.arange(2 * 3 * 8, dtype=np.float64).reshape(2, 3, 8)
    for x, W in ((block, 8), (block[:, :, :5], 5)):
        rows = _lib._stacked_rows(x, "x")
        assert rows.shape == (6, W) and np.shares_memory(rows, block) and rows.ctypes.data == block.ctypes.data
        assert np.array_equal(rows, x.reshape(6, W)) and _lib._plane(rows, "x").pitch == 8
    t = torch.arange(2 * 3 * 8, dtype=torch.float64).reshape(2, 3, 8)
    rows = _lib._stacked_rows(t[:, :, :5], "t")
    assert tuple(rows.shape) == (6, 5) and rows.data_ptr() == t.data_ptr() and torch.equal(rows, t[:, :, :5].reshape(6, 5))
    assert _lib._stacked_rows(block[:1, ::2], "x").shape == (2, 8)    # one stack: any row stride


def test_stacked_rows_refusals():
    block = np.zeros((4, 3, 8))
    for bad in (block[::2], block[:, :2], block[:, ::2], block.transpose(1, 0, 2), torch.zeros(4, 3, 8)[:, :2]):
        with pytest.raises(ValueError, match="one row stride apart"):
            _lib._stacked_rows(bad, "x")
    for bad in (np.zeros((3, 8)), np.zeros((2, 2, 2, 2))):
        with pytest.raises(ValueError, match="three dimensions"):
            _lib._stacked_rows(bad, "x")


def test_pairs_as_rows_is_stacked_rows_of_a_square_stack():
    x = np.arange(3 * 3 * 6, dtype=np.float64).reshape(3, 3, 6)[:, :, :4]
    K, W, rows = _lib._pairs_as_rows(x, "p")
    assert (K, W) == (3, 4) and np.array_equal(rows, x.reshape(9, 4)) and np.shares_memory(rows, x)
    for bad in (np.zeros((2, 3, 4)), np.zeros((3, 4)), [[[0.0]]]):
        with pytest.raises(ValueError):
            _lib._pairs_as_rows(bad, "p")


def test_hists_input_accepts_host_arrays_of_any_integer_type():
    H, flags = np.arange(2 * 3 * 256, dtype=np.int64).reshape(2, 3, 256), [0, 1, 0]
    H2, f2, rows, W, on_dev = _lib._hists_input(H, flags, "G")
    assert (rows, W, on_dev) == (2, 3, False) and H2.dtype == f2.dtype == np.uint32 and H2.flags.c_contiguous
    assert np.array_equal(H2, H) and f2.tolist() == flags
    Hu = H.astype(np.uint32)
    assert _lib._hists_input(Hu, np.zeros(3, np.uint32), "G")[0] is Hu    # as it is
    assert _lib._hists_input(Hu, np.zeros(3, np.uint32), "G", np.zeros((2, 3)), "H, flags and sums")[2:] == (2, 3, False)


def test_hists_input_refusals():
    H, flags = np.zeros((2, 3, 256), np.uint32), np.zeros(3, np.uint32)
    with pytest.raises(ValueError, match=r"H must be \[G \* B, W, 256\]$"):
        _lib._hists_input(H[0], flags, "G * B")
    for bad_H, bad_f in ((np.zeros((2, 3, 255), np.uint32), flags), (H, np.zeros(4, np.uint32)), (H, np.zeros((3, 1), np.uint32))):
        with pytest.raises(ValueError, match=r"H must be \[G, W, 256\] and flags \[W\], got"):
            _lib._hists_input(bad_H, bad_f, "G")
    with pytest.raises(ValueError, match="^H and flags must live on the same side"):
        _lib._hists_input(torch.zeros(2, 3, 256, dtype=torch.int32), flags, "G")
    with pytest.raises(ValueError, match="^H, flags and sums must live on the same side"):
        _lib._hists_input(H, flags, "G", torch.zeros(2, 3, dtype=torch.float64), "H, flags and sums")
    with pytest.raises(ValueError, match="contiguous 32-bit integer CUDA tensors"):   # tensors, but not on a device
        _lib._hists_input(torch.zeros(2, 3, 256, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), "G")


def test_moment_planes_accepted_forms():
    S, Q = np.arange(12, dtype=np.float64).reshape(3, 4), np.ones((3, 4))
    ins, G, W, on_dev, ptrs, ld = _lib._moment_planes((("sum", S), ("sumsq", Q), ("fsum", None)), ("sum", "sumsq"), 3)
    assert (G, W, on_dev, ld) == (3, 4, False, 4) and ptrs == [S.ctypes.data, Q.ctypes.data, None]
    assert ins[0].array is S and ins[1].array is Q and ins[2] is None
    wide = np.zeros((3, 2, 9))
    ins, G, W, _, ptrs, ld = _lib._moment_planes((("sum", wide[:, 0, 2:6]), ("sumsq", wide[:, 1, 2:6])), ("sum", "sumsq"), 3)   # one pitch: as they are
    assert ld == 18 and ptrs == [wide.ctypes.data + 16, wide.ctypes.data + 16 + 72]
    ins, G, W, _, ptrs, ld = _lib._moment_planes((("sum", S), ("sumsq", wide[:, 1, 2:6])), ("sum", "sumsq"), 3)   # two pitches: made contiguous
    assert ld == 4 and all(q.array.flags.c_contiguous for q in ins) and np.array_equal(ins[0].array, S)
    ins, _, _, _, _, ld = _lib._moment_planes((("sum", S[:, ::2]), ("sumsq", Q[:, ::2])), ("sum", "sumsq"), 3)   # a column stride: copied
    assert ld == 2 and np.array_equal(ins[0].array, S[:, ::2])


def test_moment_planes_refusals():
    S, Q = np.zeros((3, 4)), np.zeros((3, 4))
    for planes, n_groups, message in (((("sum", S), ("sumsq", None)), 3, "sum and sumsq are required"),
                                      ((("sum", None), ("sumsq", Q)), 3, "sum and sumsq are required"),
                                      ((("sum", S), ("sumsq", np.zeros((3, 5)))), 3, "share one shape"),
                                      ((("sum", S), ("sumsq", Q), ("fsum", np.zeros((4, 4)))), 3, "share one shape"),
                                      ((("sum", S), ("sumsq", Q)), 4, "have 3 rows but the engine's groups number 4"),
                                      ((("sum", S), ("sumsq", Q)), None, "groups number None"),
                                      ((("sum", S), ("sumsq", Q.astype(np.float32))), 3, "float64"),
                                      ((("sum", S), ("sumsq", torch.zeros(3, 4, dtype=torch.float64))), 3, "CPU tensor"),
                                      ((("sum", S), ("sumsq", np.zeros(12))), 3, "2-D")):
        with pytest.raises(ValueError, match=message):
            _lib._moment_planes(planes, ("sum", "sumsq"), n_groups)


def test_sums_arg():
    assert _lib._sums_arg(None, (3, 4), False, "H") == (None, None, 0)
    assert _lib._sums_arg(None, (3, 4), True, "H") == (None, None, 0)
    wide = np.zeros((3, 9))
    array, ptr, ld = _lib._sums_arg(wide[:, 2:6], (3, 4), False, "H")
    assert array.base is wide and (ptr, ld) == (wide.ctypes.data + 16, 9)
    array, ptr, ld = _lib._sums_arg(wide[:, ::2][:, :4], (3, 4), False, "H")   # a column stride: copied
    assert array.flags.c_contiguous and (ptr, ld) == (array.ctypes.data, 4)
    for bad, on_dev, message in ((np.zeros((3, 5)), False, "shape"), (np.zeros((3, 4), np.float32), False, "float64"),
                                 (torch.zeros(3, 4, dtype=torch.float64), False, "CPU tensor"), (wide[:, :4], True, "sums must live on the side of the matrix")):
        with pytest.raises(ValueError, match=message):
            _lib._sums_arg(bad, (3, 4), on_dev, "the matrix")
