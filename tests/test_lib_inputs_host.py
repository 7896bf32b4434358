"""The module-level input helpers of illico_amd._lib (_dense_input, _sparse_input, _check_chunk_bounds) on numpy inputs: they need
neither the library nor a device."""
import numpy as np
import pytest

from illico_amd import _lib


def test_dense_contiguous_float32():
    X = np.arange(40, dtype=np.float32).reshape(8, 5)
    ptr, on_dev, keep, n_rows, n_cols, ld, dt = _lib._dense_input(X)
    assert (ptr, on_dev, n_rows, n_cols, ld, dt) == (X.ctypes.data, False, 8, 5, 5, _lib.F32)
    assert keep is X


def test_dense_column_slice_is_not_copied():
    P = np.arange(80, dtype=np.float64).reshape(8, 10)
    X = P[:, 2:7]
    ptr, _, keep, n_rows, n_cols, ld, dt = _lib._dense_input(X)
    assert ptr == X.ctypes.data == P.ctypes.data + 2 * 8 and keep is X
    assert (n_rows, n_cols, ld, dt) == (8, 5, P.shape[1], _lib.F64)


@pytest.mark.parametrize("view", [lambda A: np.asfortranarray(A), lambda A: A[::-1], lambda A: A[:, ::-1], lambda A: A[:, ::2]],
                         ids=["fortran", "rows_reversed", "columns_reversed", "every_other_column"])
def test_dense_odd_strides_are_copied(view):
    X = view(np.arange(48, dtype=np.int32).reshape(8, 6))
    ptr, _, keep, n_rows, n_cols, ld, dt = _lib._dense_input(X)
    assert keep is not X and keep.flags.c_contiguous and ptr == keep.ctypes.data
    np.testing.assert_array_equal(keep, X)
    assert (n_rows, n_cols, ld, dt) == (*X.shape, X.shape[1], _lib.I32)


@pytest.mark.parametrize("view", [lambda r: np.broadcast_to(r, (8, 6)), lambda r: np.lib.stride_tricks.as_strided(np.arange(13, dtype=r.dtype), (8, 6), (r.itemsize,) * 2)],
                         ids=["zero_row_stride", "overlapping_rows"])
def test_dense_rows_closer_than_their_length_are_copied(view):
    X = view(np.arange(6, dtype=np.float32))
    assert X.strides[0] < 6 * X.itemsize
    ptr, _, keep, n_rows, n_cols, ld, dt = _lib._dense_input(X)
    assert keep is not X and keep.flags.c_contiguous and ptr == keep.ctypes.data
    np.testing.assert_array_equal(keep, X)
    assert (n_rows, n_cols, ld, dt) == (8, 6, 6, _lib.F32)


def test_dense_cpu_tensor_is_host_memory_and_never_copied():
    import torch
    T = torch.arange(80, dtype=torch.float32).reshape(8, 10)
    for X, ld in ((T, 10), (T[:, 2:8], 10), (T[3:4, 2:8], 6)):
        ptr, on_dev, keep, n_rows, n_cols, got_ld, dt = _lib._dense_input(X)
        assert keep is X and (ptr, on_dev, n_rows, n_cols, got_ld, dt) == (X.data_ptr(), False, *X.shape, ld, _lib.F32)
    for X in (torch.arange(6.).expand(8, 6), T.as_strided((8, 6), (1, 1)), T[:, ::2], T.t(), T[0], T.reshape(2, 4, 10)):
        with pytest.raises(ValueError):
            _lib._dense_input(X)


def test_dense_one_row():
    P = np.arange(10, dtype=np.float32).reshape(1, 10)
    for X in (P, P[:, 3:7]):
        ptr, _, _, n_rows, n_cols, ld, _ = _lib._dense_input(X)
        assert (ptr, n_rows, n_cols, ld) == (X.ctypes.data, 1, X.shape[1], X.shape[1])


@pytest.mark.parametrize("given,code,held", [(np.uint8, _lib.I32, np.int32), (np.float16, _lib.F32, np.float32), (np.uint32, _lib.I64, np.int64)])
def test_dense_values_are_widened(given, code, held):
    X = np.arange(12).reshape(3, 4).astype(given)
    _, _, keep, _, _, ld, dt = _lib._dense_input(X)
    assert dt == code and keep.dtype == held and ld == 4
    np.testing.assert_array_equal(keep, X)
    d = _lib._sparse_input(X.ravel(), np.zeros(12, np.int32), np.arange(13, dtype=np.int32), (12, 1))[0]
    assert d.np_dtype == held and _lib.dtype_code(d.np_dtype) == code
    np.testing.assert_array_equal(d.keep, X.ravel())


@pytest.mark.parametrize("shape", [(6,), (2, 3, 4)])
def test_dense_must_be_2d(shape):
    with pytest.raises(ValueError, match="2-D"):
        _lib._dense_input(np.zeros(shape, dtype=np.float32))


def _triple(idt, pdt):
    return np.array([1.0, 2.0, 3.0], dtype=np.float32), np.array([0, 2, 1], dtype=idt), np.array([0, 1, 3], dtype=pdt)


def test_sparse_int32_indices():
    data, indices, indptr = _triple(np.int32, np.int32)
    d, i, p, idx, n_rows, n_cols = _lib._sparse_input(data, indices, indptr, (3, 2))
    assert (idx, n_rows, n_cols) == (_lib.IDX_I32, 3, 2)
    assert (d.ptr, i.ptr, p.ptr) == (data.ctypes.data, indices.ctypes.data, indptr.ctypes.data)  # nothing is copied
    assert not (d.on_device or i.on_device or p.on_device)


@pytest.mark.parametrize("idt,pdt", [(np.int32, np.int64), (np.int64, np.int32), (np.int64, np.int64), (np.uint16, np.int32)])
def test_sparse_mixed_indices_become_int64(idt, pdt):
    data, indices, indptr = _triple(idt, pdt)
    d, i, p, idx, _, _ = _lib._sparse_input(data, indices, indptr, (3, 2))
    assert idx == _lib.IDX_I64 and i.np_dtype == p.np_dtype == np.int64 and i.keep.dtype == p.keep.dtype == np.int64
    np.testing.assert_array_equal(i.keep, indices)
    np.testing.assert_array_equal(p.keep, indptr)


@pytest.mark.parametrize("dtype", [np.complex64, np.dtype("U3"), np.dtype("O")])
def test_unsupported_value_dtype(dtype):
    bad = np.zeros(3, dtype=dtype)
    want = f"Support for element dtype {bad.dtype} is not implemented."
    with pytest.raises(KeyError) as e:
        _lib._sparse_input(bad, *_triple(np.int32, np.int32)[1:], (3, 2))
    assert e.value.args[0] == want
    with pytest.raises(KeyError) as e:
        _lib._dense_input(bad.reshape(3, 1))
    assert e.value.args[0] == want


def test_uint64_values_beyond_int64():
    with pytest.raises(KeyError) as e:
        _lib._dense_input(np.array([[2 ** 63]], dtype=np.uint64))
    assert e.value.args[0] == "uint64 values above 2**63-1 are not supported."


@pytest.mark.parametrize("lb,ub", [(-1, 3), (0, 7), (3, 2)])
def test_chunk_bounds_refused(lb, ub):
    with pytest.raises(ValueError) as e:
        _lib._check_chunk_bounds(lb, ub, 6)
    assert e.value.args[0] == f"Invalid chunk bounds: ({lb}, {ub}) for data with 6 columns."


def test_chunk_bounds_accepted():
    for lb, ub in ((2, 2), (0, 6), (0, 0), (6, 6), (1, 5)):
        assert _lib._check_chunk_bounds(lb, ub, 6) is None
