"""Matrix and plane layouts through the Engine: what _lib._dense_input, _plane and _plane_set pass to the library unchanged, copy
first, or refuse.

One matrix of 8 cells x 6 genes of small integers, two interleaved groups of 4 cells, every group against the rest (so every cell
of every plane is written).  A call on an oddly laid out X, or into windows of wider planes, must give bit for bit what the same
call gives on a contiguous X of the same side with freshly allocated planes; the cells of a backing outside the window keep their
sentinel.  Every refused device plane is cut from a backing at least four times as large as what an accepted call would write, and
the refusals are made with the library out of reach: a missing check fails the test and writes nothing.
"""
import types

import numpy as np
import pytest
import torch

from illico_amd import _lib

pytestmark = pytest.mark.gpu

N, M, G = 8, 6, 2
CODES = np.array([0, 1, 0, 1, 1, 0, 0, 1])
X = np.array([[0, 3, 0, 1, 7, 0],
              [2, 0, 0, 4, 0, 1],
              [0, 5, 1, 0, 2, 0],
              [9, 0, 0, 2, 0, 0],
              [0, 1, 6, 0, 3, 2],
              [4, 0, 0, 0, 0, 8],
              [0, 2, 3, 5, 0, 0],
              [1, 0, 0, 0, 6, 0]], dtype=np.int32)
WINDOWS = ((0, M), (1, 5))
SENTINEL = -7
SIDES = ("host", "device")


def _compressed(A):
    """(data, indices, indptr) of the rows of A, int32: the non-zero entries only."""
    rows = [np.flatnonzero(r) for r in A]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return np.concatenate([A[k][r] for k, r in enumerate(rows)]).astype(np.int32), np.concatenate(rows).astype(np.int32), indptr


@pytest.fixture(scope="module")
def engine():
    eng = _lib.Engine(0)
    counts = np.bincount(CODES)
    eng.set_groups(types.SimpleNamespace(encoded_groups=CODES, counts=counts, indices=np.argsort(CODES, kind="stable"),
                                         indptr=np.concatenate([[0], np.cumsum(counts)]), encoded_ref_group=-1))
    yield eng
    eng.close()


def _host(a):
    return a.cpu().numpy() if _lib._is_torch_tensor(a) else a


def _assert_same_bits(got, want):
    got, want = (got, want) if isinstance(got, (tuple, list)) else ((got,), (want,))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(_host(g)), np.ascontiguousarray(_host(w))
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes()


METHODS = {
    "run_dense": lambda eng, A, lb, ub: eng.run_dense(A, lb, ub, scores=True),
    "group_stats": lambda eng, A, lb, ub: eng.group_stats(A, lb, ub, rest=True),
    "group_moments": lambda eng, A, lb, ub: eng.group_moments(A, lb, ub, rest=True),
    "group_value_hists": lambda eng, A, lb, ub: eng.group_value_hists(A, lb, ub),
    "rank_statistics": lambda eng, A, lb, ub: eng.rank_statistics(A, lb, ub),
}


def _rows_reversed(A):
    return np.ascontiguousarray(A[::-1])[::-1], A


def _column_window(A):
    B = np.full((N, 10), 99, dtype=A.dtype)
    B[:, 2:8] = A
    return B[:, 2:8], A


def _cuda_column_window(A):
    return torch.from_numpy(_column_window(A)[0].base).cuda()[:, 2:8], torch.from_numpy(A).cuda()


def _broadcast_row(A):
    return np.broadcast_to(A[3], (N, M)), np.ascontiguousarray(np.broadcast_to(A[3], (N, M)))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", [np.int32, np.float32], ids=["int32", "float32"])
@pytest.mark.parametrize("layout", [_rows_reversed, _column_window, _cuda_column_window, _broadcast_row])
def test_input_layout(engine, layout, dtype, method):
    given, plain = layout(X.astype(dtype))
    assert tuple(given.shape) == tuple(plain.shape) == (N, M) and _lib._is_torch_tensor(given) == _lib._is_torch_tensor(plain)
    assert np.array_equal(_host(given), _host(plain))
    for lb, ub in WINDOWS:
        _assert_same_bits(METHODS[method](engine, given, lb, ub), METHODS[method](engine, plain, lb, ub))


def _side(a, side):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if side == "device" else np.ascontiguousarray(a)


def _windows(side, dtypes, cols=M):
    """For each dtype a [G, cols + 3] backing full of the sentinel, and its window [:, 1 : cols + 1]."""
    backs = [_side(np.full((G, cols + 3), SENTINEL, dtype=dt), side) for dt in dtypes]
    return backs, [b[:, 1:cols + 1] for b in backs]


def _assert_written_inside_only(backs, wins, want):
    _assert_same_bits(wins, want)
    for b in backs:
        b = _host(b)
        w = b.shape[1] - 3
        assert (b[:, 0] == SENTINEL).all() and (b[:, w + 1:] == SENTINEL).all()


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("side", SIDES)
def test_run_dense_into_windows(engine, side, n):
    A = _side(X, side)
    want = engine.run_dense(A, 0, M, scores=n == 4, device_out=side == "device")
    backs, wins = _windows(side, [np.float64] * n)
    got = engine.run_dense(A, 0, M, out=tuple(wins))
    assert all(g is w for g, w in zip(got, wins))
    _assert_written_inside_only(backs, wins, want)


@pytest.mark.parametrize("side", SIDES)
def test_group_stats_into_windows_with_planes_left_out(engine, side):
    A = _side(X, side)
    want = engine.group_stats(A, 0, M, rest=True)
    backs, wins = _windows(side, [np.int64, np.float64])
    got = engine.group_stats(A, 0, M, out=(wins[0], None, None, wins[1]))
    assert got[0] is wins[0] and got[1] is None and got[2] is None and got[3] is wins[1]
    _assert_written_inside_only(backs, wins, (want[0], want[3]))


@pytest.mark.parametrize("side", SIDES)
def test_ttest_from_moments_into_windows(engine, side):
    moments = engine.group_moments(_side(X, side), 0, M, rest=True)
    want = engine.ttest_from_moments(*moments, want=("t", "p", "df"))
    backs, wins = _windows(side, [np.float64] * 3)
    engine.ttest_from_moments(*moments, want=("t", "p", "df"), out=tuple(wins))
    _assert_written_inside_only(backs, wins, want)
    in_backs, ins = _windows(side, [np.float64] * 4)     # ... and the same from moments that are windows themselves
    for dst, src in zip(ins, moments):
        dst[...] = src
    _assert_same_bits(engine.ttest_from_moments(*ins, want=("t", "p", "df")), want)


@pytest.mark.parametrize("side", SIDES)
def test_adjust_pvalues_into_a_window(engine, side):
    p = engine.run_dense(_side(X, side), 0, M, device_out=side == "device")[0]
    want = engine.adjust_pvalues(p, "bh")
    backs, wins = _windows(side, [np.float64])
    assert engine.adjust_pvalues(p, "bh", out=wins[0]) is wins[0]
    _assert_written_inside_only(backs, wins, (want,))
    in_backs, ins = _windows(side, [np.float64])
    ins[0][...] = p
    _assert_same_bits(engine.adjust_pvalues(ins[0], "bh"), want)


def test_three_planes_are_what_the_plain_entry_points_give(engine):
    """A call without the z-score plane goes to illico_run_*_ex with a null out_z: the planes of out=None, of a given triple on
    either side, of a deferred call on device input, and of illico_run_dense / _csc / _csr / _bound called directly are the same bits."""
    csr, csc = _compressed(X), _compressed(X.T)
    Xd, cscd = torch.from_numpy(X).cuda(), tuple(torch.from_numpy(a).cuda() for a in csc)
    triple = lambda: tuple(torch.full((G, M), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3))
    bound = engine.bind_sparse("csc", *csc, (N, M))
    lib, flags = engine.lib, engine._flags(False, True, True)
    sparse_args = lambda a: (a[0].ctypes.data, _lib.I32, a[1].ctypes.data, a[2].ctypes.data, _lib.IDX_I32, N, M)
    calls = {
        "dense": (lambda **kw: engine.run_dense(X, 0, M, **kw), lib.illico_run_dense, (X.ctypes.data, _lib.I32, N, M, M)),
        "csc": (lambda **kw: engine.run_sparse("csc", *csc, (N, M), 0, M, **kw), lib.illico_run_csc, sparse_args(csc)),
        "csr": (lambda **kw: engine.run_sparse("csr", *csr, (N, M), 0, M, **kw), lib.illico_run_csr, sparse_args(csr)),
        "bound": (lambda **kw: bound.run(0, M, **kw), lib.illico_run_bound, (bound.h,)),
    }
    for name, (run, plain, matrix) in calls.items():
        want = [np.full((G, M), SENTINEL, np.float64) for _ in range(3)]
        engine._check(plain(engine.h, *matrix, 0, M, flags, 0, *[w.ctypes.data for w in want], M))
        assert not (want[0] == SENTINEL).any() and not (want[1] == SENTINEL).any(), name   # (every p and U was written)
        got = run()
        assert len(got) == 3
        _assert_same_bits(got, want)
        given = tuple(np.full((G, M), SENTINEL, np.float64) for _ in range(3))
        assert all(a is b for a, b in zip(run(out=given), given))
        _assert_same_bits(given, want)
        given = triple()
        assert all(a is b for a, b in zip(run(out=given), given))
        _assert_same_bits(given, want)
        deferred = {"dense": lambda **kw: engine.run_dense(Xd, 0, M, **kw),
                    "csc": lambda **kw: engine.run_sparse("csc", *cscd, (N, M), 0, M, **kw)}.get(name)
        if deferred is not None:
            given = triple()
            deferred(out=given, defer=True)
            engine.synchronize()
            _assert_same_bits(given, want)
    bound.release()


class _OutOfReach:
    """Stands in for the loaded library: its functions can be looked up, and fail the test when called."""

    def __getattr__(self, name):
        def called(*args):
            raise AssertionError(f"{name} was called with arguments Python must refuse")
        return called


@pytest.fixture
def no_library(engine, monkeypatch):
    monkeypatch.setattr(engine, "lib", _OutOfReach())
    return engine


def _cuda_plane(rows=G, dtype=torch.float64, cols=M):
    """A [rows, cols] CUDA plane at the start of a backing of 4 * (G + 1) rows of float64 (or as many bytes)."""
    per_double = 8 // torch.empty((), dtype=dtype).element_size()
    return torch.zeros((4 * (G + 1) * per_double, cols), dtype=dtype, device="cuda")[:rows]


BAD_PLANES = {
    "one_row_more": lambda: (_cuda_plane(), _cuda_plane(), _cuda_plane(G + 1)),
    "float32": lambda: (_cuda_plane(), _cuda_plane(dtype=torch.float32), _cuda_plane()),
    "mixed_sides": lambda: (_cuda_plane(), np.zeros((G, M)), _cuda_plane()),
}


@pytest.mark.parametrize("bad", BAD_PLANES)
def test_bad_device_planes_are_refused_before_the_library(no_library, bad):
    eng = no_library
    Xd, csc = torch.from_numpy(X).cuda(), _compressed(X.T)
    for scores in (False, True):
        out = BAD_PLANES[bad]() + ((_cuda_plane(),) if scores else ())
        with pytest.raises(ValueError):
            eng.run_dense(Xd, 0, M, out=out)
        with pytest.raises(ValueError):
            eng.run_sparse("csc", *csc, (N, M), 0, M, out=out)
        with pytest.raises(ValueError):
            _lib.BoundMatrix(eng, None, (N, M), None).run(0, M, out=out)
    p, wrong = _cuda_plane(), BAD_PLANES[bad]()[1 if bad != "one_row_more" else 2]
    with pytest.raises(ValueError):
        eng.adjust_pvalues(p, "bh", out=wrong)
    with pytest.raises(ValueError):
        eng.ttest_from_moments(p, p, p, p, want=("p", "t"), out=(_cuda_plane(), wrong))
    with pytest.raises(ValueError):
        eng.group_moments(Xd, 0, M, out=(_cuda_plane(), wrong))
    with pytest.raises(ValueError):
        eng.group_stats(Xd, 0, M, out=(_cuda_plane(dtype=torch.int64), wrong))


@pytest.mark.parametrize("method", METHODS)
def test_expanded_device_matrix_is_refused_before_the_library(no_library, method):
    backing = torch.zeros(4 * N * M, dtype=torch.float32, device="cuda")
    for bad in (backing[:M].expand(N, M), backing.as_strided((N, M), (1, 1))):
        with pytest.raises(ValueError):
            METHODS[method](no_library, bad, 0, M)
