"""The argument checks and the input staging that the three per-group passes share, through the C ABI (no Engine wrapper).

illico_group_stats_{dense,csc,csr,bound}, illico_group_moments_{dense,csc,csr,bound} and illico_group_value_hists_{dense,csc,csr}
take a matrix the same way: every bad call below must give the same code and message from each of them, the earlier check winning
where two faults meet, and a window that starts past column 0 must read the right entries of a host CSC matrix.  The matrix is
8 cells x 6 genes of small integers, two interleaved groups of 4 cells: every expected number is exact and computed here.
"""
import ctypes

import numpy as np
import pytest

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
STATS, MOMENTS, HISTS = "group_stats", "group_moments", "group_value_hists"
ENTRIES = [(fam, shape) for fam in (STATS, MOMENTS, HISTS) for shape in ("dense", "csc", "csr", "bound") if (fam, shape) != (HISTS, "bound")]
SIDES = ("host", "device")
LB, UB = 1, 5  # the window of the good calls: a host CSC matrix is uploaded from its entry indptr[1] on


def _compressed(A):
    """(data, indices, indptr) of the rows of A, int32: the non-zero entries only."""
    rows = [np.flatnonzero(r) for r in A]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return np.concatenate([A[k][r] for k, r in enumerate(rows)]).astype(np.int32), np.concatenate(rows).astype(np.int32), indptr


CSR, CSC = _compressed(X), _compressed(X.T)


class Env:
    """One context, and the matrix in every layout on both sides."""

    def __init__(self):
        import torch
        self.lib = _lib.load()
        self.ctx = ctypes.c_void_p()
        assert self.lib.illico_ctx_create(0, ctypes.byref(self.ctx)) == 0 and self.ctx.value
        dev = lambda a: torch.from_numpy(a).cuda()
        self.keep = {"host": (X, CSC, CSR), "device": (dev(X), tuple(dev(a) for a in CSC), tuple(dev(a) for a in CSR))}
        torch.cuda.synchronize()
        ptr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
        self.dense = {s: ptr(k[0]) for s, k in self.keep.items()}
        self.sparse = {s: {"csc": [ptr(a) for a in k[1]], "csr": [ptr(a) for a in k[2]]} for s, k in self.keep.items()}
        self.flag = {"host": 0, "device": _lib.FLAG_INPUT_DEVICE}
        self.bound = {s: self.bind("csc", s) for s in SIDES}  # host: uploaded once; device: the tensors adopted
        self.bound_csr = self.bind("csr", "host")

    def bind(self, fmt, side):
        h = ctypes.c_void_p()
        fn = self.lib.illico_csc_bind if fmt == "csc" else self.lib.illico_csr_bind
        assert fn(self.ctx, *self.sparse[side][fmt][:1], _lib.I32, *self.sparse[side][fmt][1:], _lib.IDX_I32, N, M, self.flag[side], ctypes.byref(h)) == 0
        return h

    def set_groups(self):
        enc = CODES.astype(np.int64)
        cnt = np.bincount(CODES).astype(np.int64)
        idx = np.argsort(CODES, kind="stable").astype(np.int64)
        ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        assert self.lib.illico_set_groups(self.ctx, enc.ctypes.data, cnt.ctypes.data, idx.ctypes.data, ptr.ctypes.data, N, G, -1) == 0

    def err(self):
        return self.lib.illico_last_error(self.ctx).decode()

    def input_bytes(self):
        n = ctypes.c_int64(0)
        assert self.lib.illico_profile_input_bytes(self.ctx, ctypes.byref(n)) == 0
        return n.value

    def close(self):
        assert self.lib.illico_ctx_destroy(self.ctx) == 0

    def call(self, fam, shape, side="host", *, n_rows=N, n_cols=M, lb=0, ub=M, dtype=_lib.I32, idx=_lib.IDX_I32, flags=0, ld=M, out_ld=None,
             null_in=False, null_out=False, indptr=None, handle=None):
        """One call of illico_<fam>_<shape> with host outputs; returns (code, message, output arrays)."""
        W = max(ub - lb, 1)
        if fam == HISTS:
            outs = [np.zeros((G, W, 256), np.uint32), np.zeros(W, np.uint32)]
        else:
            outs = [np.zeros((G, W), k) for k in ((np.int64, np.float64) * 2 if fam == STATS else (np.float64,) * 4)]
        tail = [None if null_out else o.ctypes.data for o in outs] + ([] if fam == HISTS else [W if out_ld is None else out_ld])
        fn = getattr(self.lib, f"illico_{fam}_{shape}")
        flags |= self.flag[side]
        if shape == "dense":
            rc = fn(self.ctx, None if null_in else self.dense[side], dtype, n_rows, n_cols, ld, lb, ub, flags, *tail)
        elif shape == "bound":
            rc = fn(self.ctx, handle or self.bound[side], lb, ub, flags, *tail)
        else:
            d, i, p = self.sparse[side][shape]
            rc = fn(self.ctx, d, dtype, None if null_in else i, p if indptr is None else indptr.ctypes.data, idx, n_rows, n_cols, lb, ub, flags, *tail)
        return rc, self.err(), outs


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.set_groups()
    yield e
    e.close()


def _expected(fam, lb, ub):
    Xw = X[:, lb:ub].astype(np.int64)
    per_group = lambda f: np.stack([f(Xw[CODES == g]) for g in range(G)])
    if fam == HISTS:
        return [per_group(lambda a: np.stack([np.bincount(col, minlength=256) for col in a.T])).astype(np.uint32), np.zeros(ub - lb, np.uint32)]
    s = per_group(lambda a: a.sum(0)).astype(np.float64)
    if fam == STATS:
        nnz = per_group(lambda a: (a != 0).sum(0))
        return [nnz, s, nnz.sum(0) - nnz, s.sum(0) - s]
    q = per_group(lambda a: (a * a).sum(0)).astype(np.float64)
    return [s, q, s.sum(0) - s, q.sum(0) - q]


def _refused(got, code, text):
    rc, msg, _ = got
    assert rc == code and text in msg, (rc, msg)


def test_refused_before_set_groups():
    e = Env()
    try:
        for fam, shape in ENTRIES:
            for side in SIDES:
                _refused(e.call(fam, shape, side), _lib.ERR_NO_GROUPS, "illico_set_groups has not been called")
    finally:
        e.close()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("fam,shape", ENTRIES)
def test_bad_calls(env, fam, shape, side):
    call = lambda **kw: env.call(fam, shape, side, **kw)
    null_planes = "null out_H / out_flags" if fam == HISTS else "all four output planes are null"
    if shape != "bound":  # (a bound matrix brings its own shape and dtypes)
        _refused(call(n_rows=7), _lib.ERR_NO_GROUPS, "X has 7 rows but the groups describe 8 cells")
        _refused(call(n_rows=7, dtype=9), _lib.ERR_NO_GROUPS, "X has 7 rows")  # the earlier check wins
        _refused(call(dtype=9), _lib.ERR_DTYPE, "unsupported dtype code 9")
        _refused(call(null_in=True), _lib.ERR_ARG, "null X" if shape == "dense" else "null sparse array")
        _refused(call(null_in=True, null_out=True), _lib.ERR_ARG, null_planes)
    if shape in ("csc", "csr"):
        _refused(call(idx=5), _lib.ERR_DTYPE, "unsupported index dtype code 5")
        _refused(call(dtype=9, idx=5), _lib.ERR_DTYPE, "unsupported dtype code 9")
    if shape == "dense":
        _refused(call(ld=5), _lib.ERR_ARG, "ld smaller than n_cols")
        _refused(call(idx=5, ld=5), _lib.ERR_ARG, "ld smaller than n_cols")  # (a dense call has no index dtype to refuse)
    for lb, ub in ((-1, 3), (0, 7), (4, 2)):
        _refused(call(lb=lb, ub=ub), _lib.ERR_BOUNDS, f"Invalid chunk bounds: ({lb}, {ub}) for data with 6 columns.")
    _refused(call(lb=-1, ub=3, null_out=True), _lib.ERR_BOUNDS, "Invalid chunk bounds: (-1, 3)")  # the earlier check wins
    _refused(call(null_out=True), _lib.ERR_ARG, null_planes)
    if fam != HISTS:
        _refused(call(lb=1, ub=4, out_ld=1), _lib.ERR_ARG, "out_ld smaller than the chunk width")
        _refused(call(lb=1, ub=4, out_ld=1, null_out=True), _lib.ERR_ARG, null_planes)
    if fam == MOMENTS:
        _refused(call(flags=_lib.FLAG_LOG1P), _lib.ERR_ARG, "ILLICO_FLAG_LOG1P")
        _refused(call(flags=_lib.FLAG_LOG1P, null_out=True), _lib.ERR_ARG, "ILLICO_FLAG_LOG1P")
        _refused(call(flags=_lib.FLAG_LOG1P, lb=4, ub=2), _lib.ERR_BOUNDS, "Invalid chunk bounds: (4, 2)")
    else:
        assert call(flags=_lib.FLAG_LOG1P, lb=2, ub=2)[0] == 0  # (an empty window: accepted, nothing computed)


@pytest.mark.parametrize("fam", (STATS, MOMENTS, HISTS))
def test_host_csc_indptr_decreasing_in_the_window(env, fam):
    bad = np.array([0, 5, 3, 3, 3, 3, 3], dtype=np.int32)  # the window [1, 2) would run from entry 5 back to entry 3
    before = env.input_bytes()
    _refused(env.call(fam, "csc", lb=1, ub=2, indptr=bad), _lib.ERR_ARG, "indptr is not non-decreasing")
    assert env.input_bytes() == before


def test_bound_handle_used_after_release(env):
    h = env.bind("csc", "host")
    assert env.call(STATS, "bound", handle=h)[0] == 0
    assert env.lib.illico_matrix_release(env.ctx, h) == 0
    for fam in (STATS, MOMENTS):
        _refused(env.call(fam, "bound", handle=h), _lib.ERR_ARG, "the matrix handle does not belong to this context (or was released)")


def test_bound_handle_used_after_release_by_the_wilcoxon_entry_points(env):
    """illico_run_bound, illico_run_bound_ex and illico_matrix_touch look the handle up in the context's list before they read it."""
    h = env.bind("csr", "host")
    p, u, fc, z = (np.zeros((G, M)) for _ in range(4))
    planes = [a.ctypes.data for a in (p, u, fc)]
    assert env.lib.illico_run_bound(env.ctx, h, 0, M, 0, 0, *planes, M) == 0
    assert env.lib.illico_matrix_release(env.ctx, h) == 0
    for rc in (lambda: env.lib.illico_run_bound(env.ctx, h, 0, M, 0, 0, *planes, M),
               lambda: env.lib.illico_run_bound_ex(env.ctx, h, 0, M, 0, 0, *planes, z.ctypes.data, M),
               lambda: env.lib.illico_matrix_touch(env.ctx, h),
               lambda: env.lib.illico_matrix_release(env.ctx, h)):
        _refused((rc(), env.err(), None), _lib.ERR_ARG, "the matrix handle does not belong to this context (or was released)")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("fam,shape", ENTRIES)
def test_good_call_on_an_inner_window(env, fam, shape, side):
    want = _expected(fam, LB, UB)
    handles = [env.bound[side]] + ([env.bound_csr] if shape == "bound" and side == "host" else [])
    for h in handles:
        before = env.input_bytes()
        rc, msg, got = env.call(fam, shape, side, lb=LB, ub=UB, handle=h)
        assert rc == 0, msg
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        grew = env.input_bytes() - before
        if side == "host" and shape == "csc":    # the window's entries and its W + 1 pointers
            nnz = int(CSC[2][UB] - CSC[2][LB])
            assert grew == nnz * (4 + 4) + (UB - LB + 1) * 4
        elif side == "host" and shape == "csr":  # every row
            assert grew == int(CSR[2][N]) * (4 + 4) + (N + 1) * 4
        elif side == "device" or shape == "bound":
            assert grew == 0
