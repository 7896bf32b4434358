"""The argument checks and the input staging that the per-group passes share, through the C ABI (no Engine wrapper).

illico_group_stats_{dense,csc,csr,bound}, illico_group_moments_{dense,csc,csr,bound}, illico_group_value_hists_{dense,csc,csr} and
illico_pairwise_ranked_{dense,csc} take a matrix the same way: every bad call below must give the same code and message from each of
them, the earlier check winning where two faults meet (the ranked pair family looks at the matrix's arrays before its outputs, the
others after: its rows say so), and a window that starts past column 0 must read the right entries of a host CSC matrix.  The matrix
is 8 cells x 6 genes of small integers, two interleaved groups of 4 cells: every expected number is exact and computed here.  The two
all-pairs entry points, illico_pairwise_from_hists and illico_pairwise_ranked_dense, select their groups the same way: one set of
refusals, one text each.
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
STATS, MOMENTS, HISTS, RANKED = "group_stats", "group_moments", "group_value_hists", "pairwise_ranked"
ENTRIES = [(fam, shape) for fam in (STATS, MOMENTS, HISTS) for shape in ("dense", "csc", "csr", "bound") if (fam, shape) != (HISTS, "bound")]
ENTRIES += [(RANKED, "dense"), (RANKED, "csc")]
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

    def set_groups(self, codes=CODES):
        enc = codes.astype(np.int64)
        cnt = np.bincount(codes).astype(np.int64)
        idx = np.argsort(codes, kind="stable").astype(np.int64)
        ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        assert self.lib.illico_set_groups(self.ctx, enc.ctypes.data, cnt.ctypes.data, idx.ctypes.data, ptr.ctypes.data, N, cnt.size, -1) == 0

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
        """One call of illico_<fam>_<shape> with host outputs; returns (code, message, output arrays).  The ranked pair family: all
        groups, the window's per-group sums on the side of the matrix, two-sided; its outputs are p, U, fc, z and left."""
        W = max(ub - lb, 1)
        if fam == HISTS:
            outs = [np.zeros((G, W, 256), np.uint32), np.zeros(W, np.uint32)]
        elif fam == RANKED:
            outs = [np.zeros((G, G, W)) for _ in range(4)] + [np.zeros(W, np.uint32)]
        else:
            outs = [np.zeros((G, W), k) for k in ((np.int64, np.float64) * 2 if fam == STATS else (np.float64,) * 4)]
        ptrs = [None if null_out else o.ctypes.data for o in outs]
        flags |= self.flag[side]
        if fam == RANKED:
            import torch
            sums = np.zeros((G, W))
            if 0 <= lb < ub <= M:
                sums[:, :ub - lb] = np.stack([X[CODES == g, lb:ub].sum(0) for g in range(G)])
            sums = torch.from_numpy(sums).cuda() if side == "device" else sums
            tail = [None, 0, sums.data_ptr() if side == "device" else sums.ctypes.data, W, flags, _lib.ALTERNATIVES["two-sided"], *ptrs[:4],
                    W if out_ld is None else out_ld, ptrs[4]]
        else:
            tail = [flags] + ptrs + ([] if fam == HISTS else [W if out_ld is None else out_ld])
        fn = getattr(self.lib, f"illico_{fam}_{shape}")
        if shape == "dense":
            rc = fn(self.ctx, None if null_in else self.dense[side], dtype, n_rows, n_cols, ld, lb, ub, *tail)
        elif shape == "bound":
            rc = fn(self.ctx, handle or self.bound[side], lb, ub, *tail)
        else:
            d, i, p = self.sparse[side][shape]
            rc = fn(self.ctx, d, dtype, None if null_in else i, p if indptr is None else indptr.ctypes.data, idx, n_rows, n_cols, lb, ub, *tail)
        if fam == RANKED and side == "device":
            torch.cuda.synchronize()   # (sums is this call's own tensor)
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
    if fam == RANKED:  # U[r, g] of group g against reference r from doubled midranks among the 8 cells of the two: integers throughout
        n = N // G
        U = np.full((G, G, ub - lb), n * n / 2)
        for j, col in enumerate(Xw.T):
            rank2 = np.array([2 * (col < v).sum() + (col == v).sum() + 1 for v in col])
            for r, g in ((0, 1), (1, 0)):
                U[r, g, j] = (2 * n * n + n * (n + 1) - rank2[CODES == g].sum()) / 2
        return [None, U, None, None, np.zeros(ub - lb, np.uint32)]  # (p, the fold change and z are not this file's business)
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
    null_planes = {HISTS: "null out_H / out_flags", RANKED: "null sums, output plane or out_left"}.get(fam, "all four output planes are null")
    null_arrays = "null X" if shape == "dense" else "null sparse array"
    if shape != "bound":  # (a bound matrix brings its own shape and dtypes)
        _refused(call(n_rows=7), _lib.ERR_NO_GROUPS, "X has 7 rows but the groups describe 8 cells")
        _refused(call(n_rows=7, dtype=9), _lib.ERR_NO_GROUPS, "X has 7 rows")  # the earlier check wins
        _refused(call(dtype=9), _lib.ERR_DTYPE, "unsupported dtype code 9")
        _refused(call(null_in=True), _lib.ERR_ARG, null_arrays)
        _refused(call(null_in=True, null_out=True), _lib.ERR_ARG, null_arrays if fam == RANKED else null_planes)  # (the ranked family: arrays first)
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
    if fam == RANKED:  # (its pitches before its null planes)
        _refused(call(lb=1, ub=4, out_ld=1), _lib.ERR_ARG, "out_ld smaller than the window")
        _refused(call(lb=1, ub=4, out_ld=1, null_out=True), _lib.ERR_ARG, "out_ld smaller than the window")
        _refused(call(lb=1, ub=4, out_ld=1, null_in=True), _lib.ERR_ARG, null_arrays)
    elif fam != HISTS:
        _refused(call(lb=1, ub=4, out_ld=1), _lib.ERR_ARG, "out_ld smaller than the chunk width")
        _refused(call(lb=1, ub=4, out_ld=1, null_out=True), _lib.ERR_ARG, null_planes)
    if fam == MOMENTS:
        _refused(call(flags=_lib.FLAG_LOG1P), _lib.ERR_ARG, "ILLICO_FLAG_LOG1P")
        _refused(call(flags=_lib.FLAG_LOG1P, null_out=True), _lib.ERR_ARG, "ILLICO_FLAG_LOG1P")
        _refused(call(flags=_lib.FLAG_LOG1P, lb=4, ub=2), _lib.ERR_BOUNDS, "Invalid chunk bounds: (4, 2)")
    else:
        assert call(flags=_lib.FLAG_LOG1P, lb=2, ub=2)[0] == 0  # (an empty window: accepted, nothing computed)


@pytest.mark.parametrize("fam", (STATS, MOMENTS, HISTS, RANKED))
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
            if w is not None:
                np.testing.assert_array_equal(g, w)
        grew = env.input_bytes() - before
        if side == "host" and shape == "csc":    # the window's entries and its W + 1 pointers
            nnz = int(CSC[2][UB] - CSC[2][LB])
            assert grew == nnz * (4 + 4) + (UB - LB + 1) * 4
        elif side == "host" and shape == "csr":  # every row
            assert grew == int(CSR[2][N]) * (4 + 4) + (N + 1) * 4
        elif side == "device" or shape == "bound":
            assert grew == 0


# ---- one selection, two entry points: 3 groups over the 8 cells, one gene ----
CODES3 = np.array([0, 1, 2, 0, 1, 2, 0, 1])
SENTINEL = -7.0


@pytest.fixture(scope="module")
def env3():
    e = Env()
    e.set_groups(CODES3)
    yield e
    e.close()


def _pair_call(e, entry, sel, alternative):
    """(code, message, the four planes and left) of one call over gene 1 with host planes pre-filled with SENTINEL."""
    planes = [np.full((3, 3, 1), SENTINEL) for _ in range(4)]
    left = np.full(1, 0xABCD, np.uint32)
    sel = np.array(sel, np.int64)
    tail = [sel.ctypes.data, sel.size, None, 0, 0, alternative, *[q.ctypes.data for q in planes], 1]
    if entry == "illico_pairwise_from_hists":
        cnt = np.bincount(CODES3).astype(np.int64)
        H = np.stack([np.bincount(X[CODES3 == g, 1], minlength=256) for g in range(3)]).astype(np.uint32).reshape(3, 1, 256)
        fl = np.zeros(1, np.uint32)
        rc = e.lib.illico_pairwise_from_hists(e.ctx, H.ctypes.data, fl.ctypes.data, cnt.ctypes.data, 3, 1, *tail)
    else:
        sums = np.array([[float(X[CODES3 == g, 1].sum())] for g in range(3)])
        tail[2:4] = [sums.ctypes.data, 1]
        rc = e.lib.illico_pairwise_ranked_dense(e.ctx, e.dense["host"], _lib.I32, N, M, M, 1, 2, *tail, left.ctypes.data)
    return rc, e.err(), planes + [left]


@pytest.mark.parametrize("entry", ["illico_pairwise_from_hists", "illico_pairwise_ranked_dense"])
def test_one_pair_selection_for_both_entry_points(env3, entry):
    two_sided = _lib.ALTERNATIVES["two-sided"]
    rc, msg, _ = _pair_call(env3, entry, [2, 0], two_sided)   # (the call as such is a good one)
    assert rc == 0, msg
    for sel, alt, code, text in [([1], two_sided, _lib.ERR_ARG, "1 groups selected: a pair needs two"),
                                 ([1, 3], two_sided, _lib.ERR_ARG, "sel[1] = 3 is no group id (0 .. 2)"),
                                 ([1, -1], two_sided, _lib.ERR_ARG, "sel[1] = -1 is no group id (0 .. 2)"),
                                 ([1, 2, 1], two_sided, _lib.ERR_ARG, "group 1 is selected twice"),
                                 ([1, 2], 7, _lib.ERR_ALTERNATIVE, "Unsupported alternative hypothesis code: 7")]:
        rc, msg, outs = _pair_call(env3, entry, sel, alt)
        assert (rc, msg) == (code, text), (sel, alt, rc, msg)   # the whole text: the same from both entry points
        assert all((q == SENTINEL).all() for q in outs[:4]) and outs[4][0] == 0xABCD
