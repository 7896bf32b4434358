"""The cases of tests/csr_transpose_cases.py held to the restated plan of route_csr_transpose: every case sits on the switch, and on the
side of it, that its name says, and one entry / row / column / byte away the plan is the other one.  No GPU: a later edit of a case
that moves it off its switch fails here, wherever the suite runs."""
import numpy as np
import pytest

import csr_transpose_cases as cc


def _plan(name, **forms):
    return cc.case_plan(cc.make(name), **forms)


@pytest.mark.parametrize("name", cc.NAMES)
def test_a_case_is_what_its_name_says(name):
    c, e = cc.make(name), cc.EXPECT[name]
    m = cc.matrix(c)
    p = cc.case_plan(c)
    n_rows, n_cols = c.shape
    # a well-formed CSR matrix without duplicates, stored values never 0
    assert c.indptr[0] == 0 and c.indptr.size == n_rows + 1 and np.all(np.diff(c.indptr.astype(np.int64)) >= 0)
    assert c.indices.size == c.data.size == m.nnz <= cc.MAX_STORED and np.all(c.data != 0)
    assert c.indices.size == 0 or (c.indices.min() >= 0 and c.indices.max() < n_cols)
    assert np.unique(m.rows * n_cols + np.asarray(c.indices, dtype=np.int64)).size == m.nnz, "duplicate entries"
    assert c.labels.shape == (n_rows,) and 0 <= c.window[0] < c.window[1] <= n_cols
    assert (p.RB, p.ny, p.windows, p.gathers, p.scatters) == (e.RB, e.ny, e.windows, e.gathers, e.scatters), p
    assert p.n_blocks == -(-n_rows // p.RB)
    if e.piece is not None:
        assert max(p.pieces) == e.piece, p.pieces
    # the other forms of the same call: one workgroup per row block -- the same launches; the scatter form -- one per window, 32 768 wide
    q = cc.case_plan(c, no_split=True)
    assert q.ny == 1 and (q.RB, q.windows, q.gathers, q.scatters) == (p.RB, p.windows, p.gathers, p.scatters)
    s = cc.case_plan(c, no_gather=True)
    assert s.RB == 256 and s.gathers == 0 and s.scatters == len(s.windows) and all(w <= cc.NARROW for _, w in s.windows)
    assert sum(w for _, w in p.windows) == sum(w for _, w in s.windows) == c.window[1] - c.window[0]


def test_no_case_is_large():
    """From the shapes alone: no case holds more than about ten million stored entries."""
    for name in cc.NAMES:
        c = cc.make(name)
        if c.shape[0] * c.shape[1] > 5_000_000:     # (a case of fewer cells cannot hold more entries than that)
            assert cc.SHAPE_BOUND[name] <= cc.MAX_STORED, name
            assert int(c.indptr[-1]) <= 1.01 * cc.SHAPE_BOUND[name], name   # ... and the case is what that estimate describes
    assert max(cc.SHAPE_BOUND, key=cc.SHAPE_BOUND.get) == "ny-1-natural"


def test_sorted_means_no_strictly_descending_pair():
    ptr = np.array([0, 3, 5])
    assert cc.rows_sorted(np.array([1, 2, 9, 0, 4]), ptr)          # the pair (9, 0) straddles two rows
    assert cc.rows_sorted(np.array([1, 2, 2, 0, 4]), ptr)          # equal neighbours count as sorted
    assert not cc.rows_sorted(np.array([1, 3, 2, 0, 4]), ptr)
    assert not cc.rows_sorted(np.array([1, 2, 9, 4, 0]), ptr)      # in the last row
    assert cc.rows_sorted(np.array([5, 1]), np.array([0, 0, 1, 1, 2]))   # empty rows between


def test_rb_ladder():
    """Whole-matrix density exactly at 1/8, 1/4 and 1/2, and one stored entry more."""
    n_rows, n_cols = cc.LADDER_SHAPE
    for d, nnz in cc.LADDER.items():
        assert nnz / (n_rows * n_cols) == float(d)
        at, over = cc.make(f"rb-density-{d}-at"), cc.make(f"rb-density-{d}-over")
        assert int(at.indptr[-1]) == nnz and int(over.indptr[-1]) == nnz + 1
        a = set(zip(cc.matrix(at).rows.tolist(), at.indices.tolist()))
        assert a < set(zip(cc.matrix(over).rows.tolist(), over.indices.tolist())), "the same matrix with one entry more"
        assert cc.case_plan(over).RB * 2 == cc.case_plan(at).RB
    p = _plan("rb-density-0.5-over")
    assert (p.RB, p.n_blocks) == (64, 11)      # k_col_block_scan: its unrolled run of 8 blocks, then a remainder of 3
    assert cc.row_blocks(n_rows, n_cols, n_rows * n_cols, True)[0] == 64   # never below 64


def test_rows_against_rb():
    assert _plan("rows-1").n_blocks == 1 and cc.make("rows-1").shape[0] == 1
    assert _plan("rows-rb").n_blocks == 1 and cc.make("rows-rb").shape[0] == _plan("rows-rb").RB
    p = _plan("rows-rb+1")
    assert p.n_blocks == 2 and cc.make("rows-rb+1").shape[0] == p.RB + 1       # a last block of one row ...
    assert cc.make("rows-rb+1").indptr[-1] > cc.make("rows-rb+1").indptr[-2]   # ... which stores something
    c = cc.make("window-empty")
    assert cc.matrix(c).stored_in(*c.window[:1], c.window[1] - c.window[0]) == 0 and int(c.indptr[-1]) > 0
    for col in (c.window[0] - 1, c.window[1]):
        assert np.any(c.indices == col)


def test_split_factor():
    assert [cc.split_factor(n) for n in (1, 128, 136, 137, 512, 513, 682, 683, 1023, 1024, 2047, 2048, 5000)] == \
        [16, 16, 16, 15, 4, 4, 4, 3, 3, 2, 2, 1, 1]
    assert cc.split_factor(40, no_split=True) == 1
    assert (_plan("ny-16-136-blocks").n_blocks, _plan("ny-15-137-blocks").n_blocks) == (136, 137)
    assert cc.make("ny-15-137-blocks").shape[0] == cc.make("ny-16-136-blocks").shape[0] + 1 == 69633
    assert (_plan("ny-4").n_blocks, _plan("ny-2").n_blocks, _plan("ny-1-natural").n_blocks) == (513, 1024, 2048)
    assert cc.make("ny-4").shape[0] % 512 == 1                                  # (its last block is one row)
    assert cc.row_blocks(2047 * 64, 130, int(2047 * 64 * 130 * 0.52), True) == (64, 2047)   # one block fewer than ny-1-natural: ny = 2
    # how the tiles fall to the stretches
    assert cc.stretches(130, 4) == [(0, 64), (64, 128), (128, 130), (192, 130)]      # 1 / 1 / 1 / empty
    assert cc.stretches(130, 2) == [(0, 128), (128, 130)]                           # two tiles, then one tile of two columns
    assert cc.stretches(130, 1) == [(0, 130)]
    s = cc.stretches(1000, 16)
    assert len(s) == 16 and all(hi - lo == 64 for lo, hi in s[:15]) and s[15] == (960, 1000)   # tiles_all = 16: one tile each
    assert [hi > lo for lo, hi in cc.stretches(130, 16)] == [True] * 3 + [False] * 13
    assert [hi > lo for lo, hi in cc.stretches(130, 15)] == [True] * 3 + [False] * 12
    for name, ny in (("ny-4", 4), ("ny-2", 2), ("ny-1-natural", 1)):   # every stretch that has columns has entries
        c = cc.make(name)
        for lo, hi in cc.stretches(130, ny):
            assert hi <= lo or cc.matrix(c).stored_in(lo, hi - lo) > 0


def test_register_window():
    c = cc.make("regwin-last-full")
    m = cc.matrix(c)
    per_row = cc.window_entries_per_row(m, *c.window)
    for row, n in cc.C_INSIDE.items():
        assert per_row[row] == n, row
    assert set(per_row[:11].tolist()) >= {0, 1, 15, 16, 17, 32, 33}
    lb, ub = c.window
    row = lambda r: c.indices[c.indptr[r]:c.indptr[r + 1]]
    assert row(1).max() == lb - 1 and row(2).min() == ub                          # wholly left of / right of the window
    assert row(3).tolist() == [lb - 1, lb] and row(4).tolist() == [ub - 1, ub]
    assert np.count_nonzero((row(10) >= lb) & (row(10) < lb + cc.TILE)) > cc.REG_WINDOW
    last = c.shape[0] - 1
    assert c.shape[0] % 4 == 0 and int(c.indptr[-1]) == c.indices.size
    for ny in (16, 1):
        assert cc.refill_trace(m, lb, ub, ny, 10)[0] == [16, 5]                   # refilled in the middle of the first tile
        assert cc.refill_trace(m, lb, ub, ny, last)[0] == [16, 16]                # the matrix ends on a full refill
    short = cc.make("regwin-last-short")
    ms = cc.matrix(short)
    assert int(short.indptr[-1]) == int(c.indptr[-1]) + 1 and short.indices[-1] == ub - 1
    assert cc.refill_trace(ms, lb, ub, 1, last)[0] == [16, 16, 1]                  # the short path, one entry left
    # split over the tiles [30, 94), [94, 158), [158, 170): the first workgroup stops inside its second refill, the third one's only refill is that entry
    assert cc.refill_trace(ms, lb, ub, 16, last) == [[16, 16], [13], [1]]
    assert cc.refill_trace(m, lb, ub, 16, 0) == [[], [], []] and cc.refill_trace(m, lb, ub, 16, 2)[0] == [4]
    for name, width in (("width-63", 63), ("width-64", 64), ("width-65", 65)):
        w = cc.make(name)
        assert w.window == (lb, lb + width) and np.array_equal(w.indices, c.indices)
        edge = (lb - 1, lb, lb + width - 1, lb + width)
        assert all(np.any(w.indices == col) for col in edge), name
    for name in cc.NAMES:
        if name.startswith("types-"):
            t = cc.make(name)
            _, v, i = name.split("-")
            assert (t.data.dtype, t.indices.dtype, t.indptr.dtype) == (np.dtype(v), np.dtype(i), np.dtype(i))
            assert np.array_equal(t.indices, c.indices) and np.array_equal(t.indptr, c.indptr)
            if t.data.dtype.kind == "i":
                assert t.data.min() >= 1000                                       # far above the count tables
            if t.data.dtype == np.float64:
                assert np.any(t.data.astype(np.float32).astype(np.float64) != t.data)   # float64 proper: not narrowed to float32
    assert len([n for n in cc.NAMES if n.startswith("types-")]) + 1 == len(cc.VALUE_TYPES) * len(cc.INDEX_TYPES) == 8


def test_staging_capacity():
    lo, hi = cc.make("stage-8192"), cc.make("stage-8193")
    assert int(hi.indptr[-1]) == int(lo.indptr[-1]) + 1
    pl, ph = cc.case_plan(lo), cc.case_plan(hi)
    assert (max(pl.pieces), max(ph.pieces)) == (cc.CAP, cc.CAP + 1) and pl.RB == ph.RB == 256
    assert (pl.gathers, pl.scatters, ph.gathers, ph.scatters) == (1, 0, 1, 1)
    # every other piece is far from the capacity: the named piece is the one that decides
    m = cc.matrix(lo)
    c = np.asarray(lo.indices, dtype=np.int64)
    pieces = np.bincount((m.rows // 256) * 4 + c // 64)
    assert np.sort(pieces)[-2] < cc.CAP // 2
    p = _plan("stage-rb128-full-piece")
    assert p.RB == 128 and max(p.pieces) == 128 * 64 == cc.CAP and p.scatters == 0


def test_window_width():
    for cols, windows in ((65536, 1), (65537, 2)):
        s, u = cc.make(f"cols-{cols}-sorted"), cc.make(f"cols-{cols}-descending-pair")
        assert s.shape == u.shape == (40, cols) and cc.matrix(s).in_order and not cc.matrix(u).in_order
        assert np.array_equal(np.sort(s.indices[s.indptr[11]:s.indptr[12]]), np.sort(u.indices[u.indptr[11]:u.indptr[12]]))
        assert np.count_nonzero(s.indices != u.indices) == 2                       # one pair changed places
        assert len(cc.case_plan(s).windows) == windows and np.any(s.indices == cols - 1)
    assert _plan("cols-65537-sorted").windows[-1] == (65536, 1)


def test_overflow_above_32768_columns():
    for name, window in (("recut-piece-in-first", 0), ("recut-piece-in-second", 1)):
        c = cc.make(name)
        m = cc.matrix(c)
        p = cc.case_plan(c)
        assert m.largest_piece(0, 40000, p.RB) > cc.CAP                             # the whole window's gather overflows ...
        assert p.windows == [(0, 32768), (32768, 7232)]                             # ... it is cut at 32 768 ...
        assert [x > cc.CAP for x in p.pieces] == [window == 0, window == 1]         # ... and one of the two is redone by the scatter form
        assert (p.gathers, p.scatters) == (3, 1)


def test_halving():
    for name, width in (("halve-200", 200), ("halve-201", 201)):
        c = cc.make(name)
        m = cc.matrix(c)
        inside = m.stored_in(0, width)
        assert c.scratch_bytes == inside * (c.data.dtype.itemsize + 4) - 1
        p = cc.case_plan(c)
        assert p.halvings == 1
        one_more = cc.plan(m, 0, width, scratch_bytes=c.scratch_bytes + 1)          # one byte more: the window as a whole
        assert one_more.halvings == 0 and one_more.windows == [(0, width)]
    c = cc.make("halve-floor")
    p = cc.case_plan(c)
    assert c.scratch_bytes < 8 and p.halvings == 1 and p.windows == [(0, 64), (64, 36)]   # over the budget at every width: 64 is the floor
    assert cc.plan(cc.matrix(c), 0, 65, scratch_bytes=c.scratch_bytes).windows == [(0, 64), (64, 1)]
    assert cc.plan(cc.matrix(c), 0, 64, scratch_bytes=c.scratch_bytes).halvings == 0


def test_sorted_detection():
    s, u = cc.make("sorted-last-row"), cc.make("descending-pair-in-last-row")
    assert s.shape[0] % 4 != 0 and s.shape == u.shape
    differ = np.flatnonzero(s.indices != u.indices)
    assert differ.tolist() == [s.indices.size - 2, s.indices.size - 1]               # the last two entries of the last row
    assert cc.matrix(s).in_order and not cc.matrix(u).in_order
    assert set(cc.BOUND) == {"sorted-last-row", "descending-pair-in-last-row"}
