"""The plan of the CSR -> CSC device transposition restated, and one input on each side of every switch of that plan.

route_csr_transpose (illico_amd/csrc/sparse_driver.h:958-1048) turns a column window of a CSR matrix into CSC on the device: a counting
pass (k_csr_block_count, k_col_block_scan, k_gene_base_scan), then k_csr_tile_gather (rows in order) or k_csr_block_scatter (rows out of
order, or a piece beyond the gather form's LDS staging), kernels_sparse.h:266-479.  The CSC routes then rank the result, so an entry that
lands in the wrong column or under the wrong row gives a plausible, wrong statistic.

First half: what the driver decides for a matrix and a window, in plain numpy, with the lines it restates.  Second half: the cases, each
named for the switch it sits on and for its side.  EXPECT holds, per case, what the case is named for; tests/test_csr_transpose_cases_host.py
holds the cases to it through the model, tests/test_gpu_csr_transpose_edges.py holds the build to the model through the profiler's launch
counts of the two pass-2 families, and the planes to the CPU oracle.

Imports numpy, scipy and the oracle only.  Large cases are built as CSR arrays directly; no dense array of a case's shape is formed.
"""
import zlib
from collections import namedtuple

import numpy as np
from scipy import sparse

import oracle

REF_LABEL = "non-targeting"
CAP = 8192            # sparse_driver.h:979 -- LDS staging entries of k_csr_tile_gather (kernels_sparse.h:447: total > cap raises overflow)
TILE = 64             # kernels_sparse.h:360 TRG_COLS
RB_MAX = 512          # sparse_driver.h:983 TRG_NT * TRG_RPT (kernels_sparse.h:361-362)
SPLIT_BLOCKS = 2048   # sparse_driver.h:988
WIDE, NARROW = 65536, 32768   # sparse_driver.h:991 -- 16-bit counters of the counting pass / 32-bit cursors of the scatter form
FLOOR = 64            # sparse_driver.h:1014-1015
REG_WINDOW = 16       # kernels_sparse.h:364 TRG_WIN
DEFAULT_SCRATCH = 1 << 30   # what the GPU module sets on its own engine; every case without a budget of its own fits it
MAX_STORED = 10_000_000


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def rows_sorted(indices, indptr):
    """k_csr_sorted_check (kernels_sparse.h:678-707): bad when a < b for an entry a and the entry b before it IN THE SAME ROW -- strict, so
    equal neighbours count as sorted."""
    indices, indptr = np.asarray(indices, dtype=np.int64), np.asarray(indptr, dtype=np.int64)
    if indices.size < 2:
        return True
    desc = indices[1:] < indices[:-1]
    starts = indptr[1:-1]                       # entry k = indptr[r] starts a row: the pair (k - 1, k) straddles two rows
    starts = starts[(starts > 0) & (starts < indices.size)]
    desc[starts - 1] = False
    return not bool(desc.any())


def row_blocks(n_rows, n_cols, nnz, in_order):
    """(RB, n_blocks): sparse_driver.h:980-986.  The density is the WHOLE matrix's (sparse_driver.h:715), whatever window the call names."""
    rb = 256
    if in_order:
        density = float(nnz) / (float(max(n_rows, 1)) * float(max(n_cols, 1)))
        per_row = max(density * TILE, 1e-9)
        rb = RB_MAX
        while rb > 64 and rb * per_row > CAP // 2:
            rb >>= 1
    return rb, (n_rows + rb - 1) // rb


def split_factor(n_blocks, no_split=False):
    """ny, sparse_driver.h:988: the y extent of the launches of k_csr_block_count and k_csr_tile_gather."""
    return 1 if (n_blocks >= SPLIT_BLOCKS or no_split) else min(16, (SPLIT_BLOCKS + n_blocks - 1) // n_blocks)


def stretches(width, ny):
    """The tiles each y of k_csr_tile_gather sweeps (kernels_sparse.h:387-388): [(first column, end column)] relative to the window; an
    empty stretch has end <= first."""
    tiles_all = (width + TILE - 1) // TILE
    tiles_per = (tiles_all + ny - 1) // ny
    return [(y * tiles_per * TILE, min(width, y * tiles_per * TILE + tiles_per * TILE)) for y in range(ny)]


Plan = namedtuple("Plan", ["in_order", "RB", "n_blocks", "ny", "windows", "pieces", "halvings", "gathers", "scatters"])
# windows: [(first column, width)] actually transposed, in order; pieces: the largest (row block, 64-column tile) piece of each;
# halvings: how often a window was cut in two for the scratch budget; gathers / scatters: launches of the two pass-2 kernels


class Matrix:
    """What the model needs of a CSR matrix, computed once: per stored entry its row and column."""

    def __init__(self, data, indices, indptr, shape):
        self.data, self.indices, self.indptr, self.shape = data, indices, indptr, tuple(shape)
        self.nnz = int(indptr[-1])
        self.in_order = rows_sorted(indices, indptr)
        self._rows = None

    @property
    def rows(self):
        if self._rows is None:
            self._rows = np.repeat(np.arange(self.shape[0], dtype=np.int64), np.diff(np.asarray(self.indptr, dtype=np.int64)))
        return self._rows

    def stored_in(self, w0, wn):
        c = np.asarray(self.indices)
        return int(np.count_nonzero((c >= w0) & (c < w0 + wn)))

    def largest_piece(self, w0, wn, rb):
        c = np.asarray(self.indices, dtype=np.int64)
        inside = (c >= w0) & (c < w0 + wn)
        if not inside.any():
            return 0
        n_tiles = (wn + TILE - 1) // TILE
        key = (self.rows[inside] // rb) * n_tiles + (c[inside] - w0) // TILE   # tiles are counted from the WINDOW's first column
        return int(np.bincount(key).max())


def plan(m, col_lb, col_ub, *, value_bytes=4, scratch_bytes=DEFAULT_SCRATCH, no_split=False, no_gather=False):
    """The loop of route_csr_transpose (sparse_driver.h:970-1046) for columns [col_lb, col_ub) of `m`."""
    n_rows, n_cols = m.shape
    in_order = m.in_order and not no_gather                       # :970-978
    rb, n_blocks = row_blocks(n_rows, n_cols, m.nnz, in_order)    # :980-986
    ny = split_factor(n_blocks, no_split)                         # :988
    wmax = min(col_ub - col_lb, WIDE if (in_order and rb <= 512) else NARROW)   # :991
    windows, pieces, halvings, gathers, scatters = [], [], 0, 0, 0
    w0 = col_lb
    while w0 < col_ub:                                            # :992
        wn = min(wmax, col_ub - w0)
        total = m.stored_in(w0, wn)
        need = max(total, 1) * (value_bytes + 4)                  # :1013
        if (need > scratch_bytes or float(m.nnz) * float(wn) / float(max(n_cols, 1)) > 1.5e9) and wn > FLOOR:   # :1014
            wmax = max(FLOOR, wn // 2)
            halvings += 1
            continue
        piece = m.largest_piece(w0, wn, rb)
        gathered = False
        if in_order:                                              # :1023-1032
            gathers += 1
            gathered = piece <= CAP                               # kernels_sparse.h:447
        if not gathered and wn > NARROW:                          # :1033-1036
            wmax = NARROW
            continue
        if not gathered:                                          # :1037-1041
            scatters += 1
        windows.append((w0, wn))
        pieces.append(piece)
        w0 += wn
    return Plan(in_order, rb, n_blocks, ny, windows, pieces, halvings, gathers, scatters)


def window_entries_per_row(m, col_lb, col_ub):
    """Stored entries of every row inside [col_lb, col_ub)."""
    c = np.asarray(m.indices)
    inside = (c >= col_lb) & (c < col_ub)
    return np.bincount(m.rows[inside], minlength=m.shape[0])


def refill_trace(m, col_lb, col_ub, ny, row):
    """How the workgroups of k_csr_tile_gather walk one row with in-order indices (kernels_sparse.h:392-427, 452-470): per stretch that
    holds an entry of the row, the sizes of the register-window refills.  A stretch starts at the row's first entry at or right of its
    first column (the binary search) and its window is refilled up to the ROW's end, not the column window's: full refills read
    REG_WINDOW entries at once, the last one of a row may be short.  A refill is asked for whenever the window is consumed and the
    workgroup has not yet met an entry at or right of its current tile's end."""
    c = np.asarray(m.indices[m.indptr[row]:m.indptr[row + 1]], dtype=np.int64) - col_lb
    out = []
    for lo, hi in stretches(col_ub - col_lb, ny):
        if hi <= lo:
            continue
        k = int(np.searchsorted(c, lo, side="left"))
        sizes, have, pos = [], 0, 0      # have: entries in the register window, pos: consumed of them
        for t_end in [min(hi, t + TILE) for t in range(lo, hi, TILE)]:
            more = True
            while more:
                while pos < have and c[k - have + pos] < t_end:
                    pos += 1
                if pos < have:
                    more = False
                else:                    # consumed: refill, or the row is finished
                    left = c.size - k
                    if left <= 0:
                        more = False
                    else:
                        have, pos = min(left, REG_WINDOW), 0
                        k += have
                        sizes.append(have)
        out.append(sizes)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", ["name", "data", "indices", "indptr", "shape", "labels", "window", "scratch_bytes", "compact"])
# window: (col_lb, col_ub); scratch_bytes: None (DEFAULT_SCRATCH) or the case's own budget; compact: small enough for every input form


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _values(rng, n, dtype=np.float32):
    """Log-normalised-looking values, never 0; integers far above the count tables' range for the integer types."""
    dtype = np.dtype(dtype)
    if dtype.kind == "i":
        return rng.randint(1000, 10_000_000, size=n).astype(dtype)
    v = np.log1p(np.exp(rng.normal(0.0, 1.0, size=n)) * 3.0)
    if dtype == np.float64:
        return v + 1e-9 * rng.rand(n)     # (not representable in float32: the call is not narrowed)
    return v.astype(np.float32)


def make_labels(rng, n_rows):
    """A reference plus a handful of small groups, cells shuffled; matrices of a few rows get fewer, a single row the reference alone."""
    if n_rows >= 600:
        sizes = (250, 100, 60, 40)
    elif n_rows >= 100:
        sizes = (40, 25, 10)
    elif n_rows >= 10:
        sizes = (n_rows // 5,) * 3
    else:
        sizes = ()
    codes = np.concatenate([np.zeros(n_rows - sum(sizes), dtype=np.int64)] + [np.full(s, k + 1, dtype=np.int64) for k, s in enumerate(sizes)])
    rng.shuffle(codes)
    return np.array([REF_LABEL if c == 0 else f"pert_{c:03d}" for c in codes])


def _from_positions(rng, rows, cols, shape, dtype=np.float32, idx=np.int32):
    """CSR arrays from (row, column) pairs already in row-major order."""
    indptr = np.zeros(shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=shape[0]), out=indptr[1:])
    return _values(rng, rows.size, dtype), cols.astype(idx), indptr.astype(idx)


def _exact(rng, n_rows, n_cols, nnz, keep=None):
    """Exactly `nnz` stored entries at distinct places (small shapes); `keep`: flat positions never stored."""
    free = np.arange(n_rows * n_cols)
    if keep is not None:
        free = np.setdiff1d(free, keep)
    flat = np.sort(rng.choice(free, size=nnz, replace=False))
    return flat // n_cols, flat % n_cols


def _bernoulli(rng, n_rows, n_cols, p, chunk=8192):
    """Every cell stored with probability p, drawn a chunk of rows at a time."""
    rows, cols = [], []
    for r0 in range(0, n_rows, chunk):
        r, c = np.nonzero(rng.rand(min(chunk, n_rows - r0), n_cols) < p)
        rows.append(r.astype(np.int64) + r0)
        cols.append(c.astype(np.int64))
    return np.concatenate(rows), np.concatenate(cols)


def _sparse_columns(rng, n_rows, n_cols, p):
    """The same for a few rows and tens of thousands of columns: per row a sorted draw of columns."""
    rows, cols = [], []
    for r in range(n_rows):
        c = np.unique(rng.randint(0, n_cols, size=int(p * n_cols)))
        rows.append(np.full(c.size, r, dtype=np.int64))
        cols.append(c.astype(np.int64))
    return np.concatenate(rows), np.concatenate(cols)


def _merge(rows, cols, more_rows, more_cols, n_cols):
    """Union of two sets of positions, row-major."""
    flat = np.union1d(rows * n_cols + cols, np.asarray(more_rows, dtype=np.int64) * n_cols + np.asarray(more_cols, dtype=np.int64))
    return flat // n_cols, flat % n_cols


def _outside(rows, cols, r0, r1, c0, c1):
    keep = ~((rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1))
    return rows[keep], cols[keep]


def _descend(data, indices, indptr, row):
    """One descending pair: the last two entries of `row` change places (values with them)."""
    a, b = int(indptr[row]), int(indptr[row + 1])
    assert b - a >= 2 and indices[b - 2] != indices[b - 1]
    for arr in (data, indices):
        arr[b - 2], arr[b - 1] = arr[b - 1].copy(), arr[b - 2].copy()


# ---- the compact matrix: 48 rows x 200 columns, every row written out (the register window, the column window, the types) ----
CW = (30, 170)          # the column window of the register-window cases: tiles [30, 94), [94, 158), [158, 170)
C_ROWS, C_COLS = 48, 200
# row -> stored entries inside CW
C_INSIDE = {0: 0, 1: 0, 2: 0, 3: 1, 4: 1, 5: 15, 6: 16, 7: 17, 8: 32, 9: 33, 10: 20}


def _compact_rows(rng, last_extra):
    lb, ub = CW
    rows = {0: [],
            1: [0, 3, 7, 12, 29],                       # wholly left of the window, up to col_lb - 1
            2: [170, 171, 180, 199],                    # wholly right of it, from col_ub on
            3: [29, 30],                                # col_lb - 1 and col_lb
            4: [169, 170]}                              # col_ub - 1 and col_ub
    for r, n in ((5, 15), (6, 16), (7, 17), (8, 32), (9, 33)):
        rows[r] = sorted(rng.choice(np.arange(lb, ub), size=n, replace=False).tolist() + [5, 190])
    rows[10] = [2, 9] + list(range(40, 80, 2)) + [185]  # 20 entries inside the first tile: the window is refilled in the middle of it
    for r in range(11, C_ROWS - 1):
        rows[r] = sorted(rng.choice(C_COLS, size=rng.randint(4, 30), replace=False).tolist())
    # the matrix's last row: 20 entries in the first tile, 12 further right, nothing beyond the window -- 32 from the window's first
    # column to the end of the arrays (two full refills); with one more (column 169), a last refill of one entry
    last = list(range(31, 91, 3)) + list(range(100, 160, 5))
    assert len(last) == 32
    rows[C_ROWS - 1] = last + ([169] if last_extra else [])
    return rows


def _compact(name, last_extra=False, dtype=np.float32, idx=np.int32, window=CW):
    rng = _rng("compact")     # one matrix under every name that uses it
    rows = _compact_rows(rng, last_extra)
    r = np.concatenate([np.full(len(rows[k]), k, dtype=np.int64) for k in range(C_ROWS)])
    c = np.concatenate([np.asarray(rows[k], dtype=np.int64) for k in range(C_ROWS)])
    d, i, p = _from_positions(_rng("compact-values"), r, c, (C_ROWS, C_COLS), dtype, idx)
    return Case(name, d, i, p, (C_ROWS, C_COLS), make_labels(_rng("compact-labels"), C_ROWS), window, None, True)


VALUE_TYPES = ("float32", "float64", "int32", "int64")
INDEX_TYPES = ("int32", "int64")

LADDER_SHAPE = (704, 130)   # 91 520 cells: an eighth, a quarter and a half of them are whole numbers; 704 = 11 * 64
LADDER = {"0.125": 11440, "0.25": 22880, "0.5": 45760}


def _ladder(name, nnz):
    rng = _rng(name)
    r, c = _exact(_rng("ladder"), *LADDER_SHAPE, LADDER["0.5"] + 1)[0:2]
    # nested: the first `nnz` of one fixed draw of 45 761 places, so that "one entry more" is the same matrix with one entry more
    order = _rng("ladder-order").permutation(r.size)[:nnz]
    order.sort()
    r, c = r[order], c[order]
    d, i, p = _from_positions(rng, r, c, LADDER_SHAPE)
    return Case(name, d, i, p, LADDER_SHAPE, make_labels(rng, LADDER_SHAPE[0]), (0, LADDER_SHAPE[1]), None, True)


def _random(name, n_rows, n_cols, p, window=None, compact=False):
    rng = _rng(name)
    r, c = _bernoulli(rng, n_rows, n_cols, p)
    d, i, pt = _from_positions(rng, r, c, (n_rows, n_cols))
    return Case(name, d, i, pt, (n_rows, n_cols), make_labels(rng, n_rows), window or (0, n_cols), None, compact)


def _one_row(name):
    rng = _rng(name)
    c = np.array([0, 1, 2, 17, 63, 64, 65, 100, 127, 128, 129], dtype=np.int64)
    d, i, p = _from_positions(rng, np.zeros(c.size, dtype=np.int64), c, (1, 130))
    return Case(name, d, i, p, (1, 130), make_labels(rng, 1), (0, 130), None, True)


def _empty_window(name):
    rng = _rng(name)
    r, c = _bernoulli(rng, 300, 130, 0.1)
    r, c = _outside(r, c, 0, 300, 40, 70)
    d, i, p = _from_positions(rng, r, c, (300, 130))
    return Case(name, d, i, p, (300, 130), make_labels(rng, 300), (40, 70), None, True)


STAGE_SHAPE = (512, 256)


def _stage(name, extra):
    """RB = 256: block 0 x columns [64, 128) holds 32 entries per row -- exactly 8192 -- plus `extra`; every other cell with p = 0.15."""
    rng = _rng("stage")
    r, c = _bernoulli(rng, *STAGE_SHAPE, 0.15)
    r, c = _outside(r, c, 0, 256, 64, 128)
    pr = np.repeat(np.arange(256), 32)
    pc = np.tile(64 + 2 * np.arange(32), 256)
    if extra:
        pr, pc = np.append(pr, 100), np.append(pc, 65)
    r, c = _merge(r, c, pr, pc, STAGE_SHAPE[1])
    d, i, p = _from_positions(_rng("stage-values"), r, c, STAGE_SHAPE)
    return Case(name, d, i, p, STAGE_SHAPE, make_labels(_rng("stage-labels"), STAGE_SHAPE[0]), (0, STAGE_SHAPE[1]), None, True)


def _stage_rb128(name):
    """RB = 128: block 1 x columns [64, 128) fully stored -- 8192 entries; every other cell with p = 0.3."""
    rng = _rng(name)
    shape = (256, 192)
    r, c = _bernoulli(rng, *shape, 0.3)
    r, c = _merge(r, c, np.repeat(np.arange(128, 256), 64), np.tile(np.arange(64, 128), 128), shape[1])
    d, i, p = _from_positions(rng, r, c, shape)
    return Case(name, d, i, p, shape, make_labels(rng, shape[0]), (0, shape[1]), None, True)


def _wide(name, n_cols, descending):
    """40 rows, 2 % stored, the last column stored in row 7; `descending`: one descending pair in row 11."""
    rng = _rng("wide")            # (65 536 and 65 537 columns: the same draw over the first 65 536)
    r, c = _sparse_columns(rng, 40, 65536, 0.02)
    r, c = _merge(r, c, [7, 7], [65535, n_cols - 1], n_cols)
    d, i, p = _from_positions(_rng("wide-values"), r, c, (40, n_cols))
    if descending:
        _descend(d, i, p, 11)
    return Case(name, d, i, p, (40, n_cols), make_labels(_rng("wide-labels"), 40), (0, n_cols), None, False)


RECUT_SHAPE = (300, 40000)


def _recut(name, first_col):
    """1 % stored, and 28 adjacent columns from `first_col` on (a multiple of 64) stored in every row: a piece of 8400 entries and more."""
    rng = _rng("recut")
    r, c = _sparse_columns(rng, *RECUT_SHAPE, 0.01)
    r, c = _merge(r, c, np.repeat(np.arange(300), 28), np.tile(first_col + np.arange(28), 300), RECUT_SHAPE[1])
    d, i, p = _from_positions(_rng("recut-values"), r, c, RECUT_SHAPE)
    return Case(name, d, i, p, RECUT_SHAPE, make_labels(_rng("recut-labels"), 300), (0, RECUT_SHAPE[1]), None, False)


def _halve(name, width, budget):
    """300 rows, a tenth stored; budget(stored entries in the window) -> scratch_bytes."""
    rng = _rng("halve")
    r, c = _bernoulli(rng, 300, 201, 0.1)
    d, i, p = _from_positions(_rng("halve-values"), r, c, (300, 201))
    inside = int(np.count_nonzero(c < width))
    return Case(name, d, i, p, (300, 201), make_labels(_rng("halve-labels"), 300), (0, width), budget(inside), True)


def _last_row(name, descending):
    """43 rows (not a multiple of the sorted check's four rows per wavefront step); `descending`: one descending pair in the very last row."""
    rng = _rng("last-row")
    r, c = _bernoulli(rng, 43, 130, 0.12)
    r, c = _merge(r, c, [42, 42], [3, 120], 130)
    d, i, p = _from_positions(_rng("last-row-values"), r, c, (43, 130))
    if descending:
        _descend(d, i, p, 42)
    return Case(name, d, i, p, (43, 130), make_labels(_rng("last-row-labels"), 43), (0, 130), None, True)


BUILDERS = {}
for _d, _n in LADDER.items():
    BUILDERS[f"rb-density-{_d}-at"] = lambda name, n=_n: _ladder(name, n)
    BUILDERS[f"rb-density-{_d}-over"] = lambda name, n=_n: _ladder(name, n + 1)
BUILDERS.update({
    "rows-1": _one_row,
    "rows-rb": lambda name: _random(name, 512, 130, 0.1, compact=True),
    "rows-rb+1": lambda name: _random(name, 513, 130, 0.1, compact=True),
    "window-empty": _empty_window,
    "ny-16-136-blocks": lambda name: _random(name, 136 * 512, 130, 0.03),
    "ny-15-137-blocks": lambda name: _random(name, 136 * 512 + 1, 130, 0.03),
    "ny-4": lambda name: _random(name, 512 * 512 + 1, 130, 0.04),
    "ny-2": lambda name: _random(name, 1024 * 64, 130, 0.52),
    "ny-1-natural": lambda name: _random(name, 2048 * 64, 130, 0.52),
    "ny-16-one-tile-each": lambda name: _random(name, 300, 1000, 0.05, compact=True),
    "regwin-last-full": lambda name: _compact(name),
    "regwin-last-short": lambda name: _compact(name, last_extra=True),
    "width-63": lambda name: _compact(name, window=(30, 93)),
    "width-64": lambda name: _compact(name, window=(30, 94)),
    "width-65": lambda name: _compact(name, window=(30, 95)),
    "stage-8192": lambda name: _stage(name, False),
    "stage-8193": lambda name: _stage(name, True),
    "stage-rb128-full-piece": _stage_rb128,
    "cols-65536-sorted": lambda name: _wide(name, 65536, False),
    "cols-65537-sorted": lambda name: _wide(name, 65537, False),
    "cols-65536-descending-pair": lambda name: _wide(name, 65536, True),
    "cols-65537-descending-pair": lambda name: _wide(name, 65537, True),
    "recut-piece-in-first": lambda name: _recut(name, 640),
    "recut-piece-in-second": lambda name: _recut(name, 32768 + 640),
    "halve-200": lambda name: _halve(name, 200, lambda n: n * 8 - 1),
    "halve-201": lambda name: _halve(name, 201, lambda n: n * 8 - 1),
    "halve-floor": lambda name: _halve(name, 100, lambda n: 7),
    "sorted-last-row": lambda name: _last_row(name, False),
    "descending-pair-in-last-row": lambda name: _last_row(name, True),
})
for _v in VALUE_TYPES:
    for _i in INDEX_TYPES:
        if (_v, _i) != ("float32", "int32"):    # (that pair is regwin-last-full itself)
            BUILDERS[f"types-{_v}-{_i}"] = lambda name, v=_v, i=_i: _compact(name, dtype=np.dtype(v), idx=np.dtype(i))
NAMES = tuple(BUILDERS)
BOUND = ("sorted-last-row", "descending-pair-in-last-row")   # also run through bind_sparse: the flag is looked at when the matrix is bound

Expect = namedtuple("Expect", ["RB", "ny", "windows", "gathers", "scatters", "piece"], defaults=(None,))
# what each case is named for (piece: the largest piece over the transposed windows, where the case is about it)
_ALL130 = [(0, 130)]
EXPECT = {
    "rb-density-0.125-at": Expect(512, 16, _ALL130, 1, 0),
    "rb-density-0.125-over": Expect(256, 16, _ALL130, 1, 0),
    "rb-density-0.25-at": Expect(256, 16, _ALL130, 1, 0),
    "rb-density-0.25-over": Expect(128, 16, _ALL130, 1, 0),
    "rb-density-0.5-at": Expect(128, 16, _ALL130, 1, 0),
    "rb-density-0.5-over": Expect(64, 16, _ALL130, 1, 0),
    "rows-1": Expect(512, 16, _ALL130, 1, 0),
    "rows-rb": Expect(512, 16, _ALL130, 1, 0),
    "rows-rb+1": Expect(512, 16, _ALL130, 1, 0),
    "window-empty": Expect(512, 16, [(40, 30)], 1, 0, 0),
    "ny-16-136-blocks": Expect(512, 16, _ALL130, 1, 0),
    "ny-15-137-blocks": Expect(512, 15, _ALL130, 1, 0),
    "ny-4": Expect(512, 4, _ALL130, 1, 0),
    "ny-2": Expect(64, 2, _ALL130, 1, 0),
    "ny-1-natural": Expect(64, 1, _ALL130, 1, 0),
    "ny-16-one-tile-each": Expect(512, 16, [(0, 1000)], 1, 0),
    "regwin-last-full": Expect(512, 16, [(30, 140)], 1, 0),
    "regwin-last-short": Expect(512, 16, [(30, 140)], 1, 0),
    "width-63": Expect(512, 16, [(30, 63)], 1, 0),
    "width-64": Expect(512, 16, [(30, 64)], 1, 0),
    "width-65": Expect(512, 16, [(30, 65)], 1, 0),
    "stage-8192": Expect(256, 16, [(0, 256)], 1, 0, 8192),
    "stage-8193": Expect(256, 16, [(0, 256)], 1, 1, 8193),
    "stage-rb128-full-piece": Expect(128, 16, [(0, 192)], 1, 0, 8192),
    "cols-65536-sorted": Expect(512, 16, [(0, 65536)], 1, 0),
    "cols-65537-sorted": Expect(512, 16, [(0, 65536), (65536, 1)], 2, 0),
    "cols-65536-descending-pair": Expect(256, 16, [(0, 32768), (32768, 32768)], 0, 2),
    "cols-65537-descending-pair": Expect(256, 16, [(0, 32768), (32768, 32768), (65536, 1)], 0, 3),
    "recut-piece-in-first": Expect(512, 16, [(0, 32768), (32768, 7232)], 3, 1),
    "recut-piece-in-second": Expect(512, 16, [(0, 32768), (32768, 7232)], 3, 1),
    "halve-200": Expect(512, 16, [(0, 100), (100, 100)], 2, 0),
    "halve-201": Expect(512, 16, [(0, 100), (100, 100), (200, 1)], 3, 0),
    "halve-floor": Expect(512, 16, [(0, 64), (64, 36)], 2, 0),
    "sorted-last-row": Expect(512, 16, _ALL130, 1, 0),
    "descending-pair-in-last-row": Expect(256, 16, _ALL130, 0, 1),
}
for _name in NAMES:
    if _name.startswith("types-"):
        EXPECT[_name] = EXPECT["regwin-last-full"]

# The stored entries of the cases with many cells, from the shapes alone (rows x columns x the probability of a cell, the pieces added):
# what the host test holds below MAX_STORED
SHAPE_BOUND = {"ny-1-natural": 2048 * 64 * 130 * 0.52, "ny-2": 1024 * 64 * 130 * 0.52, "ny-4": (512 * 512 + 1) * 130 * 0.04,
               "ny-16-136-blocks": 136 * 512 * 130 * 0.03, "ny-15-137-blocks": (136 * 512 + 1) * 130 * 0.03,
               "recut-piece-in-first": 300 * 40000 * 0.01 + 300 * 28, "recut-piece-in-second": 300 * 40000 * 0.01 + 300 * 28}

_made = {}


def make(name):
    """The case of that name (the last few are kept: the sides of a switch are neighbours in a run)."""
    if name not in _made:
        if len(_made) >= 4:
            _made.clear()
        _made[name] = BUILDERS[name](name)
    return _made[name]


def matrix(c):
    return Matrix(c.data, c.indices, c.indptr, c.shape)


def case_plan(c, **forms):
    return plan(matrix(c), *c.window, value_bytes=c.data.dtype.itemsize, scratch_bytes=c.scratch_bytes or DEFAULT_SCRATCH, **forms)


def groups(labels, test):
    return oracle.encode_and_count_groups(labels, REF_LABEL if test == "ovo" else None)[1]


def as_csc(c):
    """The case for the oracle: a scipy CSC matrix of the same values in float64 (float32 stays float32, as the engine ranks it)."""
    d = c.data if c.data.dtype == np.float32 else c.data.astype(np.float64)
    m = sparse.csr_matrix((d, c.indices.astype(np.int64), c.indptr.astype(np.int64)), shape=c.shape)
    return m.tocsc()
