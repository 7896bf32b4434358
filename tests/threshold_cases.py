"""Inputs that sit on the drivers' size thresholds, with tie blocks as large as a whole group.

The drivers pick kernels, counter widths and LDS layouts from the largest ranked group, the reference size, the number of groups, the
number of groups above 255 cells and the cell count.  Every case here puts one of those integers on one side of one switch point, and
its columns hold a whole "boundary" group at ONE value, so that a per-(group, value) multiplicity, a run length or a bucket counter
reaches the group's size -- the input on which a counter that is one bit too narrow fails.  Everything is seeded: a case is its name.

Shared by tests/test_threshold_cases_host.py (the conditions on the inputs, evaluated with the CPU oracle) and
tests/test_gpu_thresholds.py (every input form of the engine against the oracle).  Imports numpy and the oracle only.
"""
import math
import zlib
from collections import namedtuple

import numpy as np

import oracle

REF_LABEL = "g00000"
N_GENES = 12
CONSTANTS = (1, 9, 62, 255, 2047, 0, -2)    # columns 0-6: 64-value table, 4-bit cell zone, byte flag, 2048-value table, no stored entry, negatives
MIXED_COLUMNS = tuple(range(11))            # the share rule covers these; column 11 is the whole-column constant
STRICT_COLUMNS = (0, 1, 3, 4, 7, 8, 10)     # the boundary group's own row holds no p of exactly 0 or 1 here
MAX_SHARE = 0.15

RANKED_EDGES = (15, 16, 17, 255, 256, 257, 1024, 1025, 65534, 65535, 65536)
REF_EDGES = (2048, 2049, 16384, 16385, 29999, 30000, 65535, 65536)
SINGLES_EDGES = (65535, 65536, 65537)
FORTIES_EDGES = (127, 128, 129)
BIG_EDGES = (8, 9, 16, 17)   # CSCC_MAX_BIG = 8 (k_csc_counts), CSRC_MAX_BIG = 16 (k_csr_counts)
CELLS_EDGES = (32767, 32768)
TOP_EDGES = (255, 256, 257)   # (every ranked-* case holds a group of 300 cells: there the LARGEST ranked group only moves from 1024 on)
_TAIL = (300, 256, 255, 40, 16, 15, 2, 1)

# name -> (group sizes, boundary groups, is the reference the boundary group)
Spec = namedtuple("Spec", ["sizes", "boundary", "ref_edge"])
Case = namedtuple("Case", ["name", "labels", "X", "boundary", "sizes"])


def _specs():
    s = {}
    for n in RANKED_EDGES:
        s[f"ranked-{n}"] = Spec((6000, n) + _TAIL, (1,), False)
    for n in TOP_EDGES:   # the edge group is the largest ranked one of an OVO call
        s[f"top-{n}"] = Spec((3000, n, 40, 16, 15, 2, 1), (1,), False)
    for n in REF_EDGES:
        s[f"ref-{n}"] = Spec((n,) + _TAIL, (0,), True)
    for G in SINGLES_EDGES:
        s[f"singles-{G}"] = Spec((3000,) + (1,) * (G - 1), (), False)
    for G in FORTIES_EDGES:
        s[f"forties-{G}"] = Spec((300,) + (40,) * (G - 1), (), False)
    for k in BIG_EDGES:   # the groups of 256 cells are what the count is about: they hold the constants
        s[f"big-{k}"] = Spec((3000,) + (256,) * k + (17,), tuple(range(1, k + 1)), False)
    s["packed-130x255"] = Spec((255,) * 131, tuple(range(1, 131)), False)
    for n in CELLS_EDGES:
        s[f"cells-{n}"] = Spec((9000, 8000, 8000, n - 25000), (1,), False)
    return s


SPECS = _specs()
# a draw in which the reference holds exactly as many cells below a constant as above it puts p = 1.0 into the boundary group's own row
# (tests/test_threshold_cases_host.py refuses that): such a case takes its next draw, a "+" more in the text its seed is hashed from.
# top-255: the first draw left 1005 reference cells at 0 and 1005 at 2 in column 0, so the OVO p of the boundary row there was 1.0.
REDRAW = {"top-255": 1}
NAMES = tuple(SPECS)

# the cases whose second-line kernels (the routes behind an engine option) are run as well
SECOND_LINE = tuple(f"ranked-{n}" for n in (255, 256, 257, 65534, 65535, 65536)) + tuple(f"ref-{n}" for n in (29999, 30000, 65535, 65536))


def make(name):
    """The case of that name: labels (shuffled rows), X float32 [cells, 12], the boundary groups, the group sizes."""
    spec = SPECS[name]
    rng = np.random.RandomState(zlib.crc32((name + "+" * REDRAW.get(name, 0)).encode()) & 0x7FFFFFFF)
    codes = np.repeat(np.arange(len(spec.sizes)), spec.sizes)
    rng.shuffle(codes)
    n = codes.size
    held = np.isin(codes, spec.boundary)
    X = np.empty((n, N_GENES), dtype=np.float32)
    for j, v in enumerate(CONSTANTS):   # symmetric around v; the boundary cells at v
        x = v + rng.randint(-1, 2, size=n)
        if not spec.ref_edge or j in (0, 1, 5):   # (a reference that is constant everywhere drives most p-values of an OVO call to 0)
            x[held] = v
        X[:, j] = x
    x = rng.randint(1, 4, size=n) * 0.25   # a non-integer tie block as large as the group
    if not spec.ref_edge:
        x[held] = 0.5
    X[:, 7] = x
    cont = ((rng.permutation(n) + 0.5 * rng.rand(n)) / n + 0.01).astype(np.float32)   # one value per stratum: no ties after the cast
    X[:, 8] = cont
    X[:, 9] = np.where(rng.rand(n) < 0.5, np.float32(0), cont)
    X[:, 10] = rng.poisson(3.0, size=n)
    X[:, 11] = 4.0   # the only whole-column constant
    labels = np.array([f"g{c:05d}" for c in codes])
    return Case(name, labels, X, tuple(spec.boundary), tuple(spec.sizes))


COUNT_KEEP = 0.04                                  # the share of the other cells that a column of the count form stores
COUNT_LAMBDAS = (0.5, 1, 2, 3, 5, 8, 12, 16, 20)   # columns 3-11 of the count form: 1 + Poisson(lambda) where stored, below 64 throughout


def count_form(c):
    """The case as a matrix that the count-valued sparse routes accept as a whole: float32 [cells, 12], every value an integer in [0, 64),
    fewer than 30 % of the cells stored.

    k_csr_counts and the dense byte windows take their verdict from a sample of the WHOLE CSR matrix (more than 2 % of the stored values
    not non-negative integers, more than 0.5 % of them 64 or more, or more than 30 % of the cells stored: the route computes nothing), and
    a window of which more than one gene in 16 leaves the pass is redone by the other routes -- the case's own 12 columns are 87-90 %
    dense and a third of their stored values are negatives or fractions.  Columns 0-2 are the case's (the boundary cells at 1, 9 and 62:
    an 8-bit cell, a 4-bit cell and the table's last value but one driven to the group's size), the other cells stored with probability
    COUNT_KEEP; columns 3-11 hold 1 + Poisson(lambda) with the same probability.  The three boundary columns are what keeps the largest
    cases below 30 %: a fourth would not fit."""
    rng = np.random.RandomState(zlib.crc32((c.name + "/counts").encode()) & 0x7FFFFFFF)
    codes = np.unique(c.labels, return_inverse=True)[1].reshape(-1)
    n = codes.size
    held = np.isin(codes, c.boundary)
    X = np.zeros((n, N_GENES), dtype=np.float32)
    for j in range(3):
        X[:, j] = np.where(held | (rng.rand(n) < COUNT_KEEP), c.X[:, j], np.float32(0))
    for j, lam in enumerate(COUNT_LAMBDAS, 3):
        X[:, j] = np.where(rng.rand(n) < COUNT_KEEP, 1 + rng.poisson(lam, size=n), 0)
    return X


def groups(labels, test):
    """The GroupContainer of a case for "ovo" (reference g00000) or "ovr"."""
    return oracle.encode_and_count_groups(labels, REF_LABEL if test == "ovo" else None)[1]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def z_want(X, g, U, tie_correct=True):
    """(mu - U) / sqrt(var0 * tie_corr) as pval_device_pre forms sigma (kernels_finalize.h), one IEEE operation at a time."""
    X = np.asarray(X, dtype=np.float64)
    N, M = X.shape
    codes, counts, ref = g.encoded_groups, g.counts, g.encoded_ref_group
    Z = np.zeros((counts.size, M))
    col_tie = None
    if ref < 0:
        col_tie = [sum(int(t) ** 3 - int(t) for t in np.unique(X[:, j], return_counts=True)[1]) for j in range(M)]
    for gi in range(counts.size):
        if gi == ref:
            continue
        n_tgt = int(counts[gi])
        if ref >= 0:
            n_ref = int(counts[ref])
            n = n_ref + n_tgt
            cells = (codes == ref) | (codes == gi)
        else:
            n_ref, n, cells = N - n_tgt, N, None
        nnn = float(n * (n - 1) * (n + 1))
        var0 = float(n_ref * n_tgt * (n_ref + n_tgt + 1)) / 12.0
        mu = float(n_ref * n_tgt) / 2.0
        for j in range(M):
            if not tie_correct:
                tie = 0.0
            elif cells is None:
                tie = float(col_tie[j])
            else:
                tie = float(sum(int(t) ** 3 - int(t) for t in np.unique(X[cells, j], return_counts=True)[1]))
            tc = 1.0 - tie / nnn
            Z[gi, j] = (mu - float(U[gi, j])) / math.sqrt(var0 * tc) if tc > 1.0e-9 else 0.0
    return Z


def z_want_fast(X, g, U, tie_correct=True):
    """z_want without the loop over groups (65 537 of them in the largest case): the same integers, then the same IEEE operations
    elementwise -- tests/test_threshold_cases_host.py holds it to z_want's bits."""
    X = np.asarray(X, dtype=np.float64)
    N, M = X.shape
    codes, ref = np.asarray(g.encoded_groups, dtype=np.int64), int(g.encoded_ref_group)
    cnt = np.asarray(g.counts, dtype=np.int64)
    G = cnt.size
    if ref >= 0:
        n_ref = np.full(G, cnt[ref], dtype=np.int64)
        n = n_ref + cnt
    else:
        n = np.full(G, N, dtype=np.int64)
        n_ref = n - cnt
    nnn = (n * (n - 1) * (n + 1)).astype(np.float64)        # < 2^53: exact
    var0 = (n_ref * cnt * (n_ref + cnt + 1)).astype(np.float64) / 12.0
    mu = (n_ref * cnt).astype(np.float64) / 2.0
    tie = np.zeros((G, M), dtype=np.int64)
    if tie_correct:
        for j in range(M):
            vals, vi = np.unique(X[:, j], return_inverse=True)
            vi = vi.reshape(-1).astype(np.int64)
            if ref < 0:
                t = np.bincount(vi, minlength=vals.size).astype(np.int64)
                tie[:, j] = int((t ** 3 - t).sum())
                continue
            r = np.bincount(vi[codes == ref], minlength=vals.size).astype(np.int64)
            key, c = np.unique(codes * vals.size + vi, return_counts=True)   # the (group, value) pairs that occur
            kg, kv = key // vals.size, key % vals.size
            t, rv = c.astype(np.int64) + r[kv], r[kv]
            col = np.full(G, int((r ** 3 - r).sum()), dtype=np.int64)          # the values a group does not hold: the reference's blocks alone
            np.add.at(col, kg, (t ** 3 - t) - (rv ** 3 - rv))
            tie[:, j] = col
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = 1.0 - tie.astype(np.float64) / nnn[:, None]
        Z = (mu[:, None] - np.asarray(U, dtype=np.float64)) / np.sqrt(var0[:, None] * tc)
    Z[~(tc > 1.0e-9)] = 0.0
    if ref >= 0:
        Z[ref] = 0.0
    return Z
