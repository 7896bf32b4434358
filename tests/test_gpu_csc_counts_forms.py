"""The forms of k_csc_counts (kernels_csc_counts.h) that no other suite launches.

What the other suites reach, from the rules of `csc_counts_layout` (sparse_driver.h) -- all of it with float32 values, int32 indices and
the 16-bit code table unless said otherwise, OVO and OVR each:

* mixed cells, 64 values: without a side table (test_gpu_sparse: ..._mixed_cells_overflow_...), with one (test_csc_counts_route), with one
  and in windows (..._taken_in_windows, whose overflowing gene is redone with 8-bit cells, side table and windows);
* 8-bit cells, 64 values, no side table (..._mixed_cells_overflow_...: the second pass and `no_csc_counts_mixed`);
* 16-bit cells, in one launch and in windows (..._take_16_bit_cells, ..._reference_of_tens_of_thousands_of_cells);
* codes read from `indices` (the device CSR -> CSC transposition): mixed cells only (test_gpu_sparse_route_trace, case 1).

What is left, and taken here: mixed and 8-bit cells in windows WITHOUT a side table; the 32-value table (8-bit cells: the 2600 groups of
test_csc_counts_route[many_groups] fit the mixed layout, whose table has 64 values, and none of its 4-bit cells overflows), with and
without a side table; 8-bit cells with a side table in one launch; 8-bit, 16-bit and 32-value tables with codes read from `indices`;
and the value / index types other than float32 / int32.  The value and the index type enter the entry rounds only (the loads, the
range test of a value), so they are crossed with one layout, not with all of them.  Windows need the 16-bit code table (the driver's
rule), and a window never has more than 2000 groups, so neither codes from `indices` nor the 32-value table meet a window.

Every case: the planes equal, bit for bit, those of the same call with `no_csc_counts_path` (the OVO reference's row, which the
reference leaves unspecified: equal), they match the oracle, and the profile shows how many launches of k_csc_counts it took.
"""
import numpy as np
import pytest
from scipy import sparse

import oracle
from conftest import assert_planes_match

pytestmark = pytest.mark.gpu

TRANSPOSED = {"no_csr_counts_path": 1, "no_dense_window_path": 1}  # CSR input: transposed on the device, `indices` then hold the group codes


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import get_engine
    return get_engine()


def _labels(rng, sizes):
    """Group g00000 (the OVO reference) first; the cells of all groups shuffled."""
    labels = np.concatenate([[f"g{i:05d}"] * int(sz) for i, sz in enumerate(sizes)])
    rng.shuffle(labels)
    return labels


def _check(engine, X, labels, test, launches, *, fmt="csc", dtype=np.float32, idx=np.int32, opts=None):
    _, g = oracle.encode_and_count_groups(labels, "g00000" if test == "ovo" else None)
    M = (sparse.csc_matrix if fmt == "csc" else sparse.csr_matrix)(X.astype(dtype))
    M.indices, M.indptr = M.indices.astype(idx), M.indptr.astype(idx)
    opts = dict(TRANSPOSED if fmt == "csr" else {}, **(opts or {}))
    engine.set_groups(g)
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        engine.profile(True)
        engine.profile_reset()
        got = engine.run_sparse(fmt, M.data, M.indices, M.indptr, M.shape, 0, M.shape[1])
        prof = engine.profile_get()
        engine.profile(False)
        engine.set_option("no_csc_counts_path", 1)
        other = engine.run_sparse(fmt, M.data, M.indices, M.indptr, M.shape, 0, M.shape[1])
    finally:
        engine.profile(False)
        for k in list(opts) + ["no_csc_counts_path"]:
            engine.set_option(k, 0)
    print({k: v["launches"] for k, v in prof.items()})
    assert prof.get("k_csc_counts", {}).get("launches", 0) == launches, prof
    ref = g.encoded_ref_group if test == "ovo" else -1
    rows = np.arange(g.counts.size) != ref
    for a, b in zip(got, other):
        assert a[rows].tobytes() == b[rows].tobytes()
        np.testing.assert_array_equal(a[~rows], b[~rows])
    assert_planes_match(got, oracle.run(X.astype(np.float64), g), ref_row=ref, what=f"{fmt} {test}")


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_windows_of_groups_without_a_side_table(engine, test):
    """Mixed cells, then 8-bit cells, 64 values, no side table, windows (WIN).  4800 groups of one or two cells (and one of 20): 33
    bytes per group of the 32-value form do not fit LDS beside 8 KB (4716 groups do), so `cscc_group_window` cuts three windows of
    1600; those fit twice per CU as mixed cells; no group exceeds 255 cells.  Gene 2 holds the value 9 in all 20 cells of one group:
    its 4-bit cell carries, the gene is redone with 8-bit cells -- three launches per pass."""
    rng = np.random.RandomState(601)
    labels = _labels(rng, [2, 20] + list(rng.randint(1, 3, size=4798)))
    n = labels.size
    X = np.zeros((n, 6), np.float32)
    X[:, 0] = rng.poisson(2.0, size=n) * (rng.rand(n) < 0.5)
    X[:, 1] = rng.randint(1, 64, size=n) * (rng.rand(n) < 0.3)        # every cell of the table
    X[:, 2] = np.where(labels == "g00001", 9.0, rng.poisson(1.0, size=n))
    X[:, 3] = rng.poisson(3.0, size=n)
    X[rng.randint(n), 3] = 70.0                                       # beyond the table: the gene leaves the kernel
    X[:, 4] = rng.poisson(0.5, size=n)
    X[rng.randint(n), 4] = 2.5                                        # fractional: leaves
    _check(engine, X, labels, test, 6)


@pytest.mark.parametrize("fmt", ["csc", "csr"])
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_the_32_value_table(engine, test, big, fmt):
    """8-bit cells, 32 values (RT = 32), with and without a side table (HAS_BIG); from CSR, codes read from `indices` (C16 off).  4300
    groups of one or two cells: one window (fewer than 4717), 65 bytes per group do not fit LDS (2394 groups do) and neither do 37 of
    the mixed layout beside 8 KB (4206 groups do): the 8-bit form with 31 values, one launch.  `big`: one group of 256 cells, all of
    them 31 in gene 3 -- a count of 256 in its 32-bit cell.  Gene 2 holds a 32 and leaves the kernel."""
    rng = np.random.RandomState(602)
    labels = _labels(rng, [2] + ([256] if big else []) + list(rng.randint(1, 3, size=4299 - big)))
    n = labels.size
    X = np.zeros((n, 6), np.float32)
    X[:, 0] = rng.poisson(2.0, size=n) * (rng.rand(n) < 0.5)
    X[:, 1] = rng.randint(1, 32, size=n) * (rng.rand(n) < 0.4)        # every cell of the table
    X[:, 2] = rng.poisson(2.0, size=n)
    X[rng.randint(n), 2] = 32.0
    X[:, 3] = 31.0
    X[:, 5] = rng.poisson(6.0, size=n) * (rng.rand(n) < 0.2)
    _check(engine, X, labels, test, 1, fmt=fmt)


@pytest.mark.parametrize("fmt", ["csc", "csr"])
@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_8bit_cells_beside_a_side_table(engine, test, fmt):
    """8-bit cells, 64 values, a side table (HAS_BIG), one launch; from CSR with codes read from `indices`.  Eight groups, one of 256
    cells (the side table's; at most eight such groups keep the call off 16-bit cells).  Gene 1 holds the value 12 in every cell:
    the 4-bit cells of the groups of 40, 17 and 16 cells carry (the group of 15 is the last that fits), gene 3 the value 63 -- the
    carry leaves the last word; both are redone with 8-bit cells: two launches."""
    rng = np.random.RandomState(603)
    labels = _labels(rng, [30, 256, 40, 17, 16, 15, 5, 1])
    n = labels.size
    X = np.zeros((n, 6), np.float32)
    X[:, 0] = rng.poisson(3.0, size=n) * (rng.rand(n) < 0.6)
    X[:, 1] = 12.0
    X[:, 2] = rng.randint(1, 64, size=n) * (rng.rand(n) < 0.5)
    X[:, 3] = 63.0
    X[:, 4] = rng.randint(1, 4, size=n)
    _check(engine, X, labels, test, 2, fmt=fmt)


def _nine_big_groups(seed):
    rng = np.random.RandomState(seed)
    labels = _labels(rng, [40] + [256] * 9 + [7, 1])
    n = labels.size
    X = np.zeros((n, 6), np.float32)
    X[:, 0] = rng.poisson(3.0, size=n) * (rng.rand(n) < 0.6)
    X[:, 1] = 5.0                                                     # 256 in one 16-bit cell
    X[:, 2] = rng.randint(1, 64, size=n) * (rng.rand(n) < 0.5)        # every cell of the table
    X[:, 3] = rng.poisson(20.0, size=n)
    X[rng.randint(n), 3] = 64.0                                       # beyond the table: leaves
    X[:, 4] = rng.randint(1, 4, size=n)
    return X, labels


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_16_bit_cells_with_codes_read_from_the_indices(engine, test):
    """16-bit cells, codes read from `indices` (C16 off): nine groups of 256 cells are one more than the side table holds, so every
    group gets 16-bit cells; CSR input is transposed on the device.  One launch."""
    X, labels = _nine_big_groups(604)
    _check(engine, X, labels, test, 1, fmt="csr")


@pytest.mark.parametrize("dtype,idx", [(np.float32, np.int64), (np.float64, np.int32), (np.float64, np.int64), (np.int32, np.int32),
                                       (np.int32, np.int64), (np.int64, np.int32), (np.int64, np.int64)])
@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_value_and_index_types(engine, test, dtype, idx):
    """The value and index types beside float32 / int32, on the 16-bit cells of nine groups of 256 cells (host arrays: float64 is not
    narrowed to float32).  One launch."""
    X, labels = _nine_big_groups(605)
    _check(engine, X, labels, test, 1, dtype=dtype, idx=idx)
