"""Which route a sparse call takes, pinned by the launches per kernel family.

The other sparse tests assert results, and mostly not which route produced them: a change to the route selection of
sparse_driver.h can send a window down a slower, still-correct route without any of them noticing.  Every case here runs once
under `engine.profile(True)` and compares `profile_get()` -- launches per kernel family, every family, nothing left out -- with a
literal table, then the planes with the oracle.

The table was recorded by running these very cases on commit 50314bb (the parent of the commit that split run_sparse_t into route
functions), on an MI355X; it is not computed by the code under test.  A family that the table names and the profile lacks (or the
other way round) fails the comparison: nothing is skipped.

What a profile can and cannot tell: the families are not split by value type, so the float64 cases use a column whose stored entries
fit k_csc_ovr_gene's LDS key buffer with four-byte keys and not with eight-byte ones -- narrowed to float32 the kernel takes every
gene (the rows of 4-f64-narrowed-* equal those of 4-f32-*: one k_finalize), in float64 it leaves that gene to the general route (the
rows of 4-f64-log1p-kept-*: a second k_finalize, k_gene_totals and k_value_sums, and k_ovr_gene).
Pass 2 of the CSR -> CSC transposition is profiled under the name of the form that ran, k_csr_tile_gather or k_csr_block_scatter (its
counting pass stays under k_sparse_seg), so the rows of case 5 differ: gather 1 / scatter 0 for the matrix with its rows in order,
0 / 1 for the one with two rows out of order -- a sorted matrix regressing to the scatter form fails here.  Those rows were recorded
again when the two names were split off, under this rule: for every row, the new k_sparse_seg plus the two new families equals the old
k_sparse_seg, and every other family is unchanged.  The planes are checked for both.
What the other rows show: case 1 has two k_csc_counts (two runs of flagged genes, transposed, no dense window: no k_ovo_fused_wide),
case 2 one k_ovo_fused_wide (the whole window once more, dense windows allowed), case 3 no k_csr_counts; in case 6 k_csc_counts is
followed by k_csc_gene (OVO) / k_csc_ovr_gene (OVR), which the two-kernel rows lack; case 7 has k_ovo_rank_compact; the deferred CSC
rows of case 8 have two k_csc_counts (the pass, then the left-over column), the CSR rows one k_csr_counts.
"""
import numpy as np
import pytest
from scipy import sparse

import oracle
from conftest import assert_planes_match
from route_trace import labels as _labels, trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import get_engine
    return get_engine()


def _dev(M):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (M.data, M.indices, M.indptr))


def _counts(seed, n=600, m=256, sizes=(100,) * 6):
    """Counts below 64, a seventh of the cells stored (the group-major CSR pass leaves matrices with 30 % stored and more to the
    dense windows), six groups of 100 cells."""
    rng = np.random.RandomState(seed)
    X = np.minimum(rng.poisson(3.0, size=(n, m)), 60).astype(np.float32) * (rng.rand(n, m) < 0.15)
    return X.astype(np.float32), _labels(rng, list(sizes)), rng


def _continuous(seed, n, m, sizes, stored=0.3):
    rng = np.random.RandomState(seed)
    X = (np.exp(rng.normal(0.0, 1.0, size=(n, m))) * (rng.rand(n, m) < stored)).astype(np.float32)
    return X, _labels(rng, list(sizes)), rng


# ---- the cases: name -> (X, labels, test, options, run(engine, M-maker) ...) built lazily ----
def _plain(fmt, device, dtype=None, **kw):
    def run(engine, X):
        M = (sparse.csr_matrix if fmt == "csr" else sparse.csc_matrix)(X if dtype is None else X.astype(dtype))
        d, i, p = _dev(M) if device else (M.data, M.indices, M.indptr)
        return engine.run_sparse(fmt, d, i, p, M.shape, 0, M.shape[1], **kw)
    return run


def _deferred(fmt):
    def run(engine, X):
        M = (sparse.csr_matrix if fmt == "csr" else sparse.csc_matrix)(X)
        d, i, p = _dev(M)
        planes = engine.run_sparse(fmt, d, i, p, M.shape, 0, M.shape[1], device_out=True, defer=True)
        engine.synchronize()
        return tuple(t.cpu().numpy() for t in planes)
    return run


def _unsorted_rows(engine, X):
    M = sparse.csr_matrix(X)
    for r in (7, 123):  # two rows whose column indices descend
        a, b = M.indptr[r], M.indptr[r + 1]
        assert b - a >= 2
        M.indices[a:b] = M.indices[a:b][::-1].copy()
        M.data[a:b] = M.data[a:b][::-1].copy()
    d, i, p = _dev(M)
    return engine.run_sparse("csr", d, i, p, M.shape, 0, M.shape[1])


def _build_cases():
    cases = {}

    def add(name, X, labels, test, run, opts=None, oracle_kw=None):
        cases[name] = dict(X=X, labels=labels, test=test, run=run, opts=opts or {}, oracle_kw=oracle_kw or {})

    for test in ("ovo", "ovr"):
        # 1: group-major CSR pass, genes 10, 30 and 200 flagged: two runs (10 .. 30 joined across the gap), exact sparse routes
        X, labels, rng = _counts(1)
        for j in (10, 30, 200):
            X[rng.randint(600), j] = 70.0
        add(f"1-csr-counts-flagged-runs-{test}", X, labels, test, _plain("csr", True))
        # 2: every eighth gene flagged (more than 1/16): the whole window once more, without the pass
        X, labels, rng = _counts(2)
        for j in range(0, 256, 8):
            X[rng.randint(600), j] = 70.0
        add(f"2-csr-counts-many-flagged-{test}", X, labels, test, _plain("csr", True))
        # 3: byte windows + fused kernels, then the covering window of genes 50 .. 150 through the exact route
        X, labels, rng = _counts(3)
        for j in (50, 150):
            X[rng.randint(600), j] = 70.0
        assert (X != 0).mean() >= 0.02
        add(f"3-csr-byte-windows-{test}", X, labels, test, _plain("csr", True), opts={"no_csr_counts_path": 1})
        # 6: k_csc_counts, then the single-kernel route (or the two-kernel route) on the two genes it left
        X, labels, rng = _counts(6, m=64)
        X[rng.randint(600), 9] = 70.0
        X[:, 40] = (X[:, 40] * 0.37).astype(np.float32)
        left = "no_csc_gene_path" if test == "ovo" else "no_csc_ovr_gene_path"
        for fmt_dev, device in (("host", False), ("device", True)):
            add(f"6-csc-counts-leftovers-{fmt_dev}-{test}", X, labels, test, _plain("csc", device))
            add(f"6-csc-counts-leftovers-two-kernel-{fmt_dev}-{test}", X, labels, test, _plain("csc", device), opts={left: 1})
        # 8: deferred count passes, one flagged gene recomputed at synchronize()
        X, labels, rng = _counts(8, m=64)
        X[rng.randint(600), 21] = 70.0
        for fmt in ("csc", "csr"):
            add(f"8-deferred-{fmt}-{test}", X, labels, test, _deferred(fmt))

    # 4: float64 that is float32 throughout (OVR; gene 3 has 20 000 stored entries: k_csc_ovr_gene's key buffer holds them as
    # four-byte keys only)
    X, labels, rng = _continuous(4, 24_000, 16, (4000,) * 6, stored=0.1)
    X[:, 3] = np.exp(rng.normal(0.0, 1.0, size=24_000)).astype(np.float32) * (rng.rand(24_000) < 0.84)
    X = np.log1p(X).astype(np.float32)  # (values that is_log1p takes)
    for fmt in ("csr", "csc"):
        add(f"4-f32-{fmt}", X, labels, "ovr", _plain(fmt, True))
        add(f"4-f64-narrowed-{fmt}", X, labels, "ovr", _plain(fmt, True, np.float64))
        add(f"4-f64-log1p-kept-{fmt}", X, labels, "ovr", _plain(fmt, True, np.float64, is_log1p=True), oracle_kw={"is_log1p": True})
    # 5: CSR -> CSC on the device, scatter form (two rows out of order) and gather form
    X, labels, rng = _continuous(5, 300, 128, (50,) * 6)
    for test in ("ovo", "ovr"):
        add(f"5-csr-transpose-gather-{test}", X, labels, test, _plain("csr", True))
        add(f"5-csr-transpose-scatter-{test}", X, labels, test, _unsorted_rows)
    # 7: two groups of 600 cells, a reference of 600: the two-kernel route with the packed rank kernel
    X, labels, rng = _continuous(7, 1800, 32, (600,) * 3)
    for dtype in (np.float32, np.float64):
        add(f"7-packed-rank-csc-{np.dtype(dtype).name}", X, labels, "ovo", _plain("csc", False, dtype))
    return cases


CASES = _build_cases()

# launches per kernel family, recorded on 50314bb; the rows with a pass 2 of the transposition recorded again (see the module docstring)
TABLE = {
    "1-csr-counts-flagged-runs-ovo": {"k_csc_counts": 2, "k_csc_gene": 2, "k_csr_counts": 1, "k_csr_tile_gather": 2, "k_finalize": 4, "k_fused_tables": 1, "k_sparse_seg": 3, "k_value_sums": 2},
    "1-csr-counts-flagged-runs-ovr": {"k_csc_counts": 2, "k_csc_ovr_gene": 2, "k_csr_counts": 1, "k_csr_tile_gather": 2, "k_finalize": 4, "k_fused_tables": 2, "k_gene_totals": 2, "k_ovr_gene": 1, "k_sparse_seg": 3, "k_value_sums": 2},
    "2-csr-counts-many-flagged-ovo": {"k_csr_counts": 1, "k_fused_tables": 3, "k_ovo_fused": 1, "k_ovo_fused_wide": 1, "k_sparse_seg": 2},
    "2-csr-counts-many-flagged-ovr": {"k_csr_counts": 1, "k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1, "k_ovr_gene": 1, "k_sparse_seg": 2},
    "3-csr-byte-windows-ovo": {"k_fused_tables": 2, "k_ovo_fused": 1, "k_ovo_fused_wide": 1, "k_sparse_seg": 1},
    "3-csr-byte-windows-ovr": {"k_fused_tables": 2, "k_ovo_fused_wide": 1, "k_ovr_fused": 1, "k_sparse_seg": 1},
    "4-f32-csc": {"k_csc_ovr_gene": 1, "k_finalize": 1, "k_gene_totals": 1, "k_value_sums": 1},
    "4-f32-csr": {"k_csc_ovr_gene": 1, "k_csr_counts": 1, "k_csr_tile_gather": 1, "k_finalize": 1, "k_fused_tables": 2, "k_gene_totals": 1, "k_ovr_gene": 1, "k_sparse_seg": 2, "k_value_sums": 1},
    "4-f64-log1p-kept-csc": {"k_csc_ovr_gene": 1, "k_finalize": 2, "k_gene_totals": 2, "k_ovr_gene": 1, "k_sparse_seg": 1, "k_value_sums": 2},
    "4-f64-log1p-kept-csr": {"k_csc_ovr_gene": 1, "k_csr_tile_gather": 1, "k_finalize": 2, "k_gene_totals": 2, "k_ovr_gene": 1, "k_sparse_seg": 2, "k_value_sums": 2},
    "4-f64-narrowed-csc": {"k_csc_ovr_gene": 1, "k_finalize": 1, "k_gene_totals": 1, "k_value_sums": 1},
    "4-f64-narrowed-csr": {"k_csc_ovr_gene": 1, "k_csr_counts": 1, "k_csr_tile_gather": 1, "k_finalize": 1, "k_fused_tables": 2, "k_gene_totals": 1, "k_ovr_gene": 1, "k_sparse_seg": 2, "k_value_sums": 1},
    "5-csr-transpose-gather-ovo": {"k_csc_gene": 1, "k_csr_counts": 1, "k_csr_tile_gather": 1, "k_finalize": 1, "k_fused_tables": 1, "k_sparse_seg": 2, "k_value_sums": 1},
    "5-csr-transpose-gather-ovr": {"k_csc_ovr_gene": 1, "k_csr_counts": 1, "k_csr_tile_gather": 1, "k_finalize": 1, "k_fused_tables": 2, "k_gene_totals": 1, "k_ovr_gene": 1, "k_sparse_seg": 2, "k_value_sums": 1},
    "5-csr-transpose-scatter-ovo": {"k_csc_gene": 1, "k_csr_block_scatter": 1, "k_csr_counts": 1, "k_finalize": 1, "k_fused_tables": 1, "k_sparse_seg": 2, "k_value_sums": 1},
    "5-csr-transpose-scatter-ovr": {"k_csc_ovr_gene": 1, "k_csr_block_scatter": 1, "k_csr_counts": 1, "k_finalize": 1, "k_fused_tables": 2, "k_gene_totals": 1, "k_ovr_gene": 1, "k_sparse_seg": 2, "k_value_sums": 1},
    "6-csc-counts-leftovers-device-ovo": {"k_csc_counts": 1, "k_csc_gene": 1, "k_finalize": 2, "k_value_sums": 1},
    "6-csc-counts-leftovers-device-ovr": {"k_csc_counts": 1, "k_csc_ovr_gene": 1, "k_finalize": 2, "k_gene_totals": 1, "k_value_sums": 1},
    "6-csc-counts-leftovers-host-ovo": {"k_csc_counts": 1, "k_csc_gene": 1, "k_finalize": 2, "k_value_sums": 1},
    "6-csc-counts-leftovers-host-ovr": {"k_csc_counts": 1, "k_csc_ovr_gene": 1, "k_finalize": 2, "k_gene_totals": 1, "k_value_sums": 1},
    "6-csc-counts-leftovers-two-kernel-device-ovo": {"k_csc_counts": 1, "k_finalize": 2, "k_ovo_rank": 1, "k_sparse_seg": 1, "k_value_sums": 1},
    "6-csc-counts-leftovers-two-kernel-device-ovr": {"k_csc_counts": 1, "k_finalize": 2, "k_gene_totals": 1, "k_ovr_gene": 1, "k_sparse_seg": 1, "k_value_sums": 1},
    "6-csc-counts-leftovers-two-kernel-host-ovo": {"k_csc_counts": 1, "k_finalize": 2, "k_ovo_rank": 1, "k_sparse_seg": 1, "k_value_sums": 1},
    "6-csc-counts-leftovers-two-kernel-host-ovr": {"k_csc_counts": 1, "k_finalize": 2, "k_gene_totals": 1, "k_ovr_gene": 1, "k_sparse_seg": 1, "k_value_sums": 1},
    "7-packed-rank-csc-float32": {"k_finalize": 1, "k_group_compact": 1, "k_ovo_rank": 1, "k_ovo_rank_compact": 1, "k_sparse_seg": 1, "k_value_sums": 1},
    "7-packed-rank-csc-float64": {"k_finalize": 1, "k_group_compact": 1, "k_ovo_rank": 1, "k_ovo_rank_compact": 1, "k_sparse_seg": 1, "k_value_sums": 1},
    "8-deferred-csc-ovo": {"k_csc_counts": 2, "k_csc_gene": 1, "k_finalize": 3, "k_value_sums": 1},
    "8-deferred-csc-ovr": {"k_csc_counts": 2, "k_csc_ovr_gene": 1, "k_finalize": 3, "k_gene_totals": 1, "k_value_sums": 1},
    "8-deferred-csr-ovo": {"k_csr_counts": 1, "k_fused_tables": 3, "k_ovo_fused": 1, "k_ovo_fused_wide": 1, "k_sparse_seg": 2},
    "8-deferred-csr-ovr": {"k_csr_counts": 1, "k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1, "k_ovr_gene": 1, "k_sparse_seg": 2},
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_sparse_route_trace(engine, name):
    case = CASES[name]
    launches, got, g = trace(engine, case)
    print(name, launches)
    assert launches == TABLE[name], name
    want = oracle.run(case["X"].astype(np.float64), g, **case["oracle_kw"])
    assert_planes_match(got, want, ref_row=g.encoded_ref_group if case["test"] == "ovo" else None, what=name)
