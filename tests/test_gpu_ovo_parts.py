"""Continuous-value OVO beyond every LDS-resident look-up (illico_amd/csrc/kernels_ovo_compact.h):

* a reference whose non-zero keys outgrow the packed rank kernel's slots is taken in VALUE-RANGE PARTS (k_ovo_rank_compact<.., PARTS>:
  4096 cells over the reference's key range, cut at j / P of the keys; every part adds its share of S2 and of the tie terms);
* a ranked group's run of more keys than k_bucket_big_runs holds in LDS is dealt into value buckets through HBM.

Both replace the reference's linear merge for sizes of any kind (illico/utils/ranking.py:52-158, illico/ovo/dense_ovo.py:111-132).
The limits are lowered by options ("packed_ref_cap", "big_runs_cap") so that small matrices take the routes; every case is held to the
oracle (U exact, p rtol 1e-12) and, bit for bit, to the statistics of the same engine with the routes switched off.
"""
import functools
import re

import numpy as np
import pytest
from scipy import sparse

import oracle
from conftest import assert_planes_match, make_labels

pytestmark = pytest.mark.gpu


@pytest.fixture()
def engine():
    from illico_amd._lib import get_engine
    eng = get_engine()
    eng.set_option("no_fused_path", 1)
    yield eng
    for k in ("no_fused_path", "packed_ref_cap", "big_runs_cap", "no_ovo_parts", "no_big_runs_global", "no_deal_runs", "profile",
              "debug_routes", "no_coop_runs", "no_packed_small_wg"):
        eng.set_option(k, 0)


def _continuous(rng, n, m, zero_frac):
    X = np.log1p(rng.poisson(6.0, size=(n, m)) * rng.uniform(0.5, 1.5, size=(n, m)))
    X *= rng.rand(n, m) >= zero_frac
    return X


def _same(a, b):
    """Two routes of one engine: p-values and statistics bit for bit (integer statistics); fold changes to 1e-13 (dense value sums
    are fixed-order sums of each route's own order)."""
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_allclose(a[2], b[2], rtol=1e-13, atol=0)


def _profiled(engine, run):
    engine.set_option("profile", 1)
    engine.profile_reset()
    try:
        planes = run()
        prof = engine.profile_get()
    finally:
        engine.set_option("profile", 0)
    return planes, prof


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("zero_frac,cap", [(0.0, 1024), (0.4, 1024), (0.0, 2048), (0.4, 3072)])
def test_reference_in_value_range_parts(engine, dtype, zero_frac, cap):
    """A reference of 6000 cells against key slots capped at 1024 / 2048 / 3072: seven parts per gene (every part looks every key up,
    the other parts' lanes masked), four, or two (the groups' runs dealt by part first: k_deal_runs).  Columns: continuous, mixed sign without
    zeros (scaled data), ties between the reference and the groups and inside groups (values rounded to a grid), a column whose
    reference is one value (a cell of the cut holds everything: the gene leaves the route, the general route computes it), a constant
    column, one outlier stretching the key range."""
    rng = np.random.RandomState(12)
    n, m, G = 14000, 40, 30
    labels = make_labels(rng, n, G, n_ref=6000)
    X = _continuous(rng, n, m, zero_frac)
    X[:, 1] = rng.randn(n) * 0.7 + 1.0                        # mixed sign, no zeros
    X[:, 2] = np.round(rng.randn(n) + 1.0, 1)                 # ~80 distinct values of either sign: ties everywhere
    X[:, 3] = np.round(X[:, 3] * 8) / 8                       # a grid: ties among non-zeros
    X[:, 4] = np.where(labels == "non-targeting", 1.5, X[:, 4])   # the reference is ONE value
    X[:, 5] = 2.25
    X[7, 6] = 3.0e30                                          # an outlier: 4095 of the 4096 cells hold nothing
    X[:, 7] = -np.abs(X[:, 7]) - 0.5                          # all negative
    X = X.astype(dtype)
    _, g = oracle.encode_and_count_groups(labels, "non-targeting")
    engine.set_groups(g)
    want = oracle.run(np.ascontiguousarray(X, dtype=np.float64) if dtype == np.float64 else X, g)
    engine.set_option("packed_ref_cap", cap)
    got, prof = _profiled(engine, lambda: engine.run_dense(X, 0, m))
    assert_planes_match(got, want, ref_row=g.encoded_ref_group, what=f"reference in parts {dtype.__name__} zeros {zero_frac} slots {cap}")
    engine.set_option("no_deal_runs", 1)
    try:
        _same(got, engine.run_dense(X, 0, m))                  # (dealt runs or masked look-ups: the same integers)
    finally:
        engine.set_option("no_deal_runs", 0)
    assert "k_ovo_rank_compact" in prof and "k_group_compact" in prof, prof
    stats = engine.rank_statistics(X, 0, m)
    engine.set_option("no_ovo_parts", 1)                      # (with the slots still capped: every gene leaves the kernel)
    old, prof_old = _profiled(engine, lambda: engine.run_dense(X, 0, m))
    stats_old = engine.rank_statistics(X, 0, m)
    _same(got, old)
    np.testing.assert_array_equal(stats[0], stats_old[0])
    np.testing.assert_array_equal(stats[1], stats_old[1])
    # without the parts every gene goes through the general routes (with them: the one-valued reference of gene 4 and what else crowds a part)
    left_old = prof_old.get("k_ovr_gene", {"launches": 0})["launches"] + prof_old.get("k_ovo_rank", {"launches": 0})["launches"]
    assert left_old > 0, (prof, prof_old)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_big_runs_dealt_through_hbm_and_parts_together(engine, dtype):
    """Groups of ~4000 cells (runs of ~2400 non-zero keys) against LDS slots capped at 512 keys: every run is dealt into value buckets
    through the second key buffer; the reference (5000 cells) is taken in parts at the same time (pieces wholly outside a part are
    skipped).  With ties inside the runs and a run that is ONE value (a bucket above 256 keys: that gene leaves the route)."""
    rng = np.random.RandomState(3)
    n, m, G = 25000, 24, 6
    labels = make_labels(rng, n, G, n_ref=5000)
    X = _continuous(rng, n, m, 0.4)
    X[:, 2] = np.round(X[:, 2] * 16) / 16
    X[:, 3] = rng.randn(n) * 0.7 + 1.0                        # mixed sign (a mean away from zero: group sums that cancel have no relative accuracy to hold)
    X[:, 4] = np.where(labels == "pert_00001", 0.75, X[:, 4])
    X = X.astype(dtype)
    _, g = oracle.encode_and_count_groups(labels, "non-targeting")
    engine.set_groups(g)
    want = oracle.run(X, g)
    engine.set_option("big_runs_cap", 512)
    got, prof = _profiled(engine, lambda: engine.run_dense(X, 0, m))
    assert_planes_match(got, want, ref_row=g.encoded_ref_group, what=f"big runs through HBM {dtype.__name__}")
    engine.set_option("packed_ref_cap", 1024)
    got2, prof2 = _profiled(engine, lambda: engine.run_dense(X, 0, m))
    _same(got, got2)
    engine.set_option("no_big_runs_global", 1)
    engine.set_option("no_ovo_parts", 1)
    old, prof_old = _profiled(engine, lambda: engine.run_dense(X, 0, m))
    _same(got, old)
    # (gene 4 leaves the packed route either way; with the routes off, every gene does)
    t = lambda p: p.get("k_ovr_gene", {"launches": 0})["launches"] + p.get("k_ovo_rank", {"launches": 0})["launches"]
    assert "k_ovo_rank_compact" in prof and "k_ovo_rank_compact" in prof2 and t(prof_old) > 0, (prof, prof2, prof_old)


@pytest.mark.parametrize("fmt", ["csc", "csr"])
def test_sparse_input_with_cluster_sized_groups_parts_and_long_runs(engine, fmt):
    """The regrouped sparse route (k_csc_regroup / k_csc_segment + k_seg_to_packed + the packed rank kernel): five clusters of ~6000
    cells, a third of the cells stored -- reference runs of ~2000 keys against slots capped at 1024 (parts), ranked runs of ~2000 keys
    against LDS slots capped at 512 (through HBM)."""
    import torch
    rng = np.random.RandomState(8)
    n, m, G = 30000, 20, 5
    labels = np.array(["non-targeting"] * 6000 + [f"pert_{1 + i % (G - 1):05d}" for i in range(n - 6000)])
    rng.shuffle(labels)
    X = _continuous(rng, n, m, 0.67).astype(np.float32)
    X[:, 1] = np.round(X[:, 1] * 4) / 4
    _, g = oracle.encode_and_count_groups(labels, "non-targeting")
    engine.set_groups(g)
    want = oracle.run(X, g)
    M = (sparse.csc_matrix if fmt == "csc" else sparse.csr_matrix)(X)
    dev = torch.device("cuda", engine.device)
    d, i, p = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (M.data, M.indices, M.indptr))
    run = lambda: engine.run_sparse(fmt, d, i, p, M.shape, 0, m)
    base = run()
    assert_planes_match(base, want, ref_row=g.encoded_ref_group, what=f"sparse clusters {fmt}")
    engine.set_option("packed_ref_cap", 1024)
    engine.set_option("big_runs_cap", 512)
    got, prof = _profiled(engine, run)
    assert_planes_match(got, want, ref_row=g.encoded_ref_group, what=f"sparse clusters {fmt}, parts + runs through HBM")
    for a, b in zip(got, base):
        np.testing.assert_array_equal(a, b)
    assert "k_ovo_rank_compact" in prof, prof


# ---- the PARTS form of the 64-group block loop and of the all-wavefront walk of long runs ----
_LEFT = re.compile(r"\[illico\] packed OVO: \d+ genes, parts \d, left (\d+) to the general route")


def _left_to_general_route(engine, capfd, run):
    """The genes the packed OVO kernels handed back, as the driver reports them with "debug_routes" (dense_driver.h): every gene
    that leaves is recomputed by the general route, so the planes alone would not show a kernel that left them all."""
    engine.set_option("debug_routes", 1)
    capfd.readouterr()
    try:
        planes = run()
    finally:
        engine.set_option("debug_routes", 0)
    lines = _LEFT.findall(capfd.readouterr().err)
    assert lines, "no route line on stderr"
    return planes, sum(int(n) for n in lines)


def _labels_of(rng, n_ref, sizes):
    labels = np.array(["non-targeting"] * n_ref + [f"pert_{1 + k:05d}" for k, s in enumerate(sizes) for _ in range(s)])
    rng.shuffle(labels)
    return labels


def _mixed_sign(rng, n):
    """Either sign, no zeros, magnitudes spread evenly over 2^-60 .. 2^60 and three in four positive.  The bucket kernels cut a run's KEY
    range evenly -- for values of either sign that range spans every exponent below the largest magnitude --, so values crowded around
    one magnitude would share a bucket, and a bucket above 256 keys sends its gene to the general route (float64 keys, 2048 buckets for a run
    of 9000 keys: two binades per bucket)."""
    return np.where(rng.rand(n) < 0.75, 1.0, -1.0) * np.exp2(rng.uniform(-60.0, 60.0, size=n))


def _with_want(X, labels, dtype):
    X = np.ascontiguousarray(X.astype(dtype))
    X.setflags(write=False)
    _, g = oracle.encode_and_count_groups(labels, "non-targeting")
    return X, g, oracle.run(X, g)


BLOCK_LOOP_SIZES = tuple(1 + i % 9 for i in range(520)) + (70, 130, 200, 256, 300)


@functools.lru_cache(maxsize=None)
def _block_loop_case(dtype, zero_frac):
    rng = np.random.RandomState(21)
    labels = _labels_of(rng, 4600, BLOCK_LOOP_SIZES)
    n, m = len(labels), 24
    X = _continuous(rng, n, m, zero_frac)
    X[:, 1] = _mixed_sign(rng, n)
    X[:, 3] = np.round(X[:, 3] * 256) / 256                   # a grid: ties with the reference and inside groups (1/8 .. 1/64 crowd the reference's table)
    X[:, 5] = 2.25                                            # constant: leaves the packed kernels
    X[:, 7] = -np.abs(rng.randn(n)) - 0.5                     # all negative, no zeros
    return _with_want(X, labels, dtype)


# genes left to the general route, recorded on an MI355X on the parent of the commit that split the rank kernel into steps: in every
# case the constant column, and nothing else
BLOCK_LOOP_LEFT = 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("zero_frac", [0.0, 0.4])
@pytest.mark.parametrize("cap", [1024, 2048])
def test_parts_in_the_block_loop(engine, capfd, dtype, zero_frac, cap):
    """PARTS x the 64-group block loop of k_ovo_rank_compact (G = 526 >= 16 wavefronts x 32): a reference of 4600 cells against 520
    groups of 1 .. 9 cells and one each of 70, 130, 200, 256 and 300 (two, three and four look-up rounds; without zeros the last is a
    run above 256 keys inside a block of small groups).  1024 slots: six parts, looked up masked; 2048: three, the runs dealt by
    k_deal_runs (pofs).  The number of genes handed to the general route is a literal recorded on the parent commit on an MI355X."""
    X, g, want = _block_loop_case(dtype, zero_frac)
    m = X.shape[1]
    engine.set_groups(g)
    engine.set_option("packed_ref_cap", cap)
    got, prof = _profiled(engine, lambda: engine.run_dense(X, 0, m))
    assert_planes_match(got, want, ref_row=g.encoded_ref_group, what=f"parts x block loop {dtype.__name__} zeros {zero_frac} slots {cap}")
    assert "k_ovo_rank_compact" in prof, prof
    again, left = _left_to_general_route(engine, capfd, lambda: engine.run_dense(X, 0, m))
    print("left", dtype.__name__, zero_frac, cap, left)
    _same(got, again)
    assert left == BLOCK_LOOP_LEFT
    engine.set_option("no_deal_runs", 1)
    try:
        _same(got, engine.run_dense(X, 0, m))
    finally:
        engine.set_option("no_deal_runs", 0)
    stats = engine.rank_statistics(X, 0, m)
    engine.set_option("no_ovo_parts", 1)
    _same(got, engine.run_dense(X, 0, m))
    stats_old = engine.rank_statistics(X, 0, m)
    np.testing.assert_array_equal(stats[0], stats_old[0])
    np.testing.assert_array_equal(stats[1], stats_old[1])


LONG_RUN_SIZES = (9000, 8300, 300, 100)


@functools.lru_cache(maxsize=None)
def _long_run_case(dtype):
    rng = np.random.RandomState(22)
    labels = _labels_of(rng, 2500, LONG_RUN_SIZES)
    n, m = len(labels), 8
    X = _continuous(rng, n, m, 0.0)
    X[:, 1] = np.round(X[:, 1] * 256) / 256                   # a grid: ties everywhere, no value 256 times in a run (1/64 crowds the reference's table)
    X[:, 2] = _mixed_sign(rng, n)
    X[:, 3] = -np.abs(X[:, 3]) - 0.5                          # all negative
    return _with_want(X, labels, dtype)


LONG_RUN_LEFT = 0  # recorded likewise: in every case nothing leaves


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("big_runs_cap", [0, 512])
def test_parts_in_the_cooperative_walk(engine, capfd, dtype, big_runs_cap):
    """PARTS x the walk of runs above OCR_COOP_MIN = 8192 keys by all the wavefronts (lr_list / lr_acc): groups of 9000 and 8300 cells
    without zeros (both listed), one of 300 (walked by one wavefront) and one of 100, against a reference of 2500 cells in three parts
    (1024 slots).  Runs dealt in LDS (cap 0) or through the second key buffer, cuts by k_bucket_big_runs_global (512).  Nothing is
    expected to leave the packed kernels: the literal was recorded on the parent commit on an MI355X."""
    X, g, want = _long_run_case(dtype)
    m = X.shape[1]
    engine.set_groups(g)
    engine.set_option("packed_ref_cap", 1024)
    engine.set_option("big_runs_cap", big_runs_cap)
    got, prof = _profiled(engine, lambda: engine.run_dense(X, 0, m))
    assert_planes_match(got, want, ref_row=g.encoded_ref_group, what=f"parts x cooperative walk {dtype.__name__} cap {big_runs_cap}")
    assert "k_ovo_rank_compact" in prof, prof
    again, left = _left_to_general_route(engine, capfd, lambda: engine.run_dense(X, 0, m))
    print("left", dtype.__name__, big_runs_cap, left)
    _same(got, again)
    assert left == LONG_RUN_LEFT
    engine.set_option("no_coop_runs", 1)
    try:
        _same(got, engine.run_dense(X, 0, m))
    finally:
        engine.set_option("no_coop_runs", 0)
    engine.set_option("no_ovo_parts", 1)
    _same(got, engine.run_dense(X, 0, m))
