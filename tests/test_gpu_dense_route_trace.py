"""Which steps a dense call takes, pinned by the launches per kernel family: the counterpart of test_gpu_sparse_route_trace.py
for dense_driver.h.

Every case runs once under `engine.profile(True)`; `profile_get()` -- launches per kernel family, every family, nothing left out --
is compared with a literal table, then the planes (and the z plane, where the case asks for one) with the oracle.

The table was recorded by running these very cases on commit 7448299 (the parent of the commit that split the dense driver into
route steps), on an MI355X, where every case's planes matched the oracle; it is not computed by the code under test.

Unless a case says otherwise: 600 cells, six groups of 100 (the first the reference of "ovo"), 256 genes, float32 Poisson(3) counts
capped at 60, device-resident.  Each case names the step of dense_driver.h it must reach.

What a profile can and cannot tell.  It counts profiled scopes, not launches, and a family covers every instance of its kernels.  So
k_fused_tables is 3 for OVO both with the reference pass split over row chunks (256 genes) and with one workgroup per tile (case 04:
6400 genes, 100 tiles) -- the reference pass, k_wide_decide, the 256-value tables; it is 1 where groups above 255 cells rule the
256-value stage out (02, 03, 15) and 2 where k_wide_decide is not asked (06 with either option).  The cell width of k_ovo_fused
(01 / 02 / 03), the one-pass and the two-pass form of OVR (01 / 07 and 03: both k_ovr_fused), the 256-value stage with work to do and
without (05 / 01), the Z instances (09) and a column window (11) have the rows of case 01: there the planes are the check -- the genes of
05 would otherwise show as k_gather_columns and a two-pass route.  13 and 14 have one row as well: k_ovo_rank over the packed layout
is launched for every batch and returns at once for the genes the packed kernel kept.
What the other rows show: k_group_value_hists for the three ways into the histogram route (03 without the option, 08); 06 and 10 the
256-value stage on the narrow matrix (k_ovo_fused_wide twice, k_gather_columns for the gather and for k_scatter_planes) against once,
in place, with either option; 12 the gathered genes through k_ovo_counts / k_ovr_counts, and k_ovr_partition + k_ovr_rank_parts for
the run that k_ovr_counts flagged; 15 k_gather_columns once and two k_finalize against three k_finalize for two column runs; 16 / 18
k_transpose_permute; 17 k_ovr_gene; 19 every per-batch family four times; 20 five windows and the flagged gene as a column run
(k_group_compact), 21 the same gene gathered on the device (k_gather_columns, k_ovo_counts / k_ovr_counts) or, without the gather, as a
run; 22 no fused family at all.  Case 06 takes 512 genes: k_wide_decide leaves the stage to the host from eight flagged tiles on.  Case
18 needs no_packed_dense as well to reach k_ovo_counts (without it the counts take the packed route: 18-no-fused-path-packed).
"""
import functools

import numpy as np
import pytest

import oracle
from conftest import assert_planes_match
from route_trace import groups, labels as make_labels, trace
from threshold_cases import z_want_fast

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import get_engine
    return get_engine()


# ---- inputs, built on first use and then shared (never modified) ----
def _counts(seed, n=600, m=256, sizes=(100,) * 6):
    rng = np.random.RandomState(seed)
    X = np.minimum(rng.poisson(3.0, size=(n, m)), 60).astype(np.float32)
    return X, make_labels(rng, list(sizes)), rng


def _continuous(seed, n=600, m=256, sizes=(100,) * 6):
    rng = np.random.RandomState(seed)
    X = np.exp(rng.normal(0.0, 1.0, size=(n, m))).astype(np.float32)
    return X, make_labels(rng, list(sizes)), rng


def _d_plain():
    return _counts(1)[:2]


def _d_groups300():
    return _counts(2, n=1800, sizes=(300,) * 6)[:2]


def _d_big_group():  # the second group has 66 000 cells: beyond the 16-bit cells of every fused form
    return _counts(3, n=70_000, m=64, sizes=(800, 66_000, 800, 800, 800, 800))[:2]


def _d_many_tiles():
    return _counts(4, m=6400)[:2]


def _d_wide_in_place():  # counts of 64 .. 255 in genes of two tiles: fewer tiles than k_wide_decide leaves to the host (8)
    X, lab, rng = _counts(5)
    for j in (10, 30, 200):
        X[rng.randint(600, size=5), j] = rng.randint(64, 256, size=5)
    return X, lab


def _d_wide_every_tile():  # 512 genes: eight tiles, one gene with counts of 64 .. 255 in each
    X, lab, rng = _counts(6, m=512)
    for t in range(8):
        X[rng.randint(600, size=5), t * 64 + 5 + t] = rng.randint(64, 256, size=5)
    return X, lab


def _d_ragged():  # the second group alone has 5000 of the 6000 cells
    return _counts(8, n=6000, sizes=[20, 5000] + [20] * 49)[:2]


def _d_leftovers():  # three scattered genes above 255, one fractional gene, one gene beyond OVRC_R (32768)
    X, lab, rng = _counts(12)
    for j in (20, 100, 200):
        X[rng.randint(600), j] = 300.0
    X[:, 150] *= np.float32(0.37)
    X[rng.randint(600), 60] = 40_000.0
    return X, lab


def _d_continuous():
    return _continuous(13)[:2]


def _d_tie_heavy():
    X, lab, rng = _continuous(14)
    X[:, 17] = rng.poisson(300.0, size=600)
    return X, lab


def _d_redo():  # a reference and two groups of 1100 cells: beyond what k_ovo_rank takes over the packed layout
    X, lab, rng = _continuous(15, n=3300, sizes=(1100,) * 3)
    for j in (10, 200):
        X[:, j] = rng.poisson(300.0, size=3300)
    return X, lab


def _d_host_counts():  # 320 genes: five windows of 64; gene 70 holds a value above 255
    X, lab, rng = _counts(20, m=320)
    X[rng.randint(600), 70] = 300.0
    return X, lab


def _d_host_continuous():
    return _continuous(22)[:2]


@functools.lru_cache(maxsize=None)
def _data(maker):
    X, lab = maker()
    X.setflags(write=False)
    return X, lab


@functools.lru_cache(maxsize=None)
def _want(maker, test, lb):
    X, lab = _data(maker)
    g = groups(lab, test)
    return oracle.run(X.astype(np.float64), g, col_lb=lb, col_ub=X.shape[1])


# ---- how a case calls the engine ----
def _device(lb=0, **kw):
    def run(engine, X):
        import torch
        return engine.run_dense(torch.tensor(X).cuda(), lb, X.shape[1], **kw)
    return run


def _host(**kw):
    def run(engine, X):
        return engine.run_dense(X, 0, X.shape[1], **kw)
    return run


def _deferred(engine, X):
    import torch
    planes = engine.run_dense(torch.tensor(X).cuda(), 0, X.shape[1], device_out=True, defer=True)
    engine.synchronize()
    return tuple(t.cpu().numpy() for t in planes)


def _build_cases():
    cases = {}

    def add(name, maker, tests, run, opts=None, lb=0, scores=False):
        for test in tests:
            cases[f"{name}-{test}"] = dict(maker=maker, test=test, run=run, opts=opts or {}, lb=lb, scores=scores)

    both = ("ovo", "ovr")
    # ---- the fused pass (run_fused_ovo) ----
    add("01-plain", _d_plain, both, _device())
    add("02-groups-of-300", _d_groups300, both, _device())
    add("03-group-of-66000-no-hist-route", _d_big_group, both, _device(), {"no_group_hist_route": 1})
    add("03-group-of-66000-hist-route", _d_big_group, both, _device())
    add("04-6400-genes", _d_many_tiles, ("ovo",), _device())
    add("05-wide-in-place", _d_wide_in_place, both, _device())
    add("06-wide-left-to-host", _d_wide_every_tile, both, _device())
    add("06-wide-no-wide-gather", _d_wide_every_tile, both, _device(), {"no_wide_gather": 1})
    add("06-wide-no-leftover-gather", _d_wide_every_tile, both, _device(), {"no_leftover_gather": 1})
    add("07-no-ovr-one-pass", _d_plain, ("ovr",), _device(), {"no_ovr_one_pass": 1})
    add("08-hist-route-few", _d_plain, both, _device(), {"group_hist_min_cells": 1})
    add("08-hist-route-ragged", _d_ragged, both, _device(), {"group_hist_min_cells": 1, "group_hist_max_wgs": 1})
    add("09-scores-plain", _d_plain, both, _device(scores=True), scores=True)
    add("09-scores-wide-in-place", _d_wide_in_place, both, _device(scores=True), scores=True)
    add("10-deferred-wide-left-to-host", _d_wide_every_tile, both, _deferred)
    add("11-column-window", _d_plain, both, _device(lb=3), lb=3)
    # ---- leftovers and the two-pass routes (run_leftovers, run_dense_twopass) ----
    add("12-gathered-leftovers", _d_leftovers, both, _device())
    add("13-continuous", _d_continuous, both, _device())
    add("14-tie-heavy-column", _d_tie_heavy, ("ovo",), _device())
    add("15-redo-gathered", _d_redo, ("ovo",), _device())
    add("15-redo-as-runs", _d_redo, ("ovo",), _device(), {"no_leftover_gather": 1})
    add("16-no-packed-dense", _d_continuous, both, _device(), {"no_packed_dense": 1})
    add("17-no-ovr-parts-path", _d_continuous, ("ovr",), _device(), {"no_ovr_parts_path": 1})
    add("18-no-fused-path-packed", _d_plain, ("ovo",), _device(), {"no_fused_path": 1})
    add("18-no-fused-path", _d_plain, ("ovo",), _device(), {"no_fused_path": 1, "no_packed_dense": 1})
    add("19-four-batches", _d_continuous, both, _device(), {"gene_batch": 64})
    # ---- host-resident input (run_dense_t, the window pipeline) ----
    add("20-host-byte-windows", _d_host_counts, both, _host(), {"gene_batch": 64})
    add("21-host-float-windows", _d_host_counts, both, _host(), {"gene_batch": 64, "host_narrow": -1})
    add("21-host-float-windows-no-gather", _d_host_counts, both, _host(), {"gene_batch": 64, "host_narrow": -1, "no_leftover_gather": 1})
    add("22-host-continuous", _d_host_continuous, both, _host())
    return cases


CASES = _build_cases()

# launches per kernel family, recorded on 7448299 (see the module docstring)
TABLE = {
    "01-plain-ovo": {"k_fused_tables": 3, "k_ovo_fused": 1, "k_ovo_fused_wide": 1},
    "01-plain-ovr": {"k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "02-groups-of-300-ovo": {"k_fused_tables": 1, "k_ovo_fused": 1},
    "02-groups-of-300-ovr": {"k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "03-group-of-66000-hist-route-ovo": {"k_fused_tables": 2, "k_group_value_hists": 1},
    "03-group-of-66000-hist-route-ovr": {"k_fused_tables": 4, "k_group_value_hists": 1, "k_ovo_fused_wide": 1},
    "03-group-of-66000-no-hist-route-ovo": {"k_fused_tables": 1, "k_ovo_fused": 1},
    "03-group-of-66000-no-hist-route-ovr": {"k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "04-6400-genes-ovo": {"k_fused_tables": 3, "k_ovo_fused": 1, "k_ovo_fused_wide": 1},
    "05-wide-in-place-ovo": {"k_fused_tables": 3, "k_ovo_fused": 1, "k_ovo_fused_wide": 1},
    "05-wide-in-place-ovr": {"k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "06-wide-left-to-host-ovo": {"k_fused_tables": 4, "k_gather_columns": 2, "k_ovo_fused": 1, "k_ovo_fused_wide": 2},
    "06-wide-left-to-host-ovr": {"k_fused_tables": 5, "k_gather_columns": 2, "k_ovo_fused_wide": 2, "k_ovr_fused": 1},
    "06-wide-no-leftover-gather-ovo": {"k_fused_tables": 2, "k_ovo_fused": 1, "k_ovo_fused_wide": 1},
    "06-wide-no-leftover-gather-ovr": {"k_fused_tables": 3, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "06-wide-no-wide-gather-ovo": {"k_fused_tables": 2, "k_ovo_fused": 1, "k_ovo_fused_wide": 1},
    "06-wide-no-wide-gather-ovr": {"k_fused_tables": 3, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "07-no-ovr-one-pass-ovr": {"k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "08-hist-route-few-ovo": {"k_fused_tables": 2, "k_group_value_hists": 1},
    "08-hist-route-few-ovr": {"k_fused_tables": 4, "k_group_value_hists": 1, "k_ovo_fused_wide": 1},
    "08-hist-route-ragged-ovo": {"k_fused_tables": 2, "k_group_value_hists": 1},
    "08-hist-route-ragged-ovr": {"k_fused_tables": 4, "k_group_value_hists": 1, "k_ovo_fused_wide": 1},
    "09-scores-plain-ovo": {"k_fused_tables": 3, "k_ovo_fused": 1, "k_ovo_fused_wide": 1},
    "09-scores-plain-ovr": {"k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "09-scores-wide-in-place-ovo": {"k_fused_tables": 3, "k_ovo_fused": 1, "k_ovo_fused_wide": 1},
    "09-scores-wide-in-place-ovr": {"k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "10-deferred-wide-left-to-host-ovo": {"k_fused_tables": 4, "k_gather_columns": 2, "k_ovo_fused": 1, "k_ovo_fused_wide": 2},
    "10-deferred-wide-left-to-host-ovr": {"k_fused_tables": 5, "k_gather_columns": 2, "k_ovo_fused_wide": 2, "k_ovr_fused": 1},
    "11-column-window-ovo": {"k_fused_tables": 3, "k_ovo_fused": 1, "k_ovo_fused_wide": 1},
    "11-column-window-ovr": {"k_fused_tables": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1},
    "12-gathered-leftovers-ovo": {"k_finalize": 1, "k_fused_tables": 3, "k_gather_columns": 1, "k_ovo_counts": 1, "k_ovo_fused": 1, "k_ovo_fused_wide": 1, "k_ovo_rank": 1, "k_transpose_permute": 1},
    "12-gathered-leftovers-ovr": {"k_finalize": 1, "k_fused_tables": 4, "k_gather_columns": 1, "k_gene_totals": 2, "k_ovo_fused_wide": 1, "k_ovr_counts": 1, "k_ovr_fused": 1, "k_ovr_partition": 2, "k_ovr_rank_parts": 2, "k_transpose_permute": 1, "k_value_sums": 2},
    "13-continuous-ovo": {"k_finalize": 1, "k_fused_tables": 3, "k_group_compact": 1, "k_ovo_fused": 1, "k_ovo_fused_wide": 1, "k_ovo_rank": 1, "k_ovo_rank_compact": 1},
    "13-continuous-ovr": {"k_finalize": 1, "k_fused_tables": 4, "k_gene_totals": 1, "k_group_compact": 1, "k_ovo_fused_wide": 1, "k_ovr_fused": 1, "k_ovr_partition": 1, "k_ovr_rank_parts": 1},
    "14-tie-heavy-column-ovo": {"k_finalize": 1, "k_fused_tables": 3, "k_group_compact": 1, "k_ovo_fused": 1, "k_ovo_fused_wide": 1, "k_ovo_rank": 1, "k_ovo_rank_compact": 1},
    "15-redo-as-runs-ovo": {"k_finalize": 3, "k_fused_tables": 1, "k_group_compact": 2, "k_ovo_counts": 2, "k_ovo_fused": 1, "k_ovo_rank_compact": 1, "k_ovr_gene": 2, "k_transpose_permute": 2},
    "15-redo-gathered-ovo": {"k_finalize": 2, "k_fused_tables": 1, "k_gather_columns": 1, "k_group_compact": 2, "k_ovo_counts": 1, "k_ovo_fused": 1, "k_ovo_rank_compact": 1, "k_ovr_gene": 1, "k_transpose_permute": 1},
    "16-no-packed-dense-ovo": {"k_finalize": 1, "k_fused_tables": 3, "k_ovo_counts": 1, "k_ovo_fused": 1, "k_ovo_fused_wide": 1, "k_ovo_rank": 1, "k_transpose_permute": 1},
    "16-no-packed-dense-ovr": {"k_finalize": 1, "k_fused_tables": 4, "k_gene_totals": 1, "k_ovo_fused_wide": 1, "k_ovr_fused": 1, "k_ovr_partition": 1, "k_ovr_rank_parts": 1, "k_transpose_permute": 1, "k_value_sums": 1},
    "17-no-ovr-parts-path-ovr": {"k_finalize": 1, "k_fused_tables": 4, "k_gene_totals": 1, "k_group_compact": 1, "k_ovo_fused_wide": 1, "k_ovr_fused": 1, "k_ovr_gene": 1},
    "18-no-fused-path-ovo": {"k_finalize": 1, "k_ovo_counts": 1, "k_ovo_rank": 1, "k_transpose_permute": 1},
    "18-no-fused-path-packed-ovo": {"k_finalize": 1, "k_group_compact": 1, "k_ovo_rank": 1, "k_ovo_rank_compact": 1},
    "19-four-batches-ovo": {"k_finalize": 4, "k_fused_tables": 3, "k_group_compact": 4, "k_ovo_fused": 1, "k_ovo_fused_wide": 1, "k_ovo_rank": 4, "k_ovo_rank_compact": 4},
    "19-four-batches-ovr": {"k_finalize": 4, "k_fused_tables": 4, "k_gene_totals": 4, "k_group_compact": 4, "k_ovo_fused_wide": 1, "k_ovr_fused": 1, "k_ovr_partition": 4, "k_ovr_rank_parts": 4},
    "20-host-byte-windows-ovo": {"k_finalize": 1, "k_fused_tables": 10, "k_group_compact": 1, "k_ovo_fused": 5, "k_ovo_fused_wide": 5, "k_ovo_rank": 1, "k_ovo_rank_compact": 1},
    "20-host-byte-windows-ovr": {"k_finalize": 1, "k_fused_tables": 10, "k_gene_totals": 1, "k_group_compact": 1, "k_ovo_fused_wide": 5, "k_ovr_fused": 5, "k_ovr_partition": 1, "k_ovr_rank_parts": 1},
    "21-host-float-windows-no-gather-ovo": {"k_finalize": 1, "k_fused_tables": 10, "k_group_compact": 1, "k_ovo_fused": 5, "k_ovo_fused_wide": 5, "k_ovo_rank": 1, "k_ovo_rank_compact": 1},
    "21-host-float-windows-no-gather-ovr": {"k_finalize": 1, "k_fused_tables": 10, "k_gene_totals": 1, "k_group_compact": 1, "k_ovo_fused_wide": 5, "k_ovr_fused": 5, "k_ovr_partition": 1, "k_ovr_rank_parts": 1},
    "21-host-float-windows-ovo": {"k_finalize": 1, "k_fused_tables": 10, "k_gather_columns": 1, "k_ovo_counts": 1, "k_ovo_fused": 5, "k_ovo_fused_wide": 5, "k_ovo_rank": 1, "k_transpose_permute": 1},
    "21-host-float-windows-ovr": {"k_finalize": 1, "k_fused_tables": 10, "k_gather_columns": 1, "k_ovo_fused_wide": 5, "k_ovr_counts": 1, "k_ovr_fused": 5, "k_transpose_permute": 1},
    "22-host-continuous-ovo": {"k_finalize": 1, "k_group_compact": 1, "k_ovo_rank": 1, "k_ovo_rank_compact": 1},
    "22-host-continuous-ovr": {"k_finalize": 1, "k_gene_totals": 1, "k_group_compact": 1, "k_ovr_partition": 1, "k_ovr_rank_parts": 1},
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_route_trace(engine, name):
    case = CASES[name]
    X, lab = _data(case["maker"])
    launches, got, g = trace(engine, dict(case, X=X, labels=lab))
    print(name, launches)
    assert launches == TABLE[name], name
    ref_row = g.encoded_ref_group if case["test"] == "ovo" else None
    assert_planes_match(got[:3], _want(case["maker"], case["test"], case["lb"]), ref_row=ref_row, what=name)
    if case["scores"]:
        want_z = z_want_fast(X, g, got[1])
        assert np.array_equal(np.ascontiguousarray(got[3]).view(np.uint64), want_z.view(np.uint64)), f"z plane {name}"


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_deferred_call_takes_the_waited_calls_steps(test):
    """resolve_pending hands a deferred call's flags to run_leftovers: from there on it is the waited call."""
    assert TABLE[f"10-deferred-wide-left-to-host-{test}"] == TABLE[f"06-wide-left-to-host-{test}"]
