"""Every group-size, reference-size, group-count and cell-count switch point of the drivers, one cell below and at / above it, on
columns whose tie blocks are as large as a whole group (tests/threshold_cases.py; the observed kernels per side: DESIGN.md section 12).

Each case goes through all five input forms of one Engine, with and without the z-score plane: U exact, p and fold change at rtol 1e-12
against the CPU oracle, z bit for bit against the float64 restatement.  z does not underflow: it still sees the tie sum where p is 0."""
import numpy as np
import pytest
from scipy import sparse

import oracle
import threshold_cases as tc
from conftest import assert_planes_match

pytestmark = pytest.mark.gpu

INPUTS = ("dense-host", "dense-device", "csc-host", "csr-host", "csr-device")

# the routes behind the first-line kernels, for the cases of tc.SECOND_LINE: option set -> the inputs it is run on
SECOND_LINE_OPTIONS = (
    ({"no_fused_path": 1}, ("dense-device", "csc-host", "csr-host")),
    ({"no_fused_path": 1, "no_packed_dense": 1}, ("dense-device", "csc-host", "csr-host")),
    ({"no_csc_counts_path": 1}, ("csc-host", "csr-host")),
    ({"no_csr_counts_path": 1}, ("csc-host", "csr-host")),
    ({"no_dense_window_path": 1}, ("dense-device", "csc-host", "csr-host")),
    ({"no_group_hist_route": 1}, ("dense-device", "csc-host", "csr-host")),
)


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


_cache = {}


def _case(name):   # one case at a time: its tests are neighbours in the run
    if name not in _cache:
        _cache.clear()
        c = tc.make(name)
        K = tc.count_form(c)
        _cache[name] = (c, {"": (c.X, sparse.csc_matrix(c.X), sparse.csr_matrix(c.X)), "counts": (K, sparse.csc_matrix(K), sparse.csr_matrix(K))})
    return _cache[name]


# What reaches the count-valued routes of the sparse drivers (k_csc_counts, k_csr_counts, the dense byte windows of CSR input):
#  * CSC asks a sample of the WINDOW's stored values: more than 2 % of them negative or fractional and k_csc_counts is not tried.  Columns
#    0-2 of a case (around 1, 9 and 62) are a count-valued window; column 5 (around 0) holds -1 and columns 6-9 negatives and fractions.
#  * CSR asks a sample of the WHOLE matrix, whatever window the call names, and wants fewer than 30 % of the cells stored: no window of a
#    case's own matrix passes.  tc.count_form is the case as a matrix that does ("counts" below).
COUNT_WINDOW = (0, 3)
SPARSE_INPUTS = ("csc-host", "csr-host", "csr-device")
# the profile's names for the kernels of launch_csr_counts_route (sparse_driver.h): a CSR call whose profile holds nothing else took every
# plane from that pass -- its verdict was good and no gene left it (a gene that leaves is redone by the sort routes, under their names)
# That reading rests on the routes that redo a call or a gene launching at least one kernel outside this set (today k_ovo_fused,
# k_ovr_fused, k_csc_gene, k_csc_ovr_gene, k_finalize; pass 2 of the CSR -> CSC transposition has names of its own, k_csr_tile_gather and
# k_csr_block_scatter): k_sparse_seg, k_fused_tables and k_ovr_gene are names they share with this pass.
# A new fall-back route made of those three names alone would pass unseen; give it a profile name of its own.
CSR_COUNTS_ROUTE = {"k_sparse_seg", "k_fused_tables", "k_csr_counts", "k_ovr_gene"}
# ... and for those of run_csc_counts_route (k_finalize: the statistics into planes; k_value_sums / k_gene_totals: the fold change)
CSC_COUNTS_ROUTE = {"k_csc_counts", "k_finalize", "k_value_sums", "k_gene_totals"}


def run_input(engine, fmt, X, C, R, window=None, **kw):
    """One call on one input form, over all genes or a window of them; host planes."""
    import torch
    lb, ub = window or (0, X.shape[1])
    if fmt == "dense-host":
        return engine.run_dense(X, lb, ub, **kw)
    if fmt == "dense-device":
        return tuple(t.cpu().numpy() for t in engine.run_dense(torch.from_numpy(X).cuda(), lb, ub, device_out=True, **kw))
    if fmt == "csc-host":
        return engine.run_sparse("csc", C.data, C.indices, C.indptr, C.shape, lb, ub, **kw)
    if fmt == "csr-host":
        return engine.run_sparse("csr", R.data, R.indices, R.indptr, R.shape, lb, ub, **kw)
    assert fmt == "csr-device"
    d, i, p = (torch.from_numpy(a).cuda() for a in (R.data, R.indices, R.indptr))
    return engine.run_sparse("csr", d, i, p, R.shape, lb, ub, **kw)


def _check(got, want, g, X, what, window=None):
    if window:
        want, X = tuple(w[:, window[0]:window[1]] for w in want), X[:, window[0]:window[1]]
    assert_planes_match(got[:3], want, ref_row=g.encoded_ref_group, what=what)
    if len(got) == 4:
        z, zw = got[3], tc.z_want_fast(X, g, got[1])
        bad = np.argwhere(tc.bits(z) != tc.bits(zw))
        assert bad.size == 0, f"z {what}: {bad.shape[0]} entries differ, first (group, gene) {tuple(bad[0])}: {z[tuple(bad[0])]!r} != {zw[tuple(bad[0])]!r}"


@pytest.mark.parametrize("test", ["ovo", "ovr"])
@pytest.mark.parametrize("name", tc.NAMES)
def test_every_input_matches_the_oracle(engine, name, test):
    c, forms = _case(name)
    X, C, R = forms[""]
    K, KC, KR = forms["counts"]
    g = tc.groups(c.labels, test)
    want, want_k = oracle.run(X, g), oracle.run(K, g)
    engine.set_groups(g)
    for fmt in INPUTS:
        _check(run_input(engine, fmt, X, C, R), want, g, X, f"{name} {test} {fmt}")
    for fmt in INPUTS:   # the Z = true instantiations of the same routes
        _check(run_input(engine, fmt, X, C, R, scores=True), want, g, X, f"{name} {test} {fmt} scores")
    for fmt in INPUTS:   # k_csc_counts on the CSC input
        _check(run_input(engine, fmt, X, C, R, COUNT_WINDOW, scores=True), want, g, X, f"{name} {test} {fmt} genes 0-2", COUNT_WINDOW)
    for fmt in SPARSE_INPUTS:   # k_csr_counts on the CSR inputs
        _check(run_input(engine, fmt, K, KC, KR, scores=True), want_k, g, K, f"{name} {test} {fmt} count form")


@pytest.mark.parametrize("test", ["ovo", "ovr"])
@pytest.mark.parametrize("name", tc.SECOND_LINE)
def test_second_line_kernels_match_the_oracle(engine, name, test):
    c, forms = _case(name)
    X, C, R = forms[""]
    K, KC, KR = forms["counts"]
    g = tc.groups(c.labels, test)
    want, want_k = oracle.run(X, g), oracle.run(K, g)
    engine.set_groups(g)
    for opts, inputs in SECOND_LINE_OPTIONS:
        for k, v in opts.items():
            engine.set_option(k, v)
        try:
            for fmt in inputs:
                _check(run_input(engine, fmt, X, C, R, scores=True), want, g, X, f"{name} {test} {fmt} {opts}")
                _check(run_input(engine, fmt, X, C, R, COUNT_WINDOW, scores=True), want, g, X, f"{name} {test} {fmt} genes 0-2 {opts}", COUNT_WINDOW)
                if fmt in SPARSE_INPUTS:   # (with k_csr_counts off the count form takes the dense byte windows, with those off the sort routes)
                    _check(run_input(engine, fmt, K, KC, KR, scores=True), want_k, g, K, f"{name} {test} {fmt} count form {opts}")
        finally:
            for k in opts:
                engine.set_option(k, 0)


@pytest.mark.parametrize("groups_per_wg", [64, 128, 130])
def test_packed_fields_full(engine, groups_per_wg):
    """k_ovr_group_hists adds a workgroup's 8-bit cells, two at a time, as 16-bit fields into one LDS histogram: 128 groups x 255 cells is
    what a field holds, and the driver caps the groups of a workgroup there.  130 groups of 255 cells, each at one value, with as many
    groups per workgroup as the option asks for (the default is 4 to 16) and the group-histogram route off."""
    c, forms = _case("packed-130x255")
    _, C, R = forms[""]
    g = tc.groups(c.labels, "ovr")
    want = oracle.run(c.X, g)
    engine.set_groups(g)
    opts = {"no_group_hist_route": 1, "fused_groups_per_wg": groups_per_wg}
    for k, v in opts.items():
        engine.set_option(k, v)
    engine.profile(True)
    engine.profile_reset()
    try:
        got = run_input(engine, "dense-device", c.X, C, R, scores=True)
        prof = engine.profile_get()
    finally:
        engine.profile(False)
        for k in opts:
            engine.set_option(k, 0)
    assert "k_ovr_fused" in prof and "k_group_value_hists" not in prof, sorted(prof)
    _check(got, want, g, c.X, f"packed-130x255 ovr dense-device {opts}")


def kernels_of(engine, name, test, spec):
    """The kernel names (profile_get) that one input of a case launches.  spec: an input form, "csc-host/window" for that input over
    COUNT_WINDOW, "csr-host/counts" for that input of the case's count form."""
    fmt, _, how = spec.partition("/")
    c, forms = _case(name)
    X, C, R = forms["counts" if how == "counts" else ""]
    engine.set_groups(tc.groups(c.labels, test))
    engine.profile(True)
    try:
        engine.profile_reset()
        run_input(engine, fmt, X, C, R, COUNT_WINDOW if how == "window" else None)
        return set(engine.profile_get())
    finally:
        engine.profile(False)


# (below, at / above, test, input, kernel, the side that launches it) -- where the driver code says that the two sides launch different
# kernels.  The switches that are template parameters of one kernel name are listed in DESIGN.md section 12 and assert nothing.
ALL, SPARSE = INPUTS, SPARSE_INPUTS
CSR_COUNTS = ("csr-host/counts", "csr-device/counts")
EDGES = tuple((lo, hi, test, fmt, kernel, side) for lo, hi, tests, fmts, kernel, side in (
    # dense_driver.h: the 256-value second pass of the fused OVO route while no ranked group exceeds 255 cells
    ("top-255", "top-256", ("ovo",), ("dense-device",), "k_ovo_fused_wide", "below"),
    # sparse_driver.h sparse_packed_rank_fits: groups of at most 256 cells stay with k_csc_gene, larger ones take the packed rank kernel
    ("top-256", "top-257", ("ovo",), SPARSE, "k_csc_gene", "below"),
    ("top-256", "top-257", ("ovo",), SPARSE, "k_ovo_rank_compact", "above"),
    # keyed_driver.h packed_leftovers_fit_sort_route: k_ovo_rank takes what the packed kernel leaves up to 1024 cells per group
    ("ranked-1024", "ranked-1025", ("ovo",), ALL, "k_ovo_rank", "below"),
    ("ranked-1024", "ranked-1025", ("ovo",), ("dense-host", "dense-device"), "k_transpose_permute", "above"),
    # core.hip counts_path_allowed: 16-bit group bins of the two-pass histogram route
    ("ranked-65535", "ranked-65536", ("ovo",), ALL, "k_ovo_counts", "below"),
    # sparse_driver.h csr_counts_route_fits: a reference below 30000 cells, 16-bit group codes, at most CSRC_MAX_BIG = 16 ranked groups
    # above 255 cells (core.hip csr_n_big; an OVR call ranks the 3000-cell group of big-16 as well: 17 on both sides)
    ("ref-29999", "ref-30000", ("ovo",), CSR_COUNTS, "k_csr_counts", "below"),
    ("singles-65535", "singles-65536", ("ovo", "ovr"), CSR_COUNTS, "k_csr_counts", "below"),
    ("big-16", "big-17", ("ovo",), CSR_COUNTS, "k_csr_counts", "below"),
    # dense_driver.h: the group-histogram route from group_hist_min_cells = 32768 cells on
    ("cells-32767", "cells-32768", ("ovo", "ovr"), ("dense-device",), "k_group_value_hists", "above"),
    ("cells-32767", "cells-32768", ("ovo",), ("dense-device",), "k_ovo_fused", "below"),
    ("cells-32767", "cells-32768", ("ovr",), ("dense-device",), "k_ovr_fused", "below"),
) for test in tests for fmt in fmts)


@pytest.mark.parametrize("lo,hi,test,fmt,kernel,side", EDGES, ids=lambda v: str(v))
def test_an_edge_is_an_edge(engine, lo, hi, test, fmt, kernel, side):
    below, above = kernels_of(engine, lo, test, fmt), kernels_of(engine, hi, test, fmt)
    with_it, without = (below, above) if side == "below" else (above, below)
    assert kernel in with_it and kernel not in without, f"{lo}: {sorted(below)}\n{hi}: {sorted(above)}"
    if kernel == "k_csr_counts":   # ... and it is that pass which fills the planes, not a launch that returns on its verdict
        assert with_it <= CSR_COUNTS_ROUTE, sorted(with_it)


# The cases whose planes must come from the count passes themselves, every gene of the call: the switches inside k_csc_counts and
# k_csr_counts (slabs / 16-bit cells from CSCC_MAX_BIG = 8 big groups on, 16-bit cells + 64-bit sweep terms from a reference of 30000,
# the 15 of a 4-bit cell, a group of 255 / 256 / 257 cells beside larger ones, the largest group that fits) are template parameters and
# per-group widths of one kernel name: what is asserted is that the kernel ran and that no other route supplied a gene.
COUNT_PASSES = tuple((name, test, spec) for name, tests, specs in (
    ("big-8", ("ovo", "ovr"), ("csc-host/window",) + CSR_COUNTS),
    ("big-9", ("ovo", "ovr"), ("csc-host/window",) + CSR_COUNTS),
    ("big-16", ("ovo", "ovr"), ("csc-host/window",)),
    ("ref-29999", ("ovo", "ovr"), ("csc-host/window",)),
    ("ref-30000", ("ovo", "ovr"), ("csc-host/window",)),
    ("ranked-15", ("ovo", "ovr"), ("csc-host/window",) + CSR_COUNTS),
    ("ranked-256", ("ovo", "ovr"), ("csc-host/window",) + CSR_COUNTS),
    ("ranked-257", ("ovo", "ovr"), ("csc-host/window",) + CSR_COUNTS),
    ("ranked-65535", ("ovo", "ovr"), ("csc-host/window",) + CSR_COUNTS),
    ("forties-128", ("ovo", "ovr"), ("csc-host/window",) + CSR_COUNTS),
) for test in tests for spec in specs)


@pytest.mark.parametrize("name,test,spec", COUNT_PASSES, ids=lambda v: str(v))
def test_the_count_passes_fill_the_planes(engine, name, test, spec):
    seen = kernels_of(engine, name, test, spec)
    kernel, route = ("k_csc_counts", CSC_COUNTS_ROUTE) if spec.startswith("csc") else ("k_csr_counts", CSR_COUNTS_ROUTE)
    assert kernel in seen and seen <= route, sorted(seen)
