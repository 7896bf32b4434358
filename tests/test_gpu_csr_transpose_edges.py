"""The CSR -> CSC device transposition at every switch of its plan (tests/csr_transpose_cases.py: the plan restated, and the cases).

Per case, OVO and OVR: the planes against the CPU oracle at the suite's tolerances, and the launches of k_csr_tile_gather and
k_csr_block_scatter under the profiler against the restated plan, exactly -- in three forms of the same call: as pinned, with one
workgroup per row block ("no_csr_transpose_split": the ny = 1 store path of the counting pass, one stretch in the gather form) and with
the scatter form for every window ("no_csr_tile_gather").  The three forms give the same U, p and fold change bit for bit: the
transposition only moves entries, the rank kernels do not depend on the order inside a column, and the value sums are exact whatever
order the regroup leaves (sparse_driver.h, above launch_seg_value_sums).  Compact cases also run from host arrays; every case runs once
with the engine's default options (and the module's scratch budget, not the case's), against the oracle only.

Pinned: "no_csr_counts_path", "no_dense_window_path" and "no_csr_densify_any", so that every case reaches the transposition whatever
its density.  The module has an engine of its own: "scratch_bytes" has no "0 = default", and a shared engine must not keep a changed
value."""
import numpy as np
import pytest

import csr_transpose_cases as cc
import oracle
from conftest import assert_planes_match
from threshold_cases import bits

pytestmark = pytest.mark.gpu

BASE = {"no_csr_counts_path": 1, "no_dense_window_path": 1, "no_csr_densify_any": 1}
FORMS = (("pinned", {}, {}), ("one workgroup per row block", {"no_csr_transpose_split": 1}, {"no_split": True}),
         ("scatter form", {"no_csr_tile_gather": 1}, {"no_gather": True}))
GATHER, SCATTER = "k_csr_tile_gather", "k_csr_block_scatter"


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import Engine
    e = Engine(0)
    e.set_option("scratch_bytes", cc.DEFAULT_SCRATCH)
    yield e
    e.close()


class options:
    """Flags for the time of a block; "scratch_bytes" goes back to the module's value, not to 0."""

    def __init__(self, engine, *sets, scratch_bytes=None):
        self.engine, self.opts, self.scratch = engine, {k: v for s in sets for k, v in s.items()}, scratch_bytes

    def __enter__(self):
        for k, v in self.opts.items():
            self.engine.set_option(k, v)
        if self.scratch is not None:
            self.engine.set_option("scratch_bytes", self.scratch)

    def __exit__(self, *exc):
        for k in self.opts:
            self.engine.set_option(k, 0)
        self.engine.set_option("scratch_bytes", cc.DEFAULT_SCRATCH)


_cache = {}


def _case(name, test):
    """(case, groups, what the oracle says, the three arrays on the device); the oracle's planes are computed once and not written to."""
    import torch
    key = (name, test)
    if key not in _cache:
        if len(_cache) >= 4:
            _cache.clear()
        c = cc.make(name)
        g = cc.groups(c.labels, test)
        want = oracle.run(cc.as_csc(c), g, col_lb=c.window[0], col_ub=c.window[1])
        for w in want:
            w.setflags(write=False)
        dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c.data, c.indices, c.indptr))
        _cache[key] = (c, g, want, dev)
    return _cache[key]


def _profiled(engine, run):
    """(planes on the host, launches per kernel family) of one call."""
    engine.profile(True)
    engine.profile_reset()
    try:
        got = run()
        prof = engine.profile_get()
    finally:
        engine.profile(False)
    return tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in got), {k: v["launches"] for k, v in prof.items()}


def _pass2(launches):
    return launches.get(GATHER, 0), launches.get(SCATTER, 0)


@pytest.mark.parametrize("test", ["ovo", "ovr"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_every_form_matches_the_oracle_and_the_plan(engine, name, test):
    c, g, want, dev = _case(name, test)
    ref_row = g.encoded_ref_group if test == "ovo" else None
    engine.set_groups(g)
    run_dev = lambda: engine.run_sparse("csr", *dev, c.shape, *c.window)
    run_host = lambda: engine.run_sparse("csr", c.data, c.indices, c.indptr, c.shape, *c.window)
    planes = {}
    for form, opts, model in FORMS:
        p = cc.case_plan(c, **model)
        inputs = (("device", run_dev), ("host", run_host)) if c.compact else (("device", run_dev),)
        for where, run in inputs:
            what = f"{name} {test} {form} {where}"
            with options(engine, BASE, opts, scratch_bytes=c.scratch_bytes):
                got, launches = _profiled(engine, run)
            print(what, sorted(launches.items()), p)
            assert _pass2(launches) == (p.gathers, p.scatters), f"{what}: {sorted(launches.items())}, the plan: {p}"
            assert_planes_match(got, want, ref_row=ref_row, what=what)
            planes.setdefault(form, got)
    # the same bits whatever form transposed the window (the reference group's own row is left unspecified)
    rows = np.arange(g.counts.size) != (g.encoded_ref_group if test == "ovo" else -1)
    first = planes[FORMS[0][0]]
    for form, _, _ in FORMS[1:]:
        for k, plane in enumerate(("p", "U", "fold change")):
            a, b = bits(first[k][rows]), bits(planes[form][k][rows])
            bad = np.argwhere(a != b)
            assert bad.size == 0, f"{name} {test} {plane}: {form} differs from the pinned form in {bad.shape[0]} entries, first {tuple(bad[0])}"
    # the engine's defaults: whatever route they take must be right
    got = tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in run_dev())
    assert_planes_match(got, want, ref_row=ref_row, what=f"{name} {test} defaults")


@pytest.mark.parametrize("test", ["ovo", "ovr"])
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", cc.BOUND)
def test_a_bound_matrix_keeps_its_row_order_verdict(engine, name, where, test):
    """bind_sparse looks at the rows' order once; a call on the bound matrix takes the gather form when they were in order and the
    scatter form when they were not (route_csr_transpose asks again only then)."""
    c, g, want, dev = _case(name, test)
    p = cc.case_plan(c)
    assert (p.gathers, p.scatters) == ((1, 0) if name == "sorted-last-row" else (0, 1))
    engine.set_groups(g)
    with options(engine, BASE):
        m = engine.bind_sparse("csr", *(dev if where == "device" else (c.data, c.indices, c.indptr)), c.shape)
        try:
            got, launches = _profiled(engine, lambda: m.run(*c.window))
        finally:
            m.release()
    assert _pass2(launches) == (p.gathers, p.scatters), sorted(launches.items())
    assert_planes_match(got, want, ref_row=g.encoded_ref_group if test == "ovo" else None, what=f"{name} {test} bound {where}")
