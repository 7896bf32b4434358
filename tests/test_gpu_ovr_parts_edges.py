"""Every switch point of dense OVR's value-range parts route, one key (one cell, one group) below and at / above it
(tests/ovr_parts_cases.py; the numbers per key width and the kernels seen per side: DESIGN.md section 12b).

Each case goes through Engine.run_dense as a host array and as a device tensor in the three layouts the partition can read (packed rows,
padded rows, plain group-contiguous rows), over all genes and over genes 1-11, with and without the z-score plane: U exact, p and fold
change at rtol 1e-12 against the CPU oracle, z bit for bit against the float64 restatement.  test_an_edge_is_an_edge holds the restated
plan of the case module against the build: k_ovr_gene runs in a call exactly when the model says a gene leaves the route.  The fused
count pass is off in every pinned run (no_fused_path, as in test_ovr_dense_value_range_parts_route): the two-pass routes take every gene,
whatever a probe of its values says; one run per case keeps the engine's defaults."""
import numpy as np
import pytest

import oracle
import ovr_parts_cases as oc
import threshold_cases as tc
from conftest import assert_planes_match
from route_trace import trace

pytestmark = pytest.mark.gpu

BASE = {"no_fused_path": 1}
WINDOW = (1, oc.N_GENES)
# the options that name the other side of a switch inside the route: one wavefront per block, one workgroup of 1024 threads per CU with the
# whole LDS (K doubles: a part beyond the key slots of the default is ranked in LDS), the sorted form for every part, padded rows when a
# group exceeds 65535 cells (none does here: the same launches)
OTHER_FORMS = ("no_ovr_part_coop", "ovr_rank_whole", "csc_ovr_sorted_form", "no_ovr_packed_big")
PARTITION, RANK, GENERAL = "k_ovr_partition", "k_ovr_rank_parts", "k_ovr_gene"


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


_cache = {}


def _case(name):   # the sides of an edge at a time: their tests are neighbours in the run
    import torch
    if name not in _cache:
        if len(_cache) >= 3:
            _cache.clear()
        c = oc.make(name)
        g = oc.groups(c.labels)
        _cache[name] = (c, g, oracle.run(c.X, g), torch.from_numpy(c.X).cuda())
    return _cache[name]


class options:
    def __init__(self, engine, *sets):
        self.engine, self.opts = engine, {k: v for s in sets for k, v in s.items()}

    def __enter__(self):
        for k, v in self.opts.items():
            self.engine.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.engine.set_option(k, 0)


def _run(engine, X, window=None, **kw):
    lb, ub = window or (0, oc.N_GENES)
    got = engine.run_dense(X, lb, ub, **kw)
    return tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in got)


def _check(got, want, g, X, what, window=None):
    if window:
        want, X = tuple(w[:, window[0]:window[1]] for w in want), X[:, window[0]:window[1]]
    assert_planes_match(got[:3], want, what=what)
    if len(got) == 4:
        z, zw = got[3], tc.z_want_fast(X, g, got[1])
        bad = np.argwhere(tc.bits(z) != tc.bits(zw))
        assert bad.size == 0, f"z {what}: {bad.shape[0]} entries differ, first (group, gene) {tuple(bad[0])}: {z[tuple(bad[0])]!r} != {zw[tuple(bad[0])]!r}"


@pytest.mark.parametrize("name", oc.NAMES)
def test_every_layout_matches_the_oracle(engine, name):
    c, g, want, Xd = _case(name)
    engine.set_groups(g)
    for layout in oc.LAYOUTS:
        with options(engine, BASE, c.opts, oc.LAYOUT_OPTS[layout]):
            _check(_run(engine, c.X), want, g, c.X, f"{name} {layout} host")
            _check(_run(engine, Xd, scores=layout == "packed"), want, g, c.X, f"{name} {layout} device")
            _check(_run(engine, c.X, WINDOW, scores=layout != "packed"), want, g, c.X, f"{name} {layout} host genes 1-11", WINDOW)
            _check(_run(engine, Xd, WINDOW), want, g, c.X, f"{name} {layout} device genes 1-11", WINDOW)
    with options(engine, c.opts):   # the engine's defaults: the fused pass first, what it leaves gathered for the two-pass routes
        _check(_run(engine, Xd, scores=True), want, g, c.X, f"{name} defaults device")


def launches_of(engine, name, layout, **more):
    """kernel family -> launches of one device-resident run of a case in one layout."""
    c, g, _, Xd = _case(name)
    case = {"labels": c.labels, "test": "ovr", "opts": dict(BASE, **c.opts, **oc.LAYOUT_OPTS[layout], **more), "X": Xd,
            "run": lambda e, X: e.run_dense(X, 0, oc.N_GENES)}
    return trace(engine, case)[0]


@pytest.mark.parametrize("edge,form", [(e, f) for e, spec in oc.EDGES.items() for f in spec.forms])
def test_an_edge_is_an_edge(engine, edge, form):
    """What the driver code says about a call (not a recording of a run):
     * run_ovr_dense_parts launches the partition and the rank kernel once per gene batch, or neither (the gate cap * 255 < N: the whole
       batch goes to run_ovr_dense_batch, k_ovr_gene);
     * a gene that the partition flags (no plan: more parts than ids) or the rank kernel flags (a part beyond the key slots that holds
       more than one value) is recomputed by run_ovr_dense_batch: k_ovr_gene and one more k_gene_totals, in the packed layout after one
       more k_group_compact (the flagged genes' padded rows) -- no other family;
     * every other switch is a branch inside one of the two kernels: the same launches on both sides.
    So k_ovr_gene in the profile of a call says exactly that some gene left, and the model (tests/ovr_parts_cases.py) says which."""
    spec = oc.EDGES[edge]
    seen = {layout: {} for layout in oc.LAYOUTS}
    for side in spec.sides:
        name = f"{edge}-{form}-{side}"
        c = _case(name)[0]
        route = oc.case_sizing(c).route
        assert route == (spec.expect.get(side) != "no-route"), name
        for layout in oc.LAYOUTS:
            got = seen[layout][side] = launches_of(engine, name, layout)
            what = f"{name} {layout}: {sorted(got.items())}"
            assert (got.get(PARTITION, 0), got.get(RANK, 0)) == ((1, 1) if route else (0, 0)), what
            assert (GENERAL in got) == oc.leaves(c, layout), what
            if spec.expect.get(side) is not None:
                assert (GENERAL in got) == (spec.expect[side] != "stays"), what
            assert ("k_group_compact" in got) == (layout != "plain") and ("k_transpose_permute" in got) == (layout == "plain"), what
    for layout in oc.LAYOUTS:
        first = seen[layout][spec.sides[0]]
        for side in spec.sides[1:]:
            other = seen[layout][side]
            what = f"{edge}-{form} {layout}\n{spec.sides[0]}: {sorted(first.items())}\n{side}: {sorted(other.items())}"
            left = GENERAL in other
            if edge == "D":
                assert set(other) >= (set(first) - {PARTITION, RANK, "k_value_sums"}) | {GENERAL}, what
            elif left and GENERAL not in first:
                assert set(other) == set(first) | {GENERAL} and other["k_gene_totals"] == first["k_gene_totals"] + 1, what
            elif spec.step == "key" and not left:
                assert other == first, what
            elif not left:
                assert set(other) == set(first), what
    if edge == "G":   # the same gene with every part in the sorted form: part 0 rounds up to exactly cap keys -- it stays
        got = launches_of(engine, f"G-{form}-lo", "packed", csc_ovr_sorted_form=1)
        assert GENERAL not in got and got[PARTITION] == got[RANK] == 1, sorted(got.items())
    if edge in ("F", "Fp") and form == "4":   # one workgroup per CU with the whole LDS: twice the key slots, K + 1 keys are ranked in LDS -- nothing leaves
        c = _case(f"{edge}-{form}-hi")[0]
        assert oc.case_sizing(c, whole=True).K >= 2 * oc.case_sizing(c).K and not any(not m.stays for m in oc.case_model(c, "packed", whole=True)[1])
        got = launches_of(engine, f"{edge}-{form}-hi", "packed", ovr_rank_whole=1)
        assert GENERAL not in got, sorted(got.items())


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_other_form_gives_the_same_bits(engine, name):
    """The p and U planes of a case are the same bytes in the three layouts and under the options that name the other side of a switch;
    so are the rank statistics before finalisation."""
    c, g, _, Xd = _case(name)
    engine.set_groups(g)
    with options(engine, BASE, c.opts):
        a = _run(engine, Xd, scores=True)
        sa = engine.rank_statistics(Xd, 0, oc.N_GENES)
    others = [(lay, oc.LAYOUT_OPTS[lay]) for lay in oc.LAYOUTS[1:]] + [(o, {o: 1}) for o in OTHER_FORMS]
    for what, opts in others:
        with options(engine, BASE, c.opts, opts):
            b = _run(engine, Xd, scores=True)
            sb = engine.rank_statistics(Xd, 0, oc.N_GENES)
        for k in (0, 1, 3):
            assert np.array_equal(tc.bits(a[k]), tc.bits(b[k])), f"{name} plane {k} with {what}"
        np.testing.assert_array_equal(sa[0], sb[0], err_msg=f"{name} two_u with {what}")
        np.testing.assert_array_equal(sa[1], sb[1], err_msg=f"{name} tie sums with {what}")
