"""Every switch point the per-gene sparse kernels decide on the device, one stored entry below and at / above it (tests/gene_edge_cases.py;
the values per key width and the kernels seen per side: DESIGN.md section 12a).

Each case goes through the three sparse input forms of one Engine (the CSR forms reach the per-gene kernels through the device
transposition), over all genes and as a column window that starts after gene 0, with the count-valued routes on and off, with and without
the z-score plane: U exact, p and fold change at rtol 1e-12 against the CPU oracle, z bit for bit against the float64 restatement.
test_an_edge_is_an_edge holds the restated sizing functions of the case module against the build: the launches per kernel family differ
between the two sides as the driver code says, and an eight-byte case (float64 or int64) handed over as float32 takes the other side."""
import numpy as np
import pytest
from scipy import sparse

import gene_edge_cases as ge
import oracle
import threshold_cases as tc
from conftest import assert_planes_match

pytestmark = pytest.mark.gpu

INPUTS = ("csc-host", "csr-host", "csr-device")
WINDOW = (1, ge.N_GENES)
# the count-valued routes off: every gene reaches k_csc_gene / k_csc_ovr_gene (a sample of the stored values decides otherwise: the
# ordinary genes of a case hold fractions and negatives, but a sample is a sample)
COUNTS_OFF = {"no_csc_counts_path": 1, "no_csr_counts_path": 1, "no_dense_window_path": 1}
# ... for the group-size edges of the packed rank route: the sparse window is not written out dense either (their constant columns store
# every cell), the dense input skips the fused count pass
SPARSE_SECOND = dict(COUNTS_OFF, no_csr_densify_any=1)
DENSE_SECOND = {"no_fused_path": 1}
RUN_OPTIONS = ("no_big_runs_global", "no_coop_runs", "no_big_runs_wide")
# the edges whose value halves with eight-byte keys and whose new side shows in the profile
BY_WIDTH = ("ovr-leave", "ovr-sorted14", "ovr-sorted13", "crowd-bucket-cap", "crowd-avg-cap", "ovo-total", "ovo-quarter", "long-ovr")


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


_cache = {}


def _case(name):   # the two sides of an edge at a time: their tests are neighbours in the run
    if name not in _cache:
        if len(_cache) >= 2:
            _cache.clear()
        c = ge.make(name)
        g = ge.groups(c.labels, c.test)
        _cache[name] = (c, g, sparse.csc_matrix(c.X), sparse.csr_matrix(c.X), oracle.run(c.X, g))
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


def inputs_of(edge):
    return INPUTS + (("dense-device",) if ge.EDGES[edge].kind == "ranked" else ())


def second_line(edge, fmt):
    """The options under which an input of a case reaches the kernels its edge is about, whatever a sample of its values says."""
    spec = ge.EDGES[edge]
    if spec.kind == "ranked":
        return DENSE_SECOND if fmt == "dense-device" else SPARSE_SECOND
    return dict(COUNTS_OFF, **spec.pin)


def run_input(engine, fmt, C, R, window=None, **kw):
    import torch
    lb, ub = window or (0, C.shape[1])
    if fmt == "dense-device":
        X = np.ascontiguousarray(R.toarray())
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


@pytest.mark.parametrize("name", ge.NAMES)
def test_every_input_matches_the_oracle(engine, name):
    c, g, C, R, want = _case(name)
    engine.set_groups(g)
    spec = ge.EDGES[c.edge]
    for fmt in inputs_of(c.edge):
        with options(engine, spec.pin):
            _check(run_input(engine, fmt, C, R), want, g, c.X, f"{name} {fmt}")
            _check(run_input(engine, fmt, C, R, WINDOW, scores=True), want, g, c.X, f"{name} {fmt} genes 1-11 scores", WINDOW)
        with options(engine, second_line(c.edge, fmt)):
            _check(run_input(engine, fmt, C, R, scores=True), want, g, c.X, f"{name} {fmt} second line, scores")
            _check(run_input(engine, fmt, C, R, WINDOW), want, g, c.X, f"{name} {fmt} genes 1-11, second line", WINDOW)
        if spec.kind == "ranked" and fmt in ("csc-host", "dense-device"):   # the options that name the other side of a run-length switch
            for opt in RUN_OPTIONS:
                with options(engine, second_line(c.edge, fmt), {opt: 1}):
                    _check(run_input(engine, fmt, C, R, scores=True), want, g, c.X, f"{name} {fmt} {opt}")


def launches_of(engine, name, fmt, as_float32=False, window=None):
    """kernel family -> launches of one input of a case, the count-valued routes off."""
    c, g, C, R, _ = _case(name)
    if as_float32:
        C, R = C.astype(np.float32), R.astype(np.float32)
    engine.set_groups(g)
    with options(engine, second_line(c.edge, fmt)):
        engine.profile(True)
        try:
            engine.profile_reset()
            run_input(engine, fmt, C, R, window)
            return {k: v["launches"] for k, v in engine.profile_get().items()}
        finally:
            engine.profile(False)


@pytest.mark.parametrize("edge,form,fmt", [(e, w, f) for e in ge.EDGES for w in ge.FORMS for f in inputs_of(e)])
def test_an_edge_is_an_edge(engine, edge, form, fmt):
    """What the driver code says about the two sides (not a recording of a run):
     * a gene that leaves k_csc_ovr_gene is the only one of its call: the two-kernel route regroups it (k_sparse_seg), ranks it
       (k_ovr_gene) and forms its planes in a batch of its own -- one more k_value_sums, k_gene_totals and k_finalize;
     * a gene that leaves k_csc_gene is regrouped (k_sparse_seg) and ranked by k_ovo_rank (four-byte keys; eight-byte keys go to the
       packed rank kernel first: only the regrouping is asserted there);
     * run_csc_gene_route skips its launch when fewer than a quarter of the genes fit the key slots;
     * a window whose columns hold more than long_column stored entries on average is written out dense (k_densify) and ranked by the
       dense routes; below, the per-gene kernels take it (OVR) or the regrouped runs go to the packed rank kernel (OVO, groups of
       thousands of cells);
     * the packed rank route deals every run above 256 keys under k_group_compact, whatever its length, and ranks under
       k_ovo_rank_compact;
     * every other switch is a template parameter, an LDS size or a branch inside one kernel: equal families on both sides."""
    spec = ge.EDGES[edge]
    lo, hi = (launches_of(engine, f"{edge}-{form}-{side}", fmt) for side in ge.SIDES)
    what = f"lo: {sorted(lo.items())}\nhi: {sorted(hi.items())}"
    kind = fmt[:3]
    if spec.kind == "ranked":   # (two draws of a case: the families, not the launches)
        assert set(lo) == set(hi) and {"k_group_compact", "k_ovo_rank_compact"} <= set(lo), what
    elif spec.kind == "window":
        assert "k_densify" in hi and "k_densify" not in lo, what
        if spec.test == "ovr":
            assert "k_csc_ovr_gene" in lo, what
        # a window without the boundary gene: CSC asks the window (5 x L entries), CSR the whole matrix
        part = launches_of(engine, f"{edge}-{form}-hi", fmt, window=(0, ge.B))
        assert ("k_densify" in part) == (kind == "csr"), f"genes 0-4 of hi: {sorted(part.items())}"
    elif edge == "ovo-quarter":
        assert "k_csc_gene" in lo and set(hi) == set(lo) - {"k_csc_gene"}, what
    elif spec.appear is None:
        assert lo == hi, what
        if edge.startswith("regroup"):   # the two-kernel route forced: both regroup kernels are timed under k_sparse_seg
            assert "k_sparse_seg" in lo and "k_csc_gene" not in lo and "k_csc_ovr_gene" not in lo, what
        else:
            assert ("k_csc_ovr_gene" if spec.test == "ovr" else "k_csc_gene") in lo, what
    else:
        appear = spec.appear[kind]
        if form != "4":
            appear = tuple(k for k in appear if k != "k_ovo_rank")
        for k in appear:
            assert k in hi and k not in lo, what
        if spec.test == "ovr":
            assert lo["k_csc_ovr_gene"] == hi["k_csc_ovr_gene"] == 1, what
            for k in ("k_finalize", "k_gene_totals", "k_value_sums"):
                assert hi[k] == lo[k] + 1, what
        else:
            assert lo["k_csc_gene"] == hi["k_csc_gene"] == 1 and (kind == "csr" or "k_sparse_seg" not in lo), what
    if form != "4" and edge in BY_WIDTH:   # the same numbers with four-byte keys: twice the key slots, the old side
        narrow = launches_of(engine, f"{edge}-{form}-hi", fmt, as_float32=True)
        # (ovo-quarter: there every gene of the call fits, and none is left for the routes that the long genes of lo take)
        assert "k_csc_gene" in narrow if edge == "ovo-quarter" else set(narrow) == set(lo), f"{what}\nhi as float32: {sorted(narrow.items())}"


BIT_EQUAL = tuple((e, w, s) for e, spec in ge.EDGES.items() if spec.bit_equal for w in ge.FORMS for s in ge.SIDES)


@pytest.mark.parametrize("edge,form,side", BIT_EQUAL)
def test_the_other_form_gives_the_same_bits(engine, edge, form, side):
    """The option that names the other side of a switch (the sorted form for every gene, the full-size LDS layout, the sorted reference
    run) against the default, plane for plane."""
    spec = ge.EDGES[edge]
    c, g, C, R, _ = _case(f"{edge}-{form}-{side}")
    engine.set_groups(g)
    for fmt in ("csc-host", "csr-device") + inputs_of(edge)[3:]:
        with options(engine, second_line(edge, fmt)):
            a = run_input(engine, fmt, C, R, scores=True)
        with options(engine, second_line(edge, fmt), {spec.bit_equal: 1}):
            b = run_input(engine, fmt, C, R, scores=True)
        rows = np.arange(g.counts.size) != g.encoded_ref_group   # (the reference's own row is left unspecified)
        for k, (x, y) in enumerate(zip(a, b)):
            x, y = x[rows], y[rows]
            assert np.array_equal(tc.bits(x), tc.bits(y)), f"{edge}-{form}-{side} {fmt} plane {k} with {spec.bit_equal}"
