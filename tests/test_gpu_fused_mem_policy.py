"""The cache policies of the fused dense OVO pass ("fused_mem_policy", include/illico_hip.h) change how bytes travel, never the bytes.

Every case runs the device-resident dense OVO call under each forced policy -- loads default (1) or non-temporal (2), plus stores
8 B (4), 16 B (8) or 16 B write-through (12) -- twice, into planes filled with a sentinel, and requires
  * every plane byte-identical to policy 5 (default loads, 8-byte stores: the code before the policies existed), run after run;
  * policy 5 itself equal to the CPU oracle at the dense tests' bar: statistic exact, p and fold change rtol 1e-12, reference row masked;
  * nothing written outside the planes (views into larger allocations keep their sentinel around them);
  * the first pass to be ONE launch of the form the planes allow: the engine's profile names the 16-byte forms "k_ovo_fused_st16", the
    8-byte form "k_ovo_fused"; 16 bytes need every plane's first column on a 16-byte boundary and an even row stride.
The 16-byte forms pair neighbouring lanes, so the cases are the places where a pair can break: an odd number of genes, windows and views
whose first column is 8 but not 16 bytes aligned or whose row stride is odd (the engine must take the 8-byte form), and columns that later
kernels on the stream write again (the 256-value second pass, the host's two-pass routes) after the write-through stores.
"""
import numpy as np
import pytest

import oracle
from conftest import assert_planes_match

pytestmark = pytest.mark.gpu

POLICIES = (5, 6, 9, 10, 13, 14)
N_CELLS, N_GROUPS, N_GENES = 3000, 24, 130
REF, SINGLE, EMPTY, BIG = 2, 3, 5, 9  # the reference is not the first code; a group of one cell, of none, and of 300 (16-bit cells)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import get_engine
    eng = get_engine()
    yield eng
    eng.profile(False)
    eng.set_option("fused_mem_policy", 0)


def _group_container(big):
    """24 groups over 3000 cells.  big = 300: no ranked group fits 8-bit multiplicities (the 16-bit-cell kernels, no 256-value second
    pass); big = 200: every ranked group does (the 8-bit-cell kernels and the second pass)."""
    rng = np.random.RandomState(17)
    fixed = {REF: 220, SINGLE: 1, EMPTY: 0, BIG: big}
    others = [k for k in range(N_GROUPS) if k not in fixed]
    codes = np.concatenate([np.full(n, k) for k, n in fixed.items()] +
                           [np.array(others)[rng.randint(0, len(others), size=N_CELLS - sum(fixed.values()))]]).astype(np.int64)
    rng.shuffle(codes)
    counts = np.bincount(codes, minlength=N_GROUPS).astype(np.int64)
    assert counts[EMPTY] == 0 and counts[SINGLE] == 1 and counts[BIG] == big and np.delete(counts, [REF, BIG]).max() <= 255
    return oracle.GroupContainer(codes, counts, np.argsort(codes, kind="stable").astype(np.int64),
                                 np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), REF)


def _counts_matrix():
    rng = np.random.RandomState(23)
    X = np.minimum(rng.poisson(rng.uniform(0.1, 15, size=N_GENES), size=(N_CELLS, N_GENES)), 63).astype(np.float32)
    X[rng.rand(N_CELLS, N_GENES) < 0.5] = 0
    return X


_CACHE = {}


def _shared(key, make):
    """One matrix, one container, one oracle result per key for the whole module; handed out read-only."""
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _groups(big):
    return _shared(("groups", big), lambda: _group_container(big))


def _matrix(kind="counts"):
    def make():
        X = _counts_matrix().copy()
        if kind == "rewritten":
            X[11, 7] = 100.0   # beyond the 64-value table: the 256-value second pass (or, with a 300-cell group, the host) rewrites column 7
            X[40, 70] = 0.5    # no count at all: the host's two-pass routes rewrite column 70
        return X
    return _shared(("matrix", kind), make)


def _oracle(kind, big, lb=0, ub=N_GENES):
    return _shared(("oracle", kind, big, lb, ub), lambda: tuple(oracle.run(_matrix(kind)[:, lb:ub].astype(np.float64), _groups(big))))


def _layout(kind, flat, W, lb):
    """The [G, W] plane inside a flat allocation.  full: columns [lb, lb + W) of a [G, N_GENES] plane; odd_ld: an odd row stride;
    base8: first element 8 but not 16 bytes aligned."""
    G = N_GROUPS
    if kind == "plain":
        return flat[:G * W].view(G, W)
    if kind == "full":
        return flat[:G * N_GENES].view(G, N_GENES)[:, lb:lb + W]
    if kind == "odd_ld":
        ld = W + 1 + (W & 1)
        return flat[:G * ld].view(G, ld)[:, :W]
    assert kind == "base8"
    return flat[1:1 + G * W].view(G, W)


def _check(engine, X, big, expect16, *, lb=0, ub=None, layout="plain", scores=False, kind="counts"):
    """expect16: the planes of this case allow the 16-byte store forms."""
    import torch
    ub = X.shape[1] if ub is None else ub
    W = ub - lb
    g = _groups(big)
    engine.set_groups(g)
    Xd = torch.from_numpy(np.array(X, order="C")).cuda()
    n_planes = 4 if scores else 3
    size = N_GROUPS * (N_GENES + 2) + 16
    covered = _layout(layout, torch.arange(size), W, lb).reshape(-1).numpy()
    outside = np.ones(size, dtype=bool)
    outside[covered] = False
    results = {}
    engine.profile(True)
    for pol in POLICIES:
        engine.set_option("fused_mem_policy", pol)
        for rep in range(2):
            flats = [torch.full((size,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(n_planes)]
            assert all(f.data_ptr() % 16 == 0 for f in flats)
            planes = tuple(_layout(layout, f, W, lb) for f in flats)
            if layout == "base8":
                assert all(p.data_ptr() % 16 == 8 for p in planes)
            engine.profile_reset()
            engine.run_dense(Xd, lb, ub, out=planes)
            engine.synchronize()
            assert expect16 == (planes[0].stride(0) % 2 == 0 and all(p.data_ptr() % 16 == 0 for p in planes)), "the case's own layout"
            wide = pol >= 8 and expect16
            prof = engine.profile_get()
            launched = {k: prof.get(k, {}).get("launches", 0) for k in ("k_ovo_fused", "k_ovo_fused_st16")}
            assert launched == {"k_ovo_fused": 0 if wide else 1, "k_ovo_fused_st16": 1 if wide else 0}, f"policy {pol}, {layout}: {launched}"
            got = [p.cpu().numpy().copy() for p in planes]
            for f in flats:
                assert np.all(f.cpu().numpy()[outside] == SENTINEL), f"policy {pol}: a store outside the plane"
            assert not any(np.any(a == SENTINEL) for a in got), f"policy {pol}: an element was never written"
            results.setdefault(pol, []).append(got)
    engine.profile(False)
    base = results[5][0]
    for pol in POLICIES:
        for rep, got in enumerate(results[pol]):
            for name, a, b in zip("p U fc z".split(), got, base):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"policy {pol} run {rep}: plane {name} differs from policy 5"
    assert_planes_match(tuple(base[:3]), _oracle(kind, big, lb, ub), ref_row=REF, what=f"policy 5, {layout} [{lb}, {ub})")
    return base


@pytest.mark.parametrize("big", [300, 200])
@pytest.mark.parametrize("layout", ["plain", "full"])
@pytest.mark.parametrize("genes", [130, 129])
def test_tile_tails_and_odd_widths(engine, genes, layout, big):
    """130 genes: a partial third tile, even; 129: the last lane has no partner and writes 8 bytes -- in the 16-byte forms when the
    planes are the first 129 columns of 130-column ones (full), in the 8-byte form when they are 129 columns wide (plain: odd stride)."""
    _check(engine, _matrix()[:, :genes], big, layout == "full" or genes % 2 == 0, ub=genes, layout=layout)


@pytest.mark.parametrize("lb,ub,layout,expect16", [(33, 129, "plain", True), (33, 129, "full", False), (32, 130, "full", True),
                                                   (32, 129, "full", True), (0, 130, "odd_ld", False), (0, 129, "odd_ld", False),
                                                   (0, 130, "base8", False), (0, 129, "base8", False)])
def test_column_windows_and_plane_strides(engine, lb, ub, layout, expect16):
    """Planes as views: of full-width planes at the window's columns (lb odd: first column 8 bytes off a 16-byte boundary), with an odd row
    stride, with a base that is 8 but not 16 bytes aligned -- the 16-byte policies must fall back to 8-byte stores there."""
    _check(engine, _matrix(), 300, expect16, lb=lb, ub=ub, layout=layout)


@pytest.mark.parametrize("big", [300, 200])
def test_columns_rewritten_by_later_kernels(engine, big):
    """A value of 100 sends its gene to the 256-value second pass (big = 200) or to the host's two-pass routes (big = 300), a fractional
    value always to the latter: both rewrite the gene's column on the same stream after the first pass's stores."""
    _check(engine, _matrix("rewritten"), big, True, kind="rewritten")


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_input_types(engine, dtype):
    _check(engine, _matrix().astype(dtype), 300, True)


@pytest.mark.parametrize("big", [300, 200])
@pytest.mark.parametrize("genes", [130, 129])
def test_with_score_plane(engine, genes, big):
    """Four planes: the odd lanes' second store carries z."""
    base = _check(engine, _matrix("rewritten")[:, :genes], big, True, ub=genes, scores=True, kind="rewritten", layout="full")
    assert np.all(base[3][REF] == 0.0)
