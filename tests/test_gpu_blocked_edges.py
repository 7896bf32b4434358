"""The blocked Wilcoxon routes where tests/test_gpu_blocked.py is blind: a reference that is not group 0 (so that ``ref * B + b`` is not
``b``, and the reference's row among a block's groups is not its id), all 256 bins of the value walk, tests of 2 097 151 cells (the
largest the integer sums are built for), several windows and every option of the plane feeder, a ``row_map`` entry of -1 over cells
that exist, and a pitched ``sums`` plane against the rest.

Tolerances are those of tests/test_gpu_blocked.py: the statistic equal; z, p, fold change and auc at rtol 1e-12, atol 0, against the
float64 model of tests/blocked_model.py; bytes where two device routes must agree.  tests/test_blocked_edges_host.py holds the builders
to what these cases need (no p below 1e-300, the sizes at the limit, the bins occupied)."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from illico_amd import AnnDataLite, _lib, blocked_wilcoxon, differential_expression
from illico_amd import blocked as blocked_mod
from illico_amd.blocked import compound_groups
from blocked_model import (ALTERNATIVES, LIMIT_CELLS, blocked_model, block_stats, combine, combine_planes, edge_case, limit_case,
                           make_case, stats_from_hists, z_block)
from test_gpu_blocked import COLUMNS, SENTINEL, _adata, _assert_model, _block_planes, _container_input, _planes

pytestmark = pytest.mark.gpu

CONTAINERS = ["dense-host", "dense-device", "csc", "csr"]
QUARTER = np.float32(0.25)


@functools.lru_cache(maxsize=None)
def _case(G, B, W, values="small"):
    return make_case(G, B, W, values=values)


@functools.lru_cache(maxsize=None)
def _stats(G, B, W, ref, values="small"):
    c = _case(G, B, W, values)
    return block_stats(c.X, c.g_codes, c.b_codes, G, B, ref)


def _name(ref):
    return None if ref is None else f"grp{ref:03d}"


def _compound_sums(case):
    """float64 [G * B, W]: the value sums of the compounds (exact: small integers)."""
    k = case.g_codes * case.B + case.b_codes
    return np.stack([case.X[k == c].astype(np.float64).sum(axis=0) for c in range(case.G * case.B)])


def _side(x, side):
    """A host array as it is, or its copy on the device (uint32 words as int32: the engine takes any 32-bit integer tensor)."""
    if side == "host":
        return x
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


# ---- 1. a reference that is not group 0 ----
G_REF = [(G, ref) for G in (3, 5, 9) for ref in (G // 2, G - 1)]


@pytest.mark.parametrize("W", [63, 65])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("G,ref", G_REF)
def test_a_reference_other_than_group_zero(G, ref, B, W):
    """Both feeders of blocked_wilcoxon against the model; the plane feeder (the float32 copy + 0.25: the same ranks) gives the count
    feeder's statistic, z, p and n_blocks exactly."""
    case = _case(G, B, W)
    st = _stats(G, B, W, ref)
    adata, shifted = _adata(case.X, case), _adata(case.X + QUARTER, case)
    for alternative in ALTERNATIVES:
        for tie_correct in (True, False):
            what = f"ref={ref} {alternative} tie={tie_correct}"
            got = blocked_wilcoxon(adata, False, "g", "b", _name(ref), alternative=alternative, tie_correct=tie_correct)
            assert got.attrs["n_flagged_genes"] == 0
            planes = _planes(got, G)
            _assert_model(planes, combine(st, ref, alternative, tie_correct), what)
            got = blocked_wilcoxon(shifted, False, "g", "b", _name(ref), alternative=alternative, tie_correct=tie_correct)
            assert got.attrs["n_flagged_genes"] == W
            plane_fed = _planes(got, G)
            for c in ("p_value", "statistic", "z_score", "n_blocks"):
                np.testing.assert_array_equal(plane_fed[c], planes[c], err_msg=f"{c} {what}")


@pytest.mark.parametrize("W", [63, 65])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("G,ref", G_REF)
def test_the_two_feeders_agree_on_another_reference(G, ref, B, W):
    """Engine.blocked_from_planes on the planes of per-block engine calls and Engine.blocked_from_hists, with one sums plane: byte for
    byte in all four planes."""
    case = _case(G, B, W)
    eng = _lib.get_engine()
    comp = compound_groups(case.g_codes, case.b_codes, G, B)
    counts = np.asarray(comp.counts)
    Xd = torch.from_numpy(case.X).cuda()
    for tie_correct in (True, False):
        zs, us, row_map = _block_planes(eng, case.X, case, ref, tie_correct)
        eng.set_groups(comp)
        H, fl = eng.group_value_hists(Xd, 0, W)
        assert int(fl.sum()) == 0
        sums = eng.group_stats(Xd, 0, W)[1]
        for alternative in ALTERNATIVES:
            a = eng.blocked_from_hists(H, fl, counts=counts, n_blocks=B, ref=ref, sums=sums, tie_correct=tie_correct, alternative=alternative)
            b = eng.blocked_from_planes(zs, us, row_map, counts=counts, ref=ref, sums=sums, alternative=alternative)
            for name, x, y in zip(COLUMNS, a, b):
                assert _host(x).tobytes() == _host(y).tobytes(), (name, ref, tie_correct, alternative)
            if tie_correct:
                want = combine(_stats(G, B, W, ref), ref, alternative, True)
                np.testing.assert_array_equal(_host(a[1]), want.statistic)
                np.testing.assert_allclose(_host(a[3]), want.z, rtol=1e-12, atol=0)
                np.testing.assert_allclose(_host(a[2]), want.fold, rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind", ["dense-host", "csc"])
@pytest.mark.parametrize("values", ["counts", "plus-quarter"])
def test_one_block_is_the_unblocked_call_with_reference_one(values, kind):
    case = _case(3, 2, 65)
    X = case.X if values == "counts" else case.X + QUARTER
    adata = _adata(_container_input(X, kind), case, B=1)
    got = blocked_wilcoxon(adata, False, "g", "b", "grp001")
    want = differential_expression(adata, False, "g", "grp001", scores=True, use_continuity=False)
    assert got.attrs["n_flagged_genes"] == (0 if values == "counts" else 65) and got.index.equals(want.index)
    assert got["statistic"].to_numpy().tobytes() == want["statistic"].to_numpy().tobytes()
    assert got["z_score"].to_numpy().tobytes() == want["z_score"].to_numpy().tobytes()
    np.testing.assert_allclose(got["p_value"].to_numpy(), want["p_value"].to_numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["fold_change"].to_numpy(), want["fold_change"].to_numpy(), rtol=1e-12, atol=0)
    stat = got["statistic"].to_numpy().reshape(3, 65)
    assert (stat[1] == -1).all() and (stat[[0, 2]] >= 0).all()


# ---- 2. blocks that do not count, with a rotated reference ----
@pytest.mark.parametrize("mode", ["reference", "rest"])
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("kind", ["group-absent", "reference-absent", "no-shared-block", "one-against-one", "constant-block", "constant-gene",
                                  "below-reference-absent"])
def test_blocks_that_do_not_count_with_a_rotated_reference(kind, r, mode):
    case = edge_case(kind, ref=r)
    ref = r if mode == "reference" else None
    for X in (case.X, case.X + QUARTER):  # the count feeder, the plane feeder
        want = blocked_model(X, *case[1:], ref=ref)
        got = blocked_wilcoxon(_adata(X, case), False, "g", "b", _name(ref))
        assert got.attrs["n_flagged_genes"] == (0 if X is case.X else X.shape[1])
        planes = _planes(got, case.G)
        _assert_model(planes, want, f"{kind} ref={ref}")
        dead = want.n_blocks == 0
        assert list(np.flatnonzero(dead)) == ([(3 + r) % 4] if kind == "no-shared-block" and ref is not None else [])
        for c in COLUMNS + ("p_value_adj", "auc"):
            assert np.isnan(planes[c][dead]).all() and not np.isnan(planes[c][~dead]).any(), c


# ---- 3. the whole value range ----
@pytest.mark.parametrize("kind", CONTAINERS)
@pytest.mark.parametrize("G,B,W", [(3, 2, 65), (5, 3, 129)])
def test_the_whole_value_range(G, B, W, kind):
    case = _case(G, B, W, "full-range")
    adata = _adata(_container_input(case.X, kind), case)
    for ref in (None, 0, G - 1):
        got = blocked_wilcoxon(adata, False, "g", "b", _name(ref))
        assert got.attrs["n_flagged_genes"] == 0
        _assert_model(_planes(got, G), combine(_stats(G, B, W, ref, "full-range"), ref), f"ref={ref} {kind}")


# ---- 4. the count limit ----
@functools.lru_cache(maxsize=None)
def _limit(mode):
    H, flags, counts, ref = limit_case(mode)
    return H, flags, counts, ref, stats_from_hists(H[:, :3], counts, ref)


@pytest.mark.parametrize("side", ["host", "device"])
@pytest.mark.parametrize("mode", ["reference", "rest"])
def test_tests_of_2097151_cells(mode, side):
    """The largest test the entry points accept, from synthetic histograms: against the model in Python integers.  Gene 3 is flagged
    and the planes are 5 columns wider than the call: both keep the caller's bytes."""
    H, flags, counts, ref, st = _limit(mode)
    G, B, W = 3, 2, 4
    assert int((st.n_g + st.n_r).max()) == LIMIT_CELLS
    eng = _lib.get_engine()
    Hs, fs = _side(H, side), _side(flags, side)
    rows = np.arange(G) != (-1 if ref is None else ref)
    for tie_correct in (True, False):
        zb = np.array([[[z_block(int(st.n_g[g, b]), int(st.n_r[g, b]), st.tie[g, b, j] if tie_correct else 0.0, st.U[g, b, j])
                         for j in range(3)] for g in range(G)] for b in range(B)])
        ub = np.ascontiguousarray(st.U.transpose(1, 0, 2))
        for alternative in ALTERNATIVES:
            what = f"{mode} {side} tie={tie_correct} {alternative}"
            want = combine(st, ref, alternative, tie_correct)
            wide = [_side(np.full((G, W + 5), SENTINEL), side) for _ in range(4)]
            eng.blocked_from_hists(Hs, fs, counts=counts, n_blocks=B, ref=ref, tie_correct=tie_correct, alternative=alternative,
                                   out=[q[:, :W] for q in wide])
            p, stat, fold, z = (_host(q) for q in wide)
            for q in (p, stat, fold, z):
                assert (q[:, 3:] == SENTINEL).all(), what
            np.testing.assert_array_equal(stat[:, :3], want.statistic, err_msg=what)
            np.testing.assert_allclose(z[:, :3], want.z, rtol=1e-12, atol=0, err_msg=what)
            np.testing.assert_allclose(p[:, :3], want.p, rtol=1e-12, atol=0, err_msg=what)
            np.testing.assert_allclose(fold[:, :3], want.fold, rtol=1e-12, atol=0, err_msg=what)
            if tie_correct:  # all cells of a block in one bin: the tie sum is n^3 - n itself, and z is 0, not small
                assert (z[:, 0] == 0).all() and (p[rows, 0] == (1.0 if alternative == "two-sided" else 0.5)).all(), what
            # the plane entry takes the same sizes, and from the model's per-block z and U gives the same bytes
            got = eng.blocked_from_planes(_side(zb, side), _side(ub, side), np.tile(np.arange(G, dtype=np.int32), (B, 1)), counts=counts,
                                          ref=ref, alternative=alternative)
            assert got[2] is None
            for name, x, y in (("p", got[0], p), ("statistic", got[1], stat), ("z", got[3], z)):
                assert _host(x).tobytes() == np.ascontiguousarray(y[:, :3]).tobytes(), (name, what)


@pytest.mark.parametrize("mode", ["reference", "rest"])
def test_one_cell_beyond_the_limit_is_refused(mode):
    H, flags, counts, ref, _ = _limit(mode)
    G, B, W = 3, 2, 4
    eng = _lib.get_engine()
    more = counts.copy()
    more[0, 0] += 1
    out = [np.full((G, W), SENTINEL) for _ in range(4)]
    rc = eng.lib.illico_blocked_from_hists(eng.h, H.ctypes.data, flags.ctypes.data, more.ctypes.data, G, B, W, -1 if ref is None else ref, None, 0,
                                           _lib.FLAG_TIE_CORRECT, 0, *[q.ctypes.data for q in out], W)
    assert rc == _lib.ERR_UNSUPPORTED and b"2097152 cells" in eng.lib.illico_last_error(eng.h)
    z = np.zeros((B * G, W))
    row_map = np.tile(np.arange(G, dtype=np.int32), (B, 1))
    rc = eng.lib.illico_blocked_from_planes(eng.h, z.ctypes.data, z.ctypes.data, W, row_map.ctypes.data, more.ctypes.data, G, B, W,
                                            -1 if ref is None else ref, None, 0, 0, 0, out[0].ctypes.data, out[1].ctypes.data, None, out[3].ctypes.data, W)
    assert rc == _lib.ERR_UNSUPPORTED
    assert all((q == SENTINEL).all() for q in out)


# ---- 5. the plane feeder's windows and options ----
FLAGGED_RUNS = list(range(60, 69)) + list(range(126, 132))


@functools.lru_cache(maxsize=None)
def _scattered_case():
    """200 full-range genes of which 70 are flagged: the runs 60 .. 68 and 126 .. 131 (across the 64-gene tile boundaries) and 55
    single columns below 126 -- so that the feeder's first window of 64 genes is scattered and its second is the run 126 .. 131."""
    case = make_case(3, 2, 200, values="full-range")
    X = case.X.copy()
    rng = np.random.RandomState(11)
    N = X.shape[0]
    free = np.setdiff1d(np.arange(126), FLAGGED_RUNS)
    flagged = np.sort(np.concatenate([FLAGGED_RUNS, rng.choice(free, 55, replace=False)]))
    for k, j in enumerate(flagged):
        if k % 4 == 0:
            X[:, j] = rng.randint(0, 4, N) + 0.5
        elif k % 4 == 1:
            X[:, j] = -1.0 * rng.randint(0, 3, N)
        elif k % 4 == 2:
            X[:, j] = 256.0 + rng.randint(0, 3, N)
        else:
            X[:, j] = rng.randn(N).astype(np.float32)
    return case._replace(X=X), flagged


@functools.lru_cache(maxsize=None)
def _scattered_stats(ref):
    case, _ = _scattered_case()
    return block_stats(case.X, case.g_codes, case.b_codes, case.G, case.B, ref)


@pytest.mark.parametrize("ref", [None, 1], ids=["rest", "reference"])
def test_two_windows_of_scattered_flagged_genes(ref, monkeypatch):
    case, flagged = _scattered_case()
    G, B = case.G, case.B
    assert flagged.size == 70 and list(flagged[64:]) == list(range(126, 132)) and set(FLAGGED_RUNS) <= set(flagged)
    adata = _adata(case.X, case)
    options = (("less", False), ("greater", False), ("two-sided", True))
    want = [blocked_wilcoxon(adata, False, "g", "b", _name(ref), alternative=alt, tie_correct=tie) for alt, tie in options]
    eng = _lib.get_engine()
    seen = []
    real = eng.blocked_from_planes
    monkeypatch.setattr(blocked_mod, "BLOCK_WINDOW_BYTES", 64 * (3 * G * B + 6 * G) * 8)
    monkeypatch.setattr(eng, "blocked_from_planes", lambda z, U, row_map, **kw: (seen.append(int(z.shape[2])), real(z, U, row_map, **kw))[1])
    for (alt, tie), unwindowed in zip(options, want):
        del seen[:]
        got = blocked_wilcoxon(adata, False, "g", "b", _name(ref), alternative=alt, tie_correct=tie)
        assert seen == [64, 6] and got.attrs["n_flagged_genes"] == 70 == unwindowed.attrs["n_flagged_genes"]
        pd.testing.assert_frame_equal(got, unwindowed, check_exact=True)
        _assert_model(_planes(got, G), combine(_scattered_stats(ref), ref, alt, tie), f"ref={ref} {alt} tie={tie}")


@functools.lru_cache(maxsize=None)
def _log_case(dtype):
    case = make_case(3, 3, 65, values="full-range")
    return case._replace(X=np.log1p(case.X.astype(np.float64)).astype(dtype))


@pytest.mark.parametrize("ref", [None, 2], ids=["rest", "reference"])
def test_a_log_normalised_matrix(ref):
    """Every gene flagged, is_log1p=True: the plane feeder's main use, in float64 against the model -- the fold change of expm1 sums at
    rtol 1e-12, the bound tests/test_gpu_group_stats.py holds such sums to -- on every container."""
    case = _log_case(np.float64)
    want = blocked_model(*case, ref=ref, is_log1p=True)
    for kind in CONTAINERS:
        got = blocked_wilcoxon(_adata(_container_input(case.X, kind), case), True, "g", "b", _name(ref))
        assert got.attrs["n_flagged_genes"] == 65 and got.attrs["n_plane_genes"] == 65
        _assert_model(_planes(got, case.G), want, f"ref={ref} {kind}")


@pytest.mark.parametrize("ref", [None, 2], ids=["rest", "reference"])
def test_a_log_normalised_matrix_in_float32(ref):
    """The same in float32: p, statistic and z against the model; the device takes expm1 in float32 and the model does not, so the fold
    change is held to be the same bytes on every container only."""
    case = _log_case(np.float32)
    want = blocked_model(*case, ref=ref, is_log1p=True)
    folds = []
    for kind in CONTAINERS:
        got = blocked_wilcoxon(_adata(_container_input(case.X, kind), case), True, "g", "b", _name(ref))
        assert got.attrs["n_flagged_genes"] == 65
        planes = _planes(got, case.G)
        np.testing.assert_array_equal(planes["statistic"], want.statistic, err_msg=kind)
        np.testing.assert_allclose(planes["z_score"], want.z, rtol=1e-12, atol=0, err_msg=kind)
        np.testing.assert_allclose(planes["p_value"], want.p, rtol=1e-12, atol=0, err_msg=kind)
        np.testing.assert_allclose(planes["auc"], want.auc, rtol=1e-12, atol=0, err_msg=kind)
        assert (planes["n_blocks"] == 3).all() and np.isfinite(planes["fold_change"]).all()
        folds.append(planes["fold_change"].tobytes())
    assert len(set(folds)) == 1


# ---- 6. row_map = -1 for a compound that has cells ----
@pytest.mark.parametrize("side", ["host", "device"])
@pytest.mark.parametrize("ref", [None, 1], ids=["rest", "reference"])
@pytest.mark.parametrize("B", [2, 3])
def test_a_row_map_entry_of_minus_one_skips_a_block_that_has_cells(B, ref, side):
    G, W = 3, 65
    case = _case(G, B, W)
    eng = _lib.get_engine()
    counts = np.asarray(compound_groups(case.g_codes, case.b_codes, G, B).counts)
    zs, us, row_map = _block_planes(eng, case.X, case, ref, True)
    st = _stats(G, B, W, ref)
    g, b = 2, 1  # a test group's compound, with cells
    assert counts.reshape(G, B)[g, b] > 0 and row_map[b, g] >= 0
    row_map[b, g] = -1
    zin, uin = (zs, us) if side == "device" else (zs.cpu().numpy(), us.cpu().numpy())
    for alternative in ALTERNATIVES:
        p, stat, fold, z = (_host(q) for q in eng.blocked_from_planes(zin, uin, row_map, counts=counts, ref=ref, sums=_side(_compound_sums(case), side),
                                                                      alternative=alternative))
        wp, wstat, wz = combine_planes(_host(zs), _host(us), row_map, counts.reshape(G, B), ref, alternative)
        np.testing.assert_array_equal(stat, wstat)
        np.testing.assert_allclose(z, wz, rtol=1e-12, atol=0)
        np.testing.assert_allclose(p, wp, rtol=1e-12, atol=0)
        # ... which is the model without that block for that row: n_blocks one less, the fold change pooled over the others
        used = st.used.copy()
        used[g, b] = False
        want = combine(st._replace(used=used), ref, alternative)
        assert list(want.n_blocks) == [B if k != g else B - 1 for k in range(G)]
        np.testing.assert_array_equal(stat, want.statistic)
        np.testing.assert_allclose(z, want.z, rtol=1e-12, atol=0)
        np.testing.assert_allclose(p, want.p, rtol=1e-12, atol=0)
        np.testing.assert_allclose(fold, want.fold, rtol=1e-12, atol=0)
        assert not (stat[g] == combine(st, ref, alternative).statistic[g]).all()
        if B == 2:  # one block left: its z as it stands in the plane
            assert z[g].tobytes() == _host(zs)[0, row_map[0, g]].tobytes()


# ---- 7. a pitched sums plane ----
@pytest.mark.parametrize("side", ["host", "device"])
@pytest.mark.parametrize("ref", [None, 2], ids=["rest", "reference"])
def test_a_pitched_sums_plane(ref, side):
    """sums_ld = W + 3 into both entry points, the padding NaN: against the rest the block totals are formed from the pitched plane."""
    G, B, W = 3, 3, 65
    case = _case(G, B, W)
    eng = _lib.get_engine()
    comp = compound_groups(case.g_codes, case.b_codes, G, B)
    counts = np.asarray(comp.counts)
    wide = np.full((G * B, W + 3), np.nan)
    wide[:, :W] = _compound_sums(case) * 2.0  # (not the sums of the histograms: the plane is what is read)
    sums = _side(wide, side)[:, :W]
    want = combine(_stats(G, B, W, ref), ref)
    want_fold = want.fold  # both pooled sums are doubled: the ratio is the same number
    zs, us, row_map = _block_planes(eng, case.X, case, ref, True)
    eng.set_groups(comp)
    H, fl = eng.group_value_hists(_side(case.X, side), 0, W)
    a = eng.blocked_from_hists(H, fl, counts=counts, n_blocks=B, ref=ref, sums=sums)
    zin, uin = (zs, us) if side == "device" else (zs.cpu().numpy(), us.cpu().numpy())
    b = eng.blocked_from_planes(zin, uin, row_map, counts=counts, ref=ref, sums=sums)
    for got in (a, b):
        p, stat, fold, z = (_host(q) for q in got)
        assert not np.isnan(fold).any()
        np.testing.assert_allclose(fold, want_fold, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(stat, want.statistic)
        np.testing.assert_allclose(z, want.z, rtol=1e-12, atol=0)
        np.testing.assert_allclose(p, want.p, rtol=1e-12, atol=0)
    assert np.isnan(wide[:, W:]).all()
