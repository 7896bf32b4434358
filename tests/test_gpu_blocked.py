"""Blocked Wilcoxon tests on the device -- blocked_wilcoxon, Engine.blocked_from_hists / blocked_from_planes and the two C entry points
(include/illico_hip_blocked.h) -- against the numpy model of tests/blocked_model.py and, with one block, against the unblocked call.

Tolerances: the statistic is a sum of half-integers (exact); z, p and the fold change are float64 formulas restated operation by
operation, the model's erfc being scipy's: rtol 1e-12, the project's bound for such planes.  No p of these inputs is below 1e-300
(tests/test_blocked_host.py holds the builders to that), so no case is skipped."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch
from scipy import sparse, stats

from illico_amd import AnnDataLite, _lib, blocked_wilcoxon, differential_expression
from illico_amd import blocked as blocked_mod
from illico_amd.blocked import compound_groups
from illico_amd.utils.groups import GroupContainer
from blocked_model import ALTERNATIVES, blocked_model, block_stats, combine, edge_case, labels_of, make_case

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
COLUMNS = ("p_value", "statistic", "fold_change", "z_score")


def _adata(X, case, B=None):
    b = case.b_codes if B is None else np.zeros_like(case.b_codes)
    return AnnDataLite(X, obs=pd.DataFrame({"g": labels_of(case.g_codes, "grp"), "b": labels_of(b, "blk")}))


def _planes(df, G):
    return {c: df[c].to_numpy().reshape(G, -1) for c in df.columns}


def _assert_model(got, want, what=""):
    """A frame's planes against a BlockedResult: statistic equal, z / p / fold at rtol 1e-12, NaN where the model has NaN."""
    np.testing.assert_array_equal(got["statistic"], want.statistic, err_msg=f"statistic {what}")
    np.testing.assert_allclose(got["z_score"], want.z, rtol=1e-12, atol=0, err_msg=f"z {what}")
    np.testing.assert_allclose(got["p_value"], want.p, rtol=1e-12, atol=0, err_msg=f"p {what}")
    np.testing.assert_allclose(got["fold_change"], want.fold, rtol=1e-12, atol=0, err_msg=f"fold {what}")
    np.testing.assert_allclose(got["auc"], want.auc, rtol=1e-12, atol=0, err_msg=f"auc {what}")
    np.testing.assert_array_equal(got["n_blocks"], np.repeat(want.n_blocks[:, None], got["n_blocks"].shape[1], axis=1), err_msg=f"n_blocks {what}")


@functools.lru_cache(maxsize=None)
def _case(G, B, W):
    return make_case(G, B, W)


@functools.lru_cache(maxsize=None)
def _stats(G, B, W, ref):
    c = _case(G, B, W)
    return block_stats(c.X, c.g_codes, c.b_codes, G, B, ref)


# ---- 1. one block: the row of the unblocked call ----
def _container_input(X, kind):
    if kind == "dense-host":
        return X
    if kind == "dense-device":
        return torch.from_numpy(X).cuda()
    return sparse.csc_matrix(X) if kind == "csc" else sparse.csr_matrix(X)


@pytest.mark.parametrize("kind", ["dense-host", "dense-device", "csc", "csr"])
@pytest.mark.parametrize("reference", ["grp000", None], ids=["reference", "rest"])
@pytest.mark.parametrize("values", ["counts", "plus-quarter"])
def test_one_block_is_the_unblocked_call(values, reference, kind):
    """B = 1 against differential_expression(scores=True, use_continuity=False): statistic and z_score equal as bytes, p and the fold
    change at rtol 1e-12 -- through the histogram feeder (counts) and the plane feeder (the float32 copy + 0.25)."""
    case = _case(3, 2, 65)
    X = case.X if values == "counts" else (case.X + np.float32(0.25))
    adata = _adata(_container_input(X, kind), case, B=1)
    got = blocked_wilcoxon(adata, False, "g", "b", reference)
    want = differential_expression(adata, False, "g", reference, scores=True, use_continuity=False)
    assert got.attrs["n_flagged_genes"] == (0 if values == "counts" else 65) and got.attrs["blocks"] == ["blk000"]
    assert got.index.equals(want.index)
    assert got["statistic"].to_numpy().tobytes() == want["statistic"].to_numpy().tobytes()
    assert got["z_score"].to_numpy().tobytes() == want["z_score"].to_numpy().tobytes()
    np.testing.assert_allclose(got["p_value"].to_numpy(), want["p_value"].to_numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["fold_change"].to_numpy(), want["fold_change"].to_numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["p_value_adj"].to_numpy(), want["p_value_adj"].to_numpy(), rtol=1e-12, atol=0)
    assert (got["n_blocks"] == 1).all()


# ---- 2. small shapes against the model ----
@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("B", [2, 3, 5])
@pytest.mark.parametrize("G", [2, 3, 5])
def test_small_shapes_against_the_model(G, B, W):
    case = _case(G, B, W)
    adata = _adata(case.X, case)
    for ref, reference in ((0, "grp000"), (None, None)):
        st = _stats(G, B, W, ref)
        for alternative in ALTERNATIVES:
            for tie_correct in (True, False):
                got = blocked_wilcoxon(adata, False, "g", "b", reference, alternative=alternative, tie_correct=tie_correct)
                assert got.attrs["n_flagged_genes"] == 0
                _assert_model(_planes(got, G), combine(st, ref, alternative, tie_correct), f"ref={ref} {alternative} tie={tie_correct}")


# ---- 3. the two feeders agree ----
def _block_planes(eng, X, case, ref, tie_correct):
    """z and U planes [B, G, W] (device) of one engine call per block on the block's rows, and the row map."""
    G, B, W = case.G, case.B, X.shape[1]
    zs = torch.zeros((B, G, W), dtype=torch.float64, device="cuda")
    us = torch.zeros((B, G, W), dtype=torch.float64, device="cuda")
    row_map = np.full((B, G), -1, dtype=np.int32)
    for b in range(B):
        rows = np.flatnonzero(case.b_codes == b)
        present, local = np.unique(case.g_codes[rows], return_inverse=True)
        n = np.bincount(local, minlength=present.size).astype(np.int64)
        grp = GroupContainer(local.astype(np.int64), n, np.argsort(local, kind="stable").astype(np.int64),
                             np.concatenate([[0], np.cumsum(n)]).astype(np.int64), -1 if ref is None else int(np.searchsorted(present, ref)))
        eng.set_groups(grp)
        p, U, fc, z = eng.run_dense(np.ascontiguousarray(X[rows]), 0, W, use_continuity=False, tie_correct=tie_correct, scores=True, device_out=True)
        us[b, :present.size], zs[b, :present.size] = U, z
        row_map[b, present] = np.arange(present.size)
    return zs, us, row_map


@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("B", [2, 3, 5])
@pytest.mark.parametrize("G", [2, 3, 5])
def test_the_two_feeders_agree(G, B, W):
    """blocked_from_planes on the planes of per-block engine calls equals blocked_from_hists byte for byte in z, statistic and p -- and
    in the fold change when both get the same sums plane."""
    case = _case(G, B, W)
    eng = _lib.get_engine()
    comp = compound_groups(case.g_codes, case.b_codes, G, B)
    counts = np.asarray(comp.counts)
    Xd = torch.from_numpy(case.X).cuda()
    for ref in (0, None):
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
                    assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (name, ref, tie_correct, alternative)
            no_fc = eng.blocked_from_planes(zs, us, row_map, counts=counts, ref=ref)
            assert no_fc[2] is None and no_fc[3].cpu().numpy().tobytes() == eng.blocked_from_hists(
                H, fl, counts=counts, n_blocks=B, ref=ref, tie_correct=tie_correct)[3].cpu().numpy().tobytes()


# ---- 4. blocks that do not count ----
@pytest.mark.parametrize("reference", ["grp000", None], ids=["reference", "rest"])
@pytest.mark.parametrize("kind", ["group-absent", "reference-absent", "no-shared-block", "one-against-one", "constant-block", "constant-gene"])
def test_blocks_that_do_not_count(kind, reference):
    case = edge_case(kind)
    ref = None if reference is None else 0
    want = blocked_model(*case, ref=ref)
    got = blocked_wilcoxon(_adata(case.X, case), False, "g", "b", reference)
    planes = _planes(got, case.G)
    _assert_model(planes, want, kind)
    dead = want.n_blocks == 0
    assert dead.any() == (kind == "no-shared-block" and ref == 0)
    for c in COLUMNS + ("p_value_adj", "auc"):
        assert np.isnan(planes[c][dead]).all() and not np.isnan(planes[c][~dead]).any(), c
    # the adjustment ignores the NaN rows: each live group across its genes, as scipy does it
    np.testing.assert_allclose(planes["p_value_adj"][~dead], stats.false_discovery_control(want.p[~dead], axis=1), rtol=1e-12, atol=0)
    if kind == "constant-gene":
        assert (planes["z_score"][:, 2] == 0).all() and (planes["p_value"][:, 2] == 1).all()
    # the float32 copy + 0.25 takes the plane feeder: the same ranks, so the same tests
    shifted = _planes(blocked_wilcoxon(_adata(case.X + np.float32(0.25), case), False, "g", "b", reference), case.G)
    for c in ("p_value", "statistic", "z_score", "n_blocks"):
        np.testing.assert_array_equal(shifted[c], planes[c], err_msg=c)


# ---- 5. a mixed window ----
def _mixed_case():
    case = make_case(3, 3, 130)
    X = case.X.copy()
    rng = np.random.RandomState(5)
    N = X.shape[0]
    flagged = [3, 62, 63, 64, 66, 100, 127, 129]
    X[:, 3] = rng.randint(0, 4, N) + 0.5
    X[:, 62] = rng.randint(0, 4, N) - 1.0
    X[:, 63] = np.where(rng.rand(N) < 0.3, 256.0, rng.randint(0, 3, N))
    X[:, 64] = rng.randn(N).astype(np.float32)
    X[:, 66] = rng.randint(0, 3, N) * 0.5
    X[:, 100] = -1.0 * rng.randint(0, 3, N)
    X[:, 127] = rng.rand(N).astype(np.float32)
    X[:, 129] = 256.0 + rng.randint(0, 3, N)
    return case._replace(X=X), flagged


@pytest.mark.parametrize("reference", ["grp000", None], ids=["reference", "rest"])
def test_mixed_window(reference):
    """Flagged genes (halves, negatives, values beyond 255, float noise) between count genes, across the 64-gene tile boundary."""
    case, flagged = _mixed_case()
    ref = None if reference is None else 0
    for kind in ("dense-host", "csc"):
        got = blocked_wilcoxon(AnnDataLite(_container_input(case.X, kind), obs=_adata(case.X, case).obs), False, "g", "b", reference)
        assert got.attrs["n_flagged_genes"] == len(flagged) and got.attrs["n_plane_genes"] == len(flagged)
        assert got.attrs["blocks"] == ["blk000", "blk001", "blk002"]
        _assert_model(_planes(got, case.G), blocked_model(*case, ref=ref), kind)


@pytest.mark.parametrize("side", ["host", "device"])
@pytest.mark.parametrize("ref", [0, None], ids=["reference", "rest"])
def test_pitch_and_flagged_columns_keep_the_callers_bytes(ref, side):
    """Through the C entry with out_ld > n_cols: the padding and the flagged columns come back as they were."""
    case, flagged = _mixed_case()
    G, B, W = case.G, case.B, case.X.shape[1]
    eng = _lib.get_engine()
    comp = compound_groups(case.g_codes, case.b_codes, G, B)
    eng.set_groups(comp)
    X = torch.from_numpy(case.X).cuda() if side == "device" else case.X
    H, fl = eng.group_value_hists(X, 0, W)
    assert sorted(np.flatnonzero(np.asarray(fl.cpu() if side == "device" else fl)).tolist()) == flagged
    wide = [np.full((G, W + 5), SENTINEL) for _ in range(4)]
    wide = [torch.from_numpy(q).cuda() for q in wide] if side == "device" else wide
    eng.blocked_from_hists(H, fl, counts=np.asarray(comp.counts), n_blocks=B, ref=ref, out=[q[:, :W] for q in wide])
    want = blocked_model(*case, ref=ref)
    live = np.setdiff1d(np.arange(W), flagged)
    for q, w in zip(wide, (want.p, want.statistic, want.fold, want.z)):
        q = q.cpu().numpy() if side == "device" else q
        assert (q[:, W:] == SENTINEL).all() and (q[:, flagged] == SENTINEL).all()
        np.testing.assert_allclose(q[:, live], w[:, live], rtol=1e-12, atol=0)
    # the plane feeder: padding of its input and output planes
    zs = torch.full((B, G, W + 3), np.nan, dtype=torch.float64, device="cuda")
    us = torch.full((B, G, W + 3), np.nan, dtype=torch.float64, device="cuda")
    z0, u0, row_map = _block_planes(eng, case.X, case, ref, True)
    zs[:, :, :W], us[:, :, :W] = z0, u0
    zin, uin = (zs[:, :, :W], us[:, :, :W]) if side == "device" else (zs.cpu().numpy()[:, :, :W], us.cpu().numpy()[:, :, :W])
    wide = [np.full((G, W + 5), SENTINEL) for _ in range(4)]
    wide = [torch.from_numpy(q).cuda() for q in wide] if side == "device" else wide
    out = [wide[0][:, :W], wide[1][:, :W], None, wide[3][:, :W]]
    eng.blocked_from_planes(zin, uin, row_map, counts=np.asarray(comp.counts), ref=ref, out=out)
    for k, w in ((0, want.p), (1, want.statistic), (3, want.z)):
        q = wide[k].cpu().numpy() if side == "device" else wide[k]
        assert (q[:, W:] == SENTINEL).all()
        np.testing.assert_allclose(q[:, :W], w, rtol=1e-12, atol=0)
    assert ((wide[2].cpu().numpy() if side == "device" else wide[2]) == SENTINEL).all()


# ---- 6. gene windows ----
def _log_counts_case():
    case = make_case(3, 2, 150)
    return case._replace(X=case.X.astype(np.float64))  # float64 0 .. 5: count-valued, and exact under expm1 sums in float64


def test_three_gene_windows(monkeypatch):
    """BLOCK_WINDOW_BYTES sized to 64 genes: windows (0, 64), (64, 128), (128, 150), under is_log1p with the fold change from the expm1
    sums -- the frame of the unwindowed call, and the model."""
    case = _log_counts_case()
    G, B = case.G, case.B
    adata = _adata(case.X, case)
    want = blocked_wilcoxon(adata, True, "g", "b", "grp000")
    per_gene = 2 * G * B * 1024 + B * 1024 + 4 * G * 8 + G * B * 8 + 4
    eng = _lib.get_engine()
    seen = []
    real = eng.blocked_from_hists
    monkeypatch.setattr(blocked_mod, "BLOCK_WINDOW_BYTES", per_gene * 64)
    monkeypatch.setattr(eng, "blocked_from_hists", lambda H, fl, **kw: (seen.append(int(H.shape[1])), real(H, fl, **kw))[1])
    got = blocked_wilcoxon(adata, True, "g", "b", "grp000")
    assert seen == [64, 64, 22]
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    _assert_model(_planes(got, G), blocked_model(*case, ref=0, is_log1p=True), "log1p windows")


def test_a_window_the_scratch_budget_refuses_is_halved(monkeypatch):
    """130 genes are three tiles of histograms; with room for two, the window (0, 130) is refused (by the histogram pass, which plans
    the same tiles) and done as (0, 128), (128, 130)."""
    case = make_case(3, 2, 130)
    G, B = case.G, case.B
    adata = _adata(torch.from_numpy(case.X).cuda(), case)
    want = blocked_wilcoxon(adata, False, "g", "b")
    eng = _lib.Engine(_lib.get_engine().device)  # (a context of its own: the shared engine keeps its scratch cap)
    try:
        # what the budgets count (pairwise.hip: pw_hists_run; blocked.hip: blk_plan): 64 KB of tiled histograms per compound group and
        # tile, 64 KB of block totals per block and tile, and the sizes (a few 256-byte slots)
        eng.set_option("scratch_bytes", (G * B + B) * 2 * 65536 + 4096)
        seen = []
        real = eng.blocked_from_hists
        eng.blocked_from_hists = lambda H, fl, **kw: (seen.append(int(H.shape[1])), real(H, fl, **kw))[1]
        with monkeypatch.context() as m:
            m.setattr(_lib, "get_engine", lambda device=None: eng)
            got = blocked_wilcoxon(adata, False, "g", "b")
    finally:
        eng.close()
    assert seen == [128, 2]
    pd.testing.assert_frame_equal(got, want, check_exact=True)


# ---- 7. refusals ----
def _c_call(eng, which, *, G=2, B=2, W=4, ref=0, counts=None, alternative=0, row_map=None, flags=4, out=None):
    """The C entry point `which` on small host arrays; returns (code, the output planes)."""
    counts = np.ascontiguousarray(np.full(max(G * B, 1), 5) if counts is None else counts, dtype=np.int64)
    out = [np.full((max(G, 1), W), SENTINEL) for _ in range(4)] if out is None else out
    sums = np.ones((max(G * B, 1), W))
    if which == "hists":
        H = np.zeros((max(G * B, 1), W, 256), dtype=np.uint32)
        H[:, :, 0] = 5
        fl = np.zeros(W, dtype=np.uint32)
        rc = eng.lib.illico_blocked_from_hists(eng.h, H.ctypes.data, fl.ctypes.data, counts.ctypes.data, G, B, W, ref, None, 0, flags, alternative,
                                               *[q.ctypes.data for q in out], W)
    else:
        z = np.zeros((max(G * B, 1), W))
        row_map = np.ascontiguousarray(np.tile(np.arange(max(G, 1)), max(B, 1)) if row_map is None else row_map, dtype=np.int32)
        rc = eng.lib.illico_blocked_from_planes(eng.h, z.ctypes.data, z.ctypes.data, W, row_map.ctypes.data, counts.ctypes.data, G, B, W, ref,
                                                sums.ctypes.data, W, flags & ~4, alternative, *[q.ctypes.data for q in out], W)
    return rc, out


REFUSALS = [
    ("no-block", dict(B=0), _lib.ERR_ARG),
    ("no-group", dict(G=0, ref=-1), _lib.ERR_ARG),
    ("one-group-with-reference", dict(G=1, ref=0), _lib.ERR_ARG),
    ("reference-beyond", dict(ref=2), _lib.ERR_ARG),
    ("reference-below", dict(ref=-2), _lib.ERR_ARG),
    ("negative-size", dict(counts=[5, 5, -1, 5]), _lib.ERR_ARG),
    ("pair-too-large", dict(counts=[1 << 20, 5, 1 << 20, 5]), _lib.ERR_UNSUPPORTED),
    ("pair-too-large-rest", dict(ref=-1, counts=[1 << 20, 5, 1 << 20, 5]), _lib.ERR_UNSUPPORTED),
    ("alternative", dict(alternative=3), _lib.ERR_ALTERNATIVE),
]


@pytest.mark.parametrize("which", ["hists", "planes"])
@pytest.mark.parametrize("name,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_of_the_c_entry_points(name, kw, code, which):
    eng = _lib.get_engine()
    rc, out = _c_call(eng, which, **kw)
    assert rc == code, (eng.lib.illico_last_error(eng.h), rc)
    assert all((q == SENTINEL).all() for q in out)  # a refused call leaves the poisoned planes as they were


@pytest.mark.parametrize("entry", [-2, 2])
def test_row_map_entries_outside_the_plane_set_are_refused(entry):
    eng = _lib.get_engine()
    rc, out = _c_call(eng, "planes", row_map=[0, 1, entry, 1])
    assert rc == _lib.ERR_ARG and b"row_map" in eng.lib.illico_last_error(eng.h)
    assert all((q == SENTINEL).all() for q in out)
    assert _c_call(eng, "planes", row_map=[0, 1, -1, 1])[0] == _lib.OK


def test_a_working_set_beyond_the_scratch_budget_is_refused():
    eng = _lib.Engine(_lib.get_engine().device)
    try:
        assert _c_call(eng, "hists")[0] == _lib.OK and _c_call(eng, "planes")[0] == _lib.OK
        eng.set_option("scratch_bytes", 1024)
        for which in ("hists", "planes"):
            rc, out = _c_call(eng, which)
            assert rc == _lib.ERR_OOM, eng.lib.illico_last_error(eng.h)
            assert all((q == SENTINEL).all() for q in out)
    finally:
        eng.close()


def test_the_accepted_small_call_is_right():
    """The arrays of _c_call are a valid call: every compound has 5 cells of value 0 -- constant blocks: z = 0, p = 1, U = n_g n_r / 2."""
    eng = _lib.get_engine()
    rc, (p, u, fc, z) = _c_call(eng, "hists")
    assert rc == _lib.OK and (p[1] == 1).all() and (z == 0).all() and (u[1] == 25.0).all() and (u[0] == -1).all() and (p[0] == 1).all()


def test_refusals_of_the_python_layer():
    case = _case(2, 2, 1)
    adata = _adata(case.X, case)
    with pytest.raises(ValueError, match="block_key"):
        blocked_wilcoxon(adata, False, "g", "batch")
    with pytest.raises(ValueError, match="not present"):
        blocked_wilcoxon(adata, False, "g", "b", "grp999")
    with pytest.raises(ValueError, match="alternative"):
        blocked_wilcoxon(adata, False, "g", "b", alternative="bigger")
    with pytest.raises(ValueError, match="correction method"):
        blocked_wilcoxon(adata, False, "g", "b", corr_method="holm")
    eng = _lib.get_engine()
    with pytest.raises(ValueError, match="n_blocks"):
        eng.blocked_from_hists(np.zeros((4, 1, 256), np.uint32), np.zeros(1, np.uint32), counts=[5] * 4, n_blocks=0)
    with pytest.raises(ValueError, match="compound groups"):
        eng.blocked_from_hists(np.zeros((4, 1, 256), np.uint32), np.zeros(1, np.uint32), counts=[5] * 4, n_blocks=3)


def test_n_genes_keeps_the_smallest_p():
    case = _case(3, 3, 65)
    adata = _adata(case.X, case)
    full = blocked_wilcoxon(adata, False, "g", "b", "grp000")
    top = blocked_wilcoxon(adata, False, "g", "b", "grp000", n_genes=7)
    assert len(top) == 3 * 7
    p = full["p_value"].to_numpy().reshape(3, 65)
    order = np.argsort(p + 0.0, axis=1, kind="stable")[:, :7]
    pd.testing.assert_frame_equal(top, full.iloc[(np.arange(3)[:, None] * 65 + order).reshape(-1)], check_exact=True)
