"""The all-pairs Wilcoxon route where tests/test_gpu_pairwise.py does not go: pairs at the size limit of the integer sums (2^21 - 1
cells, from synthetic histograms) held to exact arithmetic, the refusal boundary with values, small group counts and windows, the
strides of the C entry point; the value classifier on NaN, infinities, -0.0, a denormal and integers whose low bits look like a
count, on every layout; and the gene windows, chunks, streamed containers and options of pairwise_wilcoxon.  Builders and the exact
reference: tests/test_pairwise_host.py."""
import ctypes
import sys

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

import illico_amd.pairwise
from illico_amd import AnnDataLite, asymptotic_wilcoxon, differential_expression, pairwise_wilcoxon
from illico_amd import _lib
from illico_amd._lib import get_engine
from conftest import make_counts
from test_gpu_pairwise import LAYOUTS, _adata, _assert_blocks, _bits, _np
from test_pairwise_host import (CASE_A_FLAGGED, EDGE_MINUS_ZERO, big_exact, big_hists, case, edge_value_case, exact_planes, groups_of, held_to_exact,
                                hists_numpy, labels_of, offdiag, pairs_numpy, with_stored_zeros)

pytestmark = pytest.mark.gpu

PAYLOAD = np.array([0x7FF8DEADBEEF0123], dtype=np.uint64).view(np.float64)[0]


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _pairs_both_sides(eng, H, counts, **kw):
    """planes of pairwise_from_hists from device tensors, as numpy, after the assertion that host arrays give the same bytes"""
    W = H.shape[1]
    dev = eng.pairwise_from_hists(_dev(H, np.int32), _dev(np.zeros(W), np.int32), counts=counts, **kw)
    host = eng.pairwise_from_hists(H, np.zeros(W, dtype=np.uint32), counts=counts, **kw)
    assert all(_lib._is_torch_tensor(a) for a in dev) and all(isinstance(a, np.ndarray) for a in host)
    dev = tuple(_np(a) for a in dev)
    for k, (d, h) in enumerate(zip(dev, host)):
        assert np.array_equal(_bits(d), _bits(h)), f"plane {k}: device and host planes differ"
    return dev


def _per_reference(adata, is_log1p, r, scores):
    """the frame of asymptotic_wilcoxon with reference r; with scores, from differential_expression, which adds the z-score plane of
    the same engine call to the same three columns"""
    if scores:
        return differential_expression(adata, is_log1p, "g", reference=r, scores=True)
    return asymptotic_wilcoxon(adata, is_log1p, "g", reference=r)


# ---- A. pair arithmetic from synthetic histograms ----
@pytest.mark.parametrize("alternative", ["two-sided", "less", "greater"])
@pytest.mark.parametrize("use_continuity", [True, False])
@pytest.mark.parametrize("tie_correct", [True, False])
def test_values_at_the_size_limit_are_held_to_exact_arithmetic(alternative, use_continuity, tie_correct):
    H, n = big_hists()
    opts = dict(alternative=alternative, use_continuity=use_continuity, tie_correct=tie_correct)
    ex = big_exact(alternative, use_continuity, tie_correct)
    p, U, fc, z = _pairs_both_sides(get_engine(), H, n, scores=True, **opts)
    keep = np.broadcast_to(offdiag(n.size)[:, :, None], p.shape)
    rz, rp = held_to_exact(p, U, z, ex, keep, str(opts))
    print(f"{opts}: worst error / bound: z {rz:.4g}, p {rp:.4g}")
    # where the tie correction is well conditioned the float64 restatement is as good a reference as for any other case
    wp, wU, wfc, wz = pairs_numpy(H, n, **opts)
    well = keep & (ex["tie_corr"] >= 1.0e-3)
    assert well.sum() >= 0.80 * keep.sum()
    np.testing.assert_allclose(p[well], wp[well], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(z[well], wz[well], rtol=1e-12, atol=0.0)
    # the fold change from the integer value sums; inf where the reference's sum is 0
    np.testing.assert_allclose(fc, ex["fc"], rtol=1e-12, atol=0.0)
    assert np.isinf(ex["fc"]).any()
    d = np.arange(n.size)
    assert np.array_equal(p[d, d], np.ones((n.size, 70))) and np.array_equal(z[d, d], np.zeros((n.size, 70)))
    assert np.array_equal(U[d, d], np.broadcast_to((n.astype(np.float64) ** 2 / 2.0)[:, None], (n.size, 70)))


def test_antisymmetry_at_the_size_limit():
    H, n = big_hists()
    eng = get_engine()
    p, U, fc, z = _pairs_both_sides(eng, H, n, scores=True)
    nn = (n[:, None] * n[None, :]).astype(np.float64)
    assert np.array_equal(U + U.transpose(1, 0, 2), np.broadcast_to(nn[:, :, None], U.shape))
    assert np.array_equal(_bits(z + 0.0), _bits(-z.transpose(1, 0, 2) + 0.0))
    less = _pairs_both_sides(eng, H, n, alternative="less")[0]
    greater = _pairs_both_sides(eng, H, n, alternative="greater")[0]
    off = offdiag(n.size)
    assert np.array_equal(_bits(less[off]), _bits(greater.transpose(1, 0, 2)[off]))


def test_the_refusal_boundary_with_values():
    H, n = big_hists()
    eng = get_engine()
    full = _pairs_both_sides(eng, H, n, scores=True)
    H1, n1 = H.copy(), n.copy()
    n1[0] += 1                                                   # 2^20 + 2^20 cells: one more than the sums hold
    H1[0, :, 0] += 1
    W = H.shape[1]
    zeros = np.zeros(W, dtype=np.uint32)
    with pytest.raises(NotImplementedError, match="2097152"):
        eng.pairwise_from_hists(H1, zeros, counts=n1, scores=True)
    with pytest.raises(NotImplementedError, match="2097152"):
        eng.pairwise_from_hists(_dev(H1, np.int32), _dev(zeros, np.int32), counts=n1, scores=True)
    for sel in ([1, 2, 3, 4, 5], [0, 2, 3, 4, 5]):               # without group 0, without group 1: no pair of 2^21 cells is left
        got = _pairs_both_sides(eng, H1, n1, sel=sel, scores=True)
        same = [k for k, g in enumerate(sel) if g != 0]          # the groups that did not change
        ids = [sel[k] for k in same]
        for k in range(4):
            assert np.array_equal(_bits(got[k][np.ix_(same, same)]), _bits(full[k][np.ix_(ids, ids)])), f"sel {sel}, plane {k}"
    # the pairs of the group that grew to 2^20 cells (with 700 001 more the largest pair left), against exact arithmetic
    ex = exact_planes(H1[[0, 2, 3, 4, 5]], n1[[0, 2, 3, 4, 5]])
    with_0 = np.zeros((5, 5, 1), dtype=bool)
    with_0[0, 1:], with_0[1:, 0] = True, True
    held_to_exact(got[0], got[1], got[3], ex, with_0, "2^20 cells against the others")
    np.testing.assert_allclose(got[2], ex["fc"], rtol=1e-12, atol=0.0)


SMALL_SIZES = (90, 1, 64, 65, 2, 33, 7, 20, 18)


def _small(K, W):
    """(H int64 [K, W, 256], counts) of the first K groups and W genes of a 300-cell matrix with groups of 1 to 90 cells"""
    X = make_counts(61, 300, 129, 0.6)[0]
    codes = np.random.RandomState(161).permutation(np.repeat(np.arange(len(SMALL_SIZES)), SMALL_SIZES))
    H, flags = hists_numpy(X[:, :W], codes, len(SMALL_SIZES))
    assert not flags.any()
    return np.ascontiguousarray(H[:K]), np.asarray(SMALL_SIZES[:K], dtype=np.int64)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("K", [2, 3, 4, 5, 7, 9])
def test_small_group_counts_and_windows(K, W):
    H, n = _small(K, W)
    alternative = ("two-sided", "less", "greater")[(K + W) % 3]
    p, U, fc, z = _pairs_both_sides(get_engine(), H, n, scores=True, alternative=alternative)
    wp, wU, wfc, wz = pairs_numpy(H, n, alternative=alternative)
    assert p.shape == (K, K, W)
    np.testing.assert_array_equal(U, wU)
    np.testing.assert_allclose(p, wp, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(fc, wfc, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(z, wz, rtol=1e-12, atol=0.0)
    d = np.arange(K)
    assert np.array_equal(p[d, d], np.ones((K, W))) and np.array_equal(z[d, d], np.zeros((K, W)))
    assert np.array_equal(U[d, d], np.broadcast_to((n.astype(np.float64) ** 2 / 2.0)[:, None], (K, W)))


def test_a_non_ascending_sel_with_a_sums_plane():
    H, n = _small(9, 65)
    eng = get_engine()
    full = _pairs_both_sides(eng, H, n, scores=True)
    sel = [7, 2, 5, 0]
    sums = np.random.RandomState(162).uniform(0.5, 50.0, size=(9, 65))
    flags = np.zeros(65, dtype=np.uint32)
    dev = tuple(_np(a) for a in eng.pairwise_from_hists(_dev(H, np.int32), _dev(flags, np.int32), counts=n, sel=sel, sums=_dev(sums), scores=True))
    host = eng.pairwise_from_hists(H, flags, counts=n, sel=sel, sums=sums, scores=True)
    ns = n[sel].astype(np.float64)
    want_fc = (sums[sel][None, :, :] / ns[None, :, None]) / (sums[sel][:, None, :] / ns[:, None, None])      # [r, g, gene]
    for got in (dev, host):
        for k in (0, 1, 3):
            assert np.array_equal(_bits(got[k]), _bits(full[k][np.ix_(sel, sel)])), f"plane {k}"
        np.testing.assert_allclose(got[2], want_fc, rtol=1e-12, atol=0.0)
    assert np.array_equal(_bits(dev[2]), _bits(host[2]))


@pytest.mark.parametrize("side", ["host", "device"])
def test_strides_of_the_c_entry_point(side):
    import torch
    K, W, flagged = 5, 65, 17
    out_ld, sums_ld = W + 3, W + 5
    H, n = _small(K, W)
    eng = get_engine()
    lib = eng.lib
    H32 = np.ascontiguousarray(H, dtype=np.uint32)
    fl = np.zeros(W, dtype=np.uint32)
    fl[flagged] = 1
    sums = np.full((K, sums_ld), PAYLOAD)                        # (a NaN that is read instead of a sum shows in the fold change)
    sums[:, :W] = np.random.RandomState(163).uniform(0.5, 50.0, size=(K, W))
    want = eng.pairwise_from_hists(H32, fl, counts=n, sums=np.ascontiguousarray(sums[:, :W]), scores=True,
                                   out=tuple(np.full((K, K, W), PAYLOAD) for _ in range(4)))
    planes = [np.full((K, K, out_ld), PAYLOAD) for _ in range(4)]
    flags = _lib.FLAG_CONTINUITY | _lib.FLAG_TIE_CORRECT
    if side == "host":
        args, outs, keep = (H32, fl, sums), planes, None
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    else:
        keep = [_dev(H32.view(np.int32)), _dev(fl.view(np.int32)), _dev(sums)] + [_dev(q) for q in planes]
        args, outs = keep[:3], keep[3:]
        ptr = lambda a: ctypes.c_void_p(a.data_ptr())
        flags |= _lib.FLAG_INPUT_DEVICE | _lib.FLAG_OUTPUT_DEVICE
        torch.cuda.synchronize()                                 # (the raw entry point runs on the engine's stream, not on torch's)
    rc = lib.illico_pairwise_from_hists(eng.h, ptr(args[0]), ptr(args[1]), n.ctypes.data_as(ctypes.c_void_p), K, W, None, 0, ptr(args[2]), sums_ld, flags,
                                        0, *(ptr(q) for q in outs), out_ld)
    assert rc == _lib.OK, (lib.illico_last_error(eng.h) or b"").decode()
    eng.synchronize()
    ok = fl == 0
    for k in range(4):
        got = _np(outs[k])
        assert np.all(_bits(got[:, :, W:]) == _bits(PAYLOAD)), f"plane {k}: the padding was written"
        assert np.all(_bits(got[:, :, flagged]) == _bits(PAYLOAD)) and np.all(_bits(want[k][:, :, flagged]) == _bits(PAYLOAD)), f"plane {k}: the flagged gene"
        assert np.array_equal(_bits(got[:, :, :W][:, :, ok]), _bits(want[k][:, :, ok])), f"plane {k}"
        assert not np.isnan(got[:, :, :W][:, :, ok]).any()


# ---- B. the value classifier, on every layout ----
def _edge_hists(eng, layout, X, lb, ub):
    """(H int64 [G, W, 256], flags bool [W]) of one input layout; sparse layouts store every special value and a -0.0"""
    kind, side = layout.split()
    if kind == "dense":
        H, fl = eng.group_value_hists(_dev(X) if side == "device" else X, lb, ub)
    else:
        M = with_stored_zeros(X, kind)
        idt = np.int64 if (kind == "csc") == (side == "host") else np.int32   # both index widths, on both sides
        arrs = (M.data, M.indices.astype(idt), M.indptr.astype(idt))
        if side == "device":
            arrs = tuple(_dev(a) for a in arrs)
        H, fl = eng.group_value_hists_sparse(kind, *arrs, M.shape, lb, ub)
    return _np(H).astype(np.int64) & 0xFFFFFFFF, _np(fl) != 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_the_classifier_on_every_kind_of_value(dtype, layout):
    X, codes, counts, flagged, nan_genes = edge_value_case(dtype)
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    H, flags = _edge_hists(eng, layout, X, 0, X.shape[1])
    wantH, want_flags = hists_numpy(X, codes, counts.size)
    assert np.array_equal(np.flatnonzero(want_flags), sorted(flagged))
    assert np.array_equal(flags, want_flags), {j: flagged.get(j, "a gene without a special value") for j in np.flatnonzero(flags != want_flags)}
    ok = ~want_flags
    np.testing.assert_array_equal(H[:, ok], wantH[:, ok])        # the lanes next to a flagged gene stay exact
    assert np.array_equal(H[:, ok].sum(axis=2), np.broadcast_to(counts[:, None], (counts.size, int(ok.sum()))))
    # -0.0 counts in bin 0: per group, the gene's zeros of either sign, of which the rows [::4] hold -0.0 (0 for an integer type)
    zero = X[:, EDGE_MINUS_ZERO] == 0
    assert zero[::4].all() and (np.dtype(dtype).kind != "f" or np.signbit(X[::4, EDGE_MINUS_ZERO]).all())
    assert np.array_equal(H[:, EDGE_MINUS_ZERO, 0], np.bincount(codes[zero], minlength=counts.size))


def _edge_adata(fmt):
    X, codes, counts, flagged, nan_genes = edge_value_case(np.float32)
    Xc = X if fmt == "dense" else with_stored_zeros(X, fmt)
    return AnnDataLite(Xc, obs=pd.DataFrame({"g": labels_of(codes)}))


@pytest.mark.parametrize("fmt", ["dense", "csr"])
def test_flagged_genes_of_every_kind_end_to_end(fmt):
    X, codes, counts, flagged, nan_genes = edge_value_case(np.float32)
    adata = _edge_adata(fmt)
    with np.errstate(all="ignore"):
        df = pairwise_wilcoxon(adata, False, "g", scores=True)
        assert df.attrs["n_flagged_genes"] == len(flagged)
        labels = [f"g{k:03d}" for k in range(counts.size)]
        fl = np.array(sorted(j for j in flagged if j not in nan_genes))
        nan = np.array(nan_genes)
        for r in labels:
            ref = _per_reference(adata, False, r, True)
            for g in labels:
                if g == r:
                    continue
                mine, theirs = df.xs((g, r), level=("pert", "reference")), ref.xs(g, level="pert")
                assert list(mine.index) == list(theirs.index)
                for col in ("p_value", "statistic", "fold_change", "z_score"):
                    a, b = mine[col].to_numpy(), theirs[col].to_numpy()
                    if col == "statistic":
                        np.testing.assert_array_equal(a[fl], b[fl], err_msg=f"{g} vs {r}")
                    else:
                        np.testing.assert_allclose(a[fl], b[fl], rtol=1e-12, atol=0.0, equal_nan=col == "fold_change", err_msg=f"{col}, {g} vs {r}")
                    # (what the one-versus-reference route makes of NaN is its own subject: here, the same bytes)
                    assert np.array_equal(_bits(a[nan]), _bits(b[nan])), f"{col} of the gene with NaN, {g} vs {r}"


# ---- C. windows, chunks and options of pairwise_wilcoxon ----
LABELS_A = [f"g{k:03d}" for k in range(8)]
#: case A with a flagged gene in the middle window and in the ragged last tile as well
WIDE_FLAGGED = CASE_A_FLAGGED + (70, 129)


def _case_a_wide():
    X, codes, counts = case("A")
    X = X.copy()
    X[5, 70] = 300.0
    X[::13, 129] = 0.5
    return X, codes


def _blocks_equal_per_reference(df, adata, labels, flagged, *, is_log1p=False, scores=False):
    """every (pert, reference) block of df against asymptotic_wilcoxon with that reference: statistic equal, p and fold change at rtol
    1e-12; with scores z bit for bit for the count-valued genes and at rtol 1e-12 for the flagged ones"""
    M = adata.shape[1]
    ok = np.ones(M, dtype=bool)
    ok[list(flagged)] = False
    for r in labels:
        ref = _per_reference(adata, is_log1p, r, scores)
        for g in labels:
            if g == r:
                continue
            mine, theirs = df.xs((g, r), level=("pert", "reference")), ref.xs(g, level="pert")
            assert list(mine.index) == list(theirs.index) and len(mine) == M
            np.testing.assert_array_equal(mine["statistic"].to_numpy(), theirs["statistic"].to_numpy(), err_msg=f"{g} vs {r}")
            np.testing.assert_allclose(mine["p_value"].to_numpy(), theirs["p_value"].to_numpy(), rtol=1e-12, atol=0.0, err_msg=f"{g} vs {r}")
            np.testing.assert_allclose(mine["fold_change"].to_numpy(), theirs["fold_change"].to_numpy(), rtol=1e-12, atol=0.0, equal_nan=True,
                                       err_msg=f"{g} vs {r}")
            if scores:
                a, b = mine["z_score"].to_numpy(), theirs["z_score"].to_numpy()
                assert np.array_equal(_bits(a[ok]), _bits(b[ok])), f"z_score, {g} vs {r}"
                np.testing.assert_allclose(a[~ok], b[~ok], rtol=1e-12, atol=0.0, err_msg=f"z_score of flagged genes, {g} vs {r}")


def _profiled(eng, fn):
    eng.profile(True)
    try:
        eng.profile_reset()
        out = fn()
        return out, eng.profile_get()
    finally:
        eng.profile(False)


@pytest.mark.parametrize("fmt", ["dense", "csr", "csc"])
def test_several_gene_windows(monkeypatch, fmt):
    X, codes = _case_a_wide()
    adata = _adata(X, codes, fmt)
    want = pairwise_wilcoxon(adata, False, "g", scores=True)
    monkeypatch.setattr(illico_amd.pairwise, "PAIR_WINDOW_BYTES", 1)     # the width has a floor of one tile: windows (0, 64), (64, 128), (128, 130)
    got, prof = _profiled(get_engine(), lambda: pairwise_wilcoxon(adata, False, "g", scores=True))
    assert prof["k_pw_pairs"]["launches"] == 3, prof
    assert got.attrs["n_flagged_genes"] == want.attrs["n_flagged_genes"] == len(WIDE_FLAGGED)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    _assert_blocks(got, adata, LABELS_A)
    _blocks_equal_per_reference(got, adata, LABELS_A[2:4], WIDE_FLAGGED, scores=True)


def test_a_refused_window_is_halved(monkeypatch):
    X, codes, counts = case("A")
    X = X.copy()                                                 # no flagged gene here (test_several_gene_windows has them in every window):
    X[:, 7], X[:, 9], X[::11, 11] = np.minimum(X[:, 7], 255), np.floor(X[:, 9]), 1   # the one-versus-reference fallback plans its own scratch
    adata = _adata(X, codes)
    want = pairwise_wilcoxon(adata, False, "g", scores=True)
    assert want.attrs["n_flagged_genes"] == 0
    G, N = counts.size, X.shape[0]
    eng = _lib.Engine(get_engine().device)                       # (a context of its own: the shared engine keeps its scratch cap)
    try:
        # what pw_budget counts for the histogram pass (pairwise.hip: pw_hists_run): 64 KB of tiled histograms per group and tile, and
        # the staged rows of a host matrix.  Two tiles and 128 genes fit, three tiles do not; the pair call (K x tiles x 64 KB) fits
        # whenever that does.  (A change of what the budget counts is meant to show here: the windows below are stated exactly.)
        eng.set_option("scratch_bytes", G * 2 * 65536 + N * 128 * 4)
        with monkeypatch.context() as m:
            m.setattr(_lib, "get_engine", lambda device=None: eng)
            got, prof = _profiled(eng, lambda: pairwise_wilcoxon(adata, False, "g", scores=True))
    finally:
        eng.close()
    assert prof["k_pw_pairs"]["launches"] == 2, prof               # (0, 130) refused, then (0, 128) and (128, 130)
    assert got.attrs["n_flagged_genes"] == 0
    pd.testing.assert_frame_equal(got, want, check_exact=True)


@pytest.mark.parametrize("kind", ["h5-dense", "backed-csc"])
def test_streamed_containers_are_read_chunk_by_chunk(tmp_path, monkeypatch, kind):
    from illico_amd.utils.registry import H5pyBackedCSCDataHandler, H5pyDatasetDataHandler, data_handler_registry
    from test_gpu_out_of_core import FakeBackedCSC, FakeH5Dataset
    X, codes = _case_a_wide()
    obs = pd.DataFrame({"g": labels_of(codes)})
    want = pairwise_wilcoxon(AnnDataLite(X if kind == "h5-dense" else sparse.csc_matrix(X), obs=obs), False, "g", scores=True)
    cls, handler = (FakeH5Dataset, H5pyDatasetDataHandler) if kind == "h5-dense" else (FakeBackedCSC, H5pyBackedCSCDataHandler)
    monkeypatch.setattr(sys.modules["illico_amd.asymptotic_wilcoxon"], "STREAM_CHUNK_BYTES", 2600 * 4 * 50)   # 50 genes per chunk
    ds = cls(tmp_path / "x.backed", X)
    data_handler_registry[cls] = handler                         # what h5py.Dataset / anndata's _CSCDataset are registered under
    try:
        got = pairwise_wilcoxon(AnnDataLite(ds, obs=obs), False, "g", scores=True)
    finally:
        data_handler_registry.pop(cls, None)
    # one read per chunk, in order; the flagged columns (genes 7, 9, 11 / 70 / 129: every chunk has some) are gathered from the chunk
    # that was read for the histogram pass, so they cost no further read
    assert ds.reads == [(0, 50), (50, 100), (100, 130)]
    assert got.attrs["n_flagged_genes"] == len(WIDE_FLAGGED)
    pd.testing.assert_frame_equal(got, want, check_exact=True)


@pytest.mark.parametrize("fmt", ["dense", "csr", "csc"])
def test_is_log1p_on_every_container_and_with_a_subset_of_groups(fmt):
    X, codes, counts = case("A")
    adata = _adata(X, codes, fmt)
    # (gene 5 holds 253 .. 255: its float32 expm1 overflows, and inf / inf is NaN on both sides)
    with np.errstate(all="ignore"):
        df = pairwise_wilcoxon(adata, True, "g")
        assert df.attrs["n_flagged_genes"] == 3
        _blocks_equal_per_reference(df, adata, LABELS_A, CASE_A_FLAGGED, is_log1p=True)
        sub = ["g006", "g001", "g004"]                           # sel together with the sums plane
        part = pairwise_wilcoxon(adata, True, "g", groups=sub)
    order = sorted(sub)
    assert list(dict.fromkeys((g, r) for g, r, _ in part.index)) == [(g, r) for r in order for g in order if g != r]
    for (g, r), block in part.groupby(level=("pert", "reference"), sort=False):
        ref = df.xs((g, r), level=("pert", "reference"))
        for col in part.columns:
            assert np.array_equal(_bits(block[col].to_numpy()), _bits(ref[col].to_numpy())), f"{col}, {g} vs {r}"


@pytest.mark.parametrize("fmt", ["dense", "csr", "csc"])
def test_z_scores_equal_the_one_versus_reference_z_scores(fmt):
    X, codes, counts = case("A")
    adata = _adata(X, codes, fmt)
    df = pairwise_wilcoxon(adata, False, "g", scores=True)
    _blocks_equal_per_reference(df, adata, LABELS_A, CASE_A_FLAGGED, scores=True)


def test_a_device_tensor_as_the_matrix():
    X, codes = _case_a_wide()
    want = pairwise_wilcoxon(_adata(X, codes), False, "g", scores=True)
    got = pairwise_wilcoxon(AnnDataLite(_dev(X), obs=pd.DataFrame({"g": labels_of(codes)})), False, "g", scores=True)
    assert got.attrs["n_flagged_genes"] == len(WIDE_FLAGGED)
    assert got.index.equals(want.index) and list(got.columns) == list(want.columns)
    ok = ~got.index.get_level_values("feature").isin([f"gene_{j}" for j in WIDE_FLAGGED])
    assert ok.sum() == 8 * 7 * (130 - len(WIDE_FLAGGED))
    for col in got.columns:                                      # count-valued genes: the same histograms; flagged ones: another engine route
        a, b = got[col].to_numpy(), want[col].to_numpy()
        assert np.array_equal(_bits(a[ok]), _bits(b[ok])), col
        if col == "statistic":
            np.testing.assert_array_equal(a, b)
        else:
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0.0, err_msg=col)
