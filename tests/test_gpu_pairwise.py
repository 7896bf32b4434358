"""All-pairs Wilcoxon tests on the device: per-(group, gene) value histograms from every input layout (illico_group_value_hists_*), the
pairs from them (illico_pairwise_from_hists) against the CPU oracle run once per reference and against the one-versus-reference
engine routes bit for bit, and pairwise_wilcoxon end to end.  Cases and the numpy restatement: tests/test_pairwise_host.py."""
import ctypes

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

from illico_amd import AnnDataLite, asymptotic_wilcoxon, pairwise_wilcoxon
from illico_amd import _lib
from illico_amd._lib import get_engine
from test_pairwise_host import CASE_A_FLAGGED, case, groups_of, hists_numpy, labels_of, offdiag, oracle_slabs

pytestmark = pytest.mark.gpu

LAYOUTS = ["dense host", "dense device", "csc host", "csc device", "csr host", "csr device"]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _with_explicit_zero(X, fmt):
    """scipy CSC / CSR of X with one stored zero added (at a cell that is zero)"""
    r, c = np.nonzero(X)
    zr, zc = (a[0] for a in np.nonzero(X == 0))
    M = sparse.coo_matrix((np.append(X[r, c], X.dtype.type(0)), (np.append(r, zr), np.append(c, zc))), shape=X.shape)
    M = M.tocsc() if fmt == "csc" else M.tocsr()
    assert M.nnz == r.size + 1
    return M


def _hists(eng, layout, X, lb, ub):
    """(H int64 [G, W, 256], flags bool [W]) of one input layout"""
    import torch
    kind, side = layout.split()
    if kind == "dense":
        H, fl = eng.group_value_hists(torch.from_numpy(X).cuda() if side == "device" else X, lb, ub)
    else:
        M = _with_explicit_zero(X, kind)
        idt = np.int64 if (kind == "csc") == (side == "host") else np.int32   # both index widths, on both sides
        arrs = (M.data, M.indices.astype(idt), M.indptr.astype(idt))
        if side == "device":
            arrs = tuple(torch.from_numpy(a).cuda() for a in arrs)
        H, fl = eng.group_value_hists_sparse(kind, *arrs, M.shape, lb, ub)
    assert _lib._is_torch_tensor(H) == (side == "device")
    return _np(H).astype(np.int64) & 0xFFFFFFFF, _np(fl) != 0


def _device_hists(eng, name):
    import torch
    X, codes, counts = case(name)
    eng.set_groups(groups_of(codes))
    return eng.group_value_hists(torch.from_numpy(X).cuda(), 0, X.shape[1])


def _check_against_oracle(got, name, flags, what, **opts):
    X, codes, counts = case(name)
    want = oracle_slabs(name, **opts)
    keep = offdiag(counts.size)[:, :, None] & ~flags[None, None, :]
    p, U, fc = (_np(a) for a in got[:3])
    np.testing.assert_array_equal(U[keep], want[1][keep], err_msg=f"statistic {what}")
    np.testing.assert_allclose(p[keep], want[0][keep], rtol=1e-12, atol=0.0, err_msg=f"p_value {what}")
    np.testing.assert_allclose(fc[keep], want[2][keep], rtol=1e-12, atol=0.0, equal_nan=True, err_msg=f"fold_change {what}")


# ---- histograms ----
@pytest.mark.parametrize("window", [(0, 130), (37, 101)])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_histograms_equal_numpy_counts(dtype, layout, window):
    X, codes, counts = case("A")
    integer = np.dtype(dtype).kind == "i"
    Xt = np.floor(X).astype(dtype) if integer else X.astype(dtype)   # the integer version: gene 9 loses its halves
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    lb, ub = window
    H, flags = _hists(eng, layout, Xt, lb, ub)
    wantH, want_flags = hists_numpy(Xt, codes, counts.size)
    flagged = (7, 11) if integer else CASE_A_FLAGGED
    assert np.array_equal(np.flatnonzero(want_flags), flagged)
    assert np.array_equal(lb + np.flatnonzero(flags), [j for j in flagged if lb <= j < ub])
    ok = ~want_flags[lb:ub]
    assert H.shape == (counts.size, ub - lb, 256)
    np.testing.assert_array_equal(H[:, ok], wantH[:, lb:ub][:, ok])
    assert np.array_equal(H[:, ok].sum(axis=2), np.broadcast_to(counts[:, None], (counts.size, int(ok.sum()))))


@pytest.mark.parametrize("name", ["B", "C"])
@pytest.mark.parametrize("layout", ["dense device", "csc device", "csr host"])
def test_histograms_wide_cells_and_many_groups(name, layout):
    X, codes, counts = case(name)
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    H, flags = _hists(eng, layout, X, 0, X.shape[1])
    wantH, want_flags = hists_numpy(X, codes, counts.size)
    assert not flags.any() and not want_flags.any()
    np.testing.assert_array_equal(H, wantH)
    if name == "B":
        assert H[0, 0, 2] == 66000  # beyond a 16-bit cell


# ---- pairs ----
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_pairs_match_the_oracle_for_every_reference(name):
    eng = get_engine()
    H, fl = _device_hists(eng, name)
    got = eng.pairwise_from_hists(H, fl)
    flags = _np(fl) != 0
    _check_against_oracle(got, name, flags, f"case {name}")
    X, codes, counts = case(name)
    p, U = _np(got[0]), _np(got[1])
    d = np.arange(counts.size)
    assert np.array_equal(p[d, d][:, ~flags], np.ones((counts.size, int((~flags).sum()))))
    assert np.array_equal(U[d, d][:, ~flags], np.broadcast_to((counts ** 2 / 2.0)[:, None], (counts.size, int((~flags).sum()))))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pairs_from_every_input_layout(layout):
    import torch
    X, codes, counts = case("A")
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    kind, side = layout.split()
    if kind == "dense":
        H, fl = eng.group_value_hists(torch.from_numpy(X).cuda() if side == "device" else X, 0, X.shape[1])
    else:
        M = _with_explicit_zero(X, kind)
        arrs = (M.data, M.indices, M.indptr)
        if side == "device":
            arrs = tuple(torch.from_numpy(a).cuda() for a in arrs)
        H, fl = eng.group_value_hists_sparse(kind, *arrs, M.shape, 0, X.shape[1])
    got = eng.pairwise_from_hists(H, fl)                      # host histograms give host planes, device ones device planes
    assert _lib._is_torch_tensor(got[0]) == (side == "device")
    _check_against_oracle(got, "A", _np(fl) != 0, layout)


@pytest.mark.parametrize("alternative", ["two-sided", "less", "greater"])
@pytest.mark.parametrize("use_continuity", [True, False])
@pytest.mark.parametrize("tie_correct", [True, False])
def test_pairs_options(alternative, use_continuity, tie_correct):
    eng = get_engine()
    H, fl = _device_hists(eng, "A")
    opts = dict(alternative=alternative, use_continuity=use_continuity, tie_correct=tie_correct)
    _check_against_oracle(eng.pairwise_from_hists(H, fl, **opts), "A", _np(fl) != 0, str(opts), **opts)


def test_pairs_log1p_fold_change_from_group_stats_sums():
    import torch
    X, codes, counts = case("A")
    eng = get_engine()
    H, fl = _device_hists(eng, "A")
    Xd = torch.from_numpy(X).cuda()
    sums = eng.group_stats(Xd, 0, X.shape[1], is_log1p=True)[1]
    got = eng.pairwise_from_hists(H, fl, sums=sums, is_log1p=True)
    # (gene 5 holds 253 .. 255: its float32 expm1 overflows, and inf / inf is NaN on both sides)
    _check_against_oracle(got, "A", _np(fl) != 0, "is_log1p", is_log1p=True)


def test_pairs_are_the_engine_planes_bit_for_bit():
    import torch
    X, codes, counts = case("A")
    eng = get_engine()
    H, fl = _device_hists(eng, "A")
    p, U, fc, z = (_np(a) for a in eng.pairwise_from_hists(H, fl, scores=True))
    ok = ~(_np(fl) != 0)
    Xd = torch.from_numpy(X).cuda()
    for r in range(counts.size):
        eng.set_groups(groups_of(codes, r))
        ep, eU, efc, ez = eng.run_dense(Xd, 0, X.shape[1], scores=True)
        rows = np.arange(counts.size) != r
        for mine, theirs, what in ((U[r], eU, "U"), (p[r], ep, "p"), (z[r], ez, "z")):
            assert np.array_equal(_bits(mine[rows][:, ok]), _bits(theirs[rows][:, ok])), f"{what}, reference {r}"
        np.testing.assert_allclose(fc[r][rows][:, ok], efc[rows][:, ok], rtol=1e-12, atol=0.0)


def test_pairs_antisymmetry():
    X, codes, counts = case("A")
    eng = get_engine()
    H, fl = _device_hists(eng, "A")
    ok = ~(_np(fl) != 0)
    p, U, fc, z = (_np(a)[:, :, ok] for a in eng.pairwise_from_hists(H, fl, scores=True))
    nn = (counts[:, None] * counts[None, :]).astype(np.float64)
    assert np.array_equal(U + U.transpose(1, 0, 2), np.broadcast_to(nn[:, :, None], U.shape))
    assert np.array_equal(_bits(z + 0.0), _bits(-z.transpose(1, 0, 2) + 0.0))
    assert np.array_equal(z[np.arange(8), np.arange(8)], np.zeros((8, int(ok.sum()))))
    assert np.array_equal(z[:, :, 3], np.zeros((8, 8)))  # gene 3 is constant (no flagged gene comes before it)
    less = _np(eng.pairwise_from_hists(H, fl, alternative="less")[0])[:, :, ok]
    greater = _np(eng.pairwise_from_hists(H, fl, alternative="greater")[0])[:, :, ok]
    off = offdiag(8)
    assert np.array_equal(_bits(less[off]), _bits(greater.transpose(1, 0, 2)[off]))


def test_sel_gives_the_sub_block_and_flagged_genes_stay_untouched():
    import torch
    eng = get_engine()
    H, fl = _device_hists(eng, "A")
    flags = _np(fl) != 0
    full = tuple(_np(a) for a in eng.pairwise_from_hists(H, fl, scores=True))
    sel = [6, 1, 4]
    payload = np.array([0x7FF8DEADBEEF0123], dtype=np.uint64).view(np.float64)[0]
    out = tuple(torch.full((3, 3, 130), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4))
    for o in out:
        o.view(torch.int64).fill_(int(np.array([payload]).view(np.int64)[0]))
    got = eng.pairwise_from_hists(H, fl, sel=sel, scores=True, out=out)
    for k in range(4):
        g = _np(got[k])
        want = full[k][np.ix_(sel, sel)]
        assert np.array_equal(_bits(g[:, :, ~flags]), _bits(want[:, :, ~flags])), f"plane {k}"
        assert np.all(_bits(g[:, :, flags]) == _bits(payload)), f"plane {k}: flagged genes were written"
    # host histograms and planes: the same bytes, the flagged columns of the caller's planes come back as they were
    hout = tuple(np.full((3, 3, 130), payload) for _ in range(4))
    eng.pairwise_from_hists(_np(H).view(np.uint32), _np(fl).view(np.uint32), sel=sel, scores=True, out=hout)
    for k in range(4):
        assert np.array_equal(_bits(hout[k]), _bits(_np(got[k]))), f"host plane {k}"


def test_refusals_before_anything_is_written():
    eng = get_engine()
    lib = eng.lib
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    H, fl = np.zeros((3, 1, 256), np.uint32), np.zeros(1, np.uint32)
    planes = [np.full((3, 3, 1), -7.0) for _ in range(3)]

    def call(counts, sel=None, alt=0):
        counts = np.asarray(counts, dtype=np.int64)
        s = None if sel is None else np.asarray(sel, dtype=np.int64)
        return lib.illico_pairwise_from_hists(eng.h, vp(H), vp(fl), vp(counts), 3, 1, None if s is None else vp(s), 0 if s is None else s.size, None, 0,
                                              _lib.FLAG_CONTINUITY | _lib.FLAG_TIE_CORRECT, alt, vp(planes[0]), vp(planes[1]), vp(planes[2]), None, 1)

    # a pair of 2^21 cells is refused from the sizes alone: no matrix of that size exists here
    assert call([1 << 20, 1 << 20, 5]) == _lib.ERR_UNSUPPORTED
    assert call([(1 << 20) - 1, 1 << 20, 5]) == _lib.OK and all(np.all(q != -7.0) for q in planes)
    for q in planes:
        q.fill(-7.0)
    assert call([1 << 20, 1 << 20, 5], sel=[0, 2]) == _lib.OK   # the large pair is not selected
    for q in planes:
        q.fill(-7.0)
    assert call([3, 4, 5], sel=[1]) == _lib.ERR_ARG
    assert call([3, 4, 5], sel=[1, 3]) == _lib.ERR_ARG
    assert call([3, 4, 5], sel=[1, -1]) == _lib.ERR_ARG
    assert call([3, 4, 5], sel=[1, 2, 1]) == _lib.ERR_ARG
    assert call([3, 4, 5], alt=7) == _lib.ERR_ALTERNATIVE
    assert all(np.all(q == -7.0) for q in planes)
    with pytest.raises(NotImplementedError, match="2097152"):
        eng.pairwise_from_hists(H, fl, counts=[1 << 20, 1 << 20, 5])
    with pytest.raises(ValueError):
        eng.pairwise_from_hists(H, fl, counts=[3, 4, 5], sel=[0])


# ---- end to end ----
def _adata(X, codes, fmt="dense"):
    Xc = {"dense": lambda a: a, "csr": sparse.csr_matrix, "csc": sparse.csc_matrix}[fmt](X)
    return AnnDataLite(Xc, obs=pd.DataFrame({"g": labels_of(codes)}))


def _assert_blocks(df, adata, labels, *, scores=False, **kw):
    """every (pert, reference) block of df is the pert's rows of asymptotic_wilcoxon with that reference"""
    M = adata.shape[1]
    for r in labels:
        ref = asymptotic_wilcoxon(adata, False, "g", reference=r, **kw)
        for g in labels:
            if g == r:
                assert (g, r) not in df.index.droplevel("feature")
                continue
            mine, theirs = df.xs((g, r), level=("pert", "reference")), ref.xs(g, level="pert")
            assert list(mine.index) == list(theirs.index) and len(mine) == M
            np.testing.assert_array_equal(mine["statistic"].to_numpy(), theirs["statistic"].to_numpy(), err_msg=f"{g} vs {r}")
            np.testing.assert_allclose(mine["p_value"].to_numpy(), theirs["p_value"].to_numpy(), rtol=1e-12, atol=0.0, err_msg=f"{g} vs {r}")
            np.testing.assert_allclose(mine["fold_change"].to_numpy(), theirs["fold_change"].to_numpy(), rtol=1e-12, atol=0.0, equal_nan=True)


@pytest.mark.parametrize("fmt", ["dense", "csr", "csc"])
def test_pairwise_wilcoxon_equals_one_call_per_reference(fmt):
    X, codes, counts = case("A")
    adata = _adata(X, codes, fmt)
    df = pairwise_wilcoxon(adata, False, "g")
    labels = [f"g{k:03d}" for k in range(8)]
    assert df.attrs["n_flagged_genes"] == 3
    assert list(df.columns) == ["p_value", "statistic", "fold_change"] and df.index.names == ["pert", "reference", "feature"]
    # reference-major, then pert, then gene; no group against itself
    want_index = [(g, r, f"gene_{j}") for r in labels for g in labels if g != r for j in range(130)]
    assert list(df.index) == want_index
    assert not df.isna().any().any()
    _assert_blocks(df, adata, labels)


def test_pairwise_wilcoxon_groups_scores_and_adjustment():
    X, codes, counts = case("A")
    adata = _adata(X, codes)
    sub = ["g006", "g001", "g004"]
    df = pairwise_wilcoxon(adata, False, "g", groups=sub, scores=True, corr_method="benjamini-hochberg", alternative="greater", use_continuity=False)
    assert list(df.columns) == ["p_value", "statistic", "fold_change", "z_score", "p_value_adj"]
    order = sorted(sub)
    assert list(dict.fromkeys((g, r) for g, r, _ in df.index)) == [(g, r) for r in order for g in order if g != r]
    _assert_blocks(df, adata, order, alternative="greater", use_continuity=False)
    full = pairwise_wilcoxon(adata, False, "g", scores=True, alternative="greater", use_continuity=False)
    eng = get_engine()
    for (g, r), block in df.groupby(level=("pert", "reference"), sort=False):
        ref = full.xs((g, r), level=("pert", "reference"))
        assert np.array_equal(_bits(block["z_score"].to_numpy()), _bits(ref["z_score"].to_numpy()))
        adj = eng.adjust_pvalues(np.ascontiguousarray(block["p_value"].to_numpy()[None, :]), "bh")
        assert np.array_equal(_bits(block["p_value_adj"].to_numpy()), _bits(adj[0]))


def test_count_valued_input_runs_the_pair_route_alone():
    X, codes, counts = case("A")
    keep = np.setdiff1d(np.arange(130), CASE_A_FLAGGED)
    adata = _adata(np.ascontiguousarray(X[:, keep]), codes)
    eng = get_engine()
    eng.profile(True)
    try:
        eng.profile_reset()
        df = pairwise_wilcoxon(adata, False, "g")
        prof = eng.profile_get()
    finally:
        eng.profile(False)
    assert df.attrs["n_flagged_genes"] == 0
    assert set(prof) == {"k_pw_hists_dense", "k_pw_hists_finish", "k_pw_pairs"}, prof
    want = oracle_slabs("A")
    p = df["p_value"].to_numpy().reshape(8 * 7, keep.size)
    wp = want[0][:, :, keep][offdiag(8)]
    np.testing.assert_allclose(p, wp, rtol=1e-12, atol=0.0)
