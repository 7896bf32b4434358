"""All-pairs Wilcoxon tests for any float32 / int32 values on the device (illico_pairwise_ranked_*: one sorted walk per gene) against the
CPU oracle run once per reference, the exact restatement of tests/test_pairwise_ranked_host.py, the histogram pair route and the
one-versus-reference engine routes; and pairwise_wilcoxon end to end on continuous values."""
import ctypes

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

from illico_amd import AnnDataLite, pairwise_wilcoxon
from illico_amd import _lib
from illico_amd._lib import get_engine
from test_pairwise_host import exact_planes, groups_of, held_to_exact, hists_numpy, labels_of, offdiag, with_stored_zeros
from test_pairwise_ranked_host import (KINDS, TIE_HEAVY, ints_of, ltx_numpy, ranked_case, ranked_exact, ranked_oracle_slabs, ranked_planes_numpy,
                                       recode)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ranked(eng, X, codes, lb, ub, *, layout="dense device", **kw):
    """(p, U, fc, z, left) as numpy, of one input layout, under the groups of ``codes``; the sums are the engine's own group_stats"""
    eng.set_groups(groups_of(codes))
    kind, side = layout.split()
    kw.setdefault("scores", True)
    if kind == "dense":
        Xs = _dev(X) if side == "device" else X
        sums = eng.group_stats(Xs, lb, ub)[1]
        got = eng.pairwise_ranked(Xs, lb, ub, sums=sums, **kw)
    else:
        M = with_stored_zeros(X, "csc")
        arrs = (M.data, M.indices.astype(np.int64 if side == "host" else np.int32), M.indptr.astype(np.int64 if side == "host" else np.int32))
        if side == "device":
            arrs = tuple(_dev(a) for a in arrs)
        sums = eng.group_stats_sparse("csc", *arrs, M.shape, lb, ub)[1]
        got = eng.pairwise_ranked_sparse("csc", *arrs, M.shape, lb, ub, sums=sums, **kw)
    assert _lib._is_torch_tensor(got[0]) == (side == "device")
    return tuple(_np(a) for a in got)


class _cap:
    """the engine with "pair_rank_cap" set for a block"""

    def __init__(self, eng, value):
        self.eng, self.value = eng, value

    def __enter__(self):
        self.eng.set_option("pair_rank_cap", self.value)

    def __exit__(self, *exc):
        self.eng.set_option("pair_rank_cap", 0)


# ---- small shapes against the oracle slabs ----
@pytest.mark.parametrize("W", [1, 63, 64, 65, 130])
def test_float32_windows_against_the_oracle(W):
    X, codes, counts = ranked_case("f32")
    p, U, fc, z, left = _ranked(get_engine(), X, codes, 0, W)
    assert left.shape == (W,) and not left.any()
    wp, wU, wfc = (a[:, :, :W] for a in ranked_oracle_slabs("f32"))
    keep = np.broadcast_to(offdiag(counts.size)[:, :, None], wU.shape)
    np.testing.assert_array_equal(U[keep], wU[keep])
    np.testing.assert_allclose(p[keep], wp[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(fc[keep], wfc[keep], rtol=1e-12, atol=0.0, equal_nan=True)
    d = np.arange(counts.size)
    assert np.all(p[d, d] == 1.0) and np.all(z[d, d] == 0.0) and np.array_equal(U[d, d], np.broadcast_to((counts ** 2 / 2.0)[:, None], (counts.size, W)))
    assert np.array_equal(z, -z.transpose(1, 0, 2))
    n = min(W, len(KINDS) + 3)                                     # z against the exact restatement on the constructed genes
    ex = ranked_exact("f32", tuple(range(len(KINDS) + 3)))
    np.testing.assert_allclose(z[:, :, :n], ex["z"][:, :, :n], rtol=1e-12, atol=0.0)


def test_int32_against_the_oracle():
    X, codes, counts = ranked_case("i32")
    p, U, fc, z, left = _ranked(get_engine(), X, codes, 0, X.shape[1])
    assert not left.any()
    wp, wU, wfc = ranked_oracle_slabs("i32")
    keep = np.broadcast_to(offdiag(counts.size)[:, :, None], wU.shape)
    np.testing.assert_array_equal(U[keep], wU[keep])
    np.testing.assert_allclose(p[keep], wp[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(fc[keep], wfc[keep], rtol=1e-12, atol=0.0, equal_nan=True)
    ex = ranked_exact("i32", (0, 1, 2, 3, 4, 5))
    np.testing.assert_allclose(z[:, :, :6], ex["z"], rtol=1e-12, atol=0.0)


def test_other_value_types_are_refused():
    X, codes, counts = ranked_case("f32")
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    for dt in (np.float64, np.int64):
        Xw = np.ascontiguousarray(X[:, :4]).astype(dt)
        out = tuple(np.full((8, 8, 4), 7.25) for _ in range(3)) + (np.full(4, 9, dtype=np.uint32),)
        with pytest.raises(NotImplementedError, match="float32 / int32"):
            eng.pairwise_ranked(Xw, 0, 4, sums=np.zeros((8, 4)), out=out)
        assert all(np.all(q == 7.25) for q in out[:3]) and np.all(out[3] == 9)


# ---- parts and stretches ----
def test_many_small_parts_give_the_same_bytes():
    X, codes, counts = ranked_case("f32")
    eng = get_engine()
    want = _ranked(eng, X, codes, 0, 40)
    with _cap(eng, 1024):                                          # 2660 non-zeros of a gene without zeros: three parts and more
        got = _ranked(eng, X, codes, 0, 40)
    assert not got[4].any()
    for a, b, name in zip(got, want, "p U fc z left".split()):
        assert np.array_equal(_bits(a), _bits(b)) if name != "left" else np.array_equal(a, b), name


@pytest.mark.parametrize("cap", [0, 1024])
def test_a_tie_heavy_gene_is_the_histogram_route_bit_for_bit(cap):
    X, codes, counts = ranked_case("f32")
    eng = get_engine()
    rc, d = recode(X[:, TIE_HEAVY])
    assert d <= 12
    H, _ = hists_numpy(rc[:, None].astype(np.float64), codes, counts.size)
    hp, hU, hfc, hz = eng.pairwise_from_hists(H.astype(np.uint32), np.zeros(1, dtype=np.uint32), counts=counts, scores=True)
    with _cap(eng, cap):
        p, U, fc, z, left = _ranked(eng, X, codes, TIE_HEAVY, TIE_HEAVY + 1)
    assert not left.any()
    for a, b in ((p, hp), (U, hU), (z, hz)):
        assert np.array_equal(_bits(a), _bits(b))


# ---- a part beyond the record slots ----
def _crowded_case():
    """(X float32 [4000, 2], codes, counts): gene 0 -- 3000 cells share 0.5, the others continuous around +-3; gene 1 -- 2000 neighbouring float32
    values and one outlier of 1e30 in a cell of group 0 (500 cells: within the rows the partition samples its key range from), else 0"""
    rng = np.random.RandomState(181)
    sizes = (500, 1500, 1000, 1000)
    codes = rng.permutation(np.repeat(np.arange(4), sizes))
    X = np.zeros((4000, 2), dtype=np.float32)
    X[:, 0] = ((3.0 + 0.1 * rng.normal(size=4000)) * rng.choice([-1.0, 1.0], size=4000)).astype(np.float32)   # (none within a coarse bucket of 0.5)
    X[rng.permutation(4000)[:3000], 0] = 0.5
    near = np.float32(1.0) + np.arange(2000, dtype=np.float32) * np.float32(2.0 ** -22)
    assert np.unique(near).size == 2000
    rows = rng.permutation(np.flatnonzero(codes != 0))[:2000]
    X[rows, 1] = near
    X[np.flatnonzero(codes == 0)[3], 1] = 1e30
    return X, codes.astype(np.int64), np.asarray(sizes, dtype=np.int64)


def test_one_value_beyond_the_slots_is_a_tie_block_and_many_values_leave():
    X, codes, counts = _crowded_case()
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    Xd = _dev(X)
    sums = eng.group_stats(Xd, 0, 2)[1]
    out = tuple(_dev(np.full((4, 4, 2), 7.25)) for _ in range(4)) + (_dev(np.full(2, 9, dtype=np.int32)),)
    with _cap(eng, 1024):
        eng.pairwise_ranked(Xd, 0, 2, sums=sums, scores=True, out=out)
    p, U, fc, z, left = (_np(a) for a in out)
    assert left.tolist() == [0, 2]
    assert all(np.all(q[:, :, 1] == 7.25) for q in (p, U, fc, z))           # the caller's bytes
    ex = ranked_planes_numpy(X[:, :1], codes, counts)
    keep = offdiag(4)[:, :, None]
    held_to_exact(p[:, :, :1], U[:, :, :1], z[:, :, :1], ex, keep, "3000 cells share 0.5")
    np.testing.assert_allclose(fc[:, :, :1][np.broadcast_to(keep, (4, 4, 1))], ex["fc"][np.broadcast_to(keep, (4, 4, 1))], rtol=1e-12, atol=0.0)
    # with the default slots both genes are taken, gene 0 to the same bytes
    p2, U2, fc2, z2, left2 = (_np(a) for a in eng.pairwise_ranked(Xd, 0, 2, sums=sums, scores=True))
    assert not left2.any()
    for a, b in ((p, p2), (U, U2), (z, z2), (fc, fc2)):
        assert np.array_equal(_bits(a[:, :, 0]), _bits(b[:, :, 0]))
    held_to_exact(p2[:, :, 1:], U2[:, :, 1:], z2[:, :, 1:], ranked_planes_numpy(X[:, 1:], codes, counts), keep, "2000 neighbours and an outlier")


def _assert_references(df, adata, refs, labels, *, is_log1p=False, scores=False, alternative="two-sided", use_continuity=True, tie_correct=True):
    """for the references ``refs``: df's block is the one-versus-reference call with that reference (statistic equal; p, fold change, z
    rtol 1e-12)"""
    from illico_amd.asymptotic_wilcoxon import _wilcoxon_planes
    M = adata.shape[1]
    for r in refs:
        planes, index = _wilcoxon_planes(adata, is_log1p, "g", r, 1, "auto", alternative, use_continuity, tie_correct, None, scores=scores)
        others = np.asarray(labels) != r
        mine = df.xs(r, level="reference")
        assert len(mine) == int(others.sum()) * M and list(dict.fromkeys(mine.index.get_level_values("pert"))) == list(np.asarray(labels)[others])
        want = [planes[k][others].reshape(-1) for k in range(planes.shape[0])]
        np.testing.assert_array_equal(mine["statistic"].to_numpy(), want[1], err_msg=f"reference {r}")
        for col, k in (("p_value", 0), ("fold_change", 2)) + ((("z_score", 3),) if scores else ()):
            np.testing.assert_allclose(mine[col].to_numpy(), want[k], rtol=1e-12, atol=0.0, equal_nan=True, err_msg=f"{col}, reference {r}")


def _adata(X, codes, fmt="dense"):
    Xc = {"dense": lambda a: a, "csr": sparse.csr_matrix, "csc": sparse.csc_matrix}[fmt](X)
    return AnnDataLite(Xc, obs=pd.DataFrame({"g": labels_of(codes)}))


def test_pairwise_wilcoxon_completes_a_gene_that_left():
    X, codes, counts = _crowded_case()
    adata = _adata(X, codes)
    eng = get_engine()
    with _cap(eng, 1024):
        df = pairwise_wilcoxon(adata, False, "g", scores=True)
    assert (df.attrs["n_flagged_genes"], df.attrs["n_ranked_genes"], df.attrs["n_fallback_genes"]) == (2, 1, 1)
    labels = [f"g{k:03d}" for k in range(4)]
    _assert_references(df, adata, labels, labels, scores=True)


# ---- sel ----
def test_a_subset_in_any_order():
    X, codes, counts = ranked_case("f32")
    eng = get_engine()
    full = _ranked(eng, X, codes, 0, 20)
    for sel in ([6, 2, 5], [7, 0], [1, 4]):                        # K = 2 among them; groups of one and two cells
        got = _ranked(eng, X, codes, 0, 20, sel=sel)
        assert got[0].shape == (len(sel), len(sel), 20) and not got[4].any()
        for a, b in zip(got[:4], full[:4]):
            assert np.array_equal(_bits(a), _bits(b[np.ix_(sel, sel)])), sel


def _many_groups(G, per, M, seed):
    rng = np.random.RandomState(seed)
    codes = rng.permutation(np.repeat(np.arange(G), per)).astype(np.int64)
    X = rng.lognormal(size=(G * per, M)).astype(np.float32) * (rng.rand(G * per, M) < 0.4)
    X[:, 0] = np.log1p(rng.poisson(1.0, size=G * per)).astype(np.float32)
    return X, codes, np.full(G, per, dtype=np.int64)


def test_sixty_four_groups():
    X, codes, counts = _many_groups(64, 20, 5, 191)
    eng = get_engine()
    p, U, fc, z, left = _ranked(eng, X, codes, 0, 5)
    assert not left.any()
    for j in range(5):                                             # the integers of the definition
        S2, _ = ltx_numpy(X[:, j], codes, counts, list(range(64)))
        want = np.array([[0.5 * float(2 * 20 * 20 - S2[r, g]) for g in range(64)] for r in range(64)])
        assert np.array_equal(U[:, :, j], want)
    for r in (0, 31, 63):                                          # p, z, fold change: the one-versus-reference routes
        eng.set_groups(groups_of(codes, r))
        ep, eU, efc, ez = (_np(a) for a in eng.run_dense(X, 0, 5, scores=True))
        others = np.arange(64) != r
        np.testing.assert_array_equal(U[r][others], eU[others])
        for a, b in ((p[r], ep), (z[r], ez), (fc[r], efc)):
            np.testing.assert_allclose(a[others], b[others], rtol=1e-12, atol=0.0, equal_nan=True)


def test_sixty_five_groups_are_refused_before_any_write():
    X, codes, counts = _many_groups(65, 4, 2, 192)
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    out = tuple(np.full((65, 65, 2), 7.25) for _ in range(3)) + (np.full(2, 9, dtype=np.uint32),)
    with pytest.raises(NotImplementedError, match="up to 64"):
        eng.pairwise_ranked(X, 0, 2, sums=np.zeros((65, 2)), out=out)
    assert all(np.all(q == 7.25) for q in out[:3]) and np.all(out[3] == 9)
    sub = tuple(np.full((64, 64, 2), 7.25) for _ in range(3)) + (np.full(2, 9, dtype=np.uint32),)
    eng.pairwise_ranked(X, 0, 2, sums=eng.group_stats(X, 0, 2)[1], sel=np.arange(64), out=sub)   # 64 of the 65 are taken
    assert not sub[3].any() and not any(np.any(q == 7.25) for q in sub[:3])
    for bad in ([3], [3, 3], [3, 65], [-1, 2]):
        with pytest.raises(ValueError):
            eng.pairwise_ranked(X, 0, 2, sums=np.zeros((65, 2)), sel=bad, out=tuple(np.full((len(bad),) * 2 + (2,), 7.25) for _ in range(3)) + (out[3],))
    assert np.all(out[3] == 9)


def test_pairwise_wilcoxon_beyond_sixty_four_groups_takes_the_fallback():
    X, codes, counts = _many_groups(130, 10, 4, 193)
    adata = _adata(X, codes)
    df = pairwise_wilcoxon(adata, False, "g")
    assert (df.attrs["n_flagged_genes"], df.attrs["n_ranked_genes"], df.attrs["n_fallback_genes"]) == (4, 0, 4)
    labels = [f"g{k:03d}" for k in range(130)]
    _assert_references(df, adata, ["g000", "g064", "g129"], labels)


# ---- options and layouts ----
@pytest.mark.parametrize("alternative", ["two-sided", "less", "greater"])
@pytest.mark.parametrize("use_continuity", [True, False])
@pytest.mark.parametrize("tie_correct", [True, False])
def test_options(alternative, use_continuity, tie_correct):
    X, codes, counts = ranked_case("f32")
    genes = (0, 1, 2, 6, 7)
    opts = dict(alternative=alternative, use_continuity=use_continuity, tie_correct=tie_correct)
    p, U, fc, z, left = _ranked(get_engine(), np.ascontiguousarray(X[:, list(genes)]), codes, 0, len(genes), **opts)
    ex = ranked_exact("f32", genes, **opts)
    held_to_exact(p, U, z, ex, offdiag(counts.size)[:, :, None], str(opts))


@pytest.mark.parametrize("layout", ["dense host", "csc host", "csc device"])
@pytest.mark.parametrize("window", [(0, 20), (3, 11)])
def test_layouts_give_the_same_bytes(layout, window):
    X, codes, counts = ranked_case("f32")
    Xw = np.ascontiguousarray(X[:, :20])
    eng = get_engine()
    lb, ub = window
    want = _ranked(eng, Xw, codes, lb, ub)
    got = _ranked(eng, Xw, codes, lb, ub, layout=layout)
    assert not got[4].any()
    for a, b, name in zip(got[:4], want[:4], "p U fc z".split()):
        if name == "fc":   # (the sums of a sparse layout are added in another order)
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0.0, equal_nan=True)
        else:
            assert np.array_equal(_bits(a), _bits(b)), name
    again = _ranked(eng, Xw, codes, lb, ub, layout=layout)
    for a, b in zip(got, again):
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


def test_unsorted_csc_columns_are_refused():
    X, codes, counts = ranked_case("f32")
    M = sparse.csc_matrix(X[:, :4])
    idx = M.indices.copy()
    s, e = M.indptr[1], M.indptr[2]
    idx[s:e] = idx[s:e][::-1]
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    with pytest.raises(ValueError, match="ascend"):
        eng.pairwise_ranked_sparse("csc", M.data, idx, M.indptr, M.shape, 0, 4, sums=np.zeros((8, 4)))


def test_pitches_beyond_the_window_through_the_c_entry():
    X, codes, counts = ranked_case("f32")
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    W, K, out_ld, sums_ld = 5, 8, 9, 7
    Xw = np.ascontiguousarray(X[:, :12])
    want = eng.pairwise_ranked(Xw, 2, 2 + W, sums=eng.group_stats(Xw, 2, 2 + W)[1], scores=True)
    sums = np.full((K, sums_ld), np.nan)
    sums[:, :W] = eng.group_stats(Xw, 2, 2 + W)[1]
    planes = [np.full((K, K, out_ld), 7.25) for _ in range(4)]
    left = np.full(W, 9, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = eng.lib.illico_pairwise_ranked_dense(eng.h, vp(Xw), _lib.dtype_code(np.float32), Xw.shape[0], 12, 12, 2, 2 + W, None, 0, vp(sums), sums_ld,
                                              _lib.FLAG_CONTINUITY | _lib.FLAG_TIE_CORRECT, 0, *[vp(q) for q in planes], out_ld, vp(left))
    assert rc == _lib.OK and not left.any()
    for q, w in zip(planes, want[:4]):
        assert np.array_equal(_bits(q[:, :, :W]), _bits(w)) and np.all(q[:, :, W:] == 7.25)


# ---- the 64-bit edge ----
def test_a_pair_of_two_million_cells():
    sizes = ((1 << 20) - 1, 1 << 20, 5)
    N = sum(sizes)
    rng = np.random.RandomState(201)
    codes = rng.permutation(np.repeat(np.arange(3), sizes)).astype(np.int64)
    counts = np.asarray(sizes, dtype=np.int64)
    X = np.empty((N, 2), dtype=np.float32)
    X[:, 0] = np.asarray([-1.5, 0.0, 2.0], dtype=np.float32)[codes]          # one value per group: complete separation, T near 2^63
    X[:, 1] = rng.permutation(np.arange(1, N + 1)).astype(np.float32)         # tie-free (integers below 2^24)
    eng = get_engine()
    p, U, fc, z, left = _ranked(eng, X, codes, 0, 2, layout="dense host")
    assert not left.any()
    keep = offdiag(3)[:, :, None]
    H = np.zeros((3, 1, 256), dtype=np.int64)
    H[0, 0, 0], H[1, 0, 1], H[2, 0, 2] = sizes
    rz, rp = held_to_exact(p[:, :, :1], U[:, :, :1], z[:, :, :1], exact_planes(H, counts), keep, "one value per group")
    print(f"complete separation: worst error / bound: z {rz:.4g}, p {rp:.4g}")
    by_group = [np.sort(X[codes == k, 1]) for k in range(3)]
    ints = {}
    for r in range(3):
        for g in range(3):
            below = int(np.searchsorted(by_group[r], by_group[g]).sum())     # pairs with x_r < x_g: L[g][r]
            ints[r, g, 0] = ints_of(2 * below if r != g else sizes[r] * sizes[g], 0, sizes[r], sizes[g])
    held_to_exact(p[:, :, 1:], U[:, :, 1:], z[:, :, 1:], exact_planes(np.zeros((3, 1, 1), dtype=np.int64), counts, ints=ints), keep, "tie-free")
    # one more cell: refused from the sizes, before any write
    codes2 = np.append(codes, 0)
    eng.set_groups(groups_of(codes2))
    out = tuple(np.full((3, 3, 2), 7.25) for _ in range(3)) + (np.full(2, 9, dtype=np.uint32),)
    with pytest.raises(NotImplementedError, match="2097152"):
        eng.pairwise_ranked(np.zeros((N + 1, 2), dtype=np.float32), 0, 2, sums=np.zeros((3, 2)), out=out)
    assert all(np.all(q == 7.25) for q in out[:3]) and np.all(out[3] == 9)


# ---- end to end ----
@pytest.mark.parametrize("fmt", ["dense", "csr"])
def test_a_log_normalised_matrix_takes_the_ranked_route_whole(fmt, monkeypatch):
    _, codes, counts = ranked_case("f32")
    rng = np.random.RandomState(211)                               # counts, scaled to 10 000 per cell, log1p'd: values 0 .. 9.2
    raw = rng.poisson(rng.uniform(0.05, 5.0, size=40) * rng.lognormal(0.0, 0.3, size=(codes.size, 1)))
    Xl = np.log1p(raw / (raw.sum(axis=1, keepdims=True) + 1.0) * 1.0e4).astype(np.float32)
    adata = _adata(Xl, codes, fmt)
    eng = get_engine()
    calls = []
    with monkeypatch.context() as m:
        m.setattr(_lib.Engine, "run_dense", lambda self, *a, **k: calls.append("run_dense"))
        m.setattr(_lib.Engine, "run_sparse", lambda self, *a, **k: calls.append("run_sparse"))
        eng.profile(True)
        try:
            eng.profile_reset()
            df = pairwise_wilcoxon(adata, True, "g", scores=True)
            prof = eng.profile_get()
        finally:
            eng.profile(False)
    assert calls == []
    n_flagged = df.attrs["n_flagged_genes"]
    assert n_flagged >= 30 and df.attrs["n_ranked_genes"] == n_flagged and df.attrs["n_fallback_genes"] == 0
    assert "k_pw_rank_pairs" in prof and "k_pw_rank_emit" in prof, prof
    labels = [f"g{k:03d}" for k in range(8)]
    _assert_references(df, adata, labels, labels, is_log1p=True, scores=True)
