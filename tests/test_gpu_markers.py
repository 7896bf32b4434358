"""Per-group marker statistics on the device: Engine.combine_pairs (illico_combine_pairs) bit for bit against the numpy model of
tests/markers_model.py, and pairwise_markers against that model applied to pairwise_wilcoxon's frame.

The operations are IEEE float64 comparisons, multiplications and divisions in a fixed order, so p, the representative and every selected
effect are compared by their bits.  The model of a plane is computed once per K (on the widest plane; narrower cases are its first
columns, the combination being column by column) and shared by the sides, pitches and widths."""
import functools
import math

import numpy as np
import pandas as pd
import pytest
import torch
from scipy import sparse

from illico_amd import AnnDataLite, adjust_pvalues, pairwise_markers, pairwise_wilcoxon
from illico_amd import _lib
from markers_model import METHODS, combine_model

pytestmark = pytest.mark.gpu

KS = [2, 3, 4, 5, 33, 64, 65, 256]
WS = [1, 63, 64, 65, 257]
WMAX = max(WS)
TIES = np.array([0.0, 5e-324, 1e-300, 0.5, 1.0])
FILLS = ("uniform", "ties", "ones", "ascending", "descending")
SENTINEL = -7.25


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _fill(kind, K, rng):
    """One column [K, K] of p-values indexed [r, g]."""
    r = np.arange(K, dtype=np.float64)[:, None]
    if kind == "uniform":
        return rng.random((K, K))
    if kind == "ties":
        return rng.choice(TIES, size=(K, K))
    if kind == "ones":
        return np.ones((K, K))
    if kind == "ascending":   # in r: the representative of "all" is the last reference, of "any" the first
        return np.broadcast_to((r + 1.0) / (K + 1.0), (K, K)).copy()
    return np.broadcast_to((K - r) / (K + 1.0), (K, K)).copy()


@functools.lru_cache(maxsize=None)
def _plane_set(K):
    """(P, E0, E1) float64 [K, K, WMAX + 3]: column j is filled as FILLS[(j + K) % 5]; the diagonal holds NaN (even g) or 7.0 (odd g);
    E1 names its own position, so a wrong selection shows."""
    rng = np.random.default_rng(1000 + K)
    P = np.stack([_fill(FILLS[(j + K) % len(FILLS)], K, rng) for j in range(WMAX + 3)], axis=2)
    d = np.arange(K)
    P[d, d] = np.where(d % 2 == 0, np.nan, 7.0)[:, None]
    E0 = rng.normal(size=P.shape)
    E1 = (np.arange(K * K, dtype=np.float64).reshape(K, K, 1) * 1024.0 + np.arange(P.shape[2], dtype=np.float64))
    return P, E0, E1


def _ranks(K):
    n = K - 1
    return sorted({1, math.ceil(n / 2), n})


def _method_cases(K):
    return [("all", None), ("any", None)] + [("some", j) for j in _ranks(K)]


@functools.lru_cache(maxsize=None)
def _model(K, method, rank):
    P, E0, E1 = _plane_set(K)
    return combine_model(P[:, :, :WMAX], (E0[:, :, :WMAX], E1[:, :, :WMAX]), method=method, rank=rank)


def _to_side(a, side):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if side == "device" else np.ascontiguousarray(a)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _outputs(K, W, n_eff, side, pitch):
    """Sentinel-prefilled output planes [K, W], views of [K, pitch] blocks."""
    full = [np.full((K, pitch), SENTINEL), np.full((K, pitch), -7, dtype=np.int32)] + [np.full((K, pitch), SENTINEL) for _ in range(n_eff)]
    full = [_to_side(a, side) for a in full]
    return full, tuple(a[:, :W] for a in full)


def _sentinel_of(a):
    return -7 if a.dtype == np.int32 else SENTINEL


def _engine():
    return _lib.get_engine()


@pytest.mark.parametrize("side", ["device", "host"])
@pytest.mark.parametrize("K", KS)
def test_combine_matches_the_model_bit_for_bit(K, side):
    """Every K x W, both pitches (ld = W with allocated outputs; ld = W + 3 with outputs of another pitch), the three methods, j* at
    1, ceil(n / 2) and n; every fill in every plane of five columns or more (W = 1: the fill (K) % 5)."""
    eng = _engine()
    planes = _plane_set(K)
    for W in WS:
        tight = [_to_side(a[:, :, :W], side) for a in planes]
        wide = [_to_side(a[:, :, :W + 3], side) for a in planes]
        for method, rank in _method_cases(K):
            want = [w[:, :W] for w in _model(K, method, rank)]
            got = eng.combine_pairs(tight[0], tight[1:], method=method, rank=rank)
            full, out = _outputs(K, W, 2, side, W + 5)
            got2 = eng.combine_pairs(wide[0][:, :, :W], [e[:, :, :W] for e in wide[1:]], method=method, rank=rank, out=out)
            for name, w, a, b in zip(("p", "rep", "effect 0", "effect 1"), want, got, got2):
                a, b = _host(a), _host(b)
                assert a.dtype == w.dtype and a.shape == (K, W)
                bad = np.argwhere(_bits(a) != _bits(w))
                assert bad.size == 0, f"K={K} W={W} {method} j*={rank} {name}: {len(bad)} differ, first (g, j) = {bad[0]}: {a[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"
                assert np.array_equal(_bits(b), _bits(w)), f"K={K} W={W} {method} j*={rank} {name}, pitched"
            for a in full:  # the columns beyond W of the wider output blocks are not written
                a = _host(a)
                assert (a[:, W:] == _sentinel_of(a)).all()


@pytest.mark.parametrize("side", ["device", "host"])
def test_default_rank_and_effect_counts(side):
    """rank=None is max(1, ceil(n * min_prop)); zero and four effect planes."""
    eng = _engine()
    K, W = 5, 65
    P, E0, E1 = (a[:, :, :W] for a in _plane_set(K))
    Pd = _to_side(P, side)
    for min_prop, j in ((0.5, 2), (1.0, 4), (0.01, 1), (0.75, 3)):
        got = eng.combine_pairs(Pd, method="some", min_prop=min_prop)
        want = combine_model(P, method="some", rank=j)
        assert len(got) == 2 and all(np.array_equal(_bits(_host(a)), _bits(w)) for a, w in zip(got, want))
    effects = (E0, E1, -E0, E1 + 0.5)
    got = eng.combine_pairs(Pd, [_to_side(e, side) for e in effects], method="any")
    want = combine_model(P, effects, method="any")
    assert len(got) == 6 and all(np.array_equal(_bits(_host(a)), _bits(w)) for a, w in zip(got, want))
    with pytest.raises(ValueError, match="at most 4"):
        eng.combine_pairs(Pd, [Pd] * 5, method="any")


@pytest.mark.parametrize("side", ["device", "host"])
@pytest.mark.parametrize("K, W", [(4, 65), (33, 257)])
def test_skipped_columns_are_neither_validated_nor_written(K, W, side):
    eng = _engine()
    P, E0, E1 = (a[:, :, :W].copy() for a in _plane_set(K))
    rng = np.random.default_rng(K)
    skip = (rng.random(W) < 0.4)
    skip[0] = True
    skip[W - 1] = False
    P[:, :, skip] = np.where(rng.random((K, K, int(skip.sum()))) < 0.5, np.nan, -3.0)   # what an untouched column may hold
    words = np.where(skip, rng.integers(1, 2**31 - 1, size=W), 0)
    skip_arg = torch.from_numpy(words.astype(np.int32)).cuda() if side == "device" else words.astype(np.uint32)
    for method, rank in _method_cases(K):
        want = [w[:, :W] for w in _model(K, method, rank)]
        full, out = _outputs(K, W, 2, side, W + 1)
        eng.combine_pairs(_to_side(P, side), [_to_side(E0, side), _to_side(E1, side)], method=method, rank=rank, skip=skip_arg, out=out)
        for a, w in zip(full, want):
            a = _host(a)
            assert np.array_equal(_bits(a[:, :W][:, ~skip]), _bits(w[:, ~skip]))
            assert (a[:, :W][:, skip] == _sentinel_of(a)).all() and (a[:, W:] == _sentinel_of(a)).all()


def test_host_planes_staged_in_several_batches():
    """A scratch budget that holds eight columns of a batch: the same bits, skipped columns kept, and an invalid p named by its
    column in the whole plane."""
    eng = _lib.Engine(0)
    try:
        eng.set_option("scratch_bytes", 4096)  # K = 5, one effect plane, skip: 504 bytes per column
        K, W = 5, 257
        P, E0, _ = (a[:, :, :W].copy() for a in _plane_set(K))
        skip = np.zeros(W, dtype=np.uint32)
        skip[[3, 8, 100, 256]] = 1
        P[:, :, skip != 0] = np.nan
        for method, rank in _method_cases(K):
            want = [w[:, :W] for w in _model(K, method, rank)[:3]]
            full, out = _outputs(K, W, 1, "host", W)
            eng.combine_pairs(P, [E0], method=method, rank=rank, skip=skip, out=out)
            for a, w in zip(out, want):
                assert np.array_equal(_bits(a[:, skip == 0]), _bits(w[:, skip == 0])) and (a[:, skip != 0] == _sentinel_of(a)).all()
        P[2, 1, 200] = 1.5
        with pytest.raises(ValueError, match=r"reference 2, group 1, column 200\) is 1\.5"):
            eng.combine_pairs(P, method="any", skip=skip)
    finally:
        eng.close()


@pytest.mark.parametrize("side", ["device", "host"])
@pytest.mark.parametrize("bad", [np.nan, -0.1, 1.0000001])
def test_an_invalid_p_is_named_and_nothing_is_written(bad, side):
    eng = _engine()
    K, W = 5, 65
    P, E0, _ = (a[:, :, :W].copy() for a in _plane_set(K))
    P[3, 1, 40] = bad      # the first in (reference, group, column) order ...
    P[3, 2, 7] = -1.0      # ... of two
    for method in METHODS:
        full, out = _outputs(K, W, 1, side, W + 2)
        with pytest.raises(ValueError, match=r"reference 3, group 1, column 40\) is " + ("nan:" if np.isnan(bad) else repr(float(bad)).replace(".", r"\.") + r"\d*:")):
            eng.combine_pairs(_to_side(P, side), [_to_side(E0, side)], method=method, out=out)
        for a in full:
            a = _host(a)
            assert (a == _sentinel_of(a)).all()
    # the same value in a skipped column, or on the diagonal, raises nothing
    skip = np.zeros(W, dtype=np.int32)
    skip[[40, 7]] = 1
    eng.combine_pairs(_to_side(P, side), method="any", skip=torch.from_numpy(skip).cuda() if side == "device" else skip.astype(np.uint32))


def test_refusals():
    eng = _engine()
    with pytest.raises(NotImplementedError, match="257 groups"):
        eng.combine_pairs(np.full((257, 257, 1), 0.5), method="any")
    with pytest.raises(NotImplementedError, match="257 groups"):
        eng.combine_pairs(torch.full((257, 257, 1), 0.5, dtype=torch.float64, device="cuda"), method="all")
    with pytest.raises(ValueError, match="a pair needs two"):
        eng.combine_pairs(np.full((1, 1, 4), 0.5), method="any")
    P = np.full((5, 5, 4), 0.5)
    for rank in (0, 5, -1):
        with pytest.raises(ValueError, match="rank_j"):
            eng.combine_pairs(P, method="some", rank=rank)
    with pytest.raises(ValueError, match="Unknown combination method"):
        eng.combine_pairs(P, method="top")
    with pytest.raises(ValueError, match=r"\[K, K, W\]"):
        eng.combine_pairs(np.full((5, 4, 4), 0.5), method="any")
    with pytest.raises(ValueError, match="same side"):
        eng.combine_pairs(P, [torch.from_numpy(P).cuda()], method="any")
    with pytest.raises(ValueError, match="side of p"):
        eng.combine_pairs(P, method="any", out=(torch.empty((5, 4), dtype=torch.float64, device="cuda"), torch.empty((5, 4), dtype=torch.int32, device="cuda")))
    lib = eng.lib  # the C side's own refusals, before anything is written: a null p, a pitch below W
    out_p, out_rep = np.full((5, 4), SENTINEL), np.full((5, 4), -7, dtype=np.int32)
    args = lambda p, in_ld, out_ld, method=1: (eng.h, p, None, None, None, None, 5, 4, in_ld, None, method, 1, 0, out_p.ctypes.data, out_rep.ctypes.data,
                                               None, None, None, None, out_ld)
    for a in (args(None, 4, 4), args(P.ctypes.data, 3, 4), args(P.ctypes.data, 4, 3), args(P.ctypes.data, 4, 4, method=3)):
        assert lib.illico_combine_pairs(*a) == _lib.ERR_ARG
    assert (out_p == SENTINEL).all() and (out_rep == -7).all()


def test_two_runs_give_identical_bytes():
    eng = _engine()
    K, W = 64, 257
    dev = [_to_side(a[:, :, :W], "device") for a in _plane_set(K)]
    for method, rank in _method_cases(K):
        a = eng.combine_pairs(dev[0], dev[1:], method=method, rank=rank)
        b = eng.combine_pairs(dev[0], dev[1:], method=method, rank=rank)
        assert all(_host(x).tobytes() == _host(y).tobytes() for x, y in zip(a, b))


# ---- the front end ----
N_CELLS, N_GENES, SIZES = 300, 70, (100, 80, 60, 40, 20)
CONSTANT_GENE = 11


@functools.lru_cache(maxsize=None)
def _matrix():
    """300 cells x 70 genes, float32: the even genes count-valued (Poisson), the odd ones continuous; gene 11 constant; 5 unequal groups."""
    rng = np.random.default_rng(7)
    codes = rng.permutation(np.repeat(np.arange(len(SIZES)), SIZES))
    shift = rng.random((len(SIZES), N_GENES)) * 2.0
    X = np.empty((N_CELLS, N_GENES), dtype=np.float32)
    X[:, 0::2] = rng.poisson(1.0 + shift[codes][:, 0::2])
    X[:, 1::2] = (rng.normal(size=(N_CELLS, N_GENES // 2)) + shift[codes][:, 1::2]).astype(np.float32)
    X[:, CONSTANT_GENE] = 2.5
    return X, np.array([f"g{c}" for c in codes])


def _adata(fmt, dtype=np.float32):
    X, labels = _matrix()
    X = X.astype(dtype)
    Xc = {"dense": lambda a: a, "csr": sparse.csr_matrix, "csc": sparse.csc_matrix}[fmt](X)
    return AnnDataLite(Xc, obs=pd.DataFrame({"g": labels}))


def _frame_planes(df, labels, M):
    """[K, K, M] planes (p, U, fold change, z) of pairwise_wilcoxon's frame: reference-major, then pert, then gene; the diagonal NaN."""
    K = len(labels)
    planes = np.full((4, K, K, M), np.nan)
    pos = 0
    for r in range(K):
        for g in range(K):
            if r == g:
                continue
            rows = df.iloc[pos * M:(pos + 1) * M]
            assert rows.index[0][:2] == (labels[g], labels[r])
            for k, col in enumerate(("p_value", "statistic", "fold_change", "z_score")):
                planes[k, r, g] = rows[col].to_numpy()
            pos += 1
    return planes


@functools.lru_cache(maxsize=None)
def _pair_model(groups=None):
    """(labels, the four [K, K, M] planes of pairwise_wilcoxon(scores=True) on the dense float32 matrix, the sizes of the groups)."""
    df = pairwise_wilcoxon(_adata("dense"), False, "g", scores=True, groups=None if groups is None else list(groups))
    labels = sorted(set(_matrix()[1])) if groups is None else sorted(groups)
    sizes = np.array([SIZES[int(x[1:])] for x in labels], dtype=np.float64)
    return labels, _frame_planes(df, labels, N_GENES), sizes


def _want_frame(pval_type, groups=None, min_prop=0.5):
    labels, planes, sizes = _pair_model(groups)
    p, rep, U, fc, z = combine_model(planes[0], planes[1:], method=pval_type, min_prop=min_prop)
    return labels, dict(p_value=p, reference=np.array(labels)[rep], statistic=U, fold_change=fc, z_score=z, auc=U / (sizes[:, None] * sizes[rep]))


def _assert_frame(df, labels, want, rows=None):
    K = len(labels)
    assert df.index.names == ["pert", "feature"]
    if rows is None:
        assert len(df) == K * N_GENES
        assert list(df.index.get_level_values(0)) == [x for x in labels for _ in range(N_GENES)]
        assert list(df.index.get_level_values(1)) == [f"gene_{j}" for j in range(N_GENES)] * K
    for col, w in want.items():
        w = w.reshape(-1) if rows is None else w.reshape(-1)[rows]
        got = df[col].to_numpy() if col != "reference" else np.asarray(df[col].astype(str))
        if col == "reference":
            assert isinstance(df[col].dtype, pd.CategoricalDtype) and np.array_equal(got, w)
        else:
            assert np.array_equal(got, w, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(w)), col


@pytest.mark.parametrize("fmt", ["dense", "csr", "csc"])
def test_pairwise_markers_equals_the_model_of_the_pair_frame(fmt):
    for pval_type in ("any", "some", "all"):
        df = pairwise_markers(_adata(fmt), False, "g", pval_type=pval_type)
        labels, want = _want_frame(pval_type)
        assert list(df.columns) == ["p_value", "p_value_adj", "reference", "statistic", "fold_change", "z_score", "auc"]
        _assert_frame(df, labels, want)
        adj = adjust_pvalues(np.ascontiguousarray(want["p_value"]), "benjamini-hochberg")
        assert np.array_equal(df["p_value_adj"].to_numpy(), adj.reshape(-1))
        assert df.attrs["n_flagged_genes"] == N_GENES // 2 and df.attrs["n_ranked_genes"] == N_GENES // 2 and df.attrs["n_fallback_genes"] == 0
        # the constant gene: every p is 1, so is every combination of them
        assert (df["p_value"].to_numpy().reshape(len(labels), N_GENES)[:, CONSTANT_GENE] == 1.0).all()


def test_pairwise_markers_options():
    """min_prop, corr_method (another method; None drops the column), groups= restricted to three labels, n_genes=7."""
    labels, want = _want_frame("some", min_prop=1.0)
    df = pairwise_markers(_adata("dense"), False, "g", pval_type="some", min_prop=1.0, corr_method="bonferroni")
    _assert_frame(df, labels, want)
    assert np.array_equal(df["p_value_adj"].to_numpy(), adjust_pvalues(np.ascontiguousarray(want["p_value"]), "bonferroni").reshape(-1))
    assert "p_value_adj" not in pairwise_markers(_adata("dense"), False, "g", corr_method=None).columns
    three = ("g3", "g0", "g4")
    for fmt in ("dense", "csc"):
        df = pairwise_markers(_adata(fmt), False, "g", groups=list(three), pval_type="any")
        labels, want = _want_frame("any", groups=three)
        assert labels == ["g0", "g3", "g4"]
        _assert_frame(df, labels, want)
    labels, want = _want_frame("any")
    df = pairwise_markers(_adata("dense"), False, "g", n_genes=7)
    top = np.argsort(want["p_value"], axis=1, kind="stable")[:, :7]
    rows = (np.arange(len(labels))[:, None] * N_GENES + top).reshape(-1)
    assert len(df) == 7 * len(labels) and list(df.index.get_level_values(1)) == [f"gene_{j}" for j in top.reshape(-1)]
    _assert_frame(df, labels, want, rows=rows)
    adj = adjust_pvalues(np.ascontiguousarray(want["p_value"]), "benjamini-hochberg").reshape(-1)
    assert np.array_equal(df["p_value_adj"].to_numpy(), adj[rows])
    assert df.attrs["n_flagged_genes"] == N_GENES // 2


def _collect(adata, dtype_sel=None):
    from illico_amd.group_stats import _input
    from illico_amd.pairwise import _select, pairwise_planes
    from illico_amd.utils.groups import encode_and_count_groups
    from illico_amd.utils.registry import data_handler_registry
    X = _input(adata, None)
    uniq, container = encode_and_count_groups(groups=adata.obs["g"], ref_group=None)
    sel = _select(np.asarray(uniq), None)
    blocks = []

    def sink(cols, planes, skip):
        assert all(q.is_cuda and q.dtype == torch.float64 and tuple(q.shape) == (sel.size, sel.size, len(cols)) for q in planes)
        assert skip is None or (skip.is_cuda and tuple(skip.shape) == (len(cols),))
        blocks.append((np.asarray(cols), [q.cpu().numpy() for q in planes], None if skip is None else skip.cpu().numpy()))

    res = pairwise_planes(X, data_handler_registry.get(X), container, sel, False, "two-sided", True, True, True, sink=sink)
    return res, blocks


@pytest.mark.parametrize("fmt, dtype, n_fallback", [("dense", np.float32, 0), ("csr", np.float32, 0), ("dense", np.float64, N_GENES // 2), ("csc", np.float64, N_GENES // 2)])
def test_the_sink_receives_every_gene_exactly_once(fmt, dtype, n_fallback):
    """No host planes; over the blocks of the three sites every gene is live exactly once, and what is live equals pairwise_wilcoxon's
    planes (bit for bit on the routes that frame took itself; the per-reference fallback of float64 input to the tolerance the routes
    keep among themselves: U exact, p / fold change / z to a relative 1e-12)."""
    (planes, n_flagged, n_fb), blocks = _collect(_adata(fmt, dtype))
    assert planes is None and n_flagged == N_GENES // 2 and n_fb == n_fallback
    seen = np.zeros(N_GENES, dtype=int)
    _, want, _ = _pair_model()
    off = ~np.eye(len(SIZES), dtype=bool)
    for cols, got, skip in blocks:
        live = np.ones(len(cols), dtype=bool) if skip is None else skip == 0
        seen[cols[live]] += 1
        for k in range(4):
            a, w = got[k][:, :, live][off], want[k][:, :, cols[live]][off]
            if k == 1 or dtype == np.float32:
                assert np.array_equal(a, w, equal_nan=True), (k, fmt)
            else:
                np.testing.assert_allclose(a, w, rtol=1e-12, atol=0.0, equal_nan=True)
    assert (seen == 1).all()
    assert any(skip is None for _, _, skip in blocks) == bool(n_fallback)


@pytest.mark.parametrize("fmt", ["dense", "csc"])
def test_float64_input_through_the_fallback_gives_its_float32_twin_s_answer(fmt):
    """float64 values leave the ranked route: the flagged genes take one one-versus-reference call per reference, gathered on the device.
    The matrix holds float32 values exactly, so the tests are those of the float32 twin: U bit for bit; the routes agree on p, fold
    change and z to a relative 1e-12 among themselves (tests/test_gpu_pairwise_ranked.py), and so do the combinations, each being one
    such value times an exact factor of at most K - 1 (two roundings of 2^-53 more: 1.001e-12 covers them); U / (n_g n_rep) is exact."""
    for pval_type in ("any", "some", "all"):
        df = pairwise_markers(_adata(fmt, np.float64), False, "g", pval_type=pval_type)
        assert df.attrs["n_fallback_genes"] == N_GENES // 2 and df.attrs["n_ranked_genes"] == 0
        labels, want = _want_frame(pval_type)
        assert np.array_equal(np.asarray(df["reference"].astype(str)), want["reference"].reshape(-1))
        for col in ("statistic", "auc"):
            assert np.array_equal(df[col].to_numpy(), want[col].reshape(-1)), col
        for col, rtol in (("p_value", 1.001e-12), ("fold_change", 1e-12), ("z_score", 1e-12)):
            np.testing.assert_allclose(df[col].to_numpy(), want[col].reshape(-1), rtol=rtol, atol=0.0, equal_nan=True, err_msg=col)
