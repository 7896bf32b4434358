"""All-pairs Welch t-tests on the device: Engine.pair_ttest_from_moments (illico_pair_ttest_from_moments) byte for byte against the
existing per-reference kernel (Engine.ttest_from_moments under each reference in turn) and, for the effect planes, against the numpy
model of tests/pair_ttest_model.py; pairwise_ttest against welch_ttest(reference=r); pairwise_markers(method="t-test") against
tests/markers_model.py applied to the pair planes.

No tolerance appears: t, df and p are held to the bits of k_ttest_from_moments (which DESIGN.md section 13 holds to scipy), the effect
planes to one IEEE operation per step.  The per-reference planes are computed once per (variant, alternative) on the widest plane and
shared: the test is column by column, so a narrower case is its first columns."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch
from scipy import sparse

from illico_amd import AnnDataLite, adjust_pvalues, pairwise_markers, pairwise_ttest, welch_ttest
from illico_amd import _lib
from illico_amd import pairwise as pairwise_mod
from illico_amd.utils.groups import encode_and_count_groups
from markers_model import combine_model
from pair_ttest_model import pair_model

pytestmark = pytest.mark.gpu

GENE_TILE, GROUP_TILE = _lib.PAIR_TT_GENE_TILE, _lib.PAIR_TT_GROUP_TILE   # kernels_pair_ttest.h: PT_TILE, PT_GT
SIZES = (1, 2, 3, 17, 40, 64, 200, 5, 9, 31)                              # G = 10: one above the group tile
G = len(SIZES)
WS = [1, GENE_TILE - 1, GENE_TILE, GENE_TILE + 1, 2 * GENE_TILE + 1]
WMAX = max(WS)
KS = [2, 3, GROUP_TILE - 1, GROUP_TILE, GROUP_TILE + 1, G]
SUBSET = [1, 3, 4, 6, 9]
VARIANTS = ("welch", "overestim_var")
ALTERNATIVES = ("two-sided", "less", "greater")
CONSTANT, ZERO, TWO_CONSTANTS = 0, 1, 2
SENTINEL = -7.25


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _engine():
    return _lib.get_engine()


@functools.lru_cache(maxsize=None)
def _problem():
    """(X float32 [372, WMAX] log-normalised, the group container, host planes S, Q, F (the expm1 sums), counts): column 0 constant,
    column 1 all zero, column 2 constant at 1.0 in group 3 and at 2.5 in group 4."""
    rng = np.random.default_rng(11)
    n = sum(SIZES)
    codes = rng.permutation(np.repeat(np.arange(G), SIZES))
    mu = rng.uniform(0.3, 12.0, WMAX) * (1.0 + 0.5 * rng.random((G, WMAX)))
    C = rng.poisson(mu[codes]).astype(np.float64)
    X = np.log1p(C / np.maximum(C.sum(axis=1, keepdims=True), 1.0) * 1e3).astype(np.float32)
    X[:, CONSTANT] = 1.5
    X[:, ZERO] = 0.0
    X[codes == 3, TWO_CONSTANTS] = 1.0
    X[codes == 4, TWO_CONSTANTS] = 2.5
    _, container = encode_and_count_groups(groups=pd.Series([f"g{c:02d}" for c in codes]), ref_group=None)
    container = container._replace(encoded_ref_group=-1)
    assert list(container.counts) == list(SIZES)
    eng = _engine()
    eng.set_groups(container)
    S, Q = eng.group_moments(X, 0, WMAX)
    F = eng.group_stats(X, 0, WMAX, is_log1p=True)[1]
    return X, container, S, Q, F, np.asarray(SIZES, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _per_reference(variant, alternative):
    """float64 [3, G, G, WMAX]: (p, t, df) of Engine.ttest_from_moments under the reference r, for every r -- the existing kernel."""
    _, container, S, Q, _, _ = _problem()
    eng = _engine()
    out = np.empty((3, G, G, WMAX))
    for r in range(G):
        eng.set_groups(container._replace(encoded_ref_group=r))
        for k, plane in enumerate(eng.ttest_from_moments(S, Q, variant=variant, alternative=alternative, want=("p", "t", "df"))):
            out[k, r] = plane
    eng.set_groups(container)
    return out


def _side(a, side):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if side == "device" else a


@pytest.mark.parametrize("side", ["device", "host"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_planes_equal_the_per_reference_kernel_byte_for_byte(variant, side):
    """p, t, df of every r: every W around the gene tile with all groups (views of the wider planes: in_ld > W), every K around the
    group tile and a strict subset at the full width; the three alternatives; outputs allocated, and given as views of wider blocks."""
    _, container, S, Q, _, _ = _problem()
    eng = _engine()
    eng.set_groups(container)
    Sd, Qd = _side(S, side), _side(Q, side)
    cases = [(np.arange(G), W) for W in WS] + [(np.arange(K), WMAX) for K in KS[:-1]] + [(np.asarray(SUBSET), WMAX)]
    for alternative in ALTERNATIVES:
        ref = _per_reference(variant, alternative)
        for sel, W in cases:
            want = ref[:, sel][:, :, sel][:, :, :, :W]
            got = eng.pair_ttest_from_moments(Sd[:, :W], Qd[:, :W], sel=sel, variant=variant, alternative=alternative, want=("p", "t", "df"))
            K = len(sel)
            for name, a, w in zip("p t df".split(), got, want):
                a = _host(a)
                assert a.shape == (K, K, W) and (side == "host" or got[0].is_cuda)
                bad = np.argwhere(_bits(a) != _bits(w))
                assert bad.size == 0, f"{variant} {alternative} K={K} W={W} {name}: {len(bad)} differ, first (r, g, j) = {bad[0]}: {a[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"
            d = np.arange(K)
            assert (_host(got[0])[d, d] == 1.0).all() and (_bits(_host(got[1])[d, d]) == 0).all()   # the reference-row rule: (t, p) = (+0, 1)
        # given outputs of a wider pitch, another order of want, a single plane: the columns beyond W stay as they were
        sel, W = np.asarray(SUBSET), GENE_TILE + 1
        full = [_side(np.full((len(sel), len(sel), W + 3), SENTINEL), side) for _ in range(2)]
        eng.pair_ttest_from_moments(Sd[:, :W], Qd[:, :W], sel=sel, variant=variant, alternative=alternative, want=("df", "p"),
                                    out=tuple(a[:, :, :W] for a in full))
        for a, k in zip(full, (2, 0)):
            a = _host(a)
            assert np.array_equal(_bits(a[:, :, :W]), _bits(ref[k][sel][:, sel][:, :, :W])) and (a[:, :, W:] == SENTINEL).all()


def test_special_columns_hold_what_the_issue_names():
    ref = _per_reference("welch", "two-sided")
    p, t = ref[0], ref[1]
    off = ~np.eye(G, dtype=bool)
    for col in (CONSTANT, ZERO):
        assert (p[:, :, col] == 1.0).all() and (t[:, :, col] == 0.0).all()
    assert t[3, 4, TWO_CONSTANTS] == np.inf and t[4, 3, TWO_CONSTANTS] == -np.inf and p[3, 4, TWO_CONSTANTS] == 0.0
    assert (p[0][1:] == 1.0).all() and (p[1:, 0] == 1.0).all()              # the one-cell group, on either side
    assert ((p[off][:, 3:] > 0) & (p[off][:, 3:] < 1)).mean() > 0.6         # and real tests elsewhere (a fifth of the pairs hold the one-cell group)


@pytest.mark.parametrize("side", ["device", "host"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_effect_planes_equal_the_model_byte_for_byte(variant, side):
    """fold change with and without fsum (the all-zero column: inf, on the diagonal too), Cohen's d (0 on the diagonal, NaN -> 0, inf
    kept), and t and df once more against the model's own arithmetic."""
    _, container, S, Q, F, counts = _problem()
    eng = _engine()
    eng.set_groups(container)
    Sd, Qd, Fd = (_side(a, side) for a in (S, Q, F))
    for sel in (np.arange(G), np.asarray(SUBSET)):
        for fsum, fd in ((None, None), (F, Fd)):
            M = pair_model(S, Q, counts, sel=sel, fsum=fsum, overestim=variant == "overestim_var")
            want = ("fold_change", "cohen_d", "t", "df")
            got = eng.pair_ttest_from_moments(Sd, Qd, sel=sel, fsum=fd, variant=variant, want=want)
            for name, a in zip(want, got):
                a = _host(a)
                bad = np.argwhere(_bits(a) != _bits(M[name]))
                assert bad.size == 0, f"{variant} K={len(sel)} fsum={fsum is not None} {name}: {len(bad)} differ, first {bad[0]}: {a[tuple(bad[0])]!r} != {M[name][tuple(bad[0])]!r}"
            fc, d = _host(got[0]), _host(got[1])
            k = np.arange(len(sel))
            assert np.isposinf(fc[:, :, ZERO]).all() and (fc[k, k, CONSTANT] == 1.0).all() and (_bits(d[k, k]) == 0).all()
    full = _host(eng.pair_ttest_from_moments(Sd, Qd, variant=variant, want=("cohen_d",))[0])
    assert np.isposinf(full[3, 4, TWO_CONSTANTS]) and np.isneginf(full[4, 3, TWO_CONSTANTS]) and (full[:, :, CONSTANT] == 0.0).all()


def test_host_planes_staged_in_several_windows():
    """A scratch budget that holds a few columns of a window: the same bytes."""
    _, container, S, Q, F, _ = _problem()
    want = ("p", "t", "df", "fold_change", "cohen_d")
    whole = _engine().pair_ttest_from_moments(S, Q, fsum=F, want=want)
    eng = _lib.Engine(0)
    try:
        eng.set_groups(container)
        eng.set_option("scratch_bytes", 200_000)   # G = 10: 3 * 80 + 5 * 800 bytes per column: 47 columns a window
        got = eng.pair_ttest_from_moments(S, Q, fsum=F, want=want)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, whole))
    finally:
        eng.close()


def test_the_library_s_own_refusals():
    _, container, S, Q, _, _ = _problem()
    eng = _engine()
    eng.set_groups(container)
    lib, W = eng.lib, 4
    out = np.full((G * G, W), SENTINEL)
    sel = np.arange(G, dtype=np.int32)

    def call(sel_a, K, in_ld=WMAX, out_ld=W, p=out.ctypes.data, variant=0, n_cols=W):
        return lib.illico_pair_ttest_from_moments(eng.h, S.ctypes.data, Q.ctypes.data, None, n_cols, in_ld, None if sel_a is None else sel_a.ctypes.data, K,
                                                  variant, 0, 0, p, None, None, None, None, out_ld)
    bad_order, twice, beyond = (np.array(a, dtype=np.int32) for a in ([1, 0, 2], [0, 0, 1], [0, 1, G]))
    for rc in (call(sel, 1), call(sel, 0), call(None, 3), call(bad_order, 3), call(twice, 3), call(beyond, 3), call(sel, G, p=None),
               call(sel, G, in_ld=W - 1), call(sel, G, out_ld=W - 1), call(sel, G, variant=2), call(sel, G, n_cols=-1)):
        assert rc == _lib.ERR_ARG
    assert (out == SENTINEL).all()
    assert call(sel, G) == _lib.OK and (out != SENTINEL).all()


# ---- the front end ----
N_CELLS, N_GENES, FRONT_SIZES = 300, 40, (100, 80, 60, 40, 20)
WIDE_GENES = 150   # three gene windows of 64


@functools.lru_cache(maxsize=None)
def _matrix(n_genes):
    rng = np.random.default_rng(23)
    codes = rng.permutation(np.repeat(np.arange(len(FRONT_SIZES)), FRONT_SIZES))
    mu = rng.uniform(0.3, 10.0, n_genes) * (1.0 + rng.random((len(FRONT_SIZES), n_genes)))
    C = rng.poisson(mu[codes]).astype(np.float64)
    X = np.log1p(C / np.maximum(C.sum(axis=1, keepdims=True), 1.0) * 1e3).astype(np.float32)
    X[:, 5] = 0.75   # a constant gene
    X[:, 6] = 0.0    # an all-zero gene: the fold change is inf
    return X, np.array([f"g{c}" for c in codes])


def _adata(fmt, n_genes=N_GENES):
    X, labels = _matrix(n_genes)
    Xc = {"dense": lambda a: a, "csr": sparse.csr_matrix, "csc": sparse.csc_matrix}[fmt](X)
    return AnnDataLite(Xc, obs=pd.DataFrame({"g": labels}))


def _frame_bytes(df):
    return b"".join(df[c].to_numpy().tobytes() for c in df.columns) + repr(list(df.index[:3]) + list(df.index[-3:])).encode()


@pytest.mark.parametrize("is_log1p", [False, True])
@pytest.mark.parametrize("fmt", ["dense", "csc", "csr"])
def test_frame_rows_equal_welch_ttest_per_reference(fmt, is_log1p):
    labels = sorted(set(_matrix(N_GENES)[1]))
    for variant, alternative, groups in (("welch", "two-sided", None), ("overestim_var", "greater", None), ("welch", "less", ["g4", "g0", "g2"])):
        df = pairwise_ttest(_adata(fmt), is_log1p, "g", groups=groups, variant=variant, alternative=alternative, corr_method="bh")
        chosen = labels if groups is None else sorted(groups)
        K = len(chosen)
        assert df.index.names == ["pert", "reference", "feature"] and len(df) == K * (K - 1) * N_GENES
        assert list(df.columns) == ["p_value", "statistic", "fold_change", "p_value_adj"]
        pos = 0
        for r in chosen:
            one = welch_ttest(_adata(fmt), is_log1p, "g", r, variant=variant, alternative=alternative)
            for g in chosen:
                if g == r:
                    continue
                rows, want = df.iloc[pos * N_GENES:(pos + 1) * N_GENES], one.loc[g]
                assert rows.index[0] == (g, r, "gene_0") and rows.index[-1] == (g, r, f"gene_{N_GENES - 1}")
                for col in ("p_value", "statistic", "fold_change"):
                    assert rows[col].to_numpy().tobytes() == want[col].to_numpy().tobytes(), (fmt, is_log1p, variant, g, r, col)
                adj = adjust_pvalues(np.ascontiguousarray(want["p_value"].to_numpy()[None, :]), "bh")
                assert rows["p_value_adj"].to_numpy().tobytes() == np.asarray(adj).tobytes()
                pos += 1
        assert np.isposinf(df["fold_change"].to_numpy().reshape(-1, N_GENES)[:, 6]).all()
    assert "p_value_adj" not in pairwise_ttest(_adata(fmt), is_log1p, "g").columns


@pytest.mark.parametrize("fmt", ["dense", "csc", "csr"])
def test_three_gene_windows_give_the_one_window_frame(fmt, monkeypatch):
    kw = dict(variant="welch", corr_method="bh")
    one = pairwise_ttest(_adata(fmt, WIDE_GENES), True, "g", **kw)
    marks = pairwise_markers(_adata(fmt, WIDE_GENES), True, "g", method="t-test")
    windows = []
    eng = _engine()
    inner = eng.pair_ttest_from_moments
    monkeypatch.setattr(eng, "pair_ttest_from_moments", lambda S, *a, **k: (windows.append(int(S.shape[1])), inner(S, *a, **k))[1])
    monkeypatch.setattr(pairwise_mod, "PAIR_WINDOW_BYTES", 64 * 1000)   # per gene 3 * 5 * 8 + 3 * 25 * 8 = 720 bytes: 88 genes -> 64 a window
    three = pairwise_ttest(_adata(fmt, WIDE_GENES), True, "g", **kw)
    assert windows == [64, 64, WIDE_GENES - 128]
    assert _frame_bytes(three) == _frame_bytes(one)
    del windows[:]
    marks3 = pairwise_markers(_adata(fmt, WIDE_GENES), True, "g", method="t-test")
    assert windows == [64, 64, WIDE_GENES - 128]
    assert _frame_bytes(marks3.drop(columns="reference")) == _frame_bytes(marks.drop(columns="reference"))
    assert list(marks3["reference"]) == list(marks["reference"])


def _pair_planes(fmt, is_log1p, variant, groups=None):
    """(labels, host planes dict name -> [K, K, M]) of pair_ttest_blocks with the marker planes, checked against pairwise_ttest's frame."""
    import sys
    from illico_amd.group_stats import _input
    from illico_amd.pairwise import _select
    from illico_amd.utils.registry import data_handler_registry
    pt = sys.modules["illico_amd.pairwise_ttest"]
    adata = _adata(fmt)
    X = _input(adata, None)
    uniq, container = encode_and_count_groups(groups=adata.obs["g"], ref_group=None)
    sel = _select(np.asarray(uniq), groups)
    K = int(sel.size)
    planes = {name: np.full((K, K, N_GENES), np.nan) for name in pt.MARKER_PLANES}
    seen = np.zeros(N_GENES, dtype=int)

    def sink(cols, block, skip):
        assert skip is None and all(q.is_cuda and q.dtype == torch.float64 and tuple(q.shape) == (K, K, len(cols)) for q in block)
        seen[cols] += 1
        for name, q in zip(pt.MARKER_PLANES, block):
            planes[name][:, :, cols] = q.cpu().numpy()

    pt.pair_ttest_blocks(X, data_handler_registry.get(X), container, sel, is_log1p, variant, "two-sided", pt.MARKER_PLANES, sink)
    assert (seen == 1).all()
    df = pairwise_ttest(adata, is_log1p, "g", groups=groups, variant=variant)
    off = ~np.eye(K, dtype=bool)
    for name, col in (("p", "p_value"), ("t", "statistic"), ("fold_change", "fold_change")):
        assert planes[name][off].tobytes() == df[col].to_numpy().tobytes()
    return [str(x) for x in np.asarray(uniq)[sel]], planes


@pytest.mark.parametrize("fmt", ["dense", "csc", "csr"])
def test_ttest_markers_equal_the_model_of_the_pair_planes(fmt):
    cases = [("t-test", "welch", pt, None, None) for pt in ("any", "some", "all")] + [("t-test_overestim_var", "overestim_var", "any", None, None),
                                                                                   ("t-test", "welch", "any", 5, None), ("t-test", "welch", "some", None, ["g3", "g0", "g4"])]
    for method, variant, pval_type, n_genes, groups in cases:
        labels, planes = _pair_planes(fmt, True, variant, groups=None if groups is None else tuple(groups))
        K = len(labels)
        p, rep, t, fc, dfree, d = combine_model(planes["p"], [planes[k] for k in ("t", "fold_change", "df", "cohen_d")], method=pval_type)
        df = pairwise_markers(_adata(fmt), True, "g", method=method, pval_type=pval_type, n_genes=n_genes, groups=groups)
        assert list(df.columns) == ["p_value", "p_value_adj", "reference", "statistic", "fold_change", "df", "cohen_d"] and not df.attrs
        assert df.index.names == ["pert", "feature"]
        rows = np.arange(K * N_GENES)
        if n_genes is not None:
            rows = (np.arange(K)[:, None] * N_GENES + np.argsort(p, axis=1, kind="stable")[:, :n_genes]).reshape(-1)
            assert list(df.index.get_level_values(1)) == [f"gene_{j % N_GENES}" for j in rows]
        assert len(df) == len(rows) and list(df.index.get_level_values(0)) == [labels[j // N_GENES] for j in rows]
        for col, w in (("p_value", p), ("statistic", t), ("fold_change", fc), ("df", dfree), ("cohen_d", d)):
            assert df[col].to_numpy().tobytes() == w.reshape(-1)[rows].tobytes(), (fmt, method, pval_type, col)
        assert isinstance(df["reference"].dtype, pd.CategoricalDtype)
        assert np.array_equal(np.asarray(df["reference"].astype(str)), np.array(labels)[rep].reshape(-1)[rows])
        adj = adjust_pvalues(np.ascontiguousarray(p), "benjamini-hochberg").reshape(-1)
        assert df["p_value_adj"].to_numpy().tobytes() == adj[rows].tobytes()
    assert "p_value_adj" not in pairwise_markers(_adata(fmt), True, "g", method="t-test", corr_method=None).columns


def test_the_default_method_is_the_wilcoxon_frame_it_was():
    """pairwise_markers() and method="wilcoxon" against combine_model over pairwise_wilcoxon(scores=True), as test_gpu_markers.py does."""
    from test_gpu_markers import _adata as markers_adata, _assert_frame, _want_frame
    for pval_type in ("any", "some", "all"):
        labels, want = _want_frame(pval_type)
        for kw in ({}, dict(method="wilcoxon")):
            df = pairwise_markers(markers_adata("dense"), False, "g", pval_type=pval_type, **kw)
            assert list(df.columns) == ["p_value", "p_value_adj", "reference", "statistic", "fold_change", "z_score", "auc"]
            _assert_frame(df, labels, want)
            adj = adjust_pvalues(np.ascontiguousarray(want["p_value"]), "benjamini-hochberg")
            assert np.array_equal(df["p_value_adj"].to_numpy(), adj.reshape(-1)) and "n_flagged_genes" in df.attrs
