"""Per-group multiple-testing correction and top-n ranking on the device (illico_adjust_pvalues), against scipy / numpy on the host."""
import ctypes

import numpy as np
import pandas as pd
import pytest
from scipy import sparse, stats

from conftest import make_counts, make_labels
from illico_amd import AnnDataLite, adjust_pvalues, asymptotic_wilcoxon, differential_expression
from illico_amd._lib import ADJUST_LDS_COLS

pytestmark = pytest.mark.gpu

L = ADJUST_LDS_COLS
METHODS = ["bh", "by", "bonferroni"]


def _bits(a):
    return (np.asarray(a, dtype=np.float64) + 0.0).view(np.uint64)  # (+0.0: a zero's sign is not part of the contract)


def _want(p, method):
    if method == "bonferroni":
        return np.minimum(p * p.shape[1], 1.0)
    return stats.false_discovery_control(p, axis=1, method=method)


def _check(p, method, got, what=""):
    want = _want(p, method)
    if method == "by":
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0, err_msg=what)
    else:
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, f"{what} {method}: {bad.size} differ, first {np.unravel_index(bad[0], p.shape)}"


def _plane(dist, G, M, seed=0):
    rng = np.random.default_rng(seed)
    u = rng.random((G, M))
    if dist == "uniform":
        return u
    if dist == "u8":
        return u ** 8
    if dist == "round2":
        return np.round(u, 2)
    if dist == "ones":
        return np.ones((G, M))
    if dist == "zeros":
        return np.zeros((G, M))
    if dist == "subnormal":
        sub = rng.integers(0, 1 << 40, size=(G, M), dtype=np.uint64).view(np.float64)
        return np.where(u < 0.6, sub, u ** 4)
    if dist == "negzero":
        return np.where(u < 0.3, -0.0, u ** 4)
    if dist == "band":  # M distinct values 0.5 + k ulp: every key shares its high bits
        base = np.float64(0.5).view(np.uint64)
        return np.stack([(base + rng.permutation(M).astype(np.uint64)).view(np.float64) for _ in range(G)])
    if dist == "engine":  # like the engine's output: u**4 with a block of exact zeros and a row of 1.0
        p = u ** 4
        p[:, : max(1, M // 50)] = 0.0
        p[G // 2] = 1.0
        return p
    raise ValueError(dist)


DISTS = ["uniform", "u8", "round2", "ones", "zeros", "subnormal", "negzero", "band"]
SMALL = [(1, 1), (1, 2), (3, 7), (5, 255), (5, 256), (5, 257), (3, L - 1), (3, L), (3, L + 1)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dist", DISTS)
def test_adjust_matches_scipy_small(shape, dist):
    p = _plane(dist, *shape, seed=shape[1])
    for method in METHODS:
        _check(p, method, adjust_pvalues(p, method), f"{shape} {dist}")


@pytest.mark.parametrize("shape,dists", [
    ((2000, 8000), ["engine", "round2", "negzero"]),
    ((4, 120_000), ["engine", "round2", "subnormal", "band"]),
    ((2, 1_000_000), ["engine", "band"]),
    ((3, 3 * L + 5), ["band", "ones"]),
], ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else None)
def test_adjust_matches_scipy_large(shape, dists):
    import torch
    for dist in dists:
        p = _plane(dist, *shape, seed=7)
        pd_ = torch.from_numpy(p).cuda()
        for method in METHODS:
            got = adjust_pvalues(pd_, method).cpu().numpy()
            _check(p, method, got, f"{shape} {dist}")


@pytest.mark.parametrize("shape", [(3, 7), (5, 257), (3, L), (3, L + 1), (2000, 8000), (4, 120_000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_top_n_is_the_stable_argsort(shape):
    G, M = shape
    for dist in ("round2", "negzero", "engine"):
        p = _plane(dist, G, M, seed=3)
        order = np.argsort(p + 0.0, axis=1, kind="stable")
        for n in sorted({1, min(10, M), M}):
            for method in METHODS:
                adj, top = adjust_pvalues(p, method, n_top=n)
                assert top.dtype == np.int64 and top.shape == (G, n)
                np.testing.assert_array_equal(top, order[:, :n], err_msg=f"{shape} {dist} n={n} {method}")
                if n == M and method == "bh":
                    _check(p, method, adj, "with top-n")
    with pytest.raises(ValueError):
        adjust_pvalues(p, n_top=M + 1)


@pytest.mark.parametrize("M", [300, L + 500])
def test_residency_strides_and_in_place_give_identical_bytes(M):
    import torch
    from illico_amd._lib import get_engine
    G = 37
    p = _plane("round2", G, M, seed=11)
    ref, rtop = adjust_pvalues(p, "bh", n_top=25)
    _check(p, "bh", ref)
    dev, dtop = adjust_pvalues(torch.from_numpy(p).cuda(), "bh", n_top=25)
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(ref)) and np.array_equal(dtop.cpu().numpy(), rtop)
    wide = np.full((G, M + 13), 0.25)
    wide[:, 5:5 + M] = p
    view = wide[:, 5:5 + M]
    hv, htop = adjust_pvalues(view, "bh", n_top=25)
    assert np.array_equal(_bits(hv), _bits(ref)) and np.array_equal(htop, rtop)
    wd = torch.from_numpy(wide).cuda()
    dv, dvtop = adjust_pvalues(wd[:, 5:5 + M], "bh", n_top=25)
    assert np.array_equal(_bits(dv.cpu().numpy()), _bits(ref)) and np.array_equal(dvtop.cpu().numpy(), rtop)
    assert torch.equal(wd.cpu(), torch.from_numpy(wide))  # the input is not written
    eng = get_engine()
    hp = p.copy()
    out = eng.adjust_pvalues(hp, "bh", out=hp)
    assert out is hp and np.array_equal(_bits(hp), _bits(ref))
    dp = torch.from_numpy(wide).cuda()
    inner = dp[:, 5:5 + M]
    eng.adjust_pvalues(inner, "bh", out=inner)
    got = dp.cpu().numpy()
    assert np.array_equal(_bits(got[:, 5:5 + M]), _bits(ref))
    assert np.all(got[:, :5] == 0.25) and np.all(got[:, 5 + M:] == 0.25)


@pytest.mark.parametrize("bad", [np.nan, -1e-300, 1.0000000000000002, -np.inf])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("M", [10, L + 3])
def test_invalid_p_raises_naming_the_position(bad, where, M):
    import torch
    p = np.full((3, M), 0.5)
    p[1, 3] = bad
    p[2, 0] = bad  # (a later position: the first one is named)
    with pytest.raises(ValueError):
        stats.false_discovery_control(p, axis=1)
    x = p if where == "host" else torch.from_numpy(p).cuda()
    with pytest.raises(ValueError, match=r"row 1, column 3"):
        adjust_pvalues(x, "bh", n_top=2)
    if where == "device":  # in place on the device: nothing written
        from illico_amd._lib import get_engine
        x = torch.from_numpy(p).cuda()
        with pytest.raises(ValueError):
            get_engine().adjust_pvalues(x, "bh", out=x)
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(p))


def test_deferred_plane_is_completed_before_it_is_adjusted():
    import torch
    from illico_amd._lib import get_engine
    from illico_amd.utils.groups import encode_and_count_groups
    rng = np.random.RandomState(77)
    n, m, G = 20000, 640, 40
    means = np.exp(rng.normal(2.0, 1.8, size=m)).clip(0.05, 3000.0)
    X = rng.poisson(means, size=(n, m)).astype(np.float32)
    X[rng.rand(n, m) < 0.5] = 0
    assert (X.max(axis=0) > 255).sum() > 10  # genes the fused pass leaves to be recomputed later
    labels = make_labels(rng, n, G, n_ref=1500)
    _, g = encode_and_count_groups(groups=labels, ref_group="non-targeting")
    eng = get_engine()
    eng.set_groups(g)
    Xd = torch.from_numpy(X).cuda()
    planes = tuple(torch.full((g.counts.size, m), -7.0, dtype=torch.float64, device=Xd.device) for _ in range(3))
    eng.run_dense(Xd, 0, m, out=planes, device_out=True, defer=True)
    adj, top = eng.adjust_pvalues(planes[0], "bh", n_top=20)   # no synchronize in between
    eng.synchronize()
    p = planes[0].cpu().numpy()
    assert np.all((p >= 0) & (p <= 1))
    want, wtop = eng.adjust_pvalues(p, "bh", n_top=20)
    assert np.array_equal(_bits(adj.cpu().numpy()), _bits(want)) and np.array_equal(top.cpu().numpy(), wtop)
    _check(p, "bh", want)


def test_torch_side_stream():
    import torch
    s = torch.cuda.Stream()
    torch.manual_seed(0)
    with torch.cuda.stream(s):
        p = torch.rand((300, 9000), dtype=torch.float64, device="cuda") ** 4
        p[:, :40] = 0.0
        adj, top = adjust_pvalues(p, "bh", n_top=50)
        a_cpu, t_cpu, p_cpu = adj.cpu(), top.cpu(), p.cpu()
    s.synchronize()
    pn = p_cpu.numpy()
    _check(pn, "bh", a_cpu.numpy(), "side stream")
    np.testing.assert_array_equal(t_cpu.numpy(), np.argsort(pn + 0.0, axis=1, kind="stable")[:, :50])
    adjust_pvalues(torch.zeros((1, 1), dtype=torch.float64, device="cuda"))  # (the shared engine back on the default stream)


@pytest.mark.parametrize("shape", [(2000, 8000), (4, 120_000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_runs_are_byte_identical(shape):
    import torch
    p = torch.from_numpy(_plane("round2", *shape, seed=5)).cuda()
    runs = [tuple(t.cpu().numpy().tobytes() for t in adjust_pvalues(p, "by", n_top=100)) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


def _matrix(fmt, X):
    return {"dense": X, "csc": sparse.csc_matrix(X), "csr": sparse.csr_matrix(X)}[fmt]


@pytest.mark.parametrize("fmt", ["dense", "csc", "csr"])
@pytest.mark.parametrize("reference", ["non-targeting", None], ids=["ovo", "ovr"])
@pytest.mark.parametrize("batch_size", ["auto", 64])
def test_differential_expression_end_to_end(fmt, reference, batch_size):
    X, rng = make_counts(21, 600, 300, 0.6)
    labels = make_labels(rng, 600, 7, n_ref=120)
    adata = AnnDataLite(_matrix(fmt, X), obs=pd.DataFrame({"pert": labels}))
    base = asymptotic_wilcoxon(adata, False, "pert", reference, batch_size=batch_size)
    df = differential_expression(adata, False, "pert", reference, batch_size=batch_size)
    assert list(df.columns) == ["p_value", "statistic", "fold_change", "p_value_adj"] and df["p_value_adj"].dtype == np.float64
    assert df.index.equals(base.index)
    for col in ("p_value", "statistic", "fold_change"):
        assert df[col].to_numpy().tobytes() == base[col].to_numpy().tobytes(), col
    G, M = len(set(labels)), 300
    p = base["p_value"].to_numpy().reshape(G, M)
    _check(p, "bh", df["p_value_adj"].to_numpy().reshape(G, M), "p_value_adj")
    if reference is not None:  # the reference group's row: p all 1.0, adjusted all 1.0
        ref_row = sorted(set(labels)).index(reference)
        assert np.all(p[ref_row] == 1.0) and np.all(df["p_value_adj"].to_numpy().reshape(G, M)[ref_row] == 1.0)
    top = differential_expression(adata, False, "pert", reference, batch_size=batch_size, n_genes=5, corr_method="bonferroni")
    order = np.argsort(p + 0.0, axis=1, kind="stable")[:, :5]
    rows = (np.arange(G)[:, None] * M + order).reshape(-1)
    assert top.index.equals(base.index[rows])
    assert top["p_value"].to_numpy().tobytes() == base["p_value"].to_numpy()[rows].tobytes()
    np.testing.assert_array_equal(top["p_value_adj"].to_numpy(), np.minimum(p * M, 1.0).reshape(-1)[rows])
    assert list(top.index.get_level_values("pert").unique()) == list(base.index.get_level_values("pert").unique())


def test_cabi_argument_errors_and_profile():
    from illico_amd import _lib
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.illico_ctx_create(0, ctypes.byref(ctx)) == 0
    try:
        p = _plane("round2", 4, 10)
        adj, top = np.empty((4, 10)), np.empty((4, 3), np.int64)
        P, A, T = p.ctypes.data, adj.ctypes.data, top.ctypes.data
        E = _lib.ERR_ARG
        f = lib.illico_adjust_pvalues
        assert f(None, P, 4, 10, 10, 0, 0, A, 10, 3, T, 3) == E
        assert f(ctx, None, 4, 10, 10, 0, 0, A, 10, 3, T, 3) == E       # null p
        assert f(ctx, P, 4, 10, 9, 0, 0, A, 10, 3, T, 3) == E           # in_ld < width
        assert f(ctx, P, 4, 10, 10, 0, 0, A, 9, 3, T, 3) == E           # out_ld < width
        assert f(ctx, P, 4, 10, 10, 0, 0, A, 10, 3, T, 2) == E          # top_ld < n_top
        assert f(ctx, P, 4, 10, 10, 0, 0, A, 10, 11, T, 11) == E        # n_top > n_cols
        assert f(ctx, P, 4, 10, 10, 0, 0, A, 10, -1, T, 3) == E         # n_top < 0
        assert f(ctx, P, 4, 10, 10, 0, 0, A, 10, 3, None, 3) == E       # null out_top
        assert f(ctx, P, 4, 10, 10, 0, 0, None, 10, 0, None, 1) == E    # nothing to compute
        assert f(ctx, P, 4, 10, 10, 3, 0, A, 10, 3, T, 3) == E          # unknown method
        assert f(ctx, P, -1, 10, 10, 0, 0, A, 10, 3, T, 3) == E         # negative shape
        assert f(ctx, P, 4, 10, 10, 0, 0, P, 12, 3, T, 3) == E          # in place with another pitch
        bad = p.copy()
        bad[2, 7] = np.nan
        assert f(ctx, bad.ctypes.data, 4, 10, 10, 0, 0, A, 10, 3, T, 3) == E
        assert b"row 2, column 7" in lib.illico_last_error(ctx)
        assert lib.illico_ctx_set_option(ctx, b"profile", 1) == 0
        assert lib.illico_profile_reset(ctx) == 0
        assert f(ctx, P, 4, 10, 10, 0, 0, A, 10, 3, T, 3) == 0
        _check(p, "bh", adj)
        assert f(ctx, P, 4, 10, 10, 2, 0, A, 10, 0, None, 1) == 0        # Bonferroni: elementwise
        _check(p, "bonferroni", adj)
        assert f(ctx, P, 4, 10, 10, 0, 0, None, 10, 3, T, 3) == 0        # top-n only
        np.testing.assert_array_equal(top, np.argsort(p, axis=1, kind="stable")[:, :3])
        big = _plane("engine", 2, L + 100)
        bout = np.empty_like(big)
        assert f(ctx, big.ctypes.data, 2, L + 100, L + 100, 0, 0, bout.ctypes.data, L + 100, 0, None, 1) == 0
        _check(big, "bh", bout)
        seen = {}
        for k in range(lib.illico_profile_num_kernels()):
            ms, n = ctypes.c_double(), ctypes.c_int64()
            assert lib.illico_profile_get(ctx, k, ctypes.byref(ms), ctypes.byref(n)) == 0
            if n.value:
                seen[lib.illico_profile_kernel_name(k).decode()] = n.value
        for name in ("k_adj_validate", "k_adj_sort_lds", "k_adj_bonferroni", "k_adj_merge", "k_adj_scan"):
            assert name in seen, seen
        z = np.empty((0, 10))
        assert f(ctx, z.ctypes.data, 0, 10, 10, 0, 0, A, 10, 0, None, 1) == 0   # no rows: nothing written
    finally:
        lib.illico_ctx_destroy(ctx)
