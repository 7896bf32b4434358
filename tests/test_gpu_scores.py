"""The z-score plane of the Wilcoxon routes (illico_run_*_ex) and top_by_score, against a float64 numpy restatement on the host."""
import numpy as np
import pandas as pd
import pytest
from scipy import sparse
from scipy.special import erfc

import oracle
from conftest import make_counts, make_labels
from illico_amd import AnnDataLite, asymptotic_wilcoxon, differential_expression, top_by_score
from threshold_cases import z_want

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(seed=5, n=700, m=70, G=6, n_ref=150):
    X, rng = make_counts(seed, n, m, 0.5)
    X[:, 3] = 4.0   # a constant column: z = 0
    X[:, 7] = 0.0   # an empty one
    labels = make_labels(rng, n, G, n_ref=n_ref)
    return X, labels


def _groups(labels, test):
    return oracle.encode_and_count_groups(labels, "non-targeting" if test == "ovo" else None)[1]


def _run(engine, fmt, X, **kw):
    M = X.shape[1]
    if fmt == "dense":
        return engine.run_dense(X, 0, M, scores=True, **kw)
    if fmt == "dense-device":
        import torch
        return tuple(t.cpu().numpy() for t in engine.run_dense(torch.from_numpy(X).cuda(), 0, M, scores=True, device_out=True, **kw))
    S = sparse.csc_matrix(X) if fmt == "csc" else sparse.csr_matrix(X)
    if fmt == "bound":
        bm = engine.bind_sparse("csr", S.data, S.indices, S.indptr, S.shape)
        try:
            return bm.run(0, M, scores=True, **kw)
        finally:
            bm.release()
    return engine.run_sparse(fmt, S.data, S.indices, S.indptr, S.shape, 0, M, scores=True, **kw)


@pytest.mark.parametrize("test", ["ovo", "ovr"])
@pytest.mark.parametrize("fmt", ["dense", "dense-device", "csc", "csr", "bound"])
@pytest.mark.parametrize("tie_correct", [True, False])
def test_z_plane_is_the_numpy_restatement_bit_for_bit(engine, test, fmt, tie_correct):
    X, labels = _data()
    g = _groups(labels, test)
    engine.set_groups(g)
    p, u, fc, z = _run(engine, fmt, X, tie_correct=tie_correct)
    want = z_want(X, g, u, tie_correct)
    assert np.array_equal(_bits(z), _bits(want)), f"{test} {fmt}: {np.count_nonzero(_bits(z) != _bits(want))} differ"
    assert np.all(z[:, 3] == 0.0) and np.all(z[:, 7] == 0.0)   # constant columns
    if test == "ovo":
        assert np.all(z[g.encoded_ref_group] == 0.0)           # the reference row
    # the three planes of the call are those of the call without z
    base = _run3(engine, fmt, X, tie_correct=tie_correct)
    for a, b in zip((p, u, fc), base):
        assert np.array_equal(_bits(a), _bits(b))


def _run3(engine, fmt, X, **kw):
    M = X.shape[1]
    if fmt in ("dense", "dense-device"):
        if fmt == "dense":
            return engine.run_dense(X, 0, M, **kw)
        import torch
        return tuple(t.cpu().numpy() for t in engine.run_dense(torch.from_numpy(X).cuda(), 0, M, device_out=True, **kw))
    S = sparse.csc_matrix(X) if fmt == "csc" else sparse.csr_matrix(X)
    if fmt == "bound":
        bm = engine.bind_sparse("csr", S.data, S.indices, S.indptr, S.shape)
        try:
            return bm.run(0, M, **kw)
        finally:
            bm.release()
    return engine.run_sparse(fmt, S.data, S.indices, S.indptr, S.shape, 0, M, **kw)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_dtypes_and_a_window_into_wider_planes(engine, dtype):
    X, labels = _data(seed=9)
    g = _groups(labels, "ovo")
    engine.set_groups(g)
    Xt = X.astype(dtype)
    G, M = g.counts.size, X.shape[1]
    wide = np.full((4, G, M + 20), -7.0)
    out = tuple(wide[k][:, 5:5 + 40] for k in range(4))
    engine.run_dense(Xt, 10, 50, out=out)
    want = z_want(X[:, 10:50], g, wide[1][:, 5:45])
    assert np.array_equal(_bits(wide[3][:, 5:45]), _bits(want))
    assert np.all(wide[:, :, :5] == -7.0) and np.all(wide[:, :, 45:] == -7.0)


ROUTES = {
    "fused": {},
    "two-pass": {"no_fused_path": 1},
    "sort": {"no_fused_path": 1, "no_counts_path": 1, "no_packed_dense": 1},
    "group-hists": {"group_hist_min_cells": 1},
    "batches": {"gene_batch": 64, "no_fused_path": 1},
}


def _heavy(seed=31, n=3000, m=200, G=8):
    rng = np.random.RandomState(seed)
    means = np.exp(rng.normal(1.5, 1.5, size=m)).clip(0.05, 400.0)
    X = rng.poisson(means, size=(n, m)).astype(np.float32)
    X[rng.rand(n, m) < 0.4] = 0
    assert (X.max(axis=0) > 63).sum() > 5   # genes the 64-value tables cannot take
    labels = np.array([f"c{i}" for i in rng.randint(0, G, size=n)])
    labels[:300] = "c0"   # one group above 255 cells
    return X, labels


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_same_bytes_on_every_route(engine, test):
    import torch
    X, labels = _heavy()
    g = oracle.encode_and_count_groups(labels, "c1" if test == "ovo" else None)[1]
    engine.set_groups(g)
    Xd = torch.from_numpy(X).cuda()
    M = X.shape[1]
    got = {}
    for name, opts in ROUTES.items():
        for k, v in opts.items():
            engine.set_option(k, v)
        engine.set_option("profile", 1)
        engine.profile_reset()
        try:
            got[name] = tuple(t.cpu().numpy() for t in engine.run_dense(Xd, 0, M, scores=True, device_out=True))
            prof = engine.profile_get()
        finally:
            engine.set_option("profile", 0)
            for k in opts:
                engine.set_option(k, {"group_hist_min_cells": 32768}.get(k, 0))
        if name == "fused":
            assert ("k_ovo_fused" if test == "ovo" else "k_ovr_fused") in prof or "k_group_value_hists" in prof, prof
        if name in ("two-pass", "sort", "batches"):
            assert "k_finalize_z" in prof and "k_finalize" not in prof, prof
        if name == "group-hists":
            assert "k_group_value_hists" in prof, prof
    got["host"] = engine.run_dense(X, 0, M, scores=True)
    S = sparse.csc_matrix(X)
    got["csc"] = engine.run_sparse("csc", S.data, S.indices, S.indptr, S.shape, 0, M, scores=True)
    R = sparse.csr_matrix(X)
    got["csr"] = engine.run_sparse("csr", R.data, R.indices, R.indptr, R.shape, 0, M, scores=True)
    want = z_want(X, g, got["fused"][1])
    for name, planes in got.items():
        assert np.array_equal(_bits(planes[3]), _bits(want)), name
        assert np.array_equal(_bits(planes[1]), _bits(got["fused"][1])), name


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_csr_counts_route_with_a_big_group(engine, test):
    rng = np.random.RandomState(503)
    sizes = [255, 120, 61, 33, 700, 256]
    labels = np.concatenate([[f"s{i:04d}"] * sz for i, sz in enumerate(sizes)])
    rng.shuffle(labels)
    n, m = labels.size, 300
    X = (rng.poisson(rng.uniform(0.3, 14.0, size=m), size=(n, m)) * (rng.rand(n, m) < 0.15)).astype(np.float32)
    g = oracle.encode_and_count_groups(labels, "s0000" if test == "ovo" else None)[1]
    engine.set_groups(g)
    R = sparse.csr_matrix(X)
    engine.set_option("profile", 1)
    engine.profile_reset()
    try:
        p, u, fc, z = engine.run_sparse("csr", R.data, R.indices, R.indptr, R.shape, 0, m, scores=True)
        prof = engine.profile_get()
    finally:
        engine.set_option("profile", 0)
    assert "k_csr_counts" in prof, prof
    assert np.array_equal(_bits(z), _bits(z_want(X, g, u)))


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_p_follows_z_without_continuity_for_every_alternative(engine, test):
    X, labels = _data(seed=13)
    g = _groups(labels, test)
    engine.set_groups(g)
    mask = np.arange(g.counts.size) != g.encoded_ref_group
    live = np.setdiff1d(np.arange(X.shape[1]), [3, 7])   # (outside the zero cases: the constant columns have p = 1, z = 0)
    zs = []
    for alt in ("two-sided", "greater", "less"):
        p, u, fc, z = engine.run_dense(X, 0, X.shape[1], use_continuity=False, alternative=alt, scores=True)
        zs.append(z)
        zz = z[mask][:, live]
        want = {"two-sided": erfc(np.abs(zz) / np.sqrt(2.0)), "greater": 0.5 * erfc(-zz / np.sqrt(2.0)),
                "less": 0.5 * erfc(zz / np.sqrt(2.0))}[alt]
        np.testing.assert_allclose(p[mask][:, live], want, rtol=1e-12, atol=0, err_msg=alt)
        assert np.all(p[:, [3, 7]] == 1.0) and np.all(z[:, [3, 7]] == 0.0)
        for log1p in (False, True):   # z does not depend on the options that shape p only
            z2 = engine.run_dense(X, 0, X.shape[1], alternative=alt, is_log1p=log1p, scores=True)[3]
            assert np.array_equal(_bits(z2), _bits(z))
    assert np.array_equal(_bits(zs[0]), _bits(zs[1])) and np.array_equal(_bits(zs[0]), _bits(zs[2]))


def test_deferred_call_completes_z_with_p(engine):
    import torch
    rng = np.random.RandomState(77)
    n, m, G = 20000, 640, 40
    means = np.exp(rng.normal(2.0, 1.8, size=m)).clip(0.05, 3000.0)
    X = rng.poisson(means, size=(n, m)).astype(np.float32)
    X[rng.rand(n, m) < 0.5] = 0
    labels = make_labels(rng, n, G, n_ref=1500)
    g = oracle.encode_and_count_groups(labels, "non-targeting")[1]
    engine.set_groups(g)
    Xd = torch.from_numpy(X).cuda()
    planes = tuple(torch.full((G, m), -7.0, dtype=torch.float64, device=Xd.device) for _ in range(4))
    engine.run_dense(Xd, 0, m, out=planes, device_out=True, defer=True)
    engine.synchronize()
    now = engine.run_dense(Xd, 0, m, scores=True, device_out=True)
    for a, b in zip(planes, now):
        assert torch.equal(a, b)


def test_rank_by_z_score_orders_underflowed_markers():
    rng = np.random.RandomState(3)
    n1 = n2 = 20000
    m = 40
    X = rng.poisson(3.0, size=(n1 + n2, m)).astype(np.float32)
    for k, j in enumerate(range(26, 40)):   # 14 strong markers of cluster A, stronger at higher columns
        X[:n1, j] = rng.poisson(6.0 + 0.8 * k, size=n1)
    labels = np.array(["A"] * n1 + ["B"] * n2)
    adata = AnnDataLite(X, obs=pd.DataFrame({"cl": labels}))
    base = asymptotic_wilcoxon(adata, False, "cl", None)
    full = differential_expression(adata, False, "cl", None, scores=True)
    assert list(full.columns)[-1] == "z_score" and full["z_score"].dtype == np.float64
    p = base["p_value"].to_numpy().reshape(2, m)
    z = full["z_score"].to_numpy().reshape(2, m)
    assert (p[0] == 0.0).sum() >= 12 and np.all(z[0, 26:] > 40) and np.unique(z[0, 26:]).size == 14
    by_z = differential_expression(adata, False, "cl", None, n_genes=10, rank_by="z_score")
    order_z = np.argsort(-z, axis=1, kind="stable")[:, :10]
    rows = (np.arange(2)[:, None] * m + order_z).reshape(-1)
    assert by_z.index.equals(base.index[rows])
    assert not np.array_equal(order_z[0], np.arange(26, 36))
    by_p = differential_expression(adata, False, "cl", None, n_genes=10)
    order_p = np.argsort(p + 0.0, axis=1, kind="stable")[:, :10]
    assert np.array_equal(order_p[0], np.arange(26, 36))   # column order among the p == 0 rows, as before
    assert by_p.index.equals(base.index[(np.arange(2)[:, None] * m + order_p).reshape(-1)])
    assert "z_score" not in by_p.columns


def _scores(G, M, seed=0):
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(0, 3, size=(G, M)), 1)   # many ties
    x[:, ::7] = 0.0
    x[:, 1::11] = -0.0
    x[0, min(2, M - 1)] = np.inf
    x[-1, -1] = -np.inf
    return x


@pytest.mark.parametrize("shape", [(3, 1), (5, 8192), (3, 8292), (2, 30000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_top_by_score_is_the_stable_argsort(shape):
    import torch
    G, M = shape
    x = _scores(G, M, seed=M)
    order = np.argsort(-(x + 0.0), axis=1, kind="stable")
    for n in sorted({1, min(10, M), M}):
        top = top_by_score(x, n)
        assert top.dtype == np.int64 and top.shape == (G, n)
        np.testing.assert_array_equal(top, order[:, :n], err_msg=f"{shape} n={n}")
        dtop = top_by_score(torch.from_numpy(x).cuda(), n)
        np.testing.assert_array_equal(dtop.cpu().numpy(), order[:, :n])


@pytest.mark.parametrize("where", ["host", "device"])
def test_top_by_score_refuses_nan(where):
    import torch
    x = np.zeros((3, 9000))
    x[1, 4] = np.nan
    x[2, 0] = np.nan
    xx = x if where == "host" else torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match=r"row 1, column 4"):
        top_by_score(xx, 5)
