"""Per-group non-zero counts and exact value sums on the device (illico_group_stats_*), against numpy / math.fsum on the host.

The sums are exact-limb sums: for the data below (every value within 2^-59 of its column's largest magnitude) they are the correctly
rounded sum, i.e. math.fsum bit for bit, and identical bytes across formats and runs.  Under is_log1p the device's expm1 may differ
from numpy's by an ulp of each value, so those sums are held to rtol 1e-12 against the host (and still to identical bytes across
formats)."""
import itertools
import math

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

from conftest import make_counts, make_labels
from illico_amd import AnnDataLite, asymptotic_wilcoxon, differential_expression, group_statistics
from illico_amd._lib import get_engine
from illico_amd.utils.groups import encode_and_count_groups

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.int64]


def _groups(codes_or_labels, ref=None):
    _, g = encode_and_count_groups(groups=np.asarray(codes_or_labels), ref_group=ref)
    return g


def _values(X, log1p):
    """What the sums add: float64 of X, or expm1 taken in X's dtype (float32 stays float32, ints become float64)."""
    if not log1p:
        return np.asarray(X, dtype=np.float64)
    return np.expm1(X).astype(np.float64) if X.dtype == np.float32 else np.expm1(X.astype(np.float64))


def _want(X, codes, G, log1p, exact=True):
    V = _values(X, log1p)
    nz = X != 0
    nnz = np.stack([nz[codes == g].sum(axis=0) for g in range(G)]).astype(np.int64)
    if exact:
        s = np.array([[math.fsum(V[codes == g, j][nz[codes == g, j]]) for j in range(X.shape[1])] for g in range(G)])
        r = np.array([[math.fsum(V[codes != g, j][nz[codes != g, j]]) for j in range(X.shape[1])] for g in range(G)])
    else:
        s = np.stack([np.where(nz[codes == g], V[codes == g], 0).sum(axis=0) for g in range(G)])
        r = np.stack([np.where(nz[codes != g], V[codes != g], 0).sum(axis=0) for g in range(G)])
    return nnz, s, nnz.sum(axis=0)[None, :] - nnz, r


def _bits(a):
    return (np.asarray(a, dtype=np.float64) + 0.0).view(np.uint64)


def _host(planes):
    return tuple(p if isinstance(p, np.ndarray) else (None if p is None else p.cpu().numpy()) for p in planes)


def _check(got, want, what, exact=True, rtol=1e-12, atol=None):
    got = _host(got)
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"nnz {what}")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"nnz_rest {what}")
    for k in (1, 3):
        if exact:
            bad = np.flatnonzero(_bits(got[k]) != _bits(want[k]))
            assert bad.size == 0, f"{what} plane {k}: {bad.size} differ, first {got[k].flat[bad[0]]!r} vs {want[k].flat[bad[0]]!r}"
        else:
            np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=atol or 0.0, err_msg=f"plane {k} {what}")


def _all_formats(eng, X, lb, ub, log1p, dev_out=False):
    """(name, planes) of every input layout of the same matrix, host and device input."""
    import torch
    Xs_c, Xs_r = sparse.csc_matrix(X), sparse.csr_matrix(X)
    Xd = torch.from_numpy(X).cuda()
    kw = dict(is_log1p=log1p, rest=True)
    G, W = eng.n_groups, ub - lb

    def outs():
        if not dev_out:
            return None
        return (torch.empty((G, W), dtype=torch.int64, device="cuda"), torch.empty((G, W), dtype=torch.float64, device="cuda"),
                torch.empty((G, W), dtype=torch.int64, device="cuda"), torch.empty((G, W), dtype=torch.float64, device="cuda"))
    res = [("dense host", eng.group_stats(X, lb, ub, out=outs(), **kw)),
           ("dense device", eng.group_stats(Xd, lb, ub, out=outs(), **kw))]
    for name, M in (("csc", Xs_c), ("csr", Xs_r)):
        res.append((f"{name} host", eng.group_stats_sparse(name, M.data, M.indices, M.indptr, M.shape, lb, ub, out=outs(), **kw)))
        dd = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (M.data, M.indices, M.indptr)]
        res.append((f"{name} device", eng.group_stats_sparse(name, *dd, M.shape, lb, ub, out=outs(), **kw)))
        b = eng.bind_sparse(name, M.data, M.indices, M.indptr, M.shape)
        res.append((f"{name} bound", b.group_stats(lb, ub, out=outs(), device_out=dev_out, **kw)))
        b.release()
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("log1p", [False, True])
@pytest.mark.parametrize("dev_out", [False, True])
def test_every_layout_matches_fsum(dtype, log1p, dev_out):
    X, rng = make_counts(11, 700, 70, 0.6, np.float32)
    X = X.astype(dtype)
    if log1p and dtype in (np.float32, np.float64):
        X = np.log1p(X).astype(dtype)
    elif log1p:
        X = np.minimum(X, 12)                   # expm1 of larger integers spans more than the 83 bits of the limbs
    X[:, 3] = 0                                 # an empty column
    codes = rng.randint(0, 7, size=700)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    want = _want(X, codes, 7, log1p)
    for lb, ub in ((0, 70), (5, 33)):
        w = tuple(p[:, lb:ub] for p in want)
        got = _all_formats(eng, X, lb, ub, log1p, dev_out)
        for name, planes in got:
            _check(planes, w, f"{name} {np.dtype(dtype)} log1p={log1p} dev_out={dev_out} [{lb}, {ub})", exact=not log1p)
        first = _host(got[0][1])
        for name, planes in got[1:]:  # identical bytes across layouts
            for a, b in zip(first, _host(planes)):
                assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)), name


def test_null_planes_in_every_combination():
    import torch
    X, rng = make_counts(3, 400, 40, 0.5)
    codes = rng.randint(0, 5, size=400)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    want = _want(X, codes, 5, False)
    Xd = torch.from_numpy(X).cuda()
    for mask in itertools.product([False, True], repeat=4):
        if not any(mask):
            continue
        host = tuple(np.full((5, 40), -1, dtype=(np.int64, np.float64)[k % 2]) if m else None for k, m in enumerate(mask))
        dev = tuple(torch.full((5, 40), -1, dtype=(torch.int64, torch.float64)[k % 2], device="cuda") if m else None for k, m in enumerate(mask))
        for got in (eng.group_stats(X, 0, 40, out=host), eng.group_stats(Xd, 0, 40, out=dev)):
            got = _host(got)
            for k in range(4):
                if mask[k]:
                    assert np.array_equal(np.asarray(got[k]).view(np.uint64), np.asarray(want[k]).view(np.uint64)), (mask, k)
                else:
                    assert got[k] is None


def test_window_with_wide_pitch_and_strided_dense():
    X, rng = make_counts(5, 500, 90, 0.5)
    wide = np.zeros((500, 130), np.float32)
    wide[:, :90] = X
    Xv = wide[:, :90]                                       # ld = 130 > n_cols
    codes = rng.randint(0, 6, size=500)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    want = _want(X, codes, 6, False)
    planes = (np.full((6, 200), -1, np.int64), np.full((6, 200), np.nan), np.full((6, 200), -1, np.int64), np.full((6, 200), np.nan))
    out = tuple(p[:, 7:7 + 50] for p in planes)             # out_ld = 200 > width
    eng.group_stats(Xv, 20, 70, rest=True, out=out)
    _check(out, tuple(p[:, 20:70] for p in want), "window")
    assert (planes[0][:, :7] == -1).all() and (planes[0][:, 57:] == -1).all() and np.isnan(planes[1][:, 57:]).all()


def test_continuous_negative_zeros_and_unsorted_rows():
    import torch
    rng = np.random.default_rng(9)
    n, m = 900, 60
    X = np.exp(rng.normal(0, 2, size=(n, m)))
    X[rng.random((n, m)) < 0.5] *= -1                        # mixed sign
    X[rng.random((n, m)) < 0.3] = 0.0
    X[rng.random((n, m)) < 0.05] = -0.0                      # negative zeros do not count
    codes = rng.integers(0, 8, size=n)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    absum = np.abs(X).sum(axis=0)
    tol = 1e-12 * absum
    M = sparse.csr_matrix(X)
    M.data[::7] = 0.0                                        # explicit stored zeros: not counted
    Xz = M.toarray()
    want = _want(Xz, codes, 8, False, exact=False)
    # rows of the CSR matrix in a shuffled column order
    data, ind = M.data.copy(), M.indices.copy()
    for r in range(n):
        a, b = M.indptr[r], M.indptr[r + 1]
        p = rng.permutation(b - a)
        data[a:b], ind[a:b] = M.data[a:b][p], M.indices[a:b][p]
    got_r = eng.group_stats_sparse("csr", data, ind, M.indptr, M.shape, 0, m, rest=True)
    C = sparse.csc_matrix(M)
    got_c = eng.group_stats_sparse("csc", C.data, C.indices, C.indptr, C.shape, 0, m, rest=True)
    got_d = eng.group_stats(torch.from_numpy(Xz).cuda(), 0, m, rest=True)
    for name, got in (("csr unsorted", got_r), ("csc", got_c), ("dense", got_d)):
        got = _host(got)
        np.testing.assert_array_equal(got[0], want[0], err_msg=name)
        np.testing.assert_array_equal(got[2], want[2], err_msg=name)
        assert (np.abs(got[1] - want[1]) <= tol).all() and (np.abs(got[3] - want[3]) <= tol).all(), name
        for a, b in zip(_host(got_r), got):
            assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)), name
    # CSC entries permuted within each column, and a repeated call: the same bytes
    cd, ci = C.data.copy(), C.indices.copy()
    for j in range(m):
        a, b = C.indptr[j], C.indptr[j + 1]
        p = rng.permutation(b - a)
        cd[a:b], ci[a:b] = C.data[a:b][p], C.indices[a:b][p]
    for got in (eng.group_stats_sparse("csc", cd, ci, C.indptr, C.shape, 0, m, rest=True),
                eng.group_stats_sparse("csc", C.data, C.indices, C.indptr, C.shape, 0, m, rest=True)):
        for a, b in zip(_host(got_c), _host(got)):
            assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_single_group_and_dominant_group_cancellation():
    rng = np.random.default_rng(4)
    n, m = 3000, 20
    X = rng.normal(0, 1, size=(n, m)) * 1e6
    X[:, 0] = 1.0
    eng = get_engine()
    eng.set_groups(_groups(np.zeros(n, dtype=int)))
    nnz, s, nr, sr = eng.group_stats(X, 0, m, rest=True)
    assert (nr == 0).all() and (sr == 0).all() and np.array_equal(nnz, (X != 0).sum(axis=0)[None])
    codes = np.where(rng.random(n) < 0.99, 0, 1 + rng.integers(0, 3, size=n))  # one group holds 99 % of the cells
    codes[:4] = [0, 1, 2, 3]
    X[codes == 0] += 5e7                                     # ... and nearly all the mass
    eng.set_groups(_groups(codes))
    want = _want(X, codes, 4, False)
    got = eng.group_stats(X, 0, m, rest=True)
    absum = np.stack([np.abs(X[codes != g]).sum(axis=0) for g in range(4)])
    np.testing.assert_array_equal(got[0], want[0])
    assert (np.abs(got[3] - want[3]) <= 1e-12 * absum).all()
    np.testing.assert_allclose(got[3][1:], want[3][1:], rtol=1e-12)


def test_non_finite_values_give_numpy_sums():
    X = np.arange(1, 9 * 6 + 1, dtype=np.float64).reshape(9, 6) / 10.0
    codes = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2])
    X[0, 0] = np.nan
    X[3, 1] = np.inf
    X[4, 2], X[5, 2] = np.inf, -np.inf
    X[6, 3] = -np.inf
    X[7, 4] = 800.0                                          # expm1 overflows under log1p
    eng = get_engine()
    eng.set_groups(_groups(codes))
    for log1p in (False, True):
        V = _values(X, log1p) if log1p else X
        with np.errstate(over="ignore", invalid="ignore"):
            ws = np.stack([V[codes == g].sum(axis=0) for g in range(3)])
            wr = np.stack([V[codes != g].sum(axis=0) for g in range(3)])
        for name, got in (("dense", eng.group_stats(X, 0, 6, is_log1p=log1p, rest=True)),
                          ("csc", eng.group_stats_sparse("csc", *(lambda c: (c.data, c.indices, c.indptr, c.shape))(sparse.csc_matrix(X)), 0, 6, is_log1p=log1p, rest=True)),
                          ("csr", eng.group_stats_sparse("csr", *(lambda c: (c.data, c.indices, c.indptr, c.shape))(sparse.csr_matrix(X)), 0, 6, is_log1p=log1p, rest=True))):
            np.testing.assert_array_equal(got[0], np.stack([(X[codes == g] != 0).sum(axis=0) for g in range(3)]))
            np.testing.assert_allclose(got[1], ws, rtol=1e-12, equal_nan=True, err_msg=f"{name} {log1p}")
            np.testing.assert_allclose(got[3], wr, rtol=1e-12, equal_nan=True, err_msg=f"{name} {log1p}")
            assert np.array_equal(np.isnan(got[1]), np.isnan(ws)) and np.array_equal(np.isinf(got[3]), np.isinf(wr))


def test_thirty_thousand_groups_of_ten():
    rng = np.random.default_rng(2)
    G, n, m = 30000, 300000, 24
    codes = rng.permutation(np.repeat(np.arange(G), 10))
    M = sparse.random(n, m, density=0.2, format="csc", random_state=3, dtype=np.float32)
    M.data = np.ceil(M.data * 20).astype(np.float32)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    X = M.toarray()
    nz = X != 0
    order = np.argsort(codes, kind="stable")
    want_n = np.add.reduceat(nz[order].astype(np.int64), np.arange(0, n, 10), axis=0)
    want_s = np.add.reduceat(X[order].astype(np.float64), np.arange(0, n, 10), axis=0)  # integers: exact in float64
    tot_s = X.astype(np.float64).sum(axis=0)
    R = sparse.csr_matrix(X)
    for name, got in (("csc", eng.group_stats_sparse("csc", M.data, M.indices, M.indptr, M.shape, 0, m, rest=True)),
                      ("csr", eng.group_stats_sparse("csr", R.data, R.indices, R.indptr, R.shape, 0, m, rest=True))):
        np.testing.assert_array_equal(got[0], want_n, err_msg=name)
        np.testing.assert_array_equal(got[1], want_s, err_msg=name)
        np.testing.assert_array_equal(got[2], want_n.sum(axis=0)[None] - want_n, err_msg=name)
        np.testing.assert_array_equal(got[3], tot_s[None] - want_s, err_msg=name)


def test_ten_clusters_of_100k_cells():
    import torch
    n, m = 1_000_000, 64
    rng = np.random.default_rng(5)
    codes = rng.permutation(np.repeat(np.arange(10), n // 10))
    X, _ = make_counts(8, n, m, 0.7)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    nz = X != 0
    want_n = np.stack([nz[codes == g].sum(axis=0) for g in range(10)])
    want_s = np.stack([X[codes == g].astype(np.float64).sum(axis=0) for g in range(10)])  # integers < 2^53: exact
    R = sparse.csr_matrix(X)
    for name, got in (("dense", eng.group_stats(torch.from_numpy(X).cuda(), 0, m, rest=True)),
                      ("csr", eng.group_stats_sparse("csr", R.data, R.indices, R.indptr, R.shape, 0, m, rest=True))):
        got = _host(got)
        np.testing.assert_array_equal(got[0], want_n, err_msg=name)
        np.testing.assert_array_equal(got[1], want_s, err_msg=name)
        np.testing.assert_array_equal(got[3], want_s.sum(axis=0)[None] - want_s, err_msg=name)


def test_wide_matrix():
    X, rng = make_counts(6, 100, 120000, 0.8)
    codes = rng.randint(0, 4, size=100)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    want_n = np.stack([(X[codes == g] != 0).sum(axis=0) for g in range(4)])
    want_s = np.stack([X[codes == g].astype(np.float64).sum(axis=0) for g in range(4)])
    C, R = sparse.csc_matrix(X), sparse.csr_matrix(X)
    for name, got in (("dense", eng.group_stats(X, 0, 120000)),
                      ("csc", eng.group_stats_sparse("csc", C.data, C.indices, C.indptr, C.shape, 0, 120000)),
                      ("csr", eng.group_stats_sparse("csr", R.data, R.indices, R.indptr, R.shape, 0, 120000))):
        np.testing.assert_array_equal(got[0], want_n, err_msg=name)
        np.testing.assert_array_equal(got[1], want_s, err_msg=name)


def test_sum_matches_rank_statistics_value_sum():
    X, rng = make_counts(12, 1500, 50, 0.5)
    labels = make_labels(rng, 1500, 9, n_ref=300)
    g = _groups(labels, "non-targeting")
    eng = get_engine()
    eng.set_groups(g)
    for log1p in (False, True):
        _, _, vsum = eng.rank_statistics(X, 0, 50, is_log1p=log1p)
        _, s = eng.group_stats(X, 0, 50, is_log1p=log1p)
        np.testing.assert_allclose(s, vsum.T, rtol=1e-12, atol=0)


def test_means_give_the_fold_change():
    X, rng = make_counts(13, 2000, 40, 0.6)
    X[:, 2] = 0
    labels = make_labels(rng, 2000, 8, n_ref=300)
    X[labels == "non-targeting", 5] = 0                     # reference mean 0: fold change inf
    adata = AnnDataLite(X, obs=pd.DataFrame({"pert": labels}))
    for ref in ("non-targeting", None):
        for log1p in (False, True):
            w = asymptotic_wilcoxon(adata, is_log1p=log1p, group_keys="pert", reference=ref)
            s = group_statistics(adata, "pert", ref, is_log1p=log1p)
            assert s.index.equals(w.index)
            mr = s["mean_reference"].to_numpy()
            with np.errstate(divide="ignore", invalid="ignore"):
                fc = s["mean_group"].to_numpy() / mr
            wfc = w["fold_change"].to_numpy()
            np.testing.assert_allclose(fc[mr != 0], wfc[mr != 0], rtol=1e-12, err_msg=f"{ref} {log1p}")
            assert np.isinf(wfc[mr == 0]).all()                  # (the fold change is inf wherever the reference mean is 0)
            if ref is not None:
                assert (mr.reshape(8, 40)[:, 5] == 0).all() and (mr == 0).sum() >= 2 * 8


def test_torch_side_stream_and_deferred_call():
    import torch
    X, rng = make_counts(14, 20000, 640, 0.5)
    labels = make_labels(rng, 20000, 40, n_ref=1500)
    g = _groups(labels, "non-targeting")
    eng = get_engine()
    eng.set_groups(g)
    codes = g.encoded_groups
    want = _want(X[:, :64], codes, 40, False, exact=False)
    Xd = torch.from_numpy(X).cuda()
    planes = tuple(torch.full((40, 640), -7.0, dtype=torch.float64, device="cuda") for _ in range(3))
    eng.run_dense(Xd, 0, 640, out=planes, device_out=True, defer=True)
    nnz, s = eng.group_stats(Xd, 0, 64)                       # completes the deferred call first
    eng.synchronize()
    np.testing.assert_array_equal(nnz.cpu().numpy(), want[0])
    np.testing.assert_array_equal(s.cpu().numpy(), want[1])
    p = planes[0].cpu().numpy()
    assert ((p >= 0) & (p <= 1)).all()                       # the deferred planes are complete
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Y = torch.from_numpy(X).cuda() * 2.0
        nnz2, s2, _, sr2 = eng.group_stats(Y, 0, 64, rest=True)
        a, b, c = nnz2.cpu(), s2.cpu(), sr2.cpu()
    side.synchronize()
    np.testing.assert_array_equal(a.numpy(), want[0])
    np.testing.assert_array_equal(b.numpy(), 2.0 * want[1])
    np.testing.assert_array_equal(c.numpy(), 2.0 * want[3])
    eng.group_stats(torch.zeros((20000, 1), device="cuda"), 0, 1)  # (the shared engine back on the default stream)


def _pandas_stats(X, labels, ref, log1p):
    V = _values(X, log1p)
    nz = pd.DataFrame((X != 0).astype(np.float64)).groupby(labels)
    vs = pd.DataFrame(V).groupby(labels)
    pct, mean = nz.mean(), vs.mean()
    cnt = pd.Series(labels).value_counts().sort_index()
    if ref is not None:
        pr, mr = np.tile(pct.loc[ref].to_numpy(), (len(pct), 1)), np.tile(mean.loc[ref].to_numpy(), (len(pct), 1))
    else:
        tot_n, tot_s = (X != 0).sum(axis=0), V.sum(axis=0)
        n_rest = (len(labels) - cnt.to_numpy())[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            pr = (tot_n[None] - nz.sum().to_numpy()) / n_rest
            mr = (tot_s[None] - vs.sum().to_numpy()) / n_rest
    return {"pct_group": pct.to_numpy().reshape(-1), "pct_reference": pr.reshape(-1), "mean_group": mean.to_numpy().reshape(-1),
            "mean_reference": mr.reshape(-1)}


@pytest.mark.parametrize("fmt", ["dense", "csc", "csr"])
@pytest.mark.parametrize("ref", ["non-targeting", None])
def test_public_api_matches_pandas(fmt, ref, tmp_path):
    X, rng = make_counts(15, 1200, 30, 0.6)
    labels = make_labels(rng, 1200, 6, n_ref=200)
    Xin = {"dense": X, "csc": sparse.csc_matrix(X), "csr": sparse.csr_matrix(X)}[fmt]
    for log1p in (False, True):
        if log1p:                                            # log-normalised values, as is_log1p means
            X = np.log1p(X)
            Xin = {"dense": X, "csc": sparse.csc_matrix(X), "csr": sparse.csr_matrix(X)}[fmt]
        adata = AnnDataLite(Xin, obs=pd.DataFrame({"pert": labels}))
        want = _pandas_stats(X, labels, ref, log1p)
        got = group_statistics(adata, "pert", ref, is_log1p=log1p)
        w = asymptotic_wilcoxon(adata, is_log1p=log1p, group_keys="pert", reference=ref)
        assert got.index.equals(w.index) and list(got.columns) == ["pct_group", "pct_reference", "mean_group", "mean_reference"]
        for k, v in want.items():
            np.testing.assert_allclose(got[k].to_numpy(), v, rtol=1e-12, err_msg=f"{k} {fmt} {ref} {log1p}")
        for n_genes in (None, 5):
            base = differential_expression(adata, log1p, "pert", ref, n_genes=n_genes)
            same = differential_expression(adata, log1p, "pert", ref, n_genes=n_genes, pts=False)
            pd.testing.assert_frame_equal(base, same, check_exact=True)
            de = differential_expression(adata, log1p, "pert", ref, n_genes=n_genes, pts=True)
            pd.testing.assert_frame_equal(de[base.columns], base, check_exact=True)
            pd.testing.assert_frame_equal(de[list(want)], got.loc[de.index], check_exact=True)
    if fmt == "dense":  # a streamed (file-backed) container, chunk by chunk
        mm = np.lib.format.open_memmap(tmp_path / "x.npy", mode="w+", dtype=np.float32, shape=X.shape)
        mm[:] = X
        mm.flush()
        back = np.load(tmp_path / "x.npy", mmap_mode="r")
        got = group_statistics(AnnDataLite(back, obs=pd.DataFrame({"pert": labels})), "pert", ref, is_log1p=True)
        pd.testing.assert_frame_equal(got, group_statistics(adata, "pert", ref, is_log1p=True), check_exact=True)


def test_single_group_ovr_reference_is_nan():
    X, _ = make_counts(16, 50, 8, 0.5)
    adata = AnnDataLite(X, obs=pd.DataFrame({"pert": ["a"] * 50}))
    s = group_statistics(adata, "pert", None, is_log1p=False)
    assert s["pct_reference"].isna().all() and s["mean_reference"].isna().all()
    np.testing.assert_allclose(s["pct_group"].to_numpy(), (X != 0).mean(axis=0), rtol=1e-12)


def test_full_size_c2_device_resident():
    import torch
    n, m, G = 300_000, 8000, 2000
    gen = torch.Generator(device="cuda").manual_seed(0)
    lam = torch.rand((1, m), device="cuda", generator=gen) * 6
    X = torch.poisson(lam.expand(n, m).contiguous(), generator=gen).to(torch.float32)
    X[torch.rand((n, m), device="cuda", generator=gen) < 0.5] = 0
    rng = np.random.default_rng(1)
    codes = rng.integers(0, G, size=n)
    codes[:G] = np.arange(G)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    nnz, s = eng.group_stats(X, 0, m)
    cols = np.arange(0, m, 64) + rng.integers(0, 64, size=m // 64)
    Xh = X[:, torch.from_numpy(cols).cuda()].cpu().numpy()
    del X
    torch.cuda.empty_cache()
    nnz, s = nnz.cpu().numpy()[:, cols], s.cpu().numpy()[:, cols]
    order = np.argsort(codes, kind="stable")
    starts = np.searchsorted(codes[order], np.arange(G))
    np.testing.assert_array_equal(nnz, np.add.reduceat((Xh[order] != 0).astype(np.int64), starts, axis=0))
    np.testing.assert_array_equal(s, np.add.reduceat(Xh[order].astype(np.float64), starts, axis=0))
