"""Welch's t-test on the device: exact per-group moments (illico_group_moments_*), t / df from them (illico_ttest_from_moments),
Student's t tail (illico_student_t_pvalues), and welch_ttest / differential_expression(method=...) end to end.

The moments are exact-limb sums: math.fsum bit for bit where every value and square is held exactly, and identical bytes across
layouts and runs always.  t and df are held to the bits of the numpy restatement in tests/test_ttest_host.py; the tail to scipy's."""
import numpy as np
import pandas as pd
import pytest
from scipy import sparse, stats

from conftest import make_counts
from illico_amd import AnnDataLite, asymptotic_wilcoxon, differential_expression, welch_ttest
from illico_amd import _lib
from illico_amd._lib import get_engine
from illico_amd.utils.groups import encode_and_count_groups
from test_ttest_host import fsum_moments, lognorm_nb, welch_numpy

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.int64]
#: groups held in LDS by the CSC moments kernel (kernels_group_moments.h: GM_CSC_LDS_G); beyond, global atomics
CSC_LDS_GROUPS = 2048
#: columns per workgroup of the CSR moments kernel (GM_CSR_CW)
CSR_WINDOW = 2048


def _groups(codes_or_labels, ref=None):
    _, g = encode_and_count_groups(groups=np.asarray(codes_or_labels), ref_group=ref)
    return g


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _host(planes):
    return tuple(p if isinstance(p, np.ndarray) else (None if p is None else p.cpu().numpy()) for p in planes)


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    bad = np.flatnonzero(_bits(a).reshape(-1) != _bits(b).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {a.flat[bad[0]]!r} vs {b.flat[bad[0]]!r}"


def _want_moments(X, codes, G):
    """(sum, sumsq, sum_rest, sumsq_rest) by math.fsum over the float64 values and their float64 squares"""
    V = np.asarray(X, dtype=np.float64)
    own = [fsum_moments(V, codes == g) for g in range(G)]
    rest = [fsum_moments(V, codes != g) for g in range(G)]
    return (np.stack([o[0] for o in own]), np.stack([o[1] for o in own]), np.stack([r[0] for r in rest]), np.stack([r[1] for r in rest]))


def _all_layouts(eng, X, lb, ub, dev_out=False):
    """(name, planes) of every input layout of the same matrix: dense host / device, CSC and CSR as host, device and bound"""
    import torch
    Xd = torch.from_numpy(X).cuda()
    G, W = eng.n_groups, ub - lb

    def outs():
        return tuple(torch.empty((G, W), dtype=torch.float64, device="cuda") for _ in range(4)) if dev_out else None
    res = [("dense host", eng.group_moments(X, lb, ub, rest=True, out=outs())),
           ("dense device", eng.group_moments(Xd, lb, ub, rest=True, out=outs()))]
    for name, M in (("csc", sparse.csc_matrix(X)), ("csr", sparse.csr_matrix(X))):
        res.append((f"{name} host", eng.group_moments_sparse(name, M.data, M.indices, M.indptr, M.shape, lb, ub, rest=True, out=outs())))
        dd = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (M.data, M.indices, M.indptr)]
        res.append((f"{name} device", eng.group_moments_sparse(name, *dd, M.shape, lb, ub, rest=True, out=outs())))
        b = eng.bind_sparse(name, M.data, M.indices, M.indptr, M.shape)
        res.append((f"{name} bound", b.group_moments(lb, ub, rest=True, out=outs(), device_out=dev_out)))
        b.release()
    return res


# ---- 1. exact values: math.fsum bit for bit in every layout ---------------------------------------------------------------------
_SIZES = (1, 2, 63, 1024, 1025, 485)    # 1025: two chunks, the atomic path; 2600 cells


def _exact_case(dtype):
    rng = np.random.default_rng(21)
    n, m = sum(_SIZES), 300              # 300 genes: a ragged second 256-gene tile
    if np.dtype(dtype).kind == "f":
        X = (rng.integers(-512, 513, size=(n, m)) / 64.0).astype(dtype)     # k / 64: every square is exact in float64
    else:
        X = rng.integers(0, 4096, size=(n, m)).astype(dtype)
    X[rng.random((n, m)) < 0.7] = 0
    codes = rng.permutation(np.repeat(np.arange(len(_SIZES)), _SIZES))
    return X, codes


_exact_cache = {}


def _exact(dtype):
    key = np.dtype(dtype).name
    if key not in _exact_cache:
        X, codes = _exact_case(dtype)
        _exact_cache[key] = (X, codes, _want_moments(X, codes, len(_SIZES)))
    return _exact_cache[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dev_out", [False, True])
def test_moments_are_fsum_in_every_layout(dtype, dev_out):
    X, codes, want = _exact(dtype)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    for lb, ub in ((0, 300), (37, 290)):
        got = _all_layouts(eng, X, lb, ub, dev_out)
        for name, planes in got:
            planes = _host(planes)
            for k, what in enumerate(("sum", "sumsq", "sum_rest", "sumsq_rest")):
                _same_bits(planes[k], want[k][:, lb:ub], f"{what} {name} {np.dtype(dtype)} dev_out={dev_out} [{lb}, {ub})")


# ---- 2. continuous float32 values --------------------------------------------------------------------------------------------------
def test_continuous_float32_sumsq_and_identical_bytes():
    C, rng = make_counts(8, 2600, 300, 0.7)
    X = np.log1p(C * np.float32(0.37)).astype(np.float32)
    codes = rng.permutation(np.repeat(np.arange(len(_SIZES)), _SIZES))
    eng = get_engine()
    eng.set_groups(_groups(codes))
    want = _want_moments(X, codes, len(_SIZES))
    runs = [_all_layouts(eng, X, 0, 300), _all_layouts(eng, X, 0, 300)]
    first = _host(runs[0][0][1])
    # one rounding of the total plus n 2^-83 of truncation; the sums of the values themselves are exact (float32 within 2^-59 of the largest)
    for k in (0, 2):
        _same_bits(first[k], want[k], f"plane {k}")
    for k in (1, 3):
        np.testing.assert_allclose(first[k], want[k], rtol=1e-13, atol=0.0)
    for run in runs:
        for name, planes in run:
            for k, p in enumerate(_host(planes)):
                _same_bits(p, first[k], f"{name} plane {k}")


# ---- 3. route edges of the sparse kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [CSC_LDS_GROUPS, CSC_LDS_GROUPS + 4])
def test_csc_group_limit(G):
    import torch
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 4, size=G)                      # 1 - 3 cells per group
    codes = rng.permutation(np.repeat(np.arange(G), sizes))
    n, m = codes.size, 40
    X = (rng.integers(-512, 513, size=(n, m)) / 64.0).astype(np.float32)
    X[rng.random((n, m)) < 0.7] = 0
    eng = get_engine()
    eng.set_groups(_groups(codes))
    V = X.astype(np.float64)
    S, Q = np.zeros((G, m)), np.zeros((G, m))
    np.add.at(S, codes, V)                                  # (exact: multiples of 1 / 64 and 1 / 4096 far below 2^53)
    np.add.at(Q, codes, V * V)
    want = (S, Q, S.sum(axis=0)[None] - S, Q.sum(axis=0)[None] - Q)
    M = sparse.csc_matrix(X)
    got_c = eng.group_moments_sparse("csc", M.data, M.indices, M.indptr, M.shape, 0, m, rest=True)
    got_d = eng.group_moments(torch.from_numpy(X).cuda(), 0, m, rest=True)
    for name, got in (("csc", got_c), ("dense", got_d)):
        for k, p in enumerate(_host(got)):
            _same_bits(p, want[k], f"{name} G={G} plane {k}")


def test_csr_window_edge_unsorted_rows_and_a_duplicate():
    rng = np.random.default_rng(6)
    n, m = 700, CSR_WINDOW + 2                              # one column past the window
    X = (rng.integers(-512, 513, size=(n, m)) / 64.0).astype(np.float32)
    X[rng.random((n, m)) < 0.9] = 0
    X[5, m - 1] = 3.25
    X[9, CSR_WINDOW] = -1.5
    codes = rng.integers(0, 5, size=n)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    M = sparse.csr_matrix(X)
    data, ind, ptr = M.data.copy(), M.indices.copy(), M.indptr.copy()
    for r in range(n):                                      # rows in a shuffled column order
        a, b = ptr[r], ptr[r + 1]
        p = rng.permutation(b - a)
        data[a:b], ind[a:b] = M.data[a:b][p], M.indices[a:b][p]
    # one duplicate entry: row 5 stores column m - 1 a second time (value 0.75); the dense equivalent holds both as separate values
    at = ptr[6]
    data, ind = np.insert(data, at, np.float32(0.75)), np.insert(ind, at, m - 1)
    ptr[6:] += 1
    V = X.astype(np.float64)
    want = list(_want_moments(V, codes, 5))
    g5 = codes[5]
    for g in range(5):
        own = g == g5
        want[0 if own else 2][g, m - 1] += 0.75
        want[1 if own else 3][g, m - 1] += 0.75 * 0.75
    got = _host(eng.group_moments_sparse("csr", data, ind, ptr, (n, m), 0, m, rest=True))
    for k in range(4):
        _same_bits(got[k], want[k], f"plane {k}")
    got = _host(eng.group_moments_sparse("csr", data, ind, ptr, (n, m), 3, m, rest=True))
    for k in range(4):
        _same_bits(got[k], want[k][:, 3:], f"window plane {k}")


def test_host_matrix_in_three_column_windows():
    X, codes, want = _exact(np.float32)
    G, (n, m) = len(_SIZES), X.shape
    eng = _lib.Engine(get_engine().device)                  # (a context of its own: the shared engine keeps its scratch cap)
    try:
        eng.set_groups(_groups(codes))
        # per column: 48 G + 64 bytes of planes, 4 staged output planes, the staged rows (group_moments.hip: gm_run)
        per_col = G * 48 + 64 + G * 8 * 4 + n * 4
        eng.set_option("scratch_bytes", per_col * 120)      # 300 columns -> windows of 120, 120, 60
        got = _host(eng.group_moments(X, 0, m, rest=True))
        M = sparse.csc_matrix(X)
        eng.set_option("scratch_bytes", (G * 48 + 64 + G * 8 * 4) * 120)
        got_c = _host(eng.group_moments_sparse("csc", M.data, M.indices, M.indptr, M.shape, 0, m, rest=True))
    finally:
        eng.close()
    for k in range(4):
        _same_bits(got[k], want[k], f"dense plane {k}")
        _same_bits(got_c[k], want[k], f"csc plane {k}")


# ---- 4. non-finite and extreme values -----------------------------------------------------------------------------------------------
def test_non_finite_and_extreme_values():
    import torch
    rng = np.random.default_rng(12)
    n, m, G = 400, 12, 4
    X = rng.normal(0, 1, size=(n, m))
    X[rng.random((n, m)) < 0.4] = 0.0
    codes = rng.integers(0, G, size=n)
    row = {g: int(np.flatnonzero(codes == g)[0]) for g in range(G)}
    X[row[0], 1] = np.nan
    X[row[1], 2] = np.inf
    X[row[2], 3] = -np.inf
    X[:, 4] = 0.0
    X[row[3], 4], X[row[0], 4] = 2e154, 1e154                # finite, the first one's square is not: the squares' scale is the second's
    X[:, 8] = 0.0
    X[row[3], 8] = 1e200
    X[:, 5] = -0.0
    X[row[0], 6], X[row[1], 6] = np.inf, -np.inf             # both infinities in one column, different groups
    X[row[2], 7] = 1e-200                                    # a square that underflows
    eng = get_engine()
    eng.set_groups(_groups(codes))
    with np.errstate(all="ignore"):
        S = np.stack([X[codes == g].sum(axis=0) for g in range(G)])
        Q = np.stack([(X[codes == g] ** 2).sum(axis=0) for g in range(G)])
        SR = np.stack([X[codes != g].sum(axis=0) for g in range(G)])
        QR = np.stack([(X[codes != g] ** 2).sum(axis=0) for g in range(G)])
    M_c, M_r = sparse.csc_matrix(X), sparse.csr_matrix(X)
    layouts = [("dense", eng.group_moments(X, 0, m, rest=True)), ("dense device", eng.group_moments(torch.from_numpy(X).cuda(), 0, m, rest=True)),
               ("csc", eng.group_moments_sparse("csc", M_c.data, M_c.indices, M_c.indptr, M_c.shape, 0, m, rest=True)),
               ("csr", eng.group_moments_sparse("csr", M_r.data, M_r.indices, M_r.indptr, M_r.shape, 0, m, rest=True))]
    first = _host(layouts[0][1])
    for name, got in layouts:
        got = _host(got)
        for k, want in enumerate((S, Q, SR, QR)):
            nf = ~np.isfinite(want)
            assert np.array_equal(np.isnan(got[k]), np.isnan(want)), (name, k)
            assert np.array_equal(got[k][nf & ~np.isnan(want)], want[nf & ~np.isnan(want)]), (name, k)   # +inf / -inf as numpy's
            np.testing.assert_allclose(got[k][~nf], want[~nf], rtol=1e-12, atol=1e-11, err_msg=f"{name} {k}")
            _same_bits(got[k], first[k], f"{name} plane {k}")
    assert np.isnan(first[0][0, 1]) and np.isnan(first[1][0, 1]) and np.isnan(first[2][1, 1])
    assert first[0][1, 2] == np.inf and first[1][1, 2] == np.inf and first[0][2, 3] == -np.inf and first[1][2, 3] == np.inf
    assert first[0][3, 4] == 2e154 and first[1][3, 4] == np.inf and first[1][0, 4] == 1e154 * 1e154 and first[3][0, 4] == np.inf
    assert first[0][3, 8] == 1e200 and first[1][3, 8] == np.inf and first[1][0, 8] == 0.0 and first[2][0, 8] == 1e200
    assert (first[0][:, 5] == 0).all() and (first[1][:, 5] == 0).all()
    assert np.isnan(first[2][2, 6]) and first[2][0, 6] == -np.inf and first[1][0, 6] == np.inf
    # the t-test of those cells: (0, 1) wherever t is NaN, nothing else NaN
    p, t = eng.ttest_from_moments(*first)
    tn, *_ = welch_numpy(np.bincount(codes)[:, None], first[0], first[1], (n - np.bincount(codes))[:, None], first[2], first[3])
    assert np.isnan(tn[0, 1]) and np.isnan(tn[1, 2]) and np.isnan(tn[3, 8]) and np.isnan(tn[:, 5]).all()
    assert not np.isnan(p).any() and not np.isnan(t).any()
    assert (t[np.isnan(tn)] == 0).all() and (p[np.isnan(tn)] == 1).all()
    _same_bits(t[~np.isnan(tn)], tn[~np.isnan(tn)], "t")


# ---- 5. t and df: the bits of the numpy restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [None, "g3"])
@pytest.mark.parametrize("variant", ["welch", "overestim_var"])
def test_t_and_df_bits(ref, variant):
    X, rng = lognorm_nb(17, 900, 64)
    sizes = (1, 2, 300, 250, 347)
    labels = rng.permutation(np.repeat([f"g{k}" for k in range(5)], sizes))
    X[:, 0] = np.float32(1.25)                               # a constant gene
    X[labels == "g2", 1] = np.float32(0.5)                   # constant in one group only
    X[labels == "g2", 2], X[labels != "g2", 2] = np.float32(2.0), np.float32(1.0)   # no variance anywhere, different means: t = +inf
    g = _groups(labels, ref)
    eng = get_engine()
    eng.set_groups(g)
    codes, counts, r = g.encoded_groups, np.asarray(g.counts), int(g.encoded_ref_group)
    mom = eng.group_moments(X, 0, 64, rest=True)
    S, Q, SR, QR = mom
    n1 = counts[:, None].astype(np.float64)
    if ref is None:
        n2, S2, Q2 = 900.0 - n1, SR, QR
    else:
        n2, S2, Q2 = np.full_like(n1, float(counts[r])), np.broadcast_to(S[r], S.shape), np.broadcast_to(Q[r], Q.shape)
    tn, dfn, m1, v1, m2, v2 = welch_numpy(n1, S, Q, n2, S2, Q2, overestim=variant == "overestim_var")
    want = ("p", "t", "df", "mean", "var", "mean_ref", "var_ref")
    args = mom if ref is None else mom[:2]
    p, t, df, gm1, gv1, gm2, gv2 = eng.ttest_from_moments(*args, variant=variant, want=want)
    nan = np.isnan(tn)
    if ref is not None:
        nan[r] = True                                        # the reference row: (0, 1)
    assert nan[0].all() and nan[:, 0].all()                  # the one-cell group, the constant gene
    assert (t[nan] == 0).all() and (p[nan] == 1).all()
    _same_bits(t[~nan], tn[~nan], "t")
    _same_bits(df, dfn, "df")
    for a, b, what in ((gm1, m1, "mean"), (gm2, np.broadcast_to(m2, m1.shape), "mean_ref")):
        _same_bits(a, b, what)
    for a, b, what in ((gv1, v1, "var"), (gv2, np.broadcast_to(v2, v1.shape), "var_ref")):
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        _same_bits(a[~np.isnan(a)], b[~np.isnan(b)], what)
    k2 = list(g.counts).index(300)
    if ref is None or k2 != r:
        assert t[k2, 2] == np.inf and p[k2, 2] == 0.0 and df[k2, 2] == 1.0
    assert not nan[1, 3:].any()                              # the two-cell group is tested
    # device planes in, device planes out: the same bytes
    import torch
    dm = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args)
    for a, b in zip(_host(eng.ttest_from_moments(*dm, variant=variant, want=want)), (p, t, df, gm1, gv1, gm2, gv2)):
        assert np.array_equal(_bits(np.nan_to_num(a, nan=-7.0)), _bits(np.nan_to_num(b, nan=-7.0)))
    # scipy from the same statistics (std -> square costs a few ulps)
    ok = ~nan & np.isfinite(tn)
    n2p = n1 if variant == "overestim_var" else n2
    with np.errstate(all="ignore"):
        sc = stats.ttest_ind_from_stats(m1, np.sqrt(v1), n1, np.broadcast_to(m2, m1.shape), np.sqrt(np.broadcast_to(v2, v1.shape)),
                                        np.broadcast_to(n2p, m1.shape), equal_var=False)
        a, b = v1 / n1, np.broadcast_to(v2, v1.shape) / n2p
        sc_df = (a + b) ** 2 / (a ** 2 / (n1 - 1) + b ** 2 / (n2p - 1))
    np.testing.assert_allclose(t[ok], sc.statistic[ok], rtol=1e-13, atol=0.0)
    np.testing.assert_allclose(df[ok], sc_df[ok], rtol=1e-13, atol=0.0)
    ok &= sc.pvalue >= 1e-300
    np.testing.assert_allclose(p[ok], sc.pvalue[ok], rtol=1e-9, atol=0.0)


# ---- 6. Student's t tail against scipy -----------------------------------------------------------------------------------------------
TAIL_BANDS = ((1, 10), (10, 1e2), (1e2, 1e3), (1e3, 1e4), (1e4, 1e5), (1e5, 1e6), (1e6, 4.2e6))
#: the worst relative deviation from scipy.stats.t.sf per band, measured on an MI355X
TAIL_MEASURED = (5.4e-15, 4.1e-14, 1.1e-13, 2.5e-13, 4.1e-13, 3.8e-13, 3.3e-13)
TAIL_T = np.array([1e-6, 1e-3, 0.05, 0.3, 0.9, 1.1, 1.7, 2.5, 3, 4, 6, 9, 13, 20, 30, 37, 50, 80, 150, 400])


def tail_grid():
    rng = np.random.default_rng(1)
    return [np.exp(rng.uniform(np.log(lo), np.log(hi), 40)) for lo, hi in TAIL_BANDS]


def tail_deviation(eng, df):
    """(worst relative deviation where scipy's p >= 1e-300, the p planes by alternative) of one band's df draws x TAIL_T x both signs"""
    D, T = np.meshgrid(df, np.concatenate([TAIL_T, -TAIL_T]), indexing="ij")
    worst, planes = 0.0, {}
    for alt in ("two-sided", "greater", "less"):
        got = eng.student_t_pvalues(T, D, alternative=alt)
        ref = {"two-sided": 2.0 * stats.t.sf(np.abs(T), D), "greater": stats.t.sf(T, D), "less": stats.t.sf(-T, D)}[alt]
        assert not np.isnan(got).any(), alt
        assert ((got >= 0) & (got <= 1)).all(), alt
        big = ref >= 1e-300
        assert (got[~big] <= 1e-299).all(), alt
        print(f"tail {alt}: worst {np.max(np.abs(got[big] - ref[big]) / ref[big]):.3e}")
        worst = max(worst, float(np.max(np.abs(got[big] - ref[big]) / ref[big])))
        planes[alt] = got
    return worst, planes


@pytest.mark.parametrize("band", range(len(TAIL_BANDS)))
def test_student_t_tail_against_scipy(band):
    tol = max(1e-12, 4.0 * TAIL_MEASURED[band])
    assert tol <= 1e-9                                       # anything worse is a defect, not rounding
    eng = get_engine()
    worst, planes = tail_deviation(eng, tail_grid()[band])
    print(f"band {TAIL_BANDS[band]}: worst relative deviation {worst:.3e} (tolerance {tol:.3e})")
    nt = TAIL_T.size
    two = planes["two-sided"]
    assert (np.diff(two[:, :nt], axis=1) <= 0).all()         # non-increasing in |t| along each df
    assert np.array_equal(two[:, :nt], two[:, nt:])          # symmetric
    assert np.array_equal(planes["greater"][:, :nt], planes["less"][:, nt:])
    assert worst <= tol


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------
def _e2e_data():
    X, rng = lognorm_nb(29, 1500, 120)
    X[rng.random(X.shape) < 0.3] = 0
    sizes = (2, 40, 300, 458, 500, 200)
    labels = rng.permutation(np.repeat([f"c{k}" for k in range(6)], sizes))
    return X, labels


def _scipy_ttest(V, labels, ref, variant, alternative):
    names = sorted(set(labels))
    t, p = np.zeros((len(names), V.shape[1])), np.ones((len(names), V.shape[1]))
    for k, g in enumerate(names):
        if g == ref:
            continue
        a, b = V[labels == g], (V[labels == ref] if ref is not None else V[labels != g])
        if variant == "welch":
            r = stats.ttest_ind(a, b, axis=0, equal_var=False, alternative=alternative)
        else:
            r = stats.ttest_ind_from_stats(a.mean(axis=0), a.std(axis=0, ddof=1), a.shape[0], b.mean(axis=0), b.std(axis=0, ddof=1), a.shape[0],
                                           equal_var=False, alternative=alternative)
        t[k], p[k] = r.statistic, r.pvalue
    return t, p


@pytest.mark.parametrize("ref", [None, "c4"])
@pytest.mark.parametrize("is_log1p", [False, True])
def test_welch_ttest_end_to_end(ref, is_log1p):
    X, labels = _e2e_data()
    obs = pd.DataFrame({"cl": labels})
    V = X.astype(np.float64)
    containers = {"dense": X, "csc": sparse.csc_matrix(X), "csr": sparse.csr_matrix(X)}
    wil = asymptotic_wilcoxon(AnnDataLite(X, obs=obs), is_log1p, "cl", ref)
    n_nan = n_all = 0
    first = None
    for variant in ("welch", "overestim_var"):
        for alternative in ("two-sided", "greater", "less"):
            st, sp = _scipy_ttest(V, labels, ref, variant, alternative)
            for name, M in containers.items():
                df = welch_ttest(AnnDataLite(M, obs=obs), is_log1p, "cl", ref, variant=variant, alternative=alternative)
                assert list(df.columns) == ["p_value", "statistic", "fold_change"] and df.index.equals(wil.index)
                t, p = df["statistic"].to_numpy().reshape(6, 120), df["p_value"].to_numpy().reshape(6, 120)
                nan = np.isnan(st)
                n_nan, n_all = n_nan + int(nan.sum()), n_all + nan.size
                assert (t[nan] == 0).all() and (p[nan] == 1).all()
                np.testing.assert_allclose(t[~nan], st[~nan], rtol=1e-12, atol=0.0, err_msg=f"t {name} {variant} {alternative}")
                big = ~nan & (sp >= 1e-30)
                np.testing.assert_allclose(p[big], sp[big], rtol=1e-8, atol=0.0, err_msg=f"p {name} {variant} {alternative}")
                np.testing.assert_allclose(df["fold_change"].to_numpy(), wil["fold_change"].to_numpy(), rtol=1e-12, atol=0.0, equal_nan=True)
                if (variant, alternative) == ("welch", "two-sided"):
                    if first is None:
                        first = df
                    else:
                        pd.testing.assert_frame_equal(df, first)   # the containers give identical bytes
    assert n_nan < 0.01 * n_all


@pytest.mark.parametrize("method,variant", [("t-test", "welch"), ("t-test_overestim_var", "overestim_var")])
def test_differential_expression_with_a_ttest_method(method, variant):
    X, labels = _e2e_data()
    adata = AnnDataLite(sparse.csr_matrix(X), obs=pd.DataFrame({"cl": labels}))
    base = welch_ttest(adata, True, "cl", None, variant=variant)
    df = differential_expression(adata, True, "cl", None, method=method, pts=True)
    pd.testing.assert_frame_equal(df[["p_value", "statistic", "fold_change"]], base)
    p = df["p_value"].to_numpy().reshape(6, 120)
    np.testing.assert_array_equal(df["p_value_adj"].to_numpy().reshape(6, 120), stats.false_discovery_control(p, axis=1))
    from illico_amd import group_statistics
    gs = group_statistics(adata, "cl", None, is_log1p=True)
    pd.testing.assert_frame_equal(df[list(gs.columns)], gs)
    top = differential_expression(adata, True, "cl", None, method=method, n_genes=10, rank_by="statistic")
    t = df["statistic"].to_numpy().reshape(6, 120)
    order = np.argsort(-(t + 0.0), axis=1, kind="stable")[:, :10]
    rows = (np.arange(6)[:, None] * 120 + order).reshape(-1)
    pd.testing.assert_frame_equal(top, df.drop(columns=list(gs.columns)).iloc[rows])
    by_p = differential_expression(adata, True, "cl", None, method=method, n_genes=10)
    order = np.argsort(p + 0.0, axis=1, kind="stable")[:, :10]
    pd.testing.assert_frame_equal(by_p, df.drop(columns=list(gs.columns)).iloc[(np.arange(6)[:, None] * 120 + order).reshape(-1)])


def test_method_wilcoxon_is_todays_frame():
    X, labels = _e2e_data()
    adata = AnnDataLite(X, obs=pd.DataFrame({"cl": labels}))
    for kw in (dict(), dict(n_genes=7, rank_by="z_score"), dict(pts=True, scores=True, alternative="greater")):
        pd.testing.assert_frame_equal(differential_expression(adata, True, "cl", "c4", method="wilcoxon", **kw),
                                      differential_expression(adata, True, "cl", "c4", **kw))


@pytest.mark.parametrize("kind", ["h5-dense", "backed-csc"])
def test_streamed_containers_are_read_chunk_by_chunk(tmp_path, monkeypatch, kind):
    import sys
    from illico_amd.utils.registry import H5pyBackedCSCDataHandler, H5pyDatasetDataHandler, data_handler_registry
    from test_gpu_out_of_core import FakeBackedCSC, FakeH5Dataset
    X, labels = _e2e_data()
    obs = pd.DataFrame({"cl": labels})
    want = welch_ttest(AnnDataLite(X, obs=obs), True, "cl", None)
    cls, handler = (FakeH5Dataset, H5pyDatasetDataHandler) if kind == "h5-dense" else (FakeBackedCSC, H5pyBackedCSCDataHandler)
    monkeypatch.setattr(sys.modules["illico_amd.asymptotic_wilcoxon"], "STREAM_CHUNK_BYTES", 1500 * 4 * 50)   # 50 genes per chunk
    ds = cls(tmp_path / "x.backed", X)
    data_handler_registry[cls] = handler                     # what h5py.Dataset / anndata's _CSCDataset are registered under
    try:
        got = welch_ttest(AnnDataLite(ds, obs=obs), True, "cl", None)
    finally:
        data_handler_registry.pop(cls, None)
    assert ds.reads == [(0, 50), (50, 100), (100, 120)]      # one read per chunk for both passes, in order
    pd.testing.assert_frame_equal(got, want)


# ---- 8. streams and a deferred call ----------------------------------------------------------------------------------------------------
def test_torch_side_stream_and_deferred_call():
    import torch
    X, codes, want = _exact(np.float32)
    G = len(_SIZES)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    Xd = torch.from_numpy(np.abs(X)).cuda()
    planes = tuple(torch.full((G, 300), -7.0, dtype=torch.float64, device="cuda") for _ in range(3))
    eng.run_dense(Xd, 0, 300, out=planes, device_out=True, defer=True)
    s, q = eng.group_moments(torch.from_numpy(X).cuda(), 0, 64)     # completes the deferred call first
    eng.synchronize()
    _same_bits(s.cpu().numpy(), want[0][:, :64], "sum")
    _same_bits(q.cpu().numpy(), want[1][:, :64], "sumsq")
    p = planes[0].cpu().numpy()
    assert ((p >= 0) & (p <= 1)).all()                               # the deferred planes are complete
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Y = torch.from_numpy(X).cuda() * 2.0
        mom = eng.group_moments(Y, 0, 64, rest=True)
        pt = eng.ttest_from_moments(*mom)
        host = [a.cpu() for a in mom + pt]
    side.synchronize()
    for k, scale in enumerate((2.0, 4.0, 2.0, 4.0)):
        _same_bits(host[k].numpy(), scale * want[k][:, :64], f"plane {k}")
    p0, t0 = eng.ttest_from_moments(*(scale * want[k][:, :64] for k, scale in enumerate((2.0, 4.0, 2.0, 4.0))))
    _same_bits(host[4].numpy(), p0, "p")
    _same_bits(host[5].numpy(), t0, "t")
    eng.group_moments(torch.zeros((X.shape[0], 1), device="cuda"), 0, 1)  # (the shared engine back on the default stream)


# ---- 9. error paths -------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    import ctypes
    X, codes, want = _exact(np.float32)
    G = len(_SIZES)
    eng = get_engine()
    eng.set_groups(_groups(codes))
    lib, n, m = eng.lib, X.shape[0], X.shape[1]
    out = np.zeros((G, m))
    vp = lambda a: a.ctypes.data
    assert lib.illico_group_moments_dense(eng.h, vp(X), _lib.F32, n, m, m, 0, m, _lib.FLAG_LOG1P, vp(out), None, None, None, m) == _lib.ERR_ARG
    assert b"LOG1P" in lib.illico_last_error(eng.h)
    assert lib.illico_group_moments_dense(eng.h, vp(X), _lib.F32, n, m, m, 0, m, 0, None, None, None, None, m) == _lib.ERR_ARG
    assert lib.illico_group_moments_dense(eng.h, vp(X), _lib.F32, n, m, m, 5, m + 1, 0, vp(out), None, None, None, m) == _lib.ERR_BOUNDS
    assert lib.illico_group_moments_dense(eng.h, vp(X), _lib.F32, n, m, m, 0, m, 0, vp(out), None, None, None, m - 1) == _lib.ERR_ARG
    assert lib.illico_group_moments_dense(eng.h, vp(X), 9, n, m, m, 0, m, 0, vp(out), None, None, None, m) == _lib.ERR_DTYPE
    assert lib.illico_group_moments_dense(eng.h, vp(X), _lib.F32, n - 1, m, m, 0, m, 0, vp(out), None, None, None, m) == _lib.ERR_NO_GROUPS
    with pytest.raises(ValueError):
        eng.group_moments(X, 0, m + 1)
    with pytest.raises(ValueError):
        eng.group_moments(X, 0, m, out=(None, None))
    S, Q = want[0], want[1]
    tt = lambda *a: lib.illico_ttest_from_moments(eng.h, *a)
    assert tt(vp(S), vp(Q), None, None, m, m, 0, 0, 0, vp(out), None, None, None, None, None, None, m) == _lib.ERR_ARG     # one-versus-rest without rest planes
    assert b"rest" in lib.illico_last_error(eng.h)
    with pytest.raises(ValueError):
        eng.ttest_from_moments(S, Q)
    assert tt(vp(S), vp(Q), vp(S), vp(Q), m, m, 0, 0, 0, None, None, None, None, None, None, None, m) == _lib.ERR_ARG     # all outputs null
    assert tt(vp(S), vp(Q), vp(S), vp(Q), m, m, 2, 0, 0, vp(out), None, None, None, None, None, None, m) == _lib.ERR_ARG   # unknown variant
    assert tt(vp(S), vp(Q), vp(S), vp(Q), m, m, 0, 7, 0, vp(out), None, None, None, None, None, None, m) == _lib.ERR_ALTERNATIVE
    assert tt(vp(S), vp(Q), vp(S), vp(Q), m, m - 1, 0, 0, 0, vp(out), None, None, None, None, None, None, m) == _lib.ERR_ARG
    assert lib.illico_student_t_pvalues(eng.h, vp(S), vp(Q), 4, 5, 0, vp(out)) == _lib.ERR_ALTERNATIVE
    # a context without groups
    fresh = _lib.Engine(eng.device)
    try:
        assert lib.illico_group_moments_dense(fresh.h, vp(X), _lib.F32, n, m, m, 0, m, 0, vp(out), None, None, None, m) == _lib.ERR_NO_GROUPS
        assert lib.illico_ttest_from_moments(fresh.h, vp(S), vp(Q), vp(S), vp(Q), m, m, 0, 0, 0, vp(out), None, None, None, None, None, None,
                                             m) == _lib.ERR_NO_GROUPS
    finally:
        fresh.close()
    # the engine still works
    _same_bits(eng.group_moments(X, 0, m)[0], S, "sum after the errors")
