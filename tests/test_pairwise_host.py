"""All-pairs Wilcoxon tests from per-(group, gene) value histograms: the arithmetic of include/illico_hip.h
(illico_pairwise_from_hists) restated in float64 numpy and held to the CPU oracle run once per reference, plus the argument
validation of pairwise_wilcoxon that needs no device.  tests/test_gpu_pairwise.py imports the cases and the restatement.

Pairs near the size limit of the integer sums (2^21 - 1 cells) need no matrix: big_hists() gives synthetic histograms, and pairs_exact()
is the same definition in Python integers and 50-digit mpmath, to which the float64 restatement is held here (held_to_exact() takes
device planes as well).  edge_value_case() builds the input for tests of the value classifier: every kind of value that is no count."""
import functools
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
from scipy import special

import oracle
from conftest import make_counts

HIST_VALUES = 256
#: genes of case A that hold a value which is no integer in [0, 255]
CASE_A_FLAGGED = (7, 9, 11)


def _codes(sizes, seed):
    return np.random.RandomState(seed).permutation(np.repeat(np.arange(len(sizes)), sizes))


@functools.lru_cache(maxsize=None)
def case(name):
    """(X float32 [N, M], codes int64 [N], counts int64 [G]).  The arrays are shared: do not write to them."""
    if name == "A":  # every cell width and tile edge: sizes around 64 and 256, two full gene tiles and a ragged one
        sizes = (1, 2, 63, 255, 256, 257, 1024, 742)
        codes = _codes(sizes, 131)
        X, rng = make_counts(31, 2600, 130, 0.7)
        X[:, 3] = 0                                                  # constant: p = 1, z = 0
        X[:, 5] = rng.randint(253, 256, size=2600)                   # the table's last values ...
        X[codes == 4, 5] = 255                                       # ... and a multiplicity equal to the group's size (256)
        X[:, 7] = rng.randint(254, 257, size=2600)                   # 256: flagged
        X[::7, 9] += 0.5                                             # fractional: flagged
        X[::11, 11] = -1                                             # negative: flagged
    elif name == "B":  # one histogram cell passes 65535
        sizes = (66000, 300, 5)
        codes = _codes(sizes, 132)
        X = np.random.RandomState(32).poisson(3.0, size=(sum(sizes), 4)).astype(np.float32)
        X[codes == 0, 0] = 2
    elif name == "C":  # group counts beyond 64 and 128, a ragged last block of references
        sizes = (10,) * 130
        codes = _codes(sizes, 133)
        X, _ = make_counts(9, 1300, 70, 0.7)
    else:
        raise KeyError(name)
    for a in (X, codes):
        a.setflags(write=False)
    return X, codes.astype(np.int64), np.asarray(sizes, dtype=np.int64)


def labels_of(codes):
    """string labels whose np.unique order is the order of the codes"""
    return np.array([f"g{c:03d}" for c in codes])


def groups_of(codes, ref=None):
    lab = labels_of(codes)
    return oracle.encode_and_count_groups(lab, None if ref is None else f"g{ref:03d}")[1]


@functools.lru_cache(maxsize=None)
def oracle_slabs(name, is_log1p=False, use_continuity=True, tie_correct=True, alternative="two-sided"):
    """(p, U, fc) float64 [G, G, M]: slab r = oracle.run with reference r"""
    X, codes, counts = case(name)
    out = [oracle.run(np.ascontiguousarray(X), groups_of(codes, r), is_log1p=is_log1p, use_continuity=use_continuity, tie_correct=tie_correct,
                      alternative=alternative) for r in range(counts.size)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def hists_numpy(X, codes, G):
    """(H int64 [G, M, 256], flags bool [M]): np.add.at counts of the values 0 .. 255; H of a flagged gene counts its valid values only"""
    V = np.asarray(X, dtype=np.float64)
    N, M = V.shape
    ok = (V == np.floor(V)) & (V >= 0) & (V <= HIST_VALUES - 1)
    H = np.zeros((G, M, HIST_VALUES), dtype=np.int64)
    r, c = np.nonzero(ok)
    np.add.at(H, (codes[r], c, V[r, c].astype(np.int64)), 1)
    return H, ~ok.all(axis=0)


def pairs_numpy(H, counts, *, use_continuity=True, tie_correct=True, alternative="two-sided"):
    """(p, U, fc, z) float64 [G, G, M] indexed [r, g, gene], from the histograms alone: the block of include/illico_hip.h."""
    H = np.asarray(H, dtype=np.int64)
    G, M, R = H.shape
    n = np.asarray(counts, dtype=np.int64)
    cum = np.concatenate([np.zeros((G, M, 1), dtype=np.int64), np.cumsum(H, axis=2)], axis=2)
    S = (H * np.arange(R, dtype=np.int64)).sum(axis=2)                       # exact value sums
    p, U, fc, z = (np.empty((G, G, M), dtype=np.float64) for _ in range(4))
    cc = 0.5 if use_continuity else 0.0
    for r in range(G):
        n_r, n_g = n[r], n[:, None]
        S2 = (H * (cum[r, :, :-1] + cum[r, :, 1:])[None]).sum(axis=2)        # [G, M]
        u = 0.5 * (2 * n_r * n_g - S2).astype(np.float64)
        t = H + H[r][None]
        tie = (t ** 3 - t).sum(axis=2).astype(np.float64) if tie_correct else np.zeros((G, M))
        nn = n_r + n_g
        nnn = (nn * (nn - 1) * (nn + 1)).astype(np.float64)
        var0 = (n_r * n_g * (nn + 1)).astype(np.float64) / 12.0
        n12 = (n_r * n_g).astype(np.float64)
        mu = n12 / 2.0
        tie_corr = 1.0 - tie / nnn
        live = tie_corr > 1.0e-9
        with np.errstate(invalid="ignore", divide="ignore"):
            sigma = np.sqrt(var0 * tie_corr)
            if alternative == "two-sided":
                delta = np.minimum(u, n12 - u) - mu
                pv = special.erfc(((np.abs(delta) + np.sign(delta) * cc) / sigma) / np.sqrt(2.0))
            elif alternative == "greater":
                pv = 0.5 * special.erfc((((u - mu) - cc) / sigma) / np.sqrt(2.0))
            elif alternative == "less":
                pv = 0.5 * special.erfc(-(((u - mu) + cc) / sigma) / np.sqrt(2.0))
            else:
                raise ValueError(alternative)
            zz = (mu - u) / sigma
            mu_ref = S[r].astype(np.float64) / float(n_r)
            f = (S.astype(np.float64) / n_g.astype(np.float64)) / mu_ref[None]
        p[r] = np.where(live, pv, 1.0)
        z[r] = np.where(live, zz, 0.0)
        U[r] = u
        fc[r] = np.where(mu_ref[None] == 0.0, np.inf, f)
        p[r, r], z[r, r] = 1.0, 0.0
    return p, U, fc, z


def offdiag(G):
    return ~np.eye(G, dtype=bool)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_restatement_matches_the_oracle_for_every_reference(name):
    X, codes, counts = case(name)
    G = counts.size
    H, flags = hists_numpy(X, codes, G)
    assert np.array_equal(np.flatnonzero(flags), CASE_A_FLAGGED if name == "A" else [])
    p, U, fc, z = pairs_numpy(H, counts)
    wp, wU, wfc = oracle_slabs(name)
    keep = offdiag(G)[:, :, None] & ~flags[None, None, :]
    np.testing.assert_array_equal(U[keep], wU[keep])
    np.testing.assert_allclose(p[keep], wp[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(fc[keep], wfc[keep], rtol=1e-12, atol=0.0)
    # the inputs' own condition: the p-values are mostly informative, not saturated at 0 or 1
    sat = np.mean((wp[keep] == 0.0) | (wp[keep] == 1.0))
    print(f"case {name}: {sat:.4f} of {keep.sum()} compared p-values are exactly 0 or 1")
    assert sat <= 0.20
    # antisymmetry of the definition itself
    U, z = U[:, :, ~flags], z[:, :, ~flags]
    nn = counts[:, None] * counts[None, :]
    assert np.array_equal(U + U.transpose(1, 0, 2), np.broadcast_to(nn[:, :, None].astype(np.float64), U.shape))
    assert np.array_equal(z, -z.transpose(1, 0, 2))
    assert np.array_equal(np.diagonal(U, axis1=0, axis2=1).T, np.broadcast_to((counts ** 2 / 2.0)[:, None], U.shape[1:]))


def test_restatement_less_and_greater_mirror_each_other():
    X, codes, counts = case("A")
    H, flags = hists_numpy(X, codes, counts.size)
    less = pairs_numpy(H, counts, alternative="less")[0]
    greater = pairs_numpy(H, counts, alternative="greater")[0]
    keep = offdiag(counts.size)[:, :, None] & ~flags[None, None, :]
    assert np.array_equal(less[keep], greater.transpose(1, 0, 2)[keep])


# ---- pairs at the size limit: synthetic histograms, and the definition in exact arithmetic ----
#: group sizes of big_hists(): the largest pair has 2^21 - 1 cells, the largest the integer sums of the pair kernel hold
BIG_COUNTS = ((1 << 20) - 1, 1 << 20, 700001, 65536, 5, 1)
#: its constructed genes: all cells in bin 0 / all in bin 255 / each group half and half / even groups in bin 0, odd groups in bin 255
BIG_ZERO, BIG_TOP, BIG_HALVES, BIG_SEPARATED = 66, 67, 68, 69
EXACT_DIGITS = 50
EPS4 = 4.0 * 2.0 ** -53  # the four roundings that enter 1 - tie / nnn


@functools.lru_cache(maxsize=None)
def big_hists():
    """(H int64 [6, 70, 256], counts int64 [6]).  Genes 0 .. 65: each group's size drawn multinomially from one Poisson-shaped
    distribution per gene (rate from [0.05, 40]), shared by the groups, so that p stays informative at a million cells.  Shared: do
    not write to them."""
    rng = np.random.RandomState(141)
    n = np.asarray(BIG_COUNTS, dtype=np.int64)
    H = np.zeros((n.size, 70, HIST_VALUES), dtype=np.int64)
    c = np.arange(HIST_VALUES)
    for j in range(66):
        lam = rng.uniform(0.05, 40.0)
        pmf = np.exp(c * np.log(lam) - lam - special.gammaln(c + 1.0))
        pmf /= pmf.sum()
        for g in range(n.size):
            H[g, j] = rng.multinomial(n[g], pmf)
    H[:, BIG_ZERO, 0] = n
    H[:, BIG_TOP, 255] = n
    H[:, BIG_HALVES, 0], H[:, BIG_HALVES, 255] = n // 2, n - n // 2
    H[0::2, BIG_SEPARATED, 0], H[1::2, BIG_SEPARATED, 255] = n[0::2], n[1::2]
    assert np.array_equal(H.sum(axis=2), np.broadcast_to(n[:, None], (n.size, 70)))
    for a in (H, n):
        a.setflags(write=False)
    return H, n


def pair_ints(H, counts, r, g, gene):
    """The integers of one test, group g against reference r, as Python ints: S2, two_u = 2 U, tie = sum (t^3 - t),
    nnn = n (n - 1) (n + 1), var12 = n_r n_g (n + 1) (twelve times the variance without ties), n12 = n_r n_g, the value sums S_g, S_r."""
    hg, hr = [int(x) for x in H[g][gene]], [int(x) for x in H[r][gene]]
    n_g, n_r = int(counts[g]), int(counts[r])
    cum = S2 = tie = S_g = S_r = 0
    for c, (a, b) in enumerate(zip(hg, hr)):
        S2 += a * (2 * cum + b)
        cum += b
        t = a + b
        tie += t * t * t - t
        S_g += c * a
        S_r += c * b
    n = n_g + n_r
    return dict(S2=S2, two_u=2 * n_r * n_g - S2, tie=tie, nnn=n * (n - 1) * (n + 1), var12=n_r * n_g * (n + 1), n12=n_r * n_g, n_g=n_g, n_r=n_r,
                S_g=S_g, S_r=S_r)


def pairs_exact(H, counts, r, g, gene, *, use_continuity=True, tie_correct=True, alternative="two-sided", ints=None):
    """(two_u int, tie_corr, z, p as mpmath numbers of EXACT_DIGITS digits) of group g against reference r: the definition of
    pairs_numpy without a rounding that matters.  The same rule as there: tie_corr <= 1e-9 gives p = 1 and z = 0."""
    import mpmath
    q = pair_ints(H, counts, r, g, gene) if ints is None else ints
    with mpmath.workdps(EXACT_DIGITS):
        mpf = mpmath.mpf
        tie_corr = 1 - mpf(q["tie"] if tie_correct else 0) / q["nnn"]
        if tie_corr <= mpf("1e-9"):
            return q["two_u"], tie_corr, mpf(0), mpf(1)
        sigma = mpmath.sqrt(mpf(q["var12"]) / 12 * tie_corr)
        d = mpf(q["two_u"] - q["n12"]) / 2                       # U - mu
        cc = mpf(0.5) if use_continuity else mpf(0)
        root2 = mpmath.sqrt(2)
        if alternative == "two-sided":                           # delta = min(U, n12 - U) - mu = -|d|
            p = mpmath.erfc(((abs(d) - cc) / sigma if d != 0 else mpf(0)) / root2)
        elif alternative == "greater":
            p = mpmath.erfc((d - cc) / sigma / root2) / 2
        elif alternative == "less":
            p = mpmath.erfc(-(d + cc) / sigma / root2) / 2
        else:
            raise ValueError(alternative)
        return q["two_u"], tie_corr, -d / sigma, p


def exact_planes(H, counts, *, use_continuity=True, tie_correct=True, alternative="two-sided", ints=None):
    """dict of float64 [G, G, M] planes indexed [r, g, gene], each the exact value rounded once: U, z, p, tie_corr, fc; the diagonal as
    the device defines it (p = 1, z = 0, U = n^2 / 2, fc = 1 or inf).  ``ints``: {(r, g, gene): pair_ints} computed before."""
    G, M = int(H.shape[0]), int(H.shape[1])
    Hl = H.tolist()
    out = {k: np.empty((G, G, M), dtype=np.float64) for k in ("U", "z", "p", "tie_corr", "fc")}
    for r in range(G):
        for g in range(G):
            for j in range(M):
                q = ints[r, g, j] if ints is not None else pair_ints(Hl, counts, r, g, j)
                two_u, tc, z, p = pairs_exact(Hl, counts, r, g, j, use_continuity=use_continuity, tie_correct=tie_correct, alternative=alternative, ints=q)
                if r == g:
                    z, p = 0.0, 1.0
                out["U"][r, g, j] = float(Fraction(two_u, 2))
                out["tie_corr"][r, g, j], out["z"][r, g, j], out["p"][r, g, j] = float(tc), float(z), float(p)
                out["fc"][r, g, j] = float(Fraction(q["S_g"] * q["n_r"], q["n_g"] * q["S_r"])) if q["S_r"] else np.inf
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def big_ints():
    H, n = big_hists()
    Hl = H.tolist()
    return {(r, g, j): pair_ints(Hl, n, r, g, j) for r in range(n.size) for g in range(n.size) for j in range(H.shape[1])}


@functools.lru_cache(maxsize=None)
def big_exact(alternative="two-sided", use_continuity=True, tie_correct=True):
    """exact_planes of big_hists().  Shared: do not write to them."""
    H, n = big_hists()
    return exact_planes(H, n, use_continuity=use_continuity, tie_correct=tie_correct, alternative=alternative, ints=big_ints())


def held_to_exact(p, U, z, ex, keep, what):
    """Assert planes [r, g, gene] against exact_planes ``ex`` where ``keep``: U equal; z within 1e-12 + EPS4 / tie_corr, relative, exact
    zeros equal; p within 1e-12 + (1 + z^2) EPS4 / tie_corr, relative, for p above 1e-300 (below: not above it either).  1e-12 is the
    project's tolerance between device p-values and the oracle; the second term is the conditioning of 1 - tie / nnn (four roundings
    enter it, z's relative sensitivity to them is at most 1 / (2 tie_corr)); 1 + z^2 bounds d log p / d log z of the normal tail.
    Returns the worst error / bound of z (None without z) and of p."""
    keep = np.broadcast_to(keep, ex["p"].shape)
    np.testing.assert_array_equal(np.asarray(U)[keep], ex["U"][keep], err_msg=f"statistic {what}")
    tc, ez, ep = ex["tie_corr"][keep], ex["z"][keep], ex["p"][keep]
    live = tc > 1.0e-9
    assert not np.any((tc > 1.0e-10) & (tc < 1.0e-8)), "the inputs' own condition: no tie correction at the 1e-9 rule"
    with np.errstate(divide="ignore"):
        cond = np.where(live, EPS4 / np.where(live, tc, 1.0), 0.0)
    ratios = []
    for got, want, bound, name in ((z, ez, 1.0e-12 + cond, "z_score"), (p, ep, 1.0e-12 + (1.0 + ez * ez) * cond, "p_value")):
        if got is None:
            ratios.append(None)
            continue
        got = np.asarray(got)[keep]
        fixed = ~live | (want == 0.0)                            # p = 1 and z = 0 of the 1e-9 rule, and exact zeros
        if name == "z_score":
            assert np.array_equal(got[fixed], want[fixed]), f"{name} {what}: exact zeros"
        else:
            assert np.array_equal(got[~live], want[~live]), f"{name} {what}: p = 1 where the tie correction vanishes"
        rel = (want != 0.0) & live & (np.abs(want) > 1.0e-300)
        err = np.abs(got[rel] - want[rel]) / np.abs(want[rel]) / bound[rel]
        worst = float(err.max()) if err.size else 0.0
        ratios.append(worst)
        k = int(np.argmax(err)) if err.size else 0
        assert worst <= 1.0, f"{name} {what}: error / bound = {worst:.3g} (got {got[rel][k]!r}, exact {want[rel][k]!r}, tie_corr {tc[rel][k]:.3g})"
        tiny = live & (np.abs(want) <= 1.0e-300)
        assert np.all(np.abs(got[tiny]) <= 1.0e-300 * (1.0 + bound[tiny])), f"{name} {what}: values of at most 1e-300"
    return tuple(ratios)


@pytest.mark.parametrize("alternative", ["two-sided", "less", "greater"])
def test_restatement_is_held_to_exact_arithmetic_at_the_size_limit(alternative):
    H, n = big_hists()
    assert int(n[0] + n[1]) == (1 << 21) - 1 and H.shape == (6, 70, 256)
    ex = big_exact(alternative)
    p, U, fc, z = pairs_numpy(H, n, alternative=alternative)
    keep = offdiag(n.size)[:, :, None]
    rz, rp = held_to_exact(p, U, z, ex, keep, f"restatement, {alternative}")
    np.testing.assert_allclose(fc, ex["fc"], rtol=1e-12, atol=0.0)
    ep = ex["p"][np.broadcast_to(keep, ex["p"].shape)]
    sat = float(np.mean((ep == 0.0) | (ep == 1.0)))
    print(f"big_hists, {alternative}: worst error / bound: z {rz:.4g}, p {rp:.4g}; {sat:.4f} of {ep.size} exact p-values round to 0 or 1")
    assert sat <= 0.20
    # the pair the bounds are there for: a million cells against one cell under complete separation
    tc = ex["tie_corr"][5, 0, BIG_SEPARATED]
    assert 1.0e-6 < tc < 1.0e-5


def test_exact_arithmetic_and_restatement_agree_on_a_small_case():
    X, codes, counts = case("A")
    genes = [0, 3, 5, 64, 129]                                   # gene 3 is constant: the 1e-9 rule
    H, flags = hists_numpy(X[:, genes], codes, counts.size)
    assert not flags.any()
    for opts in (dict(), dict(alternative="greater", use_continuity=False), dict(alternative="less", tie_correct=False)):
        ex = exact_planes(H, counts, **opts)
        p, U, fc, z = pairs_numpy(H, counts, **opts)
        held_to_exact(p, U, z, ex, offdiag(counts.size)[:, :, None], str(opts))
        np.testing.assert_allclose(fc, ex["fc"], rtol=1e-12, atol=0.0)
        d = np.arange(counts.size)
        assert np.array_equal(U[d, d], ex["U"][d, d]) and np.array_equal(p[d, d], ex["p"][d, d]) and np.array_equal(z[d, d], ex["z"][d, d])
    assert np.all(ex["tie_corr"][:, :, 1][offdiag(counts.size)] == 1.0)  # (tie_correct off in the last round)


# ---- the value classifier: every kind of value that is no integer in [0, 255], and the ones that only look like it ----
EDGE_SIZES = (1, 64, 65, 257, 313)
EDGE_MINUS_ZERO, EDGE_TOP = 30, 33  # unflagged genes: -0.0 (integer types: 0) in a quarter of the cells; one 255


@functools.lru_cache(maxsize=None)
def edge_value_case(dtype):
    """(X dtype [700, 66], codes int64, counts int64, flagged {gene: what}, genes that hold NaN).  Each special value sits in a gene of its
    own, at one cell of a group of more than 64 cells, beyond the group's first 8 rows; flagged genes of tile 0 have unflagged
    neighbours; genes 64 and 65, the whole ragged tile, are both flagged.  Shared: do not write to them."""
    dt = np.dtype(dtype)
    codes = _codes(EDGE_SIZES, 151)
    X = make_counts(51, 700, 66, 0.7)[0].astype(dt)
    rows = {g: np.flatnonzero(codes == g) for g in (2, 3, 4)}
    if dt.kind == "f":
        specials = [("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("denormal", np.nextafter(dt.type(0), dt.type(1))), ("255.5", 255.5),
                    ("256", 256.0), ("2^32", 2.0 ** 32)]
        if dt.itemsize == 8:
            specials += [("2^53", 2.0 ** 53), ("nextafter(255, 256)", np.nextafter(255.0, 256.0))]
        ragged = (256.0, -1.0)
    else:
        info = np.iinfo(dt)
        specials = [("-1", -1), ("256", 256), ("min", info.min), ("max", info.max)]
        if dt.itemsize == 8:
            specials += [("2^32", 1 << 32), ("2^32 + 5", (1 << 32) + 5), ("2^40 + 255", (1 << 40) + 255)]
        ragged = (256, -1)
    flagged = {}
    for k, (what, v) in enumerate(specials):
        gene, g = 2 + 3 * k, (2, 3, 4)[k % 3]
        X[rows[g][8 + (11 * k) % (rows[g].size - 8)], gene] = v
        flagged[gene] = what
    X[rows[4][100], 64], X[rows[3][200], 65] = ragged
    flagged[64], flagged[65] = "256, ragged tile", "-1, ragged tile"
    X[::4, EDGE_MINUS_ZERO] = -0.0 if dt.kind == "f" else 0
    X[rows[3][20], EDGE_TOP] = 255
    assert max(flagged) == 65 and all(j - 1 not in flagged and j + 1 not in flagged for j in flagged if j < 64)
    X.setflags(write=False)
    counts = np.asarray(EDGE_SIZES, dtype=np.int64)
    return X, codes.astype(np.int64), counts, flagged, tuple(j for j, what in flagged.items() if what == "nan")


def with_stored_zeros(X, fmt):
    """scipy CSC / CSR of X that stores every value that is not +0 (NaN, the denormal and every -0.0 included) and one more zero, -0.0
    for a float type, at a cell that is zero in a gene other than EDGE_MINUS_ZERO"""
    from scipy import sparse
    keep = (X != 0) | np.signbit(X)
    r, c = np.nonzero(keep)
    zr, zc = (a[-1] for a in np.nonzero(~keep))
    assert zc != EDGE_MINUS_ZERO
    zero = X.dtype.type(-0.0 if X.dtype.kind == "f" else 0)
    M = sparse.coo_matrix((np.append(X[r, c], zero), (np.append(r, zr), np.append(c, zc))), shape=X.shape)
    M = M.tocsc() if fmt == "csc" else M.tocsr()
    assert M.nnz == r.size + 1 and M.data.dtype == X.dtype
    return M


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_edge_value_case_flags_what_it_builds(dtype):
    X, codes, counts, flagged, nan_genes = edge_value_case(dtype)
    H, flags = hists_numpy(X, codes, counts.size)
    assert np.array_equal(np.flatnonzero(flags), sorted(flagged))
    assert len(flagged) == {"float32": 9, "float64": 11, "int32": 6, "int64": 9}[np.dtype(dtype).name]
    assert len(nan_genes) == (1 if np.dtype(dtype).kind == "f" else 0)
    ok = ~flags
    assert np.array_equal(H[:, ok].sum(axis=2), np.broadcast_to(counts[:, None], (counts.size, int(ok.sum()))))
    zero = X[:, EDGE_MINUS_ZERO] == 0                            # zeros of either sign; the rows [::4] hold -0.0 (0 for an integer type)
    assert zero[::4].all() and np.array_equal(H[:, EDGE_MINUS_ZERO, 0], np.bincount(codes[zero], minlength=counts.size))
    assert H[3, EDGE_TOP, 255] >= 1
    if np.dtype(dtype).kind == "f":
        assert np.signbit(X[::4, EDGE_MINUS_ZERO]).all() and (X[::4, EDGE_MINUS_ZERO] == 0).all()
    for fmt in ("csc", "csr"):
        M = with_stored_zeros(X, fmt)
        back = M.toarray()
        assert np.array_equal(back, X, equal_nan=True) if np.dtype(dtype).kind == "f" else np.array_equal(back, X)


# ---- argument validation of pairwise_wilcoxon: raised before any device work ----
def _adata():
    from illico_amd import AnnDataLite
    X = np.arange(24, dtype=np.float32).reshape(6, 4) % 5
    return AnnDataLite(X, obs=pd.DataFrame({"g": ["a", "a", "b", "b", "c", "c"]}))


@pytest.mark.parametrize("kw, match", [
    (dict(groups=["a", "zz"]), "not present"),
    (dict(groups=["a"]), "at least two"),
    (dict(groups=["a", "a", "b"]), "twice"),
    (dict(groups="ab"), "sequence of labels"),
    (dict(alternative="both"), "Unsupported alternative"),
    (dict(scores=1), "scores must be a bool"),
    (dict(corr_method="holm"), "correction method"),
    (dict(max_result_bytes=-1), "max_result_bytes"),
])
def test_pairwise_wilcoxon_refuses_bad_arguments(kw, match):
    from illico_amd import pairwise_wilcoxon
    with pytest.raises(ValueError, match=match):
        pairwise_wilcoxon(_adata(), False, "g", **kw)


def test_pairwise_wilcoxon_refuses_a_non_bool_is_log1p():
    from illico_amd import pairwise_wilcoxon
    with pytest.raises(ValueError, match="is_log1p must be a bool"):
        pairwise_wilcoxon(_adata(), 1, "g")


def test_pairwise_wilcoxon_refuses_a_result_beyond_max_result_bytes():
    from illico_amd import pairwise_wilcoxon
    with pytest.raises(ValueError, match=r"max_result_bytes = 1\b"):
        pairwise_wilcoxon(_adata(), False, "g", max_result_bytes=1)
    # 3 x 2 pairs x 4 genes x 8 bytes x 3 columns = 576 bytes; a fourth column with scores
    with pytest.raises(ValueError, match="768 bytes"):
        pairwise_wilcoxon(_adata(), False, "g", scores=True, max_result_bytes=767)


def test_the_entry_points_are_declared_exported_and_built():
    from pathlib import Path
    from illico_amd import _lib
    from illico_amd.csrc import build
    root = Path(__file__).resolve().parent.parent
    header = (root / "include" / "illico_hip.h").read_text()
    for name in ("illico_group_value_hists_dense", "illico_group_value_hists_csc", "illico_group_value_hists_csr", "illico_pairwise_from_hists"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    assert "pairwise" in build.UNITS and "pairwise" in build.DEV_UNITS
    assert (root / "illico_amd" / "csrc" / "pairwise.hip").exists()
