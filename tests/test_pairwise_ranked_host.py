"""All-pairs Wilcoxon tests for any values from one sorted walk per gene (illico_pairwise_ranked_*): the L / T / X definition of
include/illico_hip_ranked.h and DESIGN.md section 20 restated in numpy integers -- the zeros handled by the correction at the end, as the
device does -- and held to the CPU oracle run once per reference.  The integers are finalised by pairs_exact of test_pairwise_host
(no copy of the p-value formula here).  tests/test_gpu_pairwise_ranked.py imports the cases and the restatement;
tests/test_gpu_pairwise_ranked_edges.py the second derivation (ltx_int64), the seeded sweep and the constructed edge cases below, each
checked here for what it names."""
import functools

import numpy as np
import pytest

import oracle
from test_pairwise_host import exact_planes, groups_of, hists_numpy, offdiag, pair_ints, pairs_numpy

RANKED_SIZES = (1, 2, 63, 64, 65, 300, 1024, 1141)
#: the constructed genes of ranked_case("f32")
KINDS = ("negatives", "70 % zeros", "log1p of small counts", "constant non-zero", "all zero", "one non-zero", "-0.0", "+-inf", "denormal",
         "one ulp apart")
TIE_HEAVY = 2


@functools.lru_cache(maxsize=None)
def ranked_case(name):
    """(X [2660, M], codes int64, counts int64).  "f32": 130 float32 genes, the first ten as KINDS names them; "i32": 20 int32 genes with
    negatives and values beyond 255.  Shared: do not write to them."""
    rng = np.random.RandomState(171)
    N = sum(RANKED_SIZES)
    codes = rng.permutation(np.repeat(np.arange(len(RANKED_SIZES)), RANKED_SIZES))
    if name == "i32":
        X = rng.poisson(2.0, size=(N, 20)).astype(np.int32)
        X[rng.rand(N, 20) < 0.6] = 0
        X[:, 1] -= 3                                                  # negatives, zeros among them
        X[:, 2] = rng.randint(-100000, 100000, size=N)                # far beyond 255, nearly tie-free
        X[::5, 3] = 1000 + rng.randint(0, 3, size=X[::5, 3].size)
        X[0, 4], X[1, 4] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
        X[:, 5] = 7
    else:
        M = 130
        X = np.zeros((N, M), dtype=np.float32)
        for j in range(M):
            kind = j % 3
            if kind == 0:    # log-normalised counts: tie-heavy, mostly zero
                X[:, j] = np.log1p(rng.poisson(rng.uniform(0.2, 3.0), size=N)).astype(np.float32)
            elif kind == 1:  # continuous, 70 % zeros
                X[:, j] = rng.lognormal(size=N).astype(np.float32) * (rng.rand(N) < 0.3)
            else:            # continuous, both signs, no zero
                X[:, j] = rng.normal(size=N).astype(np.float32)
        X[:, 0] = -np.abs(rng.normal(size=N)).astype(np.float32) * (rng.rand(N) < 0.5)
        X[:, 1] = rng.lognormal(size=N).astype(np.float32) * (rng.rand(N) < 0.3)
        X[:, 2] = np.log1p(rng.poisson(1.0, size=N)).astype(np.float32)
        X[:, 3] = 2.5
        X[:, 4] = 0.0
        X[:, 5] = 0.0
        X[np.flatnonzero(codes == 5)[7], 5] = 3.25
        X[:, 6] = rng.poisson(0.7, size=N).astype(np.float32) * 0.5
        X[::4, 6] = -0.0
        X[:, 7] = rng.normal(size=N).astype(np.float32)
        X[np.flatnonzero(codes == 6)[:3], 7] = np.inf
        X[np.flatnonzero(codes == 7)[:2], 7] = -np.inf
        X[:, 8] = rng.poisson(0.3, size=N).astype(np.float32)
        X[np.flatnonzero(codes == 5)[:9], 8] = np.nextafter(np.float32(0), np.float32(1))
        X[np.flatnonzero(codes == 6)[:4], 8] = -np.nextafter(np.float32(0), np.float32(1))
        X[:, 9] = np.where(rng.rand(N) < 0.5, np.float32(1.0), np.nextafter(np.float32(1), np.float32(2)))
    for a in (X, codes):
        a.setflags(write=False)
    return X, codes.astype(np.int64), np.asarray(RANKED_SIZES, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def ranked_oracle_slabs(name, is_log1p=False, use_continuity=True, tie_correct=True, alternative="two-sided"):
    """(p, U, fc) float64 [G, G, M]: slab r = oracle.run with reference r"""
    X, codes, counts = ranked_case(name)
    out = [oracle.run(np.ascontiguousarray(X), groups_of(codes, r), is_log1p=is_log1p, use_continuity=use_continuity, tie_correct=tie_correct,
                      alternative=alternative) for r in range(counts.size)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def recode(x):
    """(codes int64 [N] in 0 .. d - 1, d): the values of one gene recoded order-preservingly; -0.0 and 0.0 share a code"""
    u, inv = np.unique(np.asarray(x, dtype=np.float64) + 0.0, return_inverse=True)
    return inv.astype(np.int64), int(u.size)


def ltx_numpy(x, codes, counts, sel):
    """(S2, tie) Python-int object arrays [K, K] indexed [r][g] of one gene: the walk over the NON-ZERO values alone, the zeros added at
    the end -- the definition as the device evaluates it."""
    v = np.asarray(x, dtype=np.float64)
    K = len(sel)
    n = [int(counts[s]) for s in sel]
    nz = v != 0
    vals, inv = np.unique(v[nz], return_inverse=True)
    t = np.zeros((K, vals.size), dtype=np.int64)
    slot = np.full(int(counts.size), -1)
    slot[np.asarray(sel)] = np.arange(K)
    s = slot[codes[nz]]
    np.add.at(t, (s[s >= 0], inv[s >= 0]), 1)
    t = t.astype(object)
    c = np.concatenate([np.zeros((K, 1), dtype=object), np.cumsum(t, axis=1)[:, :-1]], axis=1) if vals.size else t
    L = t @ c.T                                                    # L[g][r] = sum_v t_g(v) c_r(v)
    T = (t ** 3 - t).sum(axis=1) if vals.size else np.zeros(K, dtype=object)
    X = np.array([[(t[g] * t[r] * (t[g] + t[r])).sum() if vals.size else 0 for r in range(K)] for g in range(K)], dtype=object)
    neg = np.array([int(t[k][vals < 0].sum()) for k in range(K)], dtype=object)
    pos = np.array([int(t[k][vals > 0].sum()) for k in range(K)], dtype=object)
    z = np.array(n, dtype=object) - neg - pos
    L = L + np.outer(pos, z) + np.outer(z, neg)
    T = T + z ** 3 - z
    X = X + np.array([[z[g] * z[r] * (z[g] + z[r]) for r in range(K)] for g in range(K)], dtype=object)
    S2 = np.empty((K, K), dtype=object)
    tie = np.empty((K, K), dtype=object)
    for r in range(K):
        for g in range(K):
            S2[r, g] = n[g] * n[r] + L[g, r] - L[r, g]
            tie[r, g] = T[g] + T[r] + 3 * X[g, r]
    return S2, tie


def ints_of(S2, tie, n_r, n_g):
    """the record pairs_exact finalises (test_pairwise_host.pair_ints), from the walk's integers; the value sums play no part"""
    n = n_g + n_r
    return dict(S2=int(S2), two_u=2 * n_r * n_g - int(S2), tie=int(tie), nnn=n * (n - 1) * (n + 1), var12=n_r * n_g * (n + 1), n12=n_r * n_g,
                n_g=n_g, n_r=n_r, S_g=0, S_r=0)


def ranked_planes_numpy(X, codes, counts, sel=None, *, use_continuity=True, tie_correct=True, alternative="two-sided", ltx=None):
    """dict of float64 [K, K, M] planes U, p, z, tie_corr indexed [r, g, gene] (test_pairwise_host.exact_planes of the walk's integers)
    and fc from float64 sums of the values.  ``ltx``: the walk (ltx_numpy; ltx_int64 for many groups or many values)"""
    ltx = ltx_numpy if ltx is None else ltx
    sel = list(range(counts.size)) if sel is None else [int(s) for s in sel]
    K, M = len(sel), X.shape[1]
    n = [int(counts[s]) for s in sel]
    ints = {}
    for j in range(M):
        S2, tie = ltx(X[:, j], codes, counts, sel)
        for r in range(K):
            for g in range(K):
                ints[r, g, j] = ints_of(S2[r, g], tie[r, g], n[r], n[g])
    out = dict(exact_planes(np.zeros((K, M, 1), dtype=np.int64), np.asarray(n), use_continuity=use_continuity, tie_correct=tie_correct,
                            alternative=alternative, ints=ints))
    sums = np.stack([np.asarray(X, dtype=np.float64)[codes == s].sum(axis=0) for s in sel])
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = sums / np.asarray(n, dtype=np.float64)[:, None]
        out["fc"] = np.where(mean[:, None, :] == 0.0, np.inf, mean[None, :, :] / mean[:, None, :])
    return out


@functools.lru_cache(maxsize=None)
def ranked_exact(name, genes=None, **opts):
    X, codes, counts = ranked_case(name)
    return ranked_planes_numpy(X if genes is None else X[:, list(genes)], codes, counts, **opts)


def test_walk_restatement_matches_the_oracle_for_every_reference():
    X, codes, counts = ranked_case("f32")
    genes = tuple(range(len(KINDS))) + (10, 11, 12)
    # the case holds what it names
    assert (X[:, 0] < 0).any() and np.mean(X[:, 1] == 0) > 0.6 and np.unique(X[:, 2]).size < 12 and np.unique(X[:, 3]).tolist() == [2.5]
    assert not X[:, 4].any() and np.count_nonzero(X[:, 5]) == 1 and np.signbit(X[::4, 6]).all() and np.isinf(X[:, 7]).sum() == 5
    assert 0 < np.abs(X[:, 8][X[:, 8] != 0]).min() < 1e-44 and np.unique(X[:, 9]).size == 2 and np.diff(np.unique(X[:, 9]).view(np.int32)) == 1
    got = ranked_exact("f32", genes)
    wp, wU, wfc = (a[:, :, list(genes)] for a in ranked_oracle_slabs("f32"))
    keep = np.broadcast_to(offdiag(counts.size)[:, :, None], wU.shape)
    np.testing.assert_array_equal(got["U"][keep], wU[keep])
    np.testing.assert_allclose(got["p"][keep], wp[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got["fc"][keep], wfc[keep], rtol=1e-12, atol=0.0, equal_nan=True)
    sat = np.mean((wp[keep] == 0.0) | (wp[keep] == 1.0))
    print(f"{sat:.4f} of {keep.sum()} compared p-values are exactly 0 or 1")
    assert sat <= 0.35   # (the constant and the all-zero gene are 2 of 13, the single non-zero nearly so)


def test_walk_restatement_matches_the_oracle_on_integers():
    X, codes, counts = ranked_case("i32")
    assert X.min() < 0 and X.max() > 255
    genes = (0, 1, 2, 3, 4, 5)
    got = ranked_exact("i32", genes)
    wp, wU, wfc = (a[:, :, list(genes)] for a in ranked_oracle_slabs("i32"))
    keep = np.broadcast_to(offdiag(counts.size)[:, :, None], wU.shape)
    np.testing.assert_array_equal(got["U"][keep], wU[keep])
    np.testing.assert_allclose(got["p"][keep], wp[keep], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got["fc"][keep], wfc[keep], rtol=1e-12, atol=0.0, equal_nan=True)


def test_a_gene_of_few_values_gives_the_integers_of_its_histograms():
    """the bridge to the histogram pair route: recoded to 0 .. d - 1, the walk's S2 and tie are those of pair_ints / pairs_numpy"""
    X, codes, counts = ranked_case("f32")
    G = counts.size
    for gene in (TIE_HEAVY, 6, 9, 4):
        rc, d = recode(X[:, gene])
        assert d <= 256
        H, flags = hists_numpy(rc[:, None].astype(np.float64), codes, G)
        assert not flags.any()
        S2, tie = ltx_numpy(X[:, gene], codes, counts, list(range(G)))
        Hl = H.tolist()
        for r in range(G):
            for g in range(G):
                q = pair_ints(Hl, counts, r, g, 0)
                assert (S2[r, g], tie[r, g]) == (q["S2"], q["tie"]), (gene, r, g)
        # and so the statistic of pairs_numpy, bit for bit
        U = pairs_numpy(H, counts)[1][:, :, 0]
        want = np.array([[0.5 * float(2 * int(counts[r]) * int(counts[g]) - S2[r, g]) for g in range(G)] for r in range(G)])
        assert np.array_equal(U, want)


def test_a_subset_of_groups_in_any_order_is_the_same_definition():
    X, codes, counts = ranked_case("f32")
    full = ltx_numpy(X[:, 1], codes, counts, list(range(counts.size)))
    sel = [6, 2, 5]
    sub = ltx_numpy(X[:, 1], codes, counts, sel)
    for a, r in enumerate(sel):
        for b, g in enumerate(sel):
            assert sub[0][a, b] == full[0][r, g] and sub[1][a, b] == full[1][r, g]


def test_the_ranked_entry_points_are_declared_exported_and_built():
    from pathlib import Path
    from illico_amd import _lib
    from illico_amd.csrc import build
    root = Path(__file__).resolve().parent.parent
    header = (root / "include" / "illico_hip_ranked.h").read_text()
    for name in ("illico_pairwise_ranked_dense", "illico_pairwise_ranked_csc"):
        assert name in _lib.RANKED_SIGNATURES and f"int {name}(" in header
        assert hasattr(_lib.load(), name), f"{name} is not exported by the library"
    assert "pairwise_ranked" in build.UNITS and "pairwise_ranked" in build.DEV_UNITS
    assert (root / "illico_amd" / "csrc" / "pairwise_ranked.hip").exists() and (root / "illico_amd" / "csrc" / "kernels_pairwise_ranked.h").exists()
    assert hasattr(_lib.Engine, "pairwise_ranked") and hasattr(_lib.Engine, "pairwise_ranked_sparse")


# ---- a second derivation of the integers, in int64 ----
def ltx_int64(x, codes, counts, sel):
    """(S2, tie) int64 [K, K] indexed [r][g] of one gene.  The zeros go through the walk as an ordinary value -- no correction at the
    end -- and the sums are matrix products over t[K, D]: a second derivation of ltx_numpy's integers, not a faster copy of it, and
    quick at K = 64 and thousands of values.  Every term and every sum is at most (n_g + n_r)^3 <= (2 n_max)^3, so int64 cannot
    overflow while twice the largest selected group stays below 2^21 cells (the route's own limit for a pair): asserted."""
    sel = np.asarray(sel, dtype=np.int64)
    K = int(sel.size)
    n = np.asarray(counts, dtype=np.int64)[sel]
    assert 2 * int(n.max()) < 1 << 21, "int64 holds (2 n_max)^3 only below 2^21"
    slot = np.full(int(np.asarray(counts).size), -1, dtype=np.int64)
    slot[sel] = np.arange(K)
    s = slot[codes]
    mine = s >= 0
    vals, inv = np.unique(np.asarray(x, dtype=np.float64)[mine] + 0.0, return_inverse=True)   # (+ 0.0: -0.0 ties with 0.0)
    t = np.zeros((K, vals.size), dtype=np.int64)
    np.add.at(t, (s[mine], inv.reshape(-1)), 1)
    assert np.array_equal(t.sum(axis=1), n)
    c = np.cumsum(t, axis=1) - t
    L = t @ c.T                                                    # L[g][r] = sum_v t_g(v) c_r(v)
    T = (t ** 3 - t).sum(axis=1)
    t2 = t * t
    X = t2 @ t.T + t @ t2.T                                        # X[g][r] = sum_v t_g t_r (t_g + t_r)
    S2 = n[:, None] * n[None, :] + L.T - L                         # [r][g]: n_r n_g + L[g][r] - L[r][g]
    tie = T[None, :] + T[:, None] + 3 * X.T
    return S2, tie


# ---- a seeded sweep over group structure, values, sel, record slots and layouts (tests/test_gpu_pairwise_ranked_edges.py) ----
SWEEP_CASES = 24
SWEEP_GROUPS = (2, 3, 7, 8, 33, 64)
SWEEP_LAYOUTS = ("dense device", "dense host", "csc host", "csc device")
SWEEP_CAPS = (0, 1024, 2048)
SWEEP_GENES = ("tie-free, both signs, no zero", "positive, 90 % zeros", "2, 3 or 17 values around zero", "round(4 normal)",
               "non-positive, half zeros", "staircase of tie blocks 1, 2, 3, ...")


@functools.lru_cache(maxsize=None)
def sweep_case(i):
    """(X [N, 6] float32 or int32, codes int64, counts int64, plan) of sweep case i, deterministic in i; the genes as SWEEP_GENES names
    them.  plan: "cap" (pair_rank_cap), "layout", "sel" (None: all groups in order), "col_lb" (1: the window starts at an odd column
    of a wider matrix).  G cycles with i, the value type changes every six cases (so every G meets both), the layout every case.
    Shared: do not write to them."""
    rng = np.random.RandomState(3000 + i)
    G = SWEEP_GROUPS[i % 6]
    is_float = (i // 6) % 2 == 0
    N = int(rng.randint(max(200, 3 * G), 5001))
    sizes = 1 + rng.multinomial(N - G, rng.dirichlet(np.ones(G)))    # groups of one cell, very unequal groups
    codes = rng.permutation(np.repeat(np.arange(G), sizes))
    X = np.zeros((N, 6), dtype=np.float64)
    if is_float:   # (a) multiples of 2^-16: a float64 sum of them is exact, so the fold change's reference has no cancellation error
        u = np.unique(np.round(rng.normal(size=3 * N) * 65536.0) / 65536.0)
        u = u[u != 0]
        X[:, 0] = u[rng.choice(u.size, N, replace=False)]
        X[:, 1] = rng.lognormal(size=N) * (rng.rand(N) < 0.1)
    else:
        c = rng.choice(200000, N, replace=False) - 100000
        c[c >= 0] += 1
        X[:, 0] = c
        X[:, 1] = rng.randint(1, 50000, size=N) * (rng.rand(N) < 0.1)
    d = (2, 3, 17)[(i + 2 * (i // 6)) % 3]
    X[:, 2] = (rng.randint(0, d, size=N) - d // 2) * (0.75 if is_float else 3)
    X[:, 3] = np.round(4.0 * rng.normal(size=N))
    if is_float:
        X[:, 4] = -rng.lognormal(size=N) * (rng.rand(N) < 0.5)
    else:
        X[:, 4] = -rng.randint(1, 1000, size=N) * (rng.rand(N) < 0.5)
    B = int(np.ceil((np.sqrt(8.0 * N + 1.0) - 1.0) / 2.0))          # blocks of 1, 2, 3, ... cells: B of them hold N cells
    block = np.repeat(np.arange(B), np.arange(1, B + 1))[:N]
    X[rng.permutation(N), 5] = (block - B // 2) * (0.5 if is_float else 1)
    X = X.astype(np.float32 if is_float else np.int32)
    layout = SWEEP_LAYOUTS[i % 4]
    subset = (i % 2 == 0) != (i >= 12)                              # cases 5 and 11: all 64 groups, float32 and int32
    sel = tuple(int(g) for g in rng.permutation(G)[:rng.randint(2, G + 1)]) if subset else None
    plan = dict(cap=SWEEP_CAPS[(i + i // 6) % 3], layout=layout, sel=sel, col_lb=1 if i % 8 == 0 else 0)
    for a in (X, codes):
        a.setflags(write=False)
    return X, codes.astype(np.int64), sizes.astype(np.int64), plan


@functools.lru_cache(maxsize=None)
def sweep_exact(i):
    """ranked_planes_numpy of sweep case i under its sel, from ltx_int64.  Shared: do not write to them."""
    X, codes, counts, plan = sweep_case(i)
    return ranked_planes_numpy(X, codes, counts, plan["sel"], ltx=ltx_int64)


# ---- constructed cases of tests/test_gpu_pairwise_ranked_edges.py ----
#: columns of ranked_case("f32") in the NaN window; positions 0, 5 and 11 hold continuous genes without zeros (2660 records: three
#: parts and more under pair_rank_cap 1024), the start, the middle and the end of the window, two ordinary genes and more after each but the last
NAN_COLS = (11, 10, 12, 13, 15, 14, 16, 18, 19, 21, 22, 17)
NAN_GENES = (0, 5, 11)
NAN_BITS = {"positive": 0x7FC00000, "negative": 0xFFC00000}


def nan_case(sign="positive", group=6):
    """(X float32 [2660, 12] with one NaN of that sign in each gene of NAN_GENES, in a cell of ``group``; the same matrix with 0.25 in
    those three cells; codes; counts) on the groups of ranked_case"""
    X, codes, counts = ranked_case("f32")
    clean = np.ascontiguousarray(X[:, list(NAN_COLS)])
    bad = clean.copy()
    rows = np.flatnonzero(codes == group)
    for k, j in enumerate(NAN_GENES):
        bad.view(np.uint32)[rows[5 + k], j] = NAN_BITS[sign]
        clean[rows[5 + k], j] = 0.25
    return bad, clean, codes, counts


def nan_bits_as_int32():
    """(X int32 [2660, 4], codes, counts): genes 1 and 2 of ranked_case("i32") with the bit patterns of NAN_BITS in a few cells -- for
    int32 they are ordinary values, 2143289344 and -4194304"""
    X, codes, counts = ranked_case("i32")
    Xi = np.ascontiguousarray(X[:, [0, 1, 2, 3]])
    Xi[7:2660:500, 1] = np.uint32(NAN_BITS["positive"]).view(np.int32)
    Xi[9:2660:400, 2] = np.uint32(NAN_BITS["negative"]).view(np.int32)
    Xi[11:2660:300, 2] = np.uint32(NAN_BITS["positive"]).view(np.int32)
    return Xi, codes, counts


PARTITION_SIZES = (1000, 99000, 120000, 80000)


@functools.lru_cache(maxsize=None)
def partition_case():
    """(X float32 [300000, 3], codes, counts).  Gene 1: the 300 000 values 1 + k 27 2^-23, all different, inside the binade [1, 2): the
    keys are linear in the value, so the partition's 8192 coarse buckets (k_ovr_partition: (key - kmin) >> shift) fill evenly, 37 or
    38 values each -- none crowded -- and with 1024 record slots the gene needs more than the 255 parts there are (255 x 1024 =
    261 120).  Genes 0 and 2: a twentieth of the cells non-zero.  Shared: do not write to them."""
    rng = np.random.RandomState(221)
    N = sum(PARTITION_SIZES)
    codes = rng.permutation(np.repeat(np.arange(4), PARTITION_SIZES))
    X = np.zeros((N, 3), dtype=np.float32)
    for j in (0, 2):
        X[:, j] = rng.lognormal(size=N).astype(np.float32) * (rng.rand(N) < 0.05)
    X[:, 1] = (1.0 + rng.permutation(N) * (27.0 * 2.0 ** -23)).astype(np.float32)
    for a in (X, codes):
        a.setflags(write=False)
    return X, codes.astype(np.int64), np.asarray(PARTITION_SIZES, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def partition_exact():
    X, codes, counts = partition_case()
    return ranked_planes_numpy(X, codes, counts, ltx=ltx_int64)


def float_keys(x):
    """the uint32 sort keys of float32 values (common.h: key_of): ascending with the value, -0.0 folded onto 0.0"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def coarse_buckets(keys):
    """the partition's bucket of each non-zero key when its key range is that of all of them (kernels_ovr_partition.h, OVRP_LG = 13; the
    device samples the range from an eighth of the rows: a narrower range only makes the buckets finer)"""
    kmin, kmax = int(keys.min()), int(keys.max())
    shift = max(0, (kmax - kmin).bit_length() - 13)
    return np.minimum((keys.astype(np.int64) - kmin) >> shift, 8191)


CROWDED_SIZES = (500, 1500, 1000, 1000)


@functools.lru_cache(maxsize=None)
def crowded_cases():
    """(Xf float32 [4000, 4], Xi int32 [4000, 1], codes, counts).  Xf gene 0: 3000 cells share -0.5, 300 are zero, 700 continuous
    around +-3; gene 1: 1500 cells hold -0.5 and 1500 hold +0.5, 300 zero, 700 around +-3; genes 2 and 3: gene 0 with the positive /
    the negative NaN of NAN_BITS in place of -0.5.  Xi gene 0: 3000 cells hold -5, 300 zero, 700 around +-3000.  Shared: do not
    write to them."""
    rng = np.random.RandomState(231)
    codes = rng.permutation(np.repeat(np.arange(4), CROWDED_SIZES))
    order = rng.permutation(4000)
    many, zero = order[:3000], order[3000:3300]
    cont = (3.0 + 0.1 * rng.normal(size=4000)) * rng.choice([-1.0, 1.0], size=4000)
    Xf = np.repeat(cont.astype(np.float32)[:, None], 4, axis=1)
    Xf[many, 0] = -0.5
    Xf[many[:1500], 1], Xf[many[1500:], 1] = -0.5, 0.5
    Xf.view(np.uint32)[many, 2] = NAN_BITS["positive"]
    Xf.view(np.uint32)[many, 3] = NAN_BITS["negative"]
    Xf[zero] = 0.0
    Xi = np.round(cont * 1000.0).astype(np.int32)[:, None].copy()
    Xi[many] = -5
    Xi[zero] = 0
    for a in (Xf, Xi, codes):
        a.setflags(write=False)
    return Xf, Xi, codes.astype(np.int64), np.asarray(CROWDED_SIZES, dtype=np.int64)


PADDING_SIZES = (40, 60, 1400, 1500)
#: non-zeros of genes 0 .. 10 of padding_case(): around the 64-record lane chunks and the sort's 1024-record padding
PADDING_NNZ = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)
PADDING_TOP, PADDING_BOTTOM = 11, 12


@functools.lru_cache(maxsize=None)
def padding_case():
    """(X float32 [3000, 13], codes, counts).  Gene j < 11: exactly PADDING_NNZ[j] different non-zero values of both signs among zeros.
    Gene PADDING_TOP: 2500 cells of groups 2 and 3 hold different values in [1, 2), the 100 cells of groups 0 and 1 different values
    near 1000 -- above all of them; PADDING_BOTTOM is its negative.  Shared: do not write to them."""
    rng = np.random.RandomState(241)
    N = sum(PADDING_SIZES)
    codes = rng.permutation(np.repeat(np.arange(4), PADDING_SIZES))
    X = np.zeros((N, 13), dtype=np.float32)
    for j, nnz in enumerate(PADDING_NNZ):
        u = np.unique(np.round(rng.normal(size=4 * N) * 65536.0) / 65536.0)
        u = u[u != 0]
        X[rng.permutation(N)[:nnz], j] = u[rng.choice(u.size, nnz, replace=False)]
    small = np.flatnonzero(codes < 2)
    others = rng.permutation(np.flatnonzero(codes >= 2))[:2500]
    X[others, PADDING_TOP] = 1.0 + rng.permutation(4096)[:2500] * 2.0 ** -12
    X[small, PADDING_TOP] = 1000.0 + rng.permutation(small.size) * 2.0 ** -10
    X[:, PADDING_BOTTOM] = -X[:, PADDING_TOP]
    for a in (X, codes):
        a.setflags(write=False)
    return X, codes.astype(np.int64), np.asarray(PADDING_SIZES, dtype=np.int64)


def test_the_int64_derivation_gives_the_integers_of_the_walk():
    def same(x, codes, counts, sel, what):
        S2, tie = ltx_numpy(x, codes, counts, list(sel))
        S2b, tieb = ltx_int64(x, codes, counts, sel)
        assert S2b.dtype == tieb.dtype == np.int64
        assert np.array_equal(S2.astype(np.int64), S2b) and np.array_equal(tie.astype(np.int64), tieb), what
        assert all(int(a) == int(b) for a, b in zip(tie.reshape(-1), tieb.reshape(-1))), what   # (no wrap on either side of the cast)
    for i in range(4):                                             # G = 2, 3, 7, 8; subsets in cases 0 and 2
        X, codes, counts, plan = sweep_case(i)
        sel = plan["sel"] if plan["sel"] is not None else tuple(range(counts.size))
        for j in range(X.shape[1]):
            same(X[:, j], codes, counts, sel, (i, SWEEP_GENES[j]))
    X, codes, counts = ranked_case("f32")
    for j in range(len(KINDS)):
        same(X[:, j], codes, counts, tuple(range(8)), KINDS[j])
        same(X[:, j], codes, counts, (6, 2, 5), KINDS[j])
    # the bound: at N <= 5000 every sum is below (2 x 5000)^3 = 1e12, 2^63 is 9.2e18
    assert max(int(sweep_case(i)[2].max()) for i in range(SWEEP_CASES)) <= 5000 and (2 * 5000) ** 3 < 1 << 63
    with pytest.raises(AssertionError, match="2\\^21"):
        ltx_int64(np.zeros(4), np.array([0, 0, 1, 1]), np.array([1 << 20, 2]), (0, 1))


def test_the_sweep_holds_what_it_names_and_its_references_are_well_conditioned():
    seen, sat_all, n_all = set(), 0, 0
    for i in range(SWEEP_CASES):
        X, codes, counts, plan = sweep_case(i)
        G, N = counts.size, X.shape[0]
        assert G == SWEEP_GROUPS[i % 6] and max(200, 3 * G) <= N <= 5000 and counts.sum() == N and counts.min() >= 1
        assert np.array_equal(np.bincount(codes, minlength=G), counts)
        v = X.astype(np.float64)
        assert np.unique(v[:, 0]).size == N and (v[:, 0] < 0).any() and (v[:, 0] > 0).any() and not (v[:, 0] == 0).any()
        assert v[:, 1].min() == 0 and 0.85 <= np.mean(v[:, 1] == 0) <= 0.95
        assert np.unique(v[:, 2]).size in (2, 3, 17) and v[:, 2].min() < 0 and (v[:, 2] == 0).any()
        assert np.array_equal(v[:, 3], np.round(v[:, 3])) and v[:, 3].min() < 0 < v[:, 3].max() and np.unique(v[:, 3]).size < N // 4
        assert v[:, 4].max() == 0 and 0.4 <= np.mean(v[:, 4] == 0) <= 0.6
        blocks = np.unique(v[:, 5], return_counts=True)[1]
        assert np.array_equal(blocks[:-1], np.arange(1, blocks.size)) and 1 <= blocks[-1] <= blocks.size and v[:, 5].min() < 0 < v[:, 5].max()
        sel = plan["sel"]
        assert sel is None or (2 <= len(sel) <= G and len(set(sel)) == len(sel))
        seen.add((G, X.dtype.name))
        seen.add((X.dtype.name, plan["layout"], plan["col_lb"]))
        seen.add(("cap", plan["cap"], sel is None))
        if G == 64 and sel is None:
            seen.add(("all 64", X.dtype.name))
        ex = sweep_exact(i)
        K = ex["p"].shape[0]
        keep = np.broadcast_to(offdiag(K)[:, :, None], ex["p"].shape)
        tc, p = ex["tie_corr"][keep], ex["p"][keep]
        assert not np.any((tc > 1.0e-10) & (tc < 1.0e-8)), f"case {i}: held_to_exact's own input condition"
        sat = int(np.sum((p == 0.0) | (p == 1.0)))
        print(f"sweep case {i}: {X.dtype.name}, G = {G}, K = {K}, N = {N}, {plan}: {sat / p.size:.4f} of {p.size} exact p-values are 0 or 1")
        assert sat <= 0.30 * p.size, f"case {i}"
        sat_all, n_all = sat_all + sat, n_all + p.size
    print(f"the whole sweep: {sat_all / n_all:.4f} of {n_all} exact p-values are 0 or 1")
    assert sat_all <= 0.10 * n_all
    for G in SWEEP_GROUPS:
        assert (G, "float32") in seen and (G, "int32") in seen
    for layout in SWEEP_LAYOUTS:
        assert ("float32", layout, 0) in seen and (("int32", layout, 0) in seen or ("int32", layout, 1) in seen)
    assert ("int32", "dense device", 1) in seen                    # the unaligned transposition of int32
    for cap in SWEEP_CAPS:
        assert ("cap", cap, True) in seen and ("cap", cap, False) in seen
    assert ("all 64", "float32") in seen and ("all 64", "int32") in seen


def test_the_constructed_edge_cases_hold_what_they_name():
    # NaN: one cell per gene, of the sign asked for; the clean matrix differs in those three cells only
    _, codes, counts = ranked_case("f32")
    for sign in ("positive", "negative"):
        bad, clean, _, _ = nan_case(sign, group=7 if sign == "negative" else 6)
        r, c = np.nonzero(np.isnan(bad))
        assert sorted(c.tolist()) == list(NAN_GENES) and np.all(np.signbit(bad[r, c]) == (sign == "negative"))
        assert np.all(codes[r] == (7 if sign == "negative" else 6)) and not np.isnan(clean).any()
        assert np.array_equal(np.argwhere(bad.view(np.uint32) != clean.view(np.uint32)), np.argwhere(np.isnan(bad)))
        for j in NAN_GENES:                                        # continuous, no zero: 2660 records
            assert np.unique(clean[:, j]).size >= 2650 and np.all(clean[:, j] != 0)
        k = float_keys(bad[r, c])
        assert np.all(k < 0x007FFFFF) if sign == "negative" else np.all(k > 0xFF800000)
        ok = float_keys(clean)
        assert ok.min() >= 0x007FFFFF and ok.max() <= 0xFF800000
    Xi, _, _ = nan_bits_as_int32()
    assert (Xi == 2143289344).sum() >= 6 and (Xi == -4194304).sum() >= 6
    # the partition case
    X, codes, counts = partition_case()
    assert X.shape == (300000, 3) and np.unique(X[:, 1]).size == 300000 and X[:, 1].min() == 1.0 and X[:, 1].max() < 2.0
    k = np.sort(float_keys(X[:, 1]).astype(np.int64))
    assert np.all(np.diff(k) == 27)                                # the keys are linear in the value
    fill = np.bincount(coarse_buckets(k))
    assert fill.max() <= 38 and 4 * fill.max() <= 1024             # no bucket is crowded ...
    assert 300000 > 255 * 1024                                     # ... and 255 parts of 1024 records cannot hold them
    for j in (0, 2):
        assert 0.04 < np.mean(X[:, j] != 0) < 0.06
    # crowded parts
    Xf, Xi, codes, counts = crowded_cases()
    assert (Xf[:, 0] == -0.5).sum() == 3000 and (Xf[:, 0] == 0).sum() == 300 and (Xf[:, 0] < -1).sum() > 100 and (Xf[:, 0] > 1).sum() > 100
    assert (Xf[:, 1] == -0.5).sum() == 1500 and (Xf[:, 1] == 0.5).sum() == 1500 and (Xf[:, 1] == 0).sum() == 300
    assert np.isnan(Xf[:, 2]).sum() == 3000 and not np.signbit(Xf[np.isnan(Xf[:, 2]), 2]).any()
    assert np.isnan(Xf[:, 3]).sum() == 3000 and np.signbit(Xf[np.isnan(Xf[:, 3]), 3]).all()
    assert (Xi[:, 0] == -5).sum() == 3000 and (Xi[:, 0] == 0).sum() == 300 and np.abs(Xi[Xi[:, 0] != -5, 0]).max() > 2000
    for g in range(4):                                             # every group has zeros: z_g neg_r is live
        assert (Xf[codes == g, 0] == 0).any() and (Xf[codes == g, 0] == -0.5).any()
    # the two crowded values of gene 1 fall into different coarse buckets, and neither shares its bucket with another value:
    # each is a part of its own, one tie block, and the gene is taken
    nz = Xf[:, 1][Xf[:, 1] != 0]
    b = coarse_buckets(float_keys(nz))
    b_neg, b_pos = set(b[nz == -0.5].tolist()), set(b[nz == 0.5].tolist())
    assert len(b_neg) == len(b_pos) == 1 and b_neg != b_pos and not (b_neg | b_pos) & set(b[np.abs(nz) != 0.5].tolist())
    # part sizes
    X, codes, counts = padding_case()
    for j, nnz in enumerate(PADDING_NNZ):
        col = X[:, j]
        assert np.count_nonzero(col) == nnz and np.unique(col[col != 0]).size == nnz
    small = codes < 2
    top = X[:, PADDING_TOP]
    assert small.sum() == 100 and np.unique(top[top != 0]).size == 2600 and top[small].min() > top[~small].max()
    # parts are value ranges of at most 1024 records: the 2500 records below the selected ones fill at least two parts without one
    assert np.count_nonzero(top[~small]) == 2500 and 2500 > 2 * 1024
    assert np.array_equal(X[:, PADDING_BOTTOM], -top)
