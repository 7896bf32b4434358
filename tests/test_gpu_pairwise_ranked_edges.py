"""The ranked all-pairs Wilcoxon route (illico_pairwise_ranked_*) where tests/test_gpu_pairwise_ranked.py does not go: a seeded sweep over
group structure, value type, sel, record slots and layouts; every reason a gene leaves, on both output sides, and the genes after it;
crowded parts below zero, under sel, as int32 and of NaNs; part sizes at the sort's padding; more than one gene batch and the scratch
edge; the log1p fold change against the oracle.  The cases and their exact references are built and tested on the CPU in
tests/test_pairwise_ranked_host.py."""
import functools

import numpy as np
import pytest

from illico_amd import pairwise_wilcoxon
from illico_amd import _lib
from illico_amd._lib import get_engine
from test_pairwise_host import groups_of, held_to_exact, offdiag
from test_pairwise_ranked_host import (NAN_GENES, PADDING_NNZ, crowded_cases, ltx_int64, nan_bits_as_int32, nan_case, padding_case, partition_case,
                                       partition_exact, ranked_case, ranked_oracle_slabs, ranked_planes_numpy, sweep_case, sweep_exact, SWEEP_CASES)
from test_gpu_pairwise_ranked import _adata, _assert_references, _bits, _cap, _dev, _np, _ranked

pytestmark = pytest.mark.gpu

PLANES = "p U fc z".split()


def _filled(K, W, side):
    """the caller's (p, U, fc, z, left) on ``side``, the planes filled with 7.25 and left with 9"""
    out = tuple(np.full((K, K, W), 7.25) for _ in range(4)) + (np.full(W, 9, dtype=np.uint32 if side == "host" else np.int32),)
    return out if side == "host" else tuple(_dev(a) for a in out)


def _same_bytes(got, want, cols=None, what=""):
    """the four planes of two results agree bit for bit, in the gene columns ``cols`` (default: all)"""
    cols = slice(None) if cols is None else cols
    for a, b, name in zip(got[:4], want[:4], PLANES):
        assert np.array_equal(_bits(a[:, :, cols]), _bits(b[:, :, cols])), f"{name} {what}"


def _sub(ex, cols):
    return {k: v[:, :, cols] for k, v in ex.items()}


def _held(got, ex, what, cols=None):
    """p, U, z held to the exact planes and the fold change to float64 sums (rtol 1e-12), off the diagonal"""
    p, U, fc, z = got[:4] if cols is None else (a[:, :, cols] for a in got[:4])
    ex = ex if cols is None else _sub(ex, cols)
    K = p.shape[0]
    keep = offdiag(K)[:, :, None]
    ratios = held_to_exact(p, U, z, ex, keep, what)
    k3 = np.broadcast_to(keep, p.shape)
    np.testing.assert_allclose(fc[k3], ex["fc"][k3], rtol=1e-12, atol=0.0, equal_nan=True, err_msg=f"fold change {what}")
    return ratios


# ---- the sweep ----
@pytest.mark.parametrize("i", range(SWEEP_CASES))
def test_sweep_against_the_exact_integers(i):
    X, codes, counts, plan = sweep_case(i)
    ex = sweep_exact(i)
    sel = plan["sel"]
    lb = plan["col_lb"]
    Xin = np.ascontiguousarray(np.concatenate([X[:, -lb:], X], axis=1)) if lb else X   # (the window starts at an odd column of a wider matrix)
    eng = get_engine()
    with _cap(eng, plan["cap"]):
        got = _ranked(eng, Xin, codes, lb, lb + X.shape[1], layout=plan["layout"], **({} if sel is None else dict(sel=list(sel))))
    p, U, fc, z, left = got
    n = counts if sel is None else counts[list(sel)]
    K = n.size
    assert p.shape == (K, K, X.shape[1]) and left.shape == (X.shape[1],) and not left.any()
    rz, rp = _held(got, ex, f"sweep case {i}: {X.dtype.name}, K = {K} of {counts.size}, {X.shape[0]} cells, {plan}")
    print(f"sweep case {i}: worst error / bound: z {rz:.4g}, p {rp:.4g}")
    d = np.arange(K)
    assert np.all(p[d, d] == 1.0) and np.all(z[d, d] == 0.0) and np.array_equal(U[d, d], np.broadcast_to((n ** 2 / 2.0)[:, None], (K, X.shape[1])))
    assert np.array_equal(z, -z.transpose(1, 0, 2))


# ---- a NaN: reason 3 ----
# The window is narrower than the device has compute units, so every workgroup takes one gene; a workgroup whose gene left still
# returns to the queue's barrier and reads its next slot there (the place of the hang DESIGN.md section 20 records), and the queue
# hands the genes after a NaN gene to whichever workgroup asks next.  test_workgroups_go_on_after_genes_that_left has the wide window.
NAN_VARIANTS = {
    "positive": dict(sign="positive", group=6, sel=None, cap=0),
    "negative": dict(sign="negative", group=6, sel=None, cap=0),
    "in a group sel leaves out": dict(sign="positive", group=7, sel=(6, 2, 5), cap=0),   # the check runs before the slot filter
    "in the last of several parts": dict(sign="positive", group=6, sel=None, cap=1024),  # (its key is the largest)
    "in the first of several parts": dict(sign="negative", group=6, sel=None, cap=1024),
}


@pytest.mark.parametrize("layout", ["dense host", "dense device"])
@pytest.mark.parametrize("variant", list(NAN_VARIANTS))
def test_a_nan_gene_leaves_and_its_neighbours_do_not_change(variant, layout):
    v = NAN_VARIANTS[variant]
    bad, clean, codes, counts = nan_case(v["sign"], v["group"])
    sel = v["sel"]
    K, W, side = (len(sel) if sel else counts.size), bad.shape[1], layout.split()[1]
    kw = dict(layout=layout, **(dict(sel=list(sel)) if sel else {}))
    eng = get_engine()
    with _cap(eng, v["cap"]):
        want = _ranked(eng, clean, codes, 0, W, out=_filled(K, W, side), **kw)
        got = _ranked(eng, bad, codes, 0, W, out=_filled(K, W, side), **kw)
    nan = list(NAN_GENES)
    others = [j for j in range(W) if j not in nan]
    assert not want[4].any() and got[4][nan].tolist() == [3, 3, 3] and not got[4][others].any()
    assert all(np.all(q[:, :, nan] == 7.25) for q in got[:4])      # the caller's bytes
    _same_bytes(got, want, others, variant)
    _held(want, ranked_planes_numpy(clean, codes, counts, sel, ltx=ltx_int64), variant)


def test_workgroups_go_on_after_genes_that_left():
    """650 genes, more than the device has compute units: the workgroups whose first gene holds a NaN are back at the queue at once and
    take the genes beyond the first wave"""
    X, codes, counts = ranked_case("f32")
    clean = np.ascontiguousarray(np.tile(X, (1, 5)))
    W = clean.shape[1]
    nan = sorted(set(range(0, 256, 2)) | {300, 301, W - 1})
    bad = clean.copy()
    bad[np.flatnonzero(codes == 7)[3], nan] = np.nan
    clean[np.flatnonzero(codes == 7)[3], nan] = 0.25
    eng = get_engine()
    want = _ranked(eng, clean, codes, 0, W, out=_filled(8, W, "device"))
    got = _ranked(eng, bad, codes, 0, W, out=_filled(8, W, "device"))
    expect = np.zeros(W, dtype=got[4].dtype)
    expect[nan] = 3
    assert not want[4].any() and np.array_equal(got[4], expect)
    assert all(np.all(q[:, :, nan] == 7.25) for q in got[:4])
    others = np.flatnonzero(expect == 0)
    _same_bytes(got, want, others)
    plain = _ranked(eng, X, codes, 0, 130)                         # (held to the oracle in its own suite); the clean matrix repeats it
    for a, b, name in zip((want[0], want[1], want[3]), (plain[0], plain[1], plain[3]), "p U z".split()):
        assert np.array_equal(_bits(a[:, :, others]), _bits(b[:, :, others % 130])), name


def test_nan_bit_patterns_are_ordinary_int32_values():
    Xi, codes, counts = nan_bits_as_int32()
    ex = ranked_planes_numpy(Xi, codes, counts, ltx=ltx_int64)
    eng = get_engine()
    for layout in ("dense device", "csc host"):
        got = _ranked(eng, Xi, codes, 0, Xi.shape[1], layout=layout)
        assert not got[4].any()
        _held(got, ex, f"0x7FC00000 and 0xFFC00000 as int32, {layout}")


# ---- more parts than there are: reason 1 ----
@pytest.mark.parametrize("side", ["host", "device"])
def test_a_gene_the_partition_cannot_split_leaves_with_reason_1(side):
    X, codes, counts = partition_case()
    ex = partition_exact()
    eng = get_engine()
    with _cap(eng, 1024):
        got = _ranked(eng, X, codes, 0, 3, layout=f"dense {side}", out=_filled(4, 3, side))
    assert got[4].tolist() == [0, 1, 0]                            # (2 would mean a crowded coarse bucket: the input's fault)
    assert all(np.all(q[:, :, 1] == 7.25) for q in got[:4])
    _held(got, ex, "the neighbours of the gene that left", [0, 2])
    if side == "device":                                           # with the default slots the gene is taken
        full = _ranked(eng, X, codes, 0, 3)
        assert not full[4].any()
        rz, rp = _held(full, ex, "300 000 different values in one binade")
        print(f"300 000 different values: worst error / bound: z {rz:.4g}, p {rp:.4g}")
        _same_bytes(got, full, [0, 2])


# ---- end to end ----
def _labels(G):
    return [f"g{k:03d}" for k in range(G)]


def test_pairwise_wilcoxon_completes_nan_genes():
    bad, clean, codes, counts = nan_case("positive")
    adata = _adata(bad, codes)
    df = pairwise_wilcoxon(adata, False, "g", scores=True)
    assert (df.attrs["n_flagged_genes"], df.attrs["n_ranked_genes"], df.attrs["n_fallback_genes"]) == (12, 9, 3)
    _assert_references(df, adata, _labels(8), _labels(8), scores=True)


def test_pairwise_wilcoxon_completes_a_gene_the_partition_cannot_split():
    X, codes, counts = partition_case()
    adata = _adata(X, codes)
    eng = get_engine()
    with _cap(eng, 1024):
        df = pairwise_wilcoxon(adata, False, "g", scores=True)
    assert (df.attrs["n_flagged_genes"], df.attrs["n_ranked_genes"], df.attrs["n_fallback_genes"]) == (3, 2, 1)
    _assert_references(df, adata, _labels(4), _labels(4), scores=True)


# ---- crowded parts ----
@pytest.mark.parametrize("sel", [None, (3, 1), (2, 0, 1)])
def test_crowded_values_below_zero_in_pairs_and_of_nans(sel):
    """under 1024 record slots: 3000 cells at -0.5 among zeros (the zero correction z_g neg_r); 1500 cells each at -0.5 and +0.5, two
    coarse buckets (test_the_constructed_edge_cases_hold_what_they_name) and so two tie blocks -- the gene is taken; 3000 cells of one
    NaN pattern, positive / negative: the crowded part's own NaN check, either side"""
    Xf, _, codes, counts = crowded_cases()
    K = len(sel) if sel else 4
    kw = dict(sel=list(sel)) if sel else {}
    eng = get_engine()
    with _cap(eng, 1024):
        got = _ranked(eng, Xf, codes, 0, 4, out=_filled(K, 4, "device"), **kw)
    assert got[4].tolist() == [0, 0, 3, 3]
    assert all(np.all(q[:, :, 2:] == 7.25) for q in got[:4])
    ex = ranked_planes_numpy(Xf[:, :2], codes, counts, sel)
    _held(got, ex, f"3000 cells at -0.5; 1500 each at -0.5 and +0.5; sel {sel}", [0, 1])
    full = _ranked(eng, Xf, codes, 0, 4, out=_filled(K, 4, "device"), **kw)   # the default slots: every part is sorted
    assert full[4].tolist() == [0, 0, 3, 3] and all(np.all(q[:, :, 2:] == 7.25) for q in full[:4])
    _same_bytes(got, full, [0, 1])


@pytest.mark.parametrize("layout", ["dense device", "csc host"])
@pytest.mark.parametrize("sel", [None, (2, 0, 1)])
def test_a_crowded_negative_int32_value(sel, layout):
    _, Xi, codes, counts = crowded_cases()
    kw = dict(sel=list(sel)) if sel else {}
    eng = get_engine()
    with _cap(eng, 1024):
        got = _ranked(eng, Xi, codes, 0, 1, layout=layout, **kw)
    assert not got[4].any()
    _held(got, ranked_planes_numpy(Xi, codes, counts, sel), f"3000 cells at -5; sel {sel}")
    full = _ranked(eng, Xi, codes, 0, 1, layout=layout, **kw)
    assert not full[4].any()
    _same_bytes(got, full)


# ---- part sizes ----
@functools.lru_cache(maxsize=None)
def _padding_exact(sel):
    X, codes, counts = padding_case()
    return ranked_planes_numpy(X, codes, counts, sel, ltx=ltx_int64)


@pytest.mark.parametrize("cap", [0, 1024])
@pytest.mark.parametrize("sel", [None, (1, 0)])
def test_part_sizes_at_the_sorts_padding(sel, cap):
    """genes of exactly 0, 1, 63 .. 2049 records (one part each with the default slots); under sel of the two small groups the records
    taken are far fewer than the part's; and two genes whose selected records all lie in the top / the bottom part, so that under
    1024 slots the other parts take none"""
    X, codes, counts = padding_case()
    assert X.shape[1] == len(PADDING_NNZ) + 2
    eng = get_engine()
    with _cap(eng, cap):
        got = _ranked(eng, X, codes, 0, X.shape[1], **(dict(sel=list(sel)) if sel else {}))
    assert not got[4].any()
    _held(got, _padding_exact(sel), f"part sizes, sel {sel}, cap {cap}")


# ---- more than one batch ----
def _budget(N, G, K, W, *, host_in, host_out, staged):
    """(fixed, per_gene) bytes as pwr_run counts them (pairwise_ranked.hip), four planes.  fixed: the staged planes and left of host
    output (K^2 W 8 each, W 4), the staged sums of host input (G W 8), the group tables (G 4 + K 12) and 256.  per_gene: 10 bytes per
    row of the padded stride (keys, part keys, 16-bit codes), 256 part starts and 16 bytes of gene info, K^2 16 of statistics, and
    N 4 of the dense window when the input is staged (host or CSC).  A change of what the budget counts is meant to show here."""
    stride = (N + 63) // 64 * 64
    fixed = (K * K * W * 8 * 4 + W * 4 if host_out else 0) + (G * W * 8 if host_in else 0) + G * 4 + K * 12 + 256
    per_gene = stride * 10 + 256 * 4 + 16 + K * K * 16 + (N * 4 if staged else 0)
    return fixed, per_gene


@functools.lru_cache(maxsize=None)
def _batch_case():
    """(X float32 [2660, 133], the same with a NaN in column 70): ranked_case("f32") and three of its genes once more"""
    X, codes, counts = ranked_case("f32")
    Xw = np.ascontiguousarray(np.concatenate([X, X[:, 10:13]], axis=1))
    Xn = Xw.copy()
    Xn[np.flatnonzero(codes == 6)[11], 70] = np.nan
    for a in (Xw, Xn):
        a.setflags(write=False)
    return Xw, Xn


def _small_engine(budget):
    """a context of its own with that much scratch (the shared engine keeps its cap); its group sums come from the shared engine, whose
    passes plan their own scratch"""
    shared = get_engine()
    eng = _lib.Engine(shared.device)
    eng.set_option("scratch_bytes", budget)
    eng.group_stats, eng.group_stats_sparse = shared.group_stats, shared.group_stats_sparse
    return eng


@pytest.mark.parametrize("layout", ["dense host", "dense device", "csc host"])
@pytest.mark.parametrize("window", [(0, 130), (3, 133)])
def test_three_batches_give_the_bytes_of_one(window, layout):
    _, codes, counts = ranked_case("f32")
    Xw, Xn = _batch_case()
    lb, ub = window
    W, side = ub - lb, layout.split()[1]
    shared = get_engine()
    want = _ranked(shared, Xw, codes, lb, ub, layout=layout)         # (leaves the groups set on the shared engine)
    host = side == "host"
    fixed, per_gene = _budget(2660, 8, 8, W, host_in=host, host_out=host, staged=layout != "dense device")
    eng = _small_engine(fixed + 127 * per_gene)                      # floor(127 / 64) x 64 = 64 genes per batch: 64, 64, 2
    try:
        eng.profile(True)
        eng.profile_reset()
        got = _ranked(eng, Xw, codes, lb, ub, layout=layout)
        prof = eng.profile_get()
        eng.profile(False)
        left = _ranked(eng, Xn, codes, lb, ub, layout=layout, out=_filled(8, W, side))
    finally:
        eng.close()
    assert prof["k_pw_rank_pairs"]["launches"] == 3 and prof["k_pw_rank_emit"]["launches"] == 3, prof
    assert not want[4].any() and not got[4].any()
    _same_bytes(got, want, what=f"{layout} {window}")
    nan = 70 - lb                                                    # in the second batch
    assert left[4][nan] == 3 and np.count_nonzero(left[4]) == 1
    assert all(np.all(q[:, :, nan] == 7.25) for q in left[:4])
    _same_bytes(left, want, [j for j in range(W) if j != nan], f"beside the NaN gene, {layout} {window}")


def test_the_scratch_edge_of_one_batch_of_64_genes():
    _, codes, counts = ranked_case("f32")
    Xw, _ = _batch_case()
    shared = get_engine()
    want = _ranked(shared, Xw, codes, 0, 130, layout="dense host")
    fixed, per_gene = _budget(2660, 8, 8, 130, host_in=True, host_out=True, staged=True)
    eng = _small_engine(fixed + 64 * per_gene)
    try:
        got = _ranked(eng, Xw, codes, 0, 130, layout="dense host")
        eng.set_option("scratch_bytes", fixed + 64 * per_gene - 1)
        out = _filled(8, 130, "host")
        with pytest.raises(MemoryError, match="64 genes"):
            _ranked(eng, Xw, codes, 0, 130, layout="dense host", out=out)
    finally:
        eng.close()
    assert not got[4].any()
    _same_bytes(got, want)
    assert all(np.all(q == 7.25) for q in out[:4]) and np.all(out[4] == 9)   # refused before any write


# ---- log1p ----
LOG1P_GENES = [j for j in range(13) if j != 7]   # gene 7 holds +inf in three cells of group 6: the oracle's own expm1 sum is infinite there


@functools.lru_cache(maxsize=None)
def _log1p_run():
    """(p, U, fc, z, left) of the first 13 genes of ranked_case("f32") under is_log1p, the sums from group_stats(..., is_log1p=True)"""
    X, codes, counts = ranked_case("f32")
    eng = get_engine()
    eng.set_groups(groups_of(codes))
    Xd = _dev(np.ascontiguousarray(X[:, :13]))
    sums = eng.group_stats(Xd, 0, 13, is_log1p=True)[1]
    got = tuple(_np(a) for a in eng.pairwise_ranked(Xd, 0, 13, sums=sums, is_log1p=True, scores=True))
    assert np.isinf(np.expm1(X[codes == 6, 7].astype(np.float64)).sum())
    return got


def test_log1p_changes_nothing_but_the_fold_change():
    X, codes, counts = ranked_case("f32")
    p, U, fc, z, left = _log1p_run()
    assert not left.any()
    plain = _ranked(get_engine(), X, codes, 0, 13)
    assert np.array_equal(_bits(p), _bits(plain[0])) and np.array_equal(_bits(U), _bits(plain[1])) and np.array_equal(_bits(z), _bits(plain[3]))


def test_the_log1p_fold_change_against_the_oracle():
    """On continuous float32 values, where two float32 expm1 that are both within an ulp still disagree in the last bit of about a
    tenth of the values: with the device library's expm1f 156 of these 672 entries lay beyond rtol 1e-12, the largest relative
    difference 1.07e-8 (MI355X) -- in every route's log1p sums, not this route's alone.  The sums now take expm1 by the C library's
    own algorithm (common.h: expm1f_fdlibm), operation for operation, and give the oracle's value bit for bit."""
    fc = _log1p_run()[2]
    wfc = ranked_oracle_slabs("f32", is_log1p=True)[2][:, :, :13]
    keep = np.broadcast_to(offdiag(8)[:, :, None], (8, 8, len(LOG1P_GENES)))
    got, want = fc[:, :, LOG1P_GENES][keep], wfc[:, :, LOG1P_GENES][keep]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / np.abs(want)
    rel = rel[np.isfinite(rel)]
    print(f"log1p fold change against the oracle: {int((rel > 1e-12).sum())} of {keep.sum()} beyond rtol 1e-12, largest relative difference {rel.max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0.0, equal_nan=True)


def test_the_log1p_fold_change_within_the_accuracy_of_a_float32_expm1():
    """The bound that holds whichever float32 expm1 the oracle's C library has: each one is within 3 ulp (the OpenCL accuracy of
    expm1) or 1 ulp (the C library's), an ulp at most 2^-23 of the value.  A group's sum then differs by at most
    4 x 2^-23 x sum |expm1 x|, its mean by that over |sum expm1 x| relatively, and the fold change by the two groups' shares
    together (plus the 1e-12 of the exact case)."""
    X, codes, counts = ranked_case("f32")
    fc = _log1p_run()[2]
    wfc = ranked_oracle_slabs("f32", is_log1p=True)[2][:, :, :13]
    e = np.expm1(X[:, LOG1P_GENES].astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.stack([4.0 * 2.0 ** -23 * np.abs(e[codes == k]).sum(axis=0) / np.abs(e[codes == k].sum(axis=0)) for k in range(8)])   # [group, gene]
    share = np.where(np.isfinite(share), share, 0.0)                # (a group of zeros: both sides hold an exact 0)
    bound = 1.0e-12 + share[:, None, :] + share[None, :, :]
    keep = np.broadcast_to(offdiag(8)[:, :, None], bound.shape)
    got, want = fc[:, :, LOG1P_GENES][keep], wfc[:, :, LOG1P_GENES][keep]
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True)
    ratio = np.abs(got[fin] - want[fin]) / (np.abs(want[fin]) * bound[keep][fin] + 1e-300)
    print(f"log1p fold change: worst difference / bound {ratio.max():.3g}")
    assert ratio.max() <= 1.0
