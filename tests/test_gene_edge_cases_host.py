"""The case table of tests/gene_edge_cases.py, checked on the host: every case is what its name says -- by the restated sizing functions,
which tests/test_gpu_gene_edges.py holds against the real build --, its two sides differ in one stored entry, and its p-values stay where
a comparison at rtol 1e-12 can see a wrong statistic."""
import functools

import numpy as np
import pytest

import gene_edge_cases as ge
import oracle

PAIRS = tuple(f"{e}-{f}" for e in ge.EDGES for f in ge.FORMS)
DTYPE = {"4": np.float32, "8": np.float64, "8i": np.int64}


def _edge(pair_name):
    return ge.EDGES[pair_name.rsplit("-", 1)[0]]


@functools.lru_cache(maxsize=2)
def _pair(name):
    return ge.make(name + "-lo"), ge.make(name + "-hi")


@pytest.fixture(scope="module")
def pair(request):
    return _pair(request.param)


@pytest.fixture(scope="module")
def ovr_pair(request):
    return _pair(request.param)


ovo_pair = ranked_pair = window_pair = any_pair = ovr_pair


def pytest_generate_tests(metafunc):
    # pair: the edges carried by one boundary gene; ovr_pair / ovo_pair: those of them of one test; ranked_pair: the group-size edges
    for fixture, kinds, test in (("pair", ("gene", "window"), None), ("ovr_pair", ("gene",), "ovr"), ("ovo_pair", ("gene",), "ovo"),
                                 ("ranked_pair", ("ranked",), None), ("window_pair", ("window",), None), ("any_pair", ("gene", "window", "ranked"), None)):
        if fixture in metafunc.fixturenames:
            names = [p for p in PAIRS if _edge(p).kind in kinds and test in (None, _edge(p).test)]
            metafunc.parametrize(fixture, names, indirect=True, scope="module")


def _stored(c):
    return [int(np.count_nonzero(c.X[:, j])) for j in range(ge.N_GENES)]


def _column_values(c):
    """The boundary gene's stored values in CSC order."""
    col = c.X[:, ge.B]
    return col[col != 0]


def test_the_hand_derived_capacities_of_the_issue():
    assert [ge.csco_key_cap(9, lg, ks) for lg in (14, 13) for ks in (4, 8)] == [32680, 16338, 36776, 18386]
    assert len(ge.NAMES) == len(ge.EDGES) * 6 and len(set(ge.NAMES)) == len(ge.NAMES)


def test_shape_type_and_reproducibility(pair):
    for c in pair:
        assert c.X.shape[1] == ge.N_GENES and c.X.shape[0] <= 70000 and c.X.shape[0] == c.labels.size
        assert c.X.dtype == DTYPE[c.form] and c.width == c.X.dtype.itemsize
        again = ge.make(c.name)
        assert again.X.tobytes() == c.X.tobytes() and again.labels.tobytes() == c.labels.tobytes()
        uniq = np.unique(c.labels)
        assert uniq[0] == ge.REF_LABEL and np.array_equal(uniq, [f"g{i:05d}" for i in range(uniq.size)])
        if ge.EDGES[c.edge].kind == "window":
            assert uniq.size == ge.G_OVR
            continue
        few = c.test == "ovo" and c.edge not in ("ovo-total", "ovo-quarter", "regroup-ovo")
        assert uniq.size == (len(ge.OVO_FEW if few else ge.OVO_SIZES) if c.test == "ovo" else 4000 if c.edge == "ovr-accg-split" else ge.G_OVR)
        assert np.count_nonzero(c.X[:, ge.EMPTY]) == 0
        one = c.X[:, ge.ONE_VALUE]
        assert set(np.unique(one)) == {0.0, 4.0}
        # the window is not written out dense, whichever input form asks
        for fmt in ("csc", "csr"):
            assert not ge.written_out_dense(fmt, sum(_stored(c)), c.X.shape[0], ge.N_GENES, c.width, c.test == "ovo")


def test_the_eight_byte_form_needs_eight_byte_keys(pair):
    for c in pair:
        if c.form == "8i":   # int64 is never narrowed (SparseCall::may_narrow asks for double); the boundary gene is the float32 twin's keys
            col = c.X[:, ge.B]
            assert c.X.dtype == np.int64 and np.all((col == 0) | ((col >= 1) & (col <= 1 + 2 ** 23)))
            continue
        back = c.X.astype(np.float32).astype(c.X.dtype)
        assert np.array_equal(back[:, ge.B], c.X[:, ge.B])       # the boundary gene is the same numbers in both widths: the same ranks
        assert (c.width == 8) == bool(np.any(back != c.X))       # ... and float64 holds values float32 cannot


def test_the_two_sides_differ_in_one_entry(pair):
    lo, hi = pair
    if lo.edge == "ref-run":   # one reference cell more: the same matrix with that row taken out
        assert hi.X.shape[0] == lo.X.shape[0] + 1
        extra = [i for i in range(hi.X.shape[0]) if i >= lo.X.shape[0] or hi.labels[i] != lo.labels[i] or not np.array_equal(hi.X[i], lo.X[i])][0]
        assert hi.labels[extra] == ge.REF_LABEL and hi.X[extra, ge.B] == ge.tie_of(hi)
        assert np.array_equal(np.delete(hi.X, extra, axis=0), lo.X) and np.array_equal(np.delete(hi.labels, extra), lo.labels)
        return
    assert np.array_equal(lo.labels, hi.labels)
    diff = np.argwhere(lo.X != hi.X)
    assert diff.shape[0] == 1 and diff[0][1] == ge.B
    moved = ge.EDGES[lo.edge].test == "ovr" and lo.edge.startswith("crowd")
    assert (lo.X[tuple(diff[0])] != 0) == moved and hi.X[tuple(diff[0])] != 0


def test_ovr_column_sits_on_its_edge(ovr_pair):
    lo, hi = pair = ovr_pair
    ks, edge = lo.width, lo.edge
    G = 4000 if edge == "ovr-accg-split" else ge.G_OVR
    if edge == "regroup-ovr":   # (k_csc_ovr_gene is off: the column goes to the two-kernel route, where its length decides the regroup kernel)
        n_lo, n_hi = (_stored(c)[ge.B] for c in pair)
        assert (n_lo, n_hi) == (ge.regroup_key_cap(G, ks), ge.regroup_key_cap(G, ks) + 1) and n_lo < 1024 * ge.CSCR_CACHE
        assert set(np.unique(lo.X[:, ge.B])) == {0.0, ge.tie_of(lo)} and max(_stored(lo)) == n_lo
        return
    small = "no_csc_ovr_small_lds" not in ge.EDGES[edge].pin
    plans = []
    for c in pair:
        stored = _stored(c)
        ns = stored[ge.B]
        assert ns == max(stored) and sorted(stored)[-2] < ns          # the boundary gene is the longest column of the call: it sizes the plan
        plans.append((ns, ge.csc_ovr_plan(G, ks, ns, small), _column_values(c)))
    (n_lo, p_lo, v_lo), (n_hi, p_hi, v_hi) = plans
    assert n_hi == n_lo + (0 if edge.startswith("crowd") else 1)
    sorted_lo, sorted_hi = (any(ge.crowded(ge.bucket_occupancy(v, ks, p.lg))) for _, p, v in plans)
    takes_lo, takes_hi = ge.csc_ovr_takes(p_lo, n_lo, sorted_lo), ge.csc_ovr_takes(p_hi, n_hi, sorted_hi)
    mult_lo = np.unique(v_lo, return_counts=True)[1]
    if edge == "ovr-leave":
        assert takes_lo and not takes_hi and not sorted_lo and p_lo.accg and p_lo.g_lds == 0
        assert n_lo == {4: 36796, 8: 18396}[ks] and mult_lo.max() == 64 and np.count_nonzero(mult_lo == 64) == n_lo // 64
    elif edge in ("ovr-sorted14", "ovr-sorted13"):
        lg = int(edge[-2:])
        assert takes_lo and not takes_hi and sorted_lo and sorted_hi and p_lo.lg == p_hi.lg == lg and not p_hi.accg
        assert n_lo % ge.CSCO_CHUNK == 0 and n_lo <= p_lo.key_cap < n_lo + ge.CSCO_CHUNK and mult_lo.tolist() == [n_lo]   # one value
    else:
        assert takes_lo and takes_hi == (not edge.endswith("-cap"))    # (crowded at key_cap entries: too long for the sorted form)
        if not edge.startswith("crowd"):
            assert not sorted_lo and not sorted_hi and mult_lo.max() == 64     # the bucket form, every thread's tie partial from blocks of 64
    if edge == "ovr-accg-split":
        assert p_lo.accg and p_hi.accg and 0 < p_hi.g_lds == p_lo.g_lds - 2 and p_lo.g_lds < G and lo.info["strict_rows"] == hi.info["strict_rows"] == (p_hi.g_lds - 1, p_hi.g_lds, p_lo.g_lds - 1, p_lo.g_lds)
        codes = np.unique(lo.labels, return_inverse=True)[1].reshape(-1)
        own = lo.X[np.isin(codes, lo.info["strict_rows"]), ge.B]
        assert own.size == 40 and np.unique(own).size == 1 and own[0] != 0       # the cells of the groups at the split of either side: all stored, at one value
    elif edge == "ovr-lg":
        assert (p_lo.lg, p_hi.lg) == (14, 13) and n_lo == p_lo.key_cap and not p_hi.accg
    elif edge == "ovr-accg":
        assert (p_lo.accg, p_hi.accg) == (False, True) and n_lo == p_lo.key_cap and 0 < p_hi.g_lds < G
    elif edge == "ovr-short":
        full = ge.csc_ovr_plan(G, ks, n_lo, False)
        assert n_lo + 64 < full.key_cap and not n_hi + 64 < full.key_cap and p_lo == p_hi == full   # (at this length the short form changes nothing)
    elif edge.startswith("ovr-step"):
        step = int(edge[8:])
        assert n_lo == step and (p_lo.lg, p_hi.lg) == {1024: (11, 12), 2048: (12, 13), 4096: (13, 14)}[step]
    elif edge.startswith("crowd"):
        assert p_lo == p_hi and p_lo.lg == 14 and not p_lo.accg
        (mx_lo, avg_lo), (mx_hi, avg_hi) = (ge.crowded(ge.bucket_occupancy(v, ks, p_lo.lg)) for v in (v_lo, v_hi))
        occ_lo, occ_hi = (ge.bucket_occupancy(v, ks, p_lo.lg) for v in (v_lo, v_hi))
        assert np.count_nonzero(occ_lo) == mult_lo.size                        # every tie block alone in its bucket
        assert np.all(np.diff(np.flatnonzero(occ_lo)) > 1)                     # ... more than one bucket apart
        if "bucket" in edge:   # the largest bucket, and not the average
            assert (occ_lo.max(), occ_hi.max()) == (ge.CSCO_MAX_BUCKET, ge.CSCO_MAX_BUCKET + 1)
            assert (mx_lo, avg_lo, mx_hi, avg_hi) == (False, False, True, False)
        else:                  # the average, and not the largest bucket
            slack = ge.CSCO_MAX_AVG * n_lo - int((occ_lo.astype(np.int64) ** 2).sum())
            assert 0 <= slack < 8 and (mx_lo, avg_lo, mx_hi, avg_hi) == (False, False, False, True)
            if edge == "crowd-avg":
                assert slack == 0 and set(mult_lo) == {64}
        if edge.endswith("-cap"):
            assert n_lo == p_lo.key_cap == ge.csco_key_cap(G, 14, ks)


def test_ovo_gene_sits_on_its_edge(ovo_pair):
    lo, hi = pair = ovo_pair
    ks, edge = lo.width, lo.edge
    verdicts = []
    for c in pair:
        stats = ge.gene_stats(c)
        g = ge.groups(c.labels, "ovo")
        assert g.encoded_ref_group == 0 and g.counts[1:].max() == 256        # k_csc_gene's route: no ranked group above 256 cells
        plan = ge.csc_gene_plan(g.counts.size, ks, int(g.counts[0]), [s[0] for s in stats])
        assert plan.ref_buckets and plan.runend_cap == ge.RUNEND_MAX
        for j, s in enumerate(stats):                                          # the ordinary genes stay in the kernel on both sides
            if j != ge.B and not (edge == "ovo-quarter" and s[0] > plan.cap0):
                assert ge.csc_gene_takes(plan, *s) and s[1] <= ge.CSCG_MEDIUM - 32, (j, s)
        verdicts.append((plan, stats[ge.B], ge.csc_gene_takes(plan, *stats[ge.B])))
    (p_lo, s_lo, t_lo), (p_hi, s_hi, t_hi) = verdicts
    col = lo.X[:, ge.B]
    codes = np.unique(lo.labels, return_inverse=True)[1].reshape(-1)
    if edge in ("run-small", "run-medium"):
        edge_at = ge.CSCG_SMALL if edge == "run-small" else ge.CSCG_MEDIUM
        assert (s_lo[1], s_hi[1]) == (edge_at, edge_at + 1) and t_lo and t_hi == (edge == "run-small")
        run = col[(codes == 1) & (col != 0)]
        assert run.size == edge_at and np.all(run == ge.tie_of(lo))                   # the run is group 1's, one value
        others = np.bincount(codes[col != 0], minlength=codes.max() + 1)[2:]
        assert others.max() <= 16
    elif edge == "regroup-ovo":
        cap = ge.regroup_key_cap(len(ge.OVO_SIZES), ks)
        assert (s_lo[0], s_hi[0]) == (cap, cap + 1) and cap < 1024 * ge.CSCR_CACHE and set(np.unique(col)) == {0.0, ge.tie_of(lo)}
    elif edge == "ref-bucket":
        assert t_lo and t_hi and p_lo.ref_buckets and s_lo[2] <= ge.RUNEND_MAX
        occ_lo, occ_hi = (ge.ref_bucket_occupancy(c.X[:, ge.B][(codes == 0) & (c.X[:, ge.B] != 0)], ks) for c in pair)
        assert (occ_lo.max(), occ_hi.max()) == (ge.OVO_REF_MAX_BUCKET, ge.OVO_REF_MAX_BUCKET + 1)
        full = int(occ_lo.argmax())
        assert np.count_nonzero(occ_lo > 1) == 1 and occ_lo[full - 1] == occ_lo[full + 1] == 0    # the tie block alone in its bucket
        assert np.count_nonzero(col[codes == 0] == ge.tie_of(lo)) == ge.OVO_REF_MAX_BUCKET
        assert np.count_nonzero(col[codes != 0] == ge.tie_of(lo)) > 0                                    # ... and looked up by other groups
    elif edge == "ref-run":
        assert (s_lo[2], s_hi[2]) == (ge.RUNEND_MAX, ge.RUNEND_MAX + 1) and t_lo and not t_hi
        assert np.all(col[codes == 0] == ge.tie_of(lo)) and s_hi[0] <= p_hi.key_cap and s_hi[1] <= ge.CSCG_MEDIUM
    else:
        assert (s_lo[0], s_hi[0]) == (p_lo.key_cap, p_lo.key_cap + 1) and s_hi[1] <= ge.CSCG_MEDIUM and p_lo.key_cap == p_lo.cap0
        assert set(np.unique(col)) == {0.0, ge.tie_of(lo)} and t_lo and not t_hi
        if edge == "ovo-total":
            assert p_lo.launched and p_hi.launched
        else:
            fit = [sum(1 for j, s in enumerate(ge.gene_stats(c)) if s[0] <= p_lo.cap0) for c in pair]
            assert fit == [3, 2] and p_lo.launched and not p_hi.launched


def test_window_sits_on_the_long_column_edge(window_pair):
    lo, hi = window_pair
    ovo = lo.test == "ovo"
    L = {(4, False): 32768, (8, False): 16384, (4, True): 32768, (8, True): 32768}[(lo.width, ovo)]
    g = ge.groups(lo.labels, lo.test)
    if ovo:   # sparse_packed_rank_fits(c, true): what keeps the four-byte bound for eight-byte keys
        assert 1 <= g.counts[0] <= 65535 and g.counts[1:].max() <= 65535
    n = lo.X.shape[0]
    assert _stored(lo) == [L] * ge.N_GENES and _stored(hi) == [L + (j == ge.B) for j in range(ge.N_GENES)]
    assert set(np.unique(hi.X[:, ge.B])) == {0.0, ge.tie_of(hi)}
    for fmt in ("csc", "csr"):
        assert not ge.written_out_dense(fmt, sum(_stored(lo)), n, ge.N_GENES, lo.width, ovo)
        assert ge.written_out_dense(fmt, sum(_stored(hi)), n, ge.N_GENES, lo.width, ovo)
    # a window without the boundary gene: CSC asks the window, CSR still the whole matrix
    assert not ge.written_out_dense("csc", sum(_stored(hi)[:ge.B]), n, ge.B, lo.width, ovo)


def test_ranked_group_is_what_the_name_says(ranked_pair):
    for c, side in zip(ranked_pair, ge.SIDES):
        n_edge = ge.ranked_size(c.edge, c.width, side)
        assert n_edge == {"run-256": 256, "run-8192": 8192, "run-srt": {4: 32768, 8: 16384}[c.width]}[c.edge] + (side == "hi")
        uniq, counts = np.unique(c.labels, return_counts=True)
        assert uniq[0] == ge.REF_LABEL and tuple(counts) == (6000, n_edge) + ge.RANKED_TAIL == c.info["sizes"]
        assert c.X.shape == (counts.sum(), ge.N_GENES) and c.X.dtype == DTYPE[c.form]
        again = ge.make(c.name)
        assert again.X.tobytes() == c.X.tobytes() and again.labels.tobytes() == c.labels.tobytes()
        held = c.labels == "g00001"
        for j, v in enumerate(ge.RANKED_CONSTANTS + (int(ge.int_of(0.5)) if c.form == "8i" else 0.5,)):
            assert np.all(c.X[held, j] == v) and np.unique(c.X[~held, j]).size == 3       # the run: n keys, one tie block
        assert np.unique(c.X[:, 8]).size == c.X.shape[0]                                   # no ties at all
        if c.form == "8i":
            continue
        back = c.X.astype(np.float32).astype(c.X.dtype)
        assert (c.width == 8) == bool(np.any(back != c.X))
        if c.width == 8:   # ... between the float32 values: the same ranks as the float32 twin
            assert np.array_equal(np.argsort(c.X[:, 8], kind="stable"), np.argsort(back[:, 8], kind="stable")) and np.unique(back[:, 8]).size == c.X.shape[0]


def test_p_values_stay_where_a_comparison_can_see_them(any_pair):
    pair = any_pair
    for c in pair:
        g = ge.groups(c.labels, c.test)
        p = oracle.run(c.X, g)[0]
        rows = np.arange(g.counts.size) != g.encoded_ref_group
        sub = p[rows]
        share = np.mean((sub == 0.0) | (sub == 1.0))
        print(f"{c.name}: {100 * share:.2f} % of {sub.size} compared p-values are exactly 0 or 1")
        assert share <= ge.MAX_SHARE
        strict = np.flatnonzero(rows) if c.info["strict_rows"] is None else np.array(c.info["strict_rows"])
        own = p[strict][:, list(ge.RANKED_STRICT)] if ge.EDGES[c.edge].kind == "ranked" else p[strict, ge.B]
        assert not np.any((own == 0.0) | (own == 1.0)), (c.name, own)
        kind = ge.EDGES[c.edge].kind
        if kind != "window":   # the gene without a stored entry / the whole-column constant
            assert np.all(sub[:, 11 if kind == "ranked" else ge.EMPTY] == 1.0)
