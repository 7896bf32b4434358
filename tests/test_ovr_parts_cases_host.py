"""The case table of tests/ovr_parts_cases.py, checked on the host: by the restated plan -- which
tests/test_gpu_ovr_parts_edges.py holds against the real build -- the boundary gene of every case has the census its name says, the sides of
an edge are one key, one cell or one group apart, the ordinary genes stay on the route in every layout, and the p-values stay where a
comparison at rtol 1e-12 can see a wrong statistic."""
import numpy as np
import pytest

import gene_edge_cases as ge
import oracle
import ovr_parts_cases as oc

GROUPS = tuple(f"{e}-{f}" for e, spec in oc.EDGES.items() for f in spec.forms)
DTYPE = {"4": np.float32, "8": np.float64, "8i": np.int64}


def _sides(group):
    edge, form = group.rsplit("-", 1)
    return edge, form, [oc.make(f"{group}-{s}") for s in oc.EDGES[edge].sides]


def _models(c):
    return {lay: oc.case_model(c, lay) for lay in oc.LAYOUTS}


def test_the_restated_sizing_by_hand():
    for G in (9, 10, 86, 690):
        for lg in (13, 14):
            for ks in (4, 8):
                assert oc.key_cap_at(G, lg, ks, oc.MAX_LDS) == ge.csco_key_cap(G, lg, ks)
    # 10 groups: half of the LDS holds 16 296 four-byte keys beside 2^13 buckets (two workgroups per CU); 8 146 eight-byte keys are fewer
    # than 8192, so those take the whole LDS and 2^14 buckets
    s4, s8 = oc.sizing(10, 4, 40000, 9000), oc.sizing(10, 8, 40000, 9000)
    assert (s4.half, s4.lg, s4.key_cap, s4.K, s4.cap) == (True, 13, 16296, 15360, 15360)
    assert (s8.half, s8.lg, s8.key_cap, s8.K, s8.cap) == (False, 14, 16338, 15360, 15360)
    assert oc.key_cap_at(10, 13, 8, oc.MAX_LDS // 2) == 8146
    assert oc.sizing(10, 4, 40000, 9000, whole=True)[:4] == (True, False, 14, 32680)
    # ovr_parts_cap: rounded down to 1024, never below 1024, never above the route's own
    assert [oc.sizing(10, 4, 40000, 9000, pc).cap for pc in (1, 1023, 1024, 2047, 2048, 15360, 10 ** 6)] == [1024, 1024, 1024, 1024, 2048, 15360, 15360]
    # the driver's gate
    assert oc.sizing(10, 4, 261120, 9000, 1024).route and not oc.sizing(10, 4, 261121, 9000, 1024).route
    assert oc.sizing(10, 4, 15360 * 128, 9000).half and not oc.sizing(10, 4, 15360 * 128 + 1, 9000).half
    assert len(set(oc.NAMES)) == len(oc.NAMES) and all(oc.split(n) == (oc.make(n).edge, oc.make(n).form, oc.make(n).side) for n in oc.NAMES[:4])


def test_the_restated_keys_keep_the_order():
    v = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 1.0, 1.0000001, 7.0, np.inf])
    for ks in (4, 8):
        k = oc.keys(v, ks)
        assert k[3] == k[4] == oc.zero_key(ks) and np.all(np.diff(k.astype(object)) >= 0) and np.unique(k).size == v.size - 1
        assert np.array_equal(oc.keys(v[5:], ks), ge.keys_of(v[5:], ks))
    i = np.array([-(2 ** 40), -1, 0, 1, 2 ** 40])
    assert np.all(np.diff(oc.keys(i, 8).astype(object)) > 0) and oc.keys(i, 8)[2] == oc.zero_key(8)
    assert np.array_equal(oc.keys(i[3:], 8), ge.keys_of(i[3:], 8))
    # the grid: key offsets d are one float32 ulp from 1.0 on, the same buckets in every form and for the negatives
    d = np.array([0, 1, 1023, 1024, (oc.TOP << 10) + 5, (oc.OVRP_NB << 10) - 1])
    for sign in (1, -1):
        for form, ks in (("4", 4), ("8", 8), ("8i", 8)):
            k = oc.keys(oc.values_of(d, form, 10, sign), ks).astype(object)
            assert [int(x - k[0]) >> (29 if form == "8" else 0) for x in k] == d.tolist()


def test_the_block_layout_by_hand():
    bl = oc.lay_out_packed_blocks([16] * 640)
    assert bl.g0.size == 10 and np.all(bl.g1 - bl.g0 == 64) and np.all(bl.rows == 1024) and not bl.is_long.any() and bl.pk_len == 10240
    bl = oc.lay_out_packed_blocks([15] * 690)
    assert bl.g0.size == 10 and np.all(bl.g1 - bl.g0 == 69) and np.all(bl.rows == 1035) and np.all(bl.out == 1088 * np.arange(10))
    assert np.all(oc.lay_out_packed_blocks(oc.I_SIZES["65"]).g1 - oc.lay_out_packed_blocks(oc.I_SIZES["65"]).g0 == 65)
    lo, hi, third = (oc.lay_out_packed_blocks(oc.J_SIZES[s]) for s in ("lo", "hi", "65"))
    assert (lo.rows[0], lo.g1[0], bool(lo.is_long[0])) == (4096, 64, False)
    assert (hi.rows[0], hi.g1[0], bool(hi.is_long[0])) == (4097, 64, True)
    assert (third.rows[0], third.g1[0], bool(third.is_long[0])) == (4097, 65, False)
    k = oc.lay_out_packed_blocks(oc.K_SIZES)
    assert (k.g1 - k.g0).tolist() == [6, 66, 6, 4, 4] and k.is_long.tolist() == [True, False, False, False, False] and k.rows[0] == 4830
    assert oc.lay_out_packed_blocks([5, 7]).pk_len == 64 and oc.lay_out_packed_blocks(oc.H_SIZES).g0.size == 26


@pytest.fixture(scope="module")
def sides(request):
    return _sides(request.param)


layout_sides = sides


def pytest_generate_tests(metafunc):
    if "sides" in metafunc.fixturenames:
        metafunc.parametrize("sides", GROUPS, indirect=True, scope="module")
    if "layout_sides" in metafunc.fixturenames:   # edges H to K: the group structure, or where the keys lie in it, is the edge
        metafunc.parametrize("layout_sides", [g for g in GROUPS if g[0] in "HIJK"], indirect=True, scope="module")


def test_shape_type_and_reproducibility(sides):
    edge, form, cases = sides
    for c in cases:
        assert c.X.shape[1] == oc.N_GENES and c.X.shape[0] == c.labels.size < 262000 and c.X.dtype == DTYPE[form]
        assert np.array_equal(np.unique(c.labels), [f"g{i:05d}" for i in range(np.unique(c.labels).size)])
        assert c.opts == ({"ovr_parts_cap": 1024} if edge not in ("G", "B-own") else {})
        assert np.count_nonzero(c.X[:, oc.EMPTY]) == 0 and set(np.unique(c.X[:, oc.ONE_VALUE])) == {0, 4}
        assert c.X[:, 7].max() > 255 and c.X[:, 4].min() < 0
        if form == "8":     # float64 holds values float32 cannot (the boundary gene is the same numbers in both widths)
            back = c.X.astype(np.float32).astype(np.float64)
            assert np.array_equal(back[:, oc.B], c.X[:, oc.B]) and np.any(back[:, [0, 1, 8, 11]] != c.X[:, [0, 1, 8, 11]])
    oc.make.cache_clear()
    again = oc.make(cases[0].name)
    assert again.X.tobytes() == cases[0].X.tobytes() and again.labels.tobytes() == cases[0].labels.tobytes()


def test_the_position_maps_are_permutations(sides):
    _, _, cases = sides
    for c in cases:
        codes = oc.codes_of(c.labels)
        n = codes.size
        maps = oc.position_maps(codes)
        assert np.array_equal(np.sort(maps.plain), np.arange(n))
        assert np.unique(maps.padded).size == n and maps.padded.min() == 0 and maps.padded.max() < maps.blocks.pk_len
        # the padded rows are the plain rows with every block moved to its first slot: the same order of the cells
        assert np.array_equal(np.argsort(maps.padded), np.argsort(maps.plain))
        g = oc.groups(c.labels)
        assert np.array_equal(maps.order, g.indices) and np.array_equal(maps.posptr, g.indptr)
        ks = oc.key_size_of(c.X)
        nz = oc.keys(c.X[:, oc.B], ks) != oc.zero_key(ks)
        off, cnt = oc.packed_offsets(maps, nz)
        assert cnt.sum() == nz.sum() and np.all(off[~nz] == -1)
        slot = maps.blocks.out[maps.block_of[nz]] + off[nz]      # the packed rows: every key a slot of its own, in the order of the plain rows
        assert np.unique(slot).size == slot.size and np.array_equal(np.argsort(slot), np.argsort(maps.plain[nz]))
        assert np.all(off[nz] < cnt[maps.block_of[nz]]) and np.all(cnt <= maps.blocks.rows)


def test_the_sides_are_one_step_apart(sides):
    edge, form, cases = sides
    step = oc.EDGES[edge].step
    for lo, hi in zip(cases, cases[1:]):
        if step == "key":
            assert np.array_equal(lo.labels, hi.labels)
            diff = np.argwhere(lo.X != hi.X)
            more = 513 if hi.side == "hi2" else 1
            assert diff.shape[0] == more and np.all(diff[:, 1] == oc.B) and np.all(lo.X[diff[:, 0], oc.B] == 0) and np.unique(hi.X[diff[:, 0], oc.B]).size == 1
        elif step == "cell":
            assert hi.X.shape[0] == lo.X.shape[0] + 1 and np.array_equal(hi.X[:-1], lo.X) and np.array_equal(hi.labels[:-1], lo.labels) and hi.X[-1, oc.B] == 0
        elif step == "place" and hi.side in ("hi-out", "hi-none"):
            assert np.array_equal(cases[0].labels, hi.labels) and np.array_equal(np.sort(cases[0].X[:, oc.B]), np.sort(hi.X[:, oc.B]))
            others = [j for j in range(oc.N_GENES) if j != oc.B]
            assert np.array_equal(cases[0].X[:, others], hi.X[:, others])
    if edge == "J":   # one more cell with a key of its own: in the large group / as a 64th one-cell group
        lo = cases[0]
        for c in cases[1:]:
            assert c.X.shape[0] == lo.X.shape[0] + 1 and np.array_equal(c.X[:-1], lo.X) and c.X[-1, oc.B] != 0 and np.count_nonzero(c.X[-1]) == 1
            assert np.bincount(oc.codes_of(c.labels)).tolist() == oc.J_SIZES[c.side]
    if edge == "I":
        assert [np.bincount(oc.codes_of(c.labels)).tolist() for c in cases] == [oc.I_SIZES[c.side] for c in cases]


def test_the_ordinary_genes_stay_in_every_layout(sides):
    edge, _, cases = sides
    for c in cases:
        for lay, (sz, genes) in _models(c).items():
            assert sz.route == (c.name.split("-")[0] != "D" or c.side == "lo")
            for j, g in enumerate(genes):
                if j != oc.B:
                    assert g.stays and not g.bad and g.n <= oc.MOST, (c.name, lay, j, g)
            for coop in (False,):   # ... and without the COOP form (no_ovr_part_coop)
                assert all(g.stays for j, g in enumerate(oc.case_model(c, lay, coop=coop)[1]) if j != oc.B)
            assert all(g.stays for j, g in enumerate(oc.case_model(c, lay, whole=True)[1]) if j != oc.B)   # ovr_rank_whole


def _same_in_every_layout(c, fields=("n", "mx", "skew", "nbig", "n_parts", "empty", "bad", "streamed", "flagged", "stays")):
    ms = _models(c)
    b = [ms[lay][1][oc.B] for lay in oc.LAYOUTS]
    for f in fields:
        assert str(getattr(b[0], f)) == str(getattr(b[1], f)) == str(getattr(b[2], f)), (c.name, f)
    return ms["packed"][0], b[0]


def test_the_boundary_gene_sits_on_its_edge(sides):
    edge, form, cases = sides
    spec = oc.EDGES[edge]
    for c in cases:   # what the table's last column says, by the model
        want = spec.expect.get(c.side)
        for lay in oc.LAYOUTS:
            sz, genes = oc.case_model(c, lay)
            if want is not None:
                assert (sz.route, genes[oc.B].stays) == {"stays": (True, True), "leaves": (True, False), "no-route": (False, True)}[want], (c.name, lay)
            assert oc.leaves(c, lay) == (not sz.route or not genes[oc.B].stays)
    if edge in ("H", "I", "J", "K"):
        return
    per_side = {c.side: _same_in_every_layout(c) for c in cases}
    sz, lo = per_side["lo"]
    hi = per_side.get("hi", (None, None))[1]
    K, cap = sz.K, sz.cap
    assert K == cases[0].info["K"] == 15360 and cap == (K if edge in ("G", "B-own") else 1024) and lo.n0 > 0
    if edge == "A":
        assert (lo.mx, lo.skew, lo.quota, lo.n_parts) == (256, False, 768, 2) and (hi.mx, hi.skew, hi.nbig, hi.n_parts) == (257, True, 0, 3)
    elif edge == "B-own":   # K / 2 keys of two values: shares part 0 with nothing, the 7800 keys behind it are part 1; K / 2 + 1: a part of its own
        assert (lo.skew, lo.mx, lo.nbig, lo.sizes.tolist(), hi.mx, hi.nbig, hi.sizes.tolist()) == (True, K // 2, 0, [K // 2, 7800, 1], K // 2 + 1, 1, [0, K // 2 + 1, 7800, 1])
        assert K // 2 + 7800 > K
    elif edge.startswith("B"):
        assert lo.skew and hi.skew and (lo.mx, hi.mx) == ((512, 513) if edge != "B-adj" else (513, 513)) and hi.nbig == lo.nbig + 1 == (2 if edge == "B-adj" else 1)
        assert hi.n_parts == lo.n_parts + 1 and lo.empty == () and hi.empty == {"B": (), "B-first": (0,), "B-adj": (3,)}[edge]
        assert 513 in hi.sizes.tolist()
        own = oc.values_of(cases[1].info["d"], form)
        assert np.unique(own[(cases[1].info["d"] >> 10) == (0 if edge == "B-first" else 4001 if edge == "B-adj" else 4000)]).size == 2   # two values
    elif edge == "C":
        assert (lo.mx, lo.skew, lo.quota, lo.n, lo.n_parts, lo.bad) == (31, False, 993, 255 * 993, 255, False) and lo.sizes.max() < cap
        assert (hi.mx, hi.skew, hi.n, hi.bad) == (31, False, 255 * 993 + 1, True)
    elif edge == "D":
        assert [c.X.shape[0] for c in cases] == [261120, 261121] and cap * oc.OVRP_PMAX == 261120
    elif edge == "E":
        hi2 = per_side["hi2"][1]
        assert (lo.nbig, lo.top, lo.n_parts, lo.bad, int(lo.sizes.max())) == (127, 254, 255, False, 513) and len(lo.empty) == 127
        assert (hi.nbig, hi.bad, hi2.nbig, hi2.bad) == (128, True, 129, True) and lo.streamed == ()
    elif edge in ("F", "F-neg", "Fp", "Fp-neg"):
        assert int(lo.sizes.max()) == K and lo.streamed == lo.flagged == () and lo.stays and int(hi.sizes.max()) == K + 1
        assert (hi.streamed, hi.flagged) == (((2,), ()) if edge.startswith("F-") or edge == "F" else ((), (2,)))
        assert hi.n0 > 0 and hi.nneg == (hi.n if edge.endswith("neg") else 0)
    elif edge == "G":
        assert (lo.skew, lo.mx * 4, lo.quota, lo.n_parts, int(lo.sizes[0])) == (False, cap, cap - cap // 4, 2, cap - 1)
        assert -(-int(lo.sizes[0]) // 1024) * 1024 == cap <= sz.key_cap     # the sorted form rounds the part up to 1024: exactly cap
    elif edge == "T":
        assert (lo.skew, lo.quota, lo.n, lo.n_parts) == (False, 768, 768, 1)
        assert (hi.skew, hi.quota, hi.n, hi.n_parts, hi.sizes.tolist(), hi.empty) == (False, 768, 769, 2, [769, 0], (1,))
        ks = oc.key_size_of(cases[1].X)
        k = oc.keys(cases[1].X[:, oc.B], ks)
        k = k[k != oc.zero_key(ks)]
        assert np.bincount(oc.buckets_of(k, k)[0], minlength=oc.OVRP_NB)[-1] == 100


def test_the_layout_edges_are_what_their_names_say(layout_sides):
    edge, form, cases = layout_sides
    for c in cases:
        codes = oc.codes_of(c.labels)
        maps = oc.position_maps(codes)
        ks = oc.key_size_of(c.X)
        k = oc.keys(c.X[:, oc.B], ks)
        nz = k != oc.zero_key(ks)
        assert np.unique(k[nz]).size >= nz.sum() - (oc.H_SAMPLED if c.side == "hi-one" else 0)     # distinct values: a code off by one group changes U
        ms = _models(c)
        if edge == "H":
            anywhere = np.zeros(codes.size, dtype=bool)
            for lay in oc.LAYOUTS:
                for coop in (True, False):
                    anywhere |= oc.sampled(maps, nz, lay, coop)
            everywhere = oc.sampled_everywhere(codes, nz)
            lo_k, hi_k = k[nz].min(), k[nz].max()
            b = [ms[lay][1][oc.B] for lay in oc.LAYOUTS]
            if c.side == "lo":
                assert everywhere[k == lo_k].all() and everywhere[k == hi_k].all() and all(g.have_range and not g.skew and g.stays for g in b)
            elif c.side == "hi-out":   # the 600 smallest and the 600 largest keys: in cells that no layout samples
                order = np.argsort(k[nz])
                out = np.flatnonzero(nz)[np.concatenate([order[:oc.H_ENDS], order[-oc.H_ENDS:]])]
                assert not anywhere[out].any() and everywhere.sum() == oc.H_SAMPLED
                assert all(g.have_range and g.skew and g.mx >= oc.H_ENDS and g.stays for g in b)
            elif c.side in ("hi-none", "hi-none-big"):
                assert not anywhere.any() and all(not g.have_range and g.shift == 0 and g.sizes.tolist() == [0, g.n] for g in b)
                assert all(g.stays == (c.side == "hi-none") for g in b) and b[0].n == (oc.H_KEYS if c.side == "hi-none" else ms["packed"][0].K + 1)
            else:
                assert np.unique(k[anywhere]).size == 1 and anywhere.sum() == everywhere.sum() == oc.H_SAMPLED
                assert all(g.have_range and g.shift == 0 and g.nbig == 2 and g.stays for g in b)
            continue
        off, cnt = oc.packed_offsets(maps, nz)
        assert all(g.stays for lay in oc.LAYOUTS for g in ms[lay][1])
        if edge == "K":
            nnz = np.bincount(codes[nz], minlength=len(oc.K_SIZES))
            assert nnz.tolist() == oc.k_nnz(c.side)
            ends = [np.cumsum(nnz[a:b]) for a, b in zip(maps.blocks.g0, maps.blocks.g1)]
            if c.side in ("63", "64", "65"):
                at = int(c.side)
                assert [e[0] for e in ends[:3]] == [at] * 3 and [e[1] for e in ends[:3]] == [at + 448] * 3 and cnt[0] == at + 4032
            elif c.side == "sparse":
                assert cnt[0] == 3
            else:
                empty = np.flatnonzero(nnz == 0)
                first, last = np.isin(empty, maps.blocks.g0), np.isin(empty + 1, maps.blocks.g1)
                want = {"empty-first": first.all(), "empty-last": last.all(), "empty-mid": not (first | last).any(), "empty-two": np.all(np.diff(empty)[::2] == 1)}
                assert empty.size == (6 if c.side == "empty-two" else 3) and want[c.side]


def test_p_values_stay_where_a_comparison_can_see_them(sides):
    _, _, cases = sides
    for c in cases:
        g = oc.groups(c.labels)
        p, u, fc = oracle.run(c.X, g)
        varies = [j for j in range(oc.N_GENES) if np.unique(c.X[:, j]).size > 1]
        assert np.isfinite(p[:, varies]).all() and np.isfinite(u[:, varies]).all() and np.isfinite(fc[:, [j for j in varies if j not in (4, 9)]]).all()
        share = np.mean((p == 0.0) | (p == 1.0))
        print(f"{c.name}: {100 * share:.2f} % of {p.size} compared p-values are exactly 0 or 1")
        assert share <= oc.MAX_SHARE
        assert not np.any((p[:, oc.B] == 0.0) | (p[:, oc.B] == 1.0)), (c.name, p[:, oc.B])
