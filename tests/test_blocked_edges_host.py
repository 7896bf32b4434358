"""CPU tests of the builders behind tests/test_gpu_blocked_edges.py (tests/blocked_model.py): the rotated edge cases, the full-range
values, the histogram form of the model and the count-limit cases are held to what the GPU cases demand of them."""
import numpy as np
import pytest

from blocked_model import (ALTERNATIVES, LIMIT_CELLS, block_stats, blocked_model, combine, edge_case, limit_case, make_case,
                           stats_from_hists, z_block)

KINDS = ["group-absent", "reference-absent", "no-shared-block", "one-against-one", "constant-block", "constant-gene",
         "below-reference-absent"]


def _local_reference_rows(case, ref):
    """Per block that holds the reference: (its row among the groups present, as blocked.py's plane feeder finds it)."""
    rows = {}
    for b in range(case.B):
        present = np.unique(case.g_codes[case.b_codes == b])
        if ref in present:
            rows[b] = int(np.searchsorted(present, ref))
    return rows


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_rotated_edge_cases_keep_their_pattern(kind, r):
    """Group r plays the part of group 0: the same rows and values, and the n_blocks of ref = 0 rotated by r -- with a reference and
    against the rest."""
    base, case = edge_case(kind), edge_case(kind, ref=r)
    np.testing.assert_array_equal(case.X, base.X)
    np.testing.assert_array_equal(case.g_codes, (base.g_codes + r) % base.G)
    np.testing.assert_array_equal(blocked_model(*case, ref=r).n_blocks, np.roll(blocked_model(*base, ref=0).n_blocks, r))
    np.testing.assert_array_equal(blocked_model(*case).n_blocks, np.roll(blocked_model(*base).n_blocks, r))


@pytest.mark.parametrize("r", [1, 3])
def test_a_local_reference_row_differs_from_the_global_one(r):
    """What a reference other than group 0 is for: a block in which the reference has cells and a group with a smaller id has none,
    so that the reference's row among the groups present (np.searchsorted(present, ref)) is not ref.

    A rotation keeps n_blocks, so ``group-absent`` has such a block only where the absent group (2 + r) % 4 lies below r -- for r = 3,
    not for r = 1 -- and ``reference-absent`` has none that any test uses (its only incomplete block lacks the reference, and the
    plane feeder skips it; there searchsorted gives ref itself).  ``below-reference-absent`` has one for every r > 0."""
    rows = _local_reference_rows(edge_case("below-reference-absent", ref=r), r)
    assert rows[1] == r - 1 and all(rows[b] == r for b in (0, 2, 3))
    rows = _local_reference_rows(edge_case("group-absent", ref=r), r)
    assert any(row != r for row in rows.values()) == (r == 3)
    if r == 3:
        assert rows[1] == 2
    case = edge_case("reference-absent", ref=r)
    rows = _local_reference_rows(case, r)
    assert sorted(rows) == [0, 1, 3] and all(row == r for row in rows.values())
    assert int(np.searchsorted(np.unique(case.g_codes[case.b_codes == 2]), r)) == r


def _hists(case):
    G, B, W = case.G, case.B, case.X.shape[1]
    H = np.zeros((G * B, W, 256), dtype=np.uint32)
    counts = np.zeros((G, B), dtype=np.int64)
    for g in range(G):
        for b in range(B):
            rows = (case.g_codes == g) & (case.b_codes == b)
            counts[g, b] = rows.sum()
            for j in range(W):
                H[g * B + b, j] = np.bincount(case.X[rows, j].astype(np.int64), minlength=256)
    return H, counts


@pytest.mark.parametrize("ref", [None, 0, 1, 2])
def test_the_histogram_form_is_the_model(ref):
    case = make_case(3, 2, 9, values="full-range")
    H, counts = _hists(case)
    want = block_stats(case.X, case.g_codes, case.b_codes, 3, 2, ref)
    got = stats_from_hists(H, counts, ref)
    for name, x, y in zip(want._fields, got, want):
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert want.used.all()


def test_the_histogram_form_leaves_unused_blocks_out():
    case = edge_case("no-shared-block", ref=1)
    H, counts = _hists(case)
    for ref in (None, 1):
        want = block_stats(case.X, case.g_codes, case.b_codes, 4, 4, ref)
        for name, x, y in zip(want._fields, stats_from_hists(H, counts, ref), want):
            np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize("mode", ["reference", "rest"])
def test_limit_case_is_at_the_limit_and_within_the_integer_sums(mode):
    H, flags, counts, ref = limit_case(mode)
    G, B, W = 3, 2, 4
    assert H.shape == (G * B, W, 256) and H.dtype == np.uint32 and list(flags) == [0, 0, 0, 1] and (ref == 1) == (mode == "reference")
    assert (H[:, 3] == 0xFFFFFFFF).all()
    np.testing.assert_array_equal(H[:, :3].astype(np.int64).sum(axis=2), np.repeat(counts.reshape(-1, 1), 3, axis=1))
    st = stats_from_hists(H[:, :3], counts, ref)
    cells = (st.n_g + st.n_r)[st.used]
    assert cells.max() == LIMIT_CELLS == 2097151 and st.n_g[0, 0] + st.n_r[0, 0] == LIMIT_CELLS and st.used.all()
    # every tie sum fits a signed 64-bit word, the largest only just: all the cells of the largest test in one bin
    assert st.tie.max() == float(LIMIT_CELLS ** 3 - LIMIT_CELLS) and LIMIT_CELLS ** 3 - LIMIT_CELLS == 9223358842719436800 < 2 ** 63
    assert st.tie[0, 0, 0] == st.tie.max() and z_block(int(st.n_g[0, 0]), int(st.n_r[0, 0]), st.tie[0, 0, 0], st.U[0, 0, 0]) == 0.0
    # block 0 alone: gene 1 is a clear but moderate effect, gene 2 is noise
    z1 = z_block(int(st.n_g[0, 0]), int(st.n_r[0, 0]), st.tie[0, 0, 1], st.U[0, 0, 1])
    z2 = z_block(int(st.n_g[0, 0]), int(st.n_r[0, 0]), st.tie[0, 0, 2], st.U[0, 0, 2])
    assert 4.0 < z1 < 4.3 and abs(z2) < 3.0
    # every U_b is a half-integer below 2^41: the statistic, a sum of two, is exact
    assert (st.U * 2 == np.round(st.U * 2)).all() and st.U.max() < 2.0 ** 41
    rows = np.arange(G) != (-1 if ref is None else ref)
    for alternative in ALTERNATIVES:
        for tie_correct in (True, False):
            m = combine(st, ref, alternative, tie_correct)
            assert (m.p[rows] > 1e-300).all() and (m.p <= 1.0).all() and (m.n_blocks == B).all(), (alternative, tie_correct)
            if tie_correct:
                assert (m.z[:, 0] == 0).all() and (m.p[:, 0] == (1.0 if alternative == "two-sided" else 0.5))[rows].all()


@pytest.mark.parametrize("G,B,W", [(3, 2, 9), (3, 2, 65), (5, 3, 129), (3, 2, 200)])
def test_full_range_values_meet_the_demands_of_the_gpu_cases(G, B, W):
    case = make_case(G, B, W, values="full-range")
    small = make_case(G, B, W)
    assert np.array_equal(case.g_codes, small.g_codes) and np.array_equal(case.b_codes, small.b_codes)
    X = case.X
    assert X.dtype == np.float32 and (X == np.round(X)).all() and X.min() >= 0 and X.max() <= 255
    assert set(np.unique(X[:, 0])) <= set(range(248, 256)) and len(np.unique(X[:, 0])) > 1
    assert W // 2 == 1 or ((X[:, 1] % 8 == 0).all() and len(np.unique(X[:, 1])) > 8)
    assert set(np.unique(X[:, W // 2])) == {0.0, 255.0}
    for b in range(B):
        vals = np.unique(X[case.b_codes == b]).astype(np.int64)
        assert ((vals >= 6) & (vals <= 254)).sum() > 64           # bins 6 .. 254 are occupied in every block ...
        assert len(np.unique(vals // 8)) == 32                    # ... in every group of 8 the walk is unrolled by
    for ref in (None, 0, G - 1):
        st = block_stats(X, case.g_codes, case.b_codes, G, B, ref)
        for alternative in ALTERNATIVES:
            for tie_correct in (True, False):
                m = combine(st, ref, alternative, tie_correct)
                assert np.isfinite(m.p).all() and m.p.min() > 1e-300 and m.p.max() <= 1.0 and (m.n_blocks == B).all()
