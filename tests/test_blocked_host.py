"""CPU tests of the blocked Wilcoxon model (tests/blocked_model.py): held to the CPU oracle where the two overlap (one block), to an
independent form of the combination, and to the demands the GPU cases make of its builders."""
import numpy as np
import pytest
from scipy import stats

import oracle
from blocked_model import ALTERNATIVES, block_stats, blocked_model, combine, combine_planes, edge_case, make_case, z_block


def _container(g_codes, ref):
    return oracle.encode_and_count_groups(g_codes, ref)[1]


@pytest.mark.parametrize("alternative", ALTERNATIVES)
@pytest.mark.parametrize("ref", [0, None], ids=["ovo", "ovr"])
def test_one_block_is_the_oracle(ref, alternative):
    """B = 1: statistic equals the oracle's U, p the oracle's p without continuity correction, the fold change its fold change."""
    case = make_case(4, 1, 65)
    got = blocked_model(case.X, case.g_codes, np.zeros_like(case.b_codes), case.G, 1, ref, alternative)
    p, U, fc = oracle.run(case.X, _container(case.g_codes, ref), use_continuity=False, alternative=alternative)
    rows = np.arange(case.G) != (-1 if ref is None else ref)
    np.testing.assert_array_equal(got.statistic[rows], U[rows])
    np.testing.assert_allclose(got.p[rows], p[rows], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got.fold, fc, rtol=1e-12)
    assert (got.n_blocks == 1).all()
    if ref is not None:
        assert (got.p[ref] == 1).all() and (got.statistic[ref] == -1).all() and (got.z[ref] == 0).all()


def _oracle_block_z(case, ref):
    """Per-block z from the oracle alone: its one-sided p-values without continuity correction are the normal tails of -z and z
    (p_greater = sf(-z), p_less = sf(z)), inverted with scipy.stats.norm from the smaller of the two; a constant block has p = 1."""
    G, B, W = case.G, case.B, case.X.shape[1]
    z = np.zeros((G, B, W))
    for b in range(B):
        rows = np.flatnonzero(case.b_codes == b)
        present = np.unique(case.g_codes[rows])
        if present.size < 2 or (ref is not None and ref not in present):
            continue
        grp = _container(case.g_codes[rows], ref)
        pg = oracle.run(case.X[rows], grp, use_continuity=False, alternative="greater")[0]
        pl = oracle.run(case.X[rows], grp, use_continuity=False, alternative="less")[0]
        zb = np.where(pl <= pg, stats.norm.isf(pl), -stats.norm.isf(pg))
        z[present, b] = np.where((pl == 1.0) & (pg == 1.0), 0.0, zb)
    return z


@pytest.mark.parametrize("ref", [0, None], ids=["ovo", "ovr"])
@pytest.mark.parametrize("G,B,W", [(3, 3, 17), (5, 2, 9), (2, 5, 12)])
def test_model_equals_the_independent_form(G, B, W, ref):
    """Z recomputed from per-block z values that come from the oracle's p-values through scipy.stats.norm."""
    case = make_case(G, B, W)
    st = block_stats(case.X, case.g_codes, case.b_codes, G, B, ref)
    want = combine(st, ref, z_blocks=_oracle_block_z(case, ref))
    got = combine(st, ref)
    rows = np.arange(G) != (-1 if ref is None else ref)
    np.testing.assert_allclose(got.z[rows], want.z[rows], rtol=1e-12, atol=0)
    # ... and the plain formula, vectorised another way
    w = (st.n_g * st.n_r).astype(np.float64)[:, :, None]
    zb = np.array([[[0.0 if not st.used[g, b] else
                     z_block(int(st.n_g[g, b]), int(st.n_r[g, b]), st.tie[g, b, j], st.U[g, b, j])
                     for j in range(W)] for b in range(B)] for g in range(G)])
    Z = (w * zb * st.used[:, :, None]).sum(axis=1) / np.sqrt((w * w * st.used[:, :, None]).sum(axis=1))
    np.testing.assert_allclose(got.z[rows], Z[rows], rtol=1e-12, atol=1e-300)
    np.testing.assert_array_equal(got.statistic[rows], (st.U * st.used[:, :, None]).sum(axis=1)[rows])


@pytest.mark.parametrize("G", [2, 3, 5])
@pytest.mark.parametrize("B", [2, 3, 5])
def test_builders_meet_the_demands_of_the_gpu_cases(G, B):
    """The small shapes: unequal blocks, values 0 .. 5 with one gene of 0 / 255 only, and no p below 1e-300 (nor a NaN) for any
    alternative, with and without tie correction."""
    case = make_case(G, B, 65)
    sizes = np.array([[np.sum((case.g_codes == g) & (case.b_codes == b)) for b in range(B)] for g in range(G)])
    assert len(set(sizes.sum(axis=0))) == B and (sizes > 0).all()
    mid = case.X[:, 65 // 2]
    assert set(np.unique(mid)) == {0.0, 255.0} and case.X[:, np.arange(65) != 65 // 2].max() <= 5 and case.X.min() >= 0
    for ref in (0, None):
        st = block_stats(case.X, case.g_codes, case.b_codes, G, B, ref)
        for alternative in ALTERNATIVES:
            for tie_correct in (True, False):
                got = combine(st, ref, alternative, tie_correct)
                assert np.isfinite(got.p).all() and got.p.min() > 1e-300 and got.p.max() <= 1.0
                assert (got.n_blocks == B).all()


def test_blocks_that_do_not_count():
    """The edge cases say what their names say."""
    m = blocked_model(*edge_case("group-absent"), ref=0)
    assert list(m.n_blocks) == [4, 4, 3, 4] and np.isfinite(m.p).all()
    m = blocked_model(*edge_case("reference-absent"), ref=0)
    assert list(m.n_blocks) == [3, 3, 3, 3]
    m = blocked_model(*edge_case("reference-absent"))
    assert list(m.n_blocks) == [3, 4, 4, 4]
    m = blocked_model(*edge_case("no-shared-block"), ref=0)
    assert list(m.n_blocks) == [3, 3, 3, 0]
    assert np.isnan(m.p[3]).all() and np.isnan(m.statistic[3]).all() and np.isnan(m.fold[3]).all() and np.isnan(m.z[3]).all()
    case = edge_case("one-against-one")
    m = blocked_model(*case, ref=0)
    assert list(m.n_blocks) == [4, 4, 3, 3]
    st = block_stats(case.X, case.g_codes, case.b_codes, 4, 4, 0)
    assert st.n_g[1, 1] == 1 and st.n_r[1, 1] == 1 and set(np.unique(st.U[1, 1])) <= {0.0, 0.5, 1.0}
    case = edge_case("constant-block")
    st = block_stats(case.X, case.g_codes, case.b_codes, 4, 4, 0)
    n = st.n_g[1, 0] + st.n_r[1, 0]
    assert st.tie[1, 0, 1] == n ** 3 - n and st.U[1, 0, 1] == st.n_g[1, 0] * st.n_r[1, 0] / 2
    with_block = combine(st, 0)
    st3 = st._replace(used=st.used & (np.arange(4) != 0)[None, :])
    assert abs(with_block.z[1, 1]) < abs(combine(st3, 0).z[1, 1])  # z_b = 0 counts with its weight: it pulls Z towards 0
    m = blocked_model(*edge_case("constant-gene"), ref=0)
    assert (m.z[:, 2] == 0).all() and (m.p[:, 2] == 1).all()
    m = blocked_model(*edge_case("constant-gene"), alternative="greater")
    assert (m.z[:, 2] == 0).all() and (m.p[:, 2] == 0.5).all()


@pytest.mark.parametrize("ref", [0, None], ids=["ovo", "ovr"])
@pytest.mark.parametrize("kind", ["group-absent", "reference-absent", "no-shared-block", "one-against-one"])
def test_the_vectorised_combination_is_the_model(kind, ref):
    """combine_planes (the host step tools/bench_blocked.py times) on the model's own per-block z and U: the model's planes."""
    case = edge_case(kind)
    st = block_stats(case.X, case.g_codes, case.b_codes, case.G, case.B, ref)
    G, B, W = st.U.shape
    zb = np.array([[[z_block(int(st.n_g[g, b]), int(st.n_r[g, b]), st.tie[g, b, j], st.U[g, b, j]) if st.used[g, b] else 0.0
                     for j in range(W)] for g in range(G)] for b in range(B)])
    counts = np.array([[np.sum((case.g_codes == g) & (case.b_codes == b)) for b in range(B)] for g in range(G)])
    row_map = np.where(counts.T > 0, np.arange(G)[None, :], -1)
    for alternative in ALTERNATIVES:
        want = combine(st, ref, alternative)
        p, stat, z = combine_planes(zb, st.U.transpose(1, 0, 2), row_map, counts, ref, alternative)
        np.testing.assert_array_equal(stat, want.statistic)
        np.testing.assert_allclose(z, want.z, rtol=1e-12, atol=0)
        np.testing.assert_allclose(p, want.p, rtol=1e-12, atol=0)
