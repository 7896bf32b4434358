"""The case table of tests/threshold_cases.py, checked on the host with the CPU oracle: the inputs are what their names say, they are
reproducible, and their p-values stay inside the range where a comparison at rtol 1e-12 can see a wrong statistic."""
import numpy as np
import pytest

import oracle
import threshold_cases as tc
from conftest import make_counts, make_labels


@pytest.fixture(scope="module")
def case(request):
    return tc.make(request.param)


def pytest_generate_tests(metafunc):
    if "case" in metafunc.fixturenames:
        metafunc.parametrize("case", tc.NAMES, indirect=True, scope="module")


def test_the_table_holds_every_edge_of_the_issue():
    assert len(tc.NAMES) == 11 + 8 + 3 + 3 + 2 + 1 + 2 + 3 + 2   # the issue's table, top-255 / 256 / 257, big-16 / 17
    assert set(tc.SECOND_LINE) <= set(tc.NAMES) and len(tc.SECOND_LINE) == 10


def test_sizes_and_counts_are_what_the_name_says(case):
    kind, _, edge = case.name.partition("-")
    uniq, counts = np.unique(case.labels, return_counts=True)
    assert uniq[0] == tc.REF_LABEL and np.array_equal(uniq, [f"g{i:05d}" for i in range(uniq.size)])
    assert tuple(counts) == case.sizes
    assert case.X.shape == (counts.sum(), tc.N_GENES) and case.X.dtype == np.float32 and counts.sum() <= 72500
    tail = [300, 256, 255, 40, 16, 15, 2, 1]
    if kind == "ranked":
        assert list(counts) == [6000, int(edge)] + tail and case.boundary == (1,)
    elif kind == "top":
        assert list(counts) == [3000, int(edge), 40, 16, 15, 2, 1] and case.boundary == (1,) and counts[1:].max() == int(edge)
    elif kind == "ref":
        assert list(counts) == [int(edge)] + tail and case.boundary == (0,)
    elif kind == "singles":
        assert counts.size == int(edge) and counts[0] == 3000 and np.all(counts[1:] == 1) and case.boundary == ()
    elif kind == "forties":
        assert counts.size == int(edge) and counts[0] == 300 and np.all(counts[1:] == 40) and case.boundary == ()
    elif kind == "big":
        k = int(edge)
        assert list(counts) == [3000] + [256] * k + [17] and (counts > 255).sum() - 1 == k
        assert case.boundary == tuple(range(1, k + 1))
    elif kind == "packed":
        assert list(counts) == [255] * 131 and case.boundary == tuple(range(1, 131))
    elif kind == "cells":
        assert counts.size == 4 and counts.sum() == int(edge)
    else:
        raise AssertionError(case.name)


def test_columns_hold_what_the_design_says(case):
    X, codes = case.X, np.unique(case.labels, return_inverse=True)[1].reshape(-1)
    held = np.isin(codes, case.boundary)
    ref_edge = case.name.startswith("ref-")
    for j, v in enumerate(tc.CONSTANTS):
        assert set(np.unique(X[:, j])) <= {v - 1, v, v + 1}
        if held.any():
            assert np.all(X[held, j] == v) == (not ref_edge or j in (0, 1, 5))
        assert np.unique(X[~held, j]).size == 3
    assert set(np.unique(X[:, 7])) <= {0.25, 0.5, 0.75}
    if held.any():
        assert np.all(X[held, 7] == 0.5) == (not ref_edge)
    assert np.unique(X[:, 8]).size == X.shape[0] and X[:, 8].min() >= 0.01      # no ties at all
    nz = X[:, 9] != 0
    assert np.array_equal(X[nz, 9], X[nz, 8]) and 0.45 < nz.mean() < 0.55
    assert np.all(X[:, 10] == np.round(X[:, 10])) and X[:, 10].min() == 0 and X[:, 10].max() > 6
    assert np.all(X[:, 11] == 4.0)


def test_generating_a_case_twice_gives_identical_bytes(case):
    again = tc.make(case.name)
    assert again.X.tobytes() == case.X.tobytes()
    assert again.labels.tobytes() == case.labels.tobytes()
    assert again.boundary == case.boundary and again.sizes == case.sizes


def test_the_count_form_is_what_the_count_routes_of_csr_input_accept(case):
    """Integers in [0, 64) throughout, between 1.5 % (the dense byte windows' floor) and 30 % of the cells stored, the boundary cells of
    columns 0-2 as the case has them, the same bytes twice."""
    K = tc.count_form(case)
    assert K.shape == case.X.shape and K.dtype == np.float32 and tc.count_form(case).tobytes() == K.tobytes()
    assert np.array_equal(K, np.round(K)) and K.min() == 0 and K.max() < 64
    assert 0.015 <= np.mean(K != 0) < 0.3
    held = np.isin(np.unique(case.labels, return_inverse=True)[1].reshape(-1), case.boundary)
    assert np.array_equal(K[held, :3], case.X[held, :3])
    assert np.all((K[:, :3] == 0) | (K[:, :3] == case.X[:, :3]))
    assert np.mean(K[~held] != 0) < 1.5 * tc.COUNT_KEEP   # (at least 885 x 12 other cells in every case)


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_p_values_stay_where_a_comparison_can_see_them(case, test):
    g = tc.groups(case.labels, test)
    p = oracle.run(case.X, g)[0]
    rows = np.arange(g.counts.size) != g.encoded_ref_group
    sub = p[rows][:, list(tc.MIXED_COLUMNS)]
    share = np.mean((sub == 0.0) | (sub == 1.0))
    print(f"{case.name} {test}: {100 * share:.2f} % of {sub.size} compared p-values are exactly 0 or 1")
    assert share <= tc.MAX_SHARE
    for b in case.boundary:
        if b == g.encoded_ref_group:
            continue
        own = p[b, list(tc.STRICT_COLUMNS)]
        assert not np.any((own == 0.0) | (own == 1.0)), (b, own)
    assert np.all(p[rows][:, 11] == 1.0)   # the whole-column constant


def _scores_data(seed=5, n=700, m=70, G=6, n_ref=150):   # the data of tests/test_gpu_scores.py
    X, rng = make_counts(seed, n, m, 0.5)
    X[:, 3] = 4.0
    X[:, 7] = 0.0
    return X, make_labels(rng, n, G, n_ref=n_ref)


@pytest.mark.parametrize("test", ["ovo", "ovr"])
@pytest.mark.parametrize("tie_correct", [True, False])
def test_the_vectorised_z_is_the_loop_bit_for_bit(test, tie_correct):
    X, labels = _scores_data()
    g = oracle.encode_and_count_groups(labels, "non-targeting" if test == "ovo" else None)[1]
    U = oracle.run(X, g)[1]
    if test == "ovo":
        U[g.encoded_ref_group] = 0.0   # (the reference leaves this row unspecified)
    a, b = tc.z_want(X, g, U, tie_correct), tc.z_want_fast(X, g, U, tie_correct)
    assert np.array_equal(tc.bits(a), tc.bits(b))
    assert np.count_nonzero(a) > a.size // 2


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_the_vectorised_z_is_the_loop_on_a_threshold_case(test):
    c = tc.make("ranked-257")
    g = tc.groups(c.labels, test)
    U = oracle.run(c.X, g)[1]
    assert np.array_equal(tc.bits(tc.z_want(c.X, g, U)), tc.bits(tc.z_want_fast(c.X, g, U)))
