"""The two callers of the one OVR ranking body (ovr_rank_run, kernels_ovr_rank.h) held to each other on one matrix: as a dense matrix
through the value-range parts route (k_ovr_partition + k_ovr_rank_gene_parts, several parts per gene) and as a CSC matrix through
k_csc_ovr_gene, in the bucket form and in the forced sorted form.  The statistics are integers: the U plane and the p plane of the two
runs are identical, and both match the oracle."""
import numpy as np
import pytest
from scipy import sparse

import oracle
from conftest import assert_planes_match

N_CELLS, PARTS_CAP = 3000, 1024
SIZES = [1200, 800, 500, 300, 150, 47, 2, 1]


def one_matrix(dtype):
    """(X dense, M the same matrix as CSC with some zeros stored, labels).  No column is count-valued (those have routes of their own)
    and none leaves either route: every column fits the key slots of k_csc_ovr_gene, every part those of k_ovr_rank_gene_parts."""
    rng = np.random.RandomState(2310)
    n = N_CELLS
    labels = np.concatenate([[f"s{i:02d}"] * sz for i, sz in enumerate(SIZES)])
    rng.shuffle(labels)
    X = np.zeros((n, 12))
    X[:, 0] = np.log1p(rng.poisson(3.0, size=n) * rng.uniform(0.5, 1.5, size=n))      # spread, ~5 % exact zeros
    X[:, 1] = rng.randn(n)                                                            # fully dense, negatives
    X[:, 2] = np.where(rng.rand(n) < 0.5, 0.0, rng.lognormal(0.0, 1.0, size=n))       # half empty
    X[:, 3] = rng.poisson(2.0, size=n) + 0.5                                          # tie-heavy: crowded buckets
    X[:, 4] = 3.25                                                                    # constant
    X[:, 5] = 0.0                                                                     # all zero
    X[:, 6] = rng.rand(n) * 1e-3 + 5.0                                                # narrow range
    X[:, 7] = rng.exponential(1.0, size=n) * (rng.rand(n) < 0.9)                      # (CSC: every third entry a stored zero)
    X[:, 8] = np.round(rng.lognormal(0.0, 1.0, size=n), 2)                            # many exact repeats, wide range
    X[:, 9] = rng.standard_cauchy(size=n)                                             # heavy tails both ways
    X[:, 10] = np.where(rng.rand(n) < 0.3, -rng.rand(n), rng.rand(n) * 100)
    X[:, 11] = np.where(rng.rand(n) < 0.99, 0.0, rng.rand(n))                         # nearly empty
    M = sparse.csc_matrix(X.astype(dtype))
    M.data[M.indptr[7]:M.indptr[8]:3] = 0                                             # explicit stored zeros
    return np.ascontiguousarray(M.toarray()), M, labels


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def case(request):
    X, M, labels = one_matrix(request.param)
    _, g = oracle.encode_and_count_groups(labels, None)
    return X, M, g, oracle.run(X.astype(np.float64), g)


def test_the_input_is_what_the_gpu_test_needs(case):
    """Groups of 1 and 2 cells; stored zeros in the CSC form only; columns long enough for several parts of PARTS_CAP keys; the oracle's
    planes are finite wherever a column is not constant over all cells."""
    X, M, g, want = case
    assert sorted(g.counts.tolist()) == sorted(SIZES) and M.shape == X.shape == (N_CELLS, 12)
    assert (M.data == 0).sum() > 100 and np.array_equal(M.toarray(), X)
    nnz = (X != 0).sum(axis=0)
    assert (nnz > 2 * PARTS_CAP).sum() >= 6 and nnz[5] == 0 and 0 < nnz[11] < 100
    p, u, _ = want
    varying = [j for j in range(12) if j not in (4, 5)]
    assert np.isfinite(p[:, varying]).all() and np.isfinite(u).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sorted_form", [0, 1])
def test_dense_parts_and_csc_column_rank_alike(case, sorted_form):
    from illico_amd._lib import get_engine
    engine = get_engine()
    X, M, g, want = case
    engine.set_groups(g)
    dense_opts = {"no_fused_path": 1, "ovr_parts_cap": PARTS_CAP}
    csc_opts = {"no_dense_window_path": 1, "no_csc_counts_path": 1}
    got, prof = {}, {}
    engine.set_option("csc_ovr_sorted_form", sorted_form)
    engine.set_option("profile", 1)
    try:
        for name, opts in (("dense", dense_opts), ("csc", csc_opts)):
            for k, v in opts.items():
                engine.set_option(k, v)
            engine.profile_reset()
            try:
                if name == "dense":
                    got[name] = engine.run_dense(X, 0, X.shape[1])
                else:
                    got[name] = engine.run_sparse("csc", M.data, M.indices, M.indptr, M.shape, 0, M.shape[1])
                prof[name] = engine.profile_get()
            finally:
                for k in opts:
                    engine.set_option(k, 0)
    finally:
        engine.set_option("profile", 0)
        engine.set_option("csc_ovr_sorted_form", 0)
    assert "k_ovr_partition" in prof["dense"] and "k_ovr_rank_parts" in prof["dense"] and "k_csc_ovr_gene" not in prof["dense"], prof["dense"]
    assert "k_csc_ovr_gene" in prof["csc"] and "k_ovr_rank_parts" not in prof["csc"], prof["csc"]
    assert "k_ovr_gene" not in prof["dense"] and "k_ovr_gene" not in prof["csc"], prof   # no column left either route
    for name in ("dense", "csc"):
        assert_planes_match(got[name], want, what=f"{name} sorted_form={sorted_form}")
    np.testing.assert_array_equal(np.asarray(got["dense"][1]), np.asarray(got["csc"][1]), err_msg="U plane")
    np.testing.assert_array_equal(np.asarray(got["dense"][0]), np.asarray(got["csc"][0]), err_msg="p plane")
