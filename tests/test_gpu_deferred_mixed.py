"""ILLICO_FLAG_DEFER across kinds: a deferred dense call made while a deferred sparse call is in flight, and the other way round.

Every run entry point decides alone whether its own pass is enqueued before the earlier deferred call is completed (other planes)
or after (planes that overlap), whatever kind the earlier call was.  The inputs are those of
test_gpu_determinism.py::test_deferred_dense_calls_complete_their_leftover_genes cut to 96 genes: a gene with values of 64 and
more, a continuous gene and a fractional entry, so that both kinds leave genes to be recomputed.  The judge of a deferred call is
the plain call of its kind on the same engine, byte for byte.
"""
import numpy as np
import pytest
from scipy import sparse

import oracle
from conftest import assert_planes_match, make_counts, make_labels

pytestmark = pytest.mark.gpu

N, M, G = 6000, 96, 30
WINDOWS = [(0, M), (32, 80)]


@pytest.fixture(scope="module")
def engine():
    from illico_amd._lib import get_engine
    return get_engine()


@pytest.fixture(scope="module")
def inputs():
    X, rng = make_counts(41, N, M, 0.5)
    X[:, 7] = rng.poisson(70.0, size=N)                        # beyond the 64-value table
    X[:, 40] = np.log1p(X[:, 40] * rng.uniform(0.5, 1.5, N))   # continuous
    X[5, 60] = 0.5
    return X, make_labels(rng, N, G, n_ref=500)


def _groups(labels, test):
    return oracle.encode_and_count_groups(labels, "non-targeting" if test == "ovo" else None)[1]


def _planes(n=3):
    import torch
    return tuple(torch.full((G, M), -7.0, dtype=torch.float64, device="cuda") for _ in range(n))


def _same(got, want, lb, ub):
    """The window [lb, ub) of the planes holds the plain call's bytes; the columns outside it were not touched."""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a[:, lb:ub].cpu().numpy().tobytes() == b.tobytes()
        assert bool((a[:, :lb] == -7.0).all()) and bool((a[:, ub:] == -7.0).all())


@pytest.mark.parametrize("fmt", ["csc", "csr"])
@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_deferred_calls_of_different_kinds_on_other_planes(engine, inputs, test, fmt):
    import torch
    X, labels = inputs
    g = _groups(labels, test)
    Xd = torch.from_numpy(X).cuda()
    Ms = (sparse.csc_matrix if fmt == "csc" else sparse.csr_matrix)(X)
    d, i, p = (torch.from_numpy(a).cuda() for a in (Ms.data, Ms.indices, Ms.indptr))
    engine.set_groups(g)

    def dense(lb, ub, out=None, **kw):
        return engine.run_dense(Xd, lb, ub, out=None if out is None else tuple(t[:, lb:ub] for t in out), **kw)

    def sp(lb, ub, out=None, **kw):
        return engine.run_sparse(fmt, d, i, p, Ms.shape, lb, ub, out=None if out is None else tuple(t[:, lb:ub] for t in out), **kw)

    ref_row = g.encoded_ref_group if test == "ovo" else None
    want_oracle = oracle.run(X, g)
    for lb, ub in WINDOWS:
        want = {k: [t.cpu().numpy() for t in run(lb, ub, device_out=True, scores=True)] for k, run in (("dense", dense), ("sparse", sp))}
        for k in want:  # (the plain calls themselves are right, and the z plane changes nothing in the other three)
            assert_planes_match(want[k][:3], tuple(w[:, lb:ub] for w in want_oracle), ref_row=ref_row, what=f"plain {k} {fmt} {test}")
            for a, b in zip(want[k], (dense if k == "dense" else sp)(lb, ub, device_out=True)):
                assert a.tobytes() == b.cpu().numpy().tobytes()
        for first, second in ((sp, dense), (dense, sp)):
            w1, w2 = (want["sparse"], want["dense"]) if first is sp else (want["dense"], want["sparse"])
            # the second call sees a pending call of the other kind and other planes: its pass is enqueued first
            A, B = _planes(), _planes()
            first(lb, ub, out=A, defer=True)
            second(lb, ub, out=B, defer=True)
            first(lb, ub, out=A, defer=True)
            engine.synchronize()
            _same(A, w1[:3], lb, ub); _same(B, w2[:3], lb, ub)
            # the same pair, a fourth plane (the z-scores) on the second call
            A, B = _planes(), _planes(4)
            first(lb, ub, out=A, defer=True)
            second(lb, ub, out=B, defer=True)
            engine.synchronize()
            _same(A, w1[:3], lb, ub); _same(B, w2, lb, ub)


@pytest.mark.parametrize("test", ["ovo", "ovr"])
def test_bound_csr_window_while_a_deferred_dense_call_is_pending(engine, inputs, test):
    """"bound_ahead_genes": a 32-gene call of a bound CSR matrix computes its 64-gene window, a second one is served from that
    window; each finds a deferred dense call in flight and completes it first."""
    import torch
    X, labels = inputs
    g = _groups(labels, test)
    Xd = torch.from_numpy(X).cuda()
    Ms = sparse.csr_matrix(X)
    engine.set_groups(g)
    want_dense = [t.cpu().numpy() for t in engine.run_dense(Xd, 0, M, device_out=True)]
    want = oracle.run(X, g)
    ref_row = g.encoded_ref_group if test == "ovo" else None
    assert_planes_match(want_dense, want, ref_row=ref_row, what=f"plain dense {test}")
    bound = engine.bind_sparse("csr", Ms.data, Ms.indices, Ms.indptr, Ms.shape)
    engine.set_option("bound_ahead_genes", 64)
    try:
        for lb, ub in ((32, 64), (0, 32)):  # (the window [0, 64) is computed by the first call)
            D = _planes()
            engine.run_dense(Xd, 0, M, out=D, defer=True)
            got = bound.run(lb, ub)
            engine.synchronize()
            _same(D, want_dense, 0, M)
            assert_planes_match(got, tuple(w[:, lb:ub] for w in want), ref_row=ref_row, what=f"bound csr [{lb}, {ub}) {test}")
    finally:
        engine.set_option("bound_ahead_genes", 0)
        bound.release()
