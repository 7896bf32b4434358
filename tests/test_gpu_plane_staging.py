"""Host planes through the staged entry points (csrc/plane_stage.h): windows, null planes, pitches and the preload rule.

Every call is made twice on the module's own engine: with device planes under the module's scratch budget -- nothing is staged, one
window -- and with host planes that are column views of wider arrays under a budget worked out from the unit's own bytes per column,
so that the W = 150 columns go through in windows of 64, 64 and 22.  The kernels see the same numbers at other addresses and
pitches, so the results are compared by their bits.  The blocked calls take one window whatever the budget: theirs is the pitch, the
null plane and the preload part.

The module has an engine of its own: "scratch_bytes" has no "0 = default", and a shared engine must not keep a changed value."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from illico_amd import _lib
from illico_amd.utils.groups import encode_and_count_groups

pytestmark = pytest.mark.gpu

G, W, B, N = 6, 150, 2, 240
WINDOW = 64                      # 64 + 64 + 22 columns
DEFAULT_SCRATCH = 1 << 30
SENTINEL, REP_SENTINEL = -7.25, -77
#: the first and the last column of every window, and one inside
LEFT = np.array([0, 63, 64, 75, 127, 128, 149])


@pytest.fixture(scope="module")
def engine():
    e = _lib.Engine(0)
    e.set_option("scratch_bytes", DEFAULT_SCRATCH)
    yield e
    e.close()


class windows_of:
    """A budget of WINDOW columns (and half a column) of ``per_col`` staged bytes for the time of a block; then the module's again."""

    def __init__(self, engine, per_col):
        self.engine, self.bytes = engine, WINDOW * per_col + per_col // 2

    def __enter__(self):
        self.engine.set_option("scratch_bytes", self.bytes)

    def __exit__(self, *exc):
        self.engine.set_option("scratch_bytes", DEFAULT_SCRATCH)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def _view(a, fill=np.nan):
    """``a`` as the columns 3 .. 3 + W of an array 7 columns wider (the last axis), the rest holding ``fill``."""
    wide = np.full(a.shape[:-1] + (a.shape[-1] + 7,), fill, dtype=a.dtype)
    wide[..., 3:3 + a.shape[-1]] = a
    return wide[..., 3:3 + a.shape[-1]]


def _container(codes, n):
    _, c = encode_and_count_groups(groups=pd.Series([f"g{k:02d}" for k in codes]), ref_group=None)
    assert len(c.counts) == n
    return c._replace(encoded_ref_group=-1)


@functools.lru_cache(maxsize=None)
def _moments():
    """(the group container, S, Q, SR, QR host planes [G, W]) of a log-normalised matrix; computed once, not written to."""
    rng = np.random.default_rng(5)
    codes = rng.permutation(np.repeat(np.arange(G), N // G))
    X = np.log1p(rng.poisson(rng.uniform(0.3, 9.0, (G, W))[codes]).astype(np.float32))
    container = _container(codes, G)
    eng = _lib.Engine(0)
    try:
        eng.set_groups(container)
        planes = eng.group_moments(X, 0, W, rest=True)
    finally:
        eng.close()
    for q in planes:
        q.setflags(write=False)
    return (container, *planes)


@functools.lru_cache(maxsize=None)
def _pairs():
    """(p, t, df) host planes [G, G, W] of the pair t-test of ``_moments``; computed once, not written to."""
    container, S, Q, _, _ = _moments()
    eng = _lib.Engine(0)
    try:
        eng.set_groups(container)
        planes = eng.pair_ttest_from_moments(S, Q, want=("p", "t", "df"))
    finally:
        eng.close()
    for q in planes:
        q.setflags(write=False)
    return planes


def test_ttest_from_moments_with_null_planes(engine):
    container, S, Q, SR, QR = _moments()
    engine.set_groups(container)
    for want in (("p", "t", "df", "mean", "var", "mean_ref", "var_ref"), ("t", "var_ref")):   # the second: five null output planes
        whole = engine.ttest_from_moments(*(_dev(a) for a in (S, Q, SR, QR)), want=want)
        out = tuple(_view(np.full((G, W), SENTINEL)) for _ in want)
        with windows_of(engine, G * 8 * 4 + G * 8 * len(want)):
            got = engine.ttest_from_moments(*(_view(a) for a in (S, Q, SR, QR)), want=want, out=out)
        for name, a, b in zip(want, got, whole):
            assert np.array_equal(_bits(a), _bits(b)), name


def test_pair_ttest_from_moments_with_null_planes(engine):
    container, S, Q, _, _ = _moments()
    engine.set_groups(container)
    for want, fsum in ((("p", "t", "df", "fold_change", "cohen_d"), S), (("df", "cohen_d"), None)):   # the second: a null input, three null outputs
        n_in = 2 + (fsum is not None)
        whole = engine.pair_ttest_from_moments(_dev(S), _dev(Q), fsum=None if fsum is None else _dev(fsum), want=want)
        out = tuple(_view(np.full((G, G, W), SENTINEL)) for _ in want)
        with windows_of(engine, G * 8 * n_in + G * G * 8 * len(want)):
            got = engine.pair_ttest_from_moments(_view(S), _view(Q), fsum=None if fsum is None else _view(fsum), want=want, out=out)
        for name, a, b in zip(want, got, whole):
            assert np.array_equal(_bits(a), _bits(b)), name


def test_student_t_pvalues(engine):
    _, t, df = _pairs()
    t, df = np.ascontiguousarray(t[1, 2]), np.ascontiguousarray(df[1, 2])
    whole = engine.student_t_pvalues(_dev(t), _dev(df))
    with windows_of(engine, 24):   # t, df and p, one row
        got = engine.student_t_pvalues(t, df)
    assert np.array_equal(_bits(got), _bits(whole))


@pytest.mark.parametrize("with_skip", [False, True])
def test_combine_pairs_and_its_skipped_columns(engine, with_skip):
    p, t, df = _pairs()
    skip = np.zeros(W, dtype=np.uint32)
    if with_skip:
        skip[LEFT] = 1
    live = skip == 0
    kw = {"method": "some", "rank": 2}
    whole = engine.combine_pairs(_dev(p), (_dev(t), _dev(df)), skip=_dev(skip.astype(np.int32)) if with_skip else None, **kw)
    out = (_view(np.full((G, W), SENTINEL)), _view(np.full((G, W), REP_SENTINEL, dtype=np.int32), fill=0),
           _view(np.full((G, W), SENTINEL)), _view(np.full((G, W), SENTINEL)))
    with windows_of(engine, 3 * G * G * 8 + (4 if with_skip else 0) + 3 * G * 8 + G * 4):
        got = engine.combine_pairs(_view(p), (_view(t), _view(df)), skip=skip if with_skip else None, out=out, **kw)
    for k, (a, b) in enumerate(zip(got, whole)):
        assert np.array_equal(_bits(a)[:, live], _bits(b)[:, live]), k
        sentinel = REP_SENTINEL if k == 1 else SENTINEL
        assert (a[:, ~live] == sentinel).all() and (a[:, live] != sentinel).all(), k


@functools.lru_cache(maxsize=None)
def _blocked():
    """(H [G * B, W, 256], flags [W] with the columns LEFT flagged, the compound counts, the compound sums [G * B, W]) of a matrix of
    small counts under the compound coding g * B + b; computed once, not written to."""
    rng = np.random.default_rng(9)
    codes = rng.permutation(np.repeat(np.arange(G * B), N // (G * B)))
    X = rng.poisson(rng.uniform(0.5, 6.0, (G * B, W))[codes]).astype(np.float32)
    container = _container(codes, G * B)
    eng = _lib.Engine(0)
    try:
        eng.set_groups(container)
        H, flags = eng.group_value_hists(X, 0, W)
        sums = eng.group_stats(X, 0, W)[1]
    finally:
        eng.close()
    assert not flags.any()
    flags[LEFT] = 1
    for q in (H, flags, sums):
        q.setflags(write=False)
    return H, flags, np.asarray(container.counts, dtype=np.int64), sums


@pytest.mark.parametrize("ref", [None, 1])
def test_blocked_from_hists_and_its_flagged_columns(engine, ref):
    H, flags, counts, sums = _blocked()
    kw = {"counts": counts, "n_blocks": B, "ref": ref}
    whole = engine.blocked_from_hists(_dev(H.view(np.int32)), _dev(flags.view(np.int32)), sums=_dev(sums), **kw)
    out = tuple(_view(np.full((G, W), SENTINEL)) for _ in range(4))
    got = engine.blocked_from_hists(H, flags, sums=_view(sums), out=out, **kw)
    live = flags == 0
    for k, (a, b) in enumerate(zip(got, whole)):
        assert np.array_equal(_bits(a)[:, live], _bits(b)[:, live]), k
        assert (a[:, ~live] == SENTINEL).all() and (a[:, live] != SENTINEL).all(), k


@pytest.mark.parametrize("with_sums", [False, True])
def test_blocked_from_planes(engine, with_sums):
    _, _, counts, sums = _blocked()
    rng = np.random.default_rng(13)
    z, U = rng.normal(size=(B, G, W)), rng.uniform(0.0, 400.0, size=(B, G, W))
    row_map = np.tile(np.arange(G, dtype=np.int32), (B, 1))
    kw = {"counts": counts, "ref": None}
    whole = engine.blocked_from_planes(_dev(z), _dev(U), row_map, sums=_dev(sums) if with_sums else None, **kw)
    got = engine.blocked_from_planes(_view(z), _view(U), row_map, sums=_view(sums) if with_sums else None, **kw)   # without sums: a null plane
    assert (got[2] is None) == (not with_sums)
    for k, (a, b) in enumerate(zip(got, whole)):
        assert a is None and b is None or np.array_equal(_bits(a), _bits(b)), k
