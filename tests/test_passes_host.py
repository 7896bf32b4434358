"""What the Python front ends share (illico_amd/_passes.py), on the host: the bounds of the gene windows and their halving, the matrix
hand-off to a recording stand-in for the engine, the collector of flagged genes, and the messages of the argument checks."""
import sys
import weakref

import numpy as np
import pytest
import torch
from scipy import sparse

import illico_amd  # noqa: F401
from illico_amd import _lib, _passes
from illico_amd.utils.registry import CSCDataHandler, CSRDataHandler, DenseDataHandler, KernelDataFormat


class FakeHandler:
    """A handler over a numpy or scipy container: in RAM it hands the container over whole, streaming it reads the chunk alone."""

    def __init__(self, data, streams=False, fmt=KernelDataFormat.DENSE):
        self.data, self.streams, self.fmt = data, streams, fmt

    def fetch(self, lb, ub):
        return (self.data[:, lb:ub], (0, ub - lb)) if self.streams else (self.data, (lb, ub))

    @staticmethod
    def to_nb(X):
        return X


class FakeEngine:
    """Records every method call as (name, positional arguments, keywords) and returns the name."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **kw: (self.calls.append((name, a, kw)), name)[1]


def _matrix(n_genes=150, n_cells=4):
    return np.arange(n_cells * n_genes, dtype=np.float32).reshape(n_cells, n_genes)


def _seen(X, handler, per_gene, budget):
    seen = []
    _passes.walk(X, handler, per_gene, budget, lambda chunk, o0, o1: seen.append((chunk.lb, chunk.base, o0, o1)))
    return seen


# ---- window bounds ------------------------------------------------------------------------------------------------------------------
def test_windows_of_a_matrix_in_ram():
    X = _matrix()
    assert _seen(X, FakeHandler(X), 10, 700) == [(0, 0, 0, 64), (0, 0, 64, 128), (0, 0, 128, 150)]   # 70 genes fit: 64 a window
    assert _seen(X, FakeHandler(X), 10, 1) == [(0, 0, 0, 64), (0, 0, 64, 128), (0, 0, 128, 150)]     # the floor of one tile
    assert _seen(X, FakeHandler(X), 10, 1280) == [(0, 0, 0, 128), (0, 0, 128, 150)]
    assert _seen(X[:, :0], FakeHandler(X[:, :0]), 10, 700) == []


def test_windows_of_streamed_chunks_count_from_the_chunk(monkeypatch):
    X = _matrix()
    monkeypatch.setattr(sys.modules["illico_amd.asymptotic_wilcoxon"], "STREAM_CHUNK_BYTES", 4 * 4 * 100)   # 100 genes per chunk
    chunks = list(_passes.chunks(X, FakeHandler(X, streams=True)))
    assert [(c.lb, c.width, c.base, c.streams) for c in chunks] == [(0, 100, 0, True), (100, 50, 0, True)]
    assert chunks[1].X.shape == (4, 50) and chunks[1].fetched is chunks[1].X
    assert _seen(X, FakeHandler(X, streams=True), 10, 700) == [(0, 0, 0, 64), (0, 0, 64, 100), (100, 0, 0, 50)]


# ---- halving ------------------------------------------------------------------------------------------------------------------------
def _refusing_walk(n_genes, widest, error):
    """(attempts, completed windows, the weak references that were alive at the start of an attempt) of one n_genes-wide window whose
    body refuses more than ``widest`` genes."""
    attempts, done, refs, alive = [], [], [], []

    class Scratch:
        pass

    def body(chunk, o0, o1):
        alive.extend(r for r in refs if r() is not None)
        attempts.append((o0, o1))
        scratch = Scratch()
        refs.append(weakref.ref(scratch))
        if o1 - o0 > widest:
            raise error("refused")
        done.append((o0, o1))

    X = _matrix(n_genes)
    _passes.walk(X, FakeHandler(X), 1, 1 << 20, body)                  # (the budget takes the chunk whole)
    return attempts, done, alive


@pytest.mark.parametrize("error", [MemoryError, torch.cuda.OutOfMemoryError])
def test_a_refused_window_is_halved_in_order(error):
    attempts, done, alive = _refusing_walk(256, 64, error)
    assert attempts == [(0, 256), (0, 128), (0, 64), (64, 128), (128, 256), (128, 192), (192, 256)]
    assert done == [(0, 64), (64, 128), (128, 192), (192, 256)]       # [0, 256) exactly once, in order
    assert alive == []                                                 # what a refused body made is gone when the retry starts
    attempts, done, _ = _refusing_walk(192, 128, error)
    assert attempts == [(0, 192), (0, 128), (128, 192)] and done == attempts[1:]
    attempts, done, _ = _refusing_walk(130, 128, error)                # halves are rounded up to whole tiles
    assert attempts == [(0, 130), (0, 128), (128, 130)] and done == attempts[1:]


@pytest.mark.parametrize("error", [MemoryError, torch.cuda.OutOfMemoryError])
def test_a_refused_tile_raises_the_refusal(error):
    raised = error("no room for one tile")
    attempts = []

    def body(chunk, o0, o1):
        attempts.append((o0, o1))
        raise raised

    X = _matrix(200)
    with pytest.raises(error) as caught:
        _passes.walk(X, FakeHandler(X), 1, 200, body)
    assert caught.value is raised and attempts == [(0, 192), (0, 128), (0, 64)]
    with pytest.raises(ValueError, match="not a refusal"):            # any other exception passes through at once
        _passes.walk(X, FakeHandler(X), 1, 200, lambda chunk, o0, o1: (_ for _ in ()).throw(ValueError("not a refusal")))


# ---- the matrix hand-off ------------------------------------------------------------------------------------------------------------
PASSES = {"group_stats": ("group_stats", "group_stats_sparse"), "group_moments": ("group_moments", "group_moments_sparse"),
          "group_value_hists": ("group_value_hists", "group_value_hists_sparse"), "run": ("run_dense", "run_sparse"),
          "pairwise_ranked": ("pairwise_ranked", "pairwise_ranked_sparse")}


@pytest.mark.parametrize("kind", ["dense", "csc", "csr"])
def test_each_pass_calls_the_engine_method_of_its_name(kind):
    X = _matrix(20)
    container = {"dense": X, "csc": sparse.csc_matrix(X), "csr": sparse.csr_matrix(X)}[kind]
    handler = {"dense": DenseDataHandler, "csc": CSCDataHandler, "csr": CSRDataHandler}[kind](container)
    (chunk,) = _passes.chunks(container, handler)
    assert chunk.fmt == (None if kind == "dense" else kind) and (chunk.lb, chunk.width, chunk.base) == (0, 20, 0)
    out, kw = object(), dict(is_log1p=True, rest=False, sel=None)
    for name, (dense_name, sparse_name) in PASSES.items():
        eng = FakeEngine()
        assert getattr(chunk, name)(eng, 3, 17, out=out, **kw) == (dense_name if kind == "dense" else sparse_name)
        ((called, args, kwargs),) = eng.calls
        assert kwargs == dict(out=out, **kw) and kwargs["out"] is out
        if kind == "dense":
            assert called == dense_name and args[0] is container and args[1:] == (3, 17)
        else:
            assert called == sparse_name and args[0] == kind and args[4:] == (container.shape, 3, 17)
            assert all(a is b for a, b in zip(args[1:4], (chunk.X.data, chunk.X.indices, chunk.X.indptr)))
        setattr(eng, dense_name if kind == "dense" else sparse_name, lambda *a, **k: "replaced")   # looked up when the call is made
        assert getattr(chunk, name)(eng, 0, 1) == "replaced"


def test_column_ranges_count_from_the_chunk_and_gathered_genes_are_csc():
    X = _matrix(20)
    eng = FakeEngine()
    _passes.Matrix(X, lb=100, width=8, base=10).group_stats(eng, 2, 6)
    assert eng.calls[0][1][1:] == (12, 16)
    gathered = sparse.csc_matrix(X)
    _passes.Matrix(gathered).run(eng, 0, 20, device_out=True)
    assert eng.calls[1][0] == "run_sparse" and eng.calls[1][1][0] == "csc" and eng.calls[1][2] == {"device_out": True}
    assert _passes.Matrix(gathered).width == 20 and _passes.Matrix(X).fmt is None


# ---- the flagged genes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "csc"])
@pytest.mark.parametrize("streams", [False, True])
def test_flagged_genes_of_two_chunks(monkeypatch, kind, streams):
    X = _matrix()
    container = X if kind == "dense" else sparse.csc_matrix(X)
    monkeypatch.setattr(sys.modules["illico_amd.asymptotic_wilcoxon"], "STREAM_CHUNK_BYTES", 4 * 4 * 100)
    handler = FakeHandler(container, streams, KernelDataFormat.DENSE if kind == "dense" else KernelDataFormat.CSC)
    flagged = _passes.FlaggedGenes(handler)
    assert flagged.result()[0] is None and flagged.result()[1].size == 0
    chunks = list(_passes.chunks(container, handler))
    if streams:
        assert len(chunks) == 2
        notes = [[np.array([1, 5]), np.array([70])], [np.array([3])]]
    else:
        notes = [[np.array([1, 5]), np.array([70, 103])]]
    for chunk, offsets in zip(chunks, notes):
        flagged.add(chunk, [])                                         # a chunk without a flagged gene adds nothing
        flagged.add(chunk, offsets)
    Xf, cols = flagged.result()
    assert cols.tolist() == [1, 5, 70, 103]
    if kind == "dense":
        assert isinstance(Xf, np.ndarray) and Xf.flags.c_contiguous and np.array_equal(Xf, X[:, cols])
    else:
        assert Xf.format == "csc" and np.array_equal(Xf.toarray(), X[:, cols])


@pytest.mark.parametrize("kind", ["dense", "csc", "csr"])
def test_a_matrix_flagged_whole_is_taken_as_it_is_unless_it_is_csr(kind):
    X = _matrix(20)
    container = {"dense": X, "csc": sparse.csc_matrix(X), "csr": sparse.csr_matrix(X)}[kind]
    handler = {"dense": DenseDataHandler, "csc": CSCDataHandler, "csr": CSRDataHandler}[kind](container)
    (chunk,) = _passes.chunks(container, handler)
    for whole in (True, False):
        flagged = _passes.FlaggedGenes(handler, whole=whole)
        flagged.add(chunk, [np.arange(0, 12), np.arange(12, 20)])
        Xf, cols = flagged.result()
        assert cols.tolist() == list(range(20))
        assert (Xf is container) == (whole and kind != "csr")
        assert np.array_equal(Xf.toarray() if hasattr(Xf, "toarray") else Xf, X)
        assert kind == "dense" or Xf.format == ("csc" if Xf is not container else kind)
    part = _passes.FlaggedGenes(handler, whole=True)                   # all but one gene: a copy
    part.add(chunk, [np.arange(19)])
    assert part.result()[0] is not container and part.result()[0].shape == (4, 19)


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def _message(fn, *args, **kw):
    with pytest.raises(ValueError) as caught:
        fn(*args, **kw)
    return str(caught.value)


def test_the_checks_raise_the_messages_of_the_front_ends():
    assert _passes.ALTERNATIVES == ("two-sided", "less", "greater") and _passes.VARIANTS == ("welch", "overestim_var")
    assert _message(_passes.check_bool, "is_log1p", 1) == "is_log1p must be a bool, got 1"
    assert _message(_passes.check_bool, "tie_correct", "yes") == "tie_correct must be a bool, got 'yes'"
    assert _message(_passes.check_bool, "pts", None) == "pts must be a bool, got None"
    assert _message(_passes.check_alternative, "both") == "Unsupported alternative hypothesis: both"
    assert _message(_passes.check_alternative, None) == "Unsupported alternative hypothesis: None"
    assert _message(_passes.check_variant, "student") == "variant must be one of ('welch', 'overestim_var'), got 'student'"
    for bad in (0, -3, 2.5, True):
        assert _message(_passes.check_n_genes, bad) == f"n_genes must be a positive integer or None, got {bad!r}"
    for bad in (-1, 1.5, True, None):
        assert _message(_passes.check_max_result_bytes, bad) == f"max_result_bytes must be a non-negative integer, got {bad!r}"
    wanted = ("Unknown p-value correction method 'holm': one of ['benjamini-hochberg', 'benjamini-yekutieli', 'bh', 'bonferroni', 'by']")
    assert _message(_passes.check_corr_method, "holm") == _message(_passes.check_corr_method, "holm", optional=True) == wanted
    assert _message(_passes.check_corr_method, None) == wanted.replace("'holm'", "None")
    for ok in (True, False, np.True_):
        _passes.check_bool("scores", ok)
    for alternative in _passes.ALTERNATIVES:
        _passes.check_alternative(alternative)
    for ok in (None, 1, np.int64(7)):
        _passes.check_n_genes(ok)
    for ok in (0, 8 << 30, np.int64(5)):
        _passes.check_max_result_bytes(ok)
    assert _passes.check_corr_method(None, optional=True) is None
    assert _passes.check_corr_method("BH") == _passes.check_corr_method("benjamini-hochberg", optional=True) == "bh"


# ---- the frame tails ----------------------------------------------------------------------------------------------------------------
def test_adjust_and_cut_asks_the_engine_once_per_plane(monkeypatch):
    eng = FakeEngine()
    eng.adjust_pvalues = lambda p, code, n_top=0: (eng.calls.append(("adjust_pvalues", code, n_top)), ("adj", "top") if n_top else "adj")[1]
    eng.top_by_score = lambda z, n_top: (eng.calls.append(("top_by_score", z, n_top)), "by score")[1]
    monkeypatch.setattr(_lib, "get_engine", lambda device=None: eng)
    p, z = np.zeros((2, 5)), np.ones((2, 5))
    assert _passes.adjust_and_cut(p, "bh", None) == ("adj", None)
    assert _passes.adjust_and_cut(p, "by", 9) == ("adj", "top")
    assert _passes.adjust_and_cut(p, "bh", 3, z) == ("adj", "by score")
    assert _passes.adjust_and_cut(p, "bh", None, z) == ("adj", None)
    assert eng.calls == [("adjust_pvalues", "bh", 0), ("adjust_pvalues", "by", 5), ("adjust_pvalues", "bh", 0), ("top_by_score", z, 3),
                         ("adjust_pvalues", "bh", 0)]
    adj, top = _passes.adjust_and_cut(np.zeros((3, 0)), "bh", 2)       # nothing to adjust: no engine is asked
    assert adj.shape == (3, 0) and top.shape == (3, 0) and top.dtype == np.int64 and len(eng.calls) == 5
    assert _passes.adjust_and_cut(np.zeros((0, 4)), "bh", None)[1] is None


def test_cut_rows_keeps_each_groups_rows_in_the_order_given():
    import pandas as pd
    df = pd.DataFrame({"x": np.arange(12)})
    assert _passes.cut_rows(df, np.array([[3, 0], [1, 2], [0, 3]]), 4)["x"].tolist() == [3, 0, 5, 6, 8, 11]
