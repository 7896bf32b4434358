"""ctypes binding of libillico_hip.so (include/illico_hip.h) and the Engine that owns one context.

The product path has no CPU fallback: if the HIP library is missing or no MI355X is visible the
calls below raise -- nothing here imports the CPU oracle.
"""
from __future__ import annotations

import ctypes
import functools
import os
import threading
from collections import namedtuple
from pathlib import Path

import numpy as np

_SO = Path(__file__).resolve().parent / "csrc" / "libillico_hip.so"

OK = 0
ERR_ARG, ERR_BOUNDS, ERR_ALTERNATIVE, ERR_DTYPE, ERR_NO_GROUPS, ERR_UNSORTED = -1, -2, -3, -4, -5, -6
ERR_HIP, ERR_OOM, ERR_UNSUPPORTED = -10, -11, -12

F32, F64, I32, I64 = 0, 1, 2, 3
IDX_I32, IDX_I64 = 0, 1
ALTERNATIVES = {"two-sided": 0, "less": 1, "greater": 2}
FLAG_LOG1P, FLAG_CONTINUITY, FLAG_TIE_CORRECT, FLAG_INPUT_DEVICE, FLAG_OUTPUT_DEVICE, FLAG_DEFER = 1, 2, 4, 8, 16, 32

ADJ_BH, ADJ_BY, ADJ_BONFERRONI = 0, 1, 2
ADJUST_METHODS = {"bh": ADJ_BH, "by": ADJ_BY, "bonferroni": ADJ_BONFERRONI}
#: longest row of p-values one workgroup sorts in LDS (ILLICO_ADJ_LDS_COLS); longer rows take the route through device scratch
ADJUST_LDS_COLS = 8192

TT_WELCH, TT_OVERESTIM_VAR = 0, 1
TT_VARIANTS = {"welch": TT_WELCH, "overestim_var": TT_OVERESTIM_VAR}
#: the planes illico_ttest_from_moments can write, in the order of its output arguments
TT_OUTPUTS = ("p", "t", "df", "mean", "var", "mean_ref", "var_ref")

_DTYPES = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32, np.dtype(np.int64): I64}

_vp, _i64, _ci, _str = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_char_p
# How a call names its matrix, after the context: dense (X, dtype, n_rows, n_cols, ld), CSC / CSR (data, dtype, indices, indptr,
# index dtype, n_rows, n_cols), or a bound handle ...
_DENSE, _SPARSE, _BOUND = [_vp, _vp, _ci, _i64, _i64, _i64], [_vp, _vp, _ci, _vp, _vp, _ci, _i64, _i64], [_vp, _vp]
# ... and what follows it: (col_lb, col_ub, flags, ...) and the planes with their row pitch.
_RUN = [_i64, _i64, _ci, _ci, _vp, _vp, _vp, _i64]          # alternative; p, U, fold change
_RUN_EX = _RUN[:-1] + [_vp, _i64]                            # ... and z
_GROUP = [_i64, _i64, _ci, _vp, _vp, _vp, _vp, _i64]        # four planes, any of them null
_HISTS = [_i64, _i64, _ci, _vp, _vp]                         # H, flags
_RANKED = [_i64, _i64, _vp, _i64, _vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _i64, _vp]  # sel, sums, flags, alternative; p, U, fc, z; left

#: every symbol include/illico_hip.h declares: name -> (argtypes, restype)
SIGNATURES = {
    "illico_ctx_create": ([_ci, ctypes.POINTER(_vp)], _ci),
    "illico_ctx_destroy": ([_vp], _ci),
    "illico_ctx_set_stream": ([_vp, _vp], _ci),
    "illico_ctx_set_option": ([_vp, _str, _i64], _ci),
    "illico_last_error": ([_vp], _str),
    "illico_ctx_synchronize": ([_vp], _ci),
    "illico_version": (None, _str),
    "illico_set_groups": ([_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64], _ci),
    "illico_run_dense": (_DENSE + _RUN, _ci),
    "illico_run_csc": (_SPARSE + _RUN, _ci),
    "illico_run_csr": (_SPARSE + _RUN, _ci),
    "illico_run_bound": (_BOUND + _RUN, _ci),
    "illico_run_dense_ex": (_DENSE + _RUN_EX, _ci),
    "illico_run_csc_ex": (_SPARSE + _RUN_EX, _ci),
    "illico_run_csr_ex": (_SPARSE + _RUN_EX, _ci),
    "illico_run_bound_ex": (_BOUND + _RUN_EX, _ci),
    "illico_csr_bind": (_SPARSE + [_ci, ctypes.POINTER(_vp)], _ci),
    "illico_csc_bind": (_SPARSE + [_ci, ctypes.POINTER(_vp)], _ci),
    "illico_matrix_release": ([_vp, _vp], _ci),
    "illico_matrix_touch": ([_vp, _vp], _ci),
    "illico_csr_indices_sorted": ([_vp, _vp, _vp, _ci, _i64, _ci, ctypes.POINTER(_ci)], _ci),
    "illico_rank_statistics": (_DENSE + [_i64, _i64, _ci, _vp, _vp, _vp], _ci),
    "illico_planes_to_host": ([_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64], _ci),
    "illico_adjust_pvalues": ([_vp, _vp, _i64, _i64, _i64, _ci, _ci, _vp, _i64, _i64, _vp, _i64], _ci),
    "illico_top_by_score": ([_vp, _vp, _i64, _i64, _i64, _ci, _i64, _vp, _i64], _ci),
    "illico_group_stats_dense": (_DENSE + _GROUP, _ci),
    "illico_group_stats_csc": (_SPARSE + _GROUP, _ci),
    "illico_group_stats_csr": (_SPARSE + _GROUP, _ci),
    "illico_group_stats_bound": (_BOUND + _GROUP, _ci),
    "illico_group_moments_dense": (_DENSE + _GROUP, _ci),
    "illico_group_moments_csc": (_SPARSE + _GROUP, _ci),
    "illico_group_moments_csr": (_SPARSE + _GROUP, _ci),
    "illico_group_moments_bound": (_BOUND + _GROUP, _ci),
    "illico_ttest_from_moments": ([_vp] * 5 + [_i64, _i64, _ci, _ci, _ci] + [_vp] * 7 + [_i64], _ci),
    "illico_student_t_pvalues": ([_vp, _vp, _vp, _i64, _ci, _ci, _vp], _ci),
    "illico_group_value_hists_dense": (_DENSE + _HISTS, _ci),
    "illico_group_value_hists_csc": (_SPARSE + _HISTS, _ci),
    "illico_group_value_hists_csr": (_SPARSE + _HISTS, _ci),
    "illico_pairwise_from_hists": ([_vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _ci, _ci, _vp, _vp, _vp, _vp, _i64], _ci),
    "illico_profile_num_kernels": ([], _ci),
    "illico_profile_kernel_name": ([_ci], _str),
    "illico_profile_get": ([_vp, _ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_i64)], _ci),
    "illico_profile_reset": ([_vp], _ci),
    "illico_profile_input_bytes": ([_vp, ctypes.POINTER(_i64)], _ci),
}
SYMBOLS = list(SIGNATURES)
#: the symbols include/illico_hip_ranked.h declares (the ranked pair route), exported by the same library
RANKED_SIGNATURES = {
    "illico_pairwise_ranked_dense": (_DENSE + _RANKED, _ci),
    "illico_pairwise_ranked_csc": (_SPARSE + _RANKED, _ci),
}
#: the symbol include/illico_hip_markers.h declares (per-group marker statistics), exported by the same library:
#: p, four effect planes; K, W, pitch; skip; method, rank_j, flags; p, rep, four selected effect planes; pitch
MARKER_SIGNATURES = {
    "illico_combine_pairs": ([_vp] * 6 + [_i64, _i64, _i64, _vp, _ci, _i64, _ci] + [_vp] * 6 + [_i64], _ci),
}
COMBINE_METHODS = {"all": 0, "any": 1, "some": 2}
#: the symbols include/illico_hip_blocked.h declares (blocked Wilcoxon tests), exported by the same library:
#: from_hists: H, flags, counts; G, B, W, ref; sums, pitch; flags, alternative; p, statistic, fold change, z; pitch
#: from_planes: z, U, pitch; row map, counts; G, B, W, ref; sums, pitch; flags, alternative; p, statistic, fold change, z; pitch
BLOCKED_SIGNATURES = {
    "illico_blocked_from_hists": ([_vp] * 4 + [_i64] * 4 + [_vp, _i64, _ci, _ci] + [_vp] * 4 + [_i64], _ci),
    "illico_blocked_from_planes": ([_vp] * 3 + [_i64, _vp, _vp] + [_i64] * 4 + [_vp, _i64, _ci, _ci] + [_vp] * 4 + [_i64], _ci),
}
#: groups illico_combine_pairs takes at most (ILLICO_COMBINE_MAX_GROUPS), effect planes it selects at most
COMBINE_MAX_GROUPS, COMBINE_MAX_EFFECTS = 256, 4
#: the symbol include/illico_hip_pair_ttest.h declares (all-pairs Welch t-tests from moment planes), exported by the same library:
#: sum, sumsq, fsum; n_cols, pitch; sel, K; variant, alternative, flags; p, t, df, fold change, Cohen's d; pitch
PAIR_TTEST_SIGNATURES = {
    "illico_pair_ttest_from_moments": ([_vp] * 4 + [_i64, _i64, _vp, _i64, _ci, _ci, _ci] + [_vp] * 5 + [_i64], _ci),
}
#: the planes illico_pair_ttest_from_moments can write, in the order of its output arguments
PAIR_TT_OUTPUTS = ("p", "t", "df", "fold_change", "cohen_d")
#: the kernel's tiles (kernels_pair_ttest.h: PT_TILE genes, PT_GT groups) and the groups one launch takes at most
PAIR_TT_GENE_TILE, PAIR_TT_GROUP_TILE, PAIR_TT_MAX_GROUPS = 64, 8, 2880

_lib = None
_lock = threading.Lock()


def load() -> ctypes.CDLL:
    """Load libillico_hip.so; raises if it has not been built (python -m illico_amd.csrc.build)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not _SO.exists():
            raise ImportError(
                f"{_SO} is missing: the HIP engine has not been built. Run `python __graft_entry__.py` or "
                "`python illico_amd/csrc/build.py`. There is no CPU fallback.")
        lib = ctypes.CDLL(str(_SO))
        for name, (argtypes, restype) in {**SIGNATURES, **RANKED_SIGNATURES, **MARKER_SIGNATURES, **BLOCKED_SIGNATURES,
                                          **PAIR_TTEST_SIGNATURES}.items():  # a symbol the library lacks fails here, not at first use
            f = getattr(lib, name)
            f.argtypes, f.restype = argtypes, restype
        _lib = lib
        return lib


def _raise(code: int, msg: str):
    if code in (ERR_ARG, ERR_BOUNDS, ERR_ALTERNATIVE, ERR_NO_GROUPS, ERR_UNSORTED):
        raise ValueError(msg)
    if code == ERR_DTYPE:
        raise KeyError(msg)
    if code == ERR_OOM:
        raise MemoryError(msg)
    if code == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(f"illico_hip error {code}: {msg}")


def _is_torch_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


class _Buf:
    """A host ndarray or a device torch.Tensor seen as (pointer, on_device, keepalive)."""

    def __init__(self, x, dtype=None):
        if _is_torch_tensor(x):
            if not x.is_contiguous():
                raise ValueError("device tensors must be contiguous")
            self.on_device = x.is_cuda
            self.ptr = x.data_ptr()
            self.keep = x
            self.np_dtype = np.dtype(str(x.dtype).replace("torch.", ""))
        else:
            a = np.ascontiguousarray(x, dtype=dtype)
            self.on_device = False
            self.ptr = a.ctypes.data
            self.keep = a
            self.np_dtype = a.dtype


def dtype_code(np_dtype) -> int:
    try:
        return _DTYPES[np.dtype(np_dtype)]
    except KeyError as e:
        raise KeyError(f"Support for element dtype {np_dtype} is not implemented.") from e


def normalize_values(a: np.ndarray) -> np.ndarray:
    """Host arrays of dtypes the engine has no kernel for are widened losslessly (order and equality kept)."""
    dt = a.dtype
    if dt in _DTYPES:
        return a
    if dt == np.float16:
        return a.astype(np.float32)
    if dt.kind == "b" or (dt.kind in "iu" and dt.itemsize < 4):
        return a.astype(np.int32)
    if dt == np.uint32:
        return a.astype(np.int64)
    if dt == np.uint64:
        if a.size and a.max() > np.iinfo(np.int64).max:
            raise KeyError("uint64 values above 2**63-1 are not supported.")
        return a.astype(np.int64)
    raise KeyError(f"Support for element dtype {dt} is not implemented.")


def _torch():
    """torch, imported at first need: importing this module does not import it."""
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _name(dtype) -> str:
    """The name of a dtype a caller here asks for ("float64" for np.float64), which torch gives it too.  (``np.dtype(...).name`` costs
    microseconds; never for the dtype of an array that came in: names do not tell byte orders apart.)"""
    return np.dtype(dtype).name


def _dtype_name(t) -> str:
    """The element type of a torch tensor as numpy names it ("float64")."""
    return str(t.dtype).replace("torch.", "")


def _has_dtype(x, *dtypes) -> bool:
    """Whether the elements of ``x`` are exactly of one of the numpy ``dtypes``: a numpy array by its dtype itself, so that another
    byte order is another type; a tensor by the name of its own."""
    return x.dtype in dtypes if isinstance(x, np.ndarray) else _dtype_name(x) in [_name(d) for d in dtypes]


def _ptr(x):
    """The address of the first element of a numpy array or a torch tensor; None stays None."""
    return None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def _empty(shape, dtype, device=None):
    """An uninitialised numpy array, or with ``device`` (a torch device or its name) a tensor there."""
    if device is None:
        return np.empty(shape, dtype=dtype)
    return _torch().empty(tuple(shape), dtype=getattr(_torch(), _name(dtype)), device=device)


def _host_or_cuda(x, what) -> bool:
    """Whether ``x`` is a CUDA tensor; ``ValueError`` unless it is that or a numpy array."""
    if isinstance(x, np.ndarray):
        return False
    if not _is_torch_tensor(x):
        raise ValueError(f"{what} must be a numpy array or a CUDA tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise ValueError(f"{what} must be a numpy array or a CUDA tensor (got a CPU tensor)")
    return True


def _row_pitch(x):
    """The row pitch in elements of the 2-D array or tensor ``x`` if the C side can walk it -- unit column stride where it has more
    than one column; where it has more than one row, a row stride of a whole number of elements, at least the columns, so that
    rows do not overlap -- else None.  The pitch of a single row is its length."""
    rows, cols = x.shape
    (s0, s1), unit = (x.strides, x.itemsize) if isinstance(x, np.ndarray) else (x.stride(), 1)
    if (cols > 1 and s1 != unit) or (rows > 1 and (s0 % unit or s0 < cols * unit)):
        return None
    return int(s0 // unit if rows > 1 else cols)


_Plane = namedtuple("_Plane", "array ptr rows cols pitch on_device")


def _plane(x, what, *, dtype=np.float64, shape=None, copy_ok=False, writeable=False):
    """The ``_Plane`` of a [rows, cols] numpy array or CUDA tensor of exactly ``dtype`` (and ``shape``, if given) that ``_row_pitch``
    can walk.  A host array it cannot walk is copied with ``copy_ok`` and refused without; a device tensor is never copied.
    ``writeable``: refuse a read-only host array.  Every refusal is a ``ValueError``."""
    on_dev = _host_or_cuda(x, what)
    if not _has_dtype(x, dtype) or len(x.shape) != 2 or (shape is not None and tuple(x.shape) != tuple(shape)):
        raise ValueError(f"{what} must be a {np.dtype(dtype).name} 2-D plane{'' if shape is None else f' of shape {tuple(shape)}'}, "
                         f"got {x.dtype} of shape {tuple(x.shape)}")
    pitch = _row_pitch(x)
    if pitch is None:
        if on_dev or not copy_ok:
            raise ValueError(f"{what} must have unit column stride and rows that do not overlap")
        x = np.ascontiguousarray(x)
        pitch = x.shape[1]
    if writeable and not on_dev and not x.flags.writeable:
        raise ValueError(f"{what} must be writeable")
    return _Plane(x, _ptr(x), int(x.shape[0]), int(x.shape[1]), pitch, on_dev)


def _plane_set(planes, what):
    """``(pointers, FLAG_OUTPUT_DEVICE or 0, row pitch)`` of ``_Plane`` records the C side takes with one pitch: all on one side, all
    of one pitch.  A None entry gives a None pointer; the pitch of no planes at all is None."""
    given = [q for q in planes if q is not None]
    if len({q.on_device for q in given}) > 1:
        raise ValueError(f"{what} must all live on the same side (host or device)")
    if len({q.pitch for q in given}) > 1:
        raise ValueError(f"{what} must share one row stride")
    return ([None if q is None else q.ptr for q in planes], FLAG_OUTPUT_DEVICE if given and given[0].on_device else 0,
            given[0].pitch if given else None)


def _block(x, what, dtypes, shape, *, on_device=None, writeable=False):
    """``(pointer, on the device)`` of a contiguous numpy array or CUDA tensor of exactly ``shape`` whose element type is one of
    ``dtypes`` (numpy's).  ``on_device``: the side it must be on, if not None.  ``writeable``: refuse a read-only host array."""
    on_dev = _host_or_cuda(x, what)
    if not _has_dtype(x, *dtypes) or tuple(x.shape) != tuple(shape) or not (x.is_contiguous() if on_dev else x.flags.c_contiguous) \
            or (on_device is not None and on_dev != on_device) or (writeable and not on_dev and not x.flags.writeable):
        side = {None: "", True: "CUDA ", False: "host "}[on_device]
        raise ValueError(f"{what} must be a {'writeable ' if writeable else ''}contiguous {side}{' / '.join(np.dtype(d).name for d in dtypes)} array of shape {tuple(shape)}")
    return _ptr(x), on_dev


def _dense_input(X):
    """``(pointer, on the device, keepalive, n_rows, n_cols, row pitch in elements, dtype code)`` of a dense matrix: a torch tensor as
    it is (a CPU tensor is host memory); anything else as a host array widened as ``normalize_values`` says.  A view of some columns
    of a wider matrix is passed as it is; a host array that ``_row_pitch`` cannot walk is copied, such a tensor is refused."""
    is_tensor = _is_torch_tensor(X)
    if not is_tensor:
        X = normalize_values(np.asarray(X))
    if len(X.shape) != 2:
        raise ValueError(f"X must be 2-D, got {len(X.shape)} dimensions")
    ld = _row_pitch(X)
    if ld is None:
        if is_tensor:
            raise ValueError("a tensor X must be row-major with rows that do not overlap: tensors are not copied")
        X = np.ascontiguousarray(X)
        ld = X.shape[1]
    return _ptr(X), is_tensor and X.is_cuda, X, int(X.shape[0]), int(X.shape[1]), ld, dtype_code(_dtype_name(X) if is_tensor else X.dtype)


def _sparse_input(data, indices, indptr, shape):
    """``(data, indices, indptr as _Buf, index dtype code, n_rows, n_cols)`` of a CSC / CSR matrix given as its three arrays: CUDA
    tensors as they are; host values widened as ``normalize_values`` says, host indices int32 if both arrays are, else int64."""
    n_rows, n_cols = int(shape[0]), int(shape[1])
    if _is_torch_tensor(data):
        d, i, p = _Buf(data), _Buf(indices), _Buf(indptr)
    else:
        d = _Buf(normalize_values(np.asarray(data)))
        idt = np.int32 if (np.asarray(indices).dtype == np.int32 and np.asarray(indptr).dtype == np.int32) else np.int64
        i, p = _Buf(indices, idt), _Buf(indptr, idt)
    if i.np_dtype != p.np_dtype or i.np_dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise KeyError(f"Support for index dtypes {i.np_dtype}/{p.np_dtype} is not implemented.")
    if not (d.on_device == i.on_device == p.on_device):
        raise ValueError("data, indices and indptr must live on the same side (host or device)")
    return d, i, p, IDX_I32 if i.np_dtype == np.int32 else IDX_I64, n_rows, n_cols


def _check_chunk_bounds(col_lb, col_ub, n_cols):
    if col_lb < 0 or col_ub > n_cols or col_lb > col_ub:
        raise ValueError(f"Invalid chunk bounds: {(col_lb, col_ub)} for data with {n_cols} columns.")


def _n_result_planes(scores) -> int:
    """3 result planes (p, U, fold change), or 4 with the z-score plane; ``ValueError`` unless ``scores`` is a bool."""
    if not isinstance(scores, (bool, np.bool_)):
        raise ValueError(f"scores must be a bool, got {scores!r}")
    return 4 if scores else 3


def _pair_selection(sel, G):
    """``(K, keepalive, pointer)`` of the group ids a pair call compares; None selects all ``G``, in order."""
    if sel is None:
        return G, None, None
    sel = np.ascontiguousarray(sel, dtype=np.int64).reshape(-1)
    return int(sel.size), sel, sel.ctypes.data


def _pair_planes(out, n, K, W, on_dev, device, with_left):
    """``(planes, left, plane pointers, left pointer, on the device)`` of the ``n`` float64 ``[K, K, W]`` result planes of a pair
    call, and with ``with_left`` of the ``[W]`` words behind them.  ``out`` None: allocated, on ``device`` if ``on_dev``.  Given
    planes must be on the side ``on_dev`` names -- with ``left`` on the side of ``left``, wherever the input is."""
    if out is None:
        dev = device if on_dev else None
        out = [_empty((K, K, W), np.float64, dev) for _ in range(n)] + ([_empty((W,), np.int32 if on_dev else np.uint32, dev)] if with_left else [])
    out = tuple(out)
    if len(out) != n + with_left:
        raise ValueError(f"out must hold {n} planes (p, U, fold change{', z' if n == 4 else ''}){' and left' if with_left else ''}")
    planes, left = out[:n], out[n] if with_left else None
    on_dev = _host_or_cuda(left, "left") if with_left else on_dev
    ptrs = [_block(q, "an output plane", (np.float64,), (K, K, W), on_device=on_dev, writeable=True)[0] for q in planes]
    left_ptr = _block(left, "left", (np.int32, np.uint32) if on_dev else (np.uint32,), (W,), on_device=on_dev, writeable=True)[0] if with_left else None
    return planes, left, ptrs, left_ptr, on_dev


def _stacked_rows(x, what, layout="[a, b] rows of an [A, B, W]"):
    """The ``[A * B, W]`` view (never a copy) of an ``[A, B, W]`` numpy array or tensor whose ``[a, b]`` rows lie one pitch apart (a
    contiguous block, or its first W columns): row ``a * B + b`` of the view is ``x[a, b]``, and ``_plane`` describes it.
    ``ValueError`` otherwise; ``layout``: what the message calls the rows."""
    if len(x.shape) != 3:
        raise ValueError(f"{what} must have three dimensions, got shape {tuple(x.shape)}")
    A, B, W = x.shape
    is_tensor = not isinstance(x, np.ndarray)
    s0, s1, s2 = x.stride() if is_tensor else x.strides
    if A > 1 and s0 != B * s1:
        raise ValueError(f"{what}: the {layout} plane must lie one row stride apart")
    if is_tensor:
        return x.as_strided((A * B, W), (s1, s2))
    return np.lib.stride_tricks.as_strided(x, (A * B, W), (s1, s2), writeable=False)


def _pairs_as_rows(x, what):
    """``(K, W, _stacked_rows(x))`` of a ``[K, K, W]`` numpy array or CUDA tensor: row ``r * K + g`` of the view is ``x[r, g]``."""
    _host_or_cuda(x, what)
    if len(x.shape) != 3 or x.shape[0] != x.shape[1]:
        raise ValueError(f"{what} must be a [K, K, W] plane, got shape {tuple(x.shape)}")
    return int(x.shape[0]), int(x.shape[2]), _stacked_rows(x, what, "[r, g] rows of a [K, K, W]")


def _io_flags(on_dev) -> int:
    """The flags of a call whose inputs and outputs live on one side."""
    return (FLAG_INPUT_DEVICE | FLAG_OUTPUT_DEVICE) if on_dev else 0


def _tt_variant(variant) -> int:
    try:
        return TT_VARIANTS[variant]
    except (KeyError, TypeError):
        raise ValueError(f"Unknown t-test variant {variant!r}: one of {sorted(TT_VARIANTS)}") from None


def _wanted(want, names):
    """``want`` as a tuple of distinct entries of ``names``, at least one."""
    want = tuple(want)
    if not want or any(w not in names for w in want) or len(set(want)) != len(want):
        raise ValueError(f"want must name distinct planes of {names}, got {want!r}")
    return want


def _moment_planes(named_planes, required, n_groups):
    """``(ins, G, W, on the device, pointers, row pitch)`` of the moment planes ``((name, plane or None), ...)`` of a t-test call:
    float64 ``[G, W]`` planes of one shape on one side, those named in ``required`` given, ``G`` the ``n_groups`` of the engine.
    ``ins``: their ``_Plane`` records (None where not given); host planes of several pitches are made contiguous."""
    ins = [None if x is None else _plane(x, name, copy_ok=True) for name, x in named_planes]
    if any(q is None for (name, _), q in zip(named_planes, ins) if name in required):
        raise ValueError(f"{' and '.join(required)} are required")
    given = [q for q in ins if q is not None]
    G, W, on_dev = given[0].rows, given[0].cols, given[0].on_device
    if any((q.rows, q.cols) != (G, W) for q in given):
        raise ValueError("the moment planes must share one shape")
    if not any(q.on_device for q in given) and len({q.pitch for q in given}) > 1:
        ins = [None if q is None else _plane(np.ascontiguousarray(q.array), "a moment plane") for q in ins]
    ptrs, _, ld = _plane_set(ins, "the moment planes")
    if G != n_groups:
        raise ValueError(f"the moment planes have {G} rows but the engine's groups number {n_groups}")
    return ins, G, W, on_dev, ptrs, ld


def _wanted_outputs(out, want, names, on_dev, alloc, describe):
    """``(planes, pointers in the order of names, row pitch)`` of the output planes of a t-test call: ``out`` None (one ``alloc()``
    per entry of ``want``) or as many planes, each described by ``describe(plane, what)`` and on the side ``on_dev`` of the moments."""
    if out is None:
        planes = tuple(alloc() for _ in want)
    else:
        planes = tuple(out)
        if len(planes) != len(want):
            raise ValueError(f"out must hold {len(want)} planes, one per entry of want")
    outs = dict.fromkeys(names)  # in the order of the library's output arguments
    for w, pl in zip(want, planes):
        outs[w] = describe(pl, f"out[{w}]")
    ptrs, oflag, ld = _plane_set(list(outs.values()), "the output planes")
    if bool(oflag) != on_dev:
        raise ValueError("the output planes must live on the same side as the moments")
    return planes, ptrs, ld


def _hists_input(H, flags, rows_name, sums=None, names="H and flags"):
    """``(H, flags, rows, W, on the device)`` of the histograms ``[rows, W, 256]`` and gene flags ``[W]`` of ``group_value_hists``:
    contiguous 32-bit integer CUDA tensors as they are, anything else as uint32 host arrays.  ``rows_name``: what the messages call
    the rows ("G"); ``sums``, ``names``: a further array that must live on their side, and what the message then calls the three."""
    on_dev = _is_torch_tensor(H)
    if on_dev != _is_torch_tensor(flags) or (sums is not None and on_dev != _is_torch_tensor(sums)):
        raise ValueError(f"{names} must live on the same side (host or device)")
    if on_dev:
        if not (H.is_cuda and flags.is_cuda and H.is_contiguous() and flags.is_contiguous()) or H.dim() != 3 or H.element_size() != 4 \
                or flags.element_size() != 4 or H.dtype.is_floating_point or flags.dtype.is_floating_point:
            raise ValueError(f"H and flags must be contiguous 32-bit integer CUDA tensors [{rows_name}, W, 256] and [W]")
    else:
        H, flags = np.ascontiguousarray(H, dtype=np.uint32), np.ascontiguousarray(flags, dtype=np.uint32)
        if H.ndim != 3:
            raise ValueError(f"H must be [{rows_name}, W, 256]")
    rows, W, R = (int(x) for x in H.shape)
    if R != Engine.HIST_VALUES or tuple(flags.shape) != (W,):
        raise ValueError(f"H must be [{rows_name}, W, {Engine.HIST_VALUES}] and flags [W], got {tuple(H.shape)} and {tuple(flags.shape)}")
    return H, flags, rows, W, on_dev


def _sums_arg(sums, shape, on_dev, what):
    """``(array, pointer, row pitch)`` of an optional float64 ``sums`` plane of ``shape`` that must live on the side ``on_dev`` of
    ``what``; ``(None, None, 0)`` without one."""
    if sums is None:
        return None, None, 0
    sums = _plane(sums, "sums", shape=shape, copy_ok=True)
    if sums.on_device != on_dev:
        raise ValueError(f"sums must live on the side of {what} (host or device)")
    return sums.array, sums.ptr, sums.pitch


#: a matrix as the entry points take it: the C arguments that name it, the arrays behind them, where they live, its columns and the
#: symbol suffix of its kind ("dense", "csc", "csr", "bound")
_Matrix = namedtuple("_Matrix", "args keep on_device n_cols suffix")


def _dense_matrix(X):
    ptr, on_dev, keep, n_rows, n_cols, ld, dt = _dense_input(X)
    return _Matrix((ptr, dt, n_rows, n_cols, ld), (keep,), on_dev, n_cols, "dense")


def _sparse_matrix(fmt, data, indices, indptr, shape, formats=("csc", "csr")):
    if fmt not in formats:
        raise ValueError(f"fmt must be {' or '.join(repr(f) for f in formats)}, got {fmt!r}")
    d, i, p, idx, n_rows, n_cols = _sparse_input(data, indices, indptr, shape)
    return _Matrix((d.ptr, dtype_code(d.np_dtype), i.ptr, p.ptr, idx, n_rows, n_cols), (d.keep, i.keep, p.keep), d.on_device, n_cols, fmt)


def combine_rank(n: int, method: str, rank, min_prop) -> int:
    """The rank j* handed to illico_combine_pairs: ``rank`` if given, else ``max(1, ceil(n * min_prop))`` with ``min_prop`` in (0, 1];
    1 for the methods that do not read it.  ``ValueError`` for an unknown method, a bad ``min_prop`` or a ``rank`` that is no integer."""
    import math
    if not isinstance(method, str) or method not in COMBINE_METHODS:
        raise ValueError(f"Unknown combination method {method!r}: one of {sorted(COMBINE_METHODS)}")
    if isinstance(min_prop, bool) or not isinstance(min_prop, (int, float, np.integer, np.floating)) or not 0 < min_prop <= 1:
        raise ValueError(f"min_prop must be a number in (0, 1], got {min_prop!r}")
    if rank is not None and (isinstance(rank, bool) or not isinstance(rank, (int, np.integer))):
        raise ValueError(f"rank must be an integer, got {rank!r}")
    if method != "some":
        return 1
    return int(rank) if rank is not None else max(1, math.ceil(n * float(min_prop)))


class Engine:
    """One illico_ctx: one device, one stream, device scratch, the current GroupContainer."""

    def __init__(self, device: int | None = None):
        self.lib = load()
        if device is None:
            device = _current_device()
        self.device = int(device)
        h = ctypes.c_void_p()
        rc = self.lib.illico_ctx_create(self.device, ctypes.byref(h))
        if rc != OK or not h.value:
            raise RuntimeError(
                f"illico_ctx_create(device={self.device}) failed with code {rc}: no usable MI355X/HIP device. "
                "The engine has no CPU fallback.")
        self.h = h
        self._groups_key = None
        self._groups_keep = None
        self._stream = None  # None = the context's own non-blocking stream; else the hipStream_t it was bound to

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.illico_ctx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != OK:
            _raise(rc, (self.lib.illico_last_error(self.h) or b"").decode())

    def set_option(self, key: str, value: int):
        self._check(self.lib.illico_ctx_set_option(self.h, key.encode(), int(value)))

    def set_stream(self, stream_ptr: int):
        self._check(self.lib.illico_ctx_set_stream(self.h, ctypes.c_void_p(stream_ptr)))
        self._stream = int(stream_ptr)

    def _bind_torch_stream(self, *tensors):
        """Device tensors as inputs or outputs: run this call on torch's CURRENT stream of the engine's device.

        The engine's kernels are then ordered after whatever produced the inputs on that stream (``X = torch.log1p(Y)``
        just before the call) and before whatever consumes device-resident output planes on it -- the same contract
        every torch op gives.  Host arrays need nothing: the C side synchronises before it returns them.
        """
        if not any(_is_torch_tensor(t) and t.is_cuda for t in tensors):
            return
        s = int(_torch().cuda.current_stream(self.device).cuda_stream)
        if s != self._stream:
            self.set_stream(s)

    def synchronize(self):
        self._check(self.lib.illico_ctx_synchronize(self.h))

    # ---- groups (GroupContainer of illico/utils/groups.py:6-15) ----
    def set_groups(self, grpc):
        key = id(grpc)
        if self._groups_key == key and self._groups_keep is grpc:
            return
        enc = np.ascontiguousarray(grpc.encoded_groups, dtype=np.int64)
        cnt = np.ascontiguousarray(grpc.counts, dtype=np.int64)
        idx = np.ascontiguousarray(grpc.indices, dtype=np.int64)
        ptr = np.ascontiguousarray(grpc.indptr, dtype=np.int64)
        self._check(self.lib.illico_set_groups(self.h, enc.ctypes.data, cnt.ctypes.data, idx.ctypes.data,
                                               ptr.ctypes.data, enc.size, cnt.size, int(grpc.encoded_ref_group)))
        self._groups_key, self._groups_keep = key, grpc
        self.n_groups = int(cnt.size)

    @staticmethod
    def _flags(is_log1p, use_continuity, tie_correct):
        return (FLAG_LOG1P if is_log1p else 0) | (FLAG_CONTINUITY if use_continuity else 0) | \
               (FLAG_TIE_CORRECT if tie_correct else 0)

    @staticmethod
    def _alt(alternative):
        try:
            return ALTERNATIVES[alternative]
        except KeyError:
            raise ValueError(f"Unsupported alternative hypothesis: {alternative}") from None

    def _outputs(self, out, G, W, want_device, scores=False):
        """out: None (allocate host planes; four with ``scores``), a tuple of three host ndarrays (views with a common row stride
        are fine) or three device tensors -- or four: the fourth receives the z-score plane."""
        n = _n_result_planes(scores)
        if out is None:
            planes = tuple(_empty((G, W), np.float64, f"cuda:{self.device}" if want_device else None) for _ in range(n))
        else:
            planes = tuple(out)
            if len(planes) not in (3, 4) or (scores and len(planes) != 4):
                raise ValueError("out must hold 3 planes (p, U, fold change), or 4 with the z-score plane last (4 with scores=True)")
        if W == 0:  # empty chunk (lb == ub is legal, asymptotic_wilcoxon.py:49): nothing to compute
            return planes, None, 0, 1
        ptrs, flag, ld = _plane_set([_plane(p, f"output plane {k}", shape=(G, W), writeable=True) for k, p in enumerate(planes)], "output planes")
        return planes, ptrs, flag, ld

    def _rank_tests(self, m, col_lb, col_ub, is_log1p, use_continuity, tie_correct, alternative, out, device_out, defer, scores):
        """What ``run_dense``, ``run_sparse`` and ``BoundMatrix.run`` share: illico_run_<kind>_ex on the columns [col_lb, col_ub) of the
        ``_Matrix`` ``m``, with the keywords of those three.  Returns the planes of ``_outputs``; without a fourth one the library
        gets a null ``out_z``."""
        alt = self._alt(alternative)
        _check_chunk_bounds(col_lb, col_ub, m.n_cols)
        planes, ptrs, oflag, out_ld = self._outputs(out, self.n_groups, col_ub - col_lb, device_out, scores)
        if ptrs is None:
            return planes
        flags = self._flags(is_log1p, use_continuity, tie_correct) | (FLAG_INPUT_DEVICE if m.on_device else 0) | oflag | (FLAG_DEFER if defer else 0)
        self._bind_torch_stream(*m.keep, *planes)
        self._check(getattr(self.lib, f"illico_run_{m.suffix}_ex")(self.h, *m.args, col_lb, col_ub, flags, alt, *ptrs, *[None] * (4 - len(ptrs)), out_ld))
        return planes

    def run_dense(self, X, col_lb, col_ub, *, is_log1p=False, use_continuity=True, tie_correct=True, alternative="two-sided",
                  out=None, device_out=False, defer=False, scores=False):
        """The rank-sum tests of the dense columns [col_lb, col_ub) of ``X``.
        ``defer=True`` (device input and device planes only): return once the pass is enqueued; the planes are complete
        after ``synchronize()`` or the next call on this engine (ILLICO_FLAG_DEFER, include/illico_hip.h).  ``scores=True``
        (or a 4-tuple ``out``): a fourth plane, the z-score of every test (include/illico_hip.h: illico_run_dense_ex)."""
        return self._rank_tests(_dense_matrix(X), col_lb, col_ub, is_log1p, use_continuity, tie_correct, alternative, out, device_out, defer, scores)

    def run_sparse(self, fmt, data, indices, indptr, shape, col_lb, col_ub, *, is_log1p=False, use_continuity=True, tie_correct=True,
                   alternative="two-sided", out=None, device_out=False, defer=False, scores=False):
        """``run_dense`` of a CSC (``fmt="csc"``) or CSR matrix given as its three arrays.  ``defer=True`` (device-resident CSC arrays
        and device planes only; ignored elsewhere): return once the count-valued pass is enqueued; the planes are complete after
        ``synchronize()`` or the next call on this engine."""
        return self._rank_tests(_sparse_matrix("csc" if fmt == "csc" else "csr", data, indices, indptr, shape), col_lb, col_ub,
                                is_log1p, use_continuity, tie_correct, alternative, out, device_out, defer, scores)

    def bind_sparse(self, fmt, data, indices, indptr, shape):
        """Upload a host CSR / CSC matrix once (or adopt device tensors) -- illico_csr_bind / illico_csc_bind; returns a
        ``BoundMatrix`` whose ``run(col_lb, col_ub, ...)`` computes chunks without moving the matrix again."""
        d, i, p, idx, n_rows, n_cols = _sparse_input(data, indices, indptr, shape)
        h = ctypes.c_void_p()
        fn = self.lib.illico_csc_bind if fmt == "csc" else self.lib.illico_csr_bind
        self._bind_torch_stream(d.keep, i.keep, p.keep)
        self._check(fn(self.h, d.ptr, dtype_code(d.np_dtype), i.ptr, p.ptr, idx, n_rows, n_cols,
                       FLAG_INPUT_DEVICE if d.on_device else 0, ctypes.byref(h)))
        return BoundMatrix(self, h, (n_rows, n_cols), (d.keep, i.keep, p.keep) if d.on_device else None)

    def input_bytes(self) -> int:
        """Matrix bytes copied host -> device by this context so far (illico_profile_input_bytes)."""
        n = ctypes.c_int64(0)
        self._check(self.lib.illico_profile_input_bytes(self.h, ctypes.byref(n)))
        return int(n.value)

    def planes_to_host(self, planes, out=None):
        """A contiguous device tensor ``[3, n_groups, n_cols]`` of float64 planes -> a host ndarray of the same shape, through the
        context's pinned double buffer (include/illico_hip.h: illico_planes_to_host): what the gathering rank of a multi-GPU call does
        ONCE with everything it has received."""
        if not _is_torch_tensor(planes) or planes.dim() != 3 or planes.shape[0] != 3:
            raise ValueError("planes_to_host wants a contiguous CUDA tensor of shape [3, n_groups, n_cols]")
        _, G, W = (int(x) for x in planes.shape)
        base, _ = _block(planes, "planes", (np.float64,), (3, G, W), on_device=True)
        if G != getattr(self, "n_groups", -1):  # the library copies n_groups rows per plane: the groups last set on this engine
            raise ValueError(f"planes hold {G} groups, the engine's groups are {getattr(self, 'n_groups', None)} (set_groups first)")
        if out is None:
            out = np.empty((3, G, W), dtype=np.float64)
        elif not isinstance(out, np.ndarray) or out.shape != (3, G, W):
            raise ValueError("out must be a writeable float64 ndarray [3, n_groups, n_cols] whose rows are contiguous")
        ptrs, _, out_ld = _plane_set([_plane(out[k], "a plane of out", shape=(G, W), writeable=True) for k in range(3)], "the planes of out")
        self._bind_torch_stream(planes)
        self._check(self.lib.illico_planes_to_host(self.h, base, base + G * W * 8, base + 2 * G * W * 8, W, *ptrs, out_ld))
        return out

    def rank_statistics(self, X, col_lb, col_ub, *, is_log1p=False):
        """The ranking primitives before finalisation (include/illico_hip.h: illico_rank_statistics):
        ``(two_u int64 [W, G], tie_sum uint64 [W, G], value_sum float64 [W, G])`` for the dense columns [col_lb, col_ub)."""
        ptr, on_dev, keep, n_rows, n_cols, ld, dt = _dense_input(X)
        _check_chunk_bounds(col_lb, col_ub, n_cols)
        W, G = col_ub - col_lb, self.n_groups
        two_u, tie, vsum = np.zeros((W, G), np.int64), np.zeros((W, G), np.uint64), np.zeros((W, G), np.float64)
        self._bind_torch_stream(keep)
        flags = (FLAG_LOG1P if is_log1p else 0) | (FLAG_INPUT_DEVICE if on_dev else 0)
        self._check(self.lib.illico_rank_statistics(self.h, ptr, dt, n_rows, n_cols, ld, col_lb, col_ub, flags,
                                                    two_u.ctypes.data, tie.ctypes.data, vsum.ctypes.data))
        return two_u, tie, vsum

    def adjust_pvalues(self, p, method="bh", *, n_top=0, out=None):
        """Per-row multiple-testing correction of a p-value plane (include/illico_hip.h: illico_adjust_pvalues).

        ``p``: float64 ``[G, M]``, a numpy array or a CUDA tensor with unit column stride (a view of a wider plane is fine).
        ``method``: ``"bh"``, ``"by"`` or ``"bonferroni"``.  Outputs live where ``p`` lives; ``out`` (same side, float64 ``[G, M]``,
        unit column stride; ``p`` itself adjusts in place) receives the adjusted values.  Returns ``adj``, or ``(adj, top)`` with
        ``top`` int64 ``[G, n_top]`` -- each row's first ``n_top`` columns by ascending p, ties by column -- when ``n_top > 0``."""
        code = _adjust_method(method)
        p = _plane(p, "p", copy_ok=True)
        G, M, device = p.rows, p.cols, p.array.device if p.on_device else None
        n_top = _adjust_n_top(n_top, M)
        adj = _plane(_empty((G, M), np.float64, device) if out is None else out, "out", shape=(G, M), writeable=True)
        if adj.on_device != p.on_device:
            raise ValueError(f"out must be a float64 [{G}, {M}] plane on the same side as p")
        top = _empty((G, n_top), np.int64, device) if n_top else None
        if G and M:
            self._bind_torch_stream(p.array, adj.array, top)
            self._check(self.lib.illico_adjust_pvalues(self.h, p.ptr, G, M, p.pitch, code, _io_flags(p.on_device),
                                                       adj.ptr, adj.pitch, n_top, _ptr(top), max(n_top, 1)))
        return (adj.array, top) if n_top else adj.array

    def top_by_score(self, x, n_top, *, out=None):
        """Each row's first ``n_top`` columns by DESCENDING score, ties by column (include/illico_hip.h: illico_top_by_score) --
        ``np.argsort(-(x + 0.0), axis=1, kind="stable")[:, :n_top]``.  ``x``: float64 ``[G, M]``, numpy or CUDA tensor with unit
        column stride (a z-score plane); the int64 ``[G, n_top]`` result lives where ``x`` lives.  ``ValueError`` for a NaN."""
        x = _plane(x, "x", copy_ok=True)
        G, M = x.rows, x.cols
        n_top = _adjust_n_top(n_top, M)
        top = _empty((G, n_top), np.int64, x.array.device if x.on_device else None) if out is None else out
        if G and M and n_top:
            self._bind_torch_stream(x.array, top)
            self._check(self.lib.illico_top_by_score(self.h, x.ptr, G, M, x.pitch, _io_flags(x.on_device),
                                                     n_top, _ptr(top), n_top))
        return top

    # ---- per-group expression statistics (include/illico_hip.h: illico_group_stats_*) ----
    def _gs_outputs(self, out, G, W, rest, want_device, kinds=(np.int64, np.float64, np.int64, np.float64),
                    names="(nnz, sum) or 4 (nnz, sum, nnz_rest, sum_rest)"):
        """(planes, pointers, output flag, row pitch) of the statistics planes: ``out`` None (allocate nnz int64 / sum float64 [G, W],
        plus their rest planes with ``rest``) or a tuple of 2 or 4 planes in that order (nnz, sum[, nnz_rest, sum_rest]), each a
        host ndarray or a CUDA tensor of the right dtype with unit column stride, or None (not computed).  ``kinds`` / ``names``: the
        four planes' dtypes and what the error message calls them (the moment planes are four float64 ones)."""
        if out is None:
            planes = tuple(_empty((G, W), kinds[k], f"cuda:{self.device}" if want_device else None) for k in range(4 if rest else 2))
        else:
            planes = tuple(out)
            if len(planes) not in (2, 4):
                raise ValueError(f"out must hold 2 planes {names}")
        if all(p is None for p in planes):
            raise ValueError("at least one output plane is needed")
        ptrs, flag, ld = _plane_set([None if p is None else _plane(p, f"output plane {k}", dtype=kinds[k], shape=(G, W), writeable=True)
                                     for k, p in enumerate(planes)], "output planes")
        return planes, ptrs + [None] * (4 - len(ptrs)), flag, max(ld, 1)

    def _group_planes(self, family, m, col_lb, col_ub, flags, rest, out, want_device, *planes_spec):
        """illico_<family>_<kind> on the ``_Matrix`` ``m``; planes allocated here live on the device with ``want_device``;
        ``planes_spec``: the ``kinds`` and ``names`` of ``_gs_outputs`` where they are not its defaults."""
        _check_chunk_bounds(col_lb, col_ub, m.n_cols)
        G, W = self.n_groups, col_ub - col_lb
        planes, ptrs, oflag, out_ld = self._gs_outputs(out, G, W, rest, want_device, *planes_spec)
        if W == 0:
            return planes
        self._bind_torch_stream(*m.keep, *[p for p in planes if p is not None])
        self._check(getattr(self.lib, f"illico_{family}_{m.suffix}")(self.h, *m.args, col_lb, col_ub,
                                                                      flags | (FLAG_INPUT_DEVICE if m.on_device else 0) | oflag, *ptrs, out_ld))
        return planes

    def group_stats(self, X, col_lb, col_ub, *, is_log1p=False, rest=False, out=None):
        """Per-group non-zero counts and value sums of the dense columns [col_lb, col_ub) (illico_group_stats_dense).

        ``X``: a row-major numpy array or a CUDA tensor.  Returns ``(nnz, sum)`` -- int64 / float64 ``[G, W]`` -- or, with
        ``rest=True``, ``(nnz, sum, nnz_rest, sum_rest)``, living where ``X`` lives unless ``out`` (see ``_gs_outputs``) says otherwise."""
        m = _dense_matrix(X)
        return self._group_planes("group_stats", m, col_lb, col_ub, FLAG_LOG1P if is_log1p else 0, rest, out, m.on_device)

    def group_stats_sparse(self, fmt, data, indices, indptr, shape, col_lb, col_ub, *, is_log1p=False, rest=False, out=None):
        """``group_stats`` of a CSC (``fmt="csc"``) or CSR (``"csr"``) matrix given as its three arrays (numpy or CUDA tensors);
        CSR rows need not be sorted.  Duplicate entries count once per stored entry."""
        m = _sparse_matrix(fmt, data, indices, indptr, shape)
        return self._group_planes("group_stats", m, col_lb, col_ub, FLAG_LOG1P if is_log1p else 0, rest, out, m.on_device)

    # ---- per-group moments and Welch's t-test (include/illico_hip.h: illico_group_moments_*, illico_ttest_from_moments) ----
    _GM_KINDS = (np.float64, np.float64, np.float64, np.float64)
    _GM_NAMES = "(sum, sumsq) or 4 (sum, sumsq, sum_rest, sumsq_rest)"

    def group_moments(self, X, col_lb, col_ub, *, rest=False, out=None):
        """Per-group exact sums of the values and of their squares over the dense columns [col_lb, col_ub) (illico_group_moments_dense).

        ``X``: a row-major numpy array or a CUDA tensor.  Returns ``(sum, sumsq)`` -- float64 ``[G, W]`` -- or, with ``rest=True``,
        ``(sum, sumsq, sum_rest, sumsq_rest)``, living where ``X`` lives unless ``out`` (2 or 4 planes in that order, each a host
        ndarray, a CUDA tensor or None) says otherwise.  The values are taken as given: there is no ``is_log1p``."""
        m = _dense_matrix(X)
        return self._group_planes("group_moments", m, col_lb, col_ub, 0, rest, out, m.on_device, self._GM_KINDS, self._GM_NAMES)

    def group_moments_sparse(self, fmt, data, indices, indptr, shape, col_lb, col_ub, *, rest=False, out=None):
        """``group_moments`` of a CSC (``fmt="csc"``) or CSR (``"csr"``) matrix given as its three arrays (numpy or CUDA tensors);
        CSR rows need not be sorted.  Duplicate entries count as separate values."""
        m = _sparse_matrix(fmt, data, indices, indptr, shape)
        return self._group_planes("group_moments", m, col_lb, col_ub, 0, rest, out, m.on_device, self._GM_KINDS, self._GM_NAMES)

    def ttest_from_moments(self, sum, sumsq, sum_rest=None, sumsq_rest=None, *, variant="welch", alternative="two-sided",
                           want=("p", "t"), out=None):
        """Welch's t-test of every (group, gene) from moment planes (illico_ttest_from_moments), for the engine's current groups.

        ``sum`` / ``sumsq`` (and, one-versus-rest, ``sum_rest`` / ``sumsq_rest``): float64 ``[G, M]`` numpy arrays or CUDA tensors with
        unit column stride and one row stride, all on one side.  ``variant``: ``"welch"`` or ``"overestim_var"``.  ``want``: which of
        ``TT_OUTPUTS`` (``"p"``, ``"t"``, ``"df"``, ``"mean"``, ``"var"``, ``"mean_ref"``, ``"var_ref"``) to compute.  Returns a tuple of
        float64 ``[G, M]`` planes in the order of ``want``, living where the inputs live; ``out``: a tuple of as many planes to write."""
        var, alt, want = _tt_variant(variant), self._alt(alternative), _wanted(want, TT_OUTPUTS)
        ins, G, M, on_dev, in_ptrs, ld = _moment_planes((("sum", sum), ("sumsq", sumsq), ("sum_rest", sum_rest), ("sumsq_rest", sumsq_rest)),
                                                        ("sum", "sumsq"), getattr(self, "n_groups", None))
        planes, out_ptrs, out_ld = _wanted_outputs(out, want, TT_OUTPUTS, on_dev, lambda: _empty((G, M), np.float64, ins[0].array.device if on_dev else None),
                                                   lambda pl, what: _plane(pl, what, shape=(G, M), writeable=True))
        if G and M:
            self._bind_torch_stream(*[q.array for q in ins if q is not None], *planes)
            self._check(self.lib.illico_ttest_from_moments(self.h, *in_ptrs, M, max(ld, 1), var, alt, _io_flags(on_dev), *out_ptrs, out_ld))
        return planes

    def pair_ttest_from_moments(self, sum, sumsq, *, sel=None, fsum=None, variant="welch", alternative="two-sided", want=("p", "t"), out=None):
        """Welch's t-test of every ordered pair of groups from moment planes (include/illico_hip_pair_ttest.h:
        illico_pair_ttest_from_moments), for the sizes of the engine's current groups (their reference / one-versus-rest mode plays no part).

        ``sum`` / ``sumsq``: float64 ``[G, W]`` numpy arrays or CUDA tensors as ``group_moments`` returns them; ``fsum``: the sums the
        fold change is formed from (under log1p the ``expm1`` sums of ``group_stats(..., is_log1p=True)``; default ``sum``); all on one
        side, unit column stride, one row stride.  ``sel``: the K >= 2 group ids to compare, strictly ascending (default: all G).
        ``variant``: ``"welch"`` or ``"overestim_var"``.  ``want``: which of ``PAIR_TT_OUTPUTS`` (``"p"``, ``"t"``, ``"df"``,
        ``"fold_change"``, ``"cohen_d"``) to compute.  Returns a tuple of float64 ``[K, K, W]`` planes in the order of ``want``, indexed
        ``[r, g, j]`` -- group ``sel[g]`` against reference ``sel[r]``, the layout ``combine_pairs`` reads -- living where the moments
        live; ``out``: a tuple of as many planes to write (contiguous, or the first W columns of contiguous blocks of one width).
        ``plane[r]`` of ``p``, ``t``, ``df`` is, bit for bit, ``ttest_from_moments`` under the reference ``sel[r]``, rows ``sel``;
        diagonal: (t, p) = (0, 1), ``cohen_d`` 0."""
        var, alt, want = _tt_variant(variant), self._alt(alternative), _wanted(want, PAIR_TT_OUTPUTS)
        ins, G, W, on_dev, in_ptrs, ld = _moment_planes((("sum", sum), ("sumsq", sumsq), ("fsum", fsum)), ("sum", "sumsq"), getattr(self, "n_groups", None))
        sel = np.arange(G, dtype=np.int32) if sel is None else np.ascontiguousarray(sel).reshape(-1)
        if sel.dtype.kind not in "iu":
            raise ValueError(f"sel must hold integer group ids, got {sel.dtype}")
        K = int(sel.size)
        if K < 2:
            raise ValueError(f"{K} groups selected: a pair needs two")
        if sel.min() < 0 or sel.max() >= G or np.any(np.diff(sel.astype(np.int64)) <= 0):
            raise ValueError(f"sel must name group ids 0 .. {G - 1} in strictly ascending order, got {sel.tolist()}")
        if K > PAIR_TT_MAX_GROUPS:
            raise NotImplementedError(f"{K} groups selected: pair_ttest_from_moments takes up to {PAIR_TT_MAX_GROUPS}")
        sel = np.ascontiguousarray(sel, dtype=np.int32)

        def describe(pl, what):
            Ko, Wo, rows = _pairs_as_rows(pl, what)
            if (Ko, Wo) != (K, W):
                raise ValueError(f"{what} must be a [K, K, W] = {(K, K, W)} plane, got shape {tuple(pl.shape)}")
            if not on_dev and not pl.flags.writeable:
                raise ValueError(f"{what} must be writeable")
            return _plane(rows, what, shape=(K * K, W))

        planes, out_ptrs, out_ld = _wanted_outputs(out, want, PAIR_TT_OUTPUTS, on_dev,
                                                   lambda: _empty((K, K, W), np.float64, ins[0].array.device if on_dev else None), describe)
        if W:
            self._bind_torch_stream(*[q.array for q in ins if q is not None], *planes)
            self._check(self.lib.illico_pair_ttest_from_moments(self.h, *in_ptrs, W, max(ld, 1), sel.ctypes.data, K, var, alt, _io_flags(on_dev),
                                                                *out_ptrs, max(out_ld, W, 1)))
        return planes

    def student_t_pvalues(self, t, df, alternative="two-sided"):
        """Student's t tail of every (t, df) pair, elementwise (illico_student_t_pvalues): two-sided ``2 sf(|t|, df)``, ``"greater"``
        ``sf(t, df)``, ``"less"`` ``sf(-t, df)``.  ``t`` / ``df``: float64 numpy arrays or contiguous CUDA tensors of one shape; the
        result lives where they live.  NaN where the evaluation did not converge (or ``t`` is NaN)."""
        alt = self._alt(alternative)
        if _is_torch_tensor(t) != _is_torch_tensor(df):
            raise ValueError("t and df must both be numpy arrays or both CUDA tensors")
        if _is_torch_tensor(t):
            if not (t.is_cuda and df.is_cuda) or _dtype_name(t) != "float64" or _dtype_name(df) != "float64" or t.shape != df.shape:
                raise ValueError("t and df must be float64 CUDA tensors of one shape")
            t, df = t.contiguous(), df.contiguous()
            p, n, flags = _empty(t.shape, np.float64, t.device), t.numel(), _io_flags(True)
        else:
            t, df = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(df, dtype=np.float64)
            if t.shape != df.shape:
                raise ValueError(f"t and df must have one shape, got {t.shape} and {df.shape}")
            p, n, flags = np.empty_like(t), t.size, 0
        if n:
            self._bind_torch_stream(t, df, p)
            self._check(self.lib.illico_student_t_pvalues(self.h, _ptr(t), _ptr(df), n, alt, flags, _ptr(p)))
        return p

    # ---- all-pairs Wilcoxon tests from value histograms (include/illico_hip.h: illico_group_value_hists_*, illico_pairwise_from_hists) ----
    #: values a histogram holds (0 .. HIST_VALUES - 1)
    HIST_VALUES = 256

    def _hist_outputs(self, out, G, W, want_device):
        """(H, flags, pointers, output flag): ``out`` None (allocate uint32 ``[G, W, 256]`` and ``[W]`` where the input lives) or a pair
        of contiguous uint32 arrays of those shapes, both numpy or both CUDA tensors (torch has no uint32 kernels: int32 tensors)."""
        if out is None:
            dtype, dev = (np.int32, f"cuda:{self.device}") if want_device else (np.uint32, None)
            H, fl = _empty((G, W, self.HIST_VALUES), dtype, dev), _empty((W,), dtype, dev)
        else:
            H, fl = out
        (hp, h_dev), (fp, f_dev) = (_block(a, name, (np.int32, np.uint32) if _is_torch_tensor(a) else (np.uint32,), shape, writeable=True)
                                    for name, a, shape in (("H", H, (G, W, self.HIST_VALUES)), ("flags", fl, (W,))))
        if h_dev != f_dev:
            raise ValueError("H and flags must live on the same side (host or device)")
        return H, fl, [hp, fp], FLAG_OUTPUT_DEVICE if h_dev else 0

    def group_value_hists(self, X, col_lb, col_ub, out=None):
        """Per-(group, gene) histograms of the values 0 .. 255 over the dense columns [col_lb, col_ub) (illico_group_value_hists_dense),
        for the engine's current groups (their reference / one-versus-rest mode plays no part).

        ``X``: a row-major numpy array or a CUDA tensor.  Returns ``(H, flags)``: ``H[g, j, c]`` the cells of group g whose value in
        column ``col_lb + j`` is c, ``flags[j]`` non-zero when the column holds a value that is no integer in [0, 255] (``H`` of such a
        column is unspecified).  uint32 numpy arrays for host input, int32 CUDA tensors for device input, unless ``out`` (a pair of
        either) says otherwise."""
        return self._value_hists(_dense_matrix(X), col_lb, col_ub, out)

    def group_value_hists_sparse(self, fmt, data, indices, indptr, shape, col_lb, col_ub, out=None):
        """``group_value_hists`` of a CSC (``fmt="csc"``) or CSR (``"csr"``) matrix given as its three arrays (numpy or CUDA tensors):
        the dense answer -- a stored zero counts in bin 0, and so do the cells that are not stored.  CSR rows need not be sorted."""
        return self._value_hists(_sparse_matrix(fmt, data, indices, indptr, shape), col_lb, col_ub, out)

    def _value_hists(self, m, col_lb, col_ub, out):
        """illico_group_value_hists_<kind> on the ``_Matrix`` ``m``."""
        _check_chunk_bounds(col_lb, col_ub, m.n_cols)
        G, W = self.n_groups, col_ub - col_lb
        H, fl, ptrs, oflag = self._hist_outputs(out, G, W, m.on_device)
        if W == 0:
            return H, fl
        self._bind_torch_stream(*m.keep, H, fl)
        self._check(getattr(self.lib, f"illico_group_value_hists_{m.suffix}")(self.h, *m.args, col_lb, col_ub,
                                                                               (FLAG_INPUT_DEVICE if m.on_device else 0) | oflag, *ptrs))
        return H, fl

    def pairwise_from_hists(self, H, flags, *, counts=None, sel=None, sums=None, is_log1p=False, use_continuity=True, tie_correct=True,
                            alternative="two-sided", scores=False, out=None):
        """The Wilcoxon rank-sum test of every ordered pair of groups from the histograms of ``group_value_hists``
        (illico_pairwise_from_hists).

        ``H`` ``[G, W, 256]`` and ``flags`` ``[W]``: as ``group_value_hists`` returns them (numpy, or CUDA tensors).  ``sel``: the K group
        ids to compare (default: all G, in order).  ``counts``: the G group sizes (default: those of the engine's current groups).
        ``sums``: an optional float64 ``[G, W]`` plane of per-group value sums for the fold change, on the side of ``H`` (under
        ``is_log1p`` pass the ``expm1`` sums of ``group_stats(..., is_log1p=True)``: ``is_log1p`` itself changes nothing here); without
        it the sums are those of the histograms.  Returns float64 planes ``(p, U, fold_change)`` -- and ``z`` with ``scores=True`` --
        of shape ``[K, K, W]`` indexed ``[r, g, j]``: group ``sel[g]`` against reference ``sel[r]``, so that ``plane[r]`` is the
        ``[K, W]`` plane of a one-versus-reference call with that reference.  Diagonal: p = 1, U = n^2 / 2, z = 0.  The columns of
        flagged genes are left as they are in ``out`` (a tuple of 3 or 4 contiguous planes on the side of ``H``; uninitialised when
        the planes are allocated here)."""
        alt, n = self._alt(alternative), _n_result_planes(scores)
        H, flags, G, W, on_dev = _hists_input(H, flags, "G", sums, "H, flags and sums")
        if counts is None:
            if self._groups_keep is None:
                raise ValueError("counts is needed: no groups have been set on this engine")
            counts = self._groups_keep.counts
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        if counts.shape != (G,):
            raise ValueError(f"H holds {G} groups but counts has shape {counts.shape}")
        K, sel_arr, sel_ptr = _pair_selection(sel, G)
        sums_array, sums_ptr, sums_ld = _sums_arg(sums, (G, W), on_dev, "H")
        planes, _, ptrs, _, _ = _pair_planes(out, n, K, W, on_dev, H.device if on_dev else None, False)
        fl = self._flags(is_log1p, use_continuity, tie_correct) | _io_flags(on_dev)
        self._bind_torch_stream(H, flags, sums_array, *planes)
        self._check(self.lib.illico_pairwise_from_hists(self.h, _ptr(H), _ptr(flags), counts.ctypes.data, G, W, sel_ptr, K, sums_ptr, sums_ld, fl, alt,
                                                        *ptrs, *[None] * (4 - n), max(W, 1)))
        return planes

    # ---- all-pairs Wilcoxon tests for any float32 / int32 values (include/illico_hip_ranked.h: illico_pairwise_ranked_*) ----
    #: selected groups the ranked pair route takes at most
    RANKED_MAX_GROUPS = 64

    def _ranked_args(self, W, on_dev, sums, sel, is_log1p, use_continuity, tie_correct, alternative, scores, out):
        """What the two ranked entry points share: (planes, left, the C arguments after col_ub, keepalives)."""
        alt, n = self._alt(alternative), _n_result_planes(scores)
        if sums is None:
            raise ValueError("sums is required: the per-group value sums of group_stats (under is_log1p its expm1 sums)")
        sums_array, sums_ptr, sums_ld = _sums_arg(sums, (self.n_groups, W), on_dev, "the matrix")
        K, sel_arr, sel_ptr = _pair_selection(sel, self.n_groups)
        planes, left, ptrs, left_ptr, out_dev = _pair_planes(out, n, K, W, on_dev, f"cuda:{self.device}", True)
        fl = self._flags(is_log1p, use_continuity, tie_correct) | (FLAG_INPUT_DEVICE if on_dev else 0) | (FLAG_OUTPUT_DEVICE if out_dev else 0)
        args = [sel_ptr, K, sums_ptr, sums_ld, fl, alt, *ptrs, *[None] * (4 - n), max(W, 1), left_ptr]
        return planes, left, args, (sel_arr, sums_array)

    def pairwise_ranked(self, X, col_lb, col_ub, *, sums, sel=None, is_log1p=False, use_continuity=True, tie_correct=True,
                        alternative="two-sided", scores=False, out=None):
        """The Wilcoxon rank-sum test of every ordered pair of groups over the dense columns [col_lb, col_ub), whatever their values
        (illico_pairwise_ranked_dense), for the engine's current groups (their reference / one-versus-rest mode plays no part).

        ``X``: a row-major float32 / int32 numpy array or CUDA tensor.  ``sums``: the float64 ``[G, W]`` plane of per-group value sums
        for the fold change, on the side of ``X`` (``group_stats(...)[1]``; under ``is_log1p`` that of ``group_stats(..., is_log1p=True)``:
        ``is_log1p`` itself changes nothing here).  ``sel``: the K <= 64 group ids to compare (default: all G, in order).  Returns
        ``(p, U, fold_change[, z], left)``: float64 planes ``[K, K, W]`` indexed ``[r, g, j]`` as ``pairwise_from_hists`` gives them,
        and ``left`` ``[W]`` (uint32 numpy / int32 CUDA tensor): non-zero for a column the route could not take -- a NaN, more
        different values than fit crowded into one sliver of the value range -- whose entries are left as they are in ``out`` (a
        tuple of the 3 or 4 planes and ``left``, all on one side; uninitialised when allocated here).  ``NotImplementedError``: other
        value types, more than 64 selected groups, two selected groups of 2097152 cells or more together."""
        return self._ranked(_dense_matrix(X), col_lb, col_ub, sums, sel, is_log1p, use_continuity, tie_correct, alternative, scores, out)

    def pairwise_ranked_sparse(self, fmt, data, indices, indptr, shape, col_lb, col_ub, *, sums, sel=None, is_log1p=False, use_continuity=True,
                               tie_correct=True, alternative="two-sided", scores=False, out=None):
        """``pairwise_ranked`` of a CSC matrix (``fmt="csc"``) given as its three arrays (numpy or CUDA tensors): the dense answer --
        a stored zero is a zero.  The row indices of a column must ascend (scipy: ``sort_indices()``)."""
        return self._ranked(_sparse_matrix(fmt, data, indices, indptr, shape, ("csc",)), col_lb, col_ub, sums, sel, is_log1p, use_continuity,
                            tie_correct, alternative, scores, out)

    def _ranked(self, m, col_lb, col_ub, *ranked_args):
        """illico_pairwise_ranked_<kind> on the ``_Matrix`` ``m``; ``ranked_args``: what ``_ranked_args`` takes after the side."""
        _check_chunk_bounds(col_lb, col_ub, m.n_cols)
        planes, left, args, keepalive = self._ranked_args(col_ub - col_lb, m.on_device, *ranked_args)
        self._bind_torch_stream(*m.keep, keepalive[1], left, *planes)
        self._check(getattr(self.lib, f"illico_pairwise_ranked_{m.suffix}")(self.h, *m.args, col_lb, col_ub, *args))
        return (*planes, left)

    # ---- per-group marker statistics (include/illico_hip_markers.h: illico_combine_pairs) ----
    def combine_pairs(self, p, effects=(), *, method, rank=None, min_prop=0.5, skip=None, out=None):
        """The K - 1 tests of each group against every other group combined into one p-value per (group, column)
        (illico_combine_pairs; include/illico_hip_markers.h states the formulas).

        ``p``: the float64 ``[K, K, W]`` p-value plane of a pair call, indexed ``[r, g, j]`` (numpy, or a CUDA tensor; a view of the
        first W columns of a wider block is fine); its diagonal is never read.  ``effects``: up to four planes of the same layout
        (U, fold change, z ...).  ``method``: ``"all"`` (the largest p), ``"any"`` (Simes) or ``"some"`` (Holm's adjusted p of rank
        ``rank``; default ``max(1, ceil((K - 1) * min_prop))``).  ``skip``: ``[W]`` words (uint32 numpy / 32-bit integer CUDA tensor),
        non-zero for a column that is neither validated nor written.  Everything lives on one side.  Returns
        ``(p_comb float64 [K, W], rep int32 [K, W], *selected effects)``: ``rep[g, j]`` the representative reference, an index into
        the K groups, and for each effect plane its value against it; allocated on the side of ``p`` unless ``out`` (a tuple of as
        many ``[K, W]`` planes sharing one row stride) receives them.  ``ValueError``: an off-diagonal p of a live column that is NaN
        or outside [0, 1] (device input: nothing is written), K < 2, a ``rank`` outside [1, K - 1]; ``NotImplementedError``: K > 256."""
        effects = tuple(effects)
        if len(effects) > COMBINE_MAX_EFFECTS:
            raise ValueError(f"at most {COMBINE_MAX_EFFECTS} effect planes, got {len(effects)}")
        K, W, p2 = _pairs_as_rows(p, "p")
        rank_j = combine_rank(K - 1, method, rank, min_prop)
        ins = [_plane(p2, "p")]
        for k, e in enumerate(effects):
            Ke, We, e2 = _pairs_as_rows(e, f"effect plane {k}")
            if (Ke, We) != (K, W):
                raise ValueError(f"effect plane {k} has shape {tuple(e.shape)}, p has {tuple(p.shape)}")
            ins.append(_plane(e2, f"effect plane {k}"))
        in_ptrs, _, in_ld = _plane_set(ins, "p and the effect planes")
        on_dev = ins[0].on_device
        device = p.device if on_dev else None
        skip_keep = skip_ptr = None
        if skip is not None:
            if not on_dev and not _is_torch_tensor(skip):
                skip = np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint32)
            skip_ptr = _block(skip, "skip", (np.int32, np.uint32) if on_dev else (np.uint32,), (W,), on_device=on_dev)[0]
            skip_keep = skip
        if out is None:
            out = [_empty((K, W), np.float64, device), _empty((K, W), np.int32, device)] + [_empty((K, W), np.float64, device) for _ in effects]
        out = tuple(out)
        if len(out) != 2 + len(effects):
            raise ValueError(f"out must hold {2 + len(effects)} planes: p, rep and one per effect plane")
        outs = [_plane(q, f"out[{k}]", dtype=np.int32 if k == 1 else np.float64, shape=(K, W), writeable=True) for k, q in enumerate(out)]
        out_ptrs, oflag, out_ld = _plane_set(outs, "the output planes")
        if bool(oflag) != on_dev:
            raise ValueError("the output planes must live on the side of p (host or device)")
        flags = _io_flags(on_dev)
        pad = [None] * (COMBINE_MAX_EFFECTS - len(effects))
        self._bind_torch_stream(p, *effects, skip_keep, *out)
        self._check(self.lib.illico_combine_pairs(self.h, *in_ptrs, *pad, K, W, max(in_ld, W, 1), skip_ptr, COMBINE_METHODS[method], rank_j, flags,
                                                  *out_ptrs, *pad, max(out_ld, W, 1)))
        return out

    # ---- blocked Wilcoxon tests (include/illico_hip_blocked.h: illico_blocked_from_hists, illico_blocked_from_planes) ----
    @staticmethod
    def _blocked_sizes(counts, GB, n_blocks, ref):
        """``(counts int64 [G, B], G, B, ref code, n_blocks int64 [G])`` of a blocked call over ``GB`` compound groups ``g * B + b``:
        ``n_blocks[g]`` the blocks that hold both a cell of g and a reference cell (those of ``ref``, or of the rest of the block)."""
        if isinstance(n_blocks, bool) or not isinstance(n_blocks, (int, np.integer)) or n_blocks < 1:
            raise ValueError(f"n_blocks must be a positive integer, got {n_blocks!r}")
        B = int(n_blocks)
        counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
        if counts.size != GB or GB % B:
            raise ValueError(f"{GB} compound groups but counts has {counts.size} entries for {B} blocks")
        G = GB // B
        counts = counts.reshape(G, B)
        ref = -1 if ref is None else int(ref)
        if ref < -1 or ref >= G:
            raise ValueError(f"reference {ref} is no group id (0 .. {G - 1})")
        n_r = counts[ref][None, :] if ref >= 0 else counts.sum(axis=0)[None, :] - counts
        return counts, G, B, ref, ((counts > 0) & (n_r > 0)).sum(axis=1).astype(np.int64)

    def _blocked_io(self, G, B, W, sums, out, on_dev, device, with_fc=True):
        """The optional ``sums`` plane ``[G * B, W]`` and the four ``[G, W]`` result planes (p, statistic, fold change, z; the third
        None without ``with_fc``) of a blocked call whose input lives on the side ``on_dev``: (sums, planes, pointers,
        output flag, pitch); the sums as ``_sums_arg`` gives them."""
        sums = _sums_arg(sums, (G * B, W), on_dev, "the input")
        if out is None:
            out = [_empty((G, W), np.float64, device if on_dev else None) if (k != 2 or with_fc) else None for k in range(4)]
        out = tuple(out)
        if len(out) != 4 or (out[2] is not None) != with_fc or any(q is None for k, q in enumerate(out) if k != 2):
            raise ValueError("out must hold 4 planes (p, statistic, fold change, z); the fold change is None exactly when there are no sums")
        if W == 0:
            return sums, out, [None] * 4, 0, 1
        ptrs, oflag, ld = _plane_set([None if q is None else _plane(q, f"output plane {k}", shape=(G, W), writeable=True) for k, q in enumerate(out)],
                                     "output planes")
        return sums, out, ptrs, oflag, ld

    def blocked_from_hists(self, H, flags, *, counts, n_blocks, ref=None, sums=None, tie_correct=True, alternative="two-sided", out=None):
        """Blocked Wilcoxon rank-sum tests from the histograms of ``group_value_hists`` under the compound group coding ``g * B + b``
        (illico_blocked_from_hists; include/illico_hip_blocked.h states the definition).

        ``H`` ``[G * B, W, 256]`` and ``flags`` ``[W]`` as ``group_value_hists`` returns them (numpy, or CUDA tensors); ``counts``: the
        ``G * B`` compound sizes; ``n_blocks``: B; ``ref``: the reference group id, None for the rest of each block.  ``sums``: an
        optional float64 ``[G * B, W]`` plane of compound value sums for the fold change, on the side of ``H`` (under log1p the ``expm1``
        sums of ``group_stats(..., is_log1p=True)``).  Returns ``(p, statistic, fold_change, z)``, float64 ``[G, W]`` on the side of
        ``H``: each group's per-block tests combined by Stouffer's z weighted with ``n_g n_r``.  NaN in every plane where no block
        holds both samples.  The columns of flagged genes are left as they are in ``out`` (four planes with one row stride)."""
        alt = self._alt(alternative)
        H, flags, GB, W, on_dev = _hists_input(H, flags, "G * B")
        counts, G, B, ref, _ = self._blocked_sizes(counts, GB, n_blocks, ref)
        (sums_array, sums_ptr, sums_ld), planes, ptrs, oflag, out_ld = self._blocked_io(G, B, W, sums, out, on_dev, H.device if on_dev else None)
        if W and bool(oflag) != on_dev:
            raise ValueError("the output planes must live on the side of H (host or device)")
        fl = (FLAG_TIE_CORRECT if tie_correct else 0) | _io_flags(on_dev)
        self._bind_torch_stream(H, flags, sums_array, *planes)
        self._check(self.lib.illico_blocked_from_hists(self.h, _ptr(H), _ptr(flags), counts.ctypes.data, G, B, W, ref, sums_ptr, sums_ld, fl, alt,
                                                       *ptrs, max(out_ld, W, 1)))
        return planes

    def blocked_from_planes(self, z, U, row_map, *, counts, ref=None, sums=None, alternative="two-sided", out=None):
        """Blocked Wilcoxon rank-sum tests from the z and U planes of B per-block engine calls made with ``scores=True,
        use_continuity=False`` (illico_blocked_from_planes).

        ``z``, ``U``: float64 ``[B, G, W]`` (numpy, or CUDA tensors; the ``[b, row]`` rows one pitch apart); ``row_map``: int32
        ``[B, G]``, the row of group g in block b's plane set, -1 where g has no cells in b; ``counts``: the ``G * B`` compound
        sizes, ``g * B + b``; ``ref``: the reference group id, None for the rest of each block.  ``sums``: float64 ``[G * B, W]``
        compound value sums; without it there is no fold change (the third plane is None).  Returns ``(p, statistic, fold_change, z)``
        as ``blocked_from_hists`` does."""
        alt = self._alt(alternative)
        on_dev = _is_torch_tensor(z)
        if on_dev != _is_torch_tensor(U) or tuple(z.shape) != tuple(U.shape) or len(z.shape) != 3:
            raise ValueError("z and U must be [B, G, W] planes of one shape on one side (host or device)")
        B, G, W = (int(x) for x in z.shape)
        ins = [_plane(_stacked_rows(q, what, "[b, row] rows of a [B, G, W]"), what) for q, what in ((z, "z"), (U, "U"))]
        in_ptrs, _, in_ld = _plane_set(ins, "z and U")
        row_map = np.ascontiguousarray(row_map, dtype=np.int32)
        if row_map.shape != (B, G):
            raise ValueError(f"row_map must be [B, G] = {(B, G)}, got {row_map.shape}")
        counts, G2, B2, ref, _ = self._blocked_sizes(counts, G * B, B, ref)
        (sums_array, sums_ptr, sums_ld), planes, ptrs, oflag, out_ld = self._blocked_io(G, B, W, sums, out, on_dev, z.device if on_dev else None,
                                                                                        with_fc=sums is not None)
        if W and bool(oflag) != on_dev:
            raise ValueError("the output planes must live on the side of z (host or device)")
        self._bind_torch_stream(z, U, sums_array, *planes)
        self._check(self.lib.illico_blocked_from_planes(self.h, *in_ptrs, max(in_ld or 0, W, 1), row_map.ctypes.data, counts.ctypes.data, G, B, W, ref,
                                                        sums_ptr, sums_ld, _io_flags(on_dev), alt, *ptrs, max(out_ld, W, 1)))
        return planes

    def csr_indices_sorted(self, indices, indptr, n_rows) -> bool:
        i, p = _Buf(indices), _Buf(indptr)
        if i.np_dtype != p.np_dtype:
            i, p = _Buf(np.asarray(indices), np.int64), _Buf(np.asarray(indptr), np.int64)
        res = ctypes.c_int(0)
        self._bind_torch_stream(i.keep, p.keep)
        self._check(self.lib.illico_csr_indices_sorted(self.h, i.ptr, p.ptr, IDX_I32 if i.np_dtype == np.int32 else IDX_I64,
                                                       int(n_rows), FLAG_INPUT_DEVICE if i.on_device else 0,
                                                       ctypes.byref(res)))
        return bool(res.value)

    # ---- measurement hooks ----
    def profile(self, on: bool = True):
        self.set_option("profile", 1 if on else 0)

    def profile_only(self, kernel_name=None):
        """Restrict event timing to one kernel (by name); ``None`` times every kernel again."""
        kid = -1
        if kernel_name is not None:
            names = [self.lib.illico_profile_kernel_name(k).decode() for k in range(self.lib.illico_profile_num_kernels())]
            kid = names.index(kernel_name)
        self.set_option("profile_only", kid)

    def profile_reset(self):
        self._check(self.lib.illico_profile_reset(self.h))

    def profile_get(self) -> dict:
        out = {}
        for k in range(self.lib.illico_profile_num_kernels()):
            ms, n = ctypes.c_double(0), ctypes.c_int64(0)
            self._check(self.lib.illico_profile_get(self.h, k, ctypes.byref(ms), ctypes.byref(n)))
            if n.value:
                out[self.lib.illico_profile_kernel_name(k).decode()] = {"ms": ms.value, "launches": n.value}
        return out


class BoundMatrix:
    """Handle of illico_csr_bind / illico_csc_bind; ``release()`` (or garbage collection) frees the device copy."""

    def __init__(self, engine, handle, shape, keep):
        self.engine, self.h, self.shape, self._keep = engine, handle, shape, keep

    def run(self, col_lb, col_ub, *, is_log1p=False, use_continuity=True, tie_correct=True, alternative="two-sided",
            out=None, device_out=False, defer=False, scores=False):
        """``Engine.run_dense`` of the bound matrix, with its keywords.  A call with the z-score plane computes its chunk directly: the
        windows of the option "bound_ahead_genes" are neither used nor replaced by it (include/illico_hip.h: illico_run_bound_ex)."""
        return self.engine._rank_tests(self._matrix(), col_lb, col_ub, is_log1p, use_continuity, tie_correct, alternative, out, device_out, defer, scores)

    def _matrix(self):
        """The ``_Matrix`` of this handle: the library knows where its arrays live."""
        return _Matrix((self.h,), (), False, self.shape[1], "bound")

    def group_stats(self, col_lb, col_ub, *, is_log1p=False, rest=False, out=None, device_out=False):
        """``Engine.group_stats`` of the bound matrix (illico_group_stats_bound); host planes unless ``device_out`` or ``out``."""
        return self.engine._group_planes("group_stats", self._matrix(), col_lb, col_ub, FLAG_LOG1P if is_log1p else 0, rest, out, device_out)

    def group_moments(self, col_lb, col_ub, *, rest=False, out=None, device_out=False):
        """``Engine.group_moments`` of the bound matrix (illico_group_moments_bound); host planes unless ``device_out`` or ``out``."""
        return self.engine._group_planes("group_moments", self._matrix(), col_lb, col_ub, 0, rest, out, device_out, self.engine._GM_KINDS,
                                         self.engine._GM_NAMES)

    def touch(self):
        """Adopted device arrays were rewritten in place: forget what the context remembers about them (include/illico_hip.h)."""
        self.engine._check(self.engine.lib.illico_matrix_touch(self.engine.h, self.h))

    def release(self):
        if self.h is not None and self.h.value and getattr(self.engine, "h", None) is not None and self.engine.h.value:
            self.engine.lib.illico_matrix_release(self.engine.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _adjust_method(method) -> int:
    try:
        return ADJUST_METHODS[method]
    except (KeyError, TypeError):
        raise ValueError(f"Unknown p-value adjustment method {method!r}: one of {sorted(ADJUST_METHODS)}") from None


def _adjust_n_top(n_top, M) -> int:
    if isinstance(n_top, bool) or not isinstance(n_top, (int, np.integer)):
        raise ValueError(f"n_top must be an integer, got {n_top!r}")
    if n_top < 0 or n_top > M:
        raise ValueError(f"n_top = {n_top} outside [0, {M}] (the plane has {M} columns)")
    return int(n_top)


def _current_device() -> int:
    try:
        if _torch().cuda.is_available():
            return _torch().cuda.current_device()
    except Exception:
        pass
    return 0


_engines = threading.local()


def get_engine(device: int | None = None) -> Engine:
    """Per-thread, per-device engine (a context is single-threaded, include/illico_hip.h)."""
    if device is None:
        device = _current_device()
    cache = getattr(_engines, "cache", None)
    if cache is None:
        cache = _engines.cache = {}
    if device not in cache:
        eng = cache[device] = Engine(device)
        if os.environ.get("ILLICO_PREWARM", "1") != "0":
            # The first call on a host-resident dense matrix pins three staging slots and allocates three device windows (~80 ms of a
            # 190-ms first drop-in call at C2 shape): done here, on a thread of its own, while the caller is still encoding groups.  (The
            # context's lock orders it before the first engine call if that comes sooner.)
            def prewarm(e=eng):
                try:
                    e.set_option("prewarm_host_window_bytes", 256 << 20)
                except Exception:
                    pass
            threading.Thread(target=prewarm, name="illico-prewarm", daemon=True).start()
    return cache[device]
