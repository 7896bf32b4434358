#!/usr/bin/env python3
"""Blocked Wilcoxon tests (illico_amd.blocked) on device-resident input against the loop a user runs without them: one JSON line.

   python tools/bench_blocked.py [--shape clusters_csc,perts_dense] [--values counts|continuous] [--reps 3] [--loop-only]
                                 [--package-root DIR] [--scale 1.0]

Shapes:  clusters_csc   100 000 x 30 000 CSC (device arrays), 30 clusters x 4 blocks, every cluster against the rest of its block
         perts_dense    300 000 x 8000 dense float32 (device tensor), 200 perturbations x 4 blocks against a control
Values:  counts         Poisson counts, nine tenths (CSC) or half (dense) of them zero: the histogram feeder (illico_blocked_from_hists)
         continuous     the same matrix times a float factor per entry: every gene is flagged, the plane feeder (one engine call per
                        block on the block's rows, illico_blocked_from_planes)
blocked_ms   illico_amd.blocked.blocked_planes: host planes (p, statistic, fold change, z) [G, genes]; host clock, the call ends on the host
loop_ms      what gives the same p, statistic and z without the feature: the rows of each block sliced out on the device, B engine calls with
             scores=True, use_continuity=False, their z and U planes copied to the host, and the numpy combination of
             tests/blocked_model.py (combine_planes).  No fold change: the loop's planes do not carry the sums it needs.
             prep_ms / slice_ms / runs_ms / host_ms: its parts -- the blocks' group containers and the host planes (the blocked call builds
             its containers inside its time too), the slicing, the engine calls (set_groups included), the copies down and numpy.
Medians of --reps after one warm-up.  --loop-only runs the loop alone and imports nothing of the feature, so that it can run on a build
of the commit before it: --package-root names the directory that holds that build's illico_amd package.  --split adds one more
blocked call whose engine calls are timed one by one with stream events.  --scale shrinks cells and genes (a rehearsal).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


class DeviceCSC:
    """A CSC matrix whose three arrays are CUDA tensors, with the attributes the chunk loops read."""

    def __init__(self, data, indices, indptr, shape):
        self.data, self.indices, self.indptr, self.shape, self.dtype = data, indices, indptr, tuple(shape), np.dtype(np.float32)

    def rows(self, keep, new_row, n_rows):
        """The rows marked in ``keep`` (bool [N], device) as a DeviceCSC of ``n_rows`` rows; ``new_row``: each kept row's new index."""
        import torch
        M = self.shape[1]
        per_col = (self.indptr[1:] - self.indptr[:-1]).to(torch.int64)
        col = torch.repeat_interleave(torch.arange(M, device=self.data.device), per_col)
        k = keep[self.indices.to(torch.int64)]
        ptr = torch.zeros(M + 1, dtype=torch.int64, device=self.data.device)
        ptr[1:] = torch.cumsum(torch.bincount(col[k], minlength=M), 0)
        return DeviceCSC(self.data[k], new_row[self.indices[k].to(torch.int64)].to(torch.int32), ptr.to(torch.int32), (n_rows, M))


def make_input(shape, values, scale):
    import torch
    sys.path.insert(0, str(ROOT / "tools"))
    from bench_group_stats import dense_counts, to_sparse
    if shape == "clusters_csc":
        N, M, G, zeros, seed = int(100_000 * scale), int(30_000 * scale), 30, 0.9, 11
    else:
        N, M, G, zeros, seed = int(300_000 * scale), int(8000 * scale), 201, 0.5, 13
    B = 4
    X = dense_counts(N, M, zeros, seed)
    if values == "continuous":
        gen = torch.Generator(device="cuda").manual_seed(seed + 1)
        X *= 0.5 + torch.rand((N, M), device="cuda", generator=gen)
        X[0] = 0.5  # (a gene of zeros alone would stay count-valued: every gene takes the plane feeder)
    rng = np.random.default_rng(seed + 2)
    g_codes = rng.permutation(np.arange(N) % G)     # group 0 is the control of perts_dense
    b_codes = rng.integers(0, B, size=N)
    if shape == "clusters_csc":
        d, i, p = to_sparse(X, "csc")
        del X
        torch.cuda.empty_cache()
        X = DeviceCSC(d, i, p, (N, M))
    return X, g_codes, b_codes, G, B, (-1 if shape == "clusters_csc" else 0)


def block_containers(g_codes, b_codes, G, B, ref):
    """Per block: (rows, group container over the groups present, their ids); and the [B, G] row map."""
    from illico_amd.utils.groups import GroupContainer
    row_map = np.full((B, G), -1, dtype=np.int32)
    out = []
    for b in range(B):
        rows = np.flatnonzero(b_codes == b)
        present, local = np.unique(g_codes[rows], return_inverse=True)
        n = np.bincount(local, minlength=present.size).astype(np.int64)
        grp = GroupContainer(local.astype(np.int64), n, np.argsort(local, kind="stable").astype(np.int64),
                             np.concatenate([[0], np.cumsum(n)]).astype(np.int64), int(np.searchsorted(present, ref)) if ref >= 0 else -1)
        row_map[b, present] = np.arange(present.size)
        out.append((rows, grp, present))
    return out, row_map


def take_rows(X, rows):
    """The rows ``rows`` (ascending) of a device tensor or a DeviceCSC, on the device."""
    import torch
    rows_t = torch.as_tensor(rows, device="cuda")
    if not isinstance(X, DeviceCSC):
        return X[rows_t].contiguous()
    keep = torch.zeros(X.shape[0], dtype=torch.bool, device="cuda")
    keep[rows_t] = True
    new_row = torch.zeros(X.shape[0], dtype=torch.int64, device="cuda")
    new_row[rows_t] = torch.arange(rows.size, device="cuda")
    return X.rows(keep, new_row, rows.size)


def loop(eng, X, g_codes, b_codes, G, B, ref, parts):
    """The baseline: slice, B engine calls, host combination.  Returns (p, statistic, z); adds its parts' milliseconds to ``parts``."""
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    from blocked_model import combine_planes
    N, M = X.shape
    torch.cuda.synchronize()
    tp = time.perf_counter()
    blocks, row_map = block_containers(g_codes, b_codes, G, B, ref)
    counts = np.bincount(g_codes * B + b_codes, minlength=G * B).reshape(G, B)
    zs, us = np.zeros((B, G, M)), np.zeros((B, G, M))
    t0 = time.perf_counter()
    subsets = [take_rows(X, rows) for rows, grp, present in blocks]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = []
    for (rows, grp, present), Xb in zip(blocks, subsets):
        eng.set_groups(grp)
        kw = dict(use_continuity=False, scores=True, device_out=True)
        if isinstance(Xb, DeviceCSC):
            got.append(eng.run_sparse("csc", Xb.data, Xb.indices, Xb.indptr, Xb.shape, 0, M, **kw))
        else:
            got.append(eng.run_dense(Xb, 0, M, **kw))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for b, ((rows, grp, present), planes) in enumerate(zip(blocks, got)):
        us[b, :present.size], zs[b, :present.size] = planes[1].cpu().numpy(), planes[3].cpu().numpy()
    res = combine_planes(zs, us, row_map, counts, ref if ref >= 0 else None)
    t3 = time.perf_counter()
    for k, v in (("prep_ms", t0 - tp), ("slice_ms", t1 - t0), ("runs_ms", t2 - t1), ("host_ms", t3 - t2), ("loop_ms", t3 - tp)):
        parts.setdefault(k, []).append(v * 1e3)
    return res


def blocked(eng, X, g_codes, b_codes, G, B, ref, parts):
    import torch
    from illico_amd.blocked import blocked_planes
    from illico_amd.utils.registry import DataHandler, KernelDataFormat, data_handler_registry
    if isinstance(X, DeviceCSC):
        handler = DataHandler(X)
        handler.fmt = KernelDataFormat.CSC
    else:
        handler = data_handler_registry.get(X)
    torch.cuda.synchronize()
    t = time.perf_counter()
    planes, n_flagged = blocked_planes(X, handler, g_codes, b_codes, G, B, ref, False, "two-sided", True, take_rows=take_rows)
    parts.setdefault("blocked_ms", []).append((time.perf_counter() - t) * 1e3)
    return planes, n_flagged


def split_by_call(eng, fn):
    """One more call of ``fn`` with every engine call timed with stream events: {method: [milliseconds, calls]}."""
    import torch
    names = ("group_value_hists", "group_value_hists_sparse", "group_stats", "group_stats_sparse", "blocked_from_hists", "blocked_from_planes",
             "run_dense", "run_sparse")
    events, real = [], {}
    for name in names:
        real[name] = getattr(eng, name)

        def timed(*a, _f=real[name], _n=name, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = _f(*a, **kw)
            e1.record()
            events.append((_n, e0, e1))
            return r
        setattr(eng, name, timed)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for name in names:
            delattr(eng, name)
    out = {}
    for name, e0, e1 in events:
        ms, n = out.get(name, (0.0, 0))
        out[name] = (ms + e0.elapsed_time(e1), n + 1)
    return {k: [round(v[0], 2), v[1]] for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="clusters_csc,perts_dense")
    ap.add_argument("--values", default="counts", choices=("counts", "continuous"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--package-root", default=str(ROOT))
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.package_root).resolve()))
    import torch
    from illico_amd import _lib
    eng = _lib.get_engine()
    res = {"values": a.values, "reps": a.reps, "loop_only": a.loop_only, "package": str(Path(_lib.__file__).resolve().parent), "scale": a.scale}
    for shape in filter(None, a.shape.split(",")):
        X, g_codes, b_codes, G, B, ref = make_input(shape, a.values, a.scale)
        parts: dict = {}
        mine = want = None
        for rep in range(a.reps + 1):
            if not a.loop_only:
                mine, n_flagged = blocked(eng, X, g_codes, b_codes, G, B, ref, parts)
            want = loop(eng, X, g_codes, b_codes, G, B, ref, parts)
        row = {"cells": X.shape[0], "genes": X.shape[1], "groups": G, "blocks": B, "reference": ref}
        row.update({k: round(float(np.median(v[1:])), 2) for k, v in parts.items()})
        if not a.loop_only:
            row["n_flagged_genes"] = n_flagged
            row["loop_over_blocked"] = round(row["loop_ms"] / row["blocked_ms"], 3)
            live = np.arange(G) != ref
            row["same_statistic"] = bool(np.array_equal(mine[1][live], want[1][live]))
            row["same_z_bits"] = bool(np.array_equal(mine[3][live].view(np.uint64), want[2][live].view(np.uint64)))
            row["max_rel_p"] = float(np.nanmax(np.abs(mine[0][live] - want[0][live]) / np.maximum(want[0][live], 1e-300)))
            if a.split:
                row["split"] = split_by_call(eng, lambda: blocked(eng, X, g_codes, b_codes, G, B, ref, {}))
        res[shape] = row
        del X, mine, want
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
