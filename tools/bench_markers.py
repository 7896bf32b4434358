#!/usr/bin/env python3
"""Per-group marker statistics (illico_combine_pairs, illico_amd.pairwise_markers) on an MI355X: one JSON line.

   python tools/bench_markers.py [--part combine,markers] [--reps 20] [--e2e-reps 3] [--only ten_clusters_dense,csc_30_clusters]

combine   Engine.combine_pairs on device planes (p and three effect planes, uniform p^4) at K = 10, 30, 64 x W = 2400, 30 000, and at
          K = 128, 256 x W = 2400, for the three methods ("some" at its default rank): the median of --reps calls timed with stream
          events around the call, after one warm-up.  p_bytes = 8 K (K - 1) W, what the kernel must read of p; hbm_ms = p_bytes over HBM_RATE, the rate the MI355X
          sustains on a streaming read; over_hbm = ms / hbm_ms.
markers   pairwise_markers end to end at the two shapes the README quotes for the ranked route -- 1M x 2400 dense float32 on the device
          with ten clusters; 100 000 x 30 000 as an in-RAM CSC matrix with 30 clusters; a tenth of the cells non-zero, continuous values --
          against what a user does without it: pairwise_wilcoxon(scores=True) (the same code as before this entry point existed: the
          call without a sink is unchanged) followed by the numpy restatement of the combination on the host (tests/markers_model.py).
          Host clock around each call (both end on the host), the median of --e2e-reps after one warm-up; the two results are compared.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

HBM_RATE = 6.3e12  # bytes / s: what a streaming read achieves on an MI355X (8 TB/s on paper)


def bench_combine(reps):
    import torch
    from illico_amd._lib import get_engine
    eng = get_engine()
    out = {}
    for K, W in [(K, W) for K in (10, 30, 64) for W in (2400, 30_000)] + [(128, 2400), (256, 2400)]:
        gen = torch.Generator(device="cuda").manual_seed(K * 100_003 + W)
        P = torch.rand((K, K, W), device="cuda", dtype=torch.float64, generator=gen) ** 4
        effects = [torch.randn((K, K, W), device="cuda", dtype=torch.float64, generator=gen) for _ in range(3)]
        planes = (torch.empty((K, W), dtype=torch.float64, device="cuda"), torch.empty((K, W), dtype=torch.int32, device="cuda"),
                  *[torch.empty((K, W), dtype=torch.float64, device="cuda") for _ in effects])
        p_bytes = 8 * K * (K - 1) * W
        row = {"p_bytes": p_bytes, "hbm_ms": round(p_bytes / HBM_RATE * 1e3, 5)}
        for method in ("all", "any", "some"):
            eng.combine_pairs(P, effects, method=method, out=planes)
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.combine_pairs(P, effects, method=method, out=planes)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            row[method] = {"ms": round(float(np.median(ms)), 5), "min_ms": round(float(np.min(ms)), 5),
                           "over_hbm": round(float(np.median(ms)) / (p_bytes / HBM_RATE * 1e3), 2)}
        out[f"K{K}_W{W}"] = row
        del P, effects, planes
        torch.cuda.empty_cache()
    return out


def _host_restatement(df, K, M, pval_type):
    """What a user does with pairwise_wilcoxon's frame today: the [K, K, M] planes, then the model of the combination, in numpy."""
    from markers_model import combine_model
    planes = np.full((4, K, K, M), np.nan)
    off = np.flatnonzero(~np.eye(K, dtype=bool).reshape(-1))  # the frame is reference-major, then pert, then gene: row r * K + g
    for k, col in enumerate(("p_value", "statistic", "fold_change", "z_score")):
        planes[k].reshape(K * K, M)[off] = df[col].to_numpy().reshape(K * (K - 1), M)
    return combine_model(planes[0], planes[1:], method=pval_type)


def bench_markers(reps, only):
    import pandas as pd
    import torch
    from bench_group_stats import to_sparse
    from illico_amd import AnnDataLite, pairwise_markers, pairwise_wilcoxon

    def continuous(n, m, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        X = torch.exp(torch.randn((n, m), device="cuda", generator=gen))
        X[torch.rand((n, m), device="cuda", generator=gen) >= 0.1] = 0
        return X

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    out = {}
    for name, N, M, K, seed in (("ten_clusters_dense", 1_000_000, 2400, 10, 3), ("csc_30_clusters", 100_000, 30_000, 30, 5)):
        if only and name not in only:
            continue
        X = continuous(N, M, seed)
        if name.startswith("csc"):
            from scipy import sparse
            d, i, p = (a.cpu().numpy() for a in to_sparse(X, "csc"))
            del X
            torch.cuda.empty_cache()
            X = sparse.csc_matrix((d, i, p), shape=(N, M))
        labels = np.array([f"c{c:02d}" for c in np.random.default_rng(seed + 1).permutation(np.arange(N) % K)])
        adata = AnnDataLite(X, obs=pd.DataFrame({"g": pd.Categorical(labels)}))
        row = {"K": K, "genes": M, "cells": N}
        for pval_type in ("any", "some", "all"):
            legs = {"markers_ms": lambda: pairwise_markers(adata, False, "g", pval_type=pval_type, corr_method=None),
                    "pairs_ms": lambda: pairwise_wilcoxon(adata, False, "g", scores=True)}
            times = {k: [] for k in legs}
            times["host_combine_ms"] = []
            for rep in range(reps + 1):
                for k, fn in legs.items():
                    ms, res = timed(fn)
                    if rep:
                        times[k].append(ms)
                    if k == "markers_ms":
                        mine = res
                    else:
                        t = time.perf_counter()
                        want = _host_restatement(res, K, M, pval_type)
                        if rep:
                            times["host_combine_ms"].append((time.perf_counter() - t) * 1e3)
                    del res
            r = {k: round(float(np.median(v)), 2) for k, v in times.items()}
            r["today_ms"] = round(r["pairs_ms"] + r["host_combine_ms"], 2)
            r["today_over_markers"] = round(r["today_ms"] / r["markers_ms"], 2)
            r["same_p_bits"] = bool(np.array_equal(mine["p_value"].to_numpy().view(np.uint64), want[0].reshape(-1).view(np.uint64)))
            r["same_reference"] = bool(np.array_equal(mine["reference"].cat.codes.to_numpy(), want[1].reshape(-1)))
            r["attrs"] = dict(mine.attrs)
            row[pval_type] = r
            del mine, want
        out[name] = row
        del adata, X
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="combine,markers")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    parts = set(filter(None, a.part.split(",")))
    res = {"hbm_rate": HBM_RATE}
    if "combine" in parts:
        res["combine"] = bench_combine(a.reps)
    if "markers" in parts:
        res["markers"] = bench_markers(a.e2e_reps, set(filter(None, a.only.split(","))))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
