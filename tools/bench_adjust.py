#!/usr/bin/env python3
"""Device-resident p-value adjustment (Benjamini-Hochberg) with top-100, at three shapes: one JSON line.

   python tools/bench_adjust.py [--reps 20] [--method bh] [--scipy]

Planes are drawn like the engine's output (u**4, a block of exact zeros, a row of 1.0).  Each shape: one warm-up call, then the median
of --reps calls timed with CUDA events around the call, and the per-kernel times of the engine's profile (a separate pass: the profile
brackets every launch with events).  --scipy also times scipy.stats.false_discovery_control and a stable argsort on the host."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = [(2000, 8000), (5000, 30_000), (100, 120_000)]


def plane(G, M, seed=0):
    p = np.random.default_rng(seed).random((G, M)) ** 4
    p[:, : M // 50] = 0.0
    p[G // 2] = 1.0
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--method", default="bh")
    ap.add_argument("--n-top", type=int, default=100)
    ap.add_argument("--scipy", action="store_true")
    a = ap.parse_args()
    import torch
    from illico_amd._lib import get_engine
    eng = get_engine()
    res = {"method": a.method, "n_top": a.n_top, "shapes": {}}
    for G, M in SHAPES:
        p_host = plane(G, M)
        p = torch.from_numpy(p_host).cuda()
        out = torch.empty_like(p)
        eng.adjust_pvalues(p, a.method, n_top=a.n_top, out=out)  # warm-up (scratch, code objects)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.adjust_pvalues(p, a.method, n_top=a.n_top, out=out)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        eng.profile(True)
        eng.profile_reset()
        eng.adjust_pvalues(p, a.method, n_top=a.n_top, out=out)
        prof = {k: round(v["ms"], 4) for k, v in eng.profile_get().items()}
        eng.profile(False)
        r = {"median_ms": round(float(np.median(times)), 4), "min_ms": round(float(np.min(times)), 4), "kernels_ms": prof}
        if a.scipy:
            from scipy import stats
            t = time.perf_counter()
            stats.false_discovery_control(p_host, axis=1, method=a.method if a.method != "bonferroni" else "bh")
            r["scipy_adjust_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            t = time.perf_counter()
            np.argsort(p_host, axis=1, kind="stable")[:, : a.n_top]
            r["numpy_argsort_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        res["shapes"][f"{G}x{M}"] = r
        del p, out
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
