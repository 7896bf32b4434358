#!/usr/bin/env python3
"""Welch's t-test on device-resident input: the moments pass, the finalisation and both together, against the group-stats pass of
the same shape: one JSON line.

   python tools/bench_ttest.py [--reps 10] [--only c2_dense_dev,...]

Shapes (those of tools/bench_group_stats.py): C2 dense float32 (300 000 x 8000, 2000 groups); C3 (the same shape, 90 % zeros) as CSC
and as CSR; 1M x 2400 dense with ten clusters of 100 000 cells.  Per shape, one warm-up of each leg, then --reps rounds in which the legs
run one after the other (alternating, so that clock and cache state are shared), each host-timed around a synchronising call; the medians:
  group_stats_ms   illico_group_stats_* with the rest planes (the yardstick: the same input bytes)
  moments_ms       illico_group_moments_* with the rest planes, and its ratio to group_stats_ms
  ttest_ms         illico_ttest_from_moments (p and t) from device planes alone
  end_to_end_ms    moments + finalisation, what welch_ttest runs per chunk
and the per-kernel times of the engine's profile for one moments + finalisation call."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_group_stats import dense_counts, groups, to_sparse  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    from illico_amd._lib import get_engine
    from illico_amd.utils.groups import encode_and_count_groups
    eng = get_engine()
    only = set(filter(None, a.only.split(",")))
    res = {"reps": a.reps, "shapes": {}}

    def sync_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def run(name, G, W, stats, moments):
        """stats(out) / moments(out): the two passes of this shape writing the given device planes"""
        if only and name not in only:
            return
        gs_out = tuple(torch.empty((G, W), dtype=dt, device="cuda") for dt in (torch.int64, torch.float64, torch.int64, torch.float64))
        mom = tuple(torch.empty((G, W), dtype=torch.float64, device="cuda") for _ in range(4))
        pt = tuple(torch.empty((G, W), dtype=torch.float64, device="cuda") for _ in range(2))
        legs = {
            "group_stats_ms": lambda: stats(gs_out),
            "moments_ms": lambda: moments(mom),
            "ttest_ms": lambda: eng.ttest_from_moments(*mom, out=pt),
            "end_to_end_ms": lambda: (moments(mom), eng.ttest_from_moments(*mom, out=pt)),
        }
        for fn in legs.values():
            fn()
        times = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, fn in legs.items():
                times[k].append(sync_ms(fn))
        eng.profile(True)
        eng.profile_reset()
        legs["end_to_end_ms"]()
        torch.cuda.synchronize()
        prof = {k: round(v["ms"], 4) for k, v in eng.profile_get().items() if v["launches"]}
        eng.profile_reset()
        legs["group_stats_ms"]()
        torch.cuda.synchronize()
        prof_gs = {k: round(v["ms"], 4) for k, v in eng.profile_get().items() if v["launches"]}
        eng.profile(False)
        med = {k: float(np.median(v)) for k, v in times.items()}
        res["shapes"][name] = {**{k: round(v, 4) for k, v in med.items()},
                               "moments_over_group_stats": round(med["moments_ms"] / med["group_stats_ms"], 3),
                               "tests": G * W, "kernels_ms": prof, "group_stats_kernels_ms": prof_gs}

    N, M, G = 300_000, 8000, 2000
    if not only or "c2_dense_dev" in only:
        X = dense_counts(N, M, 0.5)
        X = torch.log1p(X)
        eng.set_groups(groups(N, G))
        run("c2_dense_dev", G, M, lambda o: eng.group_stats(X, 0, M, rest=True, out=o), lambda o: eng.group_moments(X, 0, M, rest=True, out=o))
        del X
        torch.cuda.empty_cache()
    if not only or only & {"c3_csc_dev", "c3_csr_dev"}:
        X = torch.log1p(dense_counts(N, M, 0.9, seed=2))
        eng.set_groups(groups(N, G))
        for fmt in ("csc", "csr"):
            d, i, p = to_sparse(X, fmt)
            run(f"c3_{fmt}_dev", G, M, lambda o: eng.group_stats_sparse(fmt, d, i, p, (N, M), 0, M, rest=True, out=o),
                lambda o: eng.group_moments_sparse(fmt, d, i, p, (N, M), 0, M, rest=True, out=o))
            del d, i, p
        del X
        torch.cuda.empty_cache()
    if not only or "ten_clusters_dense_dev" in only:
        N, M = 1_000_000, 2400
        X = torch.log1p(dense_counts(N, M, 0.5, seed=3))
        rng = np.random.default_rng(4)
        eng.set_groups(encode_and_count_groups(groups=rng.permutation(np.repeat(np.arange(10), N // 10)), ref_group=None)[1])
        run("ten_clusters_dense_dev", 10, M, lambda o: eng.group_stats(X, 0, M, rest=True, out=o), lambda o: eng.group_moments(X, 0, M, rest=True, out=o))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
