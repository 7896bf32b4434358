#!/usr/bin/env python3
"""All-pairs Welch t-tests (illico_pair_ttest_from_moments, illico_amd.pairwise_markers(method="t-test")) on an MI355X: one JSON line.

   python tools/bench_pairwise_ttest.py [--part kernel,markers] [--reps 10] [--e2e-reps 2] [--only ten_clusters_dense,csc_30_clusters]

kernel    From device-resident moment planes [G = K, W] (means, variances and group sizes drawn from a seed; 1000 K cells) to the
          [K, K, W] planes p, t, df, at K x W = 10 x 2400, 30 x 30 000, 64 x 8000, Welch two-sided and overestim_var.  Two legs,
          alternated in one process, the median of --reps with min - max after one warm-up of each, host clock around work that ends
          in a device synchronise:
            pair   one Engine.pair_ttest_from_moments call;
            loop   the way to the same planes before it existed, on the code as it stands (k_ttest_from_moments is unchanged): K times
                   set_groups with the reference sel[r], Engine.ttest_from_moments, the row gather into [K, K, W].
          The two results are compared bit for bit.  pair_event_ms: the pair call once more between two stream events.
markers   pairwise_markers(method="t-test") end to end at 1M x 2400 dense float32 on the device with ten clusters and 100 000 x 30 000
          as an in-RAM CSC matrix with 30 clusters (a tenth of the cells non-zero, log-normal values), against K calls of
          welch_ttest(reference=r) and the numpy restatement of the combination on the host (tests/markers_model.py).  Host clock, the
          median of --e2e-reps after one warm-up; the combined p and the representatives are compared.
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

SHAPES = ((10, 2400), (30, 30_000), (64, 8000))


def _stats(ms):
    return {"ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def bench_kernel(reps):
    import pandas as pd
    import torch
    from illico_amd._lib import get_engine
    from illico_amd.utils.groups import encode_and_count_groups
    eng = get_engine()
    want = ("p", "t", "df")
    out = {}
    for K, W in SHAPES:
        rng = np.random.default_rng(K * 100_003 + W)
        sizes = rng.multinomial(1000 * K - 2 * K, np.full(K, 1.0 / K)) + 2
        codes = rng.permutation(np.repeat(np.arange(K), sizes))
        _, ovr = encode_and_count_groups(groups=pd.Series([f"c{c:03d}" for c in codes]), ref_group=None)
        ovr = ovr._replace(encoded_ref_group=-1)
        per_ref = [ovr._replace(encoded_ref_group=r) for r in range(K)]
        n = np.asarray(ovr.counts, dtype=np.float64)[:, None]
        mean = rng.uniform(0.05, 3.0, W) * (1.0 + 0.3 * rng.random((K, W)))
        var = rng.uniform(0.1, 2.0, W) * (0.5 + rng.random((K, W)))
        S = mean * n
        Sd, Qd = torch.from_numpy(S).cuda(), torch.from_numpy(var * (n - 1.0) + S * mean).cuda()
        rows = torch.arange(K, device="cuda")
        planes = tuple(torch.empty((K, K, W), dtype=torch.float64, device="cuda") for _ in want)
        block = tuple(torch.empty((K, K, W), dtype=torch.float64, device="cuda") for _ in want)
        row = {"K": K, "W": W, "cells": int(sizes.sum()), "plane_bytes": 8 * K * K * W * len(want)}
        for variant in ("welch", "overestim_var"):
            def pair():
                eng.set_groups(ovr)
                eng.pair_ttest_from_moments(Sd, Qd, variant=variant, want=want, out=planes)

            def loop():
                for r in range(K):
                    eng.set_groups(per_ref[r])
                    got = eng.ttest_from_moments(Sd, Qd, variant=variant, want=want)
                    for k in range(len(want)):
                        block[k][r] = got[k][rows]

            legs = {"pair": pair, "loop": loop}
            times = {k: [] for k in legs}
            for rep in range(reps + 1):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep:
                        times[k].append((time.perf_counter() - t) * 1e3)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            eng.set_groups(ovr)
            a.record()
            eng.pair_ttest_from_moments(Sd, Qd, variant=variant, want=want, out=planes)
            b.record()
            b.synchronize()
            r = {k: _stats(v) for k, v in times.items()}
            r["pair_event_ms"] = round(a.elapsed_time(b), 4)
            r["loop_over_pair"] = round(r["loop"]["ms"] / r["pair"]["ms"], 2)
            r["loop_spread_ms"] = round(r["loop"]["max_ms"] - r["loop"]["min_ms"], 4)
            r["same_bits"] = bool(all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(planes, block)))
            row[variant] = r
        out[f"K{K}_W{W}"] = row
        del Sd, Qd, planes, block
        torch.cuda.empty_cache()
    return out


def _host_restatement(frames, K, M, pval_type):
    """What a user does with K welch_ttest frames today: stacked into [K, K, M] planes, then the model of the combination, in numpy."""
    from markers_model import combine_model
    planes = np.stack([np.stack([df[col].to_numpy().reshape(K, M) for df in frames]) for col in ("p_value", "statistic", "fold_change")])
    return combine_model(planes[0], planes[1:], method=pval_type)


def bench_markers(reps, only):
    import pandas as pd
    import torch
    from bench_group_stats import to_sparse
    from illico_amd import AnnDataLite, pairwise_markers, welch_ttest

    def lognormal(n, m, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        X = torch.log1p(torch.exp(torch.randn((n, m), device="cuda", generator=gen)))
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
        X = lognormal(N, M, seed)
        if name.startswith("csc"):
            from scipy import sparse
            d, i, p = (a.cpu().numpy() for a in to_sparse(X, "csc"))
            del X
            torch.cuda.empty_cache()
            X = sparse.csc_matrix((d, i, p), shape=(N, M))
        labels = np.array([f"c{c:02d}" for c in np.random.default_rng(seed + 1).permutation(np.arange(N) % K)])
        names = sorted(set(labels))
        adata = AnnDataLite(X, obs=pd.DataFrame({"g": pd.Categorical(labels)}))
        times = {"markers_ms": [], "welch_calls_ms": [], "host_combine_ms": []}
        for rep in range(reps + 1):
            ms, mine = timed(lambda: pairwise_markers(adata, True, "g", method="t-test", pval_type="any", corr_method=None))
            ms2, frames = timed(lambda: [welch_ttest(adata, True, "g", r) for r in names])
            t = time.perf_counter()
            want = _host_restatement(frames, K, M, "any")
            ms3 = (time.perf_counter() - t) * 1e3
            if rep:
                for k, v in zip(times, (ms, ms2, ms3)):
                    times[k].append(v)
            del frames
        r = {k: _stats(v) for k, v in times.items()}
        r.update(K=K, genes=M, cells=N)
        r["today_ms"] = round(r["welch_calls_ms"]["ms"] + r["host_combine_ms"]["ms"], 2)
        r["today_over_markers"] = round(r["today_ms"] / r["markers_ms"]["ms"], 2)
        r["same_p_bits"] = bool(np.array_equal(mine["p_value"].to_numpy().view(np.uint64), want[0].reshape(-1).view(np.uint64)))
        r["same_reference"] = bool(np.array_equal(mine["reference"].cat.codes.to_numpy(), want[1].reshape(-1)))
        out[name] = r
        del adata, X, mine, want
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernel,markers")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e-reps", type=int, default=2)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    parts = set(filter(None, a.part.split(",")))
    res = {}
    if "kernel" in parts:
        res["kernel"] = bench_kernel(a.reps)
    if "markers" in parts:
        res["markers"] = bench_markers(a.e2e_reps, set(filter(None, a.only.split(","))))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
