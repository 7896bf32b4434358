#!/usr/bin/env python3
"""Per-group non-zero counts and exact value sums (illico_group_stats_*, rest planes on), at five shapes: one JSON line.

   python tools/bench_group_stats.py [--reps 10] [--only c2_dense_dev,...]

Shapes: C2 dense float32 (300 000 x 8000, 2000 groups) device-resident and host-resident; C3 (the same shape, 90 % zeros) as CSC and
as CSR, device-resident; 1M x 2400 dense with ten clusters of 100 000 cells; C3 shape as CSC with 30 000 groups of ten cells.  Each
shape: one warm-up call, then the median of --reps calls (host-timed around a synchronising call: host input / host output are part of
the call), the GB/s on algorithmic bytes (every stored value / index read once, the planes written once), and the per-kernel times of
the engine's profile (a separate call: the profile brackets every launch with events)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def dense_counts(n, m, zeros, seed=0):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lam = (torch.rand((1, m), device="cuda", generator=gen) * 8).expand(n, m).contiguous()
    X = torch.poisson(lam, generator=gen).to(torch.float32)
    del lam
    X[torch.rand((n, m), device="cuda", generator=gen) < zeros] = 0
    return X


def to_sparse(X, fmt):
    """Device (data float32, indices int32, indptr int32) of X as CSC / CSR, built block by block (entries ascending within a column /
    row)."""
    import torch
    n, m = X.shape
    outer, step = (m, 500) if fmt == "csc" else (n, 20_000)
    data, ind, cnt = [], [], []
    for a in range(0, outer, step):
        b = min(outer, a + step)
        Xb = X[:, a:b].t().contiguous() if fmt == "csc" else X[a:b]
        nz = Xb.nonzero()
        data.append(Xb[nz[:, 0], nz[:, 1]])
        ind.append(nz[:, 1].to(torch.int32))
        cnt.append(torch.bincount(nz[:, 0], minlength=b - a))
        del Xb, nz
    ptr = torch.zeros(outer + 1, dtype=torch.int64, device=X.device)
    ptr[1:] = torch.cumsum(torch.cat(cnt), 0)
    return torch.cat(data), torch.cat(ind), ptr.to(torch.int32)


def groups(n, G, seed=1):
    from illico_amd.utils.groups import encode_and_count_groups
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, G, size=n)
    codes[:G] = np.arange(G)
    return encode_and_count_groups(groups=codes, ref_group=None)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    from illico_amd._lib import get_engine
    eng = get_engine()
    only = set(filter(None, a.only.split(",")))
    res = {"rest": True, "shapes": {}}

    def timed(name, fn, alg_bytes):
        if only and name not in only:
            return
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        eng.profile(True)
        eng.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = {k: round(v["ms"], 4) for k, v in eng.profile_get().items() if v["launches"]}
        eng.profile(False)
        med = float(np.median(times))
        res["shapes"][name] = {"median_ms": round(med, 4), "min_ms": round(float(np.min(times)), 4),
                               "gbps": round(alg_bytes / med / 1e6, 1), "kernels_ms": prof}

    def dev_out(G, W):
        return tuple(torch.empty((G, W), dtype=dt, device="cuda") for dt in (torch.int64, torch.float64, torch.int64, torch.float64))

    N, M, G = 300_000, 8000, 2000
    planes = G * M * 32
    X = dense_counts(N, M, 0.5)
    eng.set_groups(groups(N, G))
    out = dev_out(G, M)
    timed("c2_dense_dev", lambda: eng.group_stats(X, 0, M, rest=True, out=out), N * M * 4 + planes)
    if not only or "c2_dense_host" in only:
        Xh = X.cpu().numpy()
        timed("c2_dense_host", lambda: eng.group_stats(Xh, 0, M, rest=True, out=out), N * M * 4 + planes)
        del Xh
    del X
    torch.cuda.empty_cache()

    X = dense_counts(N, M, 0.9, seed=2)
    for fmt in ("csc", "csr"):
        d, i, p = to_sparse(X, fmt)
        nnz = int(d.numel())
        timed(f"c3_{fmt}_dev", lambda: eng.group_stats_sparse(fmt, d, i, p, (N, M), 0, M, rest=True, out=out), nnz * 8 + planes)
        res["shapes"].get(f"c3_{fmt}_dev", {})["nnz"] = nnz
        del d, i, p
    from illico_amd.utils.groups import encode_and_count_groups
    eng.set_groups(encode_and_count_groups(groups=np.random.default_rng(5).permutation(np.repeat(np.arange(30_000), N // 30_000)), ref_group=None)[1])
    out30 = dev_out(30_000, M)
    d, i, p = to_sparse(X, "csc")
    timed("c3_csc_30000x10_dev", lambda: eng.group_stats_sparse("csc", d, i, p, (N, M), 0, M, rest=True, out=out30), int(d.numel()) * 8 + 30_000 * M * 32)
    del d, i, p, X, out30
    torch.cuda.empty_cache()

    N, M = 1_000_000, 2400
    X = dense_counts(N, M, 0.5, seed=3)
    rng = np.random.default_rng(4)
    eng.set_groups(encode_and_count_groups(groups=rng.permutation(np.repeat(np.arange(10), N // 10)), ref_group=None)[1])
    out10 = dev_out(10, M)
    timed("ten_clusters_dense_dev", lambda: eng.group_stats(X, 0, M, rest=True, out=out10), N * M * 4 + 10 * M * 32)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
