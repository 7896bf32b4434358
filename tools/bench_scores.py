#!/usr/bin/env python3
"""What the z-score plane costs: each shape with and without it, alternating in one process, device-resident input and planes, medians;
then illico_top_by_score at two shapes.  One JSON line.

   python tools/bench_scores.py [--reps 10] [--only c2,c4,...]

Shapes: c2 (dense OVO 300k x 8k x 2k), c4 (the same OVR), c3csc / c3csr (100k x 8k x 2k counts, 90 % zeros, CSC / CSR OVO),
clusters (dense OVR, ten clusters of 100 000 cells x 8k genes); top_by_score at 2000 x 8000 and 5000 x 30 000."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def groups(n, G, n_ref, seed):
    from illico_amd.utils.groups import encode_and_count_groups
    rng = np.random.RandomState(seed)
    if n_ref is None:
        codes = rng.randint(0, G, size=n)
        labels = np.array([f"g{c:05d}" for c in codes])
        return encode_and_count_groups(labels, None)[1]
    codes = np.concatenate([np.zeros(n_ref, dtype=int), 1 + rng.randint(0, G - 1, size=n - n_ref)])
    labels = np.array(["non-targeting" if c == 0 else f"g{c:05d}" for c in codes])
    return encode_and_count_groups(labels, "non-targeting")[1]


def dense_counts(torch, n, m, seed, sparsity=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lam = torch.rand(m, device="cuda", generator=g) * 8.0 + 0.1
    X = torch.poisson(lam.expand(n, m).contiguous(), generator=g).float()
    if sparsity:
        X[torch.rand(n, m, device="cuda", generator=g) < sparsity] = 0
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="c2,c4,c3csc,c3csr,clusters,top")
    a = ap.parse_args()
    want = set(a.only.split(","))
    import torch
    from illico_amd._lib import get_engine
    eng = get_engine()
    res = {"reps": a.reps, "shapes": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def ab(name, run):
        run(False), run(True)  # warm-up of both (scratch, code objects)
        torch.cuda.synchronize()
        t = {False: [], True: []}
        for _ in range(a.reps):
            for z in (False, True):
                t[z].append(timed(lambda: run(z)))
        m0, m1 = float(np.median(t[False])), float(np.median(t[True]))
        res["shapes"][name] = {"without_z_ms": round(m0, 4), "with_z_ms": round(m1, 4), "ratio": round(m1 / m0, 4)}

    def planes(G, M):
        return tuple(torch.empty((G, M), dtype=torch.float64, device="cuda") for _ in range(4))

    for name, n, m, G, ref in (("c2", 300_000, 8000, 2000, 1500), ("c4", 300_000, 8000, 2000, None), ("clusters", 1_000_000, 8000, 10, None)):
        if name not in want:
            continue
        g = groups(n, G, ref, 0) if name != "clusters" else groups(n, G, None, 0)
        eng.set_groups(g)
        X = dense_counts(torch, n, m, 1)
        out = planes(g.counts.size, m)
        ab(name, lambda z: eng.run_dense(X, 0, m, out=out if z else out[:3], device_out=True))
        del X, out
        torch.cuda.empty_cache()
    for fmt in ("csc", "csr"):
        name = "c3" + fmt
        if name not in want:
            continue
        n, m, G = 100_000, 8000, 2000
        g = groups(n, G, 1500, 0)
        eng.set_groups(g)
        X = dense_counts(torch, n, m, 2, sparsity=0.9)
        S = X.to_sparse_csr() if fmt == "csr" else X.t().contiguous().to_sparse_csr()  # CSC = CSR of the transpose
        d, i, p = S.values().contiguous(), S.col_indices().int().contiguous(), S.crow_indices().int().contiguous()
        del X
        out = planes(G, m)
        ab(name, lambda z: eng.run_sparse(fmt, d, i, p, (n, m), 0, m, out=out if z else out[:3], device_out=True))
        del S, d, i, p, out
        torch.cuda.empty_cache()
    if "top" in want:
        for G, M in ((2000, 8000), (5000, 30_000)):
            x = torch.randn((G, M), dtype=torch.float64, device="cuda") * 10
            eng.top_by_score(x, 100)
            torch.cuda.synchronize()
            t = [timed(lambda: eng.top_by_score(x, 100)) for _ in range(a.reps)]
            res["shapes"][f"top_by_score_{G}x{M}"] = {"median_ms": round(float(np.median(t)), 4)}
            del x
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
