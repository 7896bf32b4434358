#!/usr/bin/env python3
"""All-pairs Wilcoxon tests on device-resident count input: the one-pass pair route against the loop of one one-versus-reference call
per group that it replaces: one JSON line.

   python tools/bench_pairwise.py [--reps 10] [--only ten_clusters_dense_dev,csr_30_clusters_dev] [--loop-only] [--values counts|continuous]

Shapes (the README's): 1M x 2400 dense float32 counts with ten clusters of 100 000 cells; 100 000 x 30 000 counts, 90 % zeros, as CSR
with 30 clusters.  Per shape, one warm-up of each leg, then --reps rounds in which the legs run one after the other, each host-timed
around a synchronising call; the medians:
  pair_ms          illico_group_value_hists_* + illico_pairwise_from_hists (p, U, fold change of all K x K pairs, device planes)
  loop_runs_ms     the K illico_run_* calls of the loop alone (device planes), reference after reference
  loop_ms          the same with the K illico_set_groups calls the loop needs (host work) counted in
  loop_over_pair   loop_runs_ms / pair_ms
and the per-kernel times of the engine's profile for one pair call (kernels_ms: k_pw_hists_* are the histogram pass, k_pw_pairs the
pair kernel with its layout step) and for one loop (loop_kernels_ms).  --loop-only times the loop alone: it needs none of the pair
route's entry points, so it also runs on a build that does not have them (the baseline is then not the code under test)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_group_stats import dense_counts, to_sparse  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--values", choices=["counts", "continuous"], default="counts")
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

    def clusters(N, K, seed):
        codes = np.random.default_rng(seed).permutation(np.arange(N) % K)
        ovr = encode_and_count_groups(groups=codes, ref_group=None)[1]
        return ovr, [ovr._replace(encoded_ref_group=r) for r in range(K)]

    def continuous(n, m, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        X = torch.exp(torch.randn((n, m), device="cuda", generator=gen))
        X[torch.rand((n, m), device="cuda", generator=gen) >= 0.1] = 0
        return X

    def run(name, K, M, ovr, refs, hists, ovo, ranked=None):
        """hists(out): the histogram pass writing (H, flags); ovo(out): one one-versus-reference call writing three device planes;
        ranked(sums, out): with --values continuous, the ranked pair call writing three planes and left"""
        loop_planes = tuple(torch.empty((K, M), dtype=torch.float64, device="cuda") for _ in range(3))

        def loop(runs=None):
            for g in refs:
                eng.set_groups(g)
                if runs is None:
                    ovo(loop_planes)
                else:
                    runs.append(sync_ms(lambda: ovo(loop_planes)))

        legs = {"loop_ms": loop}
        if not a.loop_only and ranked is not None:
            planes = tuple(torch.empty((K, K, M), dtype=torch.float64, device="cuda") for _ in range(3))
            fl = torch.empty((M,), dtype=torch.int32, device="cuda")   # (here: the genes the ranked route left)
            sums = torch.empty((K, M), dtype=torch.float64, device="cuda")

            def pair():
                eng.set_groups(ovr)
                ranked(sums, (*planes, fl))

            legs = {"pair_ms": pair, **legs}
        elif not a.loop_only:
            H = torch.empty((K, M, 256), dtype=torch.int32, device="cuda")
            fl = torch.empty((M,), dtype=torch.int32, device="cuda")
            planes = tuple(torch.empty((K, K, M), dtype=torch.float64, device="cuda") for _ in range(3))

            def pair():
                eng.set_groups(ovr)
                hists((H, fl))
                eng.pairwise_from_hists(H, fl, out=planes)

            legs = {"pair_ms": pair, **legs}
        for fn in legs.values():
            fn()
        times = {k: [] for k in legs}
        times["loop_runs_ms"] = []
        for _ in range(a.reps):
            for k, fn in legs.items():
                times[k].append(sync_ms(fn))
            runs = []
            loop(runs)
            times["loop_runs_ms"].append(sum(runs))
        out = {k: round(float(np.median(v)), 4) for k, v in times.items()}
        eng.profile(True)
        for k, fn in legs.items():
            eng.profile_reset()
            fn()
            torch.cuda.synchronize()
            out["kernels_ms" if k == "pair_ms" else "loop_kernels_ms"] = {n: round(v["ms"], 4) for n, v in eng.profile_get().items() if v["launches"]}
        eng.profile(False)
        if not a.loop_only:
            out["loop_over_pair"] = round(out["loop_runs_ms"] / out["pair_ms"], 3)
            out["left_genes" if ranked is not None else "flagged_genes"] = int((fl != 0).sum().item())
        out["pairs"] = K * (K - 1)
        res["shapes"][name] = out

    cont = a.values == "continuous"
    res["values"] = a.values
    if not only or "ten_clusters_dense_dev" in only:
        N, M, K = 1_000_000, 2400, 10
        X = continuous(N, M, 3) if cont else dense_counts(N, M, 0.5, seed=3)
        ovr, refs = clusters(N, K, 4)

        def ranked_dense(sums, out):
            eng.group_stats(X, 0, M, out=(None, sums))
            eng.pairwise_ranked(X, 0, M, sums=sums, out=out)

        run("ten_clusters_dense_dev", K, M, ovr, refs, lambda o: eng.group_value_hists(X, 0, M, out=o), lambda o: eng.run_dense(X, 0, M, out=o),
            ranked_dense if cont else None)
        del X
        torch.cuda.empty_cache()
    if not only or "csr_30_clusters_dev" in only:
        N, M, K = 100_000, 30_000, 30
        X = continuous(N, M, 5) if cont else dense_counts(N, M, 0.9, seed=5)
        d, i, p = to_sparse(X, "csr")
        cd, ci, cp = to_sparse(X, "csc") if cont and not a.loop_only else (None, None, None)
        del X
        torch.cuda.empty_cache()
        ovr, refs = clusters(N, K, 6)

        def ranked_csc(sums, out):
            eng.group_stats_sparse("csc", cd, ci, cp, (N, M), 0, M, out=(None, sums))
            eng.pairwise_ranked_sparse("csc", cd, ci, cp, (N, M), 0, M, sums=sums, out=out)

        run("csr_30_clusters_dev", K, M, ovr, refs, lambda o: eng.group_value_hists_sparse("csr", d, i, p, (N, M), 0, M, out=o),
            lambda o: eng.run_sparse("csr", d, i, p, (N, M), 0, M, out=o), ranked_csc if cont else None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
