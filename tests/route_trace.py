"""What the route-trace tests share (test_gpu_sparse_route_trace.py, test_gpu_dense_route_trace.py): groups, labels and one
profiled run of a case."""
import numpy as np

import oracle


def groups(labels, test):
    return oracle.encode_and_count_groups(labels, "non-targeting" if test == "ovo" else None)[1]


def labels(rng, sizes):
    """Groups of the given sizes, the first one the reference, cells shuffled."""
    codes = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(codes)
    return np.array(["non-targeting" if c == 0 else f"pert_{c:03d}" for c in codes])


def trace(engine, case):
    """One run of the case under the profiler: (launches per family, planes, groups)."""
    g = groups(case["labels"], case["test"])
    engine.set_groups(g)
    for k, v in case["opts"].items():
        engine.set_option(k, v)
    engine.profile(True)
    engine.profile_reset()
    try:
        got = case["run"](engine, case["X"])
        prof = engine.profile_get()
    finally:
        engine.profile(False)
        for k in case["opts"]:
            engine.set_option(k, 0)
    return {k: v["launches"] for k, v in prof.items()}, got, g
