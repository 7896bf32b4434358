"""Inputs that sit on the switch points of dense OVR's value-range parts route: k_ovr_partition /
k_ovr_partition_packed (kernels_ovr_partition.h) followed by k_ovr_rank_gene_parts (kernels_ovr_parts.h), sized by run_ovr_dense_parts
(keyed_impl.h).  The route decides per gene on the device -- quota plan or skewed plan, which coarse bucket gets a part of its own, when
a part is streamed, when a gene leaves for k_ovr_gene, how a packed key gets its group code back -- and every decision is a comparison
against a literal or a capacity.

The first half restates, in plain numpy and from the headers, what the driver and the kernels compute: the sizing, where a key lies in
each of the three layouts the partition can read, which keys the bucket range is sampled from, the coarse buckets, the plan and the rank
kernel's decision per part.  The second half builds the cases: one BOUNDARY GENE (column B of 12) whose keys lie on a grid that is linear
in the key, so that a bucket's census is chosen, not drawn; the other genes are ordinary, shorter, and by the model all of them stay on
the route.  tests/test_ovr_parts_cases_host.py holds the cases to the table of section 12b on the CPU; tests/test_gpu_ovr_parts_edges.py
holds the restatement to the build (test_an_edge_is_an_edge) and the kernels to the oracle.

A case is its name, "<edge>-<form>-<side>": form 4 (float32), 8 (float64) or 8i (int64), the sides of an edge one key, one cell or one
group apart.  Imports numpy, the oracle and tests/gene_edge_cases.py only.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import oracle
from gene_edge_cases import MAX_LDS, MAX_SHARE, csco_fixed_lds_bytes, csco_key_cap, int_of, keys_of  # noqa: F401 (re-exported for the tests)

N_GENES = 12
B = 5                       # the boundary gene
EMPTY, ONE_VALUE = 3, 6     # ordinary genes: all zero / one value where non-zero
MOST = 6000                 # non-zeros of an ordinary gene at most

# ---------------------------------------------------------------------------------------------------------------------------------------
# The restatement.  kernels_ovr_partition.h, kernels_ovr_parts.h, kernels_ovo_compact.h, keyed_impl.h, core.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
OVRP_NT = 512
OVRP_LG = 13
OVRP_NB = 1 << OVRP_LG
OVRP_PMAX = 255
OVRP_LONG_ROWS = 4096
GCMP_BLOCK_ROWS = 1024
CSCO_CNT_SHIFT = 40
LAYOUTS = ("packed", "padded", "plain")
LAYOUT_OPTS = {"packed": {}, "padded": {"no_ovr_packed_partition": 1}, "plain": {"no_packed_dense": 1}}


def keys(values, key_size):
    """common.h: key_of for any value -- order-preserving unsigned keys, zero (of either sign) at 0x80..0."""
    v = np.asarray(values)
    if v.dtype.kind == "i":
        assert key_size == 8
        return np.ascontiguousarray(v, dtype=np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    if key_size == 4:
        b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
        top, full = np.uint64(1 << 31), np.uint64((1 << 32) - 1)
    else:
        b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64).copy()
        top, full = np.uint64(1 << 63), np.uint64((1 << 64) - 1)
    b[b == top] = 0
    return np.where(b & top != 0, b ^ full, b | top)


def zero_key(key_size):
    return np.uint64(1 << (8 * key_size - 1))


def key_cap_at(G, lg, key_size, lds_max):
    """kernels_ovr_rank.h: csco_key_cap at any LDS budget"""
    fixed = csco_fixed_lds_bytes(G, lg)
    if fixed + 1024 * 4 + 64 > lds_max:
        return 0
    return min((lds_max - fixed) // key_size - 4, 65535 - 4)


Sizing = namedtuple("Sizing", ["route", "half", "lg", "key_cap", "K", "cap"])


def sizing(G, key_size, N, max_group, parts_cap=0, whole=False):
    """keyed_impl.h: run_ovr_dense_parts -- half, lg, key_cap, cap (ovr_parts_cap rounded down to 1024, never below 1024), and whether the
    route runs at all (cap * OVRP_PMAX < N: it does not).  K = key_cap & ~1023: the longest part the rank kernel ranks in LDS."""
    ok = G <= 65535 and max_group < (1 << 23) and float(max_group) * 2.0 * float(N) < float(1 << CSCO_CNT_SHIFT)
    kh = key_cap_at(G, 13, key_size, MAX_LDS // 2)
    half = (not whole) and kh >= 8192 and (kh & ~1023) * 128 >= N
    budget = MAX_LDS // 2 if half else MAX_LDS
    lg = 13 if half else 14
    if key_cap_at(G, lg, key_size, budget) < 12288 and not half:
        lg = 13
    key_cap = key_cap_at(G, lg, key_size, budget)
    K = cap = key_cap & ~1023
    if cap < 4096:
        ok = False
    if parts_cap > 0:
        cap = min(cap, max(1024, parts_cap & ~1023))
    if cap * OVRP_PMAX < N:
        ok = False
    return Sizing(ok, half, lg, key_cap, K, cap)


Blocks = namedtuple("Blocks", ["g0", "g1", "out", "rows", "is_long", "pk_len"])


def lay_out_packed_blocks(counts):
    """core.hip: lay_out_packed_blocks without a reference group -- consecutive groups, a block closes at GCMP_BLOCK_ROWS rows and starts
    at a multiple of 64 key slots; long: more than OVRP_LONG_ROWS rows and at most 64 groups."""
    g0, g1, out, rows_b = [], [], [], []
    pos = rows = 0
    is_open = False
    for g, n in enumerate(counts):
        if not is_open:
            g0.append(g)
            out.append(pos)
            rows, is_open = 0, True
        rows += int(n)
        if rows >= GCMP_BLOCK_ROWS:
            g1.append(g + 1)
            rows_b.append(rows)
            pos += (rows + 63) & ~63
            is_open = False
    if is_open:
        g1.append(len(counts))
        rows_b.append(rows)
        pos += (rows + 63) & ~63
    g0, g1, out, rows_b = (np.array(a, dtype=np.int64) for a in (g0, g1, out, rows_b))
    return Blocks(g0, g1, out, rows_b, (rows_b > OVRP_LONG_ROWS) & (g1 - g0 <= 64), pos)


Maps = namedtuple("Maps", ["order", "posptr", "blocks", "block_of", "plain", "padded"])


def position_maps(codes):
    """Where a cell's key lies: `plain` -- the group-contiguous rows of the plain transposition (cells of a group in cell order: the
    stable argsort of GroupContainer.indices); `padded` -- the padded rows of k_group_compact<PACK = false> (a block's groups back to
    back from the block's first slot on; what lay_out_padded_codes labels); block_of -- the block of the cell's group.  The packed rows
    depend on the gene: packed_offsets."""
    codes = np.asarray(codes, dtype=np.int64)
    N = codes.size
    counts = np.bincount(codes)
    order = np.argsort(codes, kind="stable")
    posptr = np.concatenate([[0], np.cumsum(counts)])
    bl = lay_out_packed_blocks(counts)
    blk_of_group = np.repeat(np.arange(bl.g0.size), bl.g1 - bl.g0)
    plain = np.empty(N, dtype=np.int64)
    plain[order] = np.arange(N)
    blk_in_order = blk_of_group[codes[order]]
    padded = np.empty(N, dtype=np.int64)
    padded[order] = bl.out[blk_in_order] + np.arange(N) - posptr[bl.g0[blk_in_order]]
    return Maps(order, posptr, bl, blk_of_group[codes], plain, padded)


def packed_offsets(maps, nz):
    """k_group_compact<PACK = true>: a gene's non-zero keys, block after block, a block's groups back to back, a group's cells in cell
    order -- the offset of every non-zero cell's key inside its block (-1 for a zero), and the keys per block (blk_cnt)."""
    nzo = nz[maps.order].astype(np.int64)
    before = np.cumsum(nzo) - nzo
    bio = maps.block_of[maps.order]
    start = before[maps.posptr[maps.blocks.g0]]
    off = np.full(nz.size, -1, dtype=np.int64)
    off[maps.order] = np.where(nzo != 0, before - start[bio], -1)
    return off, np.bincount(maps.block_of[nz], minlength=maps.blocks.g0.size)


def sampled(maps, nz, layout, coop=True):
    """The cells whose keys the bucket range is taken from: every 8th row of OVRP_NT positions (k_ovr_partition over the plain and the
    padded rows, the zero key left out); every 8th block (k_ovr_partition_packed); in its COOP form -- some block is long and
    no_ovr_part_coop is off -- every long block, every 8th 64-key piece of it."""
    if layout == "plain":
        return nz & ((maps.plain // OVRP_NT) % 8 == 0)
    if layout == "padded":
        return nz & ((maps.padded // OVRP_NT) % 8 == 0)
    off, _ = packed_offsets(maps, nz)
    by_block = maps.block_of % 8 == 0
    if coop and maps.blocks.is_long.any():
        by_block = np.where(maps.blocks.is_long[maps.block_of], off % (64 * 8) < 64, by_block)
    return nz & by_block


def buckets_of(k, sampled_keys):
    """kernels_ovr_rank.h: OvrBuckets over OVRP_LG bits, last = OVRP_NB - 1 (ovrp_buckets).  No sampled key: have_range is false, kmin
    = kmax = 0.  Returns (bucket of every key, shift, have_range)."""
    have = sampled_keys.size > 0
    kmin, kmax = (int(sampled_keys.min()), int(sampled_keys.max())) if have else (0, 0)
    shift = max(0, (kmax - kmin).bit_length() - OVRP_LG)
    above = k > np.uint64(kmin)
    d = np.where(above, k - np.uint64(kmin), np.uint64(0)) >> np.uint64(shift)
    return np.minimum(d, np.uint64(OVRP_NB - 1)).astype(np.int64), shift, have


GeneModel = namedtuple("GeneModel", ["n", "mx", "skew", "quota", "nbig", "n_parts", "sizes", "empty", "top", "bad", "streamed", "flagged",
                                     "stays", "have_range", "shift", "n0", "nneg"])


def plan_of(hist, cap):
    """ovrp_plan / ovrp_assign_parts_skewed: (skew, quota, nbig, n_parts or None when bad, part id of every bucket)."""
    hist = np.asarray(hist, dtype=np.int64)
    n, mx = int(hist.sum()), int(hist.max())
    excl = np.cumsum(hist) - hist
    skew = mx * 4 > cap
    if not skew:
        quota = cap - mx
        n_parts = (n - 1) // quota + 1 if n else 0
        return skew, quota, 0, (None if n_parts > OVRP_PMAX else n_parts), excl // quota
    half = cap // 2
    big = hist > half
    nbig = int(big.sum())
    if nbig > 128:
        return skew, half, nbig, None, None
    bigs_before = np.cumsum(big) - big
    big_keys_before = np.cumsum(hist * big) - hist * big
    pid = (excl - big_keys_before) // half + 2 * bigs_before + big
    top = int(pid[hist > 0].max())
    return skew, half, nbig, (None if top >= OVRP_PMAX else top + 1), pid


def gene_model(k, sampled_keys, cap, K, n_cells, key_size):
    """One gene through the partition and the rank kernel: k -- its non-zero keys.  A part of more than K keys is streamed when it holds
    one value and flags the gene when it does not (k_ovr_rank_gene_parts); a gene without a plan (bad) or with a flagged part leaves."""
    n0, nneg = n_cells - k.size, int((k < zero_key(key_size)).sum())
    bkt, shift, have = buckets_of(k, sampled_keys)
    hist = np.bincount(bkt, minlength=OVRP_NB)
    skew, quota, nbig, n_parts, pid = plan_of(hist, cap) if k.size else (False, cap, 0, 0, None)
    mx = int(hist.max())
    if n_parts is None:
        return GeneModel(k.size, mx, skew, quota, nbig, None, None, None, None, True, (), (), False, have, shift, n0, nneg)
    part = pid[bkt] if k.size else np.zeros(0, dtype=np.int64)
    sizes = np.bincount(part, minlength=n_parts)
    streamed, flagged = [], []
    for p in np.flatnonzero(sizes > K):
        kp = k[part == p]
        (streamed if kp.min() == kp.max() else flagged).append(int(p))
    return GeneModel(k.size, mx, skew, quota, nbig, n_parts, sizes, tuple(np.flatnonzero(sizes == 0)), n_parts - 1, False, tuple(streamed),
                     tuple(flagged), not flagged, have, shift, n0, nneg)


def key_size_of(X):
    return 4 if X.dtype == np.float32 else 8


def case_sizing(c, whole=False, parts_cap=None):
    counts = np.bincount(codes_of(c.labels))
    return sizing(counts.size, key_size_of(c.X), c.X.shape[0], int(counts.max()), c.opts.get("ovr_parts_cap", 0) if parts_cap is None else parts_cap,
                  whole)


def codes_of(labels):
    return np.unique(labels, return_inverse=True)[1].reshape(-1)


def case_model(c, layout, coop=True, whole=False, genes=None):
    """(sizing, [GeneModel per gene]) of a case in one layout under the case's own options."""
    sz = case_sizing(c, whole)
    maps = position_maps(codes_of(c.labels))
    ks = key_size_of(c.X)
    out = []
    for j in (range(c.X.shape[1]) if genes is None else genes):
        k = keys(c.X[:, j], ks)
        nz = k != zero_key(ks)
        out.append(gene_model(k[nz], k[sampled(maps, nz, layout, coop)], sz.cap, sz.K, c.X.shape[0], ks))
    return sz, out


def leaves(c, layout, **kw):
    """Does k_ovr_gene run in that call?  (The whole batch when the route does not apply, a flagged gene's range otherwise.)"""
    sz, genes = case_model(c, layout, **kw)
    return not sz.route or any(not g.stays for g in genes)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases
# ---------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", ["name", "edge", "form", "side", "labels", "X", "opts", "info"])
# expect: side -> "stays" (no k_ovr_gene in the call), "leaves" (the boundary gene goes to k_ovr_gene), "no-route" (no partition at all),
# None (what the model says, per layout).  step: what one side differs from the one before in ("key", "cell", "group", "place": the same
# values in other cells, "cells": one cell per group, None: cases of their own).
Edge = namedtuple("Edge", ["sides", "expect", "forms", "step", "parts_cap"], defaults=(1024,))
F48, F48I = ("4", "8"), ("4", "8", "8i")
STAYS2 = {"lo": "stays", "hi": "stays"}
EDGES = {
    "A": Edge(("lo", "hi"), STAYS2, F48I, "key"),                               # mx * 4 > cap
    "B": Edge(("lo", "hi"), STAYS2, F48, "key"),                                # c > cap / 2
    "B-first": Edge(("lo", "hi"), STAYS2, F48, "key"),                          # ... the crowded bucket first in value order
    "B-adj": Edge(("lo", "hi"), STAYS2, F48, "key"),                            # ... two big buckets side by side
    "B-own": Edge(("lo", "hi"), STAYS2, F48, "key", 0),                         # ... at the route's own cap: K / 2 keys, then more than K / 2 behind
    "C": Edge(("lo", "hi"), {"lo": "stays", "hi": "leaves"}, F48I, "key"),      # quota plan: 255 / 256 parts
    "D": Edge(("lo", "hi"), {"lo": "stays", "hi": "no-route"}, F48, "cell"),    # cap * 255 < N
    "E": Edge(("lo", "hi", "hi2"), {"lo": "stays", "hi": "leaves", "hi2": "leaves"}, F48I, "key"),   # top id 254 / 255; 129 big buckets
    "F": Edge(("lo", "hi"), STAYS2, F48I, "key"),                               # n > K: one value, streamed
    "F-neg": Edge(("lo", "hi"), STAYS2, F48, "key"),                            # ... a negative value
    "Fp": Edge(("lo", "hi"), {"lo": "stays", "hi": "leaves"}, F48, "key"),      # n > K: two values, flagged
    "Fp-neg": Edge(("lo", "hi"), {"lo": "stays", "hi": "leaves"}, F48, "key"),
    "G": Edge(("lo",), {"lo": "stays"}, F48, None, 0),                          # a part of cap - 1 keys at the route's own cap
    "T": Edge(("lo", "hi"), STAYS2, F48, "key"),                                # the last bucket reaches into a part no bucket starts
    "H": Edge(("lo", "hi-out", "hi-none", "hi-one", "hi-none-big"),                # the sampled key range
              {"lo": "stays", "hi-out": None, "hi-none": None, "hi-one": None, "hi-none-big": "leaves"}, F48, "place"),
    "I": Edge(("lo", "hi", "65"), {"lo": "stays", "hi": "stays", "65": "stays"}, F48, None),
    "J": Edge(("lo", "hi", "65"), {"lo": "stays", "hi": "stays", "65": "stays"}, F48, None),
    "K": Edge(("63", "64", "65", "empty-first", "empty-mid", "empty-last", "empty-two", "sparse"), {}, F48, None),
}
NAMES = tuple(f"{e}-{f}-{s}" for e, spec in EDGES.items() for f in spec.forms for s in spec.sides)
SIZES = (9000, 5000, 4700, 3000, 1700, 1100, 900, 300, 90, 10)   # the groups of the capacity edges, scaled to the cells a case needs
TOP = 8000               # the bucket of the largest key of a boundary gene (beyond 4096: the key range then has LG + sh bits)


REDRAW = {"J-4": 1}      # a draw that breaks the share rule of tests/test_ovr_parts_cases_host.py takes its next draw


def _seed(text):
    return zlib.crc32((text + "+" * REDRAW.get(text, 0)).encode()) & 0x7FFFFFFF


def split(name):
    """(edge, form, side) of a case name; edges and sides may hold dashes themselves."""
    for edge in sorted(EDGES, key=len, reverse=True):
        if name.startswith(edge + "-"):
            form, _, side = name[len(edge) + 1:].partition("-")
            if form in F48I and side in EDGES[edge].sides:
                return edge, form, side
    raise KeyError(name)


def grid(b, count, sh=10, values=0):
    """`count` keys of coarse bucket b as offsets d from the gene's smallest key: distinct ones (values = 0), or dealt over `values`
    neighbouring keys.  A bucket is d >> sh: it holds 1 << sh distinct keys."""
    if values:
        return (b << sh) + np.arange(count, dtype=np.int64) % values
    assert count <= 1 << sh
    return (b << sh) + np.arange(count, dtype=np.int64)


def values_of(d, form, sh=10, sign=1):
    """The values whose keys are kmin + d: float32 1 + d ulp (every key offset is one ulp from 1.0 on, through 16.0), the same numbers
    as float64 (key offsets d << 29: the same buckets), the integers 1 + d.  sign = -1: the negatives whose keys run the same way."""
    d = np.asarray(d, dtype=np.int64)
    e = d if sign > 0 else ((OVRP_NB << sh) - 1) - d
    if form == "8i":
        return sign * (1 + e)
    v = (np.uint32(0x3F800000) + e.astype(np.uint32)).view(np.float32)
    return sign * (v if form == "4" else v.astype(np.float64))


def _ordinary(rng, j, n, most=MOST):
    """Ordinary gene j in float64, at most `most` non-zeros: continuous (values float32 cannot hold), ties at quarters, negatives, one
    value where non-zero, all zero, counts beyond 255."""
    dens = (0.3, 0.45, 0.5, 0.0, 0.2, 0.0, 0.25, 0.05, 0.4, 0.1, 0.35, 0.02)[j]
    k = min(int(dens * n), most)
    rows = rng.permutation(n)[:k]
    if j == 0:
        v = rng.lognormal(0.0, 1.0, size=k)
    elif j in (1, 11):
        v = 0.01 + rng.rand(k)
    elif j == 2:
        v = rng.randint(1, 4, size=k) * 0.25
    elif j == 4:   # (on a grid of 2^-10: a group's sum is exact in any order, however much of it cancels -- the fold change is held to 1e-12)
        v = np.round(rng.randn(k) * 1024.0) / 1024.0
        v[v == 0] = 1.0 / 1024.0
    elif j == ONE_VALUE:
        v = np.full(k, 4.0)
    elif j == 7:
        v = 200.0 + rng.poisson(60.0, size=k)
    elif j == 8:
        v = rng.exponential(1.0, size=k)
    elif j == 9:
        v = rng.randint(-3, 4, size=k) * 0.25
    else:
        v = 1.0 + rng.poisson(20.0, size=k)
    col = np.zeros(n)
    col[rows] = v
    return col


def _scaled(n):
    """SIZES scaled to n cells (the last group takes the rounding)."""
    s = [max(2, int(x * n / sum(SIZES))) for x in SIZES]
    s[0] += n - sum(s)
    return s


def _labels(codes):
    return np.array([f"g{c:05d}" for c in codes])


def _finish(name, form, codes, cols, opts, info):
    edge, _, side = split(name)
    if form == "8i":
        X = np.zeros((codes.size, N_GENES), dtype=np.int64)
        for j, col in enumerate(cols):
            nz = col != 0
            if j == B or np.all(col == np.floor(col)):
                X[:, j] = col.astype(np.int64)
            else:
                X[nz, j] = int_of(col[nz])
    else:
        X = np.ascontiguousarray(np.stack(cols, axis=1).astype(np.float32 if form == "4" else np.float64))
    return Case(name, edge, form, side, _labels(codes), X, opts, info)


def _place(rng, codes, d, extra=()):
    """Cells and key offsets of a boundary gene: the smallest and the largest key in the first two cells of group 0 -- positions 0 and 1
    of the plain and of the padded rows, the first two keys of block 0 in the packed rows: sampled in every layout -- the others dealt
    over the remaining cells; `extra`: keys added on a side, in the cells that come next."""
    d = np.asarray(d, dtype=np.int64)
    anchors = np.flatnonzero(codes == 0)[:2]
    others = rng.permutation(np.setdiff1d(np.arange(codes.size), anchors))
    lo, hi = int(np.argmin(d)), int(np.argmax(d))
    assert lo != hi and np.all(np.asarray(extra) > d[lo]) and np.all(np.asarray(extra) <= d[hi])
    rest = rng.permutation(np.delete(d, [lo, hi]))
    cells = np.concatenate([anchors, others[:rest.size + len(extra)]])
    return cells, np.concatenate([[d[lo], d[hi]], rest, np.asarray(extra, dtype=np.int64)])


CELLS = {"B-own": 40000, "C": 261000, "D": 261120, "E": 72000, "F": 40000, "F-neg": 40000, "Fp": 40000, "Fp-neg": 40000, "G": 40000}   # others: 6000


def _capacity_d(edge, side, K):
    """(key offsets of the lo side, keys added on this side, log2 of the distinct keys a bucket holds, sign) of a capacity edge."""
    hi = side != "lo"
    back = np.concatenate([grid(10 + 7 * i, 20) for i in range(40)])                     # 800 keys, 20 to a bucket
    ends = np.concatenate([grid(0, 1), grid(TOP, 1)])
    if edge in ("A", "D"):   # the fullest bucket: 256 / 257 distinct keys (D: the lo side of A in 261 120 / 261 121 cells)
        return np.concatenate([ends, back, grid(4000, 256)]), grid(4000, 257)[256:] if hi and edge == "A" else (), 10, 1
    if edge == "B":      # a bucket of two values: 512 / 513 keys
        return np.concatenate([ends, back, grid(4000, 512, values=2)]), grid(4000, 1) if hi else (), 10, 1
    if edge == "B-first":   # ... which is the gene's first bucket: id 0 stays empty once it is big
        return np.concatenate([grid(TOP, 1), back, grid(0, 512, values=2)]), grid(0, 2)[1:] if hi else (), 10, 1
    if edge == "B-adj":  # ... next to a big bucket: the id between the two stays empty
        return np.concatenate([ends, back, grid(4000, 513, values=2), grid(4001, 512, values=2)]), grid(4001, 1) if hi else (), 10, 1
    if edge == "B-own":
        # the route's own cap: the first bucket holds K / 2 keys of two values, 26 buckets of 300 keys follow -- two parts of at most cap
        # keys.  (Were the bucket's id to take the + 1 at K / 2 keys already, it would share a part with what follows: more than K keys.)
        d = np.concatenate([grid(0, K // 2, values=2)] + [grid(100 + 100 * i, 300) for i in range(26)] + [grid(TOP, 1)])
        return d, grid(0, 2)[1:] if hi else (), 10, 1
    if edge == "C":      # 8168 buckets of 31 keys: mx = 31, quota = 993; 255 x 993 keys / one more
        d = np.concatenate([grid(b, 31) for b in range(8168)] + [grid(8168, 6), grid(8168, 1024)[-1:]])
        assert d.size == 255 * 993
        return d, grid(8168, 7)[6:] if hi else (), 10, 1
    if edge == "E":
        # one-value buckets of 513 keys: the 127 behind the first give ids 2 i + 2 while the first holds 512 keys (top id 254) and
        # 2 i + 3 once it holds 513 (top id 255); hi2: a 129th big bucket.  The largest key is the last big bucket's value.
        d = np.concatenate([grid(0, 1), grid(40, 512, values=1)] + [grid(100 + 60 * i, 513, values=1) for i in range(127)])
        extra = np.concatenate([grid(40, 1), grid(70, 513 if side == "hi2" else 0, values=1)]) if hi else ()
        return d, extra, 10, 1
    if edge in ("F", "F-neg"):       # a bucket of K keys of one value / K + 1
        return np.concatenate([ends, back, grid(4000, K, values=1)]), grid(4000, 1) if hi else (), 10, -1 if edge == "F-neg" else 1
    if edge in ("Fp", "Fp-neg"):     # ... of two neighbouring values
        return np.concatenate([ends, back, grid(4000, K, values=2)]), grid(4000, 1) if hi else (), 10, -1 if edge == "Fp-neg" else 1
    if edge == "G":
        # the route's own cap: quota - 1 keys in buckets of 100, then a bucket of cap / 4 distinct keys (a bucket of the 2^12 grid holds
        # 4096): mx * 4 == cap keeps the quota plan, part 0 holds cap - 1 keys
        cap, m = K, (K - K // 4 - 2) // 100
        small = np.concatenate([grid(0, 1, 12)] + [grid(1 + b, 100, 12) for b in range(m)] + [grid(3000, cap - cap // 4 - 2 - 100 * m, 12)])
        assert small.size == cap - cap // 4 - 1
        return np.concatenate([small, grid(4000, cap // 4, 12), grid(TOP, 1, 12)]), (), 12, 1
    if edge == "T":
        # quota plan (mx = 256, quota = 768), 668 / 669 keys below the LAST bucket (8191), which holds 100: on the hi side key n - 1 lies
        # in part 1 while the last bucket starts in part 0 and no bucket follows it -- part 1 is a part that no bucket starts, empty
        d = np.concatenate([grid(0, 1), back[:411], grid(4000, 256), grid(OVRP_NB - 1, 100)])
        assert d.size == 668 + 100
        return d, grid(3999, 1) if hi else (), 10, 1
    raise AssertionError(edge)


def _make_capacity(name, edge, form, side):
    spec = EDGES[edge]
    ks = 4 if form == "4" else 8
    rng = np.random.RandomState(_seed(f"{edge}-{form}"))
    n = CELLS.get(edge, 6000)
    sizes = _scaled(n)
    codes = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(codes)
    K = sizing(len(sizes), ks, n, max(sizes), spec.parts_cap).K
    d, extra, sh, sign = _capacity_d(edge, side, K)
    cols = [_ordinary(rng, j, n) for j in range(N_GENES)]
    cells, dv = _place(rng, codes, d, extra)
    col = np.zeros(n, dtype=np.int64 if form == "8i" else np.float64)
    col[cells] = values_of(dv, form, sh, sign)
    cols[B] = col
    if edge == "D" and side == "hi":   # one more cell: a row of zeros but for gene 11, in the last group
        codes = np.append(codes, len(sizes) - 1)
        cols = [np.append(c, 0.37 if j == 11 else 0) for j, c in enumerate(cols)]
    opts = {"ovr_parts_cap": spec.parts_cap} if spec.parts_cap else {}
    return _finish(name, form, codes, cols, opts, {"d": dv, "sh": sh, "sign": sign, "K": K, "cells": cells})


def _distinct(rng, n):
    """n distinct key offsets, 0 and TOP << 10 among them."""
    d = np.unique(rng.randint(1, TOP << 10, size=2 * n + 16))
    return np.concatenate([[0, TOP << 10], rng.permutation(d[d < TOP << 10])[:n - 2]])


def sampled_everywhere(codes, nz):
    """The non-zero cells whose keys every layout samples, with and without the COOP form."""
    maps = position_maps(codes)
    m = nz.copy()
    for layout in LAYOUTS:
        for coop in (True, False):
            m &= sampled(maps, nz, layout, coop)
    return m


def _extremes_sampled(codes, cells, dv):
    """Swap the smallest and the largest key into two cells that every layout samples."""
    nz = np.zeros(codes.size, dtype=bool)
    nz[cells] = True
    ok = np.flatnonzero(sampled_everywhere(codes, nz)[cells])
    assert ok.size >= 2
    dv = dv.copy()
    for at, want in ((ok[0], int(np.argmin(dv))), (ok[1], int(np.argmax(dv)))):
        dv[[at, want]] = dv[[want, at]]
    return dv


H_SIZES = (1100,) * 26   # 26 blocks, none long: blocks 0, 8, 16 and 24 are sampled
H_KEYS, H_ENDS, H_SAMPLED = 3000, 600, 150
I_SIZES = {"lo": [16] * 640, "hi": [15] * 690, "65": ([15] * 64 + [70]) * 10}
J_SIZES = {"lo": [1] * 63 + [4033] + [300] * 8, "hi": [1] * 63 + [4034] + [300] * 8, "65": [1] * 64 + [4033] + [300] * 8}
K_L, K_M, K_S, K_REST = [100, 500, 10, 10, 10, 4200], [100, 500] + [6] * 63 + [100], [100, 500, 10, 10, 10, 600], [300] * 8
K_SIZES = K_L + K_M + K_S + K_REST


def k_nnz(side):
    """Edge K: the boundary gene's non-zeros per group.  Three blocks carry the ends -- a long one (6 groups, 4830 rows: COOP), one of 66
    groups (the group ends read from memory) and a short one (the ends in lanes) -- sides 63 / 64 / 65: the first group ends at that
    offset of its block, the second at 511 / 512 / 513, the long block holds 4095 / 4096 / 4097 keys."""
    dl = {"63": -1, "65": 1}.get(side, 0)
    L, M, S = [64 + dl, 448, 5, 5, 5, 3569], [64 + dl, 448] + [3] * 63 + [50], [64 + dl, 448, 5, 5, 5, 300]
    if side == "empty-first":
        L[0] = M[0] = S[0] = 0
    elif side == "empty-mid":
        L[3] = S[3] = M[30] = 0
    elif side == "empty-last":   # (few keys elsewhere too: the p-value of a group of 4200 cells without a key stays above zero)
        return [6, 45, 5, 5, 5, 0] + [6, 45] + [1] * 63 + [0] + [6, 45, 5, 5, 5, 0] + [15] * 8
    elif side == "empty-two":
        L[2] = L[3] = S[2] = S[3] = M[30] = M[31] = 0
    elif side == "sparse":   # a nearly empty gene: three keys in the long block -- most wavefronts' first unit lies beyond them
        return [2, 0, 0, 0, 0, 1] + [6, 45] + [1] * 63 + [5] + [6, 45, 5, 5, 5, 30] + [15] * 8
    return L + M + S + [150] * 8


def _make_layout(name, edge, form, side):
    """Edges H to K: the group structure, or where the keys lie in it, is the edge; the boundary gene holds distinct values."""
    rng = np.random.RandomState(_seed(f"{edge}-{form}"))
    sizes = {"H": H_SIZES, "I": I_SIZES.get(side), "J": J_SIZES["lo"], "K": K_SIZES}[edge]
    codes = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(codes)
    n = codes.size
    cols = [_ordinary(rng, j, n) for j in range(N_GENES)]
    ks = 4 if form == "4" else 8
    K = sizing(len(sizes), ks, n, max(sizes), 1024).K
    if edge == "H":
        maps = position_maps(codes)
        assert not maps.blocks.is_long.any()
        by = [(maps.plain // OVRP_NT) % 8 == 0, (maps.padded // OVRP_NT) % 8 == 0, maps.block_of % 8 == 0]
        s_pool = np.flatnonzero(codes == 0)[:H_SAMPLED]   # positions 0 .. 149 of the plain and of the padded rows, the first keys of block 0
        assert all(b[s_pool].all() for b in by)
        u_pool = rng.permutation(np.flatnonzero(~(by[0] | by[1] | by[2])))
        d = np.sort(_distinct(rng, K + 1 if side == "hi-none-big" else H_KEYS))
        ends, tails, mid = d[[0, -1]], np.concatenate([d[1:H_ENDS], d[-H_ENDS:-1]]), rng.permutation(d[H_ENDS:-H_ENDS])
        cells = np.concatenate([s_pool, u_pool[:d.size - H_SAMPLED]])
        if side == "lo":          # the smallest and the largest key where every layout samples
            dv = np.concatenate([ends, mid[:H_SAMPLED - 2], tails, mid[H_SAMPLED - 2:]])
        elif side == "hi-out":    # the 600 smallest and the 600 largest keys where no layout samples: they fall into the first / last
            dv = np.concatenate([mid[:H_SAMPLED], ends, tails, mid[H_SAMPLED:]])   # bucket of the range of the others
        elif side == "hi-one":    # every sampled cell holds the median key
            dv = np.concatenate([np.full(H_SAMPLED, np.sort(mid)[mid.size // 2]), ends, tails, mid[:d.size - H_SAMPLED - 2 * H_ENDS]])
        else:                     # no sampled cell holds a key
            cells, dv = u_pool[:d.size], rng.permutation(d)
        assert cells.size == dv.size == np.unique(cells).size
    elif edge == "K":
        members = [rng.permutation(np.flatnonzero(codes == g)) for g in range(len(sizes))]
        cells = np.concatenate([m[:k] for m, k in zip(members, k_nnz(side))])
        dv = _extremes_sampled(codes, cells, _distinct(rng, cells.size))
    else:
        cells = rng.permutation(n)[:n // 2]
        dv = _extremes_sampled(codes, cells, _distinct(rng, cells.size))
    col = np.zeros(n, dtype=np.int64 if form == "8i" else np.float64)
    col[cells] = values_of(dv, form)
    cols[B] = col
    if edge == "J" and side != "lo":
        # the lo side and one more cell, which holds a key of its own in the boundary gene: hi -- in the large group (4034 cells: the
        # block has 4097 rows); 65 -- a one-cell group in front of it (65 groups in the block)
        codes = np.append(np.where(codes >= 63, codes + 1, codes), 63) if side == "65" else np.append(codes, 63)
        more = next(x for x in range((TOP << 10) - 1, 0, -1) if x not in set(dv.tolist()))
        cols = [np.append(c, values_of([more], form)[0] if j == B else 0) for j, c in enumerate(cols)]
        cells, dv = np.append(cells, n), np.append(dv, more)
    return _finish(name, form, codes, cols, {"ovr_parts_cap": 1024}, {"d": dv, "sh": 10, "sign": 1, "K": K, "cells": cells})


@functools.lru_cache(maxsize=6)
def make(name):
    edge, form, side = split(name)
    return (_make_layout if edge in ("H", "I", "J", "K") else _make_capacity)(name, edge, form, side)


def groups(labels):
    return oracle.encode_and_count_groups(labels, None)[1]


