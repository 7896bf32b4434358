"""Inputs that sit on the switch points the PER-GENE sparse kernels decide on the device: the stored entries of one
gene, the stored entries of one group in one gene (a run), and how a gene's values crowd into value buckets.

tests/threshold_cases.py covers what the drivers derive from the group sizes; here one BOUNDARY GENE (column B of 12) carries the edge and
the other genes are ordinary.  The entries that make up the quantity under test hold one value wherever the route allows it, so that a
tie block, a bucket counter or a run reaches the capacity itself.  Every edge exists with four-byte keys (float32) and with eight-byte
keys (float64, with values float32 cannot hold: device-resident float64 that is float32 throughout is narrowed to the float32 kernels;
and int64, which nothing narrows);
the capacities halve with the key size, so the edge values are computed per width from the host sizing functions restated below --
tests/test_gpu_gene_edges.py proves each restatement against the real build (test_an_edge_is_an_edge).

A case is its name, "<edge>-<4|8|8i>-<lo|hi>": lo is the last value on the old side of the switch, hi the first on the new side, and the two
differ in one stored entry.  Imports numpy and the oracle only.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import oracle

REF_LABEL = "g00000"
N_GENES = 12
B = 5                    # the boundary gene: not gene 0, so that a column window starting after gene 0 still holds it
EMPTY, ONE_VALUE = 3, 6  # ordinary genes: no stored entry at all / one value wherever stored
MAX_SHARE = 0.15

# ---------------------------------------------------------------------------------------------------------------------------------------
# The host sizing functions, restated (one function each).  kMaxLds: illico_amd/csrc/engine.h
# ---------------------------------------------------------------------------------------------------------------------------------------
MAX_LDS = 160 * 1024
CSCO_CHUNK = 1024        # kernels_ovr_rank.h: 64 * CSCO_K, the sort chunk of the sorted form
CSCO_MAX_BUCKET = 192
CSCO_MAX_AVG = 64
CSCG_SMALL, CSCG_MEDIUM = 32, 128   # kernels_csc_gene.h
RUNEND_MAX = 8192        # sparse_driver.h: run_csc_gene_route


def csco_fixed_lds_bytes(G, lg_buckets):
    """kernels_ovr_rank.h: csco_fixed_lds_bytes"""
    return ((G + 1) & ~1) * 8 + (2 << lg_buckets) + 256


def csco_key_cap(G, lg_buckets, key_size, accg=False):
    """kernels_ovr_rank.h: csco_key_cap (lds_max = kMaxLds)"""
    fixed = csco_fixed_lds_bytes(0 if accg else G, lg_buckets)
    if fixed + 1024 * 4 + 64 > MAX_LDS:
        return 0
    return min((MAX_LDS - fixed) // key_size - 4, 65535 - 4)


OvrPlan = namedtuple("OvrPlan", ["lg", "key_cap", "accg", "g_lds"])


def csc_ovr_plan(G, key_size, max_nnz, small_lds=True):
    """sparse_driver.h: run_csc_ovr_route -- bucket count, key slots and where the accumulators live, from the longest column of the call.
    small_lds = False: the option no_csc_ovr_small_lds."""
    lg = 14
    if csco_key_cap(G, lg, key_size) < max_nnz:
        lg = 13
    key_cap = csco_key_cap(G, lg, key_size)
    accg, g_lds = False, G
    if key_cap < max_nnz:
        lg2 = 14
        if csco_key_cap(G, lg2, key_size, True) < max_nnz:
            lg2 = 13
        cap2 = csco_key_cap(G, lg2, key_size, True)
        if cap2 > key_cap:
            accg, lg = True, lg2
            need = csco_fixed_lds_bytes(0, lg) + (min(max_nnz, cap2) + 8) * key_size
            g_lds = min(G, ((MAX_LDS - need) // 8) & ~1) if need < MAX_LDS else 0
            key_cap = min((MAX_LDS - csco_fixed_lds_bytes(g_lds, lg)) // key_size - 4, 65535 - 4)
    if not accg and small_lds and max_nnz + 64 < key_cap:
        lg_s = lg
        while lg_s > 11 and (1 << (lg_s - 1)) >= 2 * max_nnz:
            lg_s -= 1
        cap_s = min(csco_key_cap(G, lg_s, key_size), max((max_nnz + 64 + 1023) & ~1023, 2048))
        if cap_s >= max_nnz:
            lg, key_cap = lg_s, cap_s
    return OvrPlan(lg, key_cap, accg, g_lds)


def csc_ovr_takes(plan, ns, sorted_form):
    """kernels_csc_ovr.h: k_csc_ovr_gene keeps a gene of ns stored entries (k1 - k0 > P.key_cap; sorted form, ovr_rank_sorted in kernels_ovr_rank.h: ncap > key_cap)."""
    if ns > plan.key_cap:
        return False
    return not sorted_form or -(-ns // CSCO_CHUNK) * CSCO_CHUNK <= plan.key_cap


def ovo_runend_bytes(ref_cap, buckets):
    """kernels_ovo.h: ovo_runend_bytes"""
    b = (ref_cap * 2 + 15) & ~15
    t = 2 << 13
    return t if buckets and b < t else b


def cscg_lds_bytes(G, key_cap, runend_cap, key_size, buckets=False):
    """kernels_csc_gene.h: cscg_lds_bytes"""
    return ((G + 1 + 3) & ~3) * 4 + 1024 * 4 + ovo_runend_bytes(runend_cap, buckets) + 256 + key_cap * key_size


GenePlan = namedtuple("GenePlan", ["launched", "key_cap", "runend_cap", "ref_buckets", "cap0"])


def csc_gene_plan(G, key_size, n_ref, gene_nnz, ref_buckets_allowed=True):
    """sparse_driver.h: run_csc_gene_route -- key_cap / runend_cap of k_csc_gene, and whether the launch happens at all (a quarter of the
    genes must fit)."""
    runend_cap = max(1, min(n_ref, RUNEND_MAX))
    fixed0 = cscg_lds_bytes(G, 0, runend_cap, key_size, False)
    cap0 = (MAX_LDS - fixed0) // key_size if fixed0 < MAX_LDS else 0
    fit = sum(1 for x in gene_nnz if x <= cap0)
    launched = fit * 4 >= len(gene_nnz)
    ref_buckets = ref_buckets_allowed and cscg_lds_bytes(G, 0, runend_cap, key_size, True) + 16384 * key_size <= MAX_LDS
    fixed = cscg_lds_bytes(G, 0, runend_cap, key_size, ref_buckets)
    if fixed + 1024 * key_size > MAX_LDS:
        launched = False
    return GenePlan(launched, (MAX_LDS - fixed) // key_size, runend_cap, ref_buckets, cap0)


def csc_gene_takes(plan, total, longest_run, ref_run):
    """kernels_csc_gene.h: k_csc_gene keeps a gene (total > P.key_cap || maxg > CSCG_MEDIUM || nA > P.runend_cap leave)."""
    return total <= plan.key_cap and longest_run <= CSCG_MEDIUM and ref_run <= plan.runend_cap


def keys_of(values, key_size):
    """common.h: key_of for positive values -- the IEEE bits, or the integer itself (int64), with the sign bit set: order-preserving
    unsigned keys."""
    if np.asarray(values).dtype.kind == "i":
        assert key_size == 8 and np.all(np.asarray(values) > 0)
        return np.ascontiguousarray(values, dtype=np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    v = np.ascontiguousarray(values, dtype=np.float32 if key_size == 4 else np.float64)
    assert np.all(v > 0)
    return v.view(np.uint32).astype(np.uint64) ^ np.uint64(1 << 31) if key_size == 4 else v.view(np.uint64) ^ np.uint64(1 << 63)


def bucket_occupancy(values, key_size, lg_buckets):
    """kernels_ovr_rank.h, ovr_rank_run up to its count pass (ovr_sampled_range, OvrBuckets, ovr_count_keys): the bucket counters of a
    column whose stored non-zeros are `values`, in stored order.
    The key range comes from every eighth row of 1024 entries when the column holds more than 8192; shift = key bits of the range minus
    lg_buckets; the last two buckets are one."""
    keys = keys_of(values, key_size)
    step = 8 if keys.size > 8192 else 1
    sampled = keys[(np.arange(keys.size) // 1024) % step == 0]
    kmin, kmax = sampled.min(), sampled.max()
    shift = np.uint64(max(0, int(kmax - kmin).bit_length() - lg_buckets))
    last = np.uint64((1 << lg_buckets) - 2)
    b = np.where(keys > kmin, np.minimum((np.maximum(keys, kmin) - kmin) >> shift, last), np.uint64(0))
    return np.bincount(b.astype(np.int64), minlength=1 << lg_buckets)


def crowded(occ):
    """k_csc_ovr_gene step 2: which of the two crowding rules send the column to the sorted form (largest bucket, sum of squares)."""
    occ = np.asarray(occ, dtype=np.int64)
    return int(occ.max()) > CSCO_MAX_BUCKET, int((occ * occ).sum()) > CSCO_MAX_AVG * int(occ.sum())


CSCR_CACHE = 40          # kernels_csc_gene.h: entries per thread that k_csc_regroup keeps in registers


def regroup_key_cap(G, key_size):
    """sparse_driver.h: regroup_csc_batch -- the longest column k_csc_regroup stages in LDS (longer ones: k_csc_segment)"""
    fixed = ((G + 1 + 3) & ~3) * 4 + 1024 * 4
    return min((MAX_LDS - fixed) // key_size, 1024 * CSCR_CACHE) if fixed + 4096 < MAX_LDS else 0


def long_column(key_size, ovo_packed):
    """sparse_driver.h: long_column -- average stored entries per column above which a sparse window is written out dense.
    ovo_packed: an OVO call whose groups the packed rank kernel takes (sparse_packed_rank_fits(c, true))."""
    return 32768.0 if key_size == 8 and ovo_packed else 32768.0 * 4.0 / key_size


def written_out_dense(fmt, nnz, n_rows, n_cols, key_size, ovo_packed):
    """route_csr_dense_window (the whole matrix: its density times the rows) / route_csc_dense_window (the window: nnz / W), the same
    IEEE operations; OVR's 4 % density gate cannot bind below 800 000 cells at these column lengths."""
    L = long_column(key_size, ovo_packed)
    return (nnz / (float(n_rows) * float(n_cols))) * float(n_rows) > L if fmt == "csr" else nnz / float(n_cols) > L


def srt_cap(key_size):
    """kernels_ovo_compact.h: srt_cap -- the longest run k_bucket_big_runs deals in LDS"""
    return 32768 if key_size == 4 else 16384


OVO_REF_MAX_BUCKET = 48   # kernels_ovo.h
OVO_REF_BUCKETS_LG = 13


def ref_bucket_occupancy(values, key_size):
    """kernels_csc_gene.h, k_csc_gene step 4a (refbk_bucket, kernels_ovo.h): the bucket counters of a reference run -- the range is that of
    the whole run, shift = key bits of the range minus 13, the last bucket takes what lies beyond."""
    keys = keys_of(values, key_size)
    kmin, kmax = keys.min(), keys.max()
    shift = np.uint64(max(0, int(kmax - kmin).bit_length() - OVO_REF_BUCKETS_LG) if kmax != kmin else 0)
    last = (1 << OVO_REF_BUCKETS_LG) - 1
    return np.bincount(np.minimum((keys - kmin) >> shift, np.uint64(last)).astype(np.int64), minlength=last + 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases
# ---------------------------------------------------------------------------------------------------------------------------------------
OVR_SIZES = (20000, 9000, 5000, 3000, 1700, 900, 300, 90, 10)                   # 40 000 cells, 9 groups
OVO_SIZES = (RUNEND_MAX, 256, 255) + tuple(130 + (7 * i) % 90 for i in range(298))   # a reference of 8192 cells, 300 groups of at most 256
OVO_FEW = OVO_SIZES[:61]   # ... 60 of them, where the edge is a run: the gene's total then stays below the eight-byte key slots
G_OVR = len(OVR_SIZES)
SLOTS = 8190             # boundary values sit on the grid 1 + s / 8192, s = 0 .. 8190: bucket s of 8192, bucket 2 s of 16384
TIE = 1.5                # the one value of a saturated run / column

Case = namedtuple("Case", ["name", "edge", "width", "side", "test", "labels", "X", "info", "form"])
# info: "values" (OVR: the boundary gene's stored values in CSC order), "strict_rows" (the groups whose p in the boundary gene must be
# neither 0 nor 1; None: every compared group)
# edge -> (test, what the profile must show on the hi side and not on the lo side per input kind ("csc", "csr"), options that pin the
#          plan, option whose result must equal the default's bit for bit)
Edge = namedtuple("Edge", ["test", "appear", "pin", "bit_equal", "kind"], defaults=("gene",))
LEAVES_OVR = {"csc": ("k_ovr_gene",), "csr": ("k_ovr_gene",)}
# (CSR input: the device transposition is timed on both sides -- its counting pass under k_sparse_seg, pass 2 under k_csr_tile_gather)
LEAVES_OVO = {"csc": ("k_sparse_seg", "k_ovo_rank"), "csr": ("k_ovo_rank",)}
PIN = {"no_csc_ovr_small_lds": 1}
EDGES = {
    # column length, OVR (k_csc_ovr_gene; plan of run_csc_ovr_route)
    "ovr-leave": Edge("ovr", LEAVES_OVR, {}, None),              # 1: ns <= key_cap / > at the largest plan (accumulators in HBM)
    "ovr-sorted14": Edge("ovr", LEAVES_OVR, {}, None),           # 2: ncap <= key_cap / > with 2^14 buckets, the column one value
    "ovr-sorted13": Edge("ovr", LEAVES_OVR, {}, None),           # 2: ... with 2^13 buckets
    "ovr-lg": Edge("ovr", None, {}, None),                       # 3: 2^14 -> 2^13 buckets
    "ovr-accg": Edge("ovr", None, {}, None),                     # 3: accumulators in LDS -> the last groups' in HBM (g_lds < G)
    "ovr-short": Edge("ovr", None, {}, "no_csc_ovr_small_lds"),  # 3: short-column form on / off
    "ovr-step1024": Edge("ovr", None, {}, "no_csc_ovr_small_lds"),
    "ovr-step2048": Edge("ovr", None, {}, "no_csc_ovr_small_lds"),
    "ovr-step4096": Edge("ovr", None, {}, "no_csc_ovr_small_lds"),
    "ovr-accg-split": Edge("ovr", None, {}, None),               # 3: 4000 groups, the accumulators of the first g_lds in LDS, two fewer on hi
    # 5: k_csc_regroup -> k_csc_segment in the two-kernel route (forced), the column one value
    "regroup-ovr": Edge("ovr", None, {"no_csc_ovr_gene_path": 1}, None),
    "regroup-ovo": Edge("ovo", None, {"no_csc_gene_path": 1}, None),
    # 6: the window written out dense: W x L stored entries / W x L + 1 (all 12 genes: the same total for the CSR and the CSC rule)
    "long-ovr": Edge("ovr", {"csc": ("k_densify",), "csr": ("k_densify",)}, {}, None, "window"),
    "long-ovo": Edge("ovo", {"csc": ("k_densify",), "csr": ("k_densify",)}, {}, None, "window"),
    # crowding, OVR (bucket form -> sorted form)
    "crowd-bucket": Edge("ovr", None, PIN, "csc_ovr_sorted_form"),      # 10: largest bucket 192 / 193
    "crowd-avg": Edge("ovr", None, PIN, "csc_ovr_sorted_form"),         # 10: sum of squares 64 n / 64 n + 2
    # 10: the same on a column of key_cap entries -- the longest the bucket form ever sees; rounded up to a sort chunk it is beyond the
    # key slots of the sorted form, so the crowded side leaves the kernel
    "crowd-bucket-cap": Edge("ovr", LEAVES_OVR, PIN, "csc_ovr_sorted_form"),
    "crowd-avg-cap": Edge("ovr", LEAVES_OVR, PIN, "csc_ovr_sorted_form"),
    # run length and column length, OVO (k_csc_gene; plan of run_csc_gene_route)
    "run-small": Edge("ovo", None, {}, None),                           # 7: longest run 32 / 33
    "run-medium": Edge("ovo", LEAVES_OVO, {}, None),                    # 7: 128 / 129
    "ref-run": Edge("ovo", LEAVES_OVO, {}, "no_ovo_ref_buckets"),       # 8: a fully stored reference of 8192 / 8193 cells
    "ref-bucket": Edge("ovo", None, {}, "no_ovo_ref_buckets"),          # 8: largest bucket of the reference's bucket form 48 / 49 keys
    "ovo-total": Edge("ovo", LEAVES_OVO, {}, None),                     # 4: total <= key_cap / >
    "ovo-quarter": Edge("ovo", None, {}, None),                         # 4: 3 of 12 genes fit / 2 of 12: k_csc_gene present / absent
    # run length in the packed rank route (keyed_driver.h: launch_bucket_big_runs): a whole ranked group at one value, as the
    # ranked-* cases of tests/threshold_cases.py, at the group sizes that suite passes over
    "run-256": Edge("ovo", None, {}, None, "ranked"),                   # 9: 64 * OCR_KMAX keys: dealt by k_bucket_big_runs from 257 on
    "run-8192": Edge("ovo", None, {}, "no_big_runs_wide", "ranked"),    # 9: the 256-thread launch / a 1024-thread launch of its own; OCR_COOP_MIN
    "run-srt": Edge("ovo", None, {}, "no_big_runs_global", "ranked"),   # 9: srt_cap keys in LDS / through the second key buffer in HBM
}
WIDTHS = (4, 8)
# the forms of a case: float32, float64, and int64 -- eight-byte keys through key_of(int64_t), never narrowed to the float32 kernels
FORMS = ("4", "8", "8i")
SIDES = ("lo", "hi")
NAMES = tuple(f"{e}-{f}-{s}" for e in EDGES for f in FORMS for s in SIDES)
# a draw that breaks the share rule of tests/test_gene_edge_cases_host.py takes its next draw: "<edge>-<width>" -> number of redraws
REDRAW = {}


def sorted_edge(G, key_size, lg):
    """The longest one-value column the sorted form keeps at that bucket count: key_cap rounded down to a sort chunk."""
    return csco_key_cap(G, lg, key_size) // CSCO_CHUNK * CSCO_CHUNK


def leave_edge(G, key_size):
    """The longest column k_csc_ovr_gene keeps at all: the key slots of the plan with every accumulator in HBM."""
    ns = csco_key_cap(G, 13, key_size, True)
    assert csc_ovr_takes(csc_ovr_plan(G, key_size, ns), ns, False) and not csc_ovr_takes(csc_ovr_plan(G, key_size, ns + 1), ns + 1, False)
    return ns


def _blocks(ns, size):
    return [size] * (ns // size) + ([ns % size] if ns % size else [])


@functools.lru_cache(maxsize=None)
def _avg_edge_blocks(ns):
    """Block sizes with sum ns whose sum of squares is at most 64 ns and exceeds it once one entry moves from the first block to the
    second: blocks of 64 and three others a < 64 < b, c.  (ns = 40 mod 64 has no choice of a few blocks with equality: every size
    would have to be a multiple of 8.)  The choice with the smallest slack, then the smallest sizes."""
    f = lambda x: x * (x - 64)
    best = None
    for a in range(2, 64):
        for b in range(65, CSCO_MAX_BUCKET - 1):
            for c in range(1, CSCO_MAX_BUCKET):
                rest = ns - a - b - c
                slack = -(f(a) + f(b) + f(c))
                if rest >= 64 and rest % 64 == 0 and 0 <= slack < 2 * (b - a) + 2 and (best is None or slack < best[0]):
                    best = (slack, [a, b, c] + [64] * (rest // 64))
    assert best, ns
    return tuple(best[1])


def _slots(nb):
    """nb distinct grid slots from 0 to SLOTS, at least two apart."""
    assert 2 <= nb <= SLOTS // 2
    stride = SLOTS // (nb - 1)
    return [i * stride for i in range(nb - 1)] + [SLOTS]


ACCG_SPLIT_STORED = {4: 30000, 8: 15000}
ACCG_SPLIT_SIZES = (10,) * 4000


def _ovr_column(edge, key_size):
    """(block sizes of the lo side, what the hi side changes): ("add", block) one more entry in that block, ("move", from, to)."""
    G = G_OVR
    if edge == "ovr-accg-split":
        return _blocks(ACCG_SPLIT_STORED[key_size], 64), ("add", -1)
    if edge == "regroup-ovr":
        return [regroup_key_cap(G, key_size)], ("add", 0)
    if edge == "ovr-leave":
        return _blocks(leave_edge(G, key_size), 64), ("add", -1)
    if edge == "ovr-sorted14":
        return [sorted_edge(G, key_size, 14)], ("add", 0)
    if edge == "ovr-sorted13":
        return [sorted_edge(G, key_size, 13)], ("add", 0)
    if edge == "ovr-lg":
        return _blocks(csco_key_cap(G, 14, key_size), 64), ("add", -1)
    if edge == "ovr-accg":
        return _blocks(csco_key_cap(G, 13, key_size), 64), ("add", -1)
    if edge == "ovr-short":
        return _blocks(csco_key_cap(G, 14, key_size) - 65, 64), ("add", -1)
    if edge.startswith("ovr-step"):
        # (blocks of 64 sit on the average rule: one entry more in any of them would send the column to the sorted form)
        return [64] * (int(edge[8:]) // 64 - 1) + [63, 1], ("add", -2)
    cap = csco_key_cap(G, 14, key_size)
    if edge == "crowd-bucket":
        return [CSCO_MAX_BUCKET] + [32] * 100, ("move", 1, 0)
    if edge == "crowd-avg":
        return [64] * 64, ("move", 1, 0)
    if edge == "crowd-bucket-cap":
        return [CSCO_MAX_BUCKET] + _blocks(cap - CSCO_MAX_BUCKET, 32), ("move", 1, 0)
    if edge == "crowd-avg-cap":
        return list(_avg_edge_blocks(cap)), ("move", 0, 1)
    raise AssertionError(edge)


def _ordinary(rng, j, n, most, wide, scale=1.0):
    """Ordinary gene j: at most `most` stored entries.  wide: float64 values that float32 cannot hold in the continuous genes."""
    dens = scale * (0.3, 0.45, 0.5, 0.0, 0.2, 0.0, 0.25, 0.05, 0.4, 0.1, 0.35, 0.02)[j]
    k = min(int(dens * n), most)
    rows = rng.permutation(n)[:k]
    if j in (0, 7, 10):
        v = 1.0 + rng.poisson((3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 20.0)[j], size=k)   # counts
    elif j == 4:
        v = rng.randn(k)                                       # negatives stored explicitly
    elif j == ONE_VALUE:
        v = np.full(k, 4.0)
    elif j == 8:
        v = rng.randint(1, 4, size=k) * 0.25                   # non-integer ties
    else:
        v = 0.01 + rng.rand(k)                                 # continuous
    col = np.zeros(n)
    col[rows] = v if wide else v.astype(np.float32)
    return col


def _seed(text):
    return zlib.crc32(text.encode()) & 0x7FFFFFFF


def int_of(x):
    """An ordinary value as an integer: order and ties kept, never zero (values closer than 2^-20 may fall together)."""
    x = np.asarray(x, dtype=np.float64)
    return (np.sign(x) * (1 + np.floor(np.abs(x) * 2.0 ** 20))).astype(np.int64)


def grid_int_of(x):
    """A boundary value 1 + m / 2^23 (every float32 in [1, 2]) as the integer 1 + m: the same order, the same ties, and the same key
    differences as the float32 keys -- so the same buckets."""
    m = (np.asarray(x, dtype=np.float64) - 1.0) * 2.0 ** 23
    assert np.all((m >= 0) & (m <= 2 ** 23) & (m == np.floor(m)))
    return 1 + m.astype(np.int64)


def tie_of(c):
    """The one value of a saturated run / column in that case's form."""
    return int(grid_int_of(TIE)) if c.form == "8i" else TIE


def make(name):
    """The case of that name.  The int64 form is the float64 recipe on its own draw with every stored value turned into an integer by a
    map that keeps order and ties: the count-valued genes as they are, the boundary gene by grid_int_of, the others by int_of."""
    edge, form, side = name.rsplit("-", 2)
    key_size = int(form[0])
    spec = EDGES[edge]
    draw = f"{edge}-{form}"
    rng = np.random.RandomState(_seed(draw + "+" * REDRAW.get(draw, 0)))
    wide = key_size == 8
    if spec.kind == "ranked":
        c = _make_ranked(name, edge, key_size, side, wide)
    elif spec.kind == "window":
        c = _make_window(name, edge, key_size, side, rng, wide)
    else:
        c = (_make_ovr if spec.test == "ovr" else _make_ovo)(name, edge, key_size, side, rng, wide)
    if form != "8i":
        return c._replace(form=form)
    X = np.zeros(c.X.shape, dtype=np.int64)
    for j in range(N_GENES):
        col = c.X[:, j]
        nz = col != 0
        if j == B and spec.kind != "ranked":
            X[nz, j] = grid_int_of(col[nz])
        elif np.all(col == np.floor(col)):
            X[:, j] = col.astype(np.int64)
        else:
            X[nz, j] = int_of(col[nz])
    return c._replace(X=X, form=form)


def _finish(name, edge, key_size, side, test, codes, cols, info):
    X = np.stack(cols, axis=1).astype(np.float64 if key_size == 8 else np.float32)
    labels = np.array([f"g{c:05d}" for c in codes])
    return Case(name, edge, key_size, side, test, labels, np.ascontiguousarray(X), info, None)


def _make_ovr(name, edge, key_size, side, rng, wide):
    sizes = ACCG_SPLIT_SIZES if edge == "ovr-accg-split" else OVR_SIZES
    codes = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(codes)
    n = codes.size
    blocks, change = _ovr_column(edge, key_size)
    ns = sum(blocks)
    vals = np.repeat(1.0 + np.array(_slots(len(blocks)) if len(blocks) > 1 else [4096]) / 8192.0, blocks)
    block_of = np.repeat(np.arange(len(blocks)), blocks)
    order = rng.permutation(ns)
    vals, block_of = vals[order], block_of[order]
    for pos, want in ((0, 0), (1, len(blocks) - 1)):   # smallest and largest value among the entries the range is sampled from (CSC order)
        at = int(np.flatnonzero(block_of == want)[0 if want else -1])
        vals[[pos, at]], block_of[[pos, at]] = vals[[at, pos]], block_of[[at, pos]]
    perm = rng.permutation(n)
    strict = None
    if edge == "ovr-accg-split":
        # the last group with its accumulator in LDS and the first with it in HBM, on either side (one entry more moves the split down by
        # two groups): every cell of the four stored, at ONE value
        g_lo, g_hi = (csc_ovr_plan(len(sizes), key_size, k).g_lds for k in (ns, ns + 1))
        strict = (g_hi - 1, g_hi, g_lo - 1, g_lo)
        special = np.flatnonzero(np.isin(codes, strict))
        perm = np.concatenate([special, perm[~np.isin(perm, special)]])
    cols = [_ordinary(rng, j, n, ns // 2, wide) for j in range(N_GENES)]
    rows = np.sort(perm[:ns])
    if strict:
        for r in special:   # ... that of block 5
            p, q = int(np.searchsorted(rows, r)), int(np.flatnonzero((block_of == 5) & ~np.isin(rows, special) & (np.arange(ns) > 1))[0])
            if block_of[p] != 5:
                vals[[p, q]], block_of[[p, q]] = vals[[q, p]], block_of[[q, p]]
    if side == "hi" and change[0] == "add":
        blk = change[1] % len(blocks)
        extra = next(r for r in perm[ns:] if r > rows[1])   # (entries 0 and 1 stay the ends of the sampled range)
        at = int(np.searchsorted(rows, extra))
        rows = np.insert(rows, at, extra)
        vals = np.insert(vals, at, vals[block_of == blk][0])
        block_of = np.insert(block_of, at, blk)
    elif side == "hi":
        src, dst = change[1], change[2]
        at = int(np.flatnonzero((block_of == src) & (np.arange(ns) > 1))[0])
        vals[at], block_of[at] = vals[block_of == dst][0], dst
    col = np.zeros(n)
    col[rows] = vals
    cols[B] = col
    return _finish(name, edge, key_size, side, "ovr", codes, cols, {"values": vals, "strict_rows": strict})


def _make_ovo(name, edge, key_size, side, rng, wide):
    sizes = list(OVO_SIZES if edge in ("ovo-total", "ovo-quarter", "regroup-ovo") else OVO_FEW)
    if edge == "ref-run":
        sizes[0] = RUNEND_MAX + 1      # hi; lo drops one reference cell below
    codes = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(codes)
    n = codes.size
    G = len(sizes)
    members = [np.flatnonzero(codes == g) for g in range(G)]
    for m in members:
        rng.shuffle(m)
    col = np.zeros(n)
    cols = [_ordinary(rng, j, n, n, wide, 0.4) for j in range(N_GENES)]   # (at most a fifth stored: no run of 128 in a group of 256)
    strict = (1,)
    if edge in ("run-small", "run-medium"):
        r = (CSCG_SMALL if edge == "run-small" else CSCG_MEDIUM) + (side == "hi")
        col[members[1][:r]] = TIE                                        # the run: one value
        ref = members[0][: int(0.3 * sizes[0])]
        col[ref] = 1.0 + rng.rand(ref.size).astype(np.float32)   # (the boundary gene is the same numbers in both widths)
        for g in range(2, G):
            m = members[g][: 1 + (g * 5) % 16]                           # the other runs: 1 .. 16 entries
            col[m] = 1.0 + rng.rand(m.size).astype(np.float32)
    elif edge == "ref-bucket":
        # the reference run: a tie block of 48 / 49 alone in its bucket, 2000 other values one per bucket, two buckets apart (grid slots
        # 0 .. 8190 -> buckets 0 .. 8190 of 8192)
        tie_n = OVO_REF_MAX_BUCKET + (side == "hi")
        slots = [s for s in range(0, SLOTS + 1, 4) if abs(s - 4096) > 2][:1999] + [SLOTS]
        col[members[0][:OVO_REF_MAX_BUCKET + 1][:tie_n]] = TIE
        col[members[0][OVO_REF_MAX_BUCKET + 1:OVO_REF_MAX_BUCKET + 1 + len(slots)]] = 1.0 + rng.permutation(slots) / 8192.0
        for g in range(1, G):   # the other runs look up the full bucket, its neighbours and values between the reference's
            m = members[g][: 1 + (g * 5) % 16]
            col[m] = 1.0 + rng.choice([4092, 4100, 4094, 4098, 2, 8188] + list(range(1, 8190, 2)), size=m.size) / 8192.0
            if g % 3 == 0:
                col[m[0]] = TIE
    elif edge == "ref-run":
        col[members[0]] = TIE                                            # the reference run: every cell stored, one value
        for g in range(1, G):
            m = members[g][: sizes[g] * 9 // 20]                         # 45 % of each group above the reference, its zeros below
            col[m] = TIE + 0.25 * rng.randint(1, 3, size=m.size)
        strict = None
    else:   # ovo-total / ovo-quarter: the whole gene one value, `total` stored entries in runs of at most 128
        plan = csc_gene_plan(G, key_size, sizes[0], [0] * N_GENES)
        total = {"ovo-total": plan.key_cap, "ovo-quarter": plan.cap0, "regroup-ovo": regroup_key_cap(G, key_size)}[edge]
        longest = sizes[0] if edge == "regroup-ovo" else CSCG_MEDIUM - 1   # (the two-kernel route takes runs of any length)
        share = total / n
        take = [int(share * sizes[0])] + [min(int(share * s), longest) for s in sizes[1:]]
        g = 2
        while sum(take) < total:                                          # top up, group after group, no run beyond 127
            if take[g] < min(sizes[g], longest):
                take[g] += 1
            g = g + 1 if g + 1 < G else 2
        assert sum(take) == total
        if side == "hi":
            take[1] += 1
        for g in range(G):
            col[members[g][: take[g]]] = TIE
        if edge == "ovo-quarter":                                         # nine genes too long for the key slots, two short ones beside B
            for j in (0, 1, 2, 4, 7, 8, 9, 10, 11):
                rows = rng.permutation(n)[: plan.cap0 + 1 + 100 * j]
                cols[j] = np.zeros(n)
                cols[j][rows] = (0.01 + rng.rand(rows.size)) if wide else (0.01 + rng.rand(rows.size)).astype(np.float32)
    cols[B] = col
    if edge == "ref-run" and side == "lo":
        drop = members[0][-1]
        codes = np.delete(codes, drop)
        cols = [np.delete(c, drop) for c in cols]
    return _finish(name, edge, key_size, side, "ovo", codes, cols, {"strict_rows": strict})


def _make_window(name, edge, key_size, side, rng, wide):
    """Every gene holds exactly L = long_column stored entries, the boundary gene one more on the hi side: W x L / W x L + 1 in the
    window of all 12 genes, which is also the whole matrix.  The boundary gene holds one value."""
    test = EDGES[edge].test
    codes = np.repeat(np.arange(G_OVR), OVR_SIZES)
    rng.shuffle(codes)
    n = codes.size
    L = int(long_column(key_size, test == "ovo"))
    cols = []
    for j in range(N_GENES):
        perm = rng.permutation(n)
        k = L + (j == B and side == "hi")
        if j == B:
            v = np.full(k, TIE)
        elif j % 3 == 0:
            v = 1.0 + rng.poisson(3.0, size=k)
        elif j % 3 == 1:
            v = rng.randint(1, 4, size=k) * 0.25
        else:
            v = 0.01 + rng.rand(k)
        col = np.zeros(n)
        col[perm[:k]] = v if wide else v.astype(np.float32)
        cols.append(col)
    return _finish(name, edge, key_size, side, test, codes, cols, {"strict_rows": None})


RANKED_TAIL = (300, 256, 255, 40, 16, 15, 2, 1)
RANKED_CONSTANTS = (1, 9, 62, 255, 2047, 0, -2)
RANKED_STRICT = (0, 1, 3, 4, 7, 8, 10)


def ranked_size(edge, key_size, side):
    return {"run-256": 256, "run-8192": 8192, "run-srt": srt_cap(key_size)}[edge] + (side == "hi")


def _make_ranked(name, edge, key_size, side, wide):
    """The recipe of threshold_cases.make for a ranked group of n cells (a reference of 6000, the same tail of small groups): group 1's
    cells at ONE value in columns 0-7, so that its run in a gene is n keys (column 5: none) in one tie block.  A case is its name: the
    two sides are two draws.  wide: the continuous columns hold float64 values between the float32 ones."""
    n_edge = ranked_size(edge, key_size, side)
    sizes = (6000, n_edge) + RANKED_TAIL
    rng = np.random.RandomState(_seed(name + "+" * REDRAW.get(name, 0)))
    codes = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(codes)
    n = codes.size
    held = codes == 1
    cols = []
    for v in RANKED_CONSTANTS:
        x = (v + rng.randint(-1, 2, size=n)).astype(np.float64)
        x[held] = v
        cols.append(x)
    x = rng.randint(1, 4, size=n) * 0.25
    x[held] = 0.5
    cols.append(x)
    cont = (rng.permutation(n) + 0.5 * rng.rand(n)) / n + 0.01
    cont = cont if wide else cont.astype(np.float32).astype(np.float64)
    cols.append(cont)
    cols.append(np.where(rng.rand(n) < 0.5, 0.0, cont))
    cols.append(rng.poisson(3.0, size=n).astype(np.float64))
    cols.append(np.full(n, 4.0))
    return _finish(name, edge, key_size, side, "ovo", codes, cols, {"strict_rows": (1,), "sizes": sizes})


def groups(labels, test):
    return oracle.encode_and_count_groups(labels, REF_LABEL if test == "ovo" else None)[1]


def gene_stats(c):
    """Per gene of a case: stored entries, longest non-reference run, reference run -- what the per-gene kernels decide on."""
    codes = np.unique(c.labels, return_inverse=True)[1].reshape(-1)
    G = codes.max() + 1
    out = []
    for j in range(c.X.shape[1]):
        runs = np.bincount(codes[c.X[:, j] != 0], minlength=G)
        out.append((int(runs.sum()), int(runs[1:].max()), int(runs[0])))
    return out
