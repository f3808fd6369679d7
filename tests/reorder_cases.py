"""Named cases for the reorder kernels (tests/test_reorder_ref.py, tests/test_gpu_reorder.py) -- TEST INFRASTRUCTURE ONLY.

A case is a size, a bucket distribution, a capacity (which fixes the stride of the counts and offsets arrays) and a
grid (0: the renderer's own).  The sizes are the live counts at which the kernels change shape; REGIMES states, per
size, the rounds per tile R and the tiles, and tests/test_reorder_ref.py asserts it from the restated formulas, so
every case certifies the regime it names.
"""
import numpy as np

import reorder_ref as M

# n: (R, tiles)
REGIMES = {
    0: (1, 0), 1: (1, 1), 63: (1, 1), 64: (1, 1), 65: (1, 1), 255: (1, 1), 256: (1, 1), 257: (1, 2),
    65536: (1, 256),        # one chunk of the scan
    65537: (1, 257),        # two chunks of the scan, with the carry
    524288: (1, 2048),
    524289: (2, 1025),      # the last tile holds one slot
    1048577: (3, 1366),
    2097153: (5, 1639),     # the histogram's second batch of 4 rounds holds one round; the last tile runs 3 of 5 rounds
    3670017: (8, 1793),
    4194305: (9, 1821),
    8392705: (16, 2050),    # more tiles than the product grid of a 256-CU device
}
SMALL_SIZES = [n for n in REGIMES if n <= 65537]
LARGE_SIZES = [n for n in REGIMES if n > 65537]
HUGE = 8392705                                 # run for two distributions only (340 MB of ray state each way)
CPU_LIMIT = 2100000                            # brute against tile walk on the CPU up to here
FULL_CAPACITY = 41472000                       # a 1920 x 1080 x 20 pass: stride 10125, which no case's tiles equal
SMALL_GRIDS = (0, 1, 3)                        # the renderer's, one workgroup for every tile, three
FILL = 0xDEADBEEF                              # what counts, offsets, totals and live_next hold before the launch
SENTINEL = 0xA5A5A5A5                          # what the outputs and their guard words hold before the launch
GUARD = 64                                     # guard slots behind every output

SMALL_DISTRIBUTIONS = ("uniform", "mod64", "mod65", "wave_runs", "all0", "all63", "all64", "no_dead", "compaction",
                       "ascending", "descending", "survivor_first", "survivor_span_end", "survivor_span", "survivor_last")
LARGE_DISTRIBUTIONS = ("uniform", "mod64")


def capacities(n):
    return (n, FULL_CAPACITY)


def buckets(n, name):
    """The bucket bytes (0..64, 64 = dead) of distribution `name` over n slots."""
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(1000003 * len(name) + n)
    if name == "uniform":
        b = rng.integers(0, 65, n)
    elif name == "mod64":              # every wave holds 64 distinct live buckets: every peer set is a singleton
        b = i % 64
    elif name == "mod65":              # the same with the dead bucket, drifting by one slot per wave
        b = i % 65
    elif name == "wave_runs":          # one bucket per wave: every rank comes from the earlier waves' counts
        b = (i // 64) % 65
    elif name in ("all0", "all63", "all64"):
        b = np.full(n, int(name[3:]))
    elif name == "no_dead":
        b = rng.integers(0, 64, n)
    elif name == "compaction":         # sort off: live rays in bucket 0, the reorder only drops the dead
        b = rng.integers(0, 2, n) * 64
    elif name == "ascending":
        b = i * 65 // max(n, 1)
    elif name == "descending":
        b = 64 - i * 65 // max(n, 1)
    elif name.startswith("survivor_"):  # all dead but one ray, on a tile boundary
        span = M.tile_span(n)
        at = {"first": 0, "span_end": span - 1, "span": span, "last": n - 1}[name[9:]]
        b = np.full(n, 64)
        if n:
            b[min(max(at, 0), n - 1)] = 17
    else:
        raise KeyError(name)
    return b.astype(np.uint8)


def payload(n):
    """Ray state whose every 32-bit word names its slot and field: geo (n, 8), tz (n,), rid (n,), uint32."""
    s = np.arange(n, dtype=np.uint32)
    geo = (np.uint32(0x10000000) + s[:, None] * np.uint32(8) + np.arange(8, dtype=np.uint32)[None, :]).astype(np.uint32)
    return geo, np.uint32(0x40000000) + s, np.uint32(0x80000000) + s


def plain_cases():
    """(n, distribution, capacity, grid) of every plain-reorder case."""
    out = []
    for n in SMALL_SIZES:
        for d in SMALL_DISTRIBUTIONS:
            for cap in capacities(n):
                for g in SMALL_GRIDS:
                    out.append((n, d, cap, g))
    for n in LARGE_SIZES:
        for d in LARGE_DISTRIBUTIONS:
            for cap in capacities(n):
                out.append((n, d, cap, 0))
    return out


# ---- pixel tiles with the reorder on: the exchanged bytes of n_global slots and one owner's share of them
GLOBAL_SMALL = (1, 257, 65537)                 # with SMALL_GRIDS
GLOBAL_LARGE = (524289, 2097153, HUGE)         # the product grid: R = 2, 5, 16, the last with more tiles than workgroups
OWNERSHIPS = ("all", "none", "stripes37_0", "stripes37_1", "one")
STRIPE = 37


def exchanged(n, planted_zero=5, planted_high=7):
    """Exchanged bytes g (n,): bucket + 1 in 1..65, with min(n // 3, planted_zero) bytes set to 0 and
    min(n // 3, planted_high) to values in 66..255.  Returns (g, the planted count)."""
    rng = np.random.default_rng(77 + n)
    g = rng.integers(1, 66, n).astype(np.uint8)
    nz, nh = min(n // 3, planted_zero), min(n // 3, planted_high)
    where = rng.permutation(n)[:nz + nh]
    g[where[:nz]] = 0
    g[where[nz:]] = rng.integers(66, 256, nh).astype(np.uint8)
    if nh:
        g[where[nz]] = 255
    if nh > 1:
        g[where[nz + 1]] = 66
    return g, nz + nh


def ownership(n, name):
    """own (n,) uint8: nonzero where this owner holds the global slot."""
    s = np.arange(n, dtype=np.int64)
    if name == "all":
        own = np.ones(n, bool)
    elif name == "none":
        own = np.zeros(n, bool)
    elif name.startswith("stripes37_"):        # every other stripe of 37 slots: what SlotMap(37, 2, index) maps to
        own = (s // STRIPE) % 2 == int(name[-1])
    elif name == "one":
        own = s == (2 * n) // 3
    else:
        raise KeyError(name)
    return (own * np.uint8(3)).astype(np.uint8)


def global_cases():
    """(n_global, ownership, capacity, grid)."""
    out = []
    for n in GLOBAL_SMALL:
        for o in OWNERSHIPS:
            for cap in capacities(n):
                for g in SMALL_GRIDS:
                    out.append((n, o, cap, g))
    for n in GLOBAL_LARGE:
        for o in (("stripes37_1",) if n == HUGE else ("all", "stripes37_0")):
            out.append((n, o, n if n == HUGE else FULL_CAPACITY, 0))
    return out
