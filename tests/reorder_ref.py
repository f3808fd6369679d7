"""The stable 65-bucket reorder of rt_render.hip restated in numpy -- TEST INFRASTRUCTURE ONLY.

The reorder is written twice.  brute() is the definition: a stable argsort of the bucket bytes with the dead rays
(bucket 64) dropped.  tile_walk() follows the kernels' decomposition -- the live prefix cut into tiles of 256 * R
slots, per-tile bucket counts stored bucket-major, an exclusive scan per bucket, the bucket totals, the run bases and
the rank inside a tile -- so that a GPU mismatch can be placed at the histogram, the scan or the scatter.  The two
share no step: brute sorts, tile_walk only counts.
"""
import numpy as np

K_BLOCK = 256            # kBlock
K_TILE_TARGET = 2048     # kTileTarget
K_SORT_ITEMS = 16        # kSortItems
K_SORT_TILE = K_BLOCK * K_SORT_ITEMS
K_BUCKETS = 65
K_DEAD = 64


def tile_rounds(n):
    r = (n + K_BLOCK * K_TILE_TARGET - 1) // (K_BLOCK * K_TILE_TARGET)
    return min(max(r, 1), K_SORT_ITEMS)


def tile_span(n):
    return K_BLOCK * tile_rounds(n)


def tiles_of(n):
    span = tile_span(n)
    return (n + span - 1) // span


def max_tiles(n_max):
    """The most tiles any live count up to n_max is cut into."""
    if n_max >= K_TILE_TARGET * K_SORT_TILE:
        return (n_max + K_SORT_TILE - 1) // K_SORT_TILE
    return min(K_TILE_TARGET, (n_max + K_BLOCK - 1) // K_BLOCK)


def tile_stride(n_max):
    """The stride (in tiles) of the counts and offsets arrays of a pass of up to n_max rays."""
    return max(K_TILE_TARGET, (n_max + K_SORT_TILE - 1) // K_SORT_TILE)


def product_grid(n, cus):
    """The workgroups a reorder launch over n slots gets on a device of `cus` compute units."""
    return max(1, min(max_tiles(n), 8 * cus))


def last_tile_rounds(n):
    """The rounds the last tile of n slots runs (the other tiles run tile_rounds(n))."""
    base = (tiles_of(n) - 1) * tile_span(n)
    return min(tile_rounds(n), (n - base + K_BLOCK - 1) // K_BLOCK)


class FastDiv:
    """n // d for n < 2^31 as a multiply-high and a shift (rt_render.hip FastDiv), in Python integers."""

    def __init__(self, d):
        self.m, self.l = 0, 0
        if d > 1:
            self.l = (d - 1).bit_length()                       # 32 - clz(d - 1)
            self.m = (((1 << (31 + self.l)) + d - 1) // d) & 0xFFFFFFFF

    def div(self, n):
        return n if self.l == 0 else ((n * self.m) >> 32) >> (self.l - 1)


class SlotMap:
    """Bounce-0 slot -> global ray index of a pixel-tile owner: the owner's stripes back to back, its stripe j being
    global stripe j * count + index."""

    def __init__(self, stripe, count, index):
        self.stripe, self.skip, self.base = stripe, (count - 1) * stripe, index * stripe

    def ray(self, s):
        s = np.asarray(s, np.int64)
        return s + (s // self.stripe) * self.skip + self.base


def exchanged_bucket(v):
    """Bucket of an exchanged byte: v - 1 for v in 1..65, anything else reads as a dead ray."""
    v = np.asarray(v).astype(np.int64)
    return np.where((v >= 1) & (v <= K_BUCKETS), v - 1, K_DEAD).astype(np.uint8)


def bad_bytes(v):
    v = np.asarray(v)
    return int(((v < 1) | (v > K_BUCKETS)).sum())


def brute(bkt):
    """(order, live_next): order[k] = the slot whose ray lands at output slot k, for k < live_next; the dead rays'
    slots follow (nothing moves them)."""
    bkt = np.asarray(bkt, np.uint8)
    order = np.argsort(bkt, kind="stable")
    return order, int(bkt.size - (bkt == K_DEAD).sum())


class TileWalk:
    """counts, offsets: (65, tiles) -- what the kernels store at [b * stride + tile]; totals (65,); live_next;
    pos (n,): the output slot of each slot's ray (a dead ray's: its place behind the live ones, which no kernel
    stores through); runs (65,): the first output slot of each bucket."""


def tile_walk(bkt):
    bkt = np.asarray(bkt, np.uint8)
    n = bkt.size
    span, tiles = tile_span(n), tiles_of(n)
    w = TileWalk()
    w.n, w.rounds, w.span, w.tiles = n, tile_rounds(n), span, tiles
    w.counts = np.zeros((K_BUCKETS, tiles), np.int64)
    slots, tile_of, rank = [], [], []
    for b in range(K_BUCKETS):
        idx = np.flatnonzero(bkt == b)                          # this bucket's slots, ascending
        t = idx // span
        w.counts[b] = np.bincount(t, minlength=tiles) if tiles else 0
        # rank inside the tile: the bucket's rays before this one, less those of earlier tiles
        first = np.searchsorted(t, t, side="left")
        slots.append(idx)
        tile_of.append(t)
        rank.append(np.arange(idx.size) - first)
    w.offsets = np.cumsum(w.counts, axis=1) - w.counts           # exclusive scan over the tiles
    w.totals = w.counts.sum(axis=1)
    w.runs = np.cumsum(w.totals) - w.totals                      # bucket_runs: the totals of the smaller buckets
    w.live_next = n - int(w.totals[K_DEAD])
    w.pos = np.zeros(n, np.int64)
    for b in range(K_BUCKETS):
        if slots[b].size:
            w.pos[slots[b]] = w.runs[b] + w.offsets[b][tile_of[b]] + rank[b]
    return w


def strided(words, stride, fill):
    """A (65, tiles) array of the walk laid out as the kernels store it: (65 * stride,) uint32, `fill` where no
    kernel writes."""
    out = np.full((K_BUCKETS, stride), fill, np.uint32)
    out[:, :words.shape[1]] = words.astype(np.uint32)
    return out.reshape(-1)
