"""The reorder's yardstick checked on the CPU (no GPU): the regime each case names follows from the restated
formulas, the two restatements of the reorder (tests/reorder_ref.py: a stable argsort, and the kernels' tile
decomposition) agree on every case, and FastDiv in Python integers is floor division."""
import numpy as np
import pytest

import reorder_cases as K
import reorder_ref as M


def test_regime_table():
    for n, (rounds, tiles) in K.REGIMES.items():
        assert (M.tile_rounds(n), M.tiles_of(n)) == (rounds, tiles), n
    assert M.tile_span(1) == 256 and M.tile_span(8392705) == 4096
    # the scan walks a bucket's tiles in chunks of 256
    assert M.tiles_of(65536) == M.K_BLOCK and M.tiles_of(65537) == M.K_BLOCK + 1
    # the last tile of 524,289 holds one slot; of 2,097,153, 3 of its 5 rounds, the last of them one slot
    assert 524289 - (M.tiles_of(524289) - 1) * M.tile_span(524289) == 1
    assert M.last_tile_rounds(2097153) == 3 and M.tile_rounds(2097153) == 5
    assert 2097153 - (M.tiles_of(2097153) - 1) * M.tile_span(2097153) == 2 * 256 + 1
    # every size with R > 1 has a short last tile
    for n in K.LARGE_SIZES[1:]:
        assert M.tile_rounds(n) > 1 and M.last_tile_rounds(n) < M.tile_rounds(n), n
    # more tiles than workgroups: the product grid is 8 per compute unit (2048 on 256), grid overrides 1 and 3 below it
    assert M.tiles_of(K.HUGE) > M.product_grid(K.HUGE, 256) == 2048
    assert M.tiles_of(257) > 1 and M.tiles_of(65537) > 3
    # the full-size stride equals no case's tile count, so an index by `tiles` instead of the stride shows
    assert M.tile_stride(K.FULL_CAPACITY) == 10125
    assert all(M.tile_stride(n) == max(2048, -(-n // 4096)) for n in K.REGIMES)
    assert all(M.tiles_of(n) != 10125 and M.tiles_of(n) <= M.tile_stride(n) for n in K.REGIMES)
    assert all(M.max_tiles(n) >= M.tiles_of(n) for n in K.REGIMES)


def test_max_tiles_covers_every_smaller_count():
    """The grid of a pass of up to n_max rays (max_tiles) and the stride cover the tiles of every live count below it."""
    rng = np.random.default_rng(5)
    for n_max in list(K.REGIMES) + [K.FULL_CAPACITY]:
        for n in {0, 1, n_max // 2, max(n_max - 1, 0), n_max, min(n_max, 524288), min(n_max, 524289)} | \
                set(int(v) for v in rng.integers(0, n_max + 1, 50)):
            if n <= n_max:
                assert M.tiles_of(n) <= M.max_tiles(n_max) <= M.tile_stride(n_max), (n, n_max)


def _check_agreement(n, name):
    b = K.buckets(n, name)
    assert b.size == n and (b <= 64).all()
    order, live = M.brute(b)
    w = M.tile_walk(b)
    assert w.live_next == live
    assert np.array_equal(w.pos[order], np.arange(n)), (n, name)
    assert w.counts.shape == (65, K.REGIMES[n][1]) and w.counts.sum() == n
    assert np.array_equal(w.totals, np.bincount(b, minlength=65))
    return b, w


@pytest.mark.parametrize("n", K.SMALL_SIZES)
def test_brute_equals_tile_walk_small(n):
    for name in K.SMALL_DISTRIBUTIONS:
        _check_agreement(n, name)


@pytest.mark.parametrize("name", K.LARGE_DISTRIBUTIONS)
@pytest.mark.parametrize("n", [n for n in K.LARGE_SIZES if n <= K.CPU_LIMIT])
def test_brute_equals_tile_walk_large(n, name):
    _check_agreement(n, name)


def test_distributions_are_what_they_name():
    b = K.buckets(65537, "mod64")
    assert all(len(set(b[k:k + 64])) == 64 for k in range(0, 65536, 64))        # 64 distinct buckets in every wave
    b = K.buckets(65537, "wave_runs")
    assert all(len(set(b[k:k + 64])) == 1 for k in range(0, 65536, 64))         # one bucket per wave
    assert set(K.buckets(4000, "compaction")) == {0, 64} and 64 not in K.buckets(4000, "no_dead")
    assert (np.diff(K.buckets(4000, "ascending").astype(int)) >= 0).all()
    assert (np.diff(K.buckets(4000, "descending").astype(int)) <= 0).all()
    assert set(K.buckets(4000, "uniform")) == set(range(65))
    n = 524289
    for name, at in (("survivor_first", 0), ("survivor_span_end", 511), ("survivor_span", 512), ("survivor_last", n - 1)):
        assert list(np.flatnonzero(K.buckets(n, name) != 64)) == [at]
    geo, tz, rid = K.payload(1000)
    words = np.concatenate([geo.reshape(-1), tz, rid])
    assert len(set(words.tolist())) == words.size and K.SENTINEL not in words and K.FILL not in words


def test_global_cases_are_consistent():
    for n in K.GLOBAL_SMALL:
        g, planted = K.exchanged(n)
        assert M.bad_bytes(g) == planted == min(n // 3, 5) + min(n // 3, 7)
        assert (M.exchanged_bucket(g)[(g < 1) | (g > 65)] == 64).all()
        for idx in (0, 1):
            own = K.ownership(n, "stripes37_%d" % idx)
            mine = np.flatnonzero(own)
            assert np.array_equal(M.SlotMap(K.STRIPE, 2, idx).ray(np.arange(mine.size)), mine)
    assert np.array_equal(M.exchanged_bucket(np.array([0, 1, 65, 66, 255])), [64, 0, 64, 64, 64])


FASTDIV_D = [1, 2, 3, 4, 5, 7, 19, 20, 21, 255, 256, 257, 1920, 65535, 65536, 65537, 2**30, 2**30 + 1, 2**31 - 1]


def fastdiv_inputs():
    """(d, n) pairs shared with the device test: the named divisors and 2000 random ones, each with the dividends
    around its multiples and random ones, all n < 2^31."""
    rng = np.random.default_rng(11)
    ds = FASTDIV_D + [int(v) for v in rng.integers(1, 2**31, 2000)]
    pairs = []
    for d in ds:
        ns = [0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2**31 - 1] + [int(v) for v in rng.integers(0, 2**31, 8)]
        pairs += [(d, n) for n in ns if 0 <= n < 2**31]
    return pairs


def test_fastdiv_is_floor_division():
    for d, n in fastdiv_inputs():
        assert M.FastDiv(d).div(n) == n // d, (d, n)
    for d in FASTDIV_D:
        assert 0 <= M.FastDiv(d).m < 2**32
