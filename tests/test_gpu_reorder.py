"""The reorder kernels of rt_render.hip against a stable sort, bit for bit, at every tile regime.

The test build (librtamd_test.so, rtamd.test_lib()) has direct entry points that launch the product kernels on host
arrays (rt_render.hip, RTAMD_TEST_HOOKS).  Every case of tests/reorder_cases.py runs through them and is compared
with tests/reorder_ref.py: the intermediate arrays (per-tile counts, scanned offsets, totals, the next live count)
with the tile walk, so a mismatch names the kernel, and the moved ray state with the gather by numpy's stable argsort.
Outputs start as a sentinel with guard words behind them; everything a kernel has no business writing must still
hold it.  Then the small renders of the other GPU tests run through the test build with RTAMD_TEST_SORT_GRID=3, which
gives every reorder workgroup several tiles (the two kernels that replay the shading cannot be driven without a
scene), and one frame whose bounce-0 live count is in the R = 5 regime, all against the oracle.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import reorder_cases as K
import reorder_ref as M
import rtamd as R
from test_reorder_ref import fastdiv_inputs

pytestmark = pytest.mark.gpu

P, I32, I64, U32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32


@pytest.fixture(scope="module")
def T():
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    L = R.test_lib()
    L.rtamd_test_reorder_plain.argtypes = [I32, P, I32, I64, I32, U32, I32, P, P, P, P, P, P, I64, P, P, P, P, P]
    L.rtamd_test_reorder_global.argtypes = [I32, P, P, I32, I64, I32, U32, I32, P, I64, P, P, P, P, P, P,
                                            I32, P, P, I32, U32, I32, I32, P, I64, P]
    L.rtamd_test_tile_bytes.argtypes = [I32, P, I32, P, U32, I32, I32, I32, P, P, I64]
    L.rtamd_test_fastdiv.argtypes = [I32, P, P, I32, P]
    return L


def ptr(a):
    return a.ctypes.data_as(P) if a is not None else None


def check(rc, L):
    assert rc == 0, L.rt_last_error().decode()


def same(got, want, what, case):
    """Exact equality; on a mismatch, where it starts and how far it goes."""
    if not np.array_equal(got, want):
        bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
        pytest.fail("%s differs in case %r: %d of %d words, first at %d (got %#x, want %#x), last at %d" % (
            what, case, bad.size, np.asarray(want).size, bad[0], int(np.asarray(got).reshape(-1)[bad[0]]),
            int(np.asarray(want).reshape(-1)[bad[0]]), bad[-1]))


def scratch(stride):
    """counts, offsets, totals, live_next as the hooks return them."""
    return (np.zeros(65 * stride, np.uint32), np.zeros(65 * stride, np.uint32), np.zeros(65, np.uint32),
            np.zeros(1, np.uint32))


def check_scratch(got, w, stride, case, live_next):
    counts, offsets, totals, live = got
    same(counts, M.strided(w.counts, stride, K.FILL), "counts (histogram)", case)
    same(offsets, M.strided(w.offsets, stride, K.FILL), "offsets (scan)", case)
    same(totals, w.totals.astype(np.uint32), "totals (scan)", case)
    assert int(live[0]) == live_next, ("live_next (scan)", case, int(live[0]), live_next)


# ---------------------------------------------------------------- the plain reorder
@functools.lru_cache(maxsize=2)
def plain_reference(n, name):
    """Computed once per (size, distribution) and shared by its capacities and grids: the buckets, the payload, the
    stable order, the tile walk and the expected outputs (sentinel behind the live prefix and in the guard)."""
    b = K.buckets(n, name)
    order, live = M.brute(b)
    w = M.tile_walk(b)
    assert w.live_next == live
    pay = K.payload(n)
    want = []
    for a in pay:
        out = np.full((n + K.GUARD,) + a.shape[1:], K.SENTINEL, np.uint32)
        out[:live] = a[order[:live]]
        want.append(out)
    for a in (b, order) + pay + tuple(want):
        a.flags.writeable = False
    return b, w, live, pay, tuple(want)


def run_plain(T, n, name, capacity, grid):
    case = (n, name, capacity, grid)
    b, w, live, pay, want = plain_reference(n, name)
    stride = M.tile_stride(capacity)
    outs = [np.full(a.shape, K.SENTINEL, np.uint32) for a in want]
    sc = scratch(stride)
    g = C.c_int(-1)
    check(T.rtamd_test_reorder_plain(0, ptr(b), n, capacity, grid, K.FILL, stride, ptr(pay[0]), ptr(pay[1]), ptr(pay[2]),
                                     ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), n + K.GUARD, ptr(sc[0]), ptr(sc[1]),
                                     ptr(sc[2]), ptr(sc[3]), C.byref(g)), T)
    assert g.value == grid if grid else 1 <= g.value <= max(1, M.max_tiles(n)), case
    check_scratch(sc, w, stride, case, live)
    for got, exp, what in zip(outs, want, ("geo", "tz", "rid")):
        same(got, exp, what + " (scatter; sentinel from slot %d on)" % live, case)
    return g.value


@pytest.mark.parametrize("n", K.SMALL_SIZES)
def test_plain_reorder_small(T, n):
    """R = 1: every distribution, both capacities, and the grids 0 (the renderer's: a workgroup per tile), 1 and 3
    (several tiles per workgroup, so the LDS histogram, the wave counts and the runs are set up again)."""
    for name in K.SMALL_DISTRIBUTIONS:
        for cap in K.capacities(n):
            for grid in K.SMALL_GRIDS:
                run_plain(T, n, name, cap, grid)


@pytest.mark.parametrize("name", K.LARGE_DISTRIBUTIONS)
@pytest.mark.parametrize("n", [n for n in K.LARGE_SIZES if n != K.HUGE])
def test_plain_reorder_large(T, n, name):
    """R = 1..9 with the renderer's grid: short last tiles, and the histogram's later batches of four rounds."""
    for cap in K.capacities(n):
        run_plain(T, n, name, cap, 0)


@pytest.mark.parametrize("cap", K.capacities(K.HUGE))
@pytest.mark.parametrize("name", K.LARGE_DISTRIBUTIONS)
def test_plain_reorder_more_tiles_than_workgroups(T, name, cap):
    """R = 16 and 2050 tiles: on a device of up to 256 compute units the renderer's grid is smaller."""
    grid = run_plain(T, K.HUGE, name, cap, 0)
    assert grid < M.tiles_of(K.HUGE), "this device's reorder grid (%d) covers every tile" % grid


# ---------------------------------------------------------------- pixel tiles: the global rank and the local reorder
@functools.lru_cache(maxsize=2)
def global_reference(n):
    g, planted = K.exchanged(n)
    bkt = M.exchanged_bucket(g)
    w = M.tile_walk(bkt)
    order, live = M.brute(bkt)
    assert np.array_equal(w.pos[order], np.arange(n))
    return g, planted, bkt, w


def run_global(T, n, owner, capacity, grid):
    case = (n, owner, capacity, grid)
    g, planted, bkt, w = global_reference(n)
    own = K.ownership(n, owner)
    stride = M.tile_stride(capacity)
    mine = np.flatnonzero(own)                       # this owner's global slots, ascending: its local slot order
    want_newpos = np.full(n + K.GUARD, K.SENTINEL, np.uint32)
    ranked = mine[bkt[mine] != M.K_DEAD]
    want_newpos[ranked] = w.pos[ranked]
    bl = np.ascontiguousarray(bkt[mine])
    order_l, live_l = M.brute(bl)
    want_gslot = np.full(mine.size + K.GUARD, K.SENTINEL, np.uint32)
    want_gslot[:live_l] = w.pos[mine[order_l[:live_l]]]
    assert (np.diff(want_gslot[:live_l].astype(np.int64)) > 0).all()      # the owner's rays keep the global order
    gslot_in = np.ascontiguousarray(mine.astype(np.uint32))
    forms = [0] + ([2] if owner.startswith("stripes37_") else [])
    for form in forms:
        newpos = np.full(n + K.GUARD, K.SENTINEL, np.uint32)
        gslot_out = np.full(mine.size + K.GUARD, K.SENTINEL, np.uint32)
        sc = scratch(stride)
        bad, live_l_got = np.full(1, K.SENTINEL, np.uint32), np.full(1, K.SENTINEL, np.uint32)
        gr = C.c_int(-1)
        check(T.rtamd_test_reorder_global(0, ptr(g), ptr(own), n, capacity, grid, K.FILL, stride, ptr(newpos), n + K.GUARD,
                                          ptr(bad), ptr(sc[3]), ptr(sc[0]), ptr(sc[1]), ptr(sc[2]), C.byref(gr),
                                          mine.size, ptr(bl), ptr(gslot_in) if form == 0 else None, form, K.STRIPE, 2,
                                          int(owner[-1]) if form == 2 else 0, ptr(gslot_out), mine.size + K.GUARD,
                                          ptr(live_l_got)), T)
        check_scratch(sc, w, stride, case, w.live_next)
        assert int(bad[0]) == planted, ("bad", case, int(bad[0]), planted)
        same(newpos, want_newpos, "newpos (rank; written only at this owner's live slots)", case)
        assert int(live_l_got[0]) == live_l, ("local live_next", case, form)
        same(gslot_out, want_gslot, "gslot_out (scatter<%d>)" % form, case)
    return gr.value


@pytest.mark.parametrize("n", K.GLOBAL_SMALL)
def test_global_rank_small(T, n):
    for owner in K.OWNERSHIPS:
        for cap in K.capacities(n):
            for grid in K.SMALL_GRIDS:
                run_global(T, n, owner, cap, grid)


@pytest.mark.parametrize("n,owner,cap,grid", [c for c in K.global_cases() if c[0] in K.GLOBAL_LARGE])
def test_global_rank_large(T, n, owner, cap, grid):
    """The pixel-tile kernels at R = 2, 5 and 16, with short last tiles; at R = 16 with more tiles than workgroups."""
    got = run_global(T, n, owner, cap, grid)
    if n == K.HUGE:
        assert got < M.tiles_of(n), "this device's reorder grid (%d) covers every tile" % got


# ---------------------------------------------------------------- the bucket bytes of a pixel-tile owner
# n_global % 16 in {0, 1, 15}: the 16-byte bulk and the byte tail of zero_bytes_kernel; 15: no bulk at all; the
# largest: more 16-byte words than the zeroing grid has threads, and more local rays than tile_bytes_kernel's
@pytest.mark.parametrize("n", [15, 16, 17, 4096, 4097, 4111, 65536 + 15, K.HUGE])
def test_tile_bytes(T, n):
    assert n % 16 in (0, 1, 15)
    rng = np.random.default_rng(n)
    for owner in ("all", "one", "stripes37_0", "stripes37_1"):
        own = K.ownership(n, owner)
        mine = np.flatnonzero(own)
        bkt = rng.integers(0, 65, mine.size).astype(np.uint8)
        want = np.full(n + K.GUARD, 0xEE, np.uint8)
        want[:n] = 0
        want[mine] = bkt + 1
        forms = [0] + ([1] if owner.startswith("stripes37_") else [])
        for first in forms:
            G, L = np.full(n + K.GUARD, 0xEE, np.uint8), np.full(n + K.GUARD, 0xEE, np.uint8)
            gslot = np.ascontiguousarray(mine.astype(np.uint32)) if first == 0 else None
            check(T.rtamd_test_tile_bytes(0, ptr(bkt), mine.size, ptr(gslot), K.STRIPE, 2, int(owner[-1]) if first else 0,
                                          n, ptr(G), ptr(L), n + K.GUARD), T)
            same(G, want, "G (tile_bytes<%d>)" % first, (n, owner))
            same(L, want, "L (tile_bytes<%d>)" % first, (n, owner))


def test_hooks_refuse_indices_outside_their_arrays(T):
    """The hooks check on the host what a kernel would index with, so a wrong test cannot store out of bounds."""
    one = np.zeros(1, np.uint8)
    big = np.full(1, 65, np.uint8)
    w = np.zeros(65 * 2048, np.uint32)
    out = np.zeros(8 * 65, np.uint32)
    assert T.rtamd_test_reorder_plain(0, ptr(big), 1, 1, 0, 0, 2048, ptr(out), ptr(out), ptr(out), ptr(out), ptr(out),
                                      ptr(out), 65, ptr(w), ptr(w), ptr(out), ptr(out), None) != 0
    assert T.rtamd_test_reorder_plain(0, ptr(one), 1, 1, 0, 0, 2047, ptr(out), ptr(out), ptr(out), ptr(out), ptr(out),
                                      ptr(out), 65, ptr(w), ptr(w), ptr(out), ptr(out), None) != 0
    far = np.full(1, 5, np.uint32)
    assert T.rtamd_test_tile_bytes(0, ptr(one), 1, ptr(far), 1, 1, 0, 5, ptr(out), ptr(out), 64) != 0
    assert T.rtamd_test_tile_bytes(0, ptr(one), 1, None, 37, 2, 1, 37, ptr(out), ptr(out), 64) != 0


# ---------------------------------------------------------------- FastDiv on the device
def test_fastdiv_on_device(T):
    pairs = fastdiv_inputs()
    d = np.array([p[0] for p in pairs], np.uint32)
    n = np.array([p[1] for p in pairs], np.uint32)
    out = np.zeros(d.size, np.uint32)
    check(T.rtamd_test_fastdiv(0, ptr(d), ptr(n), d.size, ptr(out)), T)
    want = (n.astype(np.int64) // d.astype(np.int64)).astype(np.uint32)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, [(int(d[k]), int(n[k]), int(out[k]), int(want[k])) for k in bad[:8]]


# ---------------------------------------------------------------- renders with several tiles per workgroup
@functools.lru_cache(maxsize=None)
def oracle(scene, image, sort):
    """The oracle's render, once per scene, size and sort."""
    fb, st = O.OracleScene("%s/%s.scene" % (R.ASSETS, scene), image=image).render(sort=sort)
    fb.flags.writeable = False
    return fb, st


def check_render(T, scene, image, sort):
    ofb, ost = oracle(scene, image, sort)
    gfb, gst = R.render(R.Scene("%s/%s.scene" % (R.ASSETS, scene), image=image), sort=sort, counters=True, L=T)
    assert np.array_equal(gfb, ofb), "%d of %d floats differ" % (int((gfb != ofb).sum()), ofb.size)
    assert gst["live_segments"] == ost["live_segments"]
    assert gst["nodes_popped"] == ost["nodes_popped"]
    assert gst["internal_visits"] == ost["internal_visits"]
    assert gst["triangle_tests"] == ost["triangle_tests"]
    assert gst["misses"] == ost["misses"]
    assert gst["hits"] == ost["hits_triangle"] + ost["hits_sphere"]
    assert gst["generated_rays"] == image[0] * image[1] * image[2]


def set_knobs(monkeypatch, fused, vreorder):
    monkeypatch.setenv("RTAMD_FUSED", fused)
    monkeypatch.setenv("RTAMD_VREORDER", vreorder)


@pytest.mark.parametrize("scene,image,sort", [("cornell", (64, 64, 24, 4), True), ("cornell", (64, 64, 24, 4), False),
                                              ("cornell_plus", (48, 48, 20, 8), True)])
def test_render_three_workgroups(T, monkeypatch, scene, image, sort):
    """RTAMD_TEST_SORT_GRID=3 (test build only): every reorder kernel of the render, and the shade kernel where it
    counts the buckets, walks its tiles on three workgroups."""
    monkeypatch.setenv("RTAMD_TEST_SORT_GRID", "3")
    check_render(T, scene, image, sort)


@pytest.mark.parametrize("vreorder", ["0", "1"])
@pytest.mark.parametrize("fused", ["0", "1"])
def test_render_three_workgroups_every_reorder(T, monkeypatch, fused, vreorder):
    """The same under the knobs that pick the reorder: the moved one (sort_hist / sort_scatter), the fused replay
    (shade_kernel's histogram, sort_scatter_shade_kernel) and the virtual bounce-0 reorder (shade_rank_kernel)."""
    monkeypatch.setenv("RTAMD_TEST_SORT_GRID", "3")
    set_knobs(monkeypatch, fused, vreorder)
    check_render(T, "teapot", (96, 54, 20, 16), True)


@pytest.mark.parametrize("exchange", ["host", "device"])
def test_tiles_with_sort_on_three_workgroups(T, monkeypatch, exchange):
    """A pixel-tile render with the reorder on (test_gpu_tiles.py's teapot case) through the test build: the global
    histogram and rank and the owners' scatters with several tiles per workgroup."""
    from test_gpu_tiles import render_owners
    monkeypatch.setenv("RTAMD_TEST_SORT_GRID", "3")
    scene, image, rows, owners = "teapot", (64, 36, 20, 16), 4, 3
    ref, rst = oracle(scene, image, True)
    fb, sts = render_owners("%s/%s.scene" % (R.ASSETS, scene), image, rows, owners, exchange, L=T)
    assert np.array_equal(fb, ref)
    assert sum(s["live_segments"] for s in sts) == rst["live_segments"]


# 512 x 256 x 20 = 2,621,440 rays at bounce 0: R = 5 and 2048 tiles, the last one full.  As rays die the later
# bounces run R = 3 and R = 2 with short last tiles (asserted below from the oracle's live counts).  Product grid.
# The oracle renders this frame in 0.33 s on the GPU host (0.27 s for 256 x 256 x 20), so the size stays.
R5_IMAGE = (512, 256, 20, 4)
# 511 x 255 x 20 = 2,606,100 rays: R = 5 and a last tile of 20 slots, one round of five, at bounce 0 -- and at bounce 1
# of the virtual reorder, whose shade_rank_kernel walks every slot of the pass whatever has died
R5_SHORT_IMAGE = (511, 255, 20, 3)


@functools.lru_cache(maxsize=None)
def live_counts(scene, image):
    """The live count of every bounce of the frame's one pass, from the oracle's bucket histograms (a bounce's
    histogram counts every slot of the pass; bucket 64 holds the rays dead by then)."""
    _, _, h = O.OracleScene("%s/%s.scene" % (R.ASSETS, scene), image=image).render(sort=True, hist=True)
    n = int(h[0, 0].sum())
    return [n] + [n - int(h[0, b, 64]) for b in range(image[3] - 1)]


@pytest.mark.parametrize("vreorder", ["0", "1"])
@pytest.mark.parametrize("fused", ["0", "1"])
def test_render_r5_frame(T, monkeypatch, fused, vreorder):
    """A frame whose bounce-0 live count is in the R = 5 regime: the shade-side histogram and the two scatters that
    replay the shading run with R > 1 and, at the later bounces, short last tiles."""
    live = live_counts("cornell", R5_IMAGE)
    assert live[0] == 2621440 and M.tile_rounds(live[0]) == 5
    for n in live[1:3]:                 # the bounces that are reordered after bounce 0
        assert M.tile_rounds(n) > 1 and n % M.tile_span(n) != 0, live
    monkeypatch.delenv("RTAMD_TEST_SORT_GRID", raising=False)
    set_knobs(monkeypatch, fused, vreorder)
    check_render(T, "cornell", R5_IMAGE, True)


@pytest.mark.parametrize("fused,vreorder", [("0", "0"), ("0", "1"), ("1", "0")])
def test_render_r5_frame_short_last_tile(T, monkeypatch, fused, vreorder):
    """R = 5 with a short last tile in the pass's own ray count: shade_rank_kernel (the virtual reorder) and bounce 0
    of the shade-side histogram, of the moved reorder (sort_scatter_kernel<1>) and of the fused replay; the odd width
    and height go through FastDiv's ray -> pixel -> row."""
    n = R5_SHORT_IMAGE[0] * R5_SHORT_IMAGE[1] * R5_SHORT_IMAGE[2]
    assert M.tile_rounds(n) == 5 and M.last_tile_rounds(n) == 1 and n % M.tile_span(n) == 20
    monkeypatch.delenv("RTAMD_TEST_SORT_GRID", raising=False)
    set_knobs(monkeypatch, fused, vreorder)
    check_render(T, "cornell", R5_SHORT_IMAGE, True)
