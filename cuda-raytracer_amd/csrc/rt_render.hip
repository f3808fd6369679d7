// rt_render.hip — gfx950 kernels and pass orchestration of the MI355X path tracer.
//
// Replaces gpu_raytrace (reference raytracing.cu:170-284) and the per-ray device functions it
// launches (scene.cu:78-487), plus the bloom kernels (raytracing.cu:21-74).  Design:
//   * one lane per ray slot, 256-thread workgroups (4 wave64s);
//   * BVH as 64-B "child-pair" records: an internal node stores both children's AABBs and
//     their refs, so one 64-B load feeds both slab tests (the reference reads 32 B for the
//     popped node plus 2 x 32 B for the children); leaves are encoded in the ref itself;
//   * per-lane traversal stack in LDS, [entry][lane] layout (conflict-free ds_*_b64), with
//     a private overflow tail; the top-of-stack child is kept in registers, so only the
//     deferred (near) child of a two-hit node is ever pushed.  Pop order is the reference's
//     (far child first, scene.cu:204-225), so hits and tie-breaks are identical;
//   * the ray reorder is a stable 65-bucket multisplit (6 live key bits + terminated,
//     SURVEY §8a rows K/L): tile histograms, per-bucket scan, and a scatter that ranks with
//     seven 64-lane __ballot()s per round;
//   * accumulation is an ordered per-pixel sum (deterministic; no float atomics).
// This file holds the render's kernels, the renderer (rt_renderer: option parsing, pass contexts, the pass
// schedule) and its C ABI.  Beside it: rt_common.h (constants, DevScene, the traversal building blocks and HIP
// helpers shared with the other .hip files), scene_dev.hip (SceneDev, the resident scene a renderer owns;
// the node records come from host/bvh_records.cpp), rt_query.hip (the ray-query kernels and rt_query_*, which
// launch this file's trace_kernel through launch_trace_closest), bvh_refit.hip, rt_multi.hip.
#include "rt_common.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#pragma clang fp contract(off)

int rtamd_render_multi(const rt_scene *scene, const rt_opts *opts, float *fb_out, rt_stats *stats);   // rt_multi.hip

using namespace rtamd;

namespace {

// Tuning knobs (compile-time; -D overrides are for A/B experiments only; the traversal's are in rt_common.h).
#ifndef RT_INFLIGHT
#define RT_INFLIGHT 20                // with 24 HW queues: +1.5 % teapot, +3.4 % lamp over 16 (24 in flight: worse)
#endif
#ifndef RT_TRACE_OCC
#define RT_TRACE_OCC 0                // fixed % of the resident trace workgroups (0: adaptive, below)
#endif
#ifndef RT_TRACE_OCC_MIN
#define RT_TRACE_OCC_MIN 15
#endif
#ifndef RT_SORT_ITEMS
#define RT_SORT_ITEMS 16
#endif
#ifndef RT_SHADE_BPC
#define RT_SHADE_BPC 8
#endif
constexpr int kSortItems = RT_SORT_ITEMS;   // sort tile = kBlock * kSortItems slots (at most)
constexpr int kSortTile = kBlock * kSortItems;
// A reorder launch cuts the live prefix into tiles of 256-slot rounds, one workgroup per tile at a
// time, the rounds of a tile in sequence (each waits for its slots' loads).  Big prefixes use
// kSortItems rounds per tile; a small one (the tail bounces: 10^4-10^5 rays) uses fewer rounds and
// more tiles, aiming at kTileTarget tiles, so its few workgroups do not each walk 16 dependent rounds
// (round 3: a tail bounce's histogram and scatter took 40-60 us for ~20 k rays).  Every kernel of one
// reorder derives the same rounds from the same live count.
constexpr int kTileTarget = 2048;
__host__ __device__ __forceinline__ int tile_rounds(int n) {
    const int r = (int)(((int64_t)n + (int64_t)kBlock * kTileTarget - 1) / ((int64_t)kBlock * kTileTarget));
    return r < 1 ? 1 : (r > kSortItems ? kSortItems : r);
}
__host__ __device__ __forceinline__ int tiles_of(int n) {
    const int span = kBlock * tile_rounds(n);
    return (n + span - 1) / span;
}
// the most tiles any live count up to n_max is cut into (a launch's grid)
inline int max_tiles(int64_t n_max) {
    return n_max >= (int64_t)kTileTarget * kSortTile ? (int)((n_max + kSortTile - 1) / kSortTile)
                                                    : (int)std::min<int64_t>(kTileTarget, (n_max + kBlock - 1) / kBlock);
}
// counts/offsets stride (tiles) that covers every live count up to n_max
inline int tile_stride(int64_t n_max) {
    return (int)std::max<int64_t>(kTileTarget, (n_max + kSortTile - 1) / kSortTile);
}
constexpr int kBuckets = 65;
constexpr int kInflight = RT_INFLIGHT; // passes in flight (one stream and buffer set each)
constexpr int kStaggerUs = 4000;       // staggered start of the first passes in flight (rt_renderer::run):
constexpr int kStaggerGroup = 4;       // the first kStaggerGroup together, then one every kStaggerUs
constexpr int kStaggerMinPasses = 8;   // ...for renders of at least this many passes
constexpr int kStaggerShortUs = 2000;  // the same for runs shorter than the passes in flight (run_impl)
// Persistent trace grid as a % of the resident trace workgroups: the passes in flight share the
// chip, so each pass's trace takes 200 % / (passes in flight), at least RT_TRACE_OCC_MIN and at most
// 100 % (20 in flight: 15 %; A/B at 20 in flight: 40 % 7.51, 30 % 7.41, 20 % 7.37, 15 % 7.33,
// 10 % 7.35 ms/pass; lamp and the 13-pass share also best at 15 %).
constexpr int kTraceOccPct = RT_TRACE_OCC;
constexpr uint32_t kDead = 64;        // bucket of a terminated ray (key 0xFFFFFFFF)
constexpr uint32_t kAccFlag = 0x80000000u;   // in a ray id (rid): acc[ray] holds the ray's radiance so far
// Per-launch span words (rt_renderer_set_event_timing): 8 start slots then 8 end slots, one per XCD
// (workgroup i runs on XCD i % 8), each written by one atomic per workgroup -- one word for a whole
// 8192-wave launch serialised its waves' atomics and lengthened the span it measured (round 3:
// 0.82 vs the profiler's 0.66 ms per exclusive teapot launch).
constexpr int kSpanSlots = 8;
constexpr int kSpanWords = 2 * kSpanSlots;
#ifdef RT_PROFILE
// Wave-level traversal profile (debug builds only): see tools/variants.sh + RT_PROFILE=1.
__device__ unsigned long long g_prof[2][14];   // [bounce 0, later bounces]
#define PROF(i, v) (prof[i] += (v))
#else
#define PROF(i, v) ((void)0)
#endif

// ---------------------------------------------------------------- ray generation
// generate_initial_rays (scene.cu:78-105, raytracing.cu:76-81), evaluated where a bounce-0 ray
// is needed (trace and shade of bounce 0) instead of being written out and read back.  Ray i
// of a pass is slot i at bounce 0.  Ray state afterwards: geo[2 i .. 2 i + 1] = {o.xyz, d.x},
// {d.yz, T.xy} (what traversal reads) and tz[i] = T.z; the radiance goes to acc[ray id] (shade_kernel).
// n / d for n < 2^31 as a multiply-high and a shift (Granlund-Montgomery: m = ceil(2^(31+l)/d),
// l = ceil(log2 d)); l = 0 means d = 1.
struct FastDiv {
    uint32_t m = 0;
    int l = 0;
    static FastDiv of(uint32_t d) {
        FastDiv f;
        if (d > 1) {
            f.l = 32 - __builtin_clz(d - 1);
            f.m = (uint32_t)((((uint64_t)1 << (31 + f.l)) + d - 1) / d);
        }
        return f;
    }
    __device__ __forceinline__ uint32_t div(uint32_t n) const { return l == 0 ? n : (__umulhi(n, m) >> (l - 1)); }
};

// Bounce-0 slot -> global ray index (pixel * rtc + sample).  The whole image: the identity.
// Pixel-tile sharding (rt_opts.tile_*): the pass's slots are this owner's row stripes back to
// back, stripe j of the owner being global stripe j * tile_count + tile_index, so
//   ray = slot + (slot / stripe) * (tile_count - 1) * stripe + tile_index * stripe.
// Later bounces carry the ray index in rid[].  The same map on pixels (stripe = rows * W)
// serves accumulation.
struct SlotMap {
    FastDiv by_stripe;
    uint32_t skip, base;              // (tile_count - 1) * stripe, tile_index * stripe
    static SlotMap identity() { return SlotMap{FastDiv::of(0x7fffffffu), 0u, 0u}; }
    static SlotMap of(uint32_t stripe, int count, int index) {
        return SlotMap{FastDiv::of(stripe), (uint32_t)(count - 1) * stripe, (uint32_t)index * stripe};
    }
    __device__ __forceinline__ uint32_t ray(uint32_t s) const { return s + by_stripe.div(s) * skip + base; }
};

// Bounce-0 kernels come in two flavours: FIRST == 1 (whole image, slot = ray index) and
// FIRST == 2 (pixel tile, mapped); later bounces are FIRST == 0.  Keeping the map out of the
// whole-image kernels keeps their code (and registers) as they were.
template <int FIRST>
__device__ __forceinline__ uint32_t first_ray(const SlotMap &m, uint32_t slot) {
    return FIRST == 2 ? m.ray(slot) : slot;
}

struct PassArgs {
    int rtc;                          // rays per pixel this pass
    uint32_t gen_seed_term;           // 709579 * remaining (scene.cu:81)
    FastDiv by_rtc, by_width;         // ray index -> pixel -> row
    SlotMap map;                      // bounce-0 slot -> ray index
};

__device__ __forceinline__ V3 primary_dir(const DevScene &S, int i, const PassArgs &pa) {
    Rng rng = pcg_seed((uint32_t)i * 0x85810BEAu + pa.gen_seed_term);   // 298592570346 mod 2^32
    // the increment made opaque where it is used: as a loop-invariant 64-bit constant the compiler
    // hoisted it (and its `| 1`) out of the trace kernel's loop and spilled both to scratch, so
    // every bounce-0 refill waited for two scratch reloads
    uint32_t z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    rng.inc += z;
    const uint32_t pixel = pa.by_rtc.div((uint32_t)i);
    const uint32_t yy = pa.by_width.div(pixel);
    const int x = (int)(pixel - yy * (uint32_t)S.width), y = (int)yy;
    const float xc = (x + random01(rng)) * S.inv_w;
    const float yc = (y + random01(rng)) * S.inv_h;
    return normalise(S.tl + xc * S.sr - yc * S.su);
}

// ---------------------------------------------------------------- traversal
#ifndef RT_FUSED_MAX_TRIS
#define RT_FUSED_MAX_TRIS 4096        // fused reorder for scenes up to this many triangles (see enqueue_pass)
#endif
#ifndef RT_SORT_GRID
#define RT_SORT_GRID 0                // cap on the reorder's hist/scatter grid (0: 8 blocks per CU)
#endif
// The reorder kernels walk their tiles on at most 8 workgroups per CU.  The test build (librtamd_test.so) reads
// another cap from RTAMD_TEST_SORT_GRID, so that a small render gives every workgroup several tiles.
inline int reorder_grid_cap(int cus) {
#ifdef RTAMD_TEST_HOOKS
    if (const char *e = std::getenv("RTAMD_TEST_SORT_GRID"))
        if (std::atoi(e) > 0) return std::atoi(e);
#endif
    return cus * 8;
}
// The shade kernel walks the same tiles where it counts the buckets (shade_kernel's `counts`), so under the test
// cap its grid is capped alike; without it, RT_SHADE_BPC workgroups per CU.
inline int shade_grid_cap(int cus, int bpc) {
#ifdef RTAMD_TEST_HOOKS
    if (reorder_grid_cap(cus) != cus * 8) return reorder_grid_cap(cus);
#endif
    return cus * bpc;
}

// Closest hit for the live slots [0, *live): the sphere loop (scene.cu:338-372) and
// bvh_closest_hit_distance (scene.cu:134-241).  Persistent and wave-refilling: each wave takes
// chunks of slots from a device queue (one atomic per chunk) and hands a new slot to a lane
// as soon as that lane's ray is done, so incoherent rays of very different traversal lengths
// do not leave most lanes idle.  Output per slot: {closest t, hit index} (index -1 = miss).
// The slab pair, the flat triangle test and the leaf refs are rt_common.h's (shared with anyhit_kernel).
// VSLOT (bounce 1 of the virtual reorder, below): the launch walks every slot of the pass, slot = ray id, and a
// slot whose bounce-0 bucket (slot_bkt) is kDead is dropped at refill, before anything is counted; geo holds the slim
// hand-over's 16-B records {d, t0} (shade_kernel<.., SLIM>), the origin is bounce 0's cam + t0 * primary_dir(slot).
// Its output is lean: `hits` is a dense array of 4-B hit indices (a miss costs those 4 bytes), and a lane that hit
// also writes the hit point o + closest * d, shade_from's own expression, as 3 floats at hit_org + 3 * slot.
template <bool SORTED, bool COUNT, int FIRST, bool VSLOT = false>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void trace_kernel(DevScene S, PassArgs pa, const float4 *__restrict__ geo,
                                                       const uint32_t *__restrict__ live_count,
                                                       uint32_t *__restrict__ queue, float2 *__restrict__ hits,
                                                       uint32_t *__restrict__ overflow, Counters *__restrict__ ctr,
                                                       unsigned long long *__restrict__ tspan,
                                                       const uint8_t *__restrict__ slot_bkt = nullptr,
                                                       float *__restrict__ hit_org = nullptr) {
    __shared__ uint2 stack[(kStackLds + 1) * kBlock];   // + one scratch entry per lane
    // tspan (per-launch timing, rt_renderer_set_event_timing): {first wave start, last wave end}
    // on the device's constant-rate wall clock, so a launch's duration excludes the queueing
    // before its first wave and the stream's marker packets (what rocprofv3 reports).  The start is
    // read into scalar registers here and published with the end at exit: an atomic issued at the
    // start counts in vmcnt, so the root record's loads below waited for it, and the device-scope
    // atomics of ~2000 workgroups queue (round 3: 0.76 ms per exclusive teapot launch with the
    // timing on against 0.63 with it off, both by the profiler's dispatch durations)
    const unsigned long long t_start = wall_clock64();
    uint2 *col = stack + threadIdx.x;
    // Overflow tail of the stack (entries >= kStackLds, rare) in a global per-lane buffer,
    // [entry][lane] for coalescing; refs and distances in two 32-bit halves so the compiler cannot
    // fuse the LDS and global pops into one flat load.
    // Entry e >= kStackLds of this lane's overflow: ref at overflow[e' * lanes + lane], dist in the
    // second half (e' = e - kStackLds), addressed on use (the path is rare; no pointer registers).
    const uint32_t lanes = gridDim.x * kBlock, gl = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t dist_half = lanes * (kStackMax - kStackLds);
    // VSLOT: the lane's index is put together where the rare path uses it, from an opaque thread index, and is not
    // kept through the loop: with the refill's primary_dir the kernel otherwise spills it (12 B of scratch)
    auto overflow_lane = [&]() -> uint32_t {
        if (!VSLOT) return gl;
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        return blockIdx.x * kBlock + t;
    };
    const uint32_t L = __builtin_amdgcn_readfirstlane(*live_count);
    const uint32_t waves = gridDim.x * (kBlock / 64);
    const uint32_t chunk = min((uint32_t)kChunkMax, max((uint32_t)kChunkMin, (L / (4 * waves) + 63) & ~63u));
    // The live range is split into kQueues equal segments, each with its own queue word; a wave
    // starts on the segment of its XCD group (blockIdx % 8) and moves on when that one is drained.
    uint32_t shard = blockIdx.x % kQueues, tried = 0;
    uint32_t q_next = 0, q_end = 0;     // this wave's current chunk (wave-uniform)
    bool exhausted = false;
    int slot = -1;                      // < 0: lane has no ray
    V3 o{0, 0, 0}, d{0, 0, 0};
    float ix = 0, iy = 0, iz = 0, closest = 0;
    bool finite_inv = true;
    bool wave_nonfinite = false;        // some lane's ray has an infinite 1/d component (set at refill)
    int index = -1, sp = 0;
    uint32_t ref = 0;
    int ti = 0, te = 0;                 // the lane is in a leaf while ti < te
    unsigned pn = 0, iv = 0, tt = 0, nlive = 0;
#ifdef RT_PROFILE
    unsigned long long prof[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    // One internal node's step (both children's slabs, scene.cu:196-225) on the record {a, b, c, kids}:
    // pushes the near child when both are hit, enters the next one; returns whether the lane needs
    // its next node from the stack.
    auto node_step = [&](float4 a, float4 b, float4 c, uint2 kids) -> bool {
        if (COUNT) iv++;
        float t0, t1;
        bool h0, h1;
        slab_pair(a, b, c, o, ix, iy, iz, closest, h0, h1, t0, t1);
        if (__builtin_expect(wave_nonfinite, 0)) {
            // some lane's 1/d has an infinite component (0 * inf may give NaN): the literal
            // per-axis fold for those lanes
            float u0, u1;
            const bool g0 = slab(a.x, a.z, b.x, b.z, c.x, c.z, o, ix, iy, iz, closest, u0);
            const bool g1 = slab(a.y, a.w, b.y, b.w, c.y, c.w, o, ix, iy, iz, closest, u1);
            if (!finite_inv) { h0 = g0; h1 = g1; t0 = u0; t1 = u1; }
        }
        // The reference pushes the hit children near then far (scene.cu:204-225) and pops the
        // top: with both hit the far child is next and the near one stays on the stack; with
        // one hit that one is next.  Next is entered unless its entry distance >= closest.
        // (one predicate picks both children, logical not bitwise predicates: A/B 7.50-7.65 ->
        // 7.28-7.37 ms/pass with the refill-time non-finite ballot above)
        const bool both = h0 && h1, any = h0 || h1;
        // next = child 1 iff it is the far child of two hits (t0 < t1; a tie makes child 1 the
        // near one) or the only hit; the other child is the near one, pushed when both hit
        const bool sel1 = h1 && (!h0 || t0 < t1);
        const uint32_t next_ref = sel1 ? kids.y : kids.x, near_ref = sel1 ? kids.x : kids.y;
        const float next_t = sel1 ? t1 : t0, near_t = sel1 ? t0 : t1;
        // the near child is written either way (above the top when not pushed; entry
        // kStackLds is a scratch slot), so the push needs no branch
        col[min(sp, kStackLds) * kBlock] = make_uint2(near_ref, __float_as_uint(near_t));
        if (__builtin_expect(both && sp >= kStackLds, 0)) {
            overflow[(sp - kStackLds) * lanes + overflow_lane()] = near_ref;
            overflow[dist_half + (sp - kStackLds) * lanes + overflow_lane()] = __float_as_uint(near_t);
        }
        if (both) sp++;
        ref = any ? next_ref : ref;
        const bool descend = any && !(next_t >= closest);
        bool need = !descend;
        if (descend) {
            if (COUNT) pn++;
            if (ref & kLeaf) {
                leaf_range(S, ref, ti, te);
                need = ti == te;
            }
        }
        return need;
    };
    // Pop to the next entry nearer than closest (scene.cu:147-152), the per-entry decisions as
    // selects: the LDS entry is read for every popping lane (an empty stack reads entry 0,
    // unused), only the rare overflow-stack entries and big-leaf ranges take a branch (round 3:
    // the nested if/else form cost ~27 SALU + 7 branches more per loop body).
    auto pop_loop = [&](bool need) {
        while (need) {
            PROF(10, 1);
            const bool empty = sp == 0;
            sp = empty ? 0 : sp - 1;
            uint2 e = col[min(sp, kStackLds) * kBlock];
            // opaque: keeps the LDS read an LDS read (the compiler would otherwise fold it and the
            // rare overflow read below into one flat load through a selected pointer)
            asm volatile("" : "+v"(e.x), "+v"(e.y));
            if (__builtin_expect(__ballot(sp >= kStackLds) != 0, 0)) {   // wave-uniform, rare
                if (sp >= kStackLds) {
                    e.x = overflow[(sp - kStackLds) * lanes + overflow_lane()];
                    e.y = overflow[dist_half + (sp - kStackLds) * lanes + overflow_lane()];
                }
            }
            const bool take = !empty && !(__uint_as_float(e.y) >= closest);
            slot = empty ? -2 - slot : slot;   // done; {closest, index} stored at the next refill or at exit
            ref = take ? e.x : ref;
            if (COUNT) pn += take ? 1u : 0u;
            const bool leaf = take && (ref & kLeaf);
            if (__builtin_expect(leaf && (ref & kBigLeaf), 0)) {
                leaf_range(S, ref, ti, te);
            } else {
                ti = leaf ? (int)(ref & 0xFFFFFFu) : ti;
                te = leaf ? ti + (int)((ref >> 24) & 0x3Fu) : te;
            }
            need = !empty && (!take || (leaf && ti == te));
        }
    };
    // The result of slot s, whose ray this lane still holds: {closest, index}; VSLOT: the index, and the hit point
    // for a lane that hit (contraction is off: the two roundings per component of shade_from's no = o + closest * d).
    auto store_result = [&](int s) {
        if (VSLOT) {
            reinterpret_cast<int *>(hits)[s] = index;
            if (index != -1) {
                const V3 no = o + closest * d;
                float *p = hit_org + (size_t)s * 3;
                p[0] = no.x; p[1] = no.y; p[2] = no.z;
            }
        } else {
            hits[s] = make_float2(closest, __int_as_float(index));
        }
    };
    // The root's child-pair record is the same for every ray: read once into scalar registers, so
    // a refill runs its fresh lanes' root step without a memory round trip and they enter the loop
    // one level down (later bounces: ~1 of ~19 steps per ray).  Round 3, A/B on one box: teapot frame
    // 6.81 -> 6.67 ms/pass, driver-style 20 steps 7.05 -> 6.92, lamp 13.27 -> 12.90.  Also measured:
    // the root's two children's records in scalar registers too (a second step at refill; 6.71, 6.86,
    // 12.95: no better) and an LDS copy of the top 3-5 levels (breadth-first records) stepped at
    // refill until no lane stands on one (7.00-7.04, 7.15-7.19, 12.86-12.98: the refill's record
    // registers push the kernel into scratch spills); revision b72e94c has both (RT_ROOT_STEP=2/3).
    const bool root_internal = !(S.root_ref & kLeaf);
    float4 ra{0, 0, 0, 0}, rb{0, 0, 0, 0}, rc{0, 0, 0, 0};
    uint2 rk{0, 0};
    if (root_internal) {
        const float4 *rr = S.nodes + (size_t)S.root_ref * 4;
        const float4 x0 = rr[0], x1 = rr[1], x2 = rr[2];
        const uint2 k = *reinterpret_cast<const uint2 *>(rr + 3);
#define RT_U(v) __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)))
        ra = make_float4(RT_U(x0.x), RT_U(x0.y), RT_U(x0.z), RT_U(x0.w));
        rb = make_float4(RT_U(x1.x), RT_U(x1.y), RT_U(x1.z), RT_U(x1.w));
        rc = make_float4(RT_U(x2.x), RT_U(x2.y), RT_U(x2.z), RT_U(x2.w));
#undef RT_U
        rk = make_uint2(__builtin_amdgcn_readfirstlane(k.x), __builtin_amdgcn_readfirstlane(k.y));
    }
    while (true) {
        // ---- refill idle lanes (wave-uniform control flow)
        unsigned long long idle = __ballot(slot < 0);
        if (!exhausted && __popcll(idle) >= (FIRST ? kRefillFirst : kRefill)) {
            PROF(6, 1);
            // results of the lanes that finished since the last refill (slot -2 - s: done with slot s),
            // stored now: on gfx9 a store counts in vmcnt, so a store issued mid-loop made the next
            // step's vmcnt(0) waits (before its record loads, before an LDS pop) wait for the write as
            // well; here the stores overlap the refill's own ray loads (A/B 7.13 -> 7.00 ms/pass)
            if (slot <= -2) {
                store_result(-2 - slot);
                slot = -1;
            }
            bool fresh = false;
            // one turn hands slots to the idle lanes; VSLOT takes further turns while lanes drew dead slots
            do {
                bool got = false;       // VSLOT: the lane took a slot in this turn
                while (idle && !exhausted) {
                    if (q_next >= q_end) {
                        const uint32_t seg_lo = (uint32_t)(((uint64_t)L * shard) / kQueues);
                        const uint32_t seg_hi = (uint32_t)(((uint64_t)L * (shard + 1)) / kQueues);
                        uint32_t c = 0;
                        if (lane_id() == 0) c = atomicAdd(queue + shard * kQueueStride, chunk);
                        c = __builtin_amdgcn_readfirstlane(__shfl(c, 0)) + seg_lo;
                        if (c >= seg_hi) {
                            shard = (shard + 1) % kQueues;
                            if (++tried == kQueues) exhausted = true;
                            continue;
                        }
                        q_next = c;
                        q_end = min(c + chunk, seg_hi);
                    }
                    const uint32_t avail = q_end - q_next;
                    const uint32_t r = rank_below(idle);
                    const bool take = slot < 0 && r < avail;
                    const unsigned long long took = __ballot(take);
                    if (take) { slot = (int)(q_next + r); fresh = true; got = true; }
                    q_next += (uint32_t)__popcll(took);
                    idle &= ~took;
                }
                if (VSLOT) {            // a ray that ended at bounce 0: the lane takes another slot
                    if (got && slot_bkt[slot] == kDead) { slot = -1; fresh = false; }
                    idle = __ballot(slot < 0);
                }
            } while (VSLOT && idle && !exhausted);
            if (fresh) {
                {
                    nlive++;
                    if (FIRST) {
                        o = S.cam;
                        d = primary_dir(S, (int)first_ray<FIRST>(pa.map, (uint32_t)slot), pa);
                    } else if (VSLOT) {
                        // the slim bounce-0 hand-over (shade_kernel<.., SLIM>): 16-B records {d, t0}; the origin is
                        // bounce 0's no = o + closest * d with o = cam and d = the slot's primary ray (shade_from)
                        const float4 r = geo[slot];
                        o = S.cam + r.w * primary_dir(S, slot, pa);
                        d = v3(r.x, r.y, r.z);
                    } else {
                        const float4 *rp = geo + (size_t)slot * 2;   // ray state is in slot order
                        const float4 r0 = rp[0];
                        const float2 r1 = *reinterpret_cast<const float2 *>(rp + 1);
                        o = v3(r0.x, r0.y, r0.z);
                        d = v3(r0.w, r1.x, r1.y);
                    }
                    ix = 1 / d.x; iy = 1 / d.y; iz = 1 / d.z;
                    finite_inv = __builtin_isfinite(ix) && __builtin_isfinite(iy) && __builtin_isfinite(iz);

                    closest = 1e30f;
                    index = -1;
                    for (int i = 0; i < S.sphere_count; i++) {
                        const float4 sph = S.spheres[i];
                        float t;
                        if (ray_sphere(o, d, v3(sph.x, sph.y, sph.z), sph.w, closest, t)) { closest = t; index = i; }
                    }
                    ref = S.root_ref;   // root is popped with distance 0 < closest
                    sp = 0;
                    if (COUNT) pn++;
                    ti = te = 0;
                    if (ref & kLeaf) {
                        leaf_range(S, ref, ti, te);
                        if (ti == te) {  // no triangles at all: spheres only
                            store_result(slot);
                            slot = -1;
                        }
                    }
                }
            }
            // one ballot per refill instead of one per node step; the flag stays set until the next
            // refill even if that ray has finished (the per-lane fold below is exact for every lane)
            wave_nonfinite = __ballot(slot >= 0 && !finite_inv) != 0;
            if (root_internal && __ballot(fresh && slot >= 0)) {   // the fresh lanes' root step
                bool need = false;
                if (fresh && slot >= 0) need = node_step(ra, rb, rc, rk);
                pop_loop(need);
            }
        }
        if (!__ballot(slot >= 0)) {
            if (exhausted) break;
            PROF(7, 1);
            continue;
        }
#ifdef RT_PROFILE
        {
            const unsigned long long act = __ballot(slot >= 0), lf = __ballot(slot >= 0 && ti < te);
            PROF(0, 1); PROF(1, __popcll(act)); PROF(2, __popcll(lf));
            PROF(3, lf != 0); PROF(4, (act & ~lf) != 0);
            const bool mixed = lf != 0 && (act & ~lf) != 0;
            PROF(8, mixed);
            if (mixed) PROF(9, min(__popcll(lf), __popcll(act & ~lf)));
            // steps whose active lanes all read one record (a scalar load could serve them), and
            // steps where at least 3/4 of the active lanes read the first active lane's record
            const uintptr_t ra = slot >= 0 ? (uintptr_t)(ti < te ? S.tris + (size_t)ti * 3 : S.nodes + (size_t)ref * 4) : 0;
            const int first = __builtin_ctzll(act);
            const uintptr_t r0 = ((uintptr_t)__shfl((unsigned)(ra >> 32), first) << 32) | __shfl((unsigned)ra, first);
            const unsigned long long same = __ballot(slot >= 0 && ra == r0);
            PROF(12, same == act);
            PROF(13, 4 * __popcll(same) >= 3 * __popcll(act));
        }
#endif
        if (slot < 0) continue;
        // ---- one step: a single triangle test of the current leaf, or one internal node
        // (both children's slabs).  One triangle per step keeps the leaf branch as short as the
        // internal one, so lanes at leaves and lanes at internal nodes share a step at ~50 %
        // SIMD efficiency instead of the whole wave running a leaf's worth of triangle tests.
        // The node/triangle visit order per lane is the reference's (scene.cu:145-238).
        // Both kinds of step read their record through the same loads (a triangle's p1 e1 e2, or a
        // node's interleaved child bounds and child refs), issued before the branch, so a step
        // costs one memory round trip whatever mix of leaf and internal lanes the wave holds.
        bool need = false;              // the lane needs the next node from its stack
        const bool in_leaf = ti < te;
        const float4 *rec = in_leaf ? S.tris + (size_t)ti * 3 : S.nodes + (size_t)ref * 4;
        // The child refs are loaded by node lanes only: a leaf lane's step is 3 L1 accesses instead
        // of 4, and the gather rate of L1 accesses bounds the heavy bounces (tools/experiments/
        // gather_bench.hip).  Round 4, A/B on one box: teapot 20 steps 6.89 -> 6.81, full frame
        // 6.71 -> 6.61, lamp 12.94 -> 12.70 ms/pass (docs/history/profiles/r04/ab_kids.txt).  Loading only e2.z
        // for leaf lanes as well (a divergent one-dword load) was slower: 7.74.
        const float4 a = rec[0], b = rec[1], c = rec[2];
        uint2 kids = make_uint2(0, 0);
        if (!in_leaf) kids = *reinterpret_cast<const uint2 *>(rec + 3);
        if (in_leaf) {
            const float4 q0 = a, q1 = b;
            const float q2 = c.x;
            if (COUNT) tt++;
            float t;
            const bool hit =
                ray_triangle_flat(o, d, v3(q0.x, q0.y, q0.z), v3(q0.w, q1.x, q1.y), v3(q1.z, q1.w, q2), closest, t);
            closest = hit ? t : closest;
            index = hit ? S.sphere_count + ti : index;
            need = ++ti == te;
        } else {
            need = node_step(a, b, c, kids);
        }
#ifdef RT_PROFILE
        if (__ballot(need)) PROF(5, 1);
#endif
        pop_loop(need);
    }
    if (slot <= -2) store_result(-2 - slot);
    Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
    const unsigned long long nl = wave_sum(nlive);
    if (COUNT) {
        const unsigned long long a = wave_sum(pn), b = wave_sum(iv), t = wave_sum(tt);
        if (lane_id() == 0) {
            atomicAdd(&cs->pn, a);
            atomicAdd(&cs->iv, b);
            atomicAdd(&cs->tt, t);
            atomicAdd(&cs->st, nl * (unsigned long long)S.sphere_count);
        }
    }
    if (lane_id() == 0 && nl) atomicAdd(&cs->live, nl);
    if (tspan) {                        // the workgroup's last wave: one atomic per workgroup
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicMin(&tspan[blockIdx.x % kSpanSlots], t_start);
            atomicMax(&tspan[kSpanSlots + blockIdx.x % kSpanSlots], (unsigned long long)wall_clock64());
        }
    }
#ifdef RT_PROFILE
    prof[11] = wave_sum((unsigned)prof[10]);   // pop iterations summed over the lanes
    if (lane_id() == 0)
        for (int i = 0; i < 14; i++)
            if (i != 10) atomicAdd(&g_prof[FIRST ? 0 : 1][i], prof[i]);
#endif
}

// One ray's shading (scene.cu:376-485) at `slot`: environment lookup on a miss, otherwise
// emission + scatter.  Returns the new state; `ray` = the acc index (ray id or home index), kind = 0 miss,
// 1 triangle hit, 2 sphere hit.
struct Shaded {
    V3 no, nd, T;
    V3 C;                             // this bounce's radiance term as 0 + term (emission or sky times T)
    uint32_t ray;
    int kind;
    bool acc_holds;                   // acc[ray] holds the radiance of the earlier bounces
    uint32_t mat;                     // SLIM only: the hit's material index and whether scatter multiplied T by its
    bool spec;                        // spec (else its diffuse) albedo
    float t;                          // SLIM only: the hit's distance (no = cam + t * the primary direction)
};
constexpr uint32_t kSpecBit = 0x80;   // slim hand-over: Shaded::spec in a live bounce-0 bucket byte (buckets are 0..64)
// INLINE (scenes without triangles): the closest hit is the sphere loop (scene.cu:338-372),
// computed here instead of read from the trace kernel's output.
// A slot's coalesced inputs (hit record, ray id, seed slot, state), loaded apart from the shading.
// (Round 4 measured issuing the next round's inputs before shading this one, in the shade and the
// fused scatter-shade kernels: 72-90 VGPRs, no gain.)
struct ShadeIn {
    float2 h;
    uint32_t ray, seed;
    bool acc_holds;                   // acc[ray] holds the ray's radiance so far (kAccFlag in its rid)
    float4 r0, r1;
    float tz;
    const float *org;                 // shade_from<.., LEAN>: where a hit's point stands (3 floats); r0.xyz is unused
};
template <bool SORTED, int FIRST, bool INLINE>
__device__ __forceinline__ ShadeIn shade_in(const PassArgs &pa, int slot, const float4 *__restrict__ geo,
                                            const float *__restrict__ tz, const uint32_t *__restrict__ rid,
                                            const float2 *__restrict__ hits, const uint32_t *__restrict__ seed_of) {
    ShadeIn in{};
    // The seed follows the reference's slot (raytracing.cu:89): the position with sort on;
    // with sort off a ray keeps its original slot, which is its ray id.  At bounce 0 the
    // reference slot is the ray id (pixel-tile renders: mapped from this tile's slot).
    const uint32_t ray0 = first_ray<FIRST>(pa.map, (uint32_t)slot);   // bounce 0 only
    // Pixel tiles with the reorder on: the global post-sort slot, carried per ray (seed_of).
    // the ray id goes out with the state loads (issued at its use, it was a round trip of its own
    // between the shading and the stores)
    const uint32_t rv = FIRST ? (FIRST == 2 ? ray0 : (uint32_t)slot) : rid[slot];
    in.ray = rv & ~kAccFlag;
    in.acc_holds = (rv & kAccFlag) != 0;
    in.seed = (!FIRST && seed_of) ? seed_of[slot] : (SORTED || FIRST) ? (FIRST == 2 ? ray0 : (uint32_t)slot) : in.ray;
    if (!INLINE) in.h = hits[slot];
    if (!FIRST) {
        in.r0 = geo[(size_t)slot * 2];
        in.r1 = geo[(size_t)slot * 2 + 1];
        in.tz = tz[slot];
    }
    return in;
}
// SLIM (bounce 0 of the virtual reorder's slim hand-over): also returns the hit's material index and albedo choice.
// LEAN (bounce 1 of it, shade_rank_kernel): the trace kernel wrote the hit point (trace_kernel<.., VSLOT>), read at
// in.org by the lanes that hit, with the hit's other records; neither the ray's origin nor the hit's distance enters.
template <bool SORTED, int FIRST, bool INLINE = false, bool SLIM = false, bool LEAN = false>
__device__ __forceinline__ Shaded shade_from(const DevScene &S, const PassArgs &pa, int slot, const ShadeIn &in,
                                             uint32_t seed_term) {
    static_assert(!SLIM || FIRST == 1, "the slim hand-over leaves bounce 0, where T enters as (1,1,1)");
    static_assert(!LEAN || (!FIRST && !INLINE), "the lean result is the bounce-1 trace kernel's");
    uint32_t mat = 0;
    bool spec = false;
    Rng rng = pcg_seed(in.seed * 4137874753u + seed_term);
    float closest = in.h.x;
    int index = __float_as_int(in.h.y);
    const uint32_t ray_id = in.ray;
    V3 o, d, T;
    V3 C = v3(0, 0, 0);                 // the ray's radiance lives in acc[ray] (or is 0): only this bounce's term
    if (FIRST) {
        o = S.cam;
        d = primary_dir(S, (int)(FIRST == 2 ? in.ray : (uint32_t)slot), pa);
        // T is laundered through an empty asm: with T a compile-time (1,1,1) the gfx950
        // backend dropped T.xy on the dielectric-reflect path of scatter (ROCm 7.2 clang;
        // T.xy came out as stale registers while T.z was right).  Keeping T opaque gives the
        // same code shape as bounces >= 1, which is parity-clean.
        float tx = 1.f, ty = 1.f, tz = 1.f;
        asm volatile("" : "+v"(tx), "+v"(ty), "+v"(tz));
        T = v3(tx, ty, tz);
    } else {
        o = v3(in.r0.x, in.r0.y, in.r0.z);
        d = v3(in.r0.w, in.r1.x, in.r1.y);
        T = v3(in.r1.z, in.r1.w, in.tz);
    }
    if (INLINE) {
        closest = 1e30f;
        index = -1;
        for (int i = 0; i < S.sphere_count; i++) {
            const float4 sph = S.spheres[i];
            float t;
            if (ray_sphere(o, d, v3(sph.x, sph.y, sph.z), sph.w, closest, t)) { closest = t; index = i; }
        }
    }
    V3 no = o, nd = d;
    if (index == -1) {
        C = C + sky_color(S.env, S.env_w, S.env_h, d) * T;
        T = v3(0, 0, 0);
    } else {
        // The material index and the surface record (sphere, or the triangle quad holding the
        // normal) depend only on `index`: one round trip for both, through one selected pointer,
        // then one for the material (three before: record, index, material)
        // (the empty asm statements keep each record one 16-B load: the compiler otherwise splits
        // off the components only one branch reads -- a sphere's centre.x, the material's metal --
        // and issues them later, each a round trip of its own)
        const bool sphere = index < S.sphere_count;
        const uint32_t mi = S.mat_idx[index];
        float4 q = *(sphere ? S.spheres + index : S.tris + (size_t)(index - S.sphere_count) * 3 + 2);
        if (LEAN) no = v3(in.org[0], in.org[1], in.org[2]);   // the same round trip
        asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));
        if (!LEAN) no = o + closest * d;
        const V3 normal = sphere ? (1 / q.w) * (no - v3(q.x, q.y, q.z)) : v3(q.y, q.z, q.w);
        const float4 *mp = S.mats + (size_t)mi * 3;
        float4 m0 = mp[0], m1 = mp[1], m2 = mp[2];
        asm volatile("" : "+v"(m0.x), "+v"(m0.y), "+v"(m0.z), "+v"(m0.w), "+v"(m1.x), "+v"(m1.y), "+v"(m1.z),
                          "+v"(m1.w), "+v"(m2.x), "+v"(m2.y), "+v"(m2.z), "+v"(m2.w));
        const Mat m{v3(m0.x, m0.y, m0.z), m0.w, v3(m1.x, m1.y, m1.z), m1.w, v3(m2.x, m2.y, m2.z), m2.w};
        const bool took_spec = scatter(d, normal, m, rng, T, C, nd);
        if (SLIM) {                     // T entered as (1,1,1) and left as 1 * m.spec or 1 * m.diffuse
            spec = took_spec;
            mat = mi;
        }
    }
    return Shaded{no, nd, T, C, ray_id, index == -1 ? 0 : (index < S.sphere_count ? 2 : 1), in.acc_holds, mat, spec,
                  closest};
}
template <bool SORTED, int FIRST, bool INLINE = false, bool SLIM = false>
__device__ __forceinline__ Shaded shade_one(const DevScene &S, const PassArgs &pa, int slot,
                                            const float4 *__restrict__ geo, const float *__restrict__ tz,
                                            const uint32_t *__restrict__ rid, const float2 *__restrict__ hits,
                                            uint32_t seed_term, const uint32_t *__restrict__ seed_of = nullptr) {
    return shade_from<SORTED, FIRST, INLINE, SLIM>(S, pa, slot,
                                                   shade_in<SORTED, FIRST, INLINE>(pa, slot, geo, tz, rid, hits, seed_of),
                                                   seed_term);
}
// A nonzero radiance term of this bounce: some component with nonzero magnitude bits (adding +-0 to the
// radiance so far never changes it: that sum starts at +0 and so is never -0).
__device__ __forceinline__ bool has_radiance(V3 c) {
    return ((__float_as_uint(c.x) | __float_as_uint(c.y) | __float_as_uint(c.z)) & 0x7fffffffu) != 0;
}

// Shading for the live slots (scene.cu:376-485): environment lookup on a miss, otherwise
// emission + scatter; then the new ray state and its reorder bucket.  One lane per slot.
// Ray state lives in slot order (the reorder moves it), so every access here is coalesced.  A
// ray's radiance goes to acc[ray id] (pixel-major, what accumulation reads) when it terminates
// or after the last bounce.
__device__ __forceinline__ unsigned long long match_bucket(uint32_t b, bool valid);

// counts (or null): the reorder's per-tile bucket histogram (sort_hist_kernel's output) counted here
// as the buckets are made, so the bounce needs no histogram launch and no second read of the
// buckets; the blocks then walk whole reorder tiles instead of 256-slot strides.
#ifndef RT_SHADE_WPE
// waves-per-SIMD floor for shade_kernel: its scalar registers alone held it at 7 (101-106 SGPRs); at 8 (round 5,
// A/B after the slim state): frame -0.9 %, lamp -0.5 %, cornell_plus -1.8 %, 20 steps +-0.3 %
#define RT_SHADE_WPE 8
#endif
#ifndef RT_REPLAY_WPE
// the same for the fused replay (sort_scatter_shade_kernel): 6 waves by its 75 VGPRs; at 8 (a 20-B spill; round 5 A/B):
// teapot 20 steps -2.1 %, frame -0.5 %, cornell_plus -1.5 %, spheres +-0
#define RT_REPLAY_WPE 8
#endif
#if RT_REPLAY_WPE > 0
#define RT_REPLAY_ATTR __attribute__((amdgpu_waves_per_eu(RT_REPLAY_WPE, RT_REPLAY_WPE)))
#else
#define RT_REPLAY_ATTR
#endif
#if RT_SHADE_WPE > 0
#define RT_SHADE_ATTR __attribute__((amdgpu_waves_per_eu(RT_SHADE_WPE, RT_SHADE_WPE)))
#else
#define RT_SHADE_ATTR
#endif
// SLIM (bounce 0 of the virtual reorder, rt_renderer::vre): a surviving ray hands over 19 B instead of 41.  geo holds
// one 16-B record {d, t0} per slot (t0: this bounce's hit distance; the new origin cam + t0 * primary_dir(slot) is
// recomputed by the one kernel that needs it, the bounce-1 trace), tz holds one u16 per slot, the hit's material
// index, and bit 7 of the live bucket byte (kSpecBit) says which albedo scatter took; T and the rid flag are functions
// of those two (shade_rank_kernel rebuilds them), so no T and no rid is written.
template <bool SORTED, bool COUNT, int FIRST, bool FUSED, bool INLINE, bool SLIM = false>
__global__ __launch_bounds__(kBlock) RT_SHADE_ATTR void shade_kernel(DevScene S, PassArgs pa, float4 *__restrict__ geo,
                                                       float *__restrict__ tz, uint32_t *__restrict__ rid,
                                                       float4 *__restrict__ acc, uint8_t *__restrict__ bkt,
                                                       const uint32_t *__restrict__ live_count,
                                                       const float2 *__restrict__ hits, uint32_t seed_term, int last,
                                                       Counters *__restrict__ ctr,
                                                       const uint32_t *__restrict__ seed_of = nullptr,
                                                       uint32_t *__restrict__ counts = nullptr, int tiles = 0,
                                                       int home = 0) {
    // home (bounce 0 of a sorted render whose bounce-0 reorder is the fused replay): a surviving ray's radiance
    // lives at its home index (sort_scatter_shade_kernel), so its term here is left to the replay
    const int L = (int)__builtin_amdgcn_readfirstlane(*live_count);
    unsigned hit = 0, miss = 0, hit_sphere = 0;
    // one slot's shading and new state; returns its bucket
    auto shade_slot = [&](int slot) -> uint32_t {
        const Shaded sh = shade_one<SORTED, FIRST, INLINE, SLIM>(S, pa, slot, geo, tz, rid, hits, seed_term, seed_of);
        const V3 no = sh.no, nd = sh.nd, T = sh.T;
        miss += sh.kind == 0;
        hit += sh.kind != 0;
        hit_sphere += sh.kind == 2;
        const bool dead = is_black(T);
        if (SLIM && !dead && !last) {
            geo[slot] = make_float4(nd.x, nd.y, nd.z, sh.t);
            reinterpret_cast<uint16_t *>(tz)[slot] = (uint16_t)sh.mat;
        }
        if (!SLIM && !FUSED && !dead && !last) {     // a terminated ray's geometry is never read again
            geo[(size_t)slot * 2] = make_float4(no.x, no.y, no.z, nd.x);
            geo[(size_t)slot * 2 + 1] = make_float4(nd.y, nd.z, T.x, T.y);
            tz[slot] = T.z;
        }
        // The radiance (the reference's `collected`, scene.cu:383,417) is not carried with the ray: a bounce's
        // term goes to acc[ray id] when it is nonzero or the ray ends, added to what acc holds (kAccFlag)
        // in the reference's order -- the same sums, 12 B less state per live ray in every shade and reorder.
        const bool term = has_radiance(sh.C);
        if (dead || last || (term && !(FIRST && home))) {
            V3 C = sh.C;
            const uint32_t dst = sh.ray;      // the ray id, or (Renderer::home) its home index
            if (sh.acc_holds) {
                const float4 a = acc[dst];
                C = v3(a.y, a.z, a.w) + sh.C;
            }
            typedef float f4v __attribute__((ext_vector_type(4)));
            if (dead || last)
                // scattered 16-B writes (rays terminate in sorted, not ray-id, order): nontemporal, so
                // the radiance lines do not displace the scene records the trace kernels re-read from
                // L2 (round 4: later-bounce shade 1.73 -> 1.45 ms alone, teapot 20 steps 6.73 -> 6.41
                // ms/pass; the same hint on the coalesced ray-state, hit and bucket traffic: +1-2 %)
                __builtin_nontemporal_store(f4v{T.z, C.x, C.y, C.z}, reinterpret_cast<f4v *>(acc + dst));
            else
                acc[dst] = make_float4(T.z, C.x, C.y, C.z);   // read back at a later bounce
        }
        // the flag rides in the ray id, which the reorder moves (at bounce 0 written for every ray: the
        // reorder's bounce-0 scatter reads it there; FUSED: the replay sets it)
        if (!SLIM && !FUSED && !dead && !last && (FIRST || (term && !sh.acc_holds)))
            rid[slot] = sh.ray | (term || sh.acc_holds ? kAccFlag : 0u);
        const uint32_t bk = dead ? kDead : (SORTED ? bucket_of(no, nd, S.min_coord, S.inv_dim) : 0u);
        if (!last) bkt[slot] = (uint8_t)(bk | (SLIM && !dead && sh.spec ? kSpecBit : 0u));
        return bk;                      // without kSpecBit: the histogram counts buckets
    };
    if (counts && !last) {
        __shared__ uint32_t h[kBuckets];
        const int R = tile_rounds(L), span = kBlock * R;
        for (int tile = blockIdx.x; tile * span < L; tile += gridDim.x) {
            for (int b = threadIdx.x; b < kBuckets; b += kBlock) h[b] = 0;
            __syncthreads();
            const int base = tile * span;
            const int rounds = min(R, (L - base + kBlock - 1) / kBlock);   // block-uniform: the last tile is short
            for (int r = 0; r < rounds; r++) {
                const int slot = base + r * kBlock + threadIdx.x;
                const bool valid = slot < L;
                const uint32_t bk = valid ? shade_slot(slot) : 0u;
                const unsigned long long peers = match_bucket(bk, valid);
                if (valid && rank_below(peers) == 0) atomicAdd(&h[bk], (uint32_t)__popcll(peers));
            }
            __syncthreads();
            for (int b = threadIdx.x; b < kBuckets; b += kBlock) counts[(size_t)b * tiles + tile] = h[b];
            __syncthreads();
        }
    } else {
        for (int base = blockIdx.x * kBlock; base < L; base += gridDim.x * kBlock) {
            const int slot = base + threadIdx.x;
            if (slot < L) (void)shade_slot(slot);
        }
    }
    if (INLINE) {   // no trace kernel ran: the live segments (and the root pop, the sphere tests) count here
        Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
        const unsigned long long nl = wave_sum(hit + miss);
        if (lane_id() == 0 && nl) {
            atomicAdd(&cs->live, nl);
            if (COUNT) {
                atomicAdd(&cs->pn, nl);
                atomicAdd(&cs->st, nl * (unsigned long long)S.sphere_count);
            }
        }
    }
    if (COUNT) {
        Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
        const unsigned long long h = wave_sum(hit), m = wave_sum(miss), hs = wave_sum(hit_sphere);
        if (lane_id() == 0 && (h | m)) {
            atomicAdd(&cs->hits, h);
            atomicAdd(&cs->misses, m);
            atomicAdd(&cs->hits_sphere, hs);
        }
    }
}

__global__ void fill_live_kernel(uint32_t *__restrict__ live, uint32_t n, int count, uint32_t *__restrict__ queue,
                                 unsigned long long *__restrict__ tspan) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) live[i] = n;
    for (int k = i; k < count * kQueues * kQueueStride; k += blockDim.x) queue[k] = 0;
    if (tspan)
        for (int k = i; k < kSpanWords * count; k += blockDim.x) tspan[k] = (k % kSpanWords) >= kSpanSlots ? 0ull : ~0ull;
}


// ---------------------------------------------------------------- stable 65-bucket reorder
// Equivalent to cub::DeviceRadixSort::SortPairs on the reference keys (raytracing.cu:238-247).
// Peers = lanes of the wave holding the same bucket, from seven 64-lane ballots.
__device__ __forceinline__ unsigned long long match_bucket(uint32_t b, bool valid) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 7; bit++) {
        const unsigned long long m = __ballot((b >> bit) & 1u);
        peers &= ((b >> bit) & 1u) ? m : ~m;
    }
    return peers;
}

// run[b] = the pass's live rays in buckets < b + bucket b's rays in tiles before `tile`: the first
// wave loads the totals and offsets of the 65 buckets at once and prefix-sums the totals with a
// wave scan (one thread walking the buckets paid ~65 dependent scalar loads per tile).
__device__ __forceinline__ void bucket_runs(uint32_t *run, const uint32_t *__restrict__ offsets,
                                            const uint32_t *__restrict__ totals, int tiles, int tile) {
    static_assert(kBuckets == 65 && kDead == 64, "buckets 0..63 in one wave, the terminated bucket after them");
    if (threadIdx.x < 64) {
        const int b = (int)threadIdx.x;
        const uint32_t t = totals[b];
        uint32_t x = t;                 // inclusive scan of the totals over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (b >= off) x += y;
        }
        run[b] = x - t + offsets[(size_t)b * tiles + tile];
        if (b == 63) run[kDead] = x + offsets[(size_t)kDead * tiles + tile];
    }
}

// Per-tile bucket counts, written bucket-major: counts[b * tiles + tile].
__global__ __launch_bounds__(kBlock) void sort_hist_kernel(const uint8_t *__restrict__ bkt,
                                                           const uint32_t *__restrict__ live_count, int tiles,
                                                           uint32_t *__restrict__ counts) {
    const int n = (int)*live_count;
    const int R = tile_rounds(n), span = kBlock * R;
    __shared__ uint32_t h[kBuckets];
    // tile-stride: the grid is capped (the live prefix shrinks bounce by bounce; a block per
    // possible tile would dispatch thousands of empty workgroups in the tail bounces)
    for (int tile = blockIdx.x; tile * span < n; tile += gridDim.x) {
        for (int b = threadIdx.x; b < kBuckets; b += kBlock) h[b] = 0;
        __syncthreads();
        const int base = tile * span;
        const int rounds = min(R, (n - base + kBlock - 1) / kBlock);   // block-uniform: the last tile is short
        for (int r0 = 0; r0 < rounds; r0 += 4) {   // four rounds' loads in flight, then their ranking
            uint32_t bv[4];
            bool vv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int item = base + (r0 + k) * kBlock + threadIdx.x;
                vv[k] = r0 + k < rounds && item < n;
                bv[k] = vv[k] ? bkt[item] : 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned long long peers = match_bucket(bv[k], vv[k]);
                if (vv[k] && rank_below(peers) == 0) atomicAdd(&h[bv[k]], (uint32_t)__popcll(peers));
            }
        }
        __syncthreads();
        for (int b = threadIdx.x; b < kBuckets; b += kBlock) counts[(size_t)b * tiles + tile] = h[b];
        __syncthreads();
    }
}

// One workgroup per bucket: exclusive scan of that bucket's tile counts + bucket total.
__global__ __launch_bounds__(kBlock) void sort_scan_kernel(const uint32_t *__restrict__ counts,
                                                           const uint32_t *__restrict__ live_count, int tiles_max,
                                                           uint32_t *__restrict__ offsets, uint32_t *__restrict__ totals,
                                                           uint32_t *__restrict__ live_next) {
    const uint32_t n = *live_count;
    const int tiles = tiles_of((int)n);
    __shared__ uint32_t wsum[kBlock / 64];
    __shared__ uint32_t carry;
    const int b = blockIdx.x;
    const uint32_t *in = counts + (size_t)b * tiles_max;
    uint32_t *out = offsets + (size_t)b * tiles_max;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int start = 0; start < tiles; start += kBlock) {
        const int t = start + threadIdx.x;
        const uint32_t v = t < tiles ? in[t] : 0u;
        uint32_t x = v;                                  // inclusive wave scan
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t pre = carry;
        for (int k = 0; k < wave; k++) pre += wsum[k];
        if (t < tiles) out[t] = pre + x - v;
        __syncthreads();
        if (threadIdx.x == kBlock - 1) carry = pre + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        totals[b] = carry;
        if (b == (int)kDead) *live_next = n - carry;   // rays still live after this bounce
    }
}

// Stable scatter: rounds of 256 consecutive slots; rank = earlier rounds + earlier waves +
// earlier lanes holding the same bucket.  Live rays move with their state (geometry, T/C, ray
// id) so that the next bounce reads them in slot order; terminated rays (bucket 64, last in the
// order) have already delivered their radiance and are dropped.  At bounce 0 slot = ray id.
template <int FIRST_SRC>
__global__ __launch_bounds__(kBlock) void sort_scatter_kernel(const uint8_t *__restrict__ bkt_in,
                                                              const float4 *__restrict__ geo_in,
                                                              const float *__restrict__ tz_in,
                                                              const uint32_t *__restrict__ rid_in,
                                                              const uint32_t *__restrict__ live_count, int tiles,
                                                              const uint32_t *__restrict__ offsets,
                                                              const uint32_t *__restrict__ totals,
                                                              float4 *__restrict__ geo_out, float *__restrict__ tz_out,
                                                              uint32_t *__restrict__ rid_out, SlotMap map,
                                                              const uint32_t *__restrict__ gslot_in = nullptr,
                                                              const uint32_t *__restrict__ newpos = nullptr,
                                                              uint32_t *__restrict__ gslot_out = nullptr) {
    // gslot_out (pixel tiles with the reorder on): each moved ray also carries its new global slot,
    // newpos[its old global slot] (old global slot at bounce 0: the ray index, map.ray(item))
    const int n = (int)*live_count;
    __shared__ uint32_t run[kBuckets];
    __shared__ uint32_t wcount[kBlock / 64][kBuckets];
    const int R = tile_rounds(n), span = kBlock * R;
    for (int tile = blockIdx.x; tile * span < n; tile += gridDim.x) {   // tile-stride (capped grid)
    bucket_runs(run, offsets, totals, tiles, tile);
    for (int k = threadIdx.x; k < (kBlock / 64) * kBuckets; k += kBlock) (&wcount[0][0])[k] = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    const int base = tile * span;
    const int rounds = min(R, (n - base + kBlock - 1) / kBlock);   // block-uniform: skips a short tile's empty rounds
    for (int r = 0; r < rounds; r++) {
        const int item = base + r * kBlock + threadIdx.x;
        const bool valid = item < n;
        const uint32_t b = valid ? bkt_in[item] : 0u;
        const bool move = valid && b != kDead;
        float4 g0 = make_float4(0, 0, 0, 0), g1 = g0;
        float t = 0;
        uint32_t id = 0;
        if (move) {                     // issued before the ranking so the loads overlap it
            g0 = geo_in[(size_t)item * 2];
            g1 = geo_in[(size_t)item * 2 + 1];
            t = tz_in[item];
            id = rid_in[item];          // bounce 0: written by the shade kernel (the ray index + kAccFlag)
        }
        uint32_t gs = 0;
        if (gslot_out && move) gs = newpos[FIRST_SRC ? first_ray<FIRST_SRC>(map, (uint32_t)item) : gslot_in[item]];
        const unsigned long long peers = match_bucket(b, valid);
        const uint32_t rank = rank_below(peers);
        if (valid && rank == 0) wcount[wave][b] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (move) {
            uint32_t pos = run[b] + rank;
            for (int k = 0; k < wave; k++) pos += wcount[k][b];
            geo_out[(size_t)pos * 2] = g0;
            geo_out[(size_t)pos * 2 + 1] = g1;
            tz_out[pos] = t;
            rid_out[pos] = id;
            if (gslot_out) gslot_out[pos] = gs;
        }
        __syncthreads();
        if (threadIdx.x < kBuckets) {
            uint32_t s = 0;
            for (int k = 0; k < kBlock / 64; k++) { s += wcount[k][threadIdx.x]; wcount[k][threadIdx.x] = 0; }
            run[threadIdx.x] += s;
        }
        __syncthreads();
    }
    }
}

// ---- pixel tiles with the reorder on: the global bucket array and the global rank
// Every live ray of this owner writes bucket + 1 at its global slot (bounce 0: its ray index) of
// two zeroed arrays: G, which the exchange sums over the owners, and L, this owner's own bytes
// (L[g] != 0 iff this owner holds global slot g), which the global ranking uses to write new
// positions only for this owner's slots.
__global__ __launch_bounds__(kBlock) void zero_bytes_kernel(uint8_t *__restrict__ g, uint8_t *__restrict__ l,
                                                            const uint32_t *__restrict__ count) {
    const uint32_t n = *count;
    const uint32_t n16 = n / 16;        // 16-B stores for the bulk (buffers are hipMalloc-aligned)
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n16; i += gridDim.x * kBlock) {
        reinterpret_cast<uint4 *>(g)[i] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4 *>(l)[i] = make_uint4(0, 0, 0, 0);
    }
    for (uint32_t i = n16 * 16 + blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) g[i] = l[i] = 0;
}
template <int FIRST>
__global__ __launch_bounds__(kBlock) void tile_bytes_kernel(const uint8_t *__restrict__ bkt, const uint32_t *__restrict__ live_count,
                                                            const uint32_t *__restrict__ gslot, SlotMap map,
                                                            uint8_t *__restrict__ g, uint8_t *__restrict__ l) {
    const uint32_t n = *live_count;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t s = FIRST ? map.ray(i) : gslot[i];
        const uint8_t v = (uint8_t)(bkt[i] + 1);
        g[s] = v;
        l[s] = v;
    }
}
// After the exchange G holds bucket + 1 for every global live slot.  A byte outside [1, 65] (a slot
// no owner wrote, or an exchange that did not sum) is counted in *bad and read as a terminated ray,
// so no bucket index ever leaves [0, 64]; the host fails the render.
__device__ __forceinline__ uint32_t exchanged_bucket(uint32_t v) { return (v >= 1 && v <= kBuckets) ? v - 1 : kDead; }

// Per-tile bucket counts of the exchanged global array (sort_hist_kernel on biased bytes).
__global__ __launch_bounds__(kBlock) void gsort_hist_kernel(const uint8_t *__restrict__ g,
                                                            const uint32_t *__restrict__ live_count, int tiles,
                                                            uint32_t *__restrict__ counts, uint32_t *__restrict__ bad) {
    const int n = (int)*live_count;
    const int R = tile_rounds(n), span = kBlock * R;
    __shared__ uint32_t h[kBuckets];
    uint32_t nbad = 0;
    for (int tile = blockIdx.x; tile * span < n; tile += gridDim.x) {
        for (int b = threadIdx.x; b < kBuckets; b += kBlock) h[b] = 0;
        __syncthreads();
        const int base = tile * span;
        const int rounds = min(R, (n - base + kBlock - 1) / kBlock);
        for (int r0 = 0; r0 < rounds; r0 += 4) {   // four rounds' loads in flight, then their ranking
            uint32_t vr[4];
            bool vv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int item = base + (r0 + k) * kBlock + threadIdx.x;
                vv[k] = r0 + k < rounds && item < n;
                vr[k] = vv[k] ? g[item] : 1u;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t b = exchanged_bucket(vr[k]);
                nbad += (vv[k] && !(vr[k] >= 1 && vr[k] <= kBuckets)) ? 1u : 0u;
                const unsigned long long peers = match_bucket(b, vv[k]);
                if (vv[k] && rank_below(peers) == 0) atomicAdd(&h[b], (uint32_t)__popcll(peers));
            }
        }
        __syncthreads();
        for (int b = threadIdx.x; b < kBuckets; b += kBlock) counts[(size_t)b * tiles + tile] = h[b];
        __syncthreads();
    }
    const unsigned long long s = wave_sum(nbad);
    if (lane_id() == 0 && s) atomicAdd(bad, (uint32_t)s);
}
// The stable sort's new position of this owner's live global slots (the scatter's ranking without
// the move): newpos[g] = slots of smaller buckets + earlier slots of the same bucket, written only
// where own[g] != 0 (the other owners' slots are ranked, not stored).
__global__ __launch_bounds__(kBlock) void sort_rank_kernel(const uint8_t *__restrict__ g_in,
                                                           const uint8_t *__restrict__ own,
                                                           const uint32_t *__restrict__ live_count, int tiles,
                                                           const uint32_t *__restrict__ offsets,
                                                           const uint32_t *__restrict__ totals,
                                                           uint32_t *__restrict__ newpos) {
    const int n = (int)*live_count;
    __shared__ uint32_t run[kBuckets];
    __shared__ uint32_t wcount[kBlock / 64][kBuckets];
    const int R = tile_rounds(n), span = kBlock * R;
    for (int tile = blockIdx.x; tile * span < n; tile += gridDim.x) {
        bucket_runs(run, offsets, totals, tiles, tile);
        for (int k = threadIdx.x; k < (kBlock / 64) * kBuckets; k += kBlock) (&wcount[0][0])[k] = 0;
        __syncthreads();
        const int wave = threadIdx.x >> 6;
        const int base = tile * span;
        const int rounds = min(R, (n - base + kBlock - 1) / kBlock);   // block-uniform: skips a short tile's empty rounds
        for (int r = 0; r < rounds; r++) {
            const int item = base + r * kBlock + threadIdx.x;
            const bool valid = item < n;
            const uint32_t b = valid ? exchanged_bucket(g_in[item]) : 0u;
            const bool mine = valid && own[item] != 0;
            const unsigned long long peers = match_bucket(b, valid);
            const uint32_t rank = rank_below(peers);
            if (valid && rank == 0) wcount[wave][b] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (mine && b != kDead) {
                uint32_t pos = run[b] + rank;
                for (int k = 0; k < wave; k++) pos += wcount[k][b];
                newpos[item] = pos;
            }
            __syncthreads();
            if (threadIdx.x < kBuckets) {
                uint32_t s2 = 0;
                for (int k = 0; k < kBlock / 64; k++) { s2 += wcount[k][threadIdx.x]; wcount[k][threadIdx.x] = 0; }
                run[threadIdx.x] += s2;
            }
            __syncthreads();
        }
    }
}
// One wave that waits `ticks` of the device's constant-rate wall clock (a pass's staggered start,
// rt_renderer::run); bounded by its argument.
__global__ void delay_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

__global__ void set_count_kernel(uint32_t *__restrict__ dst, uint32_t v, const uint32_t *__restrict__ src) {
    if (threadIdx.x == 0) *dst = src ? *src : v;
}

// Fused reorder (shade_kernel<..., FUSED>): the shade kernel has written only the buckets (and the radiance of
// terminated rays); this replays the live rays' shading from the same inputs (shade_one is
// deterministic) and writes the new state straight to its sorted slot, saving the shade
// kernel's 48-B state write and the plain scatter's 48-B read per live ray.
template <bool SORTED, int FIRST, bool INLINE>
__global__ __launch_bounds__(kBlock) RT_REPLAY_ATTR void sort_scatter_shade_kernel(DevScene S, PassArgs pa,
                                                                    const uint8_t *__restrict__ bkt_in,
                                                                    const float4 *__restrict__ geo_in,
                                                                    const float *__restrict__ tz_in,
                                                                    const uint32_t *__restrict__ rid_in,
                                                                    const float2 *__restrict__ hits, uint32_t seed_term,
                                                                    const uint32_t *__restrict__ live_count, int tiles,
                                                                    const uint32_t *__restrict__ offsets,
                                                                    const uint32_t *__restrict__ totals,
                                                                    float4 *__restrict__ geo_out,
                                                                    float *__restrict__ tz_out,
                                                                    uint32_t *__restrict__ rid_out,
                                                                    float4 *__restrict__ acc = nullptr,
                                                                    uint32_t *__restrict__ home_of = nullptr,
                                                                    uint32_t home_base = 0) {
    // home_of (bounce 0, sort on): each surviving ray gets the home index home_base + its bounce-1 slot, which it
    // carries as its rid from now on: its radiance goes to acc[home], so the rays that terminate at bounce 1 -- most
    // of them -- store it coalesced (in ray-id order they were 16-B stores to scattered lines, each a partial HBM
    // line write).  A ray terminated at bounce 0 keeps acc[ray id] (written by the shade kernel, in slot = ray-id
    // order).  home_of[ray id] tells the accumulation where to read.
    const bool homes = FIRST == 1 && home_of != nullptr;
    const int n = (int)*live_count;
    __shared__ uint32_t run[kBuckets];
    __shared__ uint32_t wcount[kBlock / 64][kBuckets];
    const int R = tile_rounds(n), span = kBlock * R;
    for (int tile = blockIdx.x; tile * span < n; tile += gridDim.x) {
        bucket_runs(run, offsets, totals, tiles, tile);
        for (int k = threadIdx.x; k < (kBlock / 64) * kBuckets; k += kBlock) (&wcount[0][0])[k] = 0;
        __syncthreads();
        const int wave = threadIdx.x >> 6;
        const int base = tile * span;
        const int rounds = min(R, (n - base + kBlock - 1) / kBlock);   // block-uniform: skips a short tile's empty rounds
        for (int r = 0; r < rounds; r++) {
            const int item = base + r * kBlock + threadIdx.x;
            const bool valid = item < n;
            const uint32_t b = valid ? bkt_in[item] : 0u;
            const bool move = valid && b != kDead;
            Shaded sh{};
            if (move) sh = shade_one<SORTED, FIRST, INLINE>(S, pa, item, geo_in, tz_in, rid_in, hits, seed_term);
            const unsigned long long peers = match_bucket(b, valid);
            const uint32_t rank = rank_below(peers);
            if (valid && rank == 0) wcount[wave][b] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (move) {
                uint32_t pos = run[b] + rank;
                for (int k = 0; k < wave; k++) pos += wcount[k][b];
                geo_out[(size_t)pos * 2] = make_float4(sh.no.x, sh.no.y, sh.no.z, sh.nd.x);
                geo_out[(size_t)pos * 2 + 1] = make_float4(sh.nd.y, sh.nd.z, sh.T.x, sh.T.y);
                tz_out[pos] = sh.T.z;
                const uint32_t id = homes ? home_base + pos : sh.ray;
                if (homes) {
                    home_of[item] = id;
                    if (has_radiance(sh.C)) acc[id] = make_float4(sh.T.z, sh.C.x, sh.C.y, sh.C.z);
                }
                // the shade kernel (home: this kernel) has added a nonzero term into acc[id]: from now on acc holds the radiance
                rid_out[pos] = id | (has_radiance(sh.C) || sh.acc_holds ? kAccFlag : 0u);
            } else if (homes && valid) {
                home_of[item] = (uint32_t)item;
            }
            __syncthreads();
            if (threadIdx.x < kBuckets) {
                uint32_t s = 0;
                for (int k = 0; k < kBlock / 64; k++) { s += wcount[k][threadIdx.x]; wcount[k][threadIdx.x] = 0; }
                run[threadIdx.x] += s;
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- virtual bounce-0 reorder
// Sort on, untiled, a scene with triangles (rt_renderer::vre): the bounce-0 reorder moves nothing.  The reference's
// sorted position matters to a ray only as the seed of its next shading, and only the rays alive at bounce 2 need
// to stand in that order.  So bounce 0 shades once in place (shade_kernel<.., SLIM>, not FUSED: {d, t0}, the hit's
// material index, bucket + albedo bit, histogram, all in ray-id order) and sort_scan_kernel gives the bucket runs;
// bounce 1 traces over the ray-id slots (trace_kernel<.., VSLOT>) and shade_rank_kernel computes each live slot's
// sorted position with the scatter's own ranking, shades with that position as the seed, and moves only the survivors of bounce 1, to their
// sorted positions of the other buffer set.  The positions of the rays that ended at bounce 1 stay kDead holes of
// the bounce-1 bucket array (fill_dead_kernel), which the plain reorder that follows drops.

// The bucket bytes [0, *count) = kDead.
__global__ __launch_bounds__(kBlock) void fill_dead_kernel(uint8_t *__restrict__ bkt, const uint32_t *__restrict__ count) {
    const uint32_t n = *count;
    const uint32_t n16 = n / 16;        // 16-B stores for the bulk (the buffer is hipMalloc-aligned)
    const uint32_t w = kDead * 0x01010101u;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n16; i += gridDim.x * kBlock)
        reinterpret_cast<uint4 *>(bkt)[i] = make_uint4(w, w, w, w);
    for (uint32_t i = n16 * 16 + blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) bkt[i] = (uint8_t)kDead;
}

// Bounce 1 over the ray-id slots [0, *slot_count): the tiles and rounds of the bounce-0 histogram, the ranking of
// sort_scatter_kernel on the bounce-0 buckets, shade_kernel's shading and radiance rules with seed = the sorted
// position.  acc is indexed by ray id = slot, so a terminating ray's add is coalesced.
// Input is the slim hand-over of shade_kernel<.., SLIM>: the 16-B record {d, t0} at geo_in (d alone is read), the
// bounce-0 hit's material index mat_in[slot] and kSpecBit of the bucket byte; and the lean result of
// trace_kernel<.., VSLOT>: the hit index hit_idx[slot] and, read only by the lanes that hit, the hit point at
// hit_org + 3 * slot (shade_from<.., LEAN>).  The rest of the state is rebuilt from the material:
// T = 1 * (spec or diffuse albedo) is bounce 0's own multiply (scatter, T entering as the laundered (1,1,1)), and
// rid = slot | kAccFlag iff has_radiance(0 + emit * 1), bounce 0's own term.  Survivors leave with the full state.
template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_SHADE_ATTR void shade_rank_kernel(DevScene S, PassArgs pa,
                                                            const uint8_t *__restrict__ bkt_in,
                                                            const float4 *__restrict__ geo_in,
                                                            const uint16_t *__restrict__ mat_in,
                                                            const int *__restrict__ hit_idx,
                                                            const float *__restrict__ hit_org, uint32_t seed_term, int last,
                                                            const uint32_t *__restrict__ slot_count, int tiles,
                                                            const uint32_t *__restrict__ offsets,
                                                            const uint32_t *__restrict__ totals,
                                                            float4 *__restrict__ geo_out, float *__restrict__ tz_out,
                                                            uint32_t *__restrict__ rid_out, uint8_t *__restrict__ bkt_out,
                                                            float4 *__restrict__ acc, Counters *__restrict__ ctr) {
    const int n = (int)__builtin_amdgcn_readfirstlane(*slot_count);
    __shared__ uint32_t run[kBuckets];
    __shared__ uint32_t wcount[kBlock / 64][kBuckets];
    unsigned hit = 0, miss = 0, hit_sphere = 0;
    const int R = tile_rounds(n), span = kBlock * R;
    for (int tile = blockIdx.x; tile * span < n; tile += gridDim.x) {
        bucket_runs(run, offsets, totals, tiles, tile);
        for (int k = threadIdx.x; k < (kBlock / 64) * kBuckets; k += kBlock) (&wcount[0][0])[k] = 0;
        __syncthreads();
        const int wave = threadIdx.x >> 6;
        const int base = tile * span;
        const int rounds = min(R, (n - base + kBlock - 1) / kBlock);   // block-uniform: the last tile is short
        for (int r = 0; r < rounds; r++) {
            const int item = base + r * kBlock + threadIdx.x;
            const bool valid = item < n;
            const uint32_t byte = valid ? bkt_in[item] : 0u;
            const uint32_t b = byte & ~kSpecBit;   // a dead slot is plain kDead
            const bool move = valid && b != kDead;
            ShadeIn in{};
            float4 rec{};
            float4 alb{}, emi{};
            if (move) {                 // the loads overlap the ranking
                const float4 *mp = S.mats + (size_t)mat_in[item] * 3;
                in.h = make_float2(0.f, __int_as_float(hit_idx[item]));
                rec = geo_in[item];
                alb = mp[byte & kSpecBit ? 1 : 0];   // {specular, rough} or {diffuse, metal}
                emi = mp[2];
            }
            const unsigned long long peers = match_bucket(b, valid);
            const uint32_t rank = rank_below(peers);
            if (valid && rank == 0) wcount[wave][b] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (move) {
                uint32_t pos = run[b] + rank;
                for (int k = 0; k < wave; k++) pos += wcount[k][b];
                // as in shade_from: the 1 stays opaque, so both products are bounce 0's literal multiplies
                float one = 1.f;
                asm volatile("" : "+v"(one));
                const V3 ones = v3(one, one, one);
                const V3 T0 = ones * v3(alb.x, alb.y, alb.z);
                in.r0 = make_float4(0.f, 0.f, 0.f, rec.x);
                in.r1 = make_float4(rec.y, rec.z, T0.x, T0.y);
                in.tz = T0.z;
                in.org = hit_org + (size_t)item * 3;
                in.ray = (uint32_t)item;
                in.acc_holds = has_radiance(v3(0, 0, 0) + v3(emi.x, emi.y, emi.z) * ones);
                in.seed = pos;          // the reference's slot of this ray at bounce 1 (raytracing.cu:89)
                const Shaded sh = shade_from<true, 0, false, false, true>(S, pa, item, in, seed_term);
                const V3 no = sh.no, nd = sh.nd, T = sh.T;
                miss += sh.kind == 0;
                hit += sh.kind != 0;
                hit_sphere += sh.kind == 2;
                const bool dead = is_black(T);
                const bool term = has_radiance(sh.C);
                if (dead || last || term) {
                    V3 C = sh.C;
                    if (sh.acc_holds) {
                        const float4 a = acc[sh.ray];
                        C = v3(a.y, a.z, a.w) + sh.C;
                    }
                    typedef float f4v __attribute__((ext_vector_type(4)));
                    if (dead || last)
                        __builtin_nontemporal_store(f4v{T.z, C.x, C.y, C.z}, reinterpret_cast<f4v *>(acc + sh.ray));
                    else
                        acc[sh.ray] = make_float4(T.z, C.x, C.y, C.z);   // read back at a later bounce
                }
                if (!dead && !last) {
                    geo_out[(size_t)pos * 2] = make_float4(no.x, no.y, no.z, nd.x);
                    geo_out[(size_t)pos * 2 + 1] = make_float4(nd.y, nd.z, T.x, T.y);
                    tz_out[pos] = T.z;
                    rid_out[pos] = sh.ray | (term || sh.acc_holds ? kAccFlag : 0u);
                    bkt_out[pos] = (uint8_t)bucket_of(no, nd, S.min_coord, S.inv_dim);
                }
            }
            __syncthreads();
            if (threadIdx.x < kBuckets) {
                uint32_t s = 0;
                for (int k = 0; k < kBlock / 64; k++) { s += wcount[k][threadIdx.x]; wcount[k][threadIdx.x] = 0; }
                run[threadIdx.x] += s;
            }
            __syncthreads();
        }
    }
    if (COUNT) {
        Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
        const unsigned long long h = wave_sum(hit), m = wave_sum(miss), hs = wave_sum(hit_sphere);
        if (lane_id() == 0 && (h | m)) {
            atomicAdd(&cs->hits, h);
            atomicAdd(&cs->misses, m);
            atomicAdd(&cs->hits_sphere, hs);
        }
    }
}

// ---------------------------------------------------------------- accumulate
// Ordered per-pixel sum of the pass's samples (the caller then adds it: fb += sum, in pass order) (raytracing.cu:96-107 without
// the unordered atomics; the CPU path's order, raytracing.cu:114-120).
// A block stages the samples of kAccPixels consecutive pixels (contiguous in tc, pixel-major)
// through LDS with coalesced loads, then one lane per pixel sums them in sample order.
constexpr int kAccPixels = 64;
// TILED: the block's pixels are tile pixels (this owner's row stripes back to back), mapped to
// image pixels by `pix`; otherwise pixels of the whole image.
// home_of (sort on, fused bounce-0 reorder): sample e's radiance is at tc[home_of[e]] (sort_scatter_shade_kernel).
template <bool TILED>
__global__ __launch_bounds__(kBlock) void accumulate_kernel(const float4 *__restrict__ tc, int rtc, int pixels,
                                                            float *__restrict__ sums, SlotMap pix,
                                                            const uint32_t *__restrict__ home_of = nullptr) {
    __shared__ float col[kAccPixels * 20 * 3];
    const int p0 = blockIdx.x * kAccPixels;
    const int np = min(kAccPixels, pixels - p0);
    const int n = np * rtc;
    const float4 *src = tc + (size_t)p0 * rtc;
    for (int e = threadIdx.x; e < n; e += kBlock) {
        const float4 c = TILED     ? tc[(size_t)pix.ray((uint32_t)(p0 + e / rtc)) * rtc + e % rtc]
                         : home_of ? tc[home_of[(size_t)p0 * rtc + e]]
                                   : src[e];
        col[e * 3] = c.y;
        col[e * 3 + 1] = c.z;
        col[e * 3 + 2] = c.w;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= np) return;
    float sx = 0, sy = 0, sz = 0;
    const float *r = col + t * rtc * 3;
    for (int s = 0; s < rtc; s++) {
        sx = sx + r[s * 3];
        sy = sy + r[s * 3 + 1];
        sz = sz + r[s * 3 + 2];
    }
    const size_t p = TILED ? (size_t)pix.ray((uint32_t)(p0 + t)) : (size_t)(p0 + t);
    sums[p * 3] = sx;
    sums[p * 3 + 1] = sy;
    sums[p * 3 + 2] = sz;
}

// ---------------------------------------------------------------- bloom (raytracing.cu:21-74)
__global__ __launch_bounds__(kBlock) void high_pass_kernel(const float *__restrict__ img, float *__restrict__ out,
                                                           float threshold, int pixels) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= pixels) return;
    const V3 c = v3(img[3 * i], img[3 * i + 1], img[3 * i + 2]);
    const bool bright = dot(c, v3(0.2126f, 0.7152f, 0.0722f)) > threshold;
    out[3 * i] = bright ? c.x : 0.0f;
    out[3 * i + 1] = bright ? c.y : 0.0f;
    out[3 * i + 2] = bright ? c.z : 0.0f;
}

template <bool VERTICAL>
__global__ __launch_bounds__(kBlock) void box_blur_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                          int radius, int w, int h) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= w * h) return;
    const int x = i % w, y = i / w;
    float sx = 0, sy = 0, sz = 0;
    int count = 0;
    for (int k = -radius; k <= radius; k++) {
        const int nx = VERTICAL ? x : x + k, ny = VERTICAL ? y + k : y;
        if (VERTICAL ? (ny >= 0 && ny < h) : (nx >= 0 && nx < w)) {
            const float *p = in + ((size_t)ny * w + nx) * 3;
            sx = sx + p[0];
            sy = sy + p[1];
            sz = sz + p[2];
            count++;
        }
    }
    const float k = 1.0f / count;
    out[3 * i] = k * sx;
    out[3 * i + 1] = k * sy;
    out[3 * i + 2] = k * sz;
}

__global__ __launch_bounds__(kBlock) void add_kernel(float *__restrict__ img, const float *__restrict__ add, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) img[i] = img[i] + add[i];
}
// The same add four floats per lane (both buffers 16-B aligned; the host checks): one pass's add into
// the framebuffer is on the pass-order chain of every frame.
__global__ __launch_bounds__(kBlock) void add4_kernel(float *__restrict__ img, const float *__restrict__ add, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int n4 = n >> 2;
    if (i < n4) {
        float4 a = reinterpret_cast<float4 *>(img)[i];
        const float4 b = reinterpret_cast<const float4 *>(add)[i];
        a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w;
        reinterpret_cast<float4 *>(img)[i] = a;
    }
    if (i < (n & 3)) img[(n4 << 2) + i] = img[(n4 << 2) + i] + add[(n4 << 2) + i];
}

// ==================================================================== host side
// Hardware queues: HIP gives a process GPU_MAX_HW_QUEUES in-order hardware queues per device
// (4 by default) and maps further streams onto them round-robin, and two pass streams that share a queue
// run their passes one after the other.  The renderer keeps up to 20 passes in flight on streams of their
// own, so loading the library asks for 24 queues unless the host set the variable itself (HIP reads it
// when it initialises, at the host's first HIP call; a host that initialised HIP before loading the
// library keeps what it had), and a renderer keeps at most as many passes in flight as the variable
// grants (queues_granted).
__attribute__((constructor(101))) void rtamd_default_hw_queues() {
    setenv("GPU_MAX_HW_QUEUES", "24", 0);   // overwrite = 0: a host's own value stands
}
int queues_granted() {
    const char *q = std::getenv("GPU_MAX_HW_QUEUES");
    const int n = q ? std::atoi(q) : 0;
    return n > 0 ? n : 4;                   // HIP's default
}

}  // namespace

// The closest-hit launch of rt_query.hip (rt_common.h): trace_kernel is compiled in this file only.
int rtamd::trace_closest_blocks_per_cu(int &per_cu) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, trace_kernel<false, false, 0>, kBlock, 0));
    return RT_OK;
}
void rtamd::launch_trace_closest(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo,
                                 const uint32_t *live, uint32_t *queue, float2 *hits, uint32_t *overflow, Counters *ctr) {
    const PassArgs pa{1, 0u, FastDiv::of(1), FastDiv::of((uint32_t)ds.width), SlotMap::identity()};
    if (count)
        hipLaunchKernelGGL((trace_kernel<false, true, 0>), dim3(grid), dim3(kBlock), 0, s, ds, pa, geo, live, queue, hits,
                           overflow, ctr, nullptr);
    else
        hipLaunchKernelGGL((trace_kernel<false, false, 0>), dim3(grid), dim3(kBlock), 0, s, ds, pa, geo, live, queue, hits,
                           overflow, ctr, nullptr);
}

// Device state of one in-flight pass: its own stream, ray state, reorder buffers and queues.
// Phase timing of renderer setup, printed to stderr when RTAMD_TIMING is set.
struct InitTimer {
    std::chrono::high_resolution_clock::time_point t = std::chrono::high_resolution_clock::now();
    std::string out;
    bool on = std::getenv("RTAMD_TIMING") != nullptr;
    void mark(const char *what) {
        if (!on) return;
        const auto now = std::chrono::high_resolution_clock::now();
        char buf[96];
        std::snprintf(buf, sizeof(buf), " %s %.1f ms,", what, std::chrono::duration<double, std::milli>(now - t).count());
        out += buf;
        t = now;
    }
    void report() const { if (on) std::fprintf(stderr, "rt_renderer init:%s\n", out.c_str()); }
};

struct PassCtx {
    hipStream_t stream = nullptr;
    // Ray state in slot order, ping-ponged by the reorder (sort off: one copy, slot = ray id):
    // geo = 2 x float4 {o.xyz, d.x} {d.yz, T.xy}, tz = T.z, rid = the ray's acc index (+ kAccFlag): its ray id,
    // or its home index (Renderer::home).  acc[that] holds {T.z, C}: the radiance once a bounce added a nonzero
    // term, and finally when the ray terminates or after the last bounce.
    // Renderer::vre, between bounce 0's shade and bounce 1's (n = the pass's rays): geo[0] holds n 16-B records
    // {d, t0} (one float4 per slot), tz[0] one u16 per slot (the bounce-0 hit's material index), rid[0] nothing (the
    // slim hand-over, shade_kernel).  Bounce 1's trace result is lean: hits holds n 4-B hit indices (its first half),
    // and geo[0]'s float4s [n, 1.75 n) hold 3 floats per slot, the hit point, written and read for hits only.
    // Both are idle then: bounce 0's shade has read its hit records, nothing of geo[0] past the records is live until
    // the reorder behind bounce 1 writes the buffer anew, and a slot's entries are written by the trace that
    // shade_rank_kernel follows, so nothing of an earlier pass is read.
    DevBuf<float4> geo[2], acc;
    DevBuf<float> tz[2];
    DevBuf<uint32_t> rid[2], sort_counts, sort_offsets, sort_totals, live, queue, overflow;
    DevBuf<uint8_t> bkt;
    DevBuf<uint8_t> bkt1;             // Renderer::vre: the bounce-1 buckets at the sorted positions (bkt: bounce 0's, by ray id)
    DevBuf<float2> hits;
    // Renderer::home: acc holds 2 x max_rays entries (ray ids below max_rays for rays terminated at bounce 0,
    // home indices from max_rays on for the rest); home_of[ray id] = where the ray's radiance is
    DevBuf<uint32_t> home_of;
    DevBuf<float> psum;               // this pass's per-pixel sums (when the caller gives no buffer)
    // pixel tiles with the reorder on: global slot per ray (ping-pong with the state), the global
    // bucket bytes (exchanged) and this owner's own bytes, their ranks, the global live count
    // {current, next, bad bytes of the run} and its host copy (pinned; lg_ready is recorded after
    // the copy, so the host waits for the count, not for the bounce queued behind it)
    DevBuf<uint32_t> gslot[2], newpos, glive;
    DevBuf<uint8_t> gbytes, lbytes;
    uint32_t *lg_host = nullptr;
    hipEvent_t lg_ready = nullptr;
    // state of this context's pass in the tiled sort-on schedule
    int t_p = 0, t_k = 0, t_b = -1, t_rtc = 0, t_rem = 0, t_n = 0, t_cur = 0, t_tiles_g = 0;
    uint64_t t_lg = 0;
    hipEvent_t fb_done = nullptr;     // recorded after this context last added into the framebuffer
    hipEvent_t done = nullptr;
    std::vector<hipEvent_t> events;   // (begin, end) pairs: process launches, then reorder launches
    size_t ev = 0;

    ~PassCtx() {
        if (lg_host) (void)hipHostFree(lg_host);
        if (lg_ready) (void)hipEventDestroy(lg_ready);
        for (auto e : events) (void)hipEventDestroy(e);
        if (fb_done) (void)hipEventDestroy(fb_done);
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int open() {
        if (stream) return RT_OK;
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&fb_done, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        return RT_OK;
    }
    hipEvent_t event() {
        if (ev == events.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            events.push_back(e);
        }
        return events[ev++];
    }
};

struct rt_renderer {
    bool sort = true, counters = false;
    int tile_count = 1, tile_index = 0, tile_rows = 8;   // pixel-tile sharding (rt_opts)
    // per-bounce HIP events for rt_stats.process_ms / sort_ms (rt_renderer_set_event_timing): four
    // marker packets per bounce in every pass's stream; off, a frame runs ~2 % faster
    bool pass_events = true;
    // Fused reorder: shade writes only buckets and the scatter replays the shading (no 36-B state
    // round trip per live ray).  It pays where the bounce is HBM-streaming bound: every bounce of
    // a scene with cheap traversal (spheres: 3.82 -> 3.52 ms/pass), and bounce 0 of a big one
    // (all rays live, primary rays cheap to replay: teapot 7.68 -> 7.49, lamp 15.33 -> 15.10);
    // at later bounces of a big BVH the replay costs more than the traffic it saves (teapot,
    // every bounce: 7.79 vs 7.73; bounces 0-1: 7.71 vs 7.61 for bounce 0 alone).  RTAMD_FUSED:
    // 0 never, 1 every bounce, k >= 2 bounces <= k - 2.
    bool fused = false;
    // No triangles (spheres.scene): no trace kernel; the sphere loop runs inside the fused
    // shade/reorder (INLINE), saving the hit round trip and the trace launch per bounce.
    bool inline_hits = false;
    int fused_upto = -1;              // fused reorder at bounces <= this (when not `fused`)
    // Sort on with the fused bounce-0 reorder: a surviving ray's radiance goes to acc[home] (home = max_rays + its
    // bounce-1 slot) instead of acc[ray id] (sort_scatter_shade_kernel).  RTAMD_HOME=0: ray ids throughout.
    bool home = false;
    uint32_t home_base = 0;
    // Virtual bounce-0 reorder (shade_rank_kernel): sort on, untiled, a scene with triangles, at least 2 bounces, and
    // a scene big enough that only bounce 0 would use the fused reorder, RTAMD_FUSED unset (set, it names the moved
    // reorder to run).  RTAMD_VREORDER: 0 never, 1 whatever the scene's size and RTAMD_FUSED.  Radiance stays in
    // acc[ray id] (no home index).
    bool vre = false;
    int width = 0, height = 0, spp = 0, bounces = 0;
    SceneDev scene;                   // the device arrays, the DevScene the kernels take, the work counters
    DevBuf<float> fb;
    DevBuf<unsigned long long> tspans;   // per run: [pass][bounce] trace-launch wall-clock spans (event timing on)
    int wall_khz = 0;                    // device wall clock rate (wall_clock64 ticks per ms)
    // rt_renderer_launch_profile: the last event-timed run's first pass, per bounce
    std::vector<double> launch_ms;
    std::vector<uint32_t> launch_live;
    // staggered start of the first passes in flight (run); RTAMD_STAGGER_US overrides, 0 = off
    // the reorder's bucket histogram counted inside the shade kernel (RTAMD_SHADE_HIST=0: its own launch)
    bool shade_hist = !std::getenv("RTAMD_SHADE_HIST") || std::atoi(std::getenv("RTAMD_SHADE_HIST")) != 0;
    int stagger_us = std::getenv("RTAMD_STAGGER_US") ? std::max(0, std::min(20000, std::atoi(std::getenv("RTAMD_STAGGER_US"))))
                                                    : kStaggerUs;
    int short_stagger_us = std::getenv("RTAMD_STAGGER_SHORT_US")
                               ? std::max(0, std::min(20000, std::atoi(std::getenv("RTAMD_STAGGER_SHORT_US")))) : kStaggerShortUs;
    PassCtx ctx[kInflight];
    int pass_hint = 0;                // rt_render: the passes this renderer will ever run (0: any)
    int inflight_limit = 0;           // a cap on passes in flight set by the creator (rt_multi next to RCCL)
    int trace_blocks = 0;             // persistent trace_kernel grid of the current run
    int trace_blocks_max = 0;         // all resident trace workgroups (the overflow stacks are sized for it)
    int nctx = 1;                     // pass contexts allocated (passes in flight)
    int inflight_cap = kInflight;     // passes in flight allowed (kInflight, or RTAMD_INFLIGHT)
    hipEvent_t t_begin = nullptr, t_end = nullptr;

    ~rt_renderer() {
        (void)hipSetDevice(scene.device);
        if (run_pending && t_end) (void)hipEventSynchronize(t_end);   // an async run never finished
        for (hipEvent_t e : pass_done) (void)hipEventDestroy(e);
        if (xcomm) {
            (void)hipSetDevice(scene.device);
            // after a failed run, collectives may be pending that a dead peer never joins: abort the
            // communicator first (that ends them), and only then drain the streams
            if (failed) (void)ncclCommAbort(static_cast<ncclComm_t>(xcomm));
            for (auto &c : ctx)
                if (c.stream) (void)hipStreamSynchronize(c.stream);
            if (!failed) (void)ncclCommDestroy(static_cast<ncclComm_t>(xcomm));
        }
        if (xhost) (void)hipHostFree(xhost);
        if (t_begin) (void)hipEventDestroy(t_begin);
        if (t_end) (void)hipEventDestroy(t_end);
    }

    hipStream_t stream() const { return ctx[0].stream; }
    // pixel tiles with the reorder on: the per-bounce bucket exchange (rt_renderer_set_exchange)
    rt_exchange_fn xfn = nullptr;
    void *xuser = nullptr;
    bool x_on_device = false;
    uint8_t *xhost = nullptr;         // pinned staging of a host exchange
    // abort check polled while the host waits for a count behind an exchange (rt_multi: a peer
    // device that failed never sends its bytes); nonzero = give up with that error code
    int (*xpoll)(void *) = nullptr;
    void *xpoll_user = nullptr;
    // RCCL communicator owned by this renderer (rt_renderer_set_exchange_rccl), or null
    void *xcomm = nullptr;
    DevBuf<int32_t> sched;            // the schedule check of a run over xcomm (4 ints)
    bool tsort() const { return tile_count > 1 && sort; }
    int pass_count() const { return (spp + 19) / 20; }
    bool tiled() const { return tile_count > 1; }
    // Pixels of this owner's stripes (the last stripe of the image may be short).
    int64_t tile_pixels() const {
        if (!tiled()) return (int64_t)width * height;
        int64_t rows = 0;
        for (int k = tile_index; (int64_t)k * tile_rows < height; k += tile_count)
            rows += std::min(tile_rows, height - k * tile_rows);
        return rows * width;
    }

    // o: checked by resolve_opts
    int init(const rt_scene *sc, const rt_opts *o) {
        scene.device = o->device;       // the destructor's, should init stop before scene.init
        sort = o->sort != 0;
        counters = o->collect_counters != 0;
        tile_count = std::max(1, o->tile_count);
        tile_index = o->tile_index;
        tile_rows = o->tile_rows > 0 ? o->tile_rows : 8;
        fused = sc->triangle_count <= RT_FUSED_MAX_TRIS;
        fused_upto = fused ? -1 : 0;
        if (const char *f = std::getenv("RTAMD_FUSED")) {
            const int v = std::atoi(f);
            fused = v == 1;
            fused_upto = v >= 2 ? v - 2 : -1;
        }
        inline_hits = fused && sc->triangle_count == 0;
        if (const char *f = std::getenv("RTAMD_INLINE")) inline_hits = fused && std::atoi(f) != 0 && sc->triangle_count == 0;
        if (tsort()) {                  // per-bounce exchange between the kernels: the plain
            fused = false;              // shade/scatter pair only
            fused_upto = -1;
            inline_hits = false;
        }
        width = sc->width;
        height = sc->height;
        spp = sc->ray_count;
        bounces = sc->bounces;
        InitTimer tm;
        HIPCHK(hipSetDevice(o->device));
        tm.mark("hipSetDevice");
        // streams cost ~3.6 ms each to create and ~2 ms to destroy: context 0's now, the other
        // contexts' once the number of passes in flight is known
        if (int rc0 = ctx[0].open()) return rc0;
        tm.mark("first stream");
        HIPCHK(hipEventCreate(&t_begin));
        HIPCHK(hipEventCreate(&t_end));
        hipStream_t s0 = stream();
        int rc;
        if ((rc = scene.init(sc, o->device, s0))) return rc;
        const int64_t pixels = (int64_t)width * height;
        const int64_t max_rays = pixels * std::min(20, std::max(1, spp));
        if (max_rays > 0x7fffffff / 3) return rtamd::fail(RT_E_INVALID, "image too large for 32-bit ray indices");
        if ((rc = fb.alloc((size_t)pixels * 3))) return rc;
        int per_cu = 0;
        tm.mark("scene upload");
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, trace_kernel<true, false, false>, kBlock, 0));
        tm.mark("occupancy query");
        trace_blocks_max = std::max(1, scene.cus * std::max(1, per_cu));
        trace_blocks = trace_blocks_max;
        const int tiles = tile_stride(max_rays);
        // the default only while RTAMD_FUSED is unset: a set RTAMD_FUSED asks for the moved reorder it names
        const bool vre_can = sort && !tiled() && bounces >= 2 && sc->triangle_count > 0;
        vre = vre_can && !std::getenv("RTAMD_FUSED") && !fused && fused_upto == 0;
        if (const char *e = std::getenv("RTAMD_VREORDER")) vre = vre_can && std::atoi(e) != 0;
        home = !vre && sort && !tiled() && bounces >= 2 && (fused || fused_upto >= 0);
        if (const char *e = std::getenv("RTAMD_HOME")) home = home && std::atoi(e) != 0;
        home_base = (uint32_t)max_rays;
        // Passes in flight: up to kInflight, as many as the frame has, and no more contexts
        // than half of the free device memory holds (1080p: ~2.9 GB per context).
        const size_t ctx_bytes = (size_t)max_rays * (2 * (32 + 4 + 4) + 16 + 1 + 8 + (tsort() ? 2 * 4 + 4 + 2 : 0) +
                                                     (home ? 16 + 4 : 0) + (vre ? 1 : 0)) +
                                 (size_t)trace_blocks_max * kBlock * 8 * (kStackMax - kStackLds) + ((size_t)1 << 20);
        size_t mem_free = 0, mem_total = 0;
        HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
        // RTAMD_INFLIGHT caps the passes in flight below kInflight (bench.py: 16 next to RCCL, where
        // 20 contexts ran a 13-pass share at 12.7 instead of 8.1 ms/pass)
        size_t cap = kInflight;
        if (inflight_limit > 0) cap = std::min<size_t>(cap, (size_t)inflight_limit);
        if (const char *e = std::getenv("RTAMD_INFLIGHT")) cap = std::min<size_t>(cap, (size_t)std::max(1, std::atoi(e)));
        // one hardware queue per pass stream (20 streams on 8 queues: 11.3 ms/pass against 6.5 on 24)
        cap = std::min<size_t>(cap, (size_t)queues_granted());
        inflight_cap = (int)cap;
        if (pass_hint > 0) cap = std::min<size_t>(cap, (size_t)pass_hint);   // a one-shot render of fewer passes
        nctx = (int)std::min<size_t>({cap, (size_t)std::max(1, pass_count()),
                                                    std::max<size_t>(1, mem_free / 2 / ctx_bytes)});
        // Pixel tiles with the reorder on: the exchange order follows the passes in flight, which
        // must therefore be the same on every owner; it may not depend on this device's free memory.
        if (tsort() && (size_t)nctx < std::min<size_t>(cap, (size_t)std::max(1, pass_count())))
            return rtamd::fail(RT_E_OOM, "pixel tiles with sort on: device memory holds only " + std::to_string(nctx) +
                                             " passes in flight; set RTAMD_INFLIGHT to the same lower value on every owner");
        const int inflight = nctx;
        for (int k = 0; k < inflight; k++) {
            PassCtx &c = ctx[k];
            if ((rc = c.open())) return rc;
            for (int q = 0; q < 2; q++) {
                if ((rc = c.geo[q].alloc((size_t)max_rays * 2))) return rc;
                if ((rc = c.tz[q].alloc((size_t)max_rays))) return rc;
                if ((rc = c.rid[q].alloc((size_t)max_rays))) return rc;
            }
            if ((rc = c.bkt.alloc((size_t)max_rays))) return rc;
            if (vre && (rc = c.bkt1.alloc((size_t)max_rays))) return rc;
            if ((rc = c.acc.alloc((size_t)max_rays * (home ? 2 : 1)))) return rc;
            if (home && (rc = c.home_of.alloc((size_t)max_rays))) return rc;
            if ((rc = c.sort_counts.alloc((size_t)kBuckets * tiles))) return rc;
            if ((rc = c.sort_offsets.alloc((size_t)kBuckets * tiles))) return rc;
            if ((rc = c.sort_totals.alloc(kBuckets))) return rc;
            if ((rc = c.live.alloc((size_t)bounces + 1))) return rc;
            if ((rc = c.queue.alloc((size_t)(bounces + 1) * kQueues * kQueueStride))) return rc;
            if ((rc = c.hits.alloc((size_t)max_rays))) return rc;
            if ((rc = c.overflow.alloc((size_t)trace_blocks_max * kBlock * 2 * (kStackMax - kStackLds)))) return rc;
            if ((rc = c.psum.alloc((size_t)pixels * 3))) return rc;
            if (tsort()) {
                for (int q = 0; q < 2; q++)
                    if ((rc = c.gslot[q].alloc((size_t)max_rays))) return rc;
                // global arrays: every live slot of the whole image (max_rays = W*H*min(spp, 20))
                if ((rc = c.newpos.alloc((size_t)max_rays)) || (rc = c.gbytes.alloc((size_t)max_rays)) ||
                    (rc = c.lbytes.alloc((size_t)max_rays)) || (rc = c.glive.alloc(3)))
                    return rc;
                HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&c.lg_host), sizeof(uint32_t)));
                HIPCHK(hipEventCreateWithFlags(&c.lg_ready, hipEventDisableTiming));
            }
        }
        tm.mark("pass contexts");
        HIPCHK(hipMemsetAsync(fb.p, 0, fb.n * sizeof(float), s0));
        HIPCHK(hipStreamSynchronize(s0));
        tm.mark("sync");
        if (tm.on) tm.out += vre ? " bounce-0 reorder: virtual" : " bounce-0 reorder: moved";
        tm.report();
        return RT_OK;
    }

    // Pass p of `while (remaining_rays)` (raytracing.cu:222-254) on context c; the pass's
    // per-pixel sums go to `sums` (W*H*3).
    // tspan: kSpanWords * (bounces + 1) words for this pass's trace-launch wall-clock spans, or null
    int enqueue_pass(PassCtx &c, int p, float *sums, int64_t &sorted, unsigned long long *tspan) {
        const int before = spp - 20 * p;
        const int rtc = std::min(before, 20);
        const int remaining = before - rtc;
        const int64_t pixels = (int64_t)width * height;
        const int64_t tpix = tile_pixels();     // pixels this render casts rays for
        const int n = (int)(rtc * tpix);
        const int grid = blocks_for(n);
        const int tiles = tile_stride(n);     // counts stride; a launch's tiles follow its live count
        const int tgrid = std::min(grid, trace_blocks);
        const int sgrid = std::min(grid, shade_grid_cap(scene.cus, RT_SHADE_BPC));
        // tile-stride reorder kernels on at most 8 blocks per CU: in the tail bounces a block per
        // possible tile dispatched ~10^4 empty workgroups per launch (A/B: +0.3-0.5 %)
        const int sort_grid = std::max(1, std::min(max_tiles(n), RT_SORT_GRID > 0 ? RT_SORT_GRID : reorder_grid_cap(scene.cus)));
        hipStream_t st = c.stream;
        int cur = 0;
        if (n == 0) {                           // a tile owner with no stripe of this image
            // empty event pairs keep the stats bookkeeping aligned: (process) per bounce, (reorder) between
            for (int k = 0; pass_events && k < 3 * bounces + 2 * (bounces - 1); k++) {
                hipEvent_t e = c.event();
                if (!e) return rtamd::fail(RT_E_HIP, "hipEventCreate failed");
                HIPCHK(hipEventRecord(e, st));
            }
            HIPCHK(hipMemsetAsync(sums, 0, (size_t)pixels * 3 * sizeof(float), st));
            return RT_OK;
        }
        hipLaunchKernelGGL(fill_live_kernel, dim3(1), dim3(256), 0, st, c.live.p, (uint32_t)n, bounces + 1, c.queue.p, tspan);
        const uint32_t stripe_px = (uint32_t)(tile_rows * width);
        const SlotMap pix = tiled() ? SlotMap::of(stripe_px, tile_count, tile_index) : SlotMap::identity();
        const SlotMap map = tiled() ? SlotMap::of(stripe_px * (uint32_t)rtc, tile_count, tile_index) : SlotMap::identity();
        const PassArgs pa{rtc, 709579u * (uint32_t)remaining, FastDiv::of((uint32_t)rtc), FastDiv::of((uint32_t)width),
                          map};
        for (int b = 0; b < bounces; b++) {
            const uint32_t seed_term = 279220567u * (uint32_t)(remaining * 20 + b);
            // events per bounce: (process begin, trace end, process end), then (reorder begin, end)
            hipEvent_t e0 = nullptr, em = nullptr, e1 = nullptr;
            if (pass_events) {
                e0 = c.event(); em = c.event(); e1 = c.event();
                if (!e0 || !em || !e1) return rtamd::fail(RT_E_HIP, "hipEventCreate failed");
                HIPCHK(hipEventRecord(e0, st));
            }
            const uint32_t *lv = c.live.p + b;
            uint32_t *q = c.queue.p + (size_t)b * kQueues * kQueueStride;
            const bool last = b + 1 == bounces;
            // virtual reorder: bounce 0 shades in place (not fused), bounce 1 runs over the ray-id slots
            const bool v0 = vre && b == 0, v1 = vre && b == 1;
            const bool fuse_b = !v0 && !v1 && (fused || b <= fused_upto);
            // the shade kernel counts the buckets (bounce 1 of the virtual reorder: sort_hist_kernel, over the sorted positions)
            // (bounce 0 of it: always the shade kernel, whatever RTAMD_SHADE_HIST says -- its bucket bytes carry
            // kSpecBit, which sort_hist_kernel does not know)
            uint32_t *hist = (shade_hist || v0) && !last && !v1 ? c.sort_counts.p : nullptr;
#define RT_PROCESS3(SORTED, COUNT, FIRST)                                                                        \
    do {                                                                                                         \
        if (!inline_hits)                                                                                        \
            hipLaunchKernelGGL((trace_kernel<SORTED, COUNT, FIRST>), dim3(tgrid), dim3(kBlock), 0, st, scene.ds, pa, \
                               c.geo[cur].p, lv, q, c.hits.p, c.overflow.p, scene.ctr.p,                         \
                               tspan ? tspan + kSpanWords * b : nullptr);                                        \
        if (em) HIPCHK(hipEventRecord(em, st));                                                                  \
        if (inline_hits)                                                                                         \
            hipLaunchKernelGGL((shade_kernel<SORTED, COUNT, FIRST, true, true>), dim3(sgrid), dim3(kBlock), 0, st,\
                               scene.ds, pa, c.geo[cur].p, c.tz[cur].p, c.rid[cur].p, c.acc.p, c.bkt.p, lv, c.hits.p, \
                               seed_term, (int)last, scene.ctr.p, nullptr, hist, tiles, (int)(home && b == 0));  \
        else if (fuse_b)                                                                                         \
            hipLaunchKernelGGL((shade_kernel<SORTED, COUNT, FIRST, true, false>), dim3(sgrid), dim3(kBlock), 0, \
                               st, scene.ds, pa, c.geo[cur].p, c.tz[cur].p, c.rid[cur].p, c.acc.p, c.bkt.p, lv, c.hits.p, \
                               seed_term, (int)last, scene.ctr.p, nullptr, hist, tiles, (int)(home && b == 0));  \
        else                                                                                                     \
            hipLaunchKernelGGL((shade_kernel<SORTED, COUNT, FIRST, false, false>), dim3(sgrid), dim3(kBlock), 0, \
                               st, scene.ds, pa, c.geo[cur].p, c.tz[cur].p, c.rid[cur].p, c.acc.p, c.bkt.p, lv, c.hits.p, \
                               seed_term, (int)last, scene.ctr.p, nullptr, hist, tiles, (int)(home && b == 0));  \
    } while (0)
#define RT_PROCESS(SORTED, COUNT)                                                                                \
    do {                                                                                                         \
        if (b == 0) RT_PROCESS3(SORTED, COUNT, 1); else RT_PROCESS3(SORTED, COUNT, 0);                           \
    } while (0)
            if (v0) {
                // shades in place and hands over slim: 16-B records in geo[cur], material indices in tz[cur] (PassCtx)
#define RT_V0PROCESS(COUNT)                                                                                      \
    do {                                                                                                         \
        hipLaunchKernelGGL((trace_kernel<true, COUNT, 1>), dim3(tgrid), dim3(kBlock), 0, st, scene.ds, pa,       \
                           c.geo[cur].p, lv, q, c.hits.p, c.overflow.p, scene.ctr.p,                             \
                           tspan ? tspan + kSpanWords * b : nullptr);                                            \
        if (em) HIPCHK(hipEventRecord(em, st));                                                                  \
        hipLaunchKernelGGL((shade_kernel<true, COUNT, 1, false, false, true>), dim3(sgrid), dim3(kBlock), 0, st, \
                           scene.ds, pa, c.geo[cur].p, c.tz[cur].p, c.rid[cur].p, c.acc.p, c.bkt.p, lv, c.hits.p, \
                           seed_term, (int)last, scene.ctr.p, nullptr, hist, tiles, 0);                          \
    } while (0)
                if (counters) RT_V0PROCESS(true); else RT_V0PROCESS(false);
#undef RT_V0PROCESS
            } else if (v1) {
                // every slot of the pass (live[0]); the state is still in ray-id order, the survivors' new state
                // goes to their sorted positions of the other buffer set.  The trace's lean result: 4-B hit indices in
                // hits, the hit points behind the n 16-B records of geo[cur] (12 n of its free 16 n bytes; PassCtx)
                float *hit_org = reinterpret_cast<float *>(c.geo[cur].p + n);
#define RT_VPROCESS(COUNT)                                                                                       \
    do {                                                                                                         \
        hipLaunchKernelGGL((trace_kernel<true, COUNT, 0, true>), dim3(tgrid), dim3(kBlock), 0, st, scene.ds, pa, \
                           c.geo[cur].p, c.live.p, q, c.hits.p, c.overflow.p, scene.ctr.p,                       \
                           tspan ? tspan + kSpanWords * b : nullptr, c.bkt.p, hit_org);                          \
        if (em) HIPCHK(hipEventRecord(em, st));                                                                  \
        hipLaunchKernelGGL((shade_rank_kernel<COUNT>), dim3(sort_grid), dim3(kBlock), 0, st, scene.ds, pa, c.bkt.p, \
                           c.geo[cur].p, reinterpret_cast<const uint16_t *>(c.tz[cur].p),                        \
                           reinterpret_cast<const int *>(c.hits.p), hit_org, seed_term,                          \
                           (int)last, c.live.p, tiles, c.sort_offsets.p, c.sort_totals.p, c.geo[1 - cur].p,      \
                           c.tz[1 - cur].p, c.rid[1 - cur].p, c.bkt1.p, c.acc.p, scene.ctr.p);                   \
    } while (0)
                if (counters) RT_VPROCESS(true); else RT_VPROCESS(false);
#undef RT_VPROCESS
                cur = 1 - cur;
            } else if (sort) {
                if (counters) RT_PROCESS(true, true); else RT_PROCESS(true, false);
            } else {
                if (b == 0 && tiled()) {        // pixel tile (sort off only): mapped bounce-0 slots
                    if (counters) RT_PROCESS3(false, true, 2); else RT_PROCESS3(false, false, 2);
                } else if (counters) RT_PROCESS(false, true); else RT_PROCESS(false, false);
            }
#undef RT_PROCESS
#undef RT_PROCESS3
            HIPCHK(hipGetLastError());
            if (pass_events) HIPCHK(hipEventRecord(e1, st));
            // The reorder (sort off: every live ray has bucket 0, so it is a stable compaction
            // of the live rays) moves the live rays' state for the next bounce.
            if (b + 1 != bounces) {
                hipEvent_t s0 = nullptr, s1 = nullptr;
                if (pass_events) {
                    s0 = c.event(); s1 = c.event();
                    if (!s0 || !s1) return rtamd::fail(RT_E_HIP, "hipEventCreate failed");
                    HIPCHK(hipEventRecord(s0, st));
                }
                const uint8_t *bk = v1 ? c.bkt1.p : c.bkt.p;
                if (!hist)
                    hipLaunchKernelGGL(sort_hist_kernel, dim3(sort_grid), dim3(kBlock), 0, st, bk, lv, tiles,
                                       c.sort_counts.p);
                hipLaunchKernelGGL(sort_scan_kernel, dim3(kBuckets), dim3(kBlock), 0, st, c.sort_counts.p, lv, tiles,
                                   c.sort_offsets.p, c.sort_totals.p, c.live.p + b + 1);
                if (v0) {
                    // nothing moves: the runs and the bounce-1 live count are all bounce 1 needs (shade_rank_kernel);
                    // its buckets start as holes
                    if (b + 2 != bounces)
                        hipLaunchKernelGGL(fill_dead_kernel, dim3(sort_grid), dim3(kBlock), 0, st, c.bkt1.p, c.live.p + 1);
                } else if (fuse_b) {
#define RT_FSC2(SO, FI, IN)                                                                                      \
    hipLaunchKernelGGL((sort_scatter_shade_kernel<SO, FI, IN>), dim3(sort_grid), dim3(kBlock), 0, st, scene.ds, pa, \
                       c.bkt.p, c.geo[cur].p, c.tz[cur].p, c.rid[cur].p, c.hits.p, seed_term, lv, tiles,          \
                       c.sort_offsets.p, c.sort_totals.p, c.geo[1 - cur].p, c.tz[1 - cur].p, c.rid[1 - cur].p,    \
                       c.acc.p, home && b == 0 ? c.home_of.p : nullptr, home_base)
#define RT_FSC(SO, FI) do { if (inline_hits) RT_FSC2(SO, FI, true); else RT_FSC2(SO, FI, false); } while (0)
                    if (sort) {
                        if (b == 0) RT_FSC(true, 1); else RT_FSC(true, 0);
                    } else {
                        if (b == 0 && tiled()) RT_FSC(false, 2); else if (b == 0) RT_FSC(false, 1); else RT_FSC(false, 0);
                    }
#undef RT_FSC
#undef RT_FSC2
                } else if (b == 0 && tiled())
                    hipLaunchKernelGGL(sort_scatter_kernel<2>, dim3(sort_grid), dim3(kBlock), 0, st, c.bkt.p, c.geo[cur].p,
                                       c.tz[cur].p, c.rid[cur].p, lv, tiles, c.sort_offsets.p, c.sort_totals.p,
                                       c.geo[1 - cur].p, c.tz[1 - cur].p, c.rid[1 - cur].p, pa.map);
                else if (b == 0)
                    hipLaunchKernelGGL(sort_scatter_kernel<1>, dim3(sort_grid), dim3(kBlock), 0, st, c.bkt.p, c.geo[cur].p,
                                       c.tz[cur].p, c.rid[cur].p, lv, tiles, c.sort_offsets.p, c.sort_totals.p,
                                       c.geo[1 - cur].p, c.tz[1 - cur].p, c.rid[1 - cur].p, pa.map);
                else
                    hipLaunchKernelGGL(sort_scatter_kernel<0>, dim3(sort_grid), dim3(kBlock), 0, st, bk, c.geo[cur].p,
                                       c.tz[cur].p, c.rid[cur].p, lv, tiles, c.sort_offsets.p, c.sort_totals.p,
                                       c.geo[1 - cur].p, c.tz[1 - cur].p, c.rid[1 - cur].p, pa.map);
                HIPCHK(hipGetLastError());
                if (pass_events) HIPCHK(hipEventRecord(s1, st));
                if (!v0) cur = 1 - cur;
                if (sort) sorted += n;
            }
        }
        if (bounces == 0) {
            // rays were generated with collected = 0 and never processed (raytracing.cu:232)
            HIPCHK(hipMemsetAsync(sums, 0, (size_t)pixels * 3 * sizeof(float), st));
        } else if (!tiled()) {
            hipLaunchKernelGGL(accumulate_kernel<false>, dim3((unsigned)((pixels + kAccPixels - 1) / kAccPixels)),
                               dim3(kBlock), 0, st, c.acc.p, rtc, (int)pixels, sums, pix, home ? c.home_of.p : nullptr);
        } else {
            // other owners' pixels stay 0 in this render's pass sums
            HIPCHK(hipMemsetAsync(sums, 0, (size_t)pixels * 3 * sizeof(float), st));
            if (tpix > 0)
                hipLaunchKernelGGL(accumulate_kernel<true>, dim3((unsigned)((tpix + kAccPixels - 1) / kAccPixels)),
                                   dim3(kBlock), 0, st, c.acc.p, rtc, (int)tpix, sums, pix);
        }
        HIPCHK(hipGetLastError());
        return RT_OK;
    }

    // ---- pixel tiles with the reorder on (rt_renderer_set_exchange)
    // The passes in flight advance in steps: every step, each active context enqueues one bounce's
    // trace and shade (+ its bucket bytes), then context by context the bytes are exchanged and the
    // global ranking and the local reorder are enqueued.  The exchange of bounce b needs the global
    // live count Lg_b on the host (the all-reduce's element count); it was copied to pinned memory at
    // the end of bounce b - 1, so the host waits for that copy's event, never for the trace and
    // shade of bounce b queued behind it, and every stream keeps a bounce of work queued while the
    // host waits.  A context that finishes its pass starts the next one at the next step, and the
    // contexts' first passes start at staggered steps, so heavy first bounces and latency-bound tail
    // bounces of different passes overlap as in the untiled pipeline.  The schedule depends only on
    // the pass count, so every owner issues its exchanges in the same order (what one RCCL
    // communicator needs).
    int wait_event(hipEvent_t e) {
        if (!xpoll) {
            HIPCHK(hipEventSynchronize(e));
            return RT_OK;
        }
        for (;;) {      // abortable wait (multi-device renders: a failed peer never sends its bytes)
            const hipError_t q = hipEventQuery(e);
            if (q == hipSuccess) return RT_OK;
            if (q != hipErrorNotReady) return hip_fail(q, "hipEventQuery");
            if (int rc = xpoll(xpoll_user)) return rtamd::fail(rc, "tile exchange aborted: another device of the render failed");
            std::this_thread::yield();
        }
    }
    int tsort_begin(PassCtx &c, int p, int k) {
        const int before = spp - 20 * p;
        c.t_p = p;
        c.t_k = k;
        c.t_b = 0;
        c.t_rtc = std::min(before, 20);
        c.t_rem = before - c.t_rtc;
        c.t_n = (int)(c.t_rtc * tile_pixels());
        c.t_cur = 0;
        c.t_lg = (uint64_t)c.t_rtc * width * height;   // every generated ray is live at bounce 0
        c.t_tiles_g = tile_stride((int64_t)c.t_lg);
        hipLaunchKernelGGL(fill_live_kernel, dim3(1), dim3(256), 0, c.stream, c.live.p, (uint32_t)c.t_n, bounces + 1,
                           c.queue.p, nullptr);
        hipLaunchKernelGGL(set_count_kernel, dim3(1), dim3(64), 0, c.stream, c.glive.p, (uint32_t)c.t_lg, nullptr);
        HIPCHK(hipGetLastError());
        return RT_OK;
    }
    PassArgs tsort_args(const PassCtx &c) const {
        const uint32_t stripe_px = (uint32_t)(tile_rows * width);
        return PassArgs{c.t_rtc, 709579u * (uint32_t)c.t_rem, FastDiv::of((uint32_t)c.t_rtc), FastDiv::of((uint32_t)width),
                        SlotMap::of(stripe_px * (uint32_t)c.t_rtc, tile_count, tile_index)};
    }
    // trace + shade of bounce b, then (but after the last bounce) this owner's bucket bytes
    int tsort_front(PassCtx &c, int b, int64_t &sorted) {
        hipStream_t st = c.stream;
        const PassArgs pa = tsort_args(c);
        const int grid = blocks_for(c.t_n);
        const int tgrid = std::max(1, std::min(grid, trace_blocks));
        const int sgrid = std::max(1, std::min(grid, scene.cus * RT_SHADE_BPC));
        const uint32_t seed_term = 279220567u * (uint32_t)(c.t_rem * 20 + b);
        const uint32_t *lv = c.live.p + b;
        uint32_t *q = c.queue.p + (size_t)b * kQueues * kQueueStride;
        const int last = b + 1 == bounces;
        const int cur = c.t_cur;
        if (!last) {
            // zero G and L over the global live prefix, even for an owner without rays: its zeros are
            // its part of the sum (an owner with no stripe, e.g. more owners than stripes)
            const int zgrid = std::max(1, std::min(blocks_for((int64_t)(c.t_lg + 15) / 16), scene.cus * 8));
            hipLaunchKernelGGL(zero_bytes_kernel, dim3(zgrid), dim3(kBlock), 0, st, c.gbytes.p, c.lbytes.p, c.glive.p);
        }
        if (c.t_n == 0) return RT_OK;
#define RT_TS(COUNT)                                                                                           \
    do {                                                                                                           \
        if (b == 0) {                                                                                              \
            hipLaunchKernelGGL((trace_kernel<true, COUNT, 2>), dim3(tgrid), dim3(kBlock), 0, st, scene.ds, pa,           \
                               c.geo[cur].p, lv, q, c.hits.p, c.overflow.p, scene.ctr.p, nullptr);                       \
            hipLaunchKernelGGL((shade_kernel<true, COUNT, 2, false, false>), dim3(sgrid), dim3(kBlock), 0, st, scene.ds, \
                               pa, c.geo[cur].p, c.tz[cur].p, c.rid[cur].p, c.acc.p, c.bkt.p, lv, c.hits.p,         \
                               seed_term, last, scene.ctr.p, nullptr);                                                   \
        } else {                                                                                                   \
            hipLaunchKernelGGL((trace_kernel<true, COUNT, 0>), dim3(tgrid), dim3(kBlock), 0, st, scene.ds, pa,           \
                               c.geo[cur].p, lv, q, c.hits.p, c.overflow.p, scene.ctr.p, nullptr);                       \
            hipLaunchKernelGGL((shade_kernel<true, COUNT, 0, false, false>), dim3(sgrid), dim3(kBlock), 0, st, scene.ds, \
                               pa, c.geo[cur].p, c.tz[cur].p, c.rid[cur].p, c.acc.p, c.bkt.p, lv, c.hits.p,         \
                               seed_term, last, scene.ctr.p, c.gslot[cur].p);                                            \
        }                                                                                                          \
    } while (0)
        if (counters) RT_TS(true); else RT_TS(false);
#undef RT_TS
        if (!last) {
            if (b == 0)
                hipLaunchKernelGGL(tile_bytes_kernel<1>, dim3(sgrid), dim3(kBlock), 0, st, c.bkt.p, lv, c.gslot[cur].p,
                                   pa.map, c.gbytes.p, c.lbytes.p);
            else
                hipLaunchKernelGGL(tile_bytes_kernel<0>, dim3(sgrid), dim3(kBlock), 0, st, c.bkt.p, lv, c.gslot[cur].p,
                                   pa.map, c.gbytes.p, c.lbytes.p);
            sorted += c.t_n;
        }
        HIPCHK(hipGetLastError());
        return RT_OK;
    }
    // the exchange of bounce b's bytes, then the global ranking and this owner's reorder
    int tsort_back(PassCtx &c, int b) {
        hipStream_t st = c.stream;
        const PassArgs pa = tsort_args(c);
        if (b > 0) {                                // global live count after bounce b - 1
            if (int rc = wait_event(c.lg_ready)) return rc;
            c.t_lg = *c.lg_host;
        }
        const uint64_t lg = c.t_lg;
        if (lg > 0) {
            int rc;
            if (x_on_device) {
                rc = xfn(xuser, c.gbytes.p, lg, st);
            } else {
                HIPCHK(hipMemcpyAsync(xhost, c.gbytes.p, lg, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                rc = xfn(xuser, xhost, lg, st);
                if (!rc) {
                    HIPCHK(hipMemcpyAsync(c.gbytes.p, xhost, lg, hipMemcpyHostToDevice, st));
                    // xhost is shared by the passes in flight: the next pass's bytes overwrite it, so
                    // this copy must have read it first
                    HIPCHK(hipStreamSynchronize(st));
                }
            }
            if (rc) return rtamd::fail(RT_E_INVALID, "tile exchange callback failed (" + std::to_string(rc) + ")");
        }
        const int tg = c.t_tiles_g;
        const int ggrid = std::max(1, std::min(max_tiles((int64_t)lg), reorder_grid_cap(scene.cus)));
        // global: buckets of every live slot -> new global slots of this owner's slots (newpos) and
        // the next global live count
        hipLaunchKernelGGL(gsort_hist_kernel, dim3(ggrid), dim3(kBlock), 0, st, c.gbytes.p, c.glive.p, tg,
                           c.sort_counts.p, c.glive.p + 2);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(kBuckets), dim3(kBlock), 0, st, c.sort_counts.p, c.glive.p, tg,
                           c.sort_offsets.p, c.sort_totals.p, c.glive.p + 1);
        hipLaunchKernelGGL(sort_rank_kernel, dim3(ggrid), dim3(kBlock), 0, st, c.gbytes.p, c.lbytes.p, c.glive.p, tg,
                           c.sort_offsets.p, c.sort_totals.p, c.newpos.p);
        hipLaunchKernelGGL(set_count_kernel, dim3(1), dim3(64), 0, st, c.glive.p, 0u, c.glive.p + 1);
        HIPCHK(hipMemcpyAsync(c.lg_host, c.glive.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(c.lg_ready, st));
        // local: this owner's rays in the same stable order (local order = ascending global slot),
        // each carrying its new global slot
        const uint32_t *lv = c.live.p + b;
        const int tiles = tile_stride(c.t_n);
        const int sort_grid = std::max(1, std::min(max_tiles(c.t_n), RT_SORT_GRID > 0 ? RT_SORT_GRID : reorder_grid_cap(scene.cus)));
        const int cur = c.t_cur;
        hipLaunchKernelGGL(sort_hist_kernel, dim3(sort_grid), dim3(kBlock), 0, st, c.bkt.p, lv, tiles, c.sort_counts.p);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(kBuckets), dim3(kBlock), 0, st, c.sort_counts.p, lv, tiles,
                           c.sort_offsets.p, c.sort_totals.p, c.live.p + b + 1);
        if (b == 0)
            hipLaunchKernelGGL(sort_scatter_kernel<2>, dim3(sort_grid), dim3(kBlock), 0, st, c.bkt.p, c.geo[cur].p,
                               c.tz[cur].p, c.rid[cur].p, lv, tiles, c.sort_offsets.p, c.sort_totals.p, c.geo[1 - cur].p,
                               c.tz[1 - cur].p, c.rid[1 - cur].p, pa.map, c.gslot[cur].p, c.newpos.p, c.gslot[1 - cur].p);
        else
            hipLaunchKernelGGL(sort_scatter_kernel<0>, dim3(sort_grid), dim3(kBlock), 0, st, c.bkt.p, c.geo[cur].p,
                               c.tz[cur].p, c.rid[cur].p, lv, tiles, c.sort_offsets.p, c.sort_totals.p, c.geo[1 - cur].p,
                               c.tz[1 - cur].p, c.rid[1 - cur].p, pa.map, c.gslot[cur].p, c.newpos.p, c.gslot[1 - cur].p);
        HIPCHK(hipGetLastError());
        c.t_cur = 1 - cur;
        return RT_OK;
    }
    int tsort_end(PassCtx &c, float *sums) {
        hipStream_t st = c.stream;
        const int64_t pixels = (int64_t)width * height;
        const int64_t tpix = tile_pixels();
        HIPCHK(hipMemsetAsync(sums, 0, (size_t)pixels * 3 * sizeof(float), st));
        if (bounces > 0 && tpix > 0) {
            const SlotMap pix = SlotMap::of((uint32_t)(tile_rows * width), tile_count, tile_index);
            hipLaunchKernelGGL(accumulate_kernel<true>, dim3((unsigned)((tpix + kAccPixels - 1) / kAccPixels)),
                               dim3(kBlock), 0, st, c.acc.p, c.t_rtc, (int)tpix, sums, pix);
        }
        HIPCHK(hipGetLastError());
        return RT_OK;
    }

    // Passes pass_begin + k*stride, k < count, nctx at a time on separate streams; the
    // framebuffer adds stay in pass order through cross-stream events.
    // pitch: floats between consecutive passes' sums in pass_sums (0 = W*H*3)
    // A run that failed (or was aborted because a peer device failed) may leave collectives of this
    // renderer's communicator pending: the destructor then aborts the communicator instead of waiting
    // for its streams (which could block forever) and destroying it.
    // Set only where work (and so collectives) may have been enqueued: argument errors and misuse of
    // the async calls leave it alone, and a run that finishes cleanly clears it.
    bool failed = false;
    bool enqueued = false;            // run_impl got past validation (set per call)
    // Framebuffer accumulation (rt_renderer_set_accumulate).  Each pass's add waits for the previous
    // pass's add on another stream; when streams outnumber the hardware queues they share in-order
    // queues, and such a wait holds up every pass queued behind it there (torch's HIP runtime on the
    // torch.distributed path: 20 passes in flight ran at 11.0 instead of 6.5 ms/pass).
    // The multi-GPU drivers add the pass sums themselves and turn it off, so no pass stream waits.
    bool accumulate = true;
    int run(int pass_begin, int count, int stride, float *pass_sums, rt_stats *st, size_t pitch = 0) {
        if (run_pending) return rtamd::fail(RT_E_INVALID, "rt_renderer_run: an async run is not finished");
        int rc = run_impl(pass_begin, count, stride, pass_sums, st, pitch, false);
        if (!rc) rc = finish_run(st);
        if (rc && enqueued) failed = true;
        if (!rc) failed = false;
        return rc;
    }
    // rt_renderer_run_async: the same passes enqueued, nothing waited for; pass k's sums are complete at
    // pass_done[k] (rt_renderer_wait_pass), the run at finish_run (rt_renderer_finish).  Everything
    // finish_run reads is the state the run was enqueued with (run_*), not the renderer's current
    // settings, and the calls that would change that state or touch the framebuffer are refused
    // while the run is pending (busy()).
    bool run_pending = false;
    int run_count = 0, run_inflight = 0;
    bool run_events = false, run_tsort = false, run_inline = false;
    size_t run_span_words = 0;        // words of tspans the run's passes wrote
    int64_t run_sorted = 0, run_generated = 0;
    std::chrono::high_resolution_clock::time_point run_w0;
    double run_enq_ms = 0;
    std::vector<hipEvent_t> pass_done;
    int busy(const char *what) const {
        return run_pending ? rtamd::fail(RT_E_INVALID, std::string(what) + ": an async run is not finished (rt_renderer_finish)")
                           : RT_OK;
    }
    int run_async(int pass_begin, int count, int stride, float *pass_sums, size_t pitch = 0) {
        if (run_pending) return rtamd::fail(RT_E_INVALID, "rt_renderer_run_async: the previous run is not finished");
        if (!pass_sums) return rtamd::fail(RT_E_INVALID, "rt_renderer_run_async: the pass sums buffer is required");
        if (tsort()) return rtamd::fail(RT_E_INVALID, "rt_renderer_run_async: not for pixel tiles with sort on");
        const int rc = run_impl(pass_begin, count, stride, pass_sums, nullptr, pitch, true);
        if (rc && enqueued) failed = true;
        return rc;
    }
    // Waits for everything queued on c's stream; with an abort poll (multi-device tile renders) the
    // wait is abortable, as wait_event's: a peer that failed never finishes its side of a collective.
    int wait_stream(PassCtx &c) {
        if (!xpoll) {
            HIPCHK(hipStreamSynchronize(c.stream));
            return RT_OK;
        }
        HIPCHK(hipEventRecord(c.done, c.stream));
        return wait_event(c.done);
    }
    int run_impl(int pass_begin, int count, int stride, float *pass_sums, rt_stats *st, size_t pitch, bool async) {
        const auto w0 = std::chrono::high_resolution_clock::now();
        enqueued = false;
        HIPCHK(hipSetDevice(scene.device));
        if (stride < 1) stride = 1;
        const int P = pass_count();
        if (count < 0) count = pass_begin < P ? (P - pass_begin + stride - 1) / stride : 0;
        if (pass_begin < 0 || (count > 0 && pass_begin + (int64_t)(count - 1) * stride >= P))
            return rtamd::fail(RT_E_INVALID, "pass range outside the render");
        if (tsort() && !xfn)
            return rtamd::fail(RT_E_INVALID, "pixel tiles with sort on need the per-bounce exchange "
                                             "(rt_renderer_set_exchange)");
        if (!accumulate && !pass_sums)
            return rtamd::fail(RT_E_INVALID, "framebuffer accumulation is off: the pass sums buffer is required");
        enqueued = true;
        const int inflight = std::min(nctx, std::max(1, P));
        {   // the trace grid of this run, for the passes it actually keeps in flight
            const int concurrent = std::max(1, std::min(inflight, count));
            const int pct = kTraceOccPct > 0 ? kTraceOccPct
                                             : std::min(100, std::max(RT_TRACE_OCC_MIN, 200 / concurrent));
            trace_blocks = std::max(1, trace_blocks_max * pct / 100);
        }
        hipStream_t s0 = stream();
        if (pass_events && tspans.n < (size_t)std::max(count, 1) * kSpanWords * (bounces + 1)) {
            if (int rc = tspans.alloc((size_t)std::max(count, 1) * kSpanWords * (bounces + 1))) return rc;
        }
        if (!wall_khz) HIPCHK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, scene.device));
        HIPCHK(hipMemsetAsync(scene.ctr.p, 0, sizeof(Counters) * kCtrSlots, s0));
        HIPCHK(hipEventRecord(t_begin, s0));
        for (int k = 1; k < inflight; k++) HIPCHK(hipStreamWaitEvent(ctx[k].stream, t_begin, 0));
        for (auto &c : ctx) c.ev = 0;
        int64_t sorted = 0, generated = 0;
        const int64_t px3 = (int64_t)width * height * 3;
        hipEvent_t prev_fb = nullptr;
        auto add_pass = [&](PassCtx &c, int p, float *sums) -> int {
            generated += (int64_t)std::min(spp - 20 * p, 20) * tile_pixels();
            if (!accumulate) return RT_OK;      // the caller adds the pass sums (rt_renderer_set_accumulate)
            if (prev_fb) HIPCHK(hipStreamWaitEvent(c.stream, prev_fb, 0));
            if ((reinterpret_cast<uintptr_t>(sums) & 15) == 0)
                hipLaunchKernelGGL(add4_kernel, dim3(blocks_for(std::max<int64_t>(px3 / 4, 4))), dim3(kBlock), 0, c.stream,
                                   fb.p, sums, (int)px3);
            else
                hipLaunchKernelGGL(add_kernel, dim3(blocks_for(px3)), dim3(kBlock), 0, c.stream, fb.p, sums, (int)px3);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(c.fb_done, c.stream));
            prev_fb = c.fb_done;
            return RT_OK;
        };
        auto sums_of = [&](PassCtx &c, int k) {
            return pass_sums ? pass_sums + (size_t)k * (pitch ? pitch : (size_t)px3) : c.psum.p;
        };
        if (tsort()) {
            // staggered first passes: context j starts at step j * bounces / inflight (RTAMD_TSTAGGER=0:
            // all at step 0, i.e. the passes of a group advance together)
            const char *stg = std::getenv("RTAMD_TSTAGGER");
            const bool stagger = !stg || std::atoi(stg) != 0;
            const int nc = std::min(inflight, std::max(count, 1));
            if (xcomm) {
                // One process per GPU: the exchange order follows the passes in flight and the stagger,
                // which environment knobs (RTAMD_INFLIGHT, RTAMD_TSTAGGER) set per process.  Owners on
                // different schedules would sum bytes of different passes without any byte going
                // missing, so the schedule is checked once per run: max and -min over the owners.
                int32_t h[4] = {nc, (int)stagger, -nc, -(int)stagger};
                if (!sched.p)
                    if (int rc = sched.alloc(4)) return rc;
                HIPCHK(hipMemcpyAsync(sched.p, h, sizeof(h), hipMemcpyHostToDevice, ctx[0].stream));
                const ncclResult_t e = ncclAllReduce(sched.p, sched.p, 4, ncclInt32, ncclMax,
                                                     static_cast<ncclComm_t>(xcomm), ctx[0].stream);
                if (e != ncclSuccess) return rtamd::fail(RT_E_HIP, std::string("Error ncclAllReduce ") + ncclGetErrorString(e));
                HIPCHK(hipMemcpyAsync(h, sched.p, sizeof(h), hipMemcpyDeviceToHost, ctx[0].stream));
                if (int rc = wait_stream(ctx[0])) return rc;
                if (h[0] != -h[2] || h[1] != -h[3])
                    return rtamd::fail(RT_E_INVALID, "pixel tiles with sort on: the owners run different exchange "
                                                     "schedules (RTAMD_INFLIGHT / RTAMD_TSTAGGER must match on every owner)");
            }
            for (int j = 0; j < nc; j++) {
                ctx[j].t_b = -1;
                HIPCHK(hipMemsetAsync(ctx[j].glive.p + 2, 0, sizeof(uint32_t), ctx[j].stream));   // bad bytes of the run
            }
            int next = 0, done = 0;
            for (int step = 0; done < count; step++) {
                for (int j = 0; j < nc; j++) {       // idle contexts take the next pass (pass order)
                    PassCtx &c = ctx[j];
                    if (c.t_b < 0 && next < count && (!stagger || step >= (int64_t)j * bounces / nc)) {
                        if (int rc = tsort_begin(c, pass_begin + next * stride, next)) return rc;
                        next++;
                    }
                }
                for (int j = 0; j < nc; j++)
                    if (ctx[j].t_b >= 0 && bounces > 0)
                        if (int rc = tsort_front(ctx[j], ctx[j].t_b, sorted)) return rc;
                for (int j = 0; j < nc; j++) {
                    PassCtx &c = ctx[j];
                    if (c.t_b < 0) continue;
                    if (c.t_b + 1 < bounces) {
                        if (int rc = tsort_back(c, c.t_b)) return rc;
                        c.t_b++;
                        continue;
                    }
                    // the pass's last bounce is enqueued: accumulate it (passes end in the order they
                    // started, so the framebuffer adds stay in pass order)
                    float *sums = sums_of(c, c.t_k);
                    if (int rc = tsort_end(c, sums)) return rc;
                    if (int rc = add_pass(c, c.t_p, sums)) return rc;
                    c.t_b = -1;
                    done++;
                }
            }
            uint32_t bad = 0;
            for (int j = 0; j < nc; j++) {
                uint32_t v = 0;
                HIPCHK(hipMemcpyAsync(&v, ctx[j].glive.p + 2, sizeof(v), hipMemcpyDeviceToHost, ctx[j].stream));
                if (int rc = wait_stream(ctx[j])) return rc;
                bad += v;
            }
            if (bad)
                return rtamd::fail(RT_E_INVALID, "tile exchange: " + std::to_string(bad) +
                                                 " global slots had no owner's byte (the exchange must sum every owner's array)");
        } else {
            // Staggered start of the first passes in flight: the first kStaggerGroup start together
            // (they fill the chip), then pass k (k < passes in flight) begins (k - group + 1) *
            // kStaggerUs later (a one-wave wait on its stream).  Started together, the first passes run
            // their heavy bounces 0-1 side by side and then their latency-bound tails side by side;
            // staggered, one pass's tail overlaps another's heavy bounces (A/B: 20-pass batch 7.13 ->
            // 7.02 ms/pass, through the dist path 7.40 -> 7.19, full frame 6.84 -> 6.74, lamp 20 steps
            // 13.53 -> 13.32; one pass every 2 ms from pass 1: 7.23 -> 7.14).  Later passes start when a
            // context frees, staggered already.  RTAMD_STAGGER_US / RTAMD_STAGGER_GROUP override.  At 4 ms,
            // runs shorter than the passes in flight only waited (round 4: cornell_plus' 13 passes of 3 ms
            // 3.04 -> 3.49 ms/pass, a 13-pass rank share at 16 in flight 7.52 -> 7.61).
            // Round 6: such a run (a rank's 13-pass share of a frame at N = 8) is one batch with no steady
            // state; its passes start kStaggerShortUs apart, scaled by the rays per pass (a 1080p pass = 1;
            // cornell_plus' 512^2 passes start ~0.25 ms apart).  A/B, teapot 13-pass share:
            // 6.42 -> 6.25 ms/pass (20 in flight), 6.53 -> 6.36 through torch.distributed at 16 in flight;
            // 2 ms for the long runs as well was worse (26 passes: 6.07 -> 6.16).  RTAMD_STAGGER_SHORT_US overrides.
            const int64_t rays_per_pass = (int64_t)std::min(spp - 20 * pass_begin, 20) * tile_pixels();
            const double short_us = short_stagger_us * std::min(1.0, (double)rays_per_pass / (1920.0 * 1080.0 * 20.0));
            const long stagger_ticks = count < kStaggerMinPasses ? 0
                                       : count >= inflight_cap ? (long)stagger_us * wall_khz / 1000
                                                               : (long)(short_us * wall_khz / 1000);
            const int stagger_group = std::getenv("RTAMD_STAGGER_GROUP") ? std::max(1, std::atoi(std::getenv("RTAMD_STAGGER_GROUP")))
                                                                        : kStaggerGroup;
            for (int k = 0; k < count; k++) {
                PassCtx &c = ctx[k % inflight];
                const int p = pass_begin + k * stride;
                float *sums = sums_of(c, k);
                if (k >= stagger_group && k < inflight && stagger_ticks > 0)
                    hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(64), 0, c.stream,
                                       (unsigned long long)((k - stagger_group + 1) * stagger_ticks));
                const int rc = enqueue_pass(c, p, sums, sorted,
                                            pass_events ? tspans.p + (size_t)k * kSpanWords * (bounces + 1) : nullptr);
                if (rc) return rc;
                if (async) {                    // pass k's sums are written: what a caller's stream may wait for
                    while ((int)pass_done.size() <= k) {
                        hipEvent_t e;
                        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                        pass_done.push_back(e);
                    }
                    HIPCHK(hipEventRecord(pass_done[k], c.stream));
                }
                if (int rc2 = add_pass(c, p, sums)) return rc2;
            }
        }
        for (int k = 1; k < inflight; k++) {
            HIPCHK(hipEventRecord(ctx[k].done, ctx[k].stream));
            HIPCHK(hipStreamWaitEvent(s0, ctx[k].done, 0));
        }
        HIPCHK(hipEventRecord(t_end, s0));
        run_enq_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - w0).count();
        run_pending = true;
        run_count = count;
        run_inflight = inflight;
        run_events = pass_events;
        run_tsort = tsort();
        run_inline = inline_hits;
        run_span_words = pass_events ? (size_t)count * kSpanWords * (bounces + 1) : 0;
        run_sorted = sorted;
        run_generated = generated;
        run_w0 = w0;
        (void)async;
        return RT_OK;
    }
    // Waits for the run enqueued last and fills `st` (rt_renderer_run, rt_renderer_finish).
    int finish_run(rt_stats *st) {
        if (!run_pending) return rtamd::fail(RT_E_INVALID, "rt_renderer_finish: no run in flight");
        run_pending = false;
        HIPCHK(hipSetDevice(scene.device));
        const int count = run_count, inflight = run_inflight;
        const bool events = run_events, tsorted = run_tsort, inl = run_inline;
        const int64_t sorted = run_sorted, generated = run_generated;
        const auto w0 = run_w0;
        if (int rc = wait_event(t_end)) return rc;    // abortable when a peer device can fail
        if (std::getenv("RTAMD_TIMING"))
            std::fprintf(stderr, "rt_renderer run: %d passes enqueued in %.2f ms (host), done at %.2f ms\n", count, run_enq_ms,
                         std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - w0).count());
#ifdef RT_PROFILE
        {
            unsigned long long pr[2][14];
            HIPCHK(hipMemcpyFromSymbol(pr, HIP_SYMBOL(g_prof), sizeof(pr)));
            for (int f = 0; f < 2; f++) {
                const unsigned long long *q = pr[f];
                const double it = (double)std::max(1ull, q[0]);
                std::fprintf(stderr, "RT_PROFILE %s wave_iters %llu active/iter %.2f leaf/iter %.2f iters_with_leaf %.3f "
                             "iters_with_inner %.3f iters_with_pop %.3f refills/iter %.3f idle_iters %llu mixed %.3f "
                             "minority/mixed %.2f lane_pops/iter %.3f uniform_record %.3f three_quarters_same %.3f\n",
                             f ? "later" : "bounce0", q[0], q[1] / it, q[2] / it, q[3] / it, q[4] / it, q[5] / it,
                             q[6] / it, q[7], q[8] / it, q[9] / (double)std::max(1ull, q[8]), q[11] / it, q[12] / it, q[13] / it);
            }
            std::memset(pr, 0, sizeof(pr));
            HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_prof), pr, sizeof(pr)));
        }
#endif
        if (st) {
            std::memset(st, 0, sizeof(*st));
            Counters c{};
            if (int rc = scene.read_counters(c)) return rc;
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, t_begin, t_end));
            st->kernel_ms = ms;
            // Per context, events come in (process begin, trace end, process end) triples with
            // (reorder begin, end) pairs between them, in enqueue order.
            double proc = 0, srt = 0, trc = 0;
            uint64_t trace_launches = 0;
            for (int q = 0; events && !tsorted && q < inflight; q++) {
                const int passes_here = count > q ? (count - q + inflight - 1) / inflight : 0;
                size_t e = 0;
                for (int r = 0; r < passes_here; r++)
                    for (int b = 0; b < bounces; b++) {
                        HIPCHK(hipEventElapsedTime(&ms, ctx[q].events[e], ctx[q].events[e + 2]));
                        proc += ms;
                        e += 3;
                        if (b + 1 != bounces) {     // reorder pair (sort off: the live-ray compaction)
                            HIPCHK(hipEventElapsedTime(&ms, ctx[q].events[e], ctx[q].events[e + 1]));
                            srt += ms;
                            e += 2;
                        }
                    }
            }
            // trace launches: the device wall-clock span from the first wave's start to the last
            // wave's end (the stream's events would add the queueing before the first wave)
            launch_ms.clear();
            launch_live.clear();
            if (events && !inl && !tsorted && count > 0 && run_span_words <= tspans.n) {
                std::vector<unsigned long long> sp(run_span_words);
                HIPCHK(hipMemcpy(sp.data(), tspans.p, sp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
                for (int k = 0; k < count; k++)
                    for (int b = 0; b < bounces; b++) {
                        const unsigned long long *w = &sp[((size_t)k * (bounces + 1) + b) * kSpanWords];
                        unsigned long long t0 = ~0ull, t1 = 0;
                        for (int x = 0; x < kSpanSlots; x++) {
                            t0 = std::min(t0, w[x]);
                            t1 = std::max(t1, w[kSpanSlots + x]);
                        }
                        if (t1 >= t0 && t0 != ~0ull) {
                            trc += (double)(t1 - t0) / wall_khz;
                            trace_launches++;
                        }
                        if (k == 0) launch_ms.push_back(t1 >= t0 && t0 != ~0ull ? (double)(t1 - t0) / wall_khz : 0.0);
                    }
                if (std::getenv("RTAMD_TIMELINE")) {
                    // diagnostic: every pass's trace launches on the device clock, ms from the run's first
                    // trace start -- "pass k: start of bounce 0, 1, 2 | end of the last bounce"
                    auto span = [&](int k, int b, int end) {
                        const unsigned long long *w = &sp[((size_t)k * (bounces + 1) + b) * kSpanWords];
                        unsigned long long t = end ? 0 : ~0ull;
                        for (int x = 0; x < kSpanSlots; x++) t = end ? std::max(t, w[kSpanSlots + x]) : std::min(t, w[x]);
                        return t;
                    };
                    unsigned long long base = ~0ull;
                    for (int k = 0; k < count; k++) base = std::min(base, span(k, 0, 0));
                    for (int k = 0; k < count; k++) {
                        std::fprintf(stderr, "timeline pass %d:", k);
                        for (int b = 0; b < std::min(bounces, 3); b++)
                            std::fprintf(stderr, " %.2f", (double)(span(k, b, 0) - base) / wall_khz);
                        std::fprintf(stderr, " | %.2f\n", (double)(span(k, bounces - 1, 1) - base) / wall_khz);
                    }
                }
                // live rays per bounce of the first pass: its context's live counts, which are pass 0's
                // only when that pass was the context's last (runs of at most `inflight` passes);
                // otherwise they are reported as 0 (unknown), not as a later pass's counts
                launch_live.assign((size_t)bounces + 1, 0u);
                if (count <= inflight)
                    HIPCHK(hipMemcpy(launch_live.data(), ctx[0].live.p, launch_live.size() * sizeof(uint32_t),
                                     hipMemcpyDeviceToHost));
                launch_live.resize((size_t)bounces);
            }
            st->process_ms = proc;
            st->sort_ms = srt;
            st->trace_ms = inl ? 0.0 : trc;
            st->trace_launches = trace_launches;
            st->generated_rays = (uint64_t)generated;
            st->live_segments = c.live;
            st->sorted_items = (uint64_t)sorted;
            st->nodes_popped = c.pn;
            st->internal_visits = c.iv;
            st->triangle_tests = c.tt;
            st->sphere_tests = c.st;
            st->hits = c.hits;
            st->misses = c.misses;
            st->hits_sphere = c.hits_sphere;
            st->dead_slots = (uint64_t)generated * bounces - c.live;
            st->passes = (uint32_t)count;
            st->render_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - w0).count();
        }
        return RT_OK;
    }
};

namespace {

int run_bloom(float *d_fb, int w, int h, float threshold, int radius, hipStream_t s) {
    const int pixels = w * h;
    float *bright = nullptr, *blur = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&bright), (size_t)pixels * 3 * sizeof(float)));
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&blur), (size_t)pixels * 3 * sizeof(float));
    if (e != hipSuccess) { (void)hipFree(bright); return hip_fail(e, "hipMalloc(blur)"); }
    hipLaunchKernelGGL(high_pass_kernel, dim3(blocks_for(pixels)), dim3(kBlock), 0, s, d_fb, bright, threshold, pixels);
    hipLaunchKernelGGL(box_blur_kernel<false>, dim3(blocks_for(pixels)), dim3(kBlock), 0, s, bright, blur, radius, w, h);
    hipLaunchKernelGGL(box_blur_kernel<true>, dim3(blocks_for(pixels)), dim3(kBlock), 0, s, blur, bright, radius, w, h);
    hipLaunchKernelGGL(add_kernel, dim3(blocks_for(pixels * 3)), dim3(kBlock), 0, s, d_fb, bright, pixels * 3);
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(s);
    (void)hipFree(bright);
    (void)hipFree(blur);
    if (le != hipSuccess) return hip_fail(le, "bloom launch");
    if (se != hipSuccess) return hip_fail(se, "bloom sync");
    return RT_OK;
}

}  // namespace

extern "C" {

void rt_default_opts(rt_opts *o) {
    std::memset(o, 0, sizeof(*o));
    o->sort = 1;
    o->pass_count = -1;
    o->pass_stride = 1;
}

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_device_warmup(int32_t device) {
    InitTimer tm;
    if (device < 0 || device >= rt_device_count()) return rtamd::fail(RT_E_NODEVICE, "no such HIP device");
    tm.mark("runtime init");
    HIPCHK(hipSetDevice(device));
    tm.mark("hipSetDevice");
    hipStream_t s;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    tm.mark("stream");
    uint32_t *d = nullptr;
    HIPCHK(hipMallocAsync(reinterpret_cast<void **>(&d), 4 * sizeof(uint32_t), s));
    // one (empty: count 0 writes nothing) launch loads this library's code object on the device
    hipLaunchKernelGGL(fill_live_kernel, dim3(1), dim3(256), 0, s, d, 0u, 0, d, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipFreeAsync(d, s));
    HIPCHK(hipStreamSynchronize(s));
    tm.mark("first launch");
    HIPCHK(hipStreamDestroy(s));
    tm.mark("stream destroy");
    if (tm.on) std::fprintf(stderr, "rt_device_warmup:%s\n", tm.out.c_str());
    return RT_OK;
}

namespace {
int create_renderer(const rt_scene *scene, const rt_opts *opts, rt_renderer **out, int pass_hint,
                    int inflight_limit = 0) {
    if (!out) return rtamd::fail(RT_E_INVALID, "null output");
    *out = nullptr;
    rt_opts o;
    int rc = resolve_opts(scene, opts, o);
    if (rc) return rc;
    auto *r = new rt_renderer();
    r->pass_hint = pass_hint;
    r->inflight_limit = inflight_limit;
    rc = r->init(scene, &o);
    if (rc) { delete r; return rc; }
    *out = r;
    return RT_OK;
}
}  // namespace

int rt_renderer_create(const rt_scene *scene, const rt_opts *opts, rt_renderer **out) {
    return create_renderer(scene, opts, out, 0);
}

// rt_multi.hip: a renderer with at most `inflight` passes in flight (RTAMD_INFLIGHT may lower it further)
int rtamd_renderer_create_inflight(const rt_scene *scene, const rt_opts *opts, rt_renderer **out, int inflight) {
    return create_renderer(scene, opts, out, 0, inflight);
}

int rtamd_renderer_run_pitched(rt_renderer *r, int pass_begin, int count, int stride, float *d_pass_sums,
                               size_t pitch, rt_stats *stats) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    return r->run(pass_begin, count, stride, d_pass_sums, stats, pitch);
}

// rt_multi.hip's overlapped exchange: rt_renderer_run_async into padded pass rows (pitch floats apart)
int rtamd_renderer_run_async_pitched(rt_renderer *r, int pass_begin, int count, int stride, float *d_pass_sums,
                                     size_t pitch) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    return r->run_async(pass_begin, count, stride, d_pass_sums, pitch);
}

int rt_renderer_run(rt_renderer *r, int32_t pass_begin, int32_t count, int32_t stride, float *d_pass_sums,
                    rt_stats *stats) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    return r->run(pass_begin, count, stride, d_pass_sums, stats);
}

int rt_renderer_run_host(rt_renderer *r, int32_t pass_begin, int32_t count, int32_t stride, float *host_pass_sums,
                         rt_stats *stats) {
    if (!r || !host_pass_sums || count < 1) return rtamd::fail(RT_E_INVALID, "rt_renderer_run_host: bad argument");
    if (int rc = r->busy("rt_renderer_run_host")) return rc;
    HIPCHK(hipSetDevice(r->scene.device));
    const size_t bytes = (size_t)count * r->width * r->height * 3 * sizeof(float);
    float *d = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), bytes));
    int rc = r->run(pass_begin, count, stride, d, stats);
    if (!rc) {
        const hipError_t e = hipMemcpy(host_pass_sums, d, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy pass sums");
    }
    (void)hipFree(d);
    return rc;
}

int rt_renderer_read_framebuffer(rt_renderer *r, float *fb_out) {
    if (!r || !fb_out) return rtamd::fail(RT_E_INVALID, "null argument");
    if (int rc = r->busy("rt_renderer_read_framebuffer")) return rc;
    HIPCHK(hipSetDevice(r->scene.device));
    HIPCHK(hipMemcpyAsync(fb_out, r->fb.p, r->fb.n * sizeof(float), hipMemcpyDeviceToHost, r->stream()));
    HIPCHK(hipStreamSynchronize(r->stream()));
    return RT_OK;
}

int rt_renderer_copy_framebuffer(rt_renderer *r, float *d_out) {
    if (!r || !d_out) return rtamd::fail(RT_E_INVALID, "null argument");
    if (int rc = r->busy("rt_renderer_copy_framebuffer")) return rc;
    HIPCHK(hipSetDevice(r->scene.device));
    HIPCHK(hipMemcpyAsync(d_out, r->fb.p, r->fb.n * sizeof(float), hipMemcpyDeviceToDevice, r->stream()));
    HIPCHK(hipStreamSynchronize(r->stream()));
    return RT_OK;
}

int rt_renderer_clear(rt_renderer *r) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    if (int rc = r->busy("rt_renderer_clear")) return rc;
    HIPCHK(hipSetDevice(r->scene.device));
    HIPCHK(hipMemsetAsync(r->fb.p, 0, r->fb.n * sizeof(float), r->stream()));
    HIPCHK(hipStreamSynchronize(r->stream()));
    return RT_OK;
}

int rt_renderer_set_event_timing(rt_renderer *r, int32_t enable) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    if (int rc = r->busy("rt_renderer_set_event_timing")) return rc;
    r->pass_events = enable != 0;
    return RT_OK;
}

int rt_renderer_run_async(rt_renderer *r, int32_t pass_begin, int32_t count, int32_t stride, float *d_pass_sums) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    return r->run_async(pass_begin, count, stride, d_pass_sums);
}

int rt_renderer_wait_pass(rt_renderer *r, int32_t k, void *hip_stream) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    if (!r->run_pending || k < 0 || k >= r->run_count || k >= (int)r->pass_done.size())
        return rtamd::fail(RT_E_INVALID, "rt_renderer_wait_pass: no such pass in the async run");
    HIPCHK(hipSetDevice(r->scene.device));
    HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), r->pass_done[k], 0));
    return RT_OK;
}

int rt_renderer_finish(rt_renderer *r, rt_stats *stats) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    if (!r->run_pending) return rtamd::fail(RT_E_INVALID, "rt_renderer_finish: no run in flight");   // misuse: not a failure
    const int rc = r->finish_run(stats);
    r->failed = rc != RT_OK;
    return rc;
}

int rt_renderer_launch_profile(rt_renderer *r, int32_t cap, double *trace_ms_out, uint32_t *live_out) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    if (int rc = r->busy("rt_renderer_launch_profile")) return rc;
    const int n = (int)std::min<size_t>(r->launch_ms.size(), (size_t)std::max(cap, 0));
    for (int b = 0; b < n; b++) {
        if (trace_ms_out) trace_ms_out[b] = r->launch_ms[b];
        if (live_out) live_out[b] = b < (int)r->launch_live.size() ? r->launch_live[b] : 0u;
    }
    return n;
}

int rt_renderer_set_exchange(rt_renderer *r, rt_exchange_fn fn, void *user, int32_t on_device) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    r->xfn = fn;
    r->xuser = user;
    r->x_on_device = on_device != 0;
    if (fn && !r->x_on_device && !r->xhost && r->tsort()) {
        HIPCHK(hipSetDevice(r->scene.device));
        const size_t n = (size_t)r->width * r->height * std::min(20, std::max(1, r->spp));
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&r->xhost), n));
    }
    return RT_OK;
}

namespace {
// The per-bounce bucket-byte exchange over the renderer's own RCCL communicator: an in-place uint8
// sum over the owners on the pass's stream (every slot has one owner, so no byte exceeds 65).
int rccl_exchange(void *user, uint8_t *bytes, uint64_t n, void *stream) {
    const ncclResult_t r = ncclAllReduce(bytes, bytes, n, ncclUint8, ncclSum, static_cast<ncclComm_t>(user),
                                         static_cast<hipStream_t>(stream));
    return r == ncclSuccess ? 0 : -(int)r - 1;
}
}  // namespace

int rt_rccl_unique_id(uint8_t *id_out) {
    static_assert(sizeof(ncclUniqueId) == RT_RCCL_ID_BYTES, "RT_RCCL_ID_BYTES must match NCCL_UNIQUE_ID_BYTES");
    if (!id_out) return rtamd::fail(RT_E_INVALID, "rt_rccl_unique_id: null output");
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return rtamd::fail(RT_E_HIP, std::string("Error ncclGetUniqueId ") + ncclGetErrorString(r));
    std::memcpy(id_out, &id, sizeof(id));
    return RT_OK;
}

int rt_renderer_set_exchange_rccl(rt_renderer *r, const uint8_t *id, int32_t nranks, int32_t rank) {
    if (!r || !id || nranks < 1 || rank < 0 || rank >= nranks)
        return rtamd::fail(RT_E_INVALID, "rt_renderer_set_exchange_rccl: bad argument");
    if (r->xcomm) return rtamd::fail(RT_E_INVALID, "rt_renderer_set_exchange_rccl: the renderer already has a communicator");
    HIPCHK(hipSetDevice(r->scene.device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    const ncclResult_t e = ncclCommInitRank(&comm, nranks, uid, rank);
    if (e != ncclSuccess) return rtamd::fail(RT_E_HIP, std::string("Error ncclCommInitRank ") + ncclGetErrorString(e));
    r->xcomm = comm;
    return rt_renderer_set_exchange(r, rccl_exchange, comm, 1);
}

int rtamd_renderer_set_poll(rt_renderer *r, int (*fn)(void *), void *user) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    r->xpoll = fn;
    r->xpoll_user = user;
    return RT_OK;
}

int rt_renderer_set_accumulate(rt_renderer *r, int32_t enable) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    if (int rc = r->busy("rt_renderer_set_accumulate")) return rc;
    r->accumulate = enable != 0;
    return RT_OK;
}

int rt_renderer_set_counters(rt_renderer *r, int32_t enable) {
    if (!r) return rtamd::fail(RT_E_INVALID, "null renderer");
    if (int rc = r->busy("rt_renderer_set_counters")) return rc;
    r->counters = enable != 0;
    return RT_OK;
}

void rt_renderer_destroy(rt_renderer *r) { delete r; }

int rt_render(const rt_scene *scene, const rt_opts *opts, float *fb_out, rt_stats *stats) {
    using clk = std::chrono::high_resolution_clock;
    const auto w0 = clk::now();
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    if (!fb_out) return rtamd::fail(RT_E_INVALID, "null framebuffer");
    rt_opts o;
    if (opts) o = *opts; else rt_default_opts(&o);
    if (o.device_count >= 1) {         // multi-GPU pass sharding over RCCL (rt_multi.hip)
        const int rc = check_scene(scene);
        return rc ? rc : rtamd_render_multi(scene, &o, fb_out, stats);
    }
    rt_renderer *r = nullptr;
    // contexts only for the passes this call renders (a one-pass render needs one, not 20)
    const int P = (scene->ray_count + 19) / 20;
    const int stride = std::max(1, o.pass_stride);
    const int hint = o.pass_count >= 0 ? o.pass_count : std::max(0, (P - o.pass_begin + stride - 1) / stride);
    int rc = create_renderer(scene, &o, &r, std::max(1, hint));
    if (rc) return rc;
    // the drop-in runs like the benchmark's timed steps: no per-bounce HIP events (~2 %; process_ms,
    // sort_ms and trace_ms stay 0 unless RTAMD_EVENTS=1)
    const char *ev = std::getenv("RTAMD_EVENTS");
    r->pass_events = ev && std::atoi(ev) != 0;
    const double t_create = ms_since(w0);
    auto w1 = clk::now();
    rc = r->run(o.pass_begin, o.pass_count, o.pass_stride, nullptr, stats);
    const double t_run = ms_since(w1);
    w1 = clk::now();
    if (!rc) rc = rt_renderer_read_framebuffer(r, fb_out);
    const double t_read = ms_since(w1);
    w1 = clk::now();
    const int inflight = r->nctx;
    delete r;
    const double t_free = ms_since(w1);
    if (std::getenv("RTAMD_TIMING"))
        std::fprintf(stderr, "rt_render: create %.1f ms (%d passes in flight), run %.1f ms, read %.1f ms, destroy %.1f ms\n",
                     t_create, inflight, t_run, t_read, t_free);
    if (!rc && stats) stats->render_ms = ms_since(w0);
    return rc;
}

int rt_bloom_device(float *d_fb, int32_t w, int32_t h, float threshold, int32_t radius, int32_t device) {
    if (!d_fb || w <= 0 || h <= 0 || radius < 0) return rtamd::fail(RT_E_INVALID, "rt_bloom_device: bad argument");
    HIPCHK(hipSetDevice(device));
    return run_bloom(d_fb, w, h, threshold, radius, nullptr);
}

int rt_bloom(float *fb, int32_t w, int32_t h, float threshold, int32_t radius, int32_t device) {
    if (!fb || w <= 0 || h <= 0 || radius < 0) return rtamd::fail(RT_E_INVALID, "rt_bloom: bad argument");
    if (rt_device_count() <= device || device < 0) return rtamd::fail(RT_E_NODEVICE, "no such HIP device");
    HIPCHK(hipSetDevice(device));
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    float *d = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), bytes));
    hipError_t e = hipMemcpy(d, fb, bytes, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? run_bloom(d, w, h, threshold, radius, nullptr) : hip_fail(e, "hipMemcpy H2D");
    if (!rc) {
        e = hipMemcpy(fb, d, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy D2H");
    }
    (void)hipFree(d);
    return rc;
}

}  // extern "C"

#ifdef RTAMD_TEST_HOOKS
// ---- Test build only (librtamd_test.so, -DRTAMD_TEST_HOOKS; the product library has none of this).
// Direct entry points to the reorder kernels for tests/test_gpu_reorder.py: each takes host arrays, launches the
// kernels above, unchanged, with the renderer's own stride (tile_stride(capacity)) and grid (max_tiles(n) under
// reorder_grid_cap, or the caller's grid), on one stream, and copies the results back.  Arrays the kernels write
// are in/out: the caller's words (a sentinel, with guard words behind the payload) go to the device first, so
// what comes back shows every store.  Indices a kernel would store through are checked on the host first.
namespace {

struct TestDev {
    int cus = 0;
    hipStream_t st = nullptr;
    ~TestDev() { if (st) (void)hipStreamDestroy(st); }
    int init(int device) {
        if (device < 0 || device >= rt_device_count()) return rtamd::fail(RT_E_NODEVICE, "no such HIP device");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        HIPCHK(hipStreamCreate(&st));
        return RT_OK;
    }
    int grid(int64_t n, int override_grid) const {
        return override_grid > 0 ? override_grid
                                 : std::max(1, std::min(max_tiles(n), RT_SORT_GRID > 0 ? RT_SORT_GRID : reorder_grid_cap(cus)));
    }
};

template <class T>
int test_upload(DevBuf<T> &b, const T *src, size_t count, hipStream_t st) {
    if (int rc = b.alloc(std::max<size_t>(count, 1))) return rc;   // never a null kernel argument
    if (count) HIPCHK(hipMemcpyAsync(b.p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
    return RT_OK;
}
template <class T>
int test_download(T *dst, const DevBuf<T> &b, size_t count, hipStream_t st) {
    if (count) HIPCHK(hipMemcpyAsync(dst, b.p, count * sizeof(T), hipMemcpyDeviceToHost, st));
    return RT_OK;
}
int test_fill(DevBuf<uint32_t> &b, size_t count, uint32_t word, hipStream_t st) {
    if (int rc = b.alloc(std::max<size_t>(count, 1))) return rc;
    if (count) HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b.p), (int)word, count, st));
    return RT_OK;
}
bool buckets_ok(const uint8_t *b, int n) {
    for (int i = 0; i < n; i++)
        if (b[i] > kDead) return false;
    return true;
}
// SlotMap::ray on the host, in plain division
uint64_t host_slot_ray(uint32_t s, uint32_t stripe, int count, int index) {
    return (uint64_t)s + (uint64_t)(s / stripe) * (uint32_t)(count - 1) * stripe + (uint64_t)index * stripe;
}
bool slot_map_ok(uint32_t stripe, int count, int index, int n_local, int n_global) {
    if (stripe == 0 || count < 1 || index < 0 || index >= count) return false;
    return n_local == 0 || host_slot_ray((uint32_t)n_local - 1, stripe, count, index) < (uint64_t)n_global;
}
bool slots_ok(const uint32_t *gslot, int n_local, int n_global) {
    for (int i = 0; i < n_local; i++)
        if (gslot[i] >= (uint32_t)n_global) return false;
    return true;
}

// the scratch of one hist -> scan -> rank/scatter chain, pre-filled with `fill`
struct TestScratch {
    DevBuf<uint32_t> counts, offsets, totals, live;   // live: {n, live_next, bad}
    int stride = 0;
    int init(int n, int64_t capacity, uint32_t fill, hipStream_t st) {
        stride = tile_stride(capacity);
        int rc;
        if ((rc = test_fill(counts, (size_t)kBuckets * stride, fill, st))) return rc;
        if ((rc = test_fill(offsets, (size_t)kBuckets * stride, fill, st))) return rc;
        if ((rc = test_fill(totals, kBuckets, fill, st))) return rc;
        if ((rc = test_fill(live, 3, fill, st))) return rc;
        const uint32_t head[3] = {(uint32_t)n, fill, 0u};
        HIPCHK(hipMemcpyAsync(live.p, head, sizeof(head), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));       // head is a local
        return RT_OK;
    }
    int read(uint32_t *c, uint32_t *o, uint32_t *t, hipStream_t st) const {
        int rc;
        if (c && (rc = test_download(c, counts, (size_t)kBuckets * stride, st))) return rc;
        if (o && (rc = test_download(o, offsets, (size_t)kBuckets * stride, st))) return rc;
        if (t && (rc = test_download(t, totals, kBuckets, st))) return rc;
        return RT_OK;
    }
};

__global__ __launch_bounds__(kBlock) void fastdiv_test_kernel(const FastDiv *__restrict__ f, const uint32_t *__restrict__ n,
                                                              int count, uint32_t *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < count) out[i] = f[i].div(n[i]);
}

}  // namespace

extern "C" {

// sort_hist_kernel -> sort_scan_kernel -> sort_scatter_kernel<0> over n slots of buckets bkt[] (0..64).
// geo_in (8 words per slot), tz_in, rid_in: the payload.  geo_out, tz_out, rid_out: in/out, out_slots slots each.
// counts, offsets (65 * stride words), totals (65), live_next (1): out.  stride = tile_stride(capacity) must be
// the caller's; *grid_out = the grid launched.
int rtamd_test_reorder_plain(int device, const uint8_t *bkt, int n, int64_t capacity, int grid, uint32_t fill, int stride,
                             const uint32_t *geo_in, const uint32_t *tz_in, const uint32_t *rid_in, uint32_t *geo_out,
                             uint32_t *tz_out, uint32_t *rid_out, int64_t out_slots, uint32_t *counts, uint32_t *offsets,
                             uint32_t *totals, uint32_t *live_next, int *grid_out) {
    if (n < 0 || capacity < n || out_slots < n || !buckets_ok(bkt, n))
        return rtamd::fail(RT_E_INVALID, "rtamd_test_reorder_plain: bad argument");
    if (stride != tile_stride(capacity)) return rtamd::fail(RT_E_INVALID, "rtamd_test_reorder_plain: stride is not tile_stride(capacity)");
    TestDev d;
    TestScratch s;
    int rc;
    if ((rc = d.init(device)) || (rc = s.init(n, capacity, fill, d.st))) return rc;
    DevBuf<uint8_t> b;
    DevBuf<uint32_t> gi, ti, ri, go, to, ro;
    if ((rc = test_upload(b, bkt, (size_t)n, d.st)) || (rc = test_upload(gi, geo_in, (size_t)n * 8, d.st)) ||
        (rc = test_upload(ti, tz_in, (size_t)n, d.st)) || (rc = test_upload(ri, rid_in, (size_t)n, d.st)) ||
        (rc = test_upload(go, geo_out, (size_t)out_slots * 8, d.st)) || (rc = test_upload(to, tz_out, (size_t)out_slots, d.st)) ||
        (rc = test_upload(ro, rid_out, (size_t)out_slots, d.st)))
        return rc;
    const int g = d.grid(n, grid);
    hipLaunchKernelGGL(sort_hist_kernel, dim3(g), dim3(kBlock), 0, d.st, b.p, s.live.p, s.stride, s.counts.p);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(kBuckets), dim3(kBlock), 0, d.st, s.counts.p, s.live.p, s.stride, s.offsets.p,
                       s.totals.p, s.live.p + 1);
    hipLaunchKernelGGL(sort_scatter_kernel<0>, dim3(g), dim3(kBlock), 0, d.st, b.p, reinterpret_cast<const float4 *>(gi.p),
                       reinterpret_cast<const float *>(ti.p), ri.p, s.live.p, s.stride, s.offsets.p, s.totals.p,
                       reinterpret_cast<float4 *>(go.p), reinterpret_cast<float *>(to.p), ro.p, SlotMap::identity());
    HIPCHK(hipGetLastError());
    if ((rc = s.read(counts, offsets, totals, d.st)) || (rc = test_download(geo_out, go, (size_t)out_slots * 8, d.st)) ||
        (rc = test_download(tz_out, to, (size_t)out_slots, d.st)) || (rc = test_download(rid_out, ro, (size_t)out_slots, d.st)))
        return rc;
    HIPCHK(hipMemcpyAsync(live_next, s.live.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, d.st));
    HIPCHK(hipStreamSynchronize(d.st));
    if (grid_out) *grid_out = g;
    return RT_OK;
}

// Pixel tiles with the reorder on.  Stage 1: gsort_hist_kernel -> sort_scan_kernel -> sort_rank_kernel over the
// exchanged bytes g[] (any value) and this owner's bytes own[], n_global each.  newpos: in/out, newpos_slots words.
// bad, live_next (1 word each), counts, offsets, totals: out, as above.
// Stage 2 (n_local >= 0): this owner's n_local rays, buckets bkt_local[], reordered as tsort_back does it --
// sort_hist_kernel -> sort_scan_kernel -> sort_scatter_kernel<form> with stage 1's newpos; form 0 reads the old
// global slots from gslot_in[], form 2 takes them from SlotMap::of(stripe, tile_count, tile_index).  gslot_out:
// in/out, gslot_out_slots words; live_next_local: out.
int rtamd_test_reorder_global(int device, const uint8_t *g, const uint8_t *own, int n_global, int64_t capacity, int grid,
                              uint32_t fill, int stride, uint32_t *newpos, int64_t newpos_slots, uint32_t *bad,
                              uint32_t *live_next, uint32_t *counts, uint32_t *offsets, uint32_t *totals, int *grid_out,
                              int n_local, const uint8_t *bkt_local, const uint32_t *gslot_in, int form, uint32_t stripe,
                              int tile_count, int tile_index, uint32_t *gslot_out, int64_t gslot_out_slots,
                              uint32_t *live_next_local) {
    if (n_global < 0 || capacity < n_global || newpos_slots < n_global)
        return rtamd::fail(RT_E_INVALID, "rtamd_test_reorder_global: bad argument");
    if (stride != tile_stride(capacity)) return rtamd::fail(RT_E_INVALID, "rtamd_test_reorder_global: stride is not tile_stride(capacity)");
    if (n_local >= 0) {
        const bool ok = n_local <= n_global && gslot_out_slots >= n_local && buckets_ok(bkt_local, n_local) &&
                        (form == 0 ? slots_ok(gslot_in, n_local, n_global)
                                   : form == 2 && slot_map_ok(stripe, tile_count, tile_index, n_local, n_global));
        if (!ok) return rtamd::fail(RT_E_INVALID, "rtamd_test_reorder_global: bad local stage");
    }
    TestDev d;
    TestScratch s;
    int rc;
    if ((rc = d.init(device)) || (rc = s.init(n_global, capacity, fill, d.st))) return rc;
    DevBuf<uint8_t> gb, ob;
    DevBuf<uint32_t> np;
    if ((rc = test_upload(gb, g, (size_t)n_global, d.st)) || (rc = test_upload(ob, own, (size_t)n_global, d.st)) ||
        (rc = test_upload(np, newpos, (size_t)newpos_slots, d.st)))
        return rc;
    const int gg = d.grid(n_global, grid);
    hipLaunchKernelGGL(gsort_hist_kernel, dim3(gg), dim3(kBlock), 0, d.st, gb.p, s.live.p, s.stride, s.counts.p, s.live.p + 2);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(kBuckets), dim3(kBlock), 0, d.st, s.counts.p, s.live.p, s.stride, s.offsets.p,
                       s.totals.p, s.live.p + 1);
    hipLaunchKernelGGL(sort_rank_kernel, dim3(gg), dim3(kBlock), 0, d.st, gb.p, ob.p, s.live.p, s.stride, s.offsets.p,
                       s.totals.p, np.p);
    HIPCHK(hipGetLastError());
    if ((rc = s.read(counts, offsets, totals, d.st)) || (rc = test_download(newpos, np, (size_t)newpos_slots, d.st))) return rc;
    HIPCHK(hipMemcpyAsync(live_next, s.live.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, d.st));
    HIPCHK(hipMemcpyAsync(bad, s.live.p + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, d.st));
    HIPCHK(hipStreamSynchronize(d.st));
    if (grid_out) *grid_out = gg;
    if (n_local < 0) return RT_OK;

    TestScratch l;
    if ((rc = l.init(n_local, n_local, fill, d.st))) return rc;
    DevBuf<uint8_t> lb;
    DevBuf<uint32_t> gin, gout, go, to, ro, gi, ti, ri;
    const size_t nl = (size_t)n_local;
    if ((rc = test_upload(lb, bkt_local, nl, d.st)) || (rc = test_upload(gout, gslot_out, (size_t)gslot_out_slots, d.st)) ||
        (rc = test_fill(gi, nl * 8, 0u, d.st)) || (rc = test_fill(ti, nl, 0u, d.st)) || (rc = test_fill(ri, nl, 0u, d.st)) ||
        (rc = test_fill(go, nl * 8, 0u, d.st)) || (rc = test_fill(to, nl, 0u, d.st)) || (rc = test_fill(ro, nl, 0u, d.st)))
        return rc;
    if (form == 0) { if ((rc = test_upload(gin, gslot_in, nl, d.st))) return rc; }
    else if ((rc = test_fill(gin, nl, fill, d.st))) return rc;
    const int lg = d.grid(n_local, grid);
    const SlotMap map = form == 2 ? SlotMap::of(stripe, tile_count, tile_index) : SlotMap::identity();
    hipLaunchKernelGGL(sort_hist_kernel, dim3(lg), dim3(kBlock), 0, d.st, lb.p, l.live.p, l.stride, l.counts.p);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(kBuckets), dim3(kBlock), 0, d.st, l.counts.p, l.live.p, l.stride, l.offsets.p,
                       l.totals.p, l.live.p + 1);
#define RT_TEST_SCATTER(FORM)                                                                                          \
    hipLaunchKernelGGL(sort_scatter_kernel<FORM>, dim3(lg), dim3(kBlock), 0, d.st, lb.p, reinterpret_cast<const float4 *>(gi.p), \
                       reinterpret_cast<const float *>(ti.p), ri.p, l.live.p, l.stride, l.offsets.p, l.totals.p,       \
                       reinterpret_cast<float4 *>(go.p), reinterpret_cast<float *>(to.p), ro.p, map, gin.p, np.p, gout.p)
    if (form == 2) RT_TEST_SCATTER(2); else RT_TEST_SCATTER(0);
#undef RT_TEST_SCATTER
    HIPCHK(hipGetLastError());
    if ((rc = test_download(gslot_out, gout, (size_t)gslot_out_slots, d.st))) return rc;
    HIPCHK(hipMemcpyAsync(live_next_local, l.live.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, d.st));
    HIPCHK(hipStreamSynchronize(d.st));
    return RT_OK;
}

// zero_bytes_kernel over n_global bytes of G and L (in/out, `slots` bytes each), then tile_bytes_kernel<0> (gslot
// given) or <1> (gslot null: SlotMap::of(stripe, tile_count, tile_index)) for n_local rays of buckets bkt[]; the
// renderer's grids (tsort_front).
int rtamd_test_tile_bytes(int device, const uint8_t *bkt, int n_local, const uint32_t *gslot, uint32_t stripe,
                          int tile_count, int tile_index, int n_global, uint8_t *G, uint8_t *L, int64_t slots) {
    const bool ok = n_local >= 0 && n_global >= 0 && n_local <= n_global && slots >= n_global && buckets_ok(bkt, n_local) &&
                    (gslot ? slots_ok(gslot, n_local, n_global) : slot_map_ok(stripe, tile_count, tile_index, n_local, n_global));
    if (!ok) return rtamd::fail(RT_E_INVALID, "rtamd_test_tile_bytes: bad argument");
    TestDev d;
    int rc;
    if ((rc = d.init(device))) return rc;
    DevBuf<uint8_t> b, gb, lb;
    DevBuf<uint32_t> gs, cnt;
    const uint32_t head[2] = {(uint32_t)n_global, (uint32_t)n_local};
    if ((rc = test_upload(b, bkt, (size_t)n_local, d.st)) || (rc = test_upload(gb, G, (size_t)slots, d.st)) ||
        (rc = test_upload(lb, L, (size_t)slots, d.st)) || (rc = test_upload(gs, gslot, gslot ? (size_t)n_local : 0, d.st)) ||
        (rc = test_upload(cnt, head, 2, d.st)))
        return rc;
    const int zgrid = std::max(1, std::min(blocks_for((int64_t)((uint64_t)n_global + 15) / 16), d.cus * 8));
    const int sgrid = std::max(1, std::min(blocks_for(n_local), d.cus * RT_SHADE_BPC));
    hipLaunchKernelGGL(zero_bytes_kernel, dim3(zgrid), dim3(kBlock), 0, d.st, gb.p, lb.p, cnt.p);
    if (gslot)
        hipLaunchKernelGGL(tile_bytes_kernel<0>, dim3(sgrid), dim3(kBlock), 0, d.st, b.p, cnt.p + 1, gs.p, SlotMap::identity(),
                           gb.p, lb.p);
    else
        hipLaunchKernelGGL(tile_bytes_kernel<1>, dim3(sgrid), dim3(kBlock), 0, d.st, b.p, cnt.p + 1, gs.p,
                           SlotMap::of(stripe, tile_count, tile_index), gb.p, lb.p);
    HIPCHK(hipGetLastError());
    if ((rc = test_download(G, gb, (size_t)slots, d.st)) || (rc = test_download(L, lb, (size_t)slots, d.st))) return rc;
    HIPCHK(hipStreamSynchronize(d.st));
    return RT_OK;
}

// out[i] = FastDiv::of(d[i]).div(n[i]) on the device (d[i] >= 1, n[i] < 2^31)
int rtamd_test_fastdiv(int device, const uint32_t *dv, const uint32_t *nv, int count, uint32_t *out) {
    if (count < 0 || !dv || !nv || !out) return rtamd::fail(RT_E_INVALID, "rtamd_test_fastdiv: bad argument");
    std::vector<FastDiv> f((size_t)count);
    for (int i = 0; i < count; i++) {
        if (dv[i] == 0 || nv[i] >= 0x80000000u) return rtamd::fail(RT_E_INVALID, "rtamd_test_fastdiv: d = 0 or n >= 2^31");
        f[(size_t)i] = FastDiv::of(dv[i]);
    }
    TestDev d;
    int rc;
    if ((rc = d.init(device))) return rc;
    DevBuf<FastDiv> fb;
    DevBuf<uint32_t> nb, ob;
    if ((rc = test_upload(fb, f.data(), (size_t)count, d.st)) || (rc = test_upload(nb, nv, (size_t)count, d.st)) ||
        (rc = test_fill(ob, (size_t)count, 0xFFFFFFFFu, d.st)))
        return rc;
    hipLaunchKernelGGL(fastdiv_test_kernel, dim3(std::max(1, blocks_for(count))), dim3(kBlock), 0, d.st, fb.p, nb.p, count, ob.p);
    HIPCHK(hipGetLastError());
    if ((rc = test_download(out, ob, (size_t)count, d.st))) return rc;
    HIPCHK(hipStreamSynchronize(d.st));
    return RT_OK;
}

}  // extern "C"
#endif  // RTAMD_TEST_HOOKS
