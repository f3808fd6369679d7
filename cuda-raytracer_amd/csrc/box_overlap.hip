// box_overlap.hip — box overlap queries (rt_query_overlap_box): every primitive that meets an axis-aligned
// box, the K smallest indices kept in order, their count and the any flag.  The arithmetic is box_overlap_math.h's,
// which the host twin (cpu_query.hip) compiles too; the query object and the C ABI are rt_query.hip's.
#include "rt_common.h"
#include "box_overlap_math.h"

#pragma clang fp contract(off)

using namespace rtamd;

namespace {

// Caller boxes (n x {lo.xyz, hi.xyz}, 24-B stride) -> one 32-B slot each: {lo.xyz, valid} {hi.xyz, 0}, valid = 1 iff
// ov::valid_box.  Block 0 also starts the call: the live count, the queue shards and the work counters (as
// query_ingest_kernel does for rays).
__global__ __launch_bounds__(kBlock) void box_ingest_kernel(const float *__restrict__ boxes, uint32_t n,
                                                            float4 *__restrict__ geo, uint32_t *__restrict__ live,
                                                            uint32_t *__restrict__ queue, Counters *__restrict__ ctr) {
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) live[0] = n;
        if (threadIdx.x < kQueues) queue[threadIdx.x * kQueueStride] = 0;
        unsigned long long *w = reinterpret_cast<unsigned long long *>(ctr);
        for (uint32_t k = threadIdx.x; k < kCtrSlots * (sizeof(Counters) / sizeof(unsigned long long)); k += kBlock) w[k] = 0;
    }
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *b = boxes + (size_t)i * 6;
    const rt_vec3 lo = {b[0], b[1], b[2]}, hi = {b[3], b[4], b[5]};
    geo[(size_t)i * 2] = make_float4(lo.x, lo.y, lo.z, __uint_as_float(ov::valid_box(lo, hi) ? 1u : 0u));
    geo[(size_t)i * 2 + 1] = make_float4(hi.x, hi.y, hi.z, 0.0f);
}

typedef int i2 __attribute__((ext_vector_type(2)));

// Both children's ov::boxes_meet on the interleaved node record {lx0 lx1 ly0 ly1} {lz0 lz1 hx0 hx1} {hy0 hy1 hz0 hz1}:
// child 0 in .x and child 1 in .y, the six comparisons of each as two-wide vector compares (all ones = true).
__device__ __forceinline__ i2 meet_pair(float4 a, float4 b, float4 c, rt_vec3 qlo, rt_vec3 qhi) {
    const f2 lx = {a.x, a.y}, ly = {a.z, a.w}, lz = {b.x, b.y};
    const f2 hx = {b.z, b.w}, hy = {c.x, c.y}, hz = {c.z, c.w};
    const f2 qlx = {qlo.x, qlo.x}, qly = {qlo.y, qlo.y}, qlz = {qlo.z, qlo.z};
    const f2 qhx = {qhi.x, qhi.x}, qhy = {qhi.y, qhi.y}, qhz = {qhi.z, qhi.z};
    return (lx <= qhx) & (qlx <= hx) & (ly <= qhy) & (qly <= hy) & (lz <= qhz) & (qlz <= hz);
}

// Every primitive that meets the lane's box (rt_abi.h, "the set H"): nearest_k_kernel's persistent loop -- the same
// queue, ballot refill, scalar root record and one record load per step -- with a predicate that is held by
// construction: whether a node is entered depends on (box, node) alone, so the lane enumerates a fixed set whatever
// the order (DESIGN §11's argument).  The order used is pinned all the same, because the any-only walk stops at its
// first member and its counters depend on it: spheres in order; the root; a leaf's triangles in order; at an internal
// node child1 (the record's first) if it meets, else child2, child2 pushed when both meet; every popped entry is entered.
// The stack holds 4-B refs only, anyhit_kernel's layout (kAnyStackLds LDS entries + the scratch slot, deeper ones in
// `overflow`).
// A leaf triangle runs the three box axes first and the other ten only when those do not separate.
// A member's index is inserted into the box's list of its K smallest indices -- the insertion list, keyed on the index
// alone, in rows slot*K.. of the caller's index array; the lane reads and writes only its own earlier stores, with
// ordinary vector loads and stores.  Its count and its K-th index stay in registers.  With index == nullptr
// (wave-uniform) nothing is kept; with only any_out given (wave-uniform) the lane retires at its first member.
// At retire -- which, as in the other kernels, waits for the lane's next refill -- the lane pads entries
// [min(count, K), K) with -1 and stores count and any.  A box that is not valid retires at refill with count 0.
// Counters (COUNT): Pn nodes entered, Iv internal nodes, Tt triangle tests, sphere tests; exact in both modes, because
// the order is pinned.  tests/overlap_ref.py restates the walk.
// The loop is nearest_k_kernel's text, repeated and not shared through a template: that kernel has to compile to the
// registers it was tuned at (profiles/overlap/kernel_resources.txt).
template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void box_overlap_kernel(DevScene S, const float4 *__restrict__ geo,
                                                                           const uint32_t *__restrict__ live_count,
                                                                           uint32_t *__restrict__ queue, int K, int32_t *li,
                                                                           int32_t *__restrict__ count_out,
                                                                           uint8_t *__restrict__ any_out,
                                                                           uint32_t *__restrict__ overflow,
                                                                           Counters *__restrict__ ctr) {
    __shared__ uint32_t stack[(kAnyStackLds + 1) * kBlock];   // + one scratch entry per lane
    uint32_t *col = stack + threadIdx.x;
    // entry e >= kAnyStackLds of this lane: overflow[(e - kAnyStackLds) * lanes + lane]
    const uint32_t lanes = gridDim.x * kBlock, gl = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t L = __builtin_amdgcn_readfirstlane(*live_count);
    const uint32_t waves = gridDim.x * (kBlock / 64);
    const uint32_t chunk = min((uint32_t)kChunkMax, max((uint32_t)kChunkMin, (L / (4 * waves) + 63) & ~63u));
    uint32_t shard = blockIdx.x % kQueues, tried = 0;
    uint32_t q_next = 0, q_end = 0;     // this wave's current chunk (wave-uniform)
    bool exhausted = false;
    int slot = -1;                      // < 0: lane has no box; <= -2: done with slot -2 - slot, row not yet finished
    rt_vec3 qlo{0, 0, 0}, qhi{0, 0, 0};
    int sp = 0;
    uint32_t ref = 0;
    int ti = 0, te = 0;                 // the lane is in a leaf while ti < te
    int cnt = 0;                        // members of the lane's box so far
    int kth_idx = 0;                    // list entry K - 1, valid once cnt >= K
    unsigned pn = 0, iv = 0, tt = 0, stn = 0, nhit = 0;
    const bool keep = li != nullptr;
    const bool any_only = !keep && count_out == nullptr && any_out != nullptr;
    // One member of the lane's box `slot` (>= 0).
    auto insert = [&](int idx) {
        if (keep) {
            int j = -1;                 // the entry the new index would take before any shift
            if (cnt < K) j = cnt;
            else if (idx < kth_idx) j = K - 1;
            if (j >= 0) {
                int32_t *ri = li + (size_t)slot * K;
                while (j > 0) {
                    const int pi = ri[j - 1];
                    if (!(idx < pi)) break;
                    if (j == K - 1) kth_idx = pi;
                    ri[j] = pi;
                    j--;
                }
                if (j == K - 1) kth_idx = idx;
                ri[j] = idx;
            }
        }
        cnt++;
    };
    // The row of a finished query: padding, count and any.
    auto finish = [&](int s) {
        if (keep) {
            for (int j = min(cnt, K); j < K; j++) li[(size_t)s * K + j] = -1;
        }
        if (count_out) count_out[s] = cnt;
        if (any_out) any_out[s] = cnt > 0 ? 1 : 0;
        nhit += cnt > 0 ? 1u : 0u;
    };
    // One internal node's step: both children's boxes against the lane's.  Returns whether the lane needs its next
    // node from the stack.
    auto node_step = [&](float4 a, float4 b, float4 c, uint2 kids) -> bool {
        if (COUNT) iv++;
        const i2 m = meet_pair(a, b, c, qlo, qhi);
        const bool e0 = m.x != 0, e1 = m.y != 0;
        const bool both = e0 && e1, any = e0 || e1;
        const uint32_t next_ref = e0 ? kids.x : kids.y;
        // written either way (above the top when not pushed; entry kAnyStackLds is a scratch slot)
        col[min(sp, kAnyStackLds) * kBlock] = kids.y;
        if (__builtin_expect(both && sp >= kAnyStackLds, 0)) overflow[(sp - kAnyStackLds) * lanes + gl] = kids.y;
        if (both) sp++;
        bool need = !any;
        if (any) {
            ref = next_ref;
            if (COUNT) pn++;
            if (ref & kLeaf) {
                leaf_range(S, ref, ti, te);
                need = ti == te;
            }
        }
        return need;
    };
    // Pop: every entry on the stack is entered; an empty stack ends the query.
    auto pop_loop = [&](bool need) {
        while (need) {
            const bool empty = sp == 0;
            sp = empty ? 0 : sp - 1;
            uint32_t e = col[min(sp, kAnyStackLds) * kBlock];
            asm volatile("" : "+v"(e));   // keeps the LDS read an LDS read (see trace_kernel)
            if (__builtin_expect(__ballot(sp >= kAnyStackLds) != 0, 0)) {   // wave-uniform, rare
                if (sp >= kAnyStackLds) e = overflow[(sp - kAnyStackLds) * lanes + gl];
            }
            slot = empty ? -2 - slot : slot;
            ref = empty ? ref : e;
            if (COUNT) pn += empty ? 0u : 1u;
            const bool leaf = !empty && (ref & kLeaf);
            if (__builtin_expect(leaf && (ref & kBigLeaf), 0)) {
                leaf_range(S, ref, ti, te);
            } else {
                ti = leaf ? (int)(ref & 0xFFFFFFu) : ti;
                te = leaf ? ti + (int)((ref >> 24) & 0x3Fu) : te;
            }
            need = leaf && ti == te;
        }
    };
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
        if (!exhausted && __popcll(idle) >= kRefill) {
            if (slot <= -2) {             // rows of the lanes that finished since the last refill
                finish(-2 - slot);
                slot = -1;
            }
            bool fresh = false;
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
                if (take) { slot = (int)(q_next + r); fresh = true; }
                q_next += (uint32_t)__popcll(took);
                idle &= ~took;
            }
            if (fresh) {
                const float4 r0 = geo[(size_t)slot * 2], r1 = geo[(size_t)slot * 2 + 1];
                qlo = {r0.x, r0.y, r0.z};
                qhi = {r1.x, r1.y, r1.z};
                cnt = 0;
                ref = S.root_ref;
                sp = 0;
                ti = te = 0;
                bool done = __float_as_uint(r0.w) == 0;   // not a valid box: count 0, nothing is tested
                if (!done) {
                    for (int i = 0; i < S.sphere_count; i++) {
                        const float4 sph = S.spheres[i];
                        if (COUNT) stn++;
                        if (ov::sphere_meets({sph.x, sph.y, sph.z}, sph.w, qlo, qhi)) {
                            insert(i);
                            if (any_only) { done = true; break; }
                        }
                    }
                }
                if (!done) {
                    if (COUNT) pn++;
                    if (ref & kLeaf) {
                        leaf_range(S, ref, ti, te);
                        done = ti == te;          // no triangles at all: spheres only
                    }
                }
                if (done) {
                    finish(slot);
                    slot = -1;
                }
            }
            if (root_internal && __ballot(fresh && slot >= 0)) {   // the fresh lanes' root step
                bool need = false;
                if (fresh && slot >= 0) need = node_step(ra, rb, rc, rk);
                pop_loop(need);
            }
        }
        if (!__ballot(slot >= 0)) {
            if (exhausted) break;
            continue;
        }
        if (slot < 0) continue;
        // ---- one step: one triangle of the current leaf, or one internal node; the record is read through
        // the same loads either way (see trace_kernel)
        bool need = false;
        const bool in_leaf = ti < te;
        const float4 *rec = in_leaf ? S.tris + (size_t)ti * 3 : S.nodes + (size_t)ref * 4;
        const float4 a = rec[0], b = rec[1], c = rec[2];
        uint2 kids = make_uint2(0, 0);
        if (!in_leaf) kids = *reinterpret_cast<const uint2 *>(rec + 3);
        if (in_leaf) {
            if (COUNT) tt++;
            const rt_vec3 v0 = {a.x, a.y, a.z}, e1 = {a.w, b.x, b.y}, e2 = {b.z, b.w, c.x};
            const rt_vec3 v1 = ov::vertex(v0, e1), v2 = ov::vertex(v0, e2);
            bool meets = !ov::box_axes_separate(v0, v1, v2, qlo, qhi);
            if (meets) meets = !ov::tail_axes_separate(v0, v1, v2, e1, e2, qlo, qhi);   // most triangles stop above
            ti++;
            need = ti == te;
            if (meets) {
                insert(S.sphere_count + ti - 1);
                if (any_only) {           // the first member ends the any-only walk
                    sp = 0;
                    ti = te = 0;
                    need = true;
                }
            }
        } else {
            need = node_step(a, b, c, kids);
        }
        pop_loop(need);
    }
    if (slot <= -2) finish(-2 - slot);
    Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
    const unsigned long long nh = wave_sum(nhit);
    if (COUNT) {
        const unsigned long long a = wave_sum(pn), b = wave_sum(iv), t = wave_sum(tt), s = wave_sum(stn);
        if (lane_id() == 0) {
            atomicAdd(&cs->pn, a);
            atomicAdd(&cs->iv, b);
            atomicAdd(&cs->tt, t);
            atomicAdd(&cs->st, s);
        }
    }
    if (lane_id() == 0 && nh) atomicAdd(&cs->hits, nh);
}

}  // namespace

namespace rtamd {

int box_overlap_blocks_per_cu(int &per_cu) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, box_overlap_kernel<false>, kBlock, 0));
    return RT_OK;
}

void launch_box_ingest(int n, hipStream_t s, const float *d_boxes, float4 *geo, uint32_t *live, uint32_t *queue,
                       Counters *ctr) {
    hipLaunchKernelGGL(box_ingest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, d_boxes, (uint32_t)n, geo, live, queue,
                       ctr);
}

void launch_box_overlap(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint32_t *live,
                        uint32_t *queue, int k, const rt_overlap_out &out, uint32_t *overflow, Counters *ctr) {
    if (count)
        hipLaunchKernelGGL(box_overlap_kernel<true>, dim3(grid), dim3(kBlock), 0, s, ds, geo, live, queue, k, out.index,
                           out.count, out.any, overflow, ctr);
    else
        hipLaunchKernelGGL(box_overlap_kernel<false>, dim3(grid), dim3(kBlock), 0, s, ds, geo, live, queue, k, out.index,
                           out.count, out.any, overflow, ctr);
}

}  // namespace rtamd
