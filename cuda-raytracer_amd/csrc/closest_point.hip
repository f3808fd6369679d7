// closest_point.hip — closest-point queries (rt_query_closest_point): the ingest kernel and the
// traversal with a shrinking distance bound.  The arithmetic is closest_point_math.h's, which the host twin
// (cpu_query.hip) compiles too; the query object and the C ABI are rt_query.hip's.
#include "rt_common.h"
#include "closest_point_math.h"

#include <climits>

#pragma clang fp contract(off)

using namespace rtamd;

namespace {

// Caller points (n x {x y z}, 12-B stride) and bounds -> one 16-B slot each: {p.xyz, B2}, B2 = cp::bound2 of
// the point's max_dist (+inf without a max_dist array).  Block 0 also starts the call: the live count, the
// queue shards and the work counters (as query_ingest_kernel does for rays).
__global__ __launch_bounds__(kBlock) void point_ingest_kernel(const float *__restrict__ points,
                                                              const float *__restrict__ max_dist, uint32_t n,
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
    const float *p = points + (size_t)i * 3;
    geo[i] = make_float4(p[0], p[1], p[2], max_dist ? cp::bound2(max_dist[i]) : INFINITY);
}

// Both children's box distances on the interleaved node record {lx0 lx1 ly0 ly1} {lz0 lz1 hx0 hx1}
// {hy0 hy1 hz0 hz1}: cp::box2 of child 0 in .x and of child 1 in .y, the subtractions, squares and sums as
// packed-fp32 ops shared by the two boxes (slab_pair's scheme).  Each lane of a packed op is the scalar op.
__device__ __forceinline__ f2 box2_pair(float4 a, float4 b, float4 c, rt_vec3 p) {
    const f2 px = {p.x, p.x}, py = {p.y, p.y}, pz = {p.z, p.z};
    const f2 lx = {a.x, a.y}, ly = {a.z, a.w}, lz = {b.x, b.y};
    const f2 hx = {b.z, b.w}, hy = {c.x, c.y}, hz = {c.z, c.w};
    const f2 x1 = lx - px, x2 = px - hx;
    const f2 y1 = ly - py, y2 = py - hy;
    const f2 z1 = lz - pz, z2 = pz - hz;
    const f2 qx = {fmaxf(fmaxf(x1.x, x2.x), 0.0f), fmaxf(fmaxf(x1.y, x2.y), 0.0f)};
    const f2 qy = {fmaxf(fmaxf(y1.x, y2.x), 0.0f), fmaxf(fmaxf(y1.y, y2.y), 0.0f)};
    const f2 qz = {fmaxf(fmaxf(z1.x, z2.x), 0.0f), fmaxf(fmaxf(z1.y, z2.y), 0.0f)};
    return (qx * qx + qy * qy) + qz * qz;
}

// The nearest primitive of each point (rt_abi.h, "the walk, pinned"): one query per lane, the state
// (best2, best) in registers.  The bound shrinks as primitives are accepted, so which nodes are entered
// depends on the visit order and the order is part of the definition: spheres in order; the root; at an
// internal node the child with the smaller box distance first (a tie goes to child 0, the record's first), the
// other one pushed with its distance if it is eligible too; a leaf's triangles in order; a pop discards the
// entries whose stored distance exceeds the current best2.
// Queue, ballot refill, scalar root record and the one record load per step are trace_kernel's; so is the
// stack: (ref, box2) pairs, kStackLds entries per lane in LDS plus a scratch slot, deeper ones in `overflow`
// in trace_kernel's layout (the walk pushes at most one entry per level: kStackMax holds).
// A lane that has emptied its stack keeps (p, best2, best) until the wave's next refill (or the exit), where
// it evaluates the accepted primitive once more for the point and uv and stores the caller's rows itself.
// A point with a non-finite component, or a negative bound, retires at refill.
// Counters (COUNT): Pn = nodes entered, Iv = internal nodes stepped, Tt = triangle tests, sphere tests; exact,
// because the order is pinned.  tests/closest_point_ref.py restates the walk.
template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void closest_point_kernel(DevScene S, const float4 *__restrict__ geo,
                                                                             const uint32_t *__restrict__ live_count,
                                                                             uint32_t *__restrict__ queue,
                                                                             rt_closest_point_out out,
                                                                             uint32_t *__restrict__ overflow,
                                                                             Counters *__restrict__ ctr) {
    __shared__ uint2 stack[(kStackLds + 1) * kBlock];   // + one scratch entry per lane
    uint2 *col = stack + threadIdx.x;
    // entry e >= kStackLds of this lane: ref at overflow[(e - kStackLds) * lanes + lane], box2 in the second half
    const uint32_t lanes = gridDim.x * kBlock, gl = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t dist_half = lanes * (kStackMax - kStackLds);
    const uint32_t L = __builtin_amdgcn_readfirstlane(*live_count);
    const uint32_t waves = gridDim.x * (kBlock / 64);
    const uint32_t chunk = min((uint32_t)kChunkMax, max((uint32_t)kChunkMin, (L / (4 * waves) + 63) & ~63u));
    uint32_t shard = blockIdx.x % kQueues, tried = 0;
    uint32_t q_next = 0, q_end = 0;     // this wave's current chunk (wave-uniform)
    bool exhausted = false;
    int slot = -1;                      // < 0: lane has no point; <= -2: done with slot -2 - slot, row not yet stored
    rt_vec3 p{0, 0, 0};
    float best2 = 0;
    int best = INT_MAX;
    int sp = 0;
    uint32_t ref = 0;
    int ti = 0, te = 0;                 // the lane is in a leaf while ti < te
    unsigned pn = 0, iv = 0, tt = 0, stn = 0, nhit = 0, nsph = 0;
    // The row of a finished query: the accepted primitive evaluated once more, by the same functions.
    auto finish = [&](int s) {
        const bool hit = best != INT_MAX;
        cp::Near nr{0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
        if (hit && (out.point || out.uv)) {
            if (best < S.sphere_count) {
                const float4 sph = S.spheres[best];
                nr = cp::sphere(p, {sph.x, sph.y, sph.z}, sph.w);
            } else {
                const float4 *tr = S.tris + (size_t)(best - S.sphere_count) * 3;
                const float4 a = tr[0], b = tr[1], c = tr[2];
                nr = cp::triangle(p, {a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w, c.x});
            }
        }
        if (out.distance) out.distance[s] = hit ? sqrtf(best2) : 1e30f;
        if (out.index) out.index[s] = hit ? best : -1;
        if (out.point) {
            float *q = out.point + (size_t)s * 3;
            q[0] = nr.point.x; q[1] = nr.point.y; q[2] = nr.point.z;
        }
        if (out.uv) {
            out.uv[(size_t)s * 2] = nr.u;
            out.uv[(size_t)s * 2 + 1] = nr.v;
        }
        nhit += hit ? 1u : 0u;
        nsph += hit && best < S.sphere_count ? 1u : 0u;
    };
    // One internal node's step: both children's box distances against best2.  Returns whether the lane needs
    // its next node from the stack.
    auto node_step = [&](float4 a, float4 b, float4 c, uint2 kids) -> bool {
        if (COUNT) iv++;
        const f2 d = box2_pair(a, b, c, p);
        const bool e0 = !(d.x > best2), e1 = !(d.y > best2);
        const bool both = e0 && e1, any = e0 || e1;
        const bool sel1 = e1 && (!e0 || d.y < d.x);
        const uint32_t next_ref = sel1 ? kids.y : kids.x, far_ref = sel1 ? kids.x : kids.y;
        const float far_d = sel1 ? d.x : d.y;
        // written either way (above the top when not pushed; entry kStackLds is a scratch slot)
        col[min(sp, kStackLds) * kBlock] = make_uint2(far_ref, __float_as_uint(far_d));
        if (__builtin_expect(both && sp >= kStackLds, 0)) {
            overflow[(sp - kStackLds) * lanes + gl] = far_ref;
            overflow[dist_half + (sp - kStackLds) * lanes + gl] = __float_as_uint(far_d);
        }
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
    // Pop to the next entry whose stored distance does not exceed the current best2; an empty stack ends the query.
    auto pop_loop = [&](bool need) {
        while (need) {
            const bool empty = sp == 0;
            sp = empty ? 0 : sp - 1;
            uint2 e = col[min(sp, kStackLds) * kBlock];
            asm volatile("" : "+v"(e.x), "+v"(e.y));   // keeps the LDS read an LDS read (see trace_kernel)
            if (__builtin_expect(__ballot(sp >= kStackLds) != 0, 0)) {   // wave-uniform, rare
                if (sp >= kStackLds) {
                    e.x = overflow[(sp - kStackLds) * lanes + gl];
                    e.y = overflow[dist_half + (sp - kStackLds) * lanes + gl];
                }
            }
            const bool take = !empty && !(__uint_as_float(e.y) > best2);
            slot = empty ? -2 - slot : slot;
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
                const float4 r0 = geo[slot];
                p = {r0.x, r0.y, r0.z};
                best2 = r0.w;
                best = INT_MAX;
                ref = S.root_ref;
                sp = 0;
                ti = te = 0;
                bool done = !cp::finite3(p);      // a miss, nothing is traversed
                if (!done) {
                    for (int i = 0; i < S.sphere_count; i++) {
                        const float4 sph = S.spheres[i];
                        rt_vec3 w;
                        float len;
                        if (COUNT) stn++;
                        const float d2 = cp::sphere_dist2(p, {sph.x, sph.y, sph.z}, sph.w, w, len);
                        if (cp::accepts(d2, i, best2, best)) { best2 = d2; best = i; }
                    }
                    done = 0.0f > best2;          // a negative bound: nothing qualifies
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
            const cp::Near nr = cp::triangle(p, {a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w, c.x});
            const int idx = S.sphere_count + ti;
            const bool acc = cp::accepts(nr.dist2, idx, best2, best);
            best2 = acc ? nr.dist2 : best2;
            best = acc ? idx : best;
            ti++;
            need = ti == te;
        } else {
            need = node_step(a, b, c, kids);
        }
        pop_loop(need);
    }
    if (slot <= -2) finish(-2 - slot);
    Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
    const unsigned long long nh = wave_sum(nhit), ns = wave_sum(nsph);
    if (COUNT) {
        const unsigned long long a = wave_sum(pn), b = wave_sum(iv), t = wave_sum(tt), s = wave_sum(stn);
        if (lane_id() == 0) {
            atomicAdd(&cs->pn, a);
            atomicAdd(&cs->iv, b);
            atomicAdd(&cs->tt, t);
            atomicAdd(&cs->st, s);
        }
    }
    if (lane_id() == 0 && nh) {
        atomicAdd(&cs->hits, nh);
        if (ns) atomicAdd(&cs->hits_sphere, ns);
    }
}

}  // namespace

namespace rtamd {

int closest_point_blocks_per_cu(int &per_cu) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, closest_point_kernel<false>, kBlock, 0));
    return RT_OK;
}

void launch_point_ingest(int n, hipStream_t s, const float *d_points, const float *d_max_dist, float4 *geo, uint32_t *live,
                         uint32_t *queue, Counters *ctr) {
    hipLaunchKernelGGL(point_ingest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, d_points, d_max_dist, (uint32_t)n, geo,
                       live, queue, ctr);
}

void launch_closest_point(bool count, int n, int grid, hipStream_t s, const DevScene &ds, const float *d_points,
                          const float *d_max_dist, float4 *geo, uint32_t *live, uint32_t *queue,
                          const rt_closest_point_out &out, uint32_t *overflow, Counters *ctr) {
    launch_point_ingest(n, s, d_points, d_max_dist, geo, live, queue, ctr);
    if (count)
        hipLaunchKernelGGL(closest_point_kernel<true>, dim3(grid), dim3(kBlock), 0, s, ds, geo, live, queue, out, overflow, ctr);
    else
        hipLaunchKernelGGL(closest_point_kernel<false>, dim3(grid), dim3(kBlock), 0, s, ds, geo, live, queue, out, overflow, ctr);
}

}  // namespace rtamd
