// nearest_k.hip — range queries (rt_query_nearest_k): every primitive within a point's max_dist, the K
// nearest kept in order, and their count.  The arithmetic is closest_point_math.h's, which the host twin
// (cpu_query.hip) compiles too; the ingest is closest_point.hip's, the query object and the C ABI are rt_query.hip's.
#include "rt_common.h"
#include "closest_point_math.h"

#pragma clang fp contract(off)

using namespace rtamd;

namespace {

// Both children's box distances: closest_point.hip's box2_pair, repeated here (see the note on shared text below).
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

// Every primitive within the point's bound B2 (rt_abi.h, "the set H"): closest_point_kernel's traversal -- the same
// queue, ballot refill, scalar root record, one record load per step and box2_pair -- with the bound HELD: an accept
// never changes B2, the sphere loop runs to the end and a lane retires only when its stack is empty.  Whether a node
// is entered then depends on (point, B2, node) alone, so the lane enumerates a fixed set whatever the order
// (DESIGN §11's argument); the order used is the nearer child first, a tie to child 0 (the record's first).
// With the bound fixed the push-time test is the pop-time test: the stack holds 4-B refs only, anyhit_kernel's layout
// (kAnyStackLds LDS entries + the scratch slot, deeper ones in `overflow`), and every popped entry is entered.
// A member (dist2, index) is inserted into the point's list of its K smallest by the key (dist2 bits, index) --
// multihit_kernel's insertion list, in rows slot*K.. of ld[] and li[] (the caller's distance and index arrays, or the
// object's scratch for a half the caller left out); the lane reads and writes only its own earlier stores, with
// ordinary vector loads and stores.  Its count and the key of its K-th entry stay in registers.  With ld == nullptr
// (wave-uniform) nothing is kept and the lane only counts.
// At retire -- which, as in the other kernels, waits for the lane's next refill -- the lane turns the kept dist2
// into sqrtf(dist2) in place, evaluates `point` of each kept entry once more by cp::triangle / cp::sphere, pads
// entries [min(count, K), K) with (1e30, -1, (0, 0, 0)) and stores the count.
// Counters (COUNT): Pn nodes entered, Iv internal nodes, Tt triangle tests, sphere tests: the full walk's,
// order-independent.  tests/nearest_k_ref.py restates the walk.
// The loop is closest_point_kernel's and the list multihit_kernel's text, repeated and not shared through a template:
// those two have to compile to the registers they were tuned at (profiles/nearest_k/kernel_resources.txt).
template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void nearest_k_kernel(DevScene S, const float4 *__restrict__ geo,
                                                                         const uint32_t *__restrict__ live_count,
                                                                         uint32_t *__restrict__ queue, int K, float *ld,
                                                                         int32_t *li, float *__restrict__ point_out,
                                                                         int32_t *__restrict__ count_out,
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
    int slot = -1;                      // < 0: lane has no point; <= -2: done with slot -2 - slot, row not yet finished
    rt_vec3 p{0, 0, 0};
    float B2 = 0;
    int sp = 0;
    uint32_t ref = 0;
    int ti = 0, te = 0;                 // the lane is in a leaf while ti < te
    int cnt = 0;                        // members of the lane's point so far
    uint32_t kth_key = 0;               // key of list entry K - 1, valid once cnt >= K
    int kth_idx = 0;
    unsigned pn = 0, iv = 0, tt = 0, stn = 0, nhit = 0;
    const bool keep = ld != nullptr;
    // One member of the lane's point `slot` (>= 0).
    auto insert = [&](float d2, int idx) {
        if (keep) {
            const uint32_t key = cp::key_bits(d2);
            int j = -1;                 // the entry the new record would take before any shift
            if (cnt < K) j = cnt;
            else if (cp::key_less(key, idx, kth_key, kth_idx)) j = K - 1;
            if (j >= 0) {
                float *rd = ld + (size_t)slot * K;
                int32_t *ri = li + (size_t)slot * K;
                while (j > 0) {
                    const float pd = rd[j - 1];
                    const int pi = ri[j - 1];
                    const uint32_t pk = cp::key_bits(pd);
                    if (!cp::key_less(key, idx, pk, pi)) break;
                    if (j == K - 1) { kth_key = pk; kth_idx = pi; }
                    rd[j] = pd;
                    ri[j] = pi;
                    j--;
                }
                if (j == K - 1) { kth_key = key; kth_idx = idx; }
                rd[j] = d2;
                ri[j] = idx;
            }
        }
        cnt++;
    };
    // The row of a finished query: distances, points, padding and count.
    auto finish = [&](int s) {
        if (keep) {
            const int kept = min(cnt, K);
            for (int j = 0; j < kept; j++) {
                const size_t e = (size_t)s * K + j;
                ld[e] = sqrtf(ld[e]);
                if (point_out) {
                    const int idx = li[e];
                    cp::Near nr;
                    if (idx < S.sphere_count) {
                        const float4 sph = S.spheres[idx];
                        nr = cp::sphere(p, {sph.x, sph.y, sph.z}, sph.w);
                    } else {
                        const float4 *tr = S.tris + (size_t)(idx - S.sphere_count) * 3;
                        const float4 a = tr[0], b = tr[1], c = tr[2];
                        nr = cp::triangle(p, {a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w, c.x});
                    }
                    float *q = point_out + e * 3;
                    q[0] = nr.point.x; q[1] = nr.point.y; q[2] = nr.point.z;
                }
            }
            for (int j = kept; j < K; j++) {
                const size_t e = (size_t)s * K + j;
                ld[e] = 1e30f;
                li[e] = -1;
                if (point_out) {
                    float *q = point_out + e * 3;
                    q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f;
                }
            }
        }
        if (count_out) count_out[s] = cnt;
        nhit += cnt > 0 ? 1u : 0u;
    };
    // One internal node's step: both children's box distances against B2.  Returns whether the lane needs its next
    // node from the stack.
    auto node_step = [&](float4 a, float4 b, float4 c, uint2 kids) -> bool {
        if (COUNT) iv++;
        const f2 d = box2_pair(a, b, c, p);
        const bool e0 = !(d.x > B2), e1 = !(d.y > B2);
        const bool both = e0 && e1, any = e0 || e1;
        const bool sel1 = e1 && (!e0 || d.y < d.x);
        const uint32_t next_ref = sel1 ? kids.y : kids.x, far_ref = sel1 ? kids.x : kids.y;
        // written either way (above the top when not pushed; entry kAnyStackLds is a scratch slot)
        col[min(sp, kAnyStackLds) * kBlock] = far_ref;
        if (__builtin_expect(both && sp >= kAnyStackLds, 0)) overflow[(sp - kAnyStackLds) * lanes + gl] = far_ref;
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
                const float4 r0 = geo[slot];
                p = {r0.x, r0.y, r0.z};
                B2 = r0.w;
                cnt = 0;
                ref = S.root_ref;
                sp = 0;
                ti = te = 0;
                bool done = !cp::finite3(p);      // count 0, nothing is tested
                if (!done) {
                    for (int i = 0; i < S.sphere_count; i++) {
                        const float4 sph = S.spheres[i];
                        rt_vec3 w;
                        float len;
                        if (COUNT) stn++;
                        const float d2 = cp::sphere_dist2(p, {sph.x, sph.y, sph.z}, sph.w, w, len);
                        if (cp::within(d2, B2)) insert(d2, i);
                    }
                    done = 0.0f > B2;             // a negative bound: the root is not entered
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
            if (cp::within(nr.dist2, B2)) insert(nr.dist2, S.sphere_count + ti);
            ti++;
            need = ti == te;
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

int nearest_k_blocks_per_cu(int &per_cu) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, nearest_k_kernel<false>, kBlock, 0));
    return RT_OK;
}

void launch_nearest_k(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint32_t *live,
                      uint32_t *queue, int k, float *ld, int32_t *li, float *point, int32_t *count_out, uint32_t *overflow,
                      Counters *ctr) {
    if (count)
        hipLaunchKernelGGL(nearest_k_kernel<true>, dim3(grid), dim3(kBlock), 0, s, ds, geo, live, queue, k, ld, li, point,
                           count_out, overflow, ctr);
    else
        hipLaunchKernelGGL(nearest_k_kernel<false>, dim3(grid), dim3(kBlock), 0, s, ds, geo, live, queue, k, ld, li, point,
                           count_out, overflow, ctr);
}

}  // namespace rtamd
