// rt_query.hip — resident ray queries (rt_query_*) and the one-shot rt_trace_rays on top of
// them: the ingest, egest, hit-record, any-hit and multi-hit kernels, the query object
// and its C ABI.
// The closest-hit traversal is the renderer's trace_kernel, compiled in rt_render.hip and launched through
// rt_common.h, as are the closest-point traversal of closest_point.hip and the nearest-k one of
// nearest_k.hip and the filtered ray queries' ingest and traversals of ray_filter.hip and the
// hemisphere query's kernels of hemisphere.hip; the refit of rt_query_update_triangles is bvh_refit.hip
// (DESIGN §12).
#include "rt_common.h"
#include "bvh_refit.h"
#include "bvh_refit_math.h"
#include "hit_record_math.h"
#include "hemisphere_math.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#pragma clang fp contract(off)

using namespace rtamd;

namespace {

// ---------------------------------------------------------------- ray queries (rt_query)
// Caller rays (n x {o.xyz, d.xyz}, 24-B stride) -> the 32-B slots the traversal kernels read:
// {o.xyz, d.x} {d.y, d.z, B, 1}.  B is the any-hit bound of the ray: tmax where tmax <= 1e30, otherwise
// (larger, +inf, NaN, or no tmax array) 1e30; trace_kernel does not read it.  Block 0 also starts the
// call: the live count, the queue shards and the work counters.
__global__ __launch_bounds__(kBlock) void query_ingest_kernel(const float *__restrict__ rays, const float *__restrict__ tmax,
                                                              uint32_t n, float4 *__restrict__ geo, uint32_t *__restrict__ live,
                                                              uint32_t *__restrict__ queue, Counters *__restrict__ ctr) {
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) live[0] = n;
        if (threadIdx.x < kQueues) queue[threadIdx.x * kQueueStride] = 0;
        unsigned long long *w = reinterpret_cast<unsigned long long *>(ctr);
        for (uint32_t k = threadIdx.x; k < kCtrSlots * (sizeof(Counters) / sizeof(unsigned long long)); k += kBlock) w[k] = 0;
    }
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *r = rays + (size_t)i * 6;
    float b = 1e30f;
    if (tmax) {
        const float v = tmax[i];
        b = v <= 1e30f ? v : 1e30f;
    }
    geo[(size_t)i * 2] = make_float4(r[0], r[1], r[2], r[3]);
    geo[(size_t)i * 2 + 1] = make_float4(r[4], r[5], b, 1.0f);
}

// trace_kernel's {t, index} records -> the caller's t[] and index[]; counts the hits (and those on spheres).
__global__ __launch_bounds__(kBlock) void query_egest_kernel(const float2 *__restrict__ hits, uint32_t n, float *__restrict__ t,
                                                             int32_t *__restrict__ index, int sphere_count,
                                                             Counters *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool hit = false, sph = false;
    if (i < n) {
        const float2 h = hits[i];
        const int idx = __float_as_int(h.y);
        t[i] = h.x;
        index[i] = idx;
        hit = idx >= 0;
        sph = hit && idx < sphere_count;
    }
    const unsigned long long nh = __popcll(__ballot(hit)), ns = __popcll(__ballot(sph));
    Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
    if (lane_id() == 0 && nh) {
        atomicAdd(&cs->hits, nh);
        if (ns) atomicAdd(&cs->hits_sphere, ns);
    }
}

// trace_kernel's {t, index} records -> the caller's hit records (rt_query_closest_hit): one thread
// per ray evaluates hit_record_math.h on the ray's slots (the o, d the traversal used) and the primitive it
// hit -- the triangle's three float4s only for index >= S, the sphere's one only for 0 <= index < S -- and
// stores the fields whose pointer is given (wave-uniform tests).  Counts like query_egest_kernel.  The n x 3
// rows are stored directly at their 12-B stride: staging a block's rows through LDS for contiguous stores
// measured no faster (24.8 against 26.0 us per 2 M rays).
__global__ __launch_bounds__(kBlock) void query_hit_egest_kernel(const float2 *__restrict__ hits, const float4 *__restrict__ geo,
                                                                 uint32_t n, const float4 *__restrict__ spheres,
                                                                 const float4 *__restrict__ tris,
                                                                 const uint16_t *__restrict__ mat_idx, int sphere_count,
                                                                 rt_hit_out out, Counters *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool is_hit = false, sph = false;
    if (i < n) {
        const float2 h = hits[i];
        const int idx = __float_as_int(h.y);
        const float4 r0 = geo[(size_t)i * 2], r1 = geo[(size_t)i * 2 + 1];
        const rt_vec3 o{r0.x, r0.y, r0.z}, d{r0.w, r1.x, r1.y};
        is_hit = idx >= 0;
        sph = is_hit && idx < sphere_count;
        hit::Record rec = hit::miss();
        if (idx >= sphere_count) {
            const float4 *tr = tris + (size_t)(idx - sphere_count) * 3;
            const float4 a = tr[0], b = tr[1], c = tr[2];
            rec = hit::triangle(o, d, h.x, {a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w, c.x}, {c.y, c.z, c.w});
        } else if (is_hit) {
            const float4 s = spheres[idx];
            rec = hit::sphere(o, d, h.x, {s.x, s.y, s.z}, s.w);
        }
        if (is_hit) rec.material = (int32_t)mat_idx[idx];
        if (out.t) out.t[i] = h.x;
        if (out.index) out.index[i] = idx;
        if (out.uv) {
            out.uv[(size_t)i * 2] = rec.u;
            out.uv[(size_t)i * 2 + 1] = rec.v;
        }
        if (out.normal) {
            float *p = out.normal + (size_t)i * 3;
            p[0] = rec.normal.x; p[1] = rec.normal.y; p[2] = rec.normal.z;
        }
        if (out.position) {
            float *p = out.position + (size_t)i * 3;
            p[0] = rec.position.x; p[1] = rec.position.y; p[2] = rec.position.z;
        }
        if (out.material) out.material[i] = rec.material;
        if (out.front_face) out.front_face[i] = rec.front_face;
    }
    const unsigned long long nh = __popcll(__ballot(is_hit)), ns = __popcll(__ballot(sph));
    Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
    if (lane_id() == 0 && nh) {
        atomicAdd(&cs->hits, nh);
        if (ns) atomicAdd(&cs->hits_sphere, ns);
    }
}

// Any hit before the ray's bound B (rt_query_occluded): the reference traversal (scene.cu:338-372,
// :134-241) with `closest` held at B and never updated; the answer is 1 iff some primitive is accepted.
// The bound never shrinks, so whether a node is entered depends on (ray, B, node) alone and the answer is
// an existence statement over a fixed node set: any visit order and an exit at the first accepted
// primitive are exact.  Hence, unlike trace_kernel, which is bound to the reference's order:
//   * the lane retires at the first accepted sphere or triangle;
//   * of two hit children the near one is entered and the far one pushed;
//   * the stack holds 4-B refs only (the push-time test `entry >= B` is the pop-time test, so a child that
//     fails it is never pushed): 16 LDS entries + the scratch slot = 17 KB, deeper ones in `overflow`.
// Queue, ballot refill, scalar root record, one record load per step and the literal slab fold for lanes
// with a non-finite 1/d are trace_kernel's.  out[slot] = 0 or 1, stored at refill and at exit like hits[].
// Counters (COUNT): Pn = nodes entered, Iv = internal nodes stepped, Tt = triangle tests, sphere tests up
// to the first accepted sphere -- the oracle's numbers on unoccluded rays, order-dependent on occluded ones.
// The order is a function of (ray, B, tree) alone: spheres in order; the root; at an internal node child 1
// (the record's second) goes first iff it is entered and child 0 is not or t1 < t0 (a tie goes to child 0),
// the other one is pushed iff both are entered; a leaf's triangles in order; an exhausted leaf, or a node
// with no entered child, pops.  tests/anyhit_ref.py (AnyHitOrderRef) restates it and
// tests/test_gpu_anyhit_order.py pins the counters to it on all rays, occluded ones included.
// (kAnyStackLds is rt_common.h's: nearest_k.hip uses the same stack.)

template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void anyhit_kernel(DevScene S, const float4 *__restrict__ geo,
                                                                      const uint32_t *__restrict__ live_count,
                                                                      uint32_t *__restrict__ queue, uint8_t *__restrict__ out,
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
    int slot = -1;                      // < 0: lane has no ray; <= -2: done with slot -2 - slot, `occ` not yet stored
    V3 o{0, 0, 0}, d{0, 0, 0};
    float ix = 0, iy = 0, iz = 0, B = 0;
    bool finite_inv = true;
    bool wave_nonfinite = false;
    int sp = 0;
    uint32_t ref = 0, occ = 0;
    int ti = 0, te = 0;                 // the lane is in a leaf while ti < te
    unsigned pn = 0, iv = 0, tt = 0, stn = 0, nocc = 0;
    // One internal node's step: both children's slabs against B; a child is entered iff its box is hit
    // and !(entry >= B) (scene.cu:196-225 with :147-152 applied at push time).  Returns whether the lane
    // needs its next node from the stack.
    auto node_step = [&](float4 a, float4 b, float4 c, uint2 kids) -> bool {
        if (COUNT) iv++;
        float t0, t1;
        bool h0, h1;
        slab_pair(a, b, c, o, ix, iy, iz, B, h0, h1, t0, t1);
        if (__builtin_expect(wave_nonfinite, 0)) {
            float u0, u1;
            const bool g0 = slab(a.x, a.z, b.x, b.z, c.x, c.z, o, ix, iy, iz, B, u0);
            const bool g1 = slab(a.y, a.w, b.y, b.w, c.y, c.w, o, ix, iy, iz, B, u1);
            if (!finite_inv) { h0 = g0; h1 = g1; t0 = u0; t1 = u1; }
        }
        const bool e0 = h0 && !(t0 >= B), e1 = h1 && !(t1 >= B);
        const bool both = e0 && e1, any = e0 || e1;
        // next = child 1 iff it is the nearer of two entered children or the only one
        const bool sel1 = e1 && (!e0 || t1 < t0);
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
    // Pop: every entry on the stack is entered (it passed the bound test when it was pushed); an empty
    // stack ends the ray unoccluded.
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
            if (slot <= -2) {             // answers of the lanes that finished since the last refill
                out[-2 - slot] = (uint8_t)occ;
                nocc += occ;
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
                const float4 *rp = geo + (size_t)slot * 2;
                const float4 r0 = rp[0], r1 = rp[1];
                o = v3(r0.x, r0.y, r0.z);
                d = v3(r0.w, r1.x, r1.y);
                B = r1.z;
                ix = 1 / d.x; iy = 1 / d.y; iz = 1 / d.z;
                finite_inv = __builtin_isfinite(ix) && __builtin_isfinite(iy) && __builtin_isfinite(iz);
                occ = 0;
                for (int i = 0; i < S.sphere_count; i++) {
                    const float4 sph = S.spheres[i];
                    float t;
                    if (COUNT) stn++;
                    if (ray_sphere(o, d, v3(sph.x, sph.y, sph.z), sph.w, B, t)) { occ = 1; break; }
                }
                ref = S.root_ref;
                sp = 0;
                ti = te = 0;
                // the root is popped with distance 0: entered iff !(0 >= B) (scene.cu:147-152)
                bool done = occ || 0.0f >= B;
                if (!done) {
                    if (COUNT) pn++;
                    if (ref & kLeaf) {
                        leaf_range(S, ref, ti, te);
                        done = ti == te;    // no triangles at all: spheres only
                    }
                }
                if (done) {
                    out[slot] = (uint8_t)occ;
                    nocc += occ;
                    slot = -1;
                }
            }
            wave_nonfinite = __ballot(slot >= 0 && !finite_inv) != 0;
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
        // ---- one step: one triangle test of the current leaf, or one internal node; the record is read
        // through the same loads either way (see trace_kernel)
        bool need = false;
        const bool in_leaf = ti < te;
        const float4 *rec = in_leaf ? S.tris + (size_t)ti * 3 : S.nodes + (size_t)ref * 4;
        const float4 a = rec[0], b = rec[1], c = rec[2];
        uint2 kids = make_uint2(0, 0);
        if (!in_leaf) kids = *reinterpret_cast<const uint2 *>(rec + 3);
        if (in_leaf) {
            if (COUNT) tt++;
            float t;
            const bool hit = ray_triangle_flat(o, d, v3(a.x, a.y, a.z), v3(a.w, b.x, b.y), v3(b.z, b.w, c.x), B, t);
            ti++;
            if (hit) {                    // the first accepted triangle ends the ray
                occ = 1;
                slot = -2 - slot;
                ti = te = 0;
            } else {
                need = ti == te;
            }
        } else {
            need = node_step(a, b, c, kids);
        }
        pop_loop(need);
    }
    if (slot <= -2) {
        out[-2 - slot] = (uint8_t)occ;
        nocc += occ;
    }
    Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
    const unsigned long long no = wave_sum(nocc);
    if (COUNT) {
        const unsigned long long a = wave_sum(pn), b = wave_sum(iv), t = wave_sum(tt), s = wave_sum(stn);
        if (lane_id() == 0) {
            atomicAdd(&cs->pn, a);
            atomicAdd(&cs->iv, b);
            atomicAdd(&cs->tt, t);
            atomicAdd(&cs->st, s);
        }
    }
    if (lane_id() == 0 && no) atomicAdd(&cs->hits, no);
}

// Every hit before the ray's bound B (rt_query_multi_hit): anyhit_kernel's traversal -- the same
// predicates with `closest` held at B, the same queue, refill, root step, record load, slab fold, near-first
// order and 4-B stack -- without its exits: the sphere loop runs to the end and a lane retires only when its
// stack is empty, so it enumerates the whole accepted set, which is fixed whatever the order.
// An accepted (t, index) is inserted into the ray's list of its K smallest hits by the key (t', index), t' =
// t's bits with every NaN as 0x7FC00000 (accepted t is NaN or >= 0.005: unsigned order is numeric order, NaNs
// last).  The list lives in rows slot*K.. of lt[] and li[] -- the caller's t and index arrays, or the object's
// scratch for the one the caller left out -- and the lane reads and writes only its own earlier stores.  It
// keeps its count and the key of its K-th record in registers: once the list is full a hit that is not below
// that key costs one compare.  With lt == nullptr (wave-uniform) nothing is kept and the lane only counts.
// At retire the lane pads entries [min(count, K), K) with (1e30, -1) and stores the count; like anyhit_kernel's
// answers these stores wait for the lane's next refill.
// Counters (COUNT): Pn, Iv, Tt and S sphere tests per ray of the full traversal, order-independent.
// The loop, node_step and pop_loop are anyhit_kernel's text, repeated here and not shared through a template:
// anyhit_kernel has to compile to the registers and occupancy it was tuned at (profiles/multihit/kernel_resources.txt).
__device__ __forceinline__ uint32_t multihit_key(float t) { return t != t ? 0x7FC00000u : __float_as_uint(t); }

template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void multihit_kernel(DevScene S, const float4 *__restrict__ geo,
                                                                        const uint32_t *__restrict__ live_count,
                                                                        uint32_t *__restrict__ queue, int K, float *lt,
                                                                        int32_t *li, int32_t *__restrict__ count_out,
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
    int slot = -1;                      // < 0: lane has no ray; <= -2: done with slot -2 - slot, row not yet finished
    V3 o{0, 0, 0}, d{0, 0, 0};
    float ix = 0, iy = 0, iz = 0, B = 0;
    bool finite_inv = true;
    bool wave_nonfinite = false;
    int sp = 0;
    uint32_t ref = 0;
    int ti = 0, te = 0;                 // the lane is in a leaf while ti < te
    int cnt = 0;                        // accepted primitives of the lane's ray so far
    uint32_t kth_key = 0;               // key of list entry K - 1, valid once cnt >= K
    int kth_idx = 0;
    unsigned pn = 0, iv = 0, tt = 0, stn = 0, nhit = 0;
    const bool keep = lt != nullptr;
    // One accepted primitive of the lane's ray `slot` (>= 0).
    auto insert = [&](float t, int idx) {
        if (keep) {
            const uint32_t key = multihit_key(t);
            int j = -1;                 // the entry the new record would take before any shift
            if (cnt < K) j = cnt;
            else if (key < kth_key || (key == kth_key && idx < kth_idx)) j = K - 1;
            if (j >= 0) {
                float *rt = lt + (size_t)slot * K;
                int32_t *ri = li + (size_t)slot * K;
                while (j > 0) {
                    const float pt = rt[j - 1];
                    const int pi = ri[j - 1];
                    const uint32_t pk = multihit_key(pt);
                    if (!(pk > key || (pk == key && pi > idx))) break;
                    if (j == K - 1) { kth_key = pk; kth_idx = pi; }
                    rt[j] = pt;
                    ri[j] = pi;
                    j--;
                }
                if (j == K - 1) { kth_key = key; kth_idx = idx; }
                rt[j] = t;
                ri[j] = idx;
            }
        }
        cnt++;
    };
    // The row of a finished ray: padding and count.
    auto finish = [&](int s) {
        if (keep) {
            for (int j = min(cnt, K); j < K; j++) {
                lt[(size_t)s * K + j] = 1e30f;
                li[(size_t)s * K + j] = -1;
            }
        }
        if (count_out) count_out[s] = cnt;
        nhit += cnt > 0 ? 1u : 0u;
    };
    auto node_step = [&](float4 a, float4 b, float4 c, uint2 kids) -> bool {
        if (COUNT) iv++;
        float t0, t1;
        bool h0, h1;
        slab_pair(a, b, c, o, ix, iy, iz, B, h0, h1, t0, t1);
        if (__builtin_expect(wave_nonfinite, 0)) {
            float u0, u1;
            const bool g0 = slab(a.x, a.z, b.x, b.z, c.x, c.z, o, ix, iy, iz, B, u0);
            const bool g1 = slab(a.y, a.w, b.y, b.w, c.y, c.w, o, ix, iy, iz, B, u1);
            if (!finite_inv) { h0 = g0; h1 = g1; t0 = u0; t1 = u1; }
        }
        const bool e0 = h0 && !(t0 >= B), e1 = h1 && !(t1 >= B);
        const bool both = e0 && e1, any = e0 || e1;
        const bool sel1 = e1 && (!e0 || t1 < t0);
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
    // Pop: every entry on the stack is entered; an empty stack ends the ray.
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
                const float4 *rp = geo + (size_t)slot * 2;
                const float4 r0 = rp[0], r1 = rp[1];
                o = v3(r0.x, r0.y, r0.z);
                d = v3(r0.w, r1.x, r1.y);
                B = r1.z;
                ix = 1 / d.x; iy = 1 / d.y; iz = 1 / d.z;
                finite_inv = __builtin_isfinite(ix) && __builtin_isfinite(iy) && __builtin_isfinite(iz);
                cnt = 0;
                for (int i = 0; i < S.sphere_count; i++) {
                    const float4 sph = S.spheres[i];
                    float t;
                    if (COUNT) stn++;
                    if (ray_sphere(o, d, v3(sph.x, sph.y, sph.z), sph.w, B, t)) insert(t, i);
                }
                ref = S.root_ref;
                sp = 0;
                ti = te = 0;
                // the root is popped with distance 0: entered iff !(0 >= B) (scene.cu:147-152)
                bool done = 0.0f >= B;
                if (!done) {
                    if (COUNT) pn++;
                    if (ref & kLeaf) {
                        leaf_range(S, ref, ti, te);
                        done = ti == te;    // no triangles at all: spheres only
                    }
                }
                if (done) {
                    finish(slot);
                    slot = -1;
                }
            }
            wave_nonfinite = __ballot(slot >= 0 && !finite_inv) != 0;
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
        // ---- one step: one triangle test of the current leaf, or one internal node; the record is read
        // through the same loads either way (see trace_kernel)
        bool need = false;
        const bool in_leaf = ti < te;
        const float4 *rec = in_leaf ? S.tris + (size_t)ti * 3 : S.nodes + (size_t)ref * 4;
        const float4 a = rec[0], b = rec[1], c = rec[2];
        uint2 kids = make_uint2(0, 0);
        if (!in_leaf) kids = *reinterpret_cast<const uint2 *>(rec + 3);
        if (in_leaf) {
            if (COUNT) tt++;
            float t;
            const bool hit = ray_triangle_flat(o, d, v3(a.x, a.y, a.z), v3(a.w, b.x, b.y), v3(b.z, b.w, c.x), B, t);
            if (hit) insert(t, S.sphere_count + ti);
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

// Resident ray queries (rt_query_*): the resident scene, a stream for the host-pointer calls, and the
// scratch of one call -- the repacked rays, trace_kernel's {t, index} records, the live count and queue
// words, the overflow stacks -- kept between calls.  The device-pointer calls enqueue on the caller's stream
// and, once the scratch holds n rays, allocate nothing and never wait on the host.  Calls share the scratch,
// so each records `last` and the next call's stream waits for it; a regrow waits for it on the host
// before the old scratch is freed.
struct rt_query {
    SceneDev scene;
    hipStream_t stream = nullptr;     // the host-pointer calls' (and init's uploads')
    bool counters = false;            // rt_opts.collect_counters: the COUNT builds of the traversal kernels
    int blocks = 0;                   // most workgroups any of the traversal kernels keeps resident
    size_t cap = 0;                   // rays the scratch holds
    DevBuf<float4> geo;
    DevBuf<float2> hits;
    DevBuf<uint32_t> words, overflow; // words: live count, then the queue shards
    // staging of the host-pointer calls
    size_t host_cap = 0;
    DevBuf<float> s_rays, s_tmax, s_t;
    DevBuf<int32_t> s_index;
    DevBuf<uint8_t> s_occ;
    size_t host_hit_cap = 0;          // closest_hit_host's further staging: uv | normal | position, material
    DevBuf<float> s_hit;
    DevBuf<int32_t> s_mat;
    // multi_hit: the list words of the output the caller left out (t or index, n*k each), and
    // multi_hit_host's staging of t and index (n*k each) and count (n)
    size_t list_cap = 0, host_list_cap = 0;
    DevBuf<float> list_t, s_list_t;
    DevBuf<int32_t> list_i, s_list_i, s_count;
    // nearest_k shares those; nearest_k_host's staging of point (n*k*3)
    size_t host_point_cap = 0;
    DevBuf<float> s_list_p;
    // the filtered ray queries: {skip, ray mask} per ray, grown with geo and hits; the primitive
    // mask words (S + T, allocated in init, read by the kernels only while has_masks); the host calls' staging
    DevBuf<uint2> fil;
    DevBuf<uint32_t> masks;
    bool has_masks = false;
    int32_t prim_count = 0;           // S + T
    size_t host_filter_cap = 0;
    DevBuf<float> s_tmin;
    DevBuf<int32_t> s_skip;
    DevBuf<uint32_t> s_rmask;
    hipEvent_t last = nullptr;
    bool pending = false;             // `last` has been recorded
    int last_kind = 0;                // 0 none (an update, set_masks), 1 closest, 2 occluded, 3 multi_hit, 4 closest_point,
                                      // 5 nearest_k, 6 closest_filtered, 7 occluded_filtered, 8 hemisphere, 9 overlap_box
    int32_t last_n = 0;
    rtamd::RefitPlan plan;            // rt_query_update_triangles: level tables, built in init

    ~rt_query() {
        (void)hipSetDevice(scene.device);
        if (last) {
            if (pending) (void)hipEventSynchronize(last);
            (void)hipEventDestroy(last);
        }
        if (stream) (void)hipStreamDestroy(stream);
    }
    uint32_t *live() const { return words.p; }
    uint32_t *queue() const { return words.p + kQueueStride; }

    // o: checked by resolve_opts
    int init(const rt_scene *sc, const rt_opts *o) {
        scene.device = o->device;       // the destructor's, should init stop before scene.init
        counters = o->collect_counters != 0;
        HIPCHK(hipSetDevice(o->device));
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        int rc = scene.init(sc, o->device, stream);
        if (rc) return rc;
        int per_cu_c = 0, per_cu_a = 0, per_cu_m = 0, per_cu_p = 0, per_cu_n = 0, per_cu_fc = 0, per_cu_fa = 0, per_cu_h = 0;
        int per_cu_o = 0;
        if ((rc = trace_closest_blocks_per_cu(per_cu_c)) || (rc = closest_point_blocks_per_cu(per_cu_p)) ||
            (rc = nearest_k_blocks_per_cu(per_cu_n)) || (rc = ray_filter_blocks_per_cu(per_cu_fc, per_cu_fa)) ||
            (rc = hemisphere_blocks_per_cu(per_cu_h)) || (rc = box_overlap_blocks_per_cu(per_cu_o)))
            return rc;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_a, anyhit_kernel<false>, kBlock, 0));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_m, multihit_kernel<false>, kBlock, 0));
        blocks = std::max(1, scene.cus * std::max({1, per_cu_c, per_cu_a, per_cu_m, per_cu_p, per_cu_n, per_cu_fc, per_cu_fa, per_cu_h, per_cu_o}));
        prim_count = sc->sphere_count + sc->triangle_count;
        if ((rc = masks.alloc((size_t)prim_count))) return rc;
        HIPCHK(hipEventCreateWithFlags(&last, hipEventDisableTiming));
        if ((rc = words.alloc((size_t)(1 + kQueues) * kQueueStride))) return rc;
        if ((rc = plan.build(sc, scene.node_rec, stream))) return rc;
        // trace_kernel and filtered_closest_kernel: 2 words (ref, distance) for each of kStackMax - kStackLds entries
        // per lane; the any-hit, multi-hit, nearest-k, filtered any-hit, hemisphere and box-overlap kernels' kStackMax - kAnyStackLds one-word
        // entries fit in the same buffer
        return overflow.alloc((size_t)blocks * kBlock * 2 * (kStackMax - kStackLds));
    }
    int wait_last() {
        if (pending) HIPCHK(hipEventSynchronize(last));
        return RT_OK;
    }
    int reserve(int64_t n) {
        if ((size_t)n <= cap) return RT_OK;
        HIPCHK(hipSetDevice(scene.device));
        int rc = wait_last();           // the last call may still read the old scratch
        if (rc) return rc;
        const size_t want = std::max<size_t>({(size_t)n, 2 * cap, (size_t)kBlock});
        cap = 0;
        if ((rc = geo.alloc(want * 2)) || (rc = hits.alloc(want)) || (rc = fil.alloc(want))) return rc;
        cap = want;
        return RT_OK;
    }
    int begin(const float *d_rays, const float *d_tmax, int n, hipStream_t s) {
        HIPCHK(hipSetDevice(scene.device));
        int rc = reserve(n);
        if (rc) return rc;
        if (pending) HIPCHK(hipStreamWaitEvent(s, last, 0));
        hipLaunchKernelGGL(query_ingest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, d_rays, d_tmax, (uint32_t)n, geo.p,
                           live(), queue(), scene.ctr.p);
        return RT_OK;
    }
    int end(int kind, int n, hipStream_t s) {
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(last, s));
        pending = true;
        last_kind = kind;
        last_n = n;
        return RT_OK;
    }
    int closest(const float *d_rays, int n, float *d_t, int32_t *d_index, hipStream_t s) {
        int rc = begin(d_rays, nullptr, n, s);
        if (rc) return rc;
        launch_trace_closest(counters, std::min(blocks_for(n), blocks), s, scene.ds, geo.p, live(), queue(), hits.p,
                             overflow.p, scene.ctr.p);
        hipLaunchKernelGGL(query_egest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, hits.p, (uint32_t)n, d_t, d_index,
                           scene.ds.sphere_count, scene.ctr.p);
        return end(1, n, s);
    }
    // closest with query_hit_egest_kernel in query_egest_kernel's place: the same counters and stats
    int closest_hit(const float *d_rays, int n, const rt_hit_out &out, hipStream_t s) {
        int rc = begin(d_rays, nullptr, n, s);
        if (rc) return rc;
        launch_trace_closest(counters, std::min(blocks_for(n), blocks), s, scene.ds, geo.p, live(), queue(), hits.p,
                             overflow.p, scene.ctr.p);
        hipLaunchKernelGGL(query_hit_egest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, hits.p, geo.p, (uint32_t)n,
                           scene.ds.spheres, scene.ds.tris, scene.ds.mat_idx, scene.ds.sphere_count, out, scene.ctr.p);
        return end(1, n, s);
    }
    int occluded(const float *d_rays, const float *d_tmax, int n, uint8_t *d_occ, hipStream_t s) {
        int rc = begin(d_rays, d_tmax, n, s);
        if (rc) return rc;
        const int grid = std::min(blocks_for(n), blocks);
        if (counters)
            hipLaunchKernelGGL(anyhit_kernel<true>, dim3(grid), dim3(kBlock), 0, s, scene.ds, geo.p, live(), queue(), d_occ,
                               overflow.p, scene.ctr.p);
        else
            hipLaunchKernelGGL(anyhit_kernel<false>, dim3(grid), dim3(kBlock), 0, s, scene.ds, geo.p, live(), queue(), d_occ,
                               overflow.p, scene.ctr.p);
        return end(2, n, s);
    }
    // All hits before the bound, the k nearest kept.  The kernel keeps each ray's list in the
    // caller's rows; an output the caller left out is replaced by the object's scratch when the other one is
    // asked for, and with neither the kernel only counts.
    int multi_hit(const float *d_rays, const float *d_tmax, int n, int k, const rt_multi_hit_out &out, hipStream_t s) {
        float *lt = out.t;
        int32_t *li = out.index;
        if ((lt != nullptr) != (li != nullptr)) {
            const size_t need = (size_t)n * k;
            if (need > list_cap) {
                HIPCHK(hipSetDevice(scene.device));
                int rc = wait_last();       // the last call may still use the old lists
                if (rc) return rc;
                const size_t want = std::max(need, 2 * list_cap);
                list_cap = 0;
                if ((rc = list_t.alloc(want)) || (rc = list_i.alloc(want))) return rc;
                list_cap = want;
            }
            if (!lt) lt = list_t.p;
            if (!li) li = list_i.p;
        }
        int rc = begin(d_rays, d_tmax, n, s);
        if (rc) return rc;
        const int grid = std::min(blocks_for(n), blocks);
        if (counters)
            hipLaunchKernelGGL(multihit_kernel<true>, dim3(grid), dim3(kBlock), 0, s, scene.ds, geo.p, live(), queue(), k, lt,
                               li, out.count, overflow.p, scene.ctr.p);
        else
            hipLaunchKernelGGL(multihit_kernel<false>, dim3(grid), dim3(kBlock), 0, s, scene.ds, geo.p, live(), queue(), k, lt,
                               li, out.count, overflow.p, scene.ctr.p);
        return end(3, n, s);
    }
    int multi_hit_host(const float *rays, const float *tmax, int n, int k, const rt_multi_hit_out &out) {
        int rc = reserve_host(n);
        if (rc) return rc;
        const size_t m = (size_t)n * k;
        if (m > host_list_cap) {
            HIPCHK(hipSetDevice(scene.device));
            const size_t want = std::max(m, 2 * host_list_cap);
            host_list_cap = 0;              // the host calls are blocking: nothing reads the old staging
            if ((rc = s_list_t.alloc(want)) || (rc = s_list_i.alloc(want))) return rc;
            host_list_cap = want;
        }
        if (s_count.n < host_cap && (rc = s_count.alloc(host_cap))) return rc;
        hipStream_t s = stream;
        rt_multi_hit_out d{};
        if (out.t) d.t = s_list_t.p;
        if (out.index) d.index = s_list_i.p;
        if (out.count) d.count = s_count.p;
        HIPCHK(hipMemcpyAsync(s_rays.p, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, s));
        if (tmax) HIPCHK(hipMemcpyAsync(s_tmax.p, tmax, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = multi_hit(s_rays.p, tmax ? s_tmax.p : nullptr, n, k, d, s))) return rc;
        if (out.t) HIPCHK(hipMemcpyAsync(out.t, d.t, m * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.index) HIPCHK(hipMemcpyAsync(out.index, d.index, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.count) HIPCHK(hipMemcpyAsync(out.count, d.count, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    // The nearest surface point of each point: closest_point.hip's ingest and traversal in the
    // scratch of the ray queries (one float4 slot per point, the same queue words and overflow buffer).
    int closest_point(const float *d_points, const float *d_max_dist, int n, const rt_closest_point_out &out, hipStream_t s) {
        HIPCHK(hipSetDevice(scene.device));
        int rc = reserve(n);
        if (rc) return rc;
        if (pending) HIPCHK(hipStreamWaitEvent(s, last, 0));
        launch_closest_point(counters, n, std::min(blocks_for(n), blocks), s, scene.ds, d_points, d_max_dist, geo.p, live(),
                             queue(), out, overflow.p, scene.ctr.p);
        return end(4, n, s);
    }
    int closest_point_host(const float *points, const float *max_dist, int n, const rt_closest_point_out &out) {
        int rc = reserve_host_hit(n);
        if (rc) return rc;
        hipStream_t s = stream;
        rt_closest_point_out d{};
        if (out.distance) d.distance = s_t.p;
        if (out.index) d.index = s_index.p;
        if (out.uv) d.uv = s_hit.p;
        if (out.point) d.point = s_hit.p + 2 * host_hit_cap;
        HIPCHK(hipMemcpyAsync(s_rays.p, points, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
        if (max_dist) HIPCHK(hipMemcpyAsync(s_tmax.p, max_dist, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = closest_point(s_rays.p, max_dist ? s_tmax.p : nullptr, n, d, s))) return rc;
        const size_t m = (size_t)n;
        if (out.distance) HIPCHK(hipMemcpyAsync(out.distance, d.distance, m * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.index) HIPCHK(hipMemcpyAsync(out.index, d.index, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.uv) HIPCHK(hipMemcpyAsync(out.uv, d.uv, m * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.point) HIPCHK(hipMemcpyAsync(out.point, d.point, m * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    // Every primitive within max_dist, the k nearest kept.  The kernel keeps each point's list
    // (dist2, index) in the caller's distance and index rows; a half the caller left out lives in the multi-hit list
    // scratch when any of distance, index and point is asked for, and with none of them the kernel only counts.
    int nearest_k(const float *d_points, const float *d_max_dist, int n, int k, const rt_nearest_k_out &out, hipStream_t s) {
        float *ld = out.distance;
        int32_t *li = out.index;
        const bool keep = ld || li || out.point;
        if (keep && (!ld || !li)) {
            const size_t need = (size_t)n * k;
            if (need > list_cap) {
                HIPCHK(hipSetDevice(scene.device));
                int rc = wait_last();       // the last call may still use the old lists
                if (rc) return rc;
                const size_t want = std::max(need, 2 * list_cap);
                list_cap = 0;
                if ((rc = list_t.alloc(want)) || (rc = list_i.alloc(want))) return rc;
                list_cap = want;
            }
            if (!ld) ld = list_t.p;
            if (!li) li = list_i.p;
        }
        HIPCHK(hipSetDevice(scene.device));
        int rc = reserve(n);
        if (rc) return rc;
        if (pending) HIPCHK(hipStreamWaitEvent(s, last, 0));
        launch_point_ingest(n, s, d_points, d_max_dist, geo.p, live(), queue(), scene.ctr.p);
        launch_nearest_k(counters, std::min(blocks_for(n), blocks), s, scene.ds, geo.p, live(), queue(), k, ld, li, out.point,
                         out.count, overflow.p, scene.ctr.p);
        return end(5, n, s);
    }
    int nearest_k_host(const float *points, const float *max_dist, int n, int k, const rt_nearest_k_out &out) {
        int rc = reserve_host(n);
        if (rc) return rc;
        const size_t m = (size_t)n * k;
        if (m > host_list_cap) {
            HIPCHK(hipSetDevice(scene.device));
            const size_t want = std::max(m, 2 * host_list_cap);
            host_list_cap = 0;              // the host calls are blocking: nothing reads the old staging
            if ((rc = s_list_t.alloc(want)) || (rc = s_list_i.alloc(want))) return rc;
            host_list_cap = want;
        }
        if (out.point && m > host_point_cap) {
            HIPCHK(hipSetDevice(scene.device));
            const size_t want = std::max(m, 2 * host_point_cap);
            host_point_cap = 0;
            if ((rc = s_list_p.alloc(want * 3))) return rc;
            host_point_cap = want;
        }
        if (s_count.n < host_cap && (rc = s_count.alloc(host_cap))) return rc;
        hipStream_t s = stream;
        rt_nearest_k_out d{};
        if (out.distance) d.distance = s_list_t.p;
        if (out.index) d.index = s_list_i.p;
        if (out.point) d.point = s_list_p.p;
        if (out.count) d.count = s_count.p;
        HIPCHK(hipMemcpyAsync(s_rays.p, points, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
        if (max_dist) HIPCHK(hipMemcpyAsync(s_tmax.p, max_dist, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = nearest_k(s_rays.p, max_dist ? s_tmax.p : nullptr, n, k, d, s))) return rc;
        if (out.distance) HIPCHK(hipMemcpyAsync(out.distance, d.distance, m * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.index) HIPCHK(hipMemcpyAsync(out.index, d.index, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.point) HIPCHK(hipMemcpyAsync(out.point, d.point, m * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.count) HIPCHK(hipMemcpyAsync(out.count, d.count, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    // Every primitive that meets a box, the k smallest indices kept: box_overlap.hip's ingest and traversal in
    // the scratch of the ray queries (two float4 of geo per box, the same queue words and overflow buffer).  The kernel
    // keeps each box's list in the caller's index rows; without them nothing is kept.
    int overlap_box(const float *d_boxes, int n, int k, const rt_overlap_out &out, hipStream_t s) {
        HIPCHK(hipSetDevice(scene.device));
        int rc = reserve(n);
        if (rc) return rc;
        if (pending) HIPCHK(hipStreamWaitEvent(s, last, 0));
        launch_box_ingest(n, s, d_boxes, geo.p, live(), queue(), scene.ctr.p);
        launch_box_overlap(counters, std::min(blocks_for(n), blocks), s, scene.ds, geo.p, live(), queue(), k, out, overflow.p,
                           scene.ctr.p);
        return end(9, n, s);
    }
    int overlap_box_host(const float *boxes, int n, int k, const rt_overlap_out &out) {
        int rc = reserve_host(n);
        if (rc) return rc;
        const size_t m = (size_t)n * k;
        if (out.index && m > host_list_cap) {
            HIPCHK(hipSetDevice(scene.device));
            const size_t want = std::max(m, 2 * host_list_cap);
            host_list_cap = 0;              // the host calls are blocking: nothing reads the old staging
            if ((rc = s_list_t.alloc(want)) || (rc = s_list_i.alloc(want))) return rc;
            host_list_cap = want;
        }
        if (s_count.n < host_cap && (rc = s_count.alloc(host_cap))) return rc;
        hipStream_t s = stream;
        rt_overlap_out d{};
        if (out.index) d.index = s_list_i.p;
        if (out.count) d.count = s_count.p;
        if (out.any) d.any = s_occ.p;
        HIPCHK(hipMemcpyAsync(s_rays.p, boxes, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = overlap_box(s_rays.p, n, k, d, s))) return rc;
        if (out.index) HIPCHK(hipMemcpyAsync(out.index, d.index, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.count) HIPCHK(hipMemcpyAsync(out.count, d.count, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.any) HIPCHK(hipMemcpyAsync(out.any, d.any, (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    // The filtered ray queries: ray_filter.hip's ingest and traversals in the scratch of the ray queries;
    // the closest one's {t, index} records go through the egest kernel of closest_hit.
    int begin_filtered(const float *d_rays, const rt_ray_filter &f, int n, hipStream_t s) {
        HIPCHK(hipSetDevice(scene.device));
        int rc = reserve(n);
        if (rc) return rc;
        if (pending) HIPCHK(hipStreamWaitEvent(s, last, 0));
        launch_filter_ingest(n, s, d_rays, f, geo.p, fil.p, live(), queue(), scene.ctr.p);
        return RT_OK;
    }
    int closest_filtered(const float *d_rays, const rt_ray_filter &f, int n, const rt_hit_out &out, hipStream_t s) {
        int rc = begin_filtered(d_rays, f, n, s);
        if (rc) return rc;
        launch_filtered_closest(counters, std::min(blocks_for(n), blocks), s, scene.ds, geo.p, fil.p,
                                has_masks ? masks.p : nullptr, live(), queue(), hits.p, overflow.p, scene.ctr.p);
        hipLaunchKernelGGL(query_hit_egest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, hits.p, geo.p, (uint32_t)n,
                           scene.ds.spheres, scene.ds.tris, scene.ds.mat_idx, scene.ds.sphere_count, out, scene.ctr.p);
        return end(6, n, s);
    }
    int occluded_filtered(const float *d_rays, const rt_ray_filter &f, int n, uint8_t *d_occ, hipStream_t s) {
        int rc = begin_filtered(d_rays, f, n, s);
        if (rc) return rc;
        launch_filtered_anyhit(counters, std::min(blocks_for(n), blocks), s, scene.ds, geo.p, fil.p,
                               has_masks ? masks.p : nullptr, live(), queue(), d_occ, overflow.p, scene.ctr.p);
        return end(7, n, s);
    }
    // The hemisphere query: hemisphere.hip's ingest, traversal and egest in the scratch of the ray queries,
    // one slot and one filter row per point; the points' counts live in the first word of their `hits` records, so the
    // scratch grows with n, not with n * S.  p and out: checked by hemisphere_args.
    int hemisphere(const float *d_frames, const rt_ray_filter &f, int n, const rt_hemisphere_params &p,
                   const rt_hemisphere_out &out, hipStream_t s) {
        HIPCHK(hipSetDevice(scene.device));
        int rc = reserve(n);
        if (rc) return rc;
        if (pending) HIPCHK(hipStreamWaitEvent(s, last, 0));
        const int64_t work = (int64_t)n * p.samples;
        uint32_t *count = reinterpret_cast<uint32_t *>(hits.p);
        launch_hemisphere_ingest(n, s, d_frames, f, (uint32_t)work, geo.p, fil.p, count, live(), queue(), scene.ctr.p);
        launch_hemisphere(counters, std::min(blocks_for(work), blocks), s, scene.ds, geo.p, fil.p,
                          has_masks ? masks.p : nullptr, live(), queue(), count, p, overflow.p, scene.ctr.p);
        launch_hemisphere_egest(n, s, count, p.samples, out);
        return end(8, (int)work, s);
    }
    int hemisphere_host(const float *frames, const rt_ray_filter &f, int n, const rt_hemisphere_params &p,
                        const rt_hemisphere_out &out) {
        int rc = reserve_host(n);
        if (rc) return rc;
        hipStream_t s = stream;
        rt_ray_filter df{};
        if ((rc = stage_filter(frames, f, n, df))) return rc;
        rt_hemisphere_out d{};
        if (out.open_count) d.open_count = s_index.p;
        if (out.openness) d.openness = s_t.p;
        if ((rc = hemisphere(s_rays.p, df, n, p, d, s))) return rc;
        const size_t m = (size_t)n;
        if (out.open_count) HIPCHK(hipMemcpyAsync(out.open_count, d.open_count, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.openness) HIPCHK(hipMemcpyAsync(out.openness, d.openness, m * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    // The primitive mask words: a copy on s into the object's buffer, in the event chain like an update.
    int set_masks(const uint32_t *m, bool on_host, hipStream_t s) {
        HIPCHK(hipSetDevice(scene.device));
        if (pending) HIPCHK(hipStreamWaitEvent(s, last, 0));
        if (m && prim_count)
            HIPCHK(hipMemcpyAsync(masks.p, m, (size_t)prim_count * sizeof(uint32_t),
                                  on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
        has_masks = m != nullptr && prim_count > 0;
        int rc = end(0, 0, s);
        if (rc || !on_host) return rc;
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    // Stages the host filter's members behind the rays; d receives the device pointers.
    int stage_filter(const float *rays, const rt_ray_filter &f, int n, rt_ray_filter &d) {
        hipStream_t s = stream;
        if ((size_t)n > host_filter_cap) {
            HIPCHK(hipSetDevice(scene.device));
            const size_t want = std::max<size_t>({(size_t)n, 2 * host_filter_cap, (size_t)kBlock});
            host_filter_cap = 0;            // the host calls are blocking: nothing reads the old staging
            int rc;
            if ((rc = s_tmin.alloc(want)) || (rc = s_skip.alloc(want)) || (rc = s_rmask.alloc(want))) return rc;
            host_filter_cap = want;
        }
        const size_t m = (size_t)n;
        d = rt_ray_filter{};
        HIPCHK(hipMemcpyAsync(s_rays.p, rays, m * 6 * sizeof(float), hipMemcpyHostToDevice, s));
        if (f.tmin) {
            HIPCHK(hipMemcpyAsync(s_tmin.p, f.tmin, m * sizeof(float), hipMemcpyHostToDevice, s));
            d.tmin = s_tmin.p;
        }
        if (f.tmax) {
            HIPCHK(hipMemcpyAsync(s_tmax.p, f.tmax, m * sizeof(float), hipMemcpyHostToDevice, s));
            d.tmax = s_tmax.p;
        }
        if (f.skip) {
            HIPCHK(hipMemcpyAsync(s_skip.p, f.skip, m * sizeof(int32_t), hipMemcpyHostToDevice, s));
            d.skip = s_skip.p;
        }
        if (f.mask) {
            HIPCHK(hipMemcpyAsync(s_rmask.p, f.mask, m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            d.mask = s_rmask.p;
        }
        return RT_OK;
    }
    int closest_filtered_host(const float *rays, const rt_ray_filter &f, int n, const rt_hit_out &out) {
        int rc = reserve_host_hit(n);
        if (rc) return rc;
        hipStream_t s = stream;
        rt_ray_filter df{};
        if ((rc = stage_filter(rays, f, n, df))) return rc;
        rt_hit_out d{};
        if (out.t) d.t = s_t.p;
        if (out.index) d.index = s_index.p;
        if (out.uv) d.uv = s_hit.p;
        if (out.normal) d.normal = s_hit.p + 2 * host_hit_cap;
        if (out.position) d.position = s_hit.p + 5 * host_hit_cap;
        if (out.material) d.material = s_mat.p;
        if (out.front_face) d.front_face = s_occ.p;
        if ((rc = closest_filtered(s_rays.p, df, n, d, s))) return rc;
        const size_t m = (size_t)n;
        if (out.t) HIPCHK(hipMemcpyAsync(out.t, d.t, m * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.index) HIPCHK(hipMemcpyAsync(out.index, d.index, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.uv) HIPCHK(hipMemcpyAsync(out.uv, d.uv, m * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.normal) HIPCHK(hipMemcpyAsync(out.normal, d.normal, m * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.position) HIPCHK(hipMemcpyAsync(out.position, d.position, m * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.material) HIPCHK(hipMemcpyAsync(out.material, d.material, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.front_face) HIPCHK(hipMemcpyAsync(out.front_face, d.front_face, m, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    int occluded_filtered_host(const float *rays, const rt_ray_filter &f, int n, uint8_t *occ) {
        int rc = reserve_host(n);
        if (rc) return rc;
        hipStream_t s = stream;
        rt_ray_filter df{};
        if ((rc = stage_filter(rays, f, n, df))) return rc;
        if ((rc = occluded_filtered(s_rays.p, df, n, s_occ.p, s))) return rc;
        HIPCHK(hipMemcpyAsync(occ, s_occ.p, (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    int reserve_host(int n) {
        if ((size_t)n <= host_cap) return RT_OK;
        HIPCHK(hipSetDevice(scene.device));
        const size_t want = std::max<size_t>({(size_t)n, 2 * host_cap, (size_t)kBlock});
        host_cap = 0;                   // the host calls are blocking: nothing reads the old staging
        int rc;
        if ((rc = s_rays.alloc(want * 6)) || (rc = s_tmax.alloc(want)) || (rc = s_t.alloc(want)) ||
            (rc = s_index.alloc(want)) || (rc = s_occ.alloc(want)))
            return rc;
        host_cap = want;
        return RT_OK;
    }
    // t or index may be null (rt_trace_rays): that output is not copied back
    int closest_host(const float *rays, int n, float *t, int32_t *index) {
        int rc = reserve_host(n);
        if (rc) return rc;
        hipStream_t s = stream;
        HIPCHK(hipMemcpyAsync(s_rays.p, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = closest(s_rays.p, n, s_t.p, s_index.p, s))) return rc;
        if (t) HIPCHK(hipMemcpyAsync(t, s_t.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
        if (index) HIPCHK(hipMemcpyAsync(index, s_index.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    int reserve_host_hit(int n) {
        int rc = reserve_host(n);
        if (rc || (size_t)n <= host_hit_cap) return rc;
        HIPCHK(hipSetDevice(scene.device));
        const size_t want = std::max<size_t>({(size_t)n, 2 * host_hit_cap, (size_t)kBlock});
        host_hit_cap = 0;
        if ((rc = s_hit.alloc(want * 8)) || (rc = s_mat.alloc(want))) return rc;
        host_hit_cap = want;
        return RT_OK;
    }
    int closest_hit_host(const float *rays, int n, const rt_hit_out &out) {
        int rc = reserve_host_hit(n);
        if (rc) return rc;
        hipStream_t s = stream;
        rt_hit_out d{};
        if (out.t) d.t = s_t.p;
        if (out.index) d.index = s_index.p;
        if (out.uv) d.uv = s_hit.p;
        if (out.normal) d.normal = s_hit.p + 2 * host_hit_cap;
        if (out.position) d.position = s_hit.p + 5 * host_hit_cap;
        if (out.material) d.material = s_mat.p;
        if (out.front_face) d.front_face = s_occ.p;
        HIPCHK(hipMemcpyAsync(s_rays.p, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = closest_hit(s_rays.p, n, d, s))) return rc;
        const size_t m = (size_t)n;
        if (out.t) HIPCHK(hipMemcpyAsync(out.t, d.t, m * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.index) HIPCHK(hipMemcpyAsync(out.index, d.index, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.uv) HIPCHK(hipMemcpyAsync(out.uv, d.uv, m * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.normal) HIPCHK(hipMemcpyAsync(out.normal, d.normal, m * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.position) HIPCHK(hipMemcpyAsync(out.position, d.position, m * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.material) HIPCHK(hipMemcpyAsync(out.material, d.material, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out.front_face) HIPCHK(hipMemcpyAsync(out.front_face, d.front_face, m, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    int occluded_host(const float *rays, const float *tmax, int n, uint8_t *occ) {
        int rc = reserve_host(n);
        if (rc) return rc;
        hipStream_t s = stream;
        HIPCHK(hipMemcpyAsync(s_rays.p, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, s));
        if (tmax) HIPCHK(hipMemcpyAsync(s_tmax.p, tmax, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = occluded(s_rays.p, tmax ? s_tmax.p : nullptr, n, s_occ.p, s))) return rc;
        HIPCHK(hipMemcpyAsync(occ, s_occ.p, (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    // New vertices under the frozen topology.  An update overwrites what a query reads, so
    // it joins the `last` chain like a query: queries enqueued later, on any stream, see the new geometry.
    int update(const float *d_vertices, hipStream_t s) {
        HIPCHK(hipSetDevice(scene.device));
        if (pending) HIPCHK(hipStreamWaitEvent(s, last, 0));
        int rc = plan.enqueue(d_vertices, scene.tris.p, scene.nodes.p, scene.big.p, s);
        if (rc) return rc;
        return end(0, 0, s);
    }
    int update_host(const float *vertices) {
        HIPCHK(hipSetDevice(scene.device));
        const size_t count = (size_t)plan.triangle_count * 9;
        if (!plan.d_stage) HIPCHK(hipMalloc(reinterpret_cast<void **>(&plan.d_stage), count * sizeof(float)));
        hipStream_t s = stream;
        HIPCHK(hipMemcpyAsync(plan.d_stage, vertices, count * sizeof(float), hipMemcpyHostToDevice, s));
        int rc = update(plan.d_stage, s);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(s));
        return RT_OK;
    }
    // The device's current triangles and the node array in the scene's numbering (inspection, tests).
    int read_geometry(rt_triangle *tris_out, rt_bvh_node *bvh_out) {
        HIPCHK(hipSetDevice(scene.device));
        int rc = wait_last();
        if (rc) return rc;
        if (tris_out && plan.triangle_count)
            HIPCHK(hipMemcpy(tris_out, scene.tris.p, (size_t)plan.triangle_count * sizeof(rt_triangle), hipMemcpyDeviceToHost));
        if (!bvh_out) return RT_OK;
        using rtamd::refit::Box;
        std::copy(plan.bvh.begin(), plan.bvh.end(), bvh_out);
        if (plan.root_leaf) {
            float4 box[2];
            HIPCHK(hipMemcpy(box, plan.d_root_box, sizeof(box), hipMemcpyDeviceToHost));
            bvh_out[0].min_bound = {box[0].x, box[0].y, box[0].z};
            bvh_out[0].max_bound = {box[1].x, box[1].y, box[1].z};
            return RT_OK;
        }
        std::vector<records::Row> rec_h(plan.rec_node.size() * 4);
        HIPCHK(hipMemcpy(rec_h.data(), scene.nodes.p, rec_h.size() * sizeof(records::Row), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < plan.rec_node.size(); k++) {
            const int i = plan.rec_node[k];
            if (i < 0) continue;
            rt_bvh_node &l = bvh_out[plan.bvh[i].child1], &rr = bvh_out[plan.bvh[i].child2];
            records::unpack(&rec_h[k * 4], l.min_bound, l.max_bound, rr.min_bound, rr.max_bound);
            if (i == 0) {                   // the root's own box: the merge of its record
                Box b = rtamd::refit::empty_box();
                rtamd::refit::grow(b, Box{l.min_bound, l.max_bound});
                rtamd::refit::grow(b, Box{rr.min_bound, rr.max_bound});
                bvh_out[0].min_bound = b.lo;
                bvh_out[0].max_bound = b.hi;
            }
        }
        return RT_OK;
    }
    int stats(rt_stats *st) {
        std::memset(st, 0, sizeof(*st));
        if (!pending) return RT_OK;
        HIPCHK(hipSetDevice(scene.device));
        int rc = wait_last();
        if (rc) return rc;
        if (last_kind == 0) return RT_OK;   // an update since the last query: nothing was traced
        Counters c{};
        if ((rc = scene.read_counters(c))) return rc;
        st->nodes_popped = c.pn; st->internal_visits = c.iv; st->triangle_tests = c.tt;
        st->sphere_tests = c.st; st->hits = c.hits; st->hits_sphere = c.hits_sphere;
        st->live_segments = (uint64_t)last_n;
        st->misses = st->live_segments - st->hits;
        return RT_OK;
    }
};

extern "C" {

int rt_query_create(const rt_scene *scene, const rt_opts *opts, rt_query **out) {
    if (!out) return rtamd::fail(RT_E_INVALID, "rt_query_create: null output");
    *out = nullptr;
    rt_opts o;
    int rc = resolve_opts(scene, opts, o);
    if (rc) return rc;
    auto *q = new rt_query();
    rc = q->init(scene, &o);
    if (rc) { delete q; return rc; }
    *out = q;
    return RT_OK;
}

int rt_query_reserve(rt_query *q, int32_t n) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_reserve: null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_query_reserve: negative ray count");
    return q->reserve(n);
}

int rt_query_closest(rt_query *q, const float *d_rays, int32_t n, float *d_t, int32_t *d_index, void *hip_stream) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_closest: null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_query_closest: negative ray count");
    if (n == 0) return RT_OK;
    if (!d_rays || !d_t || !d_index) return rtamd::fail(RT_E_INVALID, "rt_query_closest: null pointer");
    return q->closest(d_rays, n, d_t, d_index, static_cast<hipStream_t>(hip_stream));
}

int rt_query_occluded(rt_query *q, const float *d_rays, const float *d_tmax, int32_t n, uint8_t *d_occluded,
                      void *hip_stream) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_occluded: null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_query_occluded: negative ray count");
    if (n == 0) return RT_OK;
    if (!d_rays || !d_occluded) return rtamd::fail(RT_E_INVALID, "rt_query_occluded: null pointer");
    return q->occluded(d_rays, d_tmax, n, d_occluded, static_cast<hipStream_t>(hip_stream));
}

int rt_query_closest_host(rt_query *q, const float *rays, int32_t n, float *t, int32_t *index) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_closest_host: null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_query_closest_host: negative ray count");
    if (n == 0) return RT_OK;
    if (!rays || !t || !index) return rtamd::fail(RT_E_INVALID, "rt_query_closest_host: null pointer");
    return q->closest_host(rays, n, t, index);
}

int rt_query_occluded_host(rt_query *q, const float *rays, const float *tmax, int32_t n, uint8_t *occluded) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_occluded_host: null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_query_occluded_host: negative ray count");
    if (n == 0) return RT_OK;
    if (!rays || !occluded) return rtamd::fail(RT_E_INVALID, "rt_query_occluded_host: null pointer");
    return q->occluded_host(rays, tmax, n, occluded);
}

int rt_query_closest_hit(rt_query *q, const float *d_rays, int32_t n, const rt_hit_out *d_out, void *hip_stream) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_closest_hit: null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_query_closest_hit: negative ray count");
    if (n == 0) return RT_OK;
    if (!d_rays || !d_out) return rtamd::fail(RT_E_INVALID, "rt_query_closest_hit: null pointer");
    return q->closest_hit(d_rays, n, *d_out, static_cast<hipStream_t>(hip_stream));
}

int rt_query_closest_hit_host(rt_query *q, const float *rays, int32_t n, const rt_hit_out *out) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_closest_hit_host: null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_query_closest_hit_host: negative ray count");
    if (n == 0) return RT_OK;
    if (!rays || !out) return rtamd::fail(RT_E_INVALID, "rt_query_closest_hit_host: null pointer");
    return q->closest_hit_host(rays, n, *out);
}

// The checks shared by the two multi-hit calls; > 0: n == 0, nothing to do.
static int multi_hit_args(const char *fn, const rt_query *q, const void *rays, int32_t n, int32_t k, const void *out) {
    const std::string f(fn);
    if (!q) return rtamd::fail(RT_E_INVALID, f + ": null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative ray count");
    if (k < 1 || k > RT_MULTI_HIT_MAX)
        return rtamd::fail(RT_E_INVALID, f + ": k " + std::to_string(k) + " is outside 1.." + std::to_string(RT_MULTI_HIT_MAX));
    if (n == 0) return 1;
    if (!rays || !out) return rtamd::fail(RT_E_INVALID, f + ": null pointer");
    if ((int64_t)n * k > INT32_MAX)
        return rtamd::fail(RT_E_INVALID, f + ": n * k = " + std::to_string((int64_t)n * k) + " does not fit int32");
    return RT_OK;
}

int rt_query_multi_hit(rt_query *q, const float *d_rays, const float *d_tmax, int32_t n, int32_t k,
                       const rt_multi_hit_out *d_out, void *hip_stream) {
    const int rc = multi_hit_args("rt_query_multi_hit", q, d_rays, n, k, d_out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->multi_hit(d_rays, d_tmax, n, k, *d_out, static_cast<hipStream_t>(hip_stream));
}

int rt_query_multi_hit_host(rt_query *q, const float *rays, const float *tmax, int32_t n, int32_t k,
                            const rt_multi_hit_out *out) {
    const int rc = multi_hit_args("rt_query_multi_hit_host", q, rays, n, k, out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->multi_hit_host(rays, tmax, n, k, *out);
}

// The checks shared by the two closest-point calls; > 0: n == 0, nothing to do.
static int closest_point_args(const char *fn, const rt_query *q, const void *points, int32_t n, const void *out) {
    const std::string f(fn);
    if (!q) return rtamd::fail(RT_E_INVALID, f + ": null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative point count");
    if (n == 0) return 1;
    if (!points || !out) return rtamd::fail(RT_E_INVALID, f + ": null pointer");
    return RT_OK;
}

int rt_query_closest_point(rt_query *q, const float *d_points, const float *d_max_dist, int32_t n,
                           const rt_closest_point_out *d_out, void *hip_stream) {
    const int rc = closest_point_args("rt_query_closest_point", q, d_points, n, d_out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->closest_point(d_points, d_max_dist, n, *d_out, static_cast<hipStream_t>(hip_stream));
}

int rt_query_closest_point_host(rt_query *q, const float *points, const float *max_dist, int32_t n,
                                const rt_closest_point_out *out) {
    const int rc = closest_point_args("rt_query_closest_point_host", q, points, n, out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->closest_point_host(points, max_dist, n, *out);
}

// The checks shared by the two nearest-k calls; > 0: n == 0, nothing to do.
static int nearest_k_args(const char *fn, const rt_query *q, const void *points, int32_t n, int32_t k, const void *out) {
    const std::string f(fn);
    if (!q) return rtamd::fail(RT_E_INVALID, f + ": null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative point count");
    if (k < 1 || k > RT_NEAREST_K_MAX)
        return rtamd::fail(RT_E_INVALID, f + ": k " + std::to_string(k) + " is outside 1.." + std::to_string(RT_NEAREST_K_MAX));
    if (n == 0) return 1;
    if (!points || !out) return rtamd::fail(RT_E_INVALID, f + ": null pointer");
    if ((int64_t)n * k > INT32_MAX)
        return rtamd::fail(RT_E_INVALID, f + ": n * k = " + std::to_string((int64_t)n * k) + " does not fit int32");
    return RT_OK;
}

int rt_query_nearest_k(rt_query *q, const float *d_points, const float *d_max_dist, int32_t n, int32_t k,
                       const rt_nearest_k_out *d_out, void *hip_stream) {
    const int rc = nearest_k_args("rt_query_nearest_k", q, d_points, n, k, d_out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->nearest_k(d_points, d_max_dist, n, k, *d_out, static_cast<hipStream_t>(hip_stream));
}

int rt_query_nearest_k_host(rt_query *q, const float *points, const float *max_dist, int32_t n, int32_t k,
                            const rt_nearest_k_out *out) {
    const int rc = nearest_k_args("rt_query_nearest_k_host", q, points, n, k, out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->nearest_k_host(points, max_dist, n, k, *out);
}

// The checks shared by the two box-overlap calls; > 0: n == 0, nothing to do.
static int overlap_box_args(const char *fn, const rt_query *q, const void *boxes, int32_t n, int32_t k, const void *out) {
    const std::string f(fn);
    if (!q) return rtamd::fail(RT_E_INVALID, f + ": null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative box count");
    if (k < 1 || k > RT_OVERLAP_K_MAX)
        return rtamd::fail(RT_E_INVALID, f + ": k " + std::to_string(k) + " is outside 1.." + std::to_string(RT_OVERLAP_K_MAX));
    if (n == 0) return 1;
    if (!boxes || !out) return rtamd::fail(RT_E_INVALID, f + ": null pointer");
    if ((int64_t)n * k > INT32_MAX)
        return rtamd::fail(RT_E_INVALID, f + ": n * k = " + std::to_string((int64_t)n * k) + " does not fit int32");
    return RT_OK;
}

int rt_query_overlap_box(rt_query *q, const float *d_boxes, int32_t n, int32_t k, const rt_overlap_out *d_out,
                         void *hip_stream) {
    const int rc = overlap_box_args("rt_query_overlap_box", q, d_boxes, n, k, d_out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->overlap_box(d_boxes, n, k, *d_out, static_cast<hipStream_t>(hip_stream));
}

int rt_query_overlap_box_host(rt_query *q, const float *boxes, int32_t n, int32_t k, const rt_overlap_out *out) {
    const int rc = overlap_box_args("rt_query_overlap_box_host", q, boxes, n, k, out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->overlap_box_host(boxes, n, k, *out);
}

// The checks shared by the four filtered calls; > 0: n == 0, nothing to do.
static int filtered_args(const char *fn, const rt_query *q, const void *rays, int32_t n, const void *out) {
    const std::string f(fn);
    if (!q) return rtamd::fail(RT_E_INVALID, f + ": null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative ray count");
    if (n == 0) return 1;
    if (!rays || !out) return rtamd::fail(RT_E_INVALID, f + ": null pointer");
    return RT_OK;
}

int rt_query_closest_filtered(rt_query *q, const float *d_rays, const rt_ray_filter *d_filter, int32_t n,
                              const rt_hit_out *d_out, void *hip_stream) {
    const int rc = filtered_args("rt_query_closest_filtered", q, d_rays, n, d_out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->closest_filtered(d_rays, d_filter ? *d_filter : rt_ray_filter{}, n, *d_out, static_cast<hipStream_t>(hip_stream));
}

int rt_query_occluded_filtered(rt_query *q, const float *d_rays, const rt_ray_filter *d_filter, int32_t n,
                               uint8_t *d_occluded, void *hip_stream) {
    const int rc = filtered_args("rt_query_occluded_filtered", q, d_rays, n, d_occluded);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->occluded_filtered(d_rays, d_filter ? *d_filter : rt_ray_filter{}, n, d_occluded,
                                static_cast<hipStream_t>(hip_stream));
}

int rt_query_closest_filtered_host(rt_query *q, const float *rays, const rt_ray_filter *filter, int32_t n,
                                   const rt_hit_out *out) {
    const int rc = filtered_args("rt_query_closest_filtered_host", q, rays, n, out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->closest_filtered_host(rays, filter ? *filter : rt_ray_filter{}, n, *out);
}

int rt_query_occluded_filtered_host(rt_query *q, const float *rays, const rt_ray_filter *filter, int32_t n,
                                    uint8_t *occluded) {
    const int rc = filtered_args("rt_query_occluded_filtered_host", q, rays, n, occluded);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->occluded_filtered_host(rays, filter ? *filter : rt_ray_filter{}, n, occluded);
}

// The checks shared by the two hemisphere calls; > 0: n == 0, nothing to do.
static int hemisphere_args(const char *fn, const rt_query *q, const void *frames, int32_t n, const rt_hemisphere_params *p,
                           const rt_hemisphere_out *out) {
    const std::string f(fn);
    if (!q) return rtamd::fail(RT_E_INVALID, f + ": null query object");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative point count");
    if (n == 0) return 1;
    if (!frames) return rtamd::fail(RT_E_INVALID, f + ": null frames");
    if (const char *why = rtamd::hemi::params_error(p, n)) return rtamd::fail(RT_E_INVALID, f + ": " + why);
    if (!out || (!out->open_count && !out->openness)) return rtamd::fail(RT_E_INVALID, f + ": no output pointer");
    return RT_OK;
}

int rt_query_hemisphere(rt_query *q, const float *d_frames, const rt_ray_filter *d_filter, int32_t n,
                        const rt_hemisphere_params *params, const rt_hemisphere_out *d_out, void *hip_stream) {
    const int rc = hemisphere_args("rt_query_hemisphere", q, d_frames, n, params, d_out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->hemisphere(d_frames, d_filter ? *d_filter : rt_ray_filter{}, n, *params, *d_out,
                         static_cast<hipStream_t>(hip_stream));
}

int rt_query_hemisphere_host(rt_query *q, const float *frames, const rt_ray_filter *filter, int32_t n,
                             const rt_hemisphere_params *params, const rt_hemisphere_out *out) {
    const int rc = hemisphere_args("rt_query_hemisphere_host", q, frames, n, params, out);
    if (rc) return rc > 0 ? RT_OK : rc;
    return q->hemisphere_host(frames, filter ? *filter : rt_ray_filter{}, n, *params, *out);
}

int rt_query_set_masks(rt_query *q, const uint32_t *d_masks, int32_t count, void *hip_stream) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_set_masks: null query object");
    if (count != q->prim_count)
        return rtamd::fail(RT_E_INVALID, "rt_query_set_masks: count " + std::to_string(count) +
                                             " is not the scene's sphere_count + triangle_count = " +
                                             std::to_string(q->prim_count));
    return q->set_masks(d_masks, false, static_cast<hipStream_t>(hip_stream));
}

int rt_query_set_masks_host(rt_query *q, const uint32_t *masks, int32_t count) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_set_masks_host: null query object");
    if (count != q->prim_count)
        return rtamd::fail(RT_E_INVALID, "rt_query_set_masks_host: count " + std::to_string(count) +
                                             " is not the scene's sphere_count + triangle_count = " +
                                             std::to_string(q->prim_count));
    return q->set_masks(masks, true, q->stream);
}

int rt_query_stats(rt_query *q, rt_stats *stats) {
    if (!q || !stats) return rtamd::fail(RT_E_INVALID, "rt_query_stats: null argument");
    return q->stats(stats);
}

int rt_query_update_triangles(rt_query *q, const float *d_vertices, int32_t triangle_count, void *hip_stream) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_update_triangles: null query object");
    if (triangle_count != q->plan.triangle_count)
        return rtamd::fail(RT_E_INVALID, "rt_query_update_triangles: triangle_count " + std::to_string(triangle_count) +
                                             " is not the scene's " + std::to_string(q->plan.triangle_count));
    if (triangle_count == 0) return RT_OK;
    if (!d_vertices) return rtamd::fail(RT_E_INVALID, "rt_query_update_triangles: null pointer");
    return q->update(d_vertices, static_cast<hipStream_t>(hip_stream));
}

int rt_query_update_triangles_host(rt_query *q, const float *vertices, int32_t triangle_count) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_update_triangles_host: null query object");
    if (triangle_count != q->plan.triangle_count)
        return rtamd::fail(RT_E_INVALID, "rt_query_update_triangles_host: triangle_count " + std::to_string(triangle_count) +
                                             " is not the scene's " + std::to_string(q->plan.triangle_count));
    if (triangle_count == 0) return RT_OK;
    if (!vertices) return rtamd::fail(RT_E_INVALID, "rt_query_update_triangles_host: null pointer");
    return q->update_host(vertices);
}

int rt_query_read_geometry(rt_query *q, rt_triangle *triangles_out, rt_bvh_node *bvh_out) {
    if (!q) return rtamd::fail(RT_E_INVALID, "rt_query_read_geometry: null query object");
    return q->read_geometry(triangles_out, bvh_out);
}

void rt_query_destroy(rt_query *q) { delete q; }

// One-shot closest hit: a query object for the length of the call.  The stats are the traversal's own
// counters (live_segments = the rays the kernel took from its queue); hits and misses stay 0.
int rt_trace_rays(const rt_scene *scene, const rt_opts *opts, const float *rays, int32_t n, float *t_out,
                  int32_t *index_out, rt_stats *stats) {
    if (n < 0 || (n > 0 && !rays)) return rtamd::fail(RT_E_INVALID, "rt_trace_rays: bad argument");
    rt_query *q = nullptr;
    int rc = rt_query_create(scene, opts, &q);
    if (rc || n == 0) {
        delete q;
        return rc;
    }
    rc = q->closest_host(rays, n, t_out, index_out);
    Counters c{};
    if (!rc && stats && !(rc = q->scene.read_counters(c))) {
        std::memset(stats, 0, sizeof(*stats));
        stats->live_segments = c.live;
        stats->nodes_popped = c.pn;
        stats->internal_visits = c.iv;
        stats->triangle_tests = c.tt;
        stats->sphere_tests = c.st;
    }
    delete q;
    return rc;
}

}  // extern "C"
