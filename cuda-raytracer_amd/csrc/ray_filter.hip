// ray_filter.hip — filtered ray queries (rt_query_closest_filtered, rt_query_occluded_filtered): a
// per-ray interval [lo, B), a primitive to skip and a visibility mask, over the resident scene.  The filter's
// arithmetic is host/ray_filter_math.h's, which the host twins (cpu_query.hip) compile too; the query object
// and the C ABI are rt_query.hip's.
#include "rt_common.h"
#include "ray_filter_math.h"

#pragma clang fp contract(off)

using namespace rtamd;

namespace {

// Caller rays and filter -> the 32-B slots query_ingest_kernel writes, {o.xyz, d.x} {d.y, d.z, B, lo}, with the
// ray's lower bound lo in the slot's spare word, and fil[i] = {skip, rm}, an array of the object's scratch that
// grows with the slots.  Every filter member is optional.  Block 0 also starts the call, as query_ingest_kernel's.
__global__ __launch_bounds__(kBlock) void filter_ingest_kernel(const float *__restrict__ rays, const float *__restrict__ tmin,
                                                               const float *__restrict__ tmax,
                                                               const int32_t *__restrict__ skip,
                                                               const uint32_t *__restrict__ mask, uint32_t n,
                                                               float4 *__restrict__ geo, uint2 *__restrict__ fil,
                                                               uint32_t *__restrict__ live, uint32_t *__restrict__ queue,
                                                               Counters *__restrict__ ctr) {
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) live[0] = n;
        if (threadIdx.x < kQueues) queue[threadIdx.x * kQueueStride] = 0;
        unsigned long long *w = reinterpret_cast<unsigned long long *>(ctr);
        for (uint32_t k = threadIdx.x; k < kCtrSlots * (sizeof(Counters) / sizeof(unsigned long long)); k += kBlock) w[k] = 0;
    }
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *r = rays + (size_t)i * 6;
    const float b = tmax ? rf::upper(tmax[i]) : 1e30f;
    const float lo = tmin ? rf::lower(tmin[i]) : kEps;
    geo[(size_t)i * 2] = make_float4(r[0], r[1], r[2], r[3]);
    geo[(size_t)i * 2 + 1] = make_float4(r[4], r[5], b, lo);
    fil[i] = make_uint2(skip ? (uint32_t)skip[i] : 0xFFFFFFFFu, mask ? mask[i] : rf::kAllBits);
}

// The filtered closest hit (rt_abi.h): the shrinking-bound walk in the near-child-first order that is
// part of the call's definition -- spheres in order; the root; at an internal node both children's slabs against
// the current `closest`, a child entered iff it is hit and !(entry >= closest), child 1 (the record's second) first
// iff it is entered and child 0 is not or t1 < t0 (a tie goes to child 0), the other one pushed with its entry
// distance iff both are entered; a leaf's triangles in order; an exhausted leaf, or a node with no entered child,
// pops; a popped entry whose distance >= the current `closest` is discarded without counting.
// A primitive is accepted iff its geometric test under the bound `closest` accepts, !(t < lo), it is not the ray's
// skip index and its mask word shares a bit with the ray's.  The mask word is loaded only after the rest has
// accepted, and only when the object holds masks (`masks` != nullptr, wave-uniform).
// The stack holds (ref, entry) pairs, trace_kernel's layout: kStackLds pairs + the scratch entry in LDS, deeper
// ones in `overflow` in two halves.  Queue, ballot refill, scalar root record, one record load per step and the
// literal slab fold for lanes with a non-finite 1/d are trace_kernel's; that text is repeated here and not shared
// through a template, so the other kernels compile to the registers they were tuned at
// (profiles/ray_filter/kernel_resources.txt).  hits[slot] = {t, index} -- (1e30, -1) on a miss -- stored at the
// lane's next refill or at exit, for query_egest_kernel / query_hit_egest_kernel.
// Counters (COUNT): Pn = nodes entered, Iv = internal nodes stepped, Tt = triangle tests, S sphere tests per ray:
// exact on every ray, the order being pinned.
template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void filtered_closest_kernel(DevScene S, const float4 *__restrict__ geo,
                                                                                const uint2 *__restrict__ fil,
                                                                                const uint32_t *__restrict__ masks,
                                                                                const uint32_t *__restrict__ live_count,
                                                                                uint32_t *__restrict__ queue,
                                                                                float2 *__restrict__ hits,
                                                                                uint32_t *__restrict__ overflow,
                                                                                Counters *__restrict__ ctr) {
    __shared__ uint2 stack[(kStackLds + 1) * kBlock];   // + one scratch entry per lane
    uint2 *col = stack + threadIdx.x;
    // entry e >= kStackLds of this lane: ref at overflow[(e - kStackLds) * lanes + lane], distance in the second half
    const uint32_t lanes = gridDim.x * kBlock, gl = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t dist_half = lanes * (kStackMax - kStackLds);
    const uint32_t L = __builtin_amdgcn_readfirstlane(*live_count);
    const uint32_t waves = gridDim.x * (kBlock / 64);
    const uint32_t chunk = min((uint32_t)kChunkMax, max((uint32_t)kChunkMin, (L / (4 * waves) + 63) & ~63u));
    uint32_t shard = blockIdx.x % kQueues, tried = 0;
    uint32_t q_next = 0, q_end = 0;     // this wave's current chunk (wave-uniform)
    bool exhausted = false;
    int slot = -1;                      // < 0: lane has no ray; <= -2: done with slot -2 - slot, record not yet stored
    V3 o{0, 0, 0}, d{0, 0, 0};
    float ix = 0, iy = 0, iz = 0, closest = 0, lo = 0;
    int skip = -1;
    uint32_t rm = 0;
    bool finite_inv = true;
    bool wave_nonfinite = false;
    int index = -1, sp = 0;
    uint32_t ref = 0;
    int ti = 0, te = 0;                 // the lane is in a leaf while ti < te
    unsigned pn = 0, iv = 0, tt = 0, stn = 0;
    // The filter's part of an accept, after the geometric test: t is accepted under `closest`.
    auto passes = [&](float t, int prim) -> bool {
        bool ok = !(t < lo) && prim != skip;
        if (ok) {
            uint32_t m = rf::kAllBits;
            if (masks) m = masks[prim];
            ok = (m & rm) != 0;
        }
        return ok;
    };
    auto record = [&]() { return make_float2(index < 0 ? 1e30f : closest, __int_as_float(index)); };
    auto node_step = [&](float4 a, float4 b, float4 c, uint2 kids) -> bool {
        if (COUNT) iv++;
        float t0, t1;
        bool h0, h1;
        slab_pair(a, b, c, o, ix, iy, iz, closest, h0, h1, t0, t1);
        if (__builtin_expect(wave_nonfinite, 0)) {
            float u0, u1;
            const bool g0 = slab(a.x, a.z, b.x, b.z, c.x, c.z, o, ix, iy, iz, closest, u0);
            const bool g1 = slab(a.y, a.w, b.y, b.w, c.y, c.w, o, ix, iy, iz, closest, u1);
            if (!finite_inv) { h0 = g0; h1 = g1; t0 = u0; t1 = u1; }
        }
        const bool e0 = h0 && !(t0 >= closest), e1 = h1 && !(t1 >= closest);
        const bool both = e0 && e1, any = e0 || e1;
        // next = child 1 iff it is the nearer of two entered children or the only one
        const bool sel1 = e1 && (!e0 || t1 < t0);
        const uint32_t next_ref = sel1 ? kids.y : kids.x, far_ref = sel1 ? kids.x : kids.y;
        const float far_t = sel1 ? t0 : t1;
        // written either way (above the top when not pushed; entry kStackLds is a scratch slot)
        col[min(sp, kStackLds) * kBlock] = make_uint2(far_ref, __float_as_uint(far_t));
        if (__builtin_expect(both && sp >= kStackLds, 0)) {
            overflow[(sp - kStackLds) * lanes + gl] = far_ref;
            overflow[dist_half + (sp - kStackLds) * lanes + gl] = __float_as_uint(far_t);
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
    // Pop to the next entry nearer than the current closest; an empty stack ends the ray.
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
            const bool take = !empty && !(__uint_as_float(e.y) >= closest);
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
            if (slot <= -2) {             // records of the lanes that finished since the last refill
                hits[-2 - slot] = record();
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
                const uint2 f = fil[slot];
                o = v3(r0.x, r0.y, r0.z);
                d = v3(r0.w, r1.x, r1.y);
                closest = r1.z;
                lo = r1.w;
                skip = (int)f.x;
                rm = f.y;
                ix = 1 / d.x; iy = 1 / d.y; iz = 1 / d.z;
                finite_inv = __builtin_isfinite(ix) && __builtin_isfinite(iy) && __builtin_isfinite(iz);
                index = -1;
                for (int i = 0; i < S.sphere_count; i++) {
                    const float4 sph = S.spheres[i];
                    float t;
                    if (COUNT) stn++;
                    if (rf::ray_sphere_lo(o, d, v3(sph.x, sph.y, sph.z), sph.w, lo, closest, t) && passes(t, i)) {
                        closest = t;
                        index = i;
                    }
                }
                ref = S.root_ref;
                sp = 0;
                ti = te = 0;
                // the root is popped with distance 0: entered iff !(0 >= closest)
                bool done = 0.0f >= closest;
                if (!done) {
                    if (COUNT) pn++;
                    if (ref & kLeaf) {
                        leaf_range(S, ref, ti, te);
                        done = ti == te;    // no triangles at all: spheres only
                    }
                }
                if (done) {
                    hits[slot] = record();
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
            bool hit = ray_triangle_flat(o, d, v3(a.x, a.y, a.z), v3(a.w, b.x, b.y), v3(b.z, b.w, c.x), closest, t);
            if (hit) hit = passes(t, S.sphere_count + ti);
            closest = hit ? t : closest;
            index = hit ? S.sphere_count + ti : index;
            need = ++ti == te;
        } else {
            need = node_step(a, b, c, kids);
        }
        pop_loop(need);
    }
    if (slot <= -2) hits[-2 - slot] = record();
    if (COUNT) {
        Counters *cs = ctr + ((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) & (kCtrSlots - 1));
        const unsigned long long a = wave_sum(pn), b = wave_sum(iv), t = wave_sum(tt), s = wave_sum(stn);
        if (lane_id() == 0) {
            atomicAdd(&cs->pn, a);
            atomicAdd(&cs->iv, b);
            atomicAdd(&cs->tt, t);
            atomicAdd(&cs->st, s);
        }
    }
}

// The filtered any-hit (rt_abi.h): anyhit_kernel's definition, pinned visit order and counters with the
// bound held at B; only the acceptance tests change, to filtered_closest_kernel's.  Eligibility depends on the ray
// and the primitive alone, so the answer is still an existence statement over a fixed node set.  The loop,
// node_step and pop_loop are anyhit_kernel's text, repeated here (see above); the stack holds 4-B refs.
template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void filtered_anyhit_kernel(DevScene S, const float4 *__restrict__ geo,
                                                                               const uint2 *__restrict__ fil,
                                                                               const uint32_t *__restrict__ masks,
                                                                               const uint32_t *__restrict__ live_count,
                                                                               uint32_t *__restrict__ queue,
                                                                               uint8_t *__restrict__ out,
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
    float ix = 0, iy = 0, iz = 0, B = 0, lo = 0;
    int skip = -1;
    uint32_t rm = 0;
    bool finite_inv = true;
    bool wave_nonfinite = false;
    int sp = 0;
    uint32_t ref = 0, occ = 0;
    int ti = 0, te = 0;                 // the lane is in a leaf while ti < te
    unsigned pn = 0, iv = 0, tt = 0, stn = 0, nocc = 0;
    auto passes = [&](float t, int prim) -> bool {
        bool ok = !(t < lo) && prim != skip;
        if (ok) {
            uint32_t m = rf::kAllBits;
            if (masks) m = masks[prim];
            ok = (m & rm) != 0;
        }
        return ok;
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
    // Pop: every entry on the stack is entered; an empty stack ends the ray unoccluded.
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
                const uint2 f = fil[slot];
                o = v3(r0.x, r0.y, r0.z);
                d = v3(r0.w, r1.x, r1.y);
                B = r1.z;
                lo = r1.w;
                skip = (int)f.x;
                rm = f.y;
                ix = 1 / d.x; iy = 1 / d.y; iz = 1 / d.z;
                finite_inv = __builtin_isfinite(ix) && __builtin_isfinite(iy) && __builtin_isfinite(iz);
                occ = 0;
                for (int i = 0; i < S.sphere_count; i++) {
                    const float4 sph = S.spheres[i];
                    float t;
                    if (COUNT) stn++;
                    if (rf::ray_sphere_lo(o, d, v3(sph.x, sph.y, sph.z), sph.w, lo, B, t) && passes(t, i)) { occ = 1; break; }
                }
                ref = S.root_ref;
                sp = 0;
                ti = te = 0;
                // the root is popped with distance 0: entered iff !(0 >= B)
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
        // ---- one step: one triangle test of the current leaf, or one internal node
        bool need = false;
        const bool in_leaf = ti < te;
        const float4 *rec = in_leaf ? S.tris + (size_t)ti * 3 : S.nodes + (size_t)ref * 4;
        const float4 a = rec[0], b = rec[1], c = rec[2];
        uint2 kids = make_uint2(0, 0);
        if (!in_leaf) kids = *reinterpret_cast<const uint2 *>(rec + 3);
        if (in_leaf) {
            if (COUNT) tt++;
            float t;
            bool hit = ray_triangle_flat(o, d, v3(a.x, a.y, a.z), v3(a.w, b.x, b.y), v3(b.z, b.w, c.x), B, t);
            if (hit) hit = passes(t, S.sphere_count + ti);
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

}  // namespace

namespace rtamd {

int ray_filter_blocks_per_cu(int &per_cu_closest, int &per_cu_anyhit) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_closest, filtered_closest_kernel<false>, kBlock, 0));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_anyhit, filtered_anyhit_kernel<false>, kBlock, 0));
    return RT_OK;
}

void launch_filter_ingest(int n, hipStream_t s, const float *d_rays, const rt_ray_filter &f, float4 *geo, uint2 *fil,
                          uint32_t *live, uint32_t *queue, Counters *ctr) {
    hipLaunchKernelGGL(filter_ingest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, d_rays, f.tmin, f.tmax, f.skip, f.mask,
                       (uint32_t)n, geo, fil, live, queue, ctr);
}

void launch_filtered_closest(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint2 *fil,
                             const uint32_t *masks, const uint32_t *live, uint32_t *queue, float2 *hits, uint32_t *overflow,
                             Counters *ctr) {
    if (count)
        hipLaunchKernelGGL(filtered_closest_kernel<true>, dim3(grid), dim3(kBlock), 0, s, ds, geo, fil, masks, live, queue,
                           hits, overflow, ctr);
    else
        hipLaunchKernelGGL(filtered_closest_kernel<false>, dim3(grid), dim3(kBlock), 0, s, ds, geo, fil, masks, live, queue,
                           hits, overflow, ctr);
}

void launch_filtered_anyhit(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint2 *fil,
                            const uint32_t *masks, const uint32_t *live, uint32_t *queue, uint8_t *out, uint32_t *overflow,
                            Counters *ctr) {
    if (count)
        hipLaunchKernelGGL(filtered_anyhit_kernel<true>, dim3(grid), dim3(kBlock), 0, s, ds, geo, fil, masks, live, queue, out,
                           overflow, ctr);
    else
        hipLaunchKernelGGL(filtered_anyhit_kernel<false>, dim3(grid), dim3(kBlock), 0, s, ds, geo, fil, masks, live, queue, out,
                           overflow, ctr);
}

}  // namespace rtamd
