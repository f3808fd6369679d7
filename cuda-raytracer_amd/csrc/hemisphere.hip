// hemisphere.hip — hemisphere visibility queries (rt_query_hemisphere): S sample rays over the hemisphere
// above each of n surface points, made in registers, walked as the filtered any-hit walks them, counted per point.
// The sample generator is host/hemisphere_math.h's and the filter's arithmetic host/ray_filter_math.h's, which the
// host twin (cpu_query.hip) compiles too; the query object and the C ABI are rt_query.hip's.
#include "rt_common.h"
#include "ray_filter_math.h"
#include "hemisphere_math.h"

#pragma clang fp contract(off)

// A/B experiments only: 1 = every escaped lane adds 1 to its point's count by itself, 0 = the lanes of a wave that
// share a point add their number with one atomic (DESIGN §18 has both measured).
#ifndef RT_HEMI_LANE_ATOMICS
#define RT_HEMI_LANE_ATOMICS 0
#endif

using namespace rtamd;

namespace {

// Caller frames and filter -> one 32-B slot per point, filter_ingest_kernel's layout with the unit normal in the
// direction's place, {p.xyz, nh.x} {nh.y, nh.z, B, lo}, and fil[i] = {skip, rm}; count[i] = 0.  Block 0 also starts
// the call with live_count = n * S work items.
__global__ __launch_bounds__(kBlock) void hemisphere_ingest_kernel(const float *__restrict__ frames, const float *__restrict__ tmin,
                                                                   const float *__restrict__ tmax,
                                                                   const int32_t *__restrict__ skip,
                                                                   const uint32_t *__restrict__ mask, uint32_t n,
                                                                   uint32_t live_count, float4 *__restrict__ geo,
                                                                   uint2 *__restrict__ fil, uint32_t *__restrict__ count,
                                                                   uint32_t *__restrict__ live, uint32_t *__restrict__ queue,
                                                                   Counters *__restrict__ ctr) {
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) live[0] = live_count;
        if (threadIdx.x < kQueues) queue[threadIdx.x * kQueueStride] = 0;
        unsigned long long *w = reinterpret_cast<unsigned long long *>(ctr);
        for (uint32_t k = threadIdx.x; k < kCtrSlots * (sizeof(Counters) / sizeof(unsigned long long)); k += kBlock) w[k] = 0;
    }
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *r = frames + (size_t)i * 6;
    const V3 nh = hemi::unit_normal(v3(r[3], r[4], r[5]));
    const float b = tmax ? rf::upper(tmax[i]) : 1e30f;
    const float lo = tmin ? rf::lower(tmin[i]) : kEps;
    geo[(size_t)i * 2] = make_float4(r[0], r[1], r[2], nh.x);
    geo[(size_t)i * 2 + 1] = make_float4(nh.y, nh.z, b, lo);
    fil[i] = make_uint2(skip ? (uint32_t)skip[i] : 0xFFFFFFFFu, mask ? mask[i] : rf::kAllBits);
    count[i] = 0;
}

// The scratch counts -> the caller's outputs, each optional.
__global__ __launch_bounds__(kBlock) void hemisphere_egest_kernel(const uint32_t *__restrict__ count, uint32_t n, float samples,
                                                                  int32_t *__restrict__ open_count,
                                                                  float *__restrict__ openness) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = count[i];
    if (open_count) open_count[i] = (int32_t)c;
    if (openness) openness[i] = (float)c / samples;
}

// The hemisphere walk (rt_abi.h): filtered_anyhit_kernel's definition, pinned visit order and counters
// over the L = n * ns work items w = i * ns + s.  At its refill a lane loads point i's slot and filter row (lanes
// with the same point share the loads), makes the sample direction of work item wbase + w in registers
// (hemisphere_math.h; wbase = point_offset * ns in uint32) and goes on as the any-hit kernel does from its refill.
// The loop, node_step and pop_loop are that kernel's text, repeated here and not shared through a template, so
// every other kernel compiles to the registers it was tuned at (profiles/hemisphere/kernel_resources.txt).
// A lane retires on an accept or on an empty stack and delivers at its next refill (or at exit): an escaped ray adds
// to count[i].  The lanes of the wave that deliver for the same point add their number with one atomic -- for
// ns >= 64 that is one or two atomics per refill instead of up to 64 on one address.
// Counters (COUNT): Pn, Iv, Tt and sphere tests per ray, summed over all L rays; hits = the occluded rays.
template <bool COUNT>
__global__ __launch_bounds__(kBlock) RT_TRACE_ATTR void hemisphere_kernel(DevScene S, const float4 *__restrict__ geo,
                                                                          const uint2 *__restrict__ fil,
                                                                          const uint32_t *__restrict__ masks,
                                                                          const uint32_t *__restrict__ live_count,
                                                                          uint32_t *__restrict__ queue,
                                                                          uint32_t *__restrict__ count, uint32_t ns,
                                                                          uint32_t wbase, uint32_t seed, int32_t mode,
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
    int slot = -1;                      // < 0: lane has no ray; <= -2: done with work item -2 - slot, not yet delivered
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
    // The answer of a lane with slot <= -2 (only those call it).
    auto deliver = [&]() {
        nocc += occ;
        if (!occ) {
            const uint32_t pi = (uint32_t)(-2 - slot) / ns;
#if RT_HEMI_LANE_ATOMICS
            atomicAdd(count + pi, 1u);
#else
            bool todo = true;
            while (todo) {                // one round per distinct point among the lanes still here
                const uint32_t key = __builtin_amdgcn_readfirstlane(pi);
                const bool mine = pi == key;
                const unsigned long long grp = __ballot(mine);
                if (mine) {
                    if (lane_id() == (uint32_t)__ffsll((long long)grp) - 1u) atomicAdd(count + key, (uint32_t)__popcll(grp));
                    todo = false;
                }
            }
#endif
        }
        slot = -1;
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
            if (slot <= -2) deliver();    // answers of the lanes that finished since the last refill
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
                const uint32_t w = (uint32_t)slot;
                const uint32_t pi = w / ns;   // the sample index w - pi * ns enters only through w itself
                const float4 *rp = geo + (size_t)pi * 2;
                const float4 r0 = rp[0], r1 = rp[1];
                const uint2 f = fil[pi];
                o = v3(r0.x, r0.y, r0.z);
                d = hemi::direction(v3(r0.w, r1.x, r1.y), wbase + w, seed, mode);
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
                if (done) slot = -2 - slot;   // delivered with the others, at the next refill or at exit
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
    if (slot <= -2) deliver();
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

int hemisphere_blocks_per_cu(int &per_cu) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, hemisphere_kernel<false>, kBlock, 0));
    return RT_OK;
}

void launch_hemisphere_ingest(int n, hipStream_t s, const float *d_frames, const rt_ray_filter &f, uint32_t live_count,
                              float4 *geo, uint2 *fil, uint32_t *count, uint32_t *live, uint32_t *queue, Counters *ctr) {
    hipLaunchKernelGGL(hemisphere_ingest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, d_frames, f.tmin, f.tmax, f.skip,
                       f.mask, (uint32_t)n, live_count, geo, fil, count, live, queue, ctr);
}

void launch_hemisphere(bool count_work, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint2 *fil,
                       const uint32_t *masks, const uint32_t *live, uint32_t *queue, uint32_t *count,
                       const rt_hemisphere_params &p, uint32_t *overflow, Counters *ctr) {
    const uint32_t ns = (uint32_t)p.samples, wbase = hemi::base(p.point_offset, ns);
    if (count_work)
        hipLaunchKernelGGL(hemisphere_kernel<true>, dim3(grid), dim3(kBlock), 0, s, ds, geo, fil, masks, live, queue, count, ns,
                           wbase, p.seed, p.mode, overflow, ctr);
    else
        hipLaunchKernelGGL(hemisphere_kernel<false>, dim3(grid), dim3(kBlock), 0, s, ds, geo, fil, masks, live, queue, count, ns,
                           wbase, p.seed, p.mode, overflow, ctr);
}

void launch_hemisphere_egest(int n, hipStream_t s, const uint32_t *count, int32_t samples, const rt_hemisphere_out &out) {
    hipLaunchKernelGGL(hemisphere_egest_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, count, (uint32_t)n, (float)samples,
                       out.open_count, out.openness);
}

}  // namespace rtamd
