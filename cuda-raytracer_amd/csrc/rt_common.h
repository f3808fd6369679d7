// rt_common.h — what more than one HIP translation unit of librtamd.so needs, each defined once:
// the workgroup, stack and queue constants, the device scene, the traversal building blocks shared by
// trace_kernel (rt_render.hip), anyhit_kernel (rt_query.hip) and the refit kernels (bvh_refit.hip), the
// host-side HIP helpers, and the resident scene (SceneDev, scene_dev.hip).  Kernels themselves stay in an
// anonymous namespace of the .hip file that launches them.
#pragma once
#include "rt_abi.h"
#include "rt_device.h"
#include "rt_host.h"
#include "bvh_records.h"

#include <string>
#include <vector>

#pragma clang fp contract(off)

// Tuning knobs shared by the traversal kernels (compile-time; -D overrides are for A/B experiments only).
#ifndef RT_STACK_LDS
#define RT_STACK_LDS 8
#endif
#ifndef RT_REFILL
#define RT_REFILL 24                  // A/B at 16 passes in flight: 24 beats 16 by ~1 % (teapot, lamp); 8 is worse
#endif
#ifndef RT_REFILL_FIRST
#define RT_REFILL_FIRST 64
#endif
#ifndef RT_CHUNK_MAX
#define RT_CHUNK_MAX 128
#endif
#ifndef RT_CHUNK_MIN
#define RT_CHUNK_MIN 64
#endif
#ifndef RT_QUEUES
#define RT_QUEUES 8
#endif
// 8 waves per SIMD (<= 64 VGPRs): the one spill left is a lane constant reloaded only on the
// overflow-stack path.  +2 % over the unconstrained 66 VGPRs (7 waves).
#ifndef RT_TRACE_WPE
#define RT_TRACE_WPE 8
#endif
#define RT_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(RT_TRACE_WPE, RT_TRACE_WPE > 8 ? RT_TRACE_WPE : 8)))

namespace rtamd {

using namespace rtd;

constexpr int kBlock = 256;           // threads per workgroup (4 waves)
constexpr int kStackLds = RT_STACK_LDS; // stack entries per lane kept in LDS (deeper: global)
constexpr int kStackMax = 32;         // >= MAX_BVH_DEPTH + 1 (scene.cu:10, :138)
constexpr int kCtrSlots = 64;       // striped copies of the work counters
constexpr int kChunkMax = RT_CHUNK_MAX; // slots a wave takes from the trace queue per atomic...
constexpr int kChunkMin = RT_CHUNK_MIN; // ...shrunk so that every wave gets ~4 chunks when few rays live
constexpr int kRefill = RT_REFILL;   // refill a wave once this many lanes are idle
constexpr int kRefillFirst = RT_REFILL_FIRST;   // same at bounce 0: a whole wave of consecutive primary rays
                                                // (~3 pixels) starts together and stays in lockstep
constexpr int kQueues = RT_QUEUES;   // trace queue shards (one per XCD group of workgroups)
constexpr int kQueueStride = 64;     // words between shards (256 B: one shard per cache line)

struct DevScene {
    const float4 *spheres;            // center.xyz, radius
    const float4 *tris;               // 3 x float4: p1.xyz e1.x | e1.yz e2.xy | e2.z n.xyz
    const uint16_t *mat_idx;
    const float4 *mats;               // 3 x float4: diffuse,metal | specular,rough | emit,ior
    const float4 *nodes;              // 4 x float4 per internal node (child-pair record, bvh_records.h)
    const int2 *big_leaves;           // {begin, end} for leaves that do not fit a ref
    const float *env;                 // env_h * env_w * 3
    int sphere_count, env_w, env_h, width, height;
    uint32_t root_ref;
    V3 cam, tl, sr, su, min_coord, inv_dim;
    float inv_w, inv_h;
};

struct Counters {                     // device-side work counters (u64, one atomic per wave)
    unsigned long long live, pn, iv, tt, st, hits, misses, hits_sphere;
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

__device__ __forceinline__ uint32_t rank_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// ---------------------------------------------------------------- traversal
typedef float f2 __attribute__((ext_vector_type(2)));

// Both children's slab tests (ray_aabb_intersection, scene.cu:109-132) on the interleaved node
// record {lx0 lx1 ly0 ly1} {lz0 lz1 hx0 hx1} {hy0 hy1 hz0 hz1}: the plane distances of the two
// boxes share packed-fp32 ops.  The reference folds the three axes in sequence,
//   tmin = fminf(fmaxf(t1, tmin), fmaxf(t2, tmin)),  tmax = fmaxf(fminf(t1, tmax), fminf(t2, tmax)),
// which for NaN-free t1/t2 is exactly tmin = max(min_x, min_y, min_z, 0) and
// tmax = min(max_x, max_y, max_z, closest) (min/max do not round; zero signs never reach a
// comparison outcome).  t is NaN only for 0 * inf, so the caller uses this form only when all of
// 1/d is finite and otherwise the literal per-axis fold (slab()).
__device__ __forceinline__ void slab_pair(float4 a, float4 b, float4 c, V3 o, float ix, float iy, float iz,
                                          float closest, bool &h0, bool &h1, float &t0, float &t1) {
    const f2 ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
    const f2 vx = {ix, ix}, vy = {iy, iy}, vz = {iz, iz};
    const f2 lx = {a.x, a.y}, ly = {a.z, a.w}, lz = {b.x, b.y};
    const f2 hx = {b.z, b.w}, hy = {c.x, c.y}, hz = {c.z, c.w};
    const f2 x1 = (lx - ox) * vx, x2 = (hx - ox) * vx;
    const f2 y1 = (ly - oy) * vy, y2 = (hy - oy) * vy;
    const f2 z1 = (lz - oz) * vz, z2 = (hz - oz) * vz;
    const float n0 = fmaxf(fmaxf(fminf(x1.x, x2.x), fminf(y1.x, y2.x)), fmaxf(fminf(z1.x, z2.x), 0.0f));
    const float f0 = fminf(fminf(fmaxf(x1.x, x2.x), fmaxf(y1.x, y2.x)), fminf(fmaxf(z1.x, z2.x), closest));
    const float n1 = fmaxf(fmaxf(fminf(x1.y, x2.y), fminf(y1.y, y2.y)), fmaxf(fminf(z1.y, z2.y), 0.0f));
    const float f1 = fminf(fminf(fmaxf(x1.y, x2.y), fmaxf(y1.y, y2.y)), fminf(fmaxf(z1.y, z2.y), closest));
    t0 = n0; t1 = n1;
    h0 = n0 <= f0;
    h1 = n1 <= f1;
}

// Möller–Trumbore (scene.cu:160-195, rt_device.h ray_triangle) with the early-outs folded into one
// predicate: every quantity is computed for every lane and the accept test is the conjunction of
// the reference's four reject tests, negated exactly as written (a NaN u, v or t rejects nothing,
// as in the branchy form).  Same values, same outcome; no divergent exec-mask regions.  In a wave
// of ~20 leaf lanes an early-out almost never skips work for all of them, so the nested branches
// only cost their exec-mask bookkeeping (round 3, with the flat pop loop below: A/B teapot full
// frame 6.94 -> 6.86 ms/pass over 5 rounds, 7.06 -> 6.86 over 3; 20 steps 7.24 -> 7.18, 7.27 -> 7.13).
__device__ __forceinline__ bool ray_triangle_flat(V3 o, V3 d, V3 p1, V3 e1, V3 e2, float closest, float &t) {
    const V3 h = cross(d, e2);
    const float a = dot(h, e1);
    const float f = 1 / a;
    const V3 s = o - p1;
    const float u = dot(s, h) * f;
    const V3 q = cross(s, e1);
    const float v = dot(d, q) * f;
    t = dot(e2, q) * f;
    const bool ok_a = a != 0;
    const bool ok_u = !(u < 0 || u > 1);
    const bool ok_v = !(v < 0 || u + v > 1);
    const bool ok_t = !(t < kEps || t >= closest);
    return ok_a & ok_u & ok_v & ok_t;
}

// Triangle range [ti, te) of a leaf ref (small leaves inline, big ones through big_leaves).
__device__ __forceinline__ void leaf_range(const DevScene &S, uint32_t ref, int &ti, int &te) {
    if (ref & kBigLeaf) {
        const int2 be = S.big_leaves[ref & 0x3FFFFFFFu];
        ti = be.x; te = be.y;
    } else {
        ti = (int)(ref & 0xFFFFFFu);
        te = ti + (int)((ref >> 24) & 0x3Fu);
    }
}

// ==================================================================== host side
inline int hip_fail(hipError_t e, const char *what) {
    return fail(e == hipErrorOutOfMemory ? RT_E_OOM : RT_E_HIP, std::string("Error ") + what + " " + hipGetErrorString(e));
}
#define HIPCHK(call)                                                 \
    do {                                                             \
        const hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) return ::rtamd::hip_fail(e_, #call);   \
    } while (0)

inline int blocks_for(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t count) {
        if (p) { (void)hipFree(p); p = nullptr; }
        n = count;
        if (!count) return RT_OK;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T)));
        return RT_OK;
    }
    // `pad` zeroed elements after the copied ones (readable slack for over-wide loads)
    int upload(const void *src, size_t count, hipStream_t s, size_t pad = 0) {
        int rc = alloc(count + pad);
        if (rc) return rc;
        if (count) HIPCHK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s));
        if (pad) HIPCHK(hipMemsetAsync(p + count, 0, pad * sizeof(T), s));
        return RT_OK;
    }
};

// A scene resident on one device (scene_dev.hip): the arrays the kernels read, the striped work counters,
// and the DevScene that points at them.  rt_renderer and rt_query each own one.
struct SceneDev {
    int device = 0, cus = 0;
    DevScene ds{};
    DevBuf<float4> spheres, tris, mats, nodes;   // tris: one float4 of slack behind the last record
    DevBuf<uint16_t> mat_idx;
    DevBuf<int2> big;
    DevBuf<float> env;
    DevBuf<Counters> ctr;             // kCtrSlots
    std::vector<int> node_rec;        // node -> child-pair record (-1: leaf), bvh_records.h

    // Validates the node array, lays out the records and uploads everything on s; returns once the
    // device holds the scene.  The caller has made `device` current.
    int init(const rt_scene *sc, int device, hipStream_t s);
    // The counter slots summed (a blocking copy: whatever wrote them must have finished).
    int read_counters(Counters &sum) const;
};

// Argument checks shared by the object constructors (scene_dev.hip): the scene's, then the options
// (null: rt_default_opts) copied to `o` with the device and the tile index checked.
int check_scene(const rt_scene *s);
int resolve_opts(const rt_scene *scene, const rt_opts *opts, rt_opts &o);

// trace_kernel<false, COUNT, 0> (closest hit of the live slots of `geo`, rt_render.hip) for rt_query.hip:
// every instantiation of the kernel is compiled once, in rt_render.hip.
int trace_closest_blocks_per_cu(int &per_cu);
void launch_trace_closest(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint32_t *live,
                          uint32_t *queue, float2 *hits, uint32_t *overflow, Counters *ctr);

// closest_point_kernel (closest_point.hip) for rt_query.hip: the ingest of n points into `geo`
// (one float4 each) and the traversal, enqueued on s.
int closest_point_blocks_per_cu(int &per_cu);
void launch_closest_point(bool count, int n, int grid, hipStream_t s, const DevScene &ds, const float *d_points,
                          const float *d_max_dist, float4 *geo, uint32_t *live, uint32_t *queue,
                          const rt_closest_point_out &out, uint32_t *overflow, Counters *ctr);
// point_ingest_kernel alone (closest_point.hip), for the other point query
void launch_point_ingest(int n, hipStream_t s, const float *d_points, const float *d_max_dist, float4 *geo, uint32_t *live,
                         uint32_t *queue, Counters *ctr);

// nearest_k_kernel (nearest_k.hip) for rt_query.hip: the traversal with the bound held, over points
// already ingested into `geo`.  ld / li: each point's k list rows (dist2 while it runs, the distance afterwards, and
// the index), both null = count only; point (n x k x 3) and count (n) are optional.
constexpr int kAnyStackLds = 16;      // 4-B stack entries per lane in LDS of the fixed-bound kernels
int nearest_k_blocks_per_cu(int &per_cu);
void launch_nearest_k(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint32_t *live,
                      uint32_t *queue, int k, float *ld, int32_t *li, float *point, int32_t *count_out, uint32_t *overflow,
                      Counters *ctr);

// filtered_closest_kernel and filtered_anyhit_kernel (ray_filter.hip) for rt_query.hip: the ingest of n
// rays and their filter (a host struct of device pointers, each optional) into `geo` (the ray's lower bound in the
// slot's spare word) and `fil` ({skip, ray mask} per ray), and the two traversals.  masks: the object's primitive
// mask words, or null when it holds none.  The closest one writes {t, index} records for the egest kernels.
int ray_filter_blocks_per_cu(int &per_cu_closest, int &per_cu_anyhit);
void launch_filter_ingest(int n, hipStream_t s, const float *d_rays, const rt_ray_filter &f, float4 *geo, uint2 *fil,
                          uint32_t *live, uint32_t *queue, Counters *ctr);
void launch_filtered_closest(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint2 *fil,
                             const uint32_t *masks, const uint32_t *live, uint32_t *queue, float2 *hits, uint32_t *overflow,
                             Counters *ctr);
void launch_filtered_anyhit(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint2 *fil,
                            const uint32_t *masks, const uint32_t *live, uint32_t *queue, uint8_t *out, uint32_t *overflow,
                            Counters *ctr);

// hemisphere_kernel (hemisphere.hip) for rt_query.hip: the ingest of n frames and their filter into `geo`
// (the unit normal in the direction's place), `fil` and `count` (zeroed), starting the queue with live_count = n * S
// work items; the traversal, which adds each point's escaped sample rays to count[i]; and the egest of the counts.
int hemisphere_blocks_per_cu(int &per_cu);
void launch_hemisphere_ingest(int n, hipStream_t s, const float *d_frames, const rt_ray_filter &f, uint32_t live_count,
                              float4 *geo, uint2 *fil, uint32_t *count, uint32_t *live, uint32_t *queue, Counters *ctr);
void launch_hemisphere(bool count_work, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint2 *fil,
                       const uint32_t *masks, const uint32_t *live, uint32_t *queue, uint32_t *count,
                       const rt_hemisphere_params &p, uint32_t *overflow, Counters *ctr);
void launch_hemisphere_egest(int n, hipStream_t s, const uint32_t *count, int32_t samples, const rt_hemisphere_out &out);

// box_overlap_kernel (box_overlap.hip) for rt_query.hip: the ingest of n boxes into `geo` (two float4 per
// box: {lo, valid} {hi, 0}) and the traversal; out: device pointers, each optional (index null = nothing kept, only any
// given = the walk stops at a box's first member).
int box_overlap_blocks_per_cu(int &per_cu);
void launch_box_ingest(int n, hipStream_t s, const float *d_boxes, float4 *geo, uint32_t *live, uint32_t *queue,
                       Counters *ctr);
void launch_box_overlap(bool count, int grid, hipStream_t s, const DevScene &ds, const float4 *geo, const uint32_t *live,
                        uint32_t *queue, int k, const rt_overlap_out &out, uint32_t *overflow, Counters *ctr);

}  // namespace rtamd
