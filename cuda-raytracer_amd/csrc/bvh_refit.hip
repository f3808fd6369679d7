// bvh_refit.hip — refit of a resident scene on gfx950 (rt_query_update_triangles).
//
// New vertices under the frozen topology: the 48-B triangle records and the three bound words of every
// 64-B child-pair node record are rewritten in place, bit-identical to the host twin rt_scene_refit
// (host/scene_refit.cpp; both evaluate host/bvh_refit_math.h).  The refs in a record's word 3 are only read.
//
// Level-synchronous, deepest level first: a record's slot is either a leaf (folded from the leaf's
// vertices in index order) or an internal child, whose box is the merge of the two boxes in that child's
// own record, which is one level deeper and was written by an earlier launch.  Workgroups hand results to
// each other at kernel boundaries only: no counters, flags or spins.  Levels that fit one workgroup
// are chained inside a single-workgroup launch with __syncthreads() between them (one workgroup runs on
// one CU, whose waves share its L1), so a 30-level chain is one launch.
#include "bvh_refit.h"
#include "bvh_refit_math.h"
#include "rt_common.h"

#include <algorithm>
#include <string>
#include <utility>

namespace rtamd {
namespace {

using refit::Box;

// One thread per triangle: 36 B in (through LDS, so the block's 9 KB are read coalesced), the 48-B
// record out.  The slack float4 behind the last record is not touched.
__global__ __launch_bounds__(kBlock) void refit_triangles_kernel(const float *__restrict__ v, int n, float4 *__restrict__ tris) {
    __shared__ float sv[kBlock * 9];
    const size_t base = (size_t)blockIdx.x * kBlock;
    const int cnt = min(kBlock, n - (int)base);
    for (int k = threadIdx.x; k < cnt * 9; k += kBlock) sv[k] = v[base * 9 + k];
    __syncthreads();
    if ((int)threadIdx.x >= cnt) return;
    float w[9];
    for (int k = 0; k < 9; k++) w[k] = sv[threadIdx.x * 9 + k];
    const rt_triangle t = refit::triangle_record(w);
    float4 *out = tris + (base + threadIdx.x) * 3;
    out[0] = make_float4(t.p1.x, t.p1.y, t.p1.z, t.p2p1.x);
    out[1] = make_float4(t.p2p1.y, t.p2p1.z, t.p3p1.x, t.p3p1.y);
    out[2] = make_float4(t.p3p1.z, t.normal.x, t.normal.y, t.normal.z);
}

// Box of one slot of a record.  Leaf ref: its triangles' vertices in index order.  Internal ref: the
// two boxes stored in that child's record (child1's, then child2's).
__device__ __forceinline__ Box slot_box(uint32_t ref, const float4 *nodes, const float *v, const int2 *big) {
    Box b = refit::empty_box();
    if (ref & kLeaf) {
        int ti, te;
        if (ref & kBigLeaf) {
            const int2 be = big[ref & 0x3FFFFFFFu];
            ti = be.x; te = be.y;
        } else {
            ti = (int)(ref & 0xFFFFFFu);
            te = ti + (int)((ref >> 24) & 0x3Fu);
        }
        for (int i = ti; i < te; i++) refit::grow(b, refit::triangle_box(v + (size_t)i * 9));
    } else {
        const float4 *c = nodes + (size_t)ref * 4;
        const float4 q0 = c[0], q1 = c[1], q2 = c[2];
        refit::grow(b, Box{{q0.x, q0.z, q1.x}, {q1.z, q2.x, q2.z}});
        refit::grow(b, Box{{q0.y, q0.w, q1.y}, {q1.w, q2.y, q2.w}});
    }
    return b;
}

__device__ __forceinline__ void refit_record(uint32_t rec, float4 *nodes, const float *v, const int2 *big) {
    float4 *q = nodes + (size_t)rec * 4;
    const float4 refs = q[3];
    const Box l = slot_box(__float_as_uint(refs.x), nodes, v, big);
    const Box r = slot_box(__float_as_uint(refs.y), nodes, v, big);
    // the two children's bounds interleaved per plane (bvh_records.h)
    q[0] = make_float4(l.lo.x, r.lo.x, l.lo.y, r.lo.y);
    q[1] = make_float4(l.lo.z, r.lo.z, l.hi.x, r.hi.x);
    q[2] = make_float4(l.hi.y, r.hi.y, l.hi.z, r.hi.z);
}

// One level: one thread per record of order[begin, begin + count).
__global__ __launch_bounds__(kBlock) void refit_level_kernel(const uint32_t *__restrict__ order, uint32_t begin, uint32_t count,
                                                           float4 *nodes, const float *__restrict__ v,
                                                           const int2 *__restrict__ big) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < count) refit_record(order[begin + k], nodes, v, big);
}

// Levels [first, first + levels), each of at most kBlock records, in ONE workgroup: a level's stores are
// complete and visible to the workgroup's other waves after the barrier (they share the CU's L1).
__global__ __launch_bounds__(kBlock) void refit_chain_kernel(const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ level_off, int first, int levels,
                                                           float4 *nodes, const float *__restrict__ v,
                                                           const int2 *__restrict__ big) {
    for (int l = first; l < first + levels; l++) {
        const uint32_t begin = level_off[l], count = level_off[l + 1] - begin;
        if (threadIdx.x < count) refit_record(order[begin + threadIdx.x], nodes, v, big);
        __syncthreads();
    }
}

// The box of a root leaf (triangles [first, first + n)), which no record stores and no traversal reads: kept so that
// rt_query_read_geometry can report the node.  One workgroup; each thread folds a contiguous chunk in
// index order and thread 0 folds the partial boxes in thread order, which equals the linear fold.
__global__ __launch_bounds__(kBlock) void refit_root_leaf_kernel(const float *__restrict__ v, int first, int n,
                                                               float4 *root_box) {
    __shared__ Box part[kBlock];
    const int chunk = (n + kBlock - 1) / kBlock;
    const int lo = min(n, (int)threadIdx.x * chunk), hi = min(n, lo + chunk);
    Box b = refit::empty_box();
    for (int i = first + lo; i < first + hi; i++) refit::grow(b, refit::triangle_box(v + (size_t)i * 9));
    part[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x != 0) return;
    Box all = refit::empty_box();
    for (int t = 0; t < kBlock; t++) refit::grow(all, part[t]);
    root_box[0] = make_float4(all.lo.x, all.lo.y, all.lo.z, 0.0f);
    root_box[1] = make_float4(all.hi.x, all.hi.y, all.hi.z, 0.0f);
}

}  // namespace

RefitPlan::~RefitPlan() {
    if (d_order) (void)hipFree(d_order);
    if (d_level_off) (void)hipFree(d_level_off);
    if (d_root_box) (void)hipFree(d_root_box);
    if (d_stage) (void)hipFree(d_stage);
}

int RefitPlan::build(const rt_scene *sc, const std::vector<int> &node_rec, hipStream_t s) {
    triangle_count = sc->triangle_count;
    const int nn = sc->bvh_node_count;
    bvh.assign(sc->bvh, sc->bvh + nn);
    auto leaf = [&](int i) { return bvh[i].child2 <= bvh[i].child1; };
    root_leaf = leaf(0);
    invalid.clear();
    for (int i = 0; i < nn; i++)
        if (leaf(i) && bvh[i].child2 < bvh[i].child1 && (bvh[i].child2 < 0 || bvh[i].child1 > triangle_count))
            invalid = "a leaf's triangle range leaves the scene's triangles";
    int nrec = 0;
    for (int i = 0; i < nn; i++) nrec = std::max(nrec, node_rec[i] + 1);
    nrec = (nrec + 1) & ~1;                 // records come in pairs
    rec_node.assign((size_t)nrec, -1);
    std::vector<int> depth((size_t)nrec, -1);
    int max_depth = -1;
    if (!root_leaf) {
        // records::build has walked the tree (it is one, at most kStackMax levels, indices in range)
        std::vector<std::pair<int, int>> todo{{0, 0}};
        while (!todo.empty()) {
            const int i = todo.back().first, d = todo.back().second;
            todo.pop_back();
            rec_node[node_rec[i]] = i;
            depth[node_rec[i]] = d;
            max_depth = std::max(max_depth, d);
            for (int c : {bvh[i].child1, bvh[i].child2})
                if (!leaf(c)) todo.push_back({c, d + 1});
        }
    }
    // counting sort by depth, deepest first; record order within a level (neighbours stay neighbours)
    const int levels = max_depth + 1;
    level_off.assign((size_t)levels + 1, 0);
    for (int r = 0; r < nrec; r++)
        if (depth[r] >= 0) level_off[(size_t)(max_depth - depth[r]) + 1]++;
    for (int l = 0; l < levels; l++) level_off[l + 1] += level_off[l];
    std::vector<uint32_t> order(level_off[levels]), fill(level_off.begin(), level_off.end() - 1);
    for (int r = 0; r < nrec; r++)
        if (depth[r] >= 0) order[fill[max_depth - depth[r]]++] = (uint32_t)r;
    launches.clear();
    for (int l = 0; l < levels;) {
        int e = l + 1;
        if (level_off[l + 1] - level_off[l] <= (uint32_t)kBlock)
            while (e < levels && level_off[e + 1] - level_off[e] <= (uint32_t)kBlock) e++;
        launches.push_back({l, e - l});
        l = e;
    }
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_root_box), 2 * sizeof(float4)));
    const float4 box_h[2] = {make_float4(bvh[0].min_bound.x, bvh[0].min_bound.y, bvh[0].min_bound.z, 0.0f),
                             make_float4(bvh[0].max_bound.x, bvh[0].max_bound.y, bvh[0].max_bound.z, 0.0f)};
    HIPCHK(hipMemcpyAsync(d_root_box, box_h, sizeof(box_h), hipMemcpyHostToDevice, s));
    if (!order.empty()) {
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_order), order.size() * sizeof(uint32_t)));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_level_off), level_off.size() * sizeof(uint32_t)));
        HIPCHK(hipMemcpyAsync(d_order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_level_off, level_off.data(), level_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));        // the host vectors above go out of scope
    return RT_OK;
}

int RefitPlan::enqueue(const float *d_vertices, float4 *tris, float4 *nodes, const int2 *big, hipStream_t s) const {
    if (!invalid.empty()) return fail(RT_E_INVALID, "rt_query_update_triangles: " + invalid);
    const int n = triangle_count;
    hipLaunchKernelGGL(refit_triangles_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_vertices, n, tris);
    if (root_leaf) {
        hipLaunchKernelGGL(refit_root_leaf_kernel, dim3(1), dim3(kBlock), 0, s, d_vertices, bvh[0].child2,
                           std::max(0, bvh[0].child1 - bvh[0].child2), d_root_box);
    } else {
        for (const Launch &l : launches) {
            const uint32_t begin = level_off[l.first_level], count = level_off[l.first_level + 1] - begin;
            if (l.level_count == 1 && count > (uint32_t)kBlock)
                hipLaunchKernelGGL(refit_level_kernel, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_order, begin,
                                   count, nodes, d_vertices, big);
            else
                hipLaunchKernelGGL(refit_chain_kernel, dim3(1), dim3(kBlock), 0, s, d_order, d_level_off, l.first_level,
                                   l.level_count, nodes, d_vertices, big);
        }
    }
    HIPCHK(hipGetLastError());
    return RT_OK;
}

}  // namespace rtamd
