// bvh_refit.h — device refit of a resident scene (csrc/bvh_refit.hip), used by rt_query (rt_query.hip).
#pragma once
#include "rt_abi.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

namespace rtamd {

// Built once per object, on the host, from the record numbering of bvh_records.h: the
// records sorted by depth (deepest level first), the level offsets, the launch list and the record ->
// node map.  Everything an update needs on the device is allocated here, so updates allocate nothing.
struct RefitPlan {
    int32_t triangle_count = 0;
    bool root_leaf = true;                  // no records: the root is a leaf (no_bvh, tiny scenes)
    std::vector<rt_bvh_node> bvh;           // host copy of the scene's nodes (children; read_geometry)
    std::vector<int32_t> rec_node;          // record -> node whose children it holds; -1 = padding
    std::vector<uint32_t> level_off;        // level k (deepest first) = order[level_off[k], level_off[k + 1])
    struct Launch { int first_level, level_count; };
    // Deepest first.  A run of consecutive levels of at most one workgroup each is one single-workgroup
    // launch (levels separated by __syncthreads()); every wider level is a launch of its own.
    std::vector<Launch> launches;
    std::string invalid;                    // why this scene cannot be refitted (a leaf range out of bounds), or empty
    uint32_t *d_order = nullptr;            // record numbers, level by level
    uint32_t *d_level_off = nullptr;
    float4 *d_root_box = nullptr;           // {lo, hi} of a root leaf, which no record holds
    float *d_stage = nullptr;               // vertices of the host-pointer update (first such call)

    ~RefitPlan();
    // node_rec: node -> its child-pair record (-1 for leaves), records::build's numbering
    int build(const rt_scene *sc, const std::vector<int> &node_rec, hipStream_t s);
    // Enqueues the triangle kernel and the level launches on s.  tris: the 48-B records (+ slack),
    // nodes: the 64-B child-pair records, big: the {begin, end} table of big leaves.
    int enqueue(const float *d_vertices, float4 *tris, float4 *nodes, const int2 *big, hipStream_t s) const;
};

}  // namespace rtamd
