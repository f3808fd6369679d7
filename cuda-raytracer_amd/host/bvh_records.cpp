// bvh_records.cpp — layout and validation of the child-pair node records (bvh_records.h).
#include "bvh_records.h"

#include <algorithm>
#include <cstring>
#include <utility>

namespace rtamd {
namespace records {

namespace {
bool is_leaf(const rt_bvh_node &nd) { return nd.child2 <= nd.child1; }   // scene.cu:859
}

std::string build(const rt_scene *sc, int max_depth, Records &out) {
    const int nn = sc->bvh_node_count;
    std::vector<int> &rec = out.node_rec;
    rec.assign((size_t)std::max(nn, 0), -1);
    int nrec = 0;
    if (nn > 0 && !is_leaf(sc->bvh[0])) {
        rec[0] = 0;
        nrec = 2;                       // record 1: padding
        std::vector<std::pair<int, int>> todo{{0, 0}};   // (internal node, its depth)
        int visited = 0;
        while (!todo.empty()) {
            const int i = todo.back().first, depth = todo.back().second;
            todo.pop_back();
            if (++visited > nn) return "BVH is not a tree";
            if (depth + 1 > max_depth)
                return "BVH deeper than the traversal stack (" + std::to_string(max_depth) + " internal levels)";
            const rt_bvh_node &nd = sc->bvh[i];
            if (nd.child1 < 0 || nd.child2 >= nn || nd.child1 >= nn || nd.child2 < 0) return "BVH child index out of range";
            const bool in1 = !is_leaf(sc->bvh[nd.child1]), in2 = !is_leaf(sc->bvh[nd.child2]);
            if (in1) rec[nd.child1] = nrec;
            if (in2) rec[nd.child2] = nrec + 1;
            if (in1 || in2) nrec += 2;
            if (in2) todo.push_back({nd.child2, depth + 1});   // child1's subtree first (depth-first)
            if (in1) todo.push_back({nd.child1, depth + 1});
        }
    }
    out.big.clear();
    auto ref_of = [&](int c) -> uint32_t {
        const rt_bvh_node &nd = sc->bvh[c];
        if (!is_leaf(nd)) return (uint32_t)rec[c];
        const int begin = nd.child2, count = nd.child1 - nd.child2;
        if (count < 64 && begin < (1 << 24)) return kLeaf | ((uint32_t)count << 24) | (uint32_t)begin;
        out.big.push_back({nd.child2, nd.child1});
        return kLeaf | kBigLeaf | (uint32_t)(out.big.size() - 1);
    };
    out.rows.assign((size_t)std::max(nrec, 1) * 4, Row{0.0f, 0.0f, 0.0f, 0.0f});
    for (int i = 0; i < nn; i++) {
        if (rec[i] < 0) continue;
        const rt_bvh_node &nd = sc->bvh[i];
        const rt_bvh_node &l = sc->bvh[nd.child1], &r = sc->bvh[nd.child2];
        Row *q = &out.rows[(size_t)rec[i] * 4];
        q[0] = {l.min_bound.x, r.min_bound.x, l.min_bound.y, r.min_bound.y};
        q[1] = {l.min_bound.z, r.min_bound.z, l.max_bound.x, r.max_bound.x};
        q[2] = {l.max_bound.y, r.max_bound.y, l.max_bound.z, r.max_bound.z};
        const uint32_t a = ref_of(nd.child1), b = ref_of(nd.child2);
        std::memcpy(&q[3].x, &a, 4);
        std::memcpy(&q[3].y, &b, 4);
    }
    out.root_ref = nn > 0 ? ref_of(0) : (kLeaf | 0u);
    if (out.big.empty()) out.big.push_back({0, 0});
    return std::string();
}

void unpack(const Row *q, rt_vec3 &min1, rt_vec3 &max1, rt_vec3 &min2, rt_vec3 &max2) {
    min1 = {q[0].x, q[0].z, q[1].x};
    max1 = {q[1].z, q[2].x, q[2].z};
    min2 = {q[0].y, q[0].w, q[1].y};
    max2 = {q[1].w, q[2].y, q[2].w};
}

}  // namespace records
}  // namespace rtamd
