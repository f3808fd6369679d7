// scene_refit.cpp — rt_scene_refit (include/rt_abi.h): the host twin of the device refit
// (csrc/bvh_refit.hip).  New vertices under the frozen topology: every triangle record and every
// node's bounds are rewritten in place, child indices, leaf ranges, triangle order and material
// indices stay.  No HIP dependency: this file compiles alone.
#include "rt_abi.h"
#include "rt_host.h"
#include "bvh_refit_math.h"

#include <vector>

using namespace rtamd;
using refit::Box;

extern "C" int rt_scene_refit(rt_scene_host *scene, const float *vertices, int32_t triangle_count) {
    if (!scene) return fail(RT_E_INVALID, "rt_scene_refit: null scene");
    const int32_t n = (int32_t)scene->triangles.size();
    if (triangle_count != n)
        return fail(RT_E_INVALID, "rt_scene_refit: triangle_count " + std::to_string(triangle_count) +
                                      " is not the scene's " + std::to_string(n));
    if (n == 0) return RT_OK;
    if (!vertices) return fail(RT_E_INVALID, "rt_scene_refit: null vertices pointer");
    std::vector<rt_bvh_node> &bvh = scene->bvh;
    const int nn = (int)bvh.size();
    // the builder appends a node's children after it, so a descending sweep meets children first
    for (int i = 0; i < nn; i++) {
        const rt_bvh_node &nd = bvh[i];
        const bool leaf = nd.child2 <= nd.child1;
        if (leaf ? (nd.child2 < 0 || nd.child1 > n) : (nd.child1 <= i || nd.child2 >= nn))
            return fail(RT_E_INVALID, "rt_scene_refit: BVH is not in the builder's order");
    }
    std::vector<Box> tri_box((size_t)n);
    for (int i = 0; i < n; i++) {
        const float *v = vertices + (size_t)i * 9;
        scene->triangles[i] = refit::triangle_record(v);
        tri_box[i] = refit::triangle_box(v);
    }
    for (int i = nn - 1; i >= 0; i--) {
        rt_bvh_node &nd = bvh[i];
        Box b = refit::empty_box();
        if (nd.child2 <= nd.child1) {
            for (int t = nd.child2; t < nd.child1; t++) refit::grow(b, tri_box[t]);
        } else {
            refit::grow(b, Box{bvh[nd.child1].min_bound, bvh[nd.child1].max_bound});
            refit::grow(b, Box{bvh[nd.child2].min_bound, bvh[nd.child2].max_bound});
        }
        nd.min_bound = b.lo;
        nd.max_bound = b.hi;
    }
    // Reorder-key bounds, as the loader computes them (scene.cu:822-830)
    rt_scene &v = scene->view;
    v.min_coord = bvh[0].min_bound;
    rt_vec3 mx = bvh[0].max_bound;
    for (const rt_sphere &sp : scene->spheres) {
        const float r = sp.radius;
        mx = {refit::fmax_(mx.x, sp.center.x + r), refit::fmax_(mx.y, sp.center.y + r), refit::fmax_(mx.z, sp.center.z + r)};
        v.min_coord = {refit::fmin_(v.min_coord.x, sp.center.x - r), refit::fmin_(v.min_coord.y, sp.center.y - r),
                       refit::fmin_(v.min_coord.z, sp.center.z - r)};
    }
    v.inv_dimensions = {1 / mx.x, 1 / mx.y, 1 / mx.z};
    return RT_OK;
}
