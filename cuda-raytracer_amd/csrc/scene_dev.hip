// scene_dev.hip — the resident scene (SceneDev, rt_common.h) and the argument checks shared by the
// renderer's and the query object's constructors.  Host code only: no kernels.
#include "rt_common.h"

#include <algorithm>
#include <utility>

namespace rtamd {

int SceneDev::init(const rt_scene *sc, int dev, hipStream_t s) {
    device = dev;
    records::Records r;
    const std::string err = records::build(sc, kStackMax, r);
    if (!err.empty()) return fail(RT_E_INVALID, err);
    node_rec = std::move(r.node_rec);
    int rc;
    if ((rc = spheres.upload(sc->spheres, sc->sphere_count, s))) return rc;
    // one float4 of slack: traversal reads 64 B at a triangle record (48 B) like at a node
    if ((rc = tris.upload(sc->triangles, (size_t)sc->triangle_count * 3, s, 1))) return rc;
    if ((rc = mats.upload(sc->materials, (size_t)sc->material_count * 3, s))) return rc;
    if ((rc = mat_idx.upload(sc->material_indices, (size_t)sc->sphere_count + sc->triangle_count, s))) return rc;
    if ((rc = nodes.upload(r.rows.data(), r.rows.size(), s))) return rc;
    if ((rc = big.upload(r.big.data(), r.big.size(), s))) return rc;
    if ((rc = env.upload(sc->environment_map, (size_t)sc->environment_map_width * sc->environment_map_height * 3, s)))
        return rc;
    if ((rc = ctr.alloc(kCtrSlots))) return rc;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    ds.spheres = spheres.p;
    ds.tris = tris.p;
    ds.mat_idx = mat_idx.p;
    ds.mats = mats.p;
    ds.nodes = nodes.p;
    ds.big_leaves = big.p;
    ds.env = env.p;
    ds.sphere_count = sc->sphere_count;
    ds.env_w = sc->environment_map_width;
    ds.env_h = sc->environment_map_height;
    ds.width = sc->width;
    ds.height = sc->height;
    ds.root_ref = r.root_ref;
    ds.cam = v3(sc->camera_position.x, sc->camera_position.y, sc->camera_position.z);
    ds.tl = v3(sc->near_plane_top_left.x, sc->near_plane_top_left.y, sc->near_plane_top_left.z);
    ds.sr = v3(sc->scaled_right.x, sc->scaled_right.y, sc->scaled_right.z);
    ds.su = v3(sc->scaled_up.x, sc->scaled_up.y, sc->scaled_up.z);
    ds.min_coord = v3(sc->min_coord.x, sc->min_coord.y, sc->min_coord.z);
    ds.inv_dim = v3(sc->inv_dimensions.x, sc->inv_dimensions.y, sc->inv_dimensions.z);
    ds.inv_w = sc->inv_width;
    ds.inv_h = sc->inv_height;
    HIPCHK(hipStreamSynchronize(s));        // the uploads read host vectors that end here
    return RT_OK;
}

int SceneDev::read_counters(Counters &sum) const {
    Counters slots[kCtrSlots];
    HIPCHK(hipMemcpy(slots, ctr.p, sizeof(slots), hipMemcpyDeviceToHost));
    sum = Counters{};
    for (const Counters &x : slots) {
        sum.live += x.live; sum.pn += x.pn; sum.iv += x.iv; sum.tt += x.tt; sum.st += x.st;
        sum.hits += x.hits; sum.misses += x.misses; sum.hits_sphere += x.hits_sphere;
    }
    return RT_OK;
}

int check_scene(const rt_scene *s) {
    if (!s) return fail(RT_E_INVALID, "null scene");
    if (s->width < 2 || s->height < 2 || s->ray_count < 0 || s->bounces < 0)
        return fail(RT_E_INVALID, "scene image must be at least 2x2 with non-negative spp/bounces");
    if (s->bvh_node_count < 1 || !s->bvh) return fail(RT_E_INVALID, "scene has no BVH root");
    if (s->environment_map_width < 1 || s->environment_map_height < 1 || !s->environment_map)
        return fail(RT_E_INVALID, "scene has no environment map");
    // sky_color keeps the reference's row stride of the map's height (scene.cu:389-391): texel ty * h + tx stays
    // below w * h only for w >= h (1 x 2 already reads index 2 of 2)
    if (s->environment_map_width < s->environment_map_height)
        return fail(RT_E_INVALID, "environment map is taller than wide: the sky lookup's row stride is the map's "
                                  "height, so it would read past the map's end");
    if ((s->sphere_count && !s->spheres) || (s->triangle_count && !s->triangles) || !s->materials ||
        (s->sphere_count + s->triangle_count && !s->material_indices))
        return fail(RT_E_INVALID, "scene array missing");
    return RT_OK;
}

int resolve_opts(const rt_scene *scene, const rt_opts *opts, rt_opts &o) {
    const int rc = check_scene(scene);
    if (rc) return rc;
    if (opts) o = *opts; else rt_default_opts(&o);
    if (rt_device_count() <= o.device || o.device < 0) return fail(RT_E_NODEVICE, "no such HIP device");
    if (o.tile_index < 0 || o.tile_index >= std::max(1, o.tile_count))
        return fail(RT_E_INVALID, "tile_index outside [0, tile_count)");
    return RT_OK;
}

}  // namespace rtamd
