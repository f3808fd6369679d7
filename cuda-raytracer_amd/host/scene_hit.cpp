// scene_hit.cpp — rt_scene_hit_records (include/rt_abi.h): the host twin of the hit-record egest kernel
// (csrc/rt_query.hip).  The records of given closest hits (t, index) on a host scene, through
// the same text (hit_record_math.h).  No HIP dependency: this file compiles alone.
#include "rt_abi.h"
#include "rt_host.h"
#include "hit_record_math.h"

#include <string>

using namespace rtamd;

extern "C" int rt_scene_hit_records(const rt_scene *scene, const float *rays, const float *t, const int32_t *index,
                                    int32_t n, const rt_hit_out *out) {
    if (!scene) return fail(RT_E_INVALID, "rt_scene_hit_records: null scene");
    if (n < 0) return fail(RT_E_INVALID, "rt_scene_hit_records: negative ray count");
    if (n == 0) return RT_OK;
    if (!rays || !t || !index || !out) return fail(RT_E_INVALID, "rt_scene_hit_records: null pointer");
    const int32_t S = scene->sphere_count, count = S + scene->triangle_count;
    for (int32_t i = 0; i < n; i++)
        if (index[i] >= count)
            return fail(RT_E_INVALID, "rt_scene_hit_records: index[" + std::to_string(i) + "] = " + std::to_string(index[i]) +
                                          " is not a primitive of the scene (" + std::to_string(count) + ")");
    for (int32_t i = 0; i < n; i++) {
        const float *r = rays + (size_t)i * 6;
        const rt_vec3 o{r[0], r[1], r[2]}, d{r[3], r[4], r[5]};
        const int32_t idx = index[i];
        hit::Record rec = hit::miss();
        if (idx >= S) {
            const rt_triangle &tr = scene->triangles[idx - S];
            rec = hit::triangle(o, d, t[i], tr.p1, tr.p2p1, tr.p3p1, tr.normal);
        } else if (idx >= 0) {
            const rt_sphere &sp = scene->spheres[idx];
            rec = hit::sphere(o, d, t[i], sp.center, sp.radius);
        }
        if (idx >= 0) rec.material = (int32_t)scene->material_indices[idx];
        if (out->uv) { out->uv[(size_t)i * 2] = rec.u; out->uv[(size_t)i * 2 + 1] = rec.v; }
        if (out->normal) {
            float *p = out->normal + (size_t)i * 3;
            p[0] = rec.normal.x; p[1] = rec.normal.y; p[2] = rec.normal.z;
        }
        if (out->position) {
            float *p = out->position + (size_t)i * 3;
            p[0] = rec.position.x; p[1] = rec.position.y; p[2] = rec.position.z;
        }
        if (out->material) out->material[i] = rec.material;
        if (out->front_face) out->front_face[i] = rec.front_face;
    }
    return RT_OK;
}
