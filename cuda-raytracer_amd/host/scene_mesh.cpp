// scene_mesh.cpp — rt_scene_from_mesh and rt_scene_from_mesh_device (include/rt_abi.h): a scene from
// vertex and index arrays instead of a scene file.  The result is defined as what rt_scene_load makes of the
// description's canonical scene file, so this file only turns the description into the state the loader has after
// its last line and hands it to the loader's own tail (finish_scene, scene_load.cpp).  No HIP dependency: the
// device entry passes the device pointers on to the device build, which scene_load.cpp reaches by a weak reference.
#include "rt_abi.h"
#include "rt_host.h"

#include <cmath>
#include <string>
#include <vector>

using namespace rtamd;

namespace {

rt_vec3 normalise(rt_vec3 v) {                        // scene_load.cpp's, as the `camera` line applies it
    const float s = 1.0f / sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return {s * v.x, s * v.y, s * v.z};
}

// Everything that can be refused without looking at a triangle, and the scene state a file's non-triangle lines
// leave behind.  `device`: the triangle arrays are device memory and are not read here.
int begin_scene(const char *who, const rt_mesh_desc *m, const rt_load_opts &opts, rt_scene_host *s,
                std::vector<uint16_t> &sphere_mats, bool &have_env, int32_t &material_count) {
    const std::string w(who);
    if (m->vertex_count < 0 || m->triangle_count < 0 || m->sphere_count < 0 || m->material_count < 0)
        return fail(RT_E_INVALID, w + ": negative count");
    if (!m->vertices && m->triangle_count > 0)
        return fail(RT_E_INVALID, w + ": null vertices with " + std::to_string(m->triangle_count) + " triangles");
    if (!m->indices && (int64_t)m->vertex_count != 3 * (int64_t)m->triangle_count)
        return fail(RT_E_INVALID, w + ": a soup of " + std::to_string(m->triangle_count) + " triangles needs " +
                                      std::to_string(3 * (int64_t)m->triangle_count) + " vertices, not " +
                                      std::to_string(m->vertex_count));
    if (!m->spheres && m->sphere_count > 0)
        return fail(RT_E_INVALID, w + ": null spheres with " + std::to_string(m->sphere_count) + " spheres");
    const bool table = m->materials && m->material_count > 0;
    if (!table && (m->triangle_materials || m->sphere_materials))
        return fail(RT_E_INVALID, w + ": material indices without a material table");
    if (m->material_count > 65535) return fail(RT_E_INVALID, w + ": more than 65535 materials");
    if ((int64_t)m->sphere_count + (int64_t)m->triangle_count > 0x7fffffff)
        return fail(RT_E_INVALID, w + ": sphere_count + triangle_count does not fit int32");
    rt_scene &v = s->view;
    scene_defaults(v);
    if (int rc = apply_image_opts(v, opts)) return rc;
    if (table) {
        s->materials.assign(m->materials, m->materials + m->material_count);
    } else {                                          // a `material` line with no parameters
        rt_material d{};
        d.diffuse_albedo = {1, 1, 1};
        d.specular_albedo = {1, 1, 1};
        s->materials.assign(1, d);
    }
    material_count = (int32_t)s->materials.size();
    if (m->sphere_count) s->spheres.assign(m->spheres, m->spheres + m->sphere_count);
    sphere_mats.assign((size_t)m->sphere_count, 0);
    if (m->sphere_materials)
        for (int32_t i = 0; i < m->sphere_count; i++) {
            if (m->sphere_materials[i] >= material_count) return mesh_bad_material("sphere", i, material_count);
            sphere_mats[i] = m->sphere_materials[i];
        }
    have_env = m->sky != nullptr;
    if (m->sky) {
        s->env.assign(1, *m->sky);
        v.environment_map_width = v.environment_map_height = 1;
    }
    if (const rt_camera_desc *c = m->camera) {        // the `camera` line (scene_load.cpp)
        v.camera_position = c->position;
        v.forward = normalise(c->forward);
        v.up = normalise(c->up);
        v.vertical_fov = (float)(c->vertical_fov_degrees * (3.14159265358979323846 / 180));
    }
    return RT_OK;
}

int from_mesh(const char *who, const rt_mesh_desc *m, const rt_load_opts *opts_in, void *stream, bool device,
              rt_scene_host **out) {
    if (!m || !out) return fail(RT_E_INVALID, std::string(who) + ": null argument");
    *out = nullptr;
    rt_load_opts opts;
    if (opts_in) opts = *opts_in; else rt_default_load_opts(&opts);
    if (device && opts.bvh_device < 0)
        return fail(RT_E_INVALID, std::string(who) + ": opts->bvh_device must name the device the arrays are on");
    auto s = new rt_scene_host();
    auto bad = [&](int code) { delete s; return code; };
    std::vector<uint16_t> sphere_mats, tri_mats;
    bool have_env = false;
    int32_t material_count = 0;
    // the refusals of both entries carry the host entry's name: the same description, the same message
    if (int rc = begin_scene("rt_scene_from_mesh", m, opts, s, sphere_mats, have_env, material_count)) return bad(rc);
    if (device) {
        const MeshDeviceInput dm{m->vertices, m->vertex_count, m->indices, m->triangle_count, m->triangle_materials,
                                 material_count, opts.bvh_device, stream};
        if (int rc = finish_scene(s, opts, have_env, sphere_mats, tri_mats, &dm)) return bad(rc);
        *out = s;
        return RT_OK;
    }
    const int32_t n = m->triangle_count;
    tri_mats.assign((size_t)n, 0);
    if (m->triangle_materials)
        for (int32_t i = 0; i < n; i++) {
            if (m->triangle_materials[i] >= material_count) return bad(mesh_bad_material("triangle", i, material_count));
            tri_mats[i] = m->triangle_materials[i];
        }
    if (m->indices)                                   // before any vertex is read, and before any finiteness check
        for (int32_t i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) {
                const int32_t q = m->indices[3 * (size_t)i + k];
                if (q < 0 || q >= m->vertex_count) return bad(mesh_bad_vertex_index(i, m->vertex_count));
            }
    s->triangles.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {                 // the `triangle` line: build representation (p1, p2, p3, centroid)
        rt_vec3 p[3];
        for (int k = 0; k < 3; k++) {
            const size_t q = m->indices ? (size_t)m->indices[3 * (size_t)i + k] : 3 * (size_t)i + k;
            p[k] = {m->vertices[3 * q], m->vertices[3 * q + 1], m->vertices[3 * q + 2]};
        }
        const float third = 1.0f / 3.0f;
        s->triangles[i] = rt_triangle{p[0], p[1], p[2],
                                      {third * ((p[0].x + p[1].x) + p[2].x), third * ((p[0].y + p[1].y) + p[2].y),
                                       third * ((p[0].z + p[1].z) + p[2].z)}};
    }
    if (int rc = finish_scene(s, opts, have_env, sphere_mats, tri_mats, nullptr)) return bad(rc);
    *out = s;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_from_mesh(const rt_mesh_desc *mesh, const rt_load_opts *opts, rt_scene_host **out) {
    return from_mesh("rt_scene_from_mesh", mesh, opts, nullptr, false, out);
}

int rt_scene_from_mesh_device(const rt_mesh_desc *mesh, const rt_load_opts *opts, void *hip_stream, rt_scene_host **out) {
    return from_mesh("rt_scene_from_mesh_device", mesh, opts, hip_stream, true, out);
}

}  // extern "C"
