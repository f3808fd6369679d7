// rt_host.h — internal helpers shared by the host-side translation units of librtamd.so.
#pragma once
#include "rt_abi.h"

#include <string>
#include <vector>

namespace rtamd {
extern thread_local std::string g_error;
// Records `msg` as the thread's rt_last_error() and returns `code`.
int fail(int code, const std::string &msg);
}  // namespace rtamd

// What rt_scene_load returns: the arrays its rt_scene view points into (scene_load.cpp fills it,
// scene_refit.cpp rewrites triangles and bounds in place).
struct rt_scene_host {
    rt_scene view{};
    std::vector<rt_sphere> spheres;
    std::vector<rt_triangle> triangles;
    std::vector<uint16_t> material_indices;
    std::vector<rt_material> materials;
    std::vector<rt_bvh_node> bvh;
    std::vector<rt_vec3> env;
    std::vector<int32_t> face_index;   // input index of scene triangle j (rt_scene_face_index); both builders fill it
    double bvh_ms = 0;
};

namespace rtamd {

// A mesh whose triangle arrays are device memory (rt_scene_from_mesh_device): what the device build reads.
struct MeshDeviceInput {
    const float *vertices;        int32_t vertex_count;
    const int32_t *indices;       int32_t triangle_count;   // NULL = soup
    const uint16_t *materials;    int32_t material_count;   // NULL = all 0; the table's (effective) size
    int device;
    void *stream;                 // synchronised before the first kernel reads the arrays
};

// Applies opts' image and exposure overrides to the view and checks the loader's image-size rule.
int apply_image_opts(rt_scene &v, const rt_load_opts &opts);

// The tail of rt_scene_load, shared with rt_scene_from_mesh (scene_mesh.cpp): overrides, validation, camera
// precompute, BVH build, ray-tracing records, reorder-key bounds and view wiring.  The scene arrives with its
// spheres, materials, env (when have_env), camera fields and image defaults set, and, unless `dm` is given,
// its triangles in build representation (p1, p2, p3, centroid).  With `dm` the triangles are assembled,
// validated, built and finalised on the device (csrc/mesh_ingest.hip) and tri_mats is ignored.
int finish_scene(rt_scene_host *s, const rt_load_opts &opts, bool have_env, const std::vector<uint16_t> &sphere_mats,
                 const std::vector<uint16_t> &tri_mats, const MeshDeviceInput *dm);

// The loader's scene defaults (scene.cu:571-574) on a fresh scene.
void scene_defaults(rt_scene &v);

// The mesh entries' refusals of a triangle's (or sphere's) material index and of a vertex index, worded once
// for the host checks and for what the device build's assemble kernel reports.
int mesh_bad_material(const char *what, int64_t i, int32_t material_count);
int mesh_bad_vertex_index(int64_t i, int32_t vertex_count);

}  // namespace rtamd
