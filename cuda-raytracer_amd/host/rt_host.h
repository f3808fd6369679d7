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
    double bvh_ms = 0;
};
