// closest_point_host_check.cpp — stand-alone driver of rt_scene_closest_point (the host twin, csrc/cpu_query.hip) for
// sanitizer runs on the CPU: no GPU, no Python.
//
// For every scene file on the command line ("path" or "path:no_bvh") it loads the scene, makes seeded points
// (uniform in the bounds inflated by 25 %, on triangles, at vertices, 1000 diagonals away, non-finite), runs the twin
// without max_dist and with a max_dist that cycles through 0, a finite radius, negative, NaN, +inf and 1e19, with
// every output alone, all and none, into exactly sized heap arrays, and compares the unbounded answer with a brute
// force over all primitives by the same functions (never nearer; differences are counted and printed).
//
//   D=cuda-raytracer_amd; I="-Iinclude -I$D/host -I$D/csrc"; S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   hipcc -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt --offload-arch=gfx950 \
//     $(for f in $S; do echo -Xarch_host $f; done) $I -c $D/csrc/cpu_query.hip -o cpu_query.o
//   clang++ -std=c++17 -O1 -g -ffp-contract=off $S $I tools/experiments/closest_point_host_check.cpp cpu_query.o \
//     $D/host/scene_load.cpp $D/host/image_io.cpp $D/host/bvh_records.cpp -lpthread -o closest_point_host_check
//   RT_ASSETS=assets ./closest_point_host_check assets/cornell.scene assets/cornell.scene:no_bvh assets/teapot.scene ...
// (clang++ = the clang hipcc drives, so that both objects carry the same sanitizer runtime.)
#include "rt_abi.h"
#include "closest_point_math.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace cp = rtamd::cp;

namespace rtamd {
// the loader's device BVH build (csrc/bvh_build.hip) is not linked: this driver builds on the host only
int gpu_build_bvh(std::vector<rt_triangle> &, uint16_t *, std::vector<rt_bvh_node> &, int, int) { return RT_E_NODEVICE; }
}  // namespace rtamd

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

int main(int argc, char **argv) {
    int failures = 0;
    for (int a = 1; a < argc; a++) {
        std::string arg = argv[a];
        bool use_bvh = true;
        const size_t colon = arg.rfind(":no_bvh");
        if (colon != std::string::npos && colon + 7 == arg.size()) { use_bvh = false; arg.resize(colon); }
        rt_load_opts lo;
        rt_default_load_opts(&lo);
        lo.use_bvh = use_bvh;
        lo.quiet = 1;
        lo.asset_root = std::getenv("RT_ASSETS");
        lo.image_override = 1;
        lo.width = lo.height = 16;
        lo.ray_count = lo.bounces = 1;
        rt_scene_host *h = nullptr;
        if (rt_scene_load(arg.c_str(), &lo, &h)) {
            std::printf("%s: load failed: %s\n", argv[a], rt_last_error());
            failures++;
            continue;
        }
        const rt_scene *s = rt_scene_view(h);
        float lo3[3] = {1e30f, 1e30f, 1e30f}, hi3[3] = {-1e30f, -1e30f, -1e30f};
        if (s->triangle_count) {
            const rt_bvh_node &r = s->bvh[0];
            lo3[0] = r.min_bound.x; lo3[1] = r.min_bound.y; lo3[2] = r.min_bound.z;
            hi3[0] = r.max_bound.x; hi3[1] = r.max_bound.y; hi3[2] = r.max_bound.z;
        }
        for (int i = 0; i < s->sphere_count; i++) {
            const rt_sphere &sp = s->spheres[i];
            const float c[3] = {sp.center.x, sp.center.y, sp.center.z};
            for (int k = 0; k < 3; k++) {
                lo3[k] = std::fmin(lo3[k], c[k] - sp.radius);
                hi3[k] = std::fmax(hi3[k], c[k] + sp.radius);
            }
        }
        double diag = 0;
        for (int k = 0; k < 3; k++) diag += (double)(hi3[k] - lo3[k]) * (hi3[k] - lo3[k]);
        diag = std::sqrt(diag);
        const int per = 200, n = 5 * per;
        std::vector<float> pts((size_t)n * 3), md(n);
        for (int i = 0; i < n; i++) {
            float *p = &pts[(size_t)i * 3];
            const int set = i / per;
            const rt_triangle *t = s->triangle_count ? &s->triangles[(int)(rnd() * s->triangle_count)] : nullptr;
            for (int k = 0; k < 3; k++) {
                const double mid = 0.5 * (lo3[k] + hi3[k]), half = 0.625 * (hi3[k] - lo3[k]);
                p[k] = (float)(mid + (2 * rnd() - 1) * half);
                if (set == 3) p[k] = (float)(mid + (rnd() < 0.5 ? -1000.0 : 1000.0) * diag);
            }
            if (t && (set == 1 || set == 2)) {
                double u = rnd(), v = rnd();
                if (u + v > 1) { u = 1 - u; v = 1 - v; }
                if (set == 2) { u = (i % 3) == 1; v = (i % 3) == 2; }
                p[0] = (float)(t->p1.x + u * t->p2p1.x + v * t->p3p1.x);
                p[1] = (float)(t->p1.y + u * t->p2p1.y + v * t->p3p1.y);
                p[2] = (float)(t->p1.z + u * t->p2p1.z + v * t->p3p1.z);
            }
            if (set == 4 && i % 4 != 3) p[(i / 4) % 3] = i % 4 == 0 ? NAN : (i % 4 == 1 ? INFINITY : -INFINITY);
            const float classes[6] = {0.0f, (float)(0.1 * diag), -1.0f, NAN, INFINITY, 1e19f};
            md[i] = classes[i % 6];
        }
        // every output alone, all and none, in arrays of exactly n rows
        std::vector<float> dist(n), point((size_t)n * 3), uv((size_t)n * 2);
        std::vector<int32_t> index(n);
        for (int bound = 0; bound < 2; bound++) {
            for (int mask = 0; mask < 16; mask++) {
                if (mask != 0 && mask != 15 && (mask & (mask - 1))) continue;
                std::vector<float> d1(mask & 1 ? n : 0), p1(mask & 4 ? (size_t)n * 3 : 0), u1(mask & 8 ? (size_t)n * 2 : 0);
                std::vector<int32_t> i1(mask & 2 ? n : 0);
                rt_closest_point_out o{mask & 1 ? d1.data() : nullptr, mask & 2 ? i1.data() : nullptr,
                                       mask & 4 ? p1.data() : nullptr, mask & 8 ? u1.data() : nullptr};
                if (rt_scene_closest_point(s, pts.data(), bound ? md.data() : nullptr, n, &o)) {
                    std::printf("%s: call failed: %s\n", argv[a], rt_last_error());
                    failures++;
                }
                if (mask == 15 && !bound) { dist = d1; index = i1; point = p1; uv = u1; }
            }
        }
        // the unbounded answer against the brute force by the same functions
        int nearer = 0, differ = 0, finite = 0;
        for (int i = 0; i < n; i++) {
            const rt_vec3 p = {pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]};
            if (!cp::finite3(p)) {
                if (index[i] != -1 || dist[i] != 1e30f) { std::printf("%s: point %d is not a miss\n", argv[a], i); failures++; }
                continue;
            }
            finite++;
            float best2 = INFINITY;
            int32_t best = INT32_MAX;
            for (int k = 0; k < s->sphere_count; k++) {
                rt_vec3 w;
                float len;
                const float d2 = cp::sphere_dist2(p, s->spheres[k].center, s->spheres[k].radius, w, len);
                if (cp::accepts(d2, k, best2, best)) { best2 = d2; best = k; }
            }
            for (int k = 0; k < s->triangle_count; k++) {
                const rt_triangle &t = s->triangles[k];
                const float d2 = cp::triangle(p, t.p1, t.p2p1, t.p3p1).dist2;
                if (cp::accepts(d2, s->sphere_count + k, best2, best)) { best2 = d2; best = s->sphere_count + k; }
            }
            const float bd = std::sqrt(best2);
            if (dist[i] < bd) nearer++;
            if (dist[i] != bd || index[i] != best) differ++;
        }
        std::printf("%s: %d points (%d finite), %d differ from the brute force, %d nearer than it\n", argv[a], n, finite, differ,
                    nearer);
        if (nearer || differ * 100 > finite) failures++;
        rt_scene_free(h);
    }
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
