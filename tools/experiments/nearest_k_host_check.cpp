// nearest_k_host_check.cpp — stand-alone driver of rt_scene_nearest_k (the host twin, csrc/cpu_query.hip) for sanitizer
// runs on the CPU: no GPU, no Python.
//
// For every scene file on the command line ("path" or "path:no_bvh") it loads the scene, makes seeded points
// (closest_point_host_check's: uniform in the bounds inflated by 25 %, on triangles, at vertices, 1000 diagonals away,
// non-finite), and runs the twin for K = 1, 8 and 64 without max_dist and with a max_dist that cycles through 0, a
// finite radius, negative, NaN, +inf and 1e19, with every output alone, all and none, into exactly sized heap arrays.
// With all outputs it checks each row: count against a brute force over all primitives by the same functions (never
// more; rows with fewer are counted and printed), the kept entries ascending by the key, the padding.
//
//   D=cuda-raytracer_amd; I="-Iinclude -I$D/host -I$D/csrc"; S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   hipcc -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt --offload-arch=gfx950 \
//     $(for f in $S; do echo -Xarch_host $f; done) $I -c $D/csrc/cpu_query.hip -o cpu_query.o
//   clang++ -std=c++17 -O1 -g -ffp-contract=off $S $I tools/experiments/nearest_k_host_check.cpp cpu_query.o \
//     $D/host/scene_load.cpp $D/host/image_io.cpp $D/host/bvh_records.cpp -lpthread -o nearest_k_host_check
//   RT_ASSETS=assets ./nearest_k_host_check assets/cornell.scene assets/cornell.scene:no_bvh assets/teapot.scene ...
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
        const int per = 60, n = 5 * per;
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
        // every output alone, all and none, in arrays of exactly n rows (n x k, n x k x 3)
        int fewer = 0, finite = 0;
        for (int k : {1, 8, 64}) {
            for (int bound = 0; bound < 2; bound++) {
                for (int mask = 0; mask < 16; mask++) {
                    if (mask != 0 && mask != 15 && (mask & (mask - 1))) continue;
                    const size_t m = (size_t)n * k;
                    std::vector<float> d1(mask & 1 ? m : 0), p1(mask & 4 ? m * 3 : 0);
                    std::vector<int32_t> i1(mask & 2 ? m : 0), c1(mask & 8 ? n : 0);
                    rt_nearest_k_out o{mask & 1 ? d1.data() : nullptr, mask & 2 ? i1.data() : nullptr,
                                       mask & 4 ? p1.data() : nullptr, mask & 8 ? c1.data() : nullptr};
                    if (rt_scene_nearest_k(s, pts.data(), bound ? md.data() : nullptr, n, k, &o)) {
                        std::printf("%s: call failed: %s\n", argv[a], rt_last_error());
                        failures++;
                        continue;
                    }
                    if (mask != 15) continue;
                    for (int i = 0; i < n; i++) {
                        const rt_vec3 p = {pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]};
                        const float b2 = bound ? cp::bound2(md[i]) : INFINITY;
                        int brute = 0;
                        if (cp::finite3(p)) {
                            for (int j = 0; j < s->sphere_count; j++) {
                                rt_vec3 w;
                                float len;
                                brute += cp::within(cp::sphere_dist2(p, s->spheres[j].center, s->spheres[j].radius, w, len), b2);
                            }
                            for (int j = 0; j < s->triangle_count; j++) {
                                const rt_triangle &t = s->triangles[j];
                                brute += cp::within(cp::triangle(p, t.p1, t.p2p1, t.p3p1).dist2, b2);
                            }
                            if (k == 1 && !bound) finite++;
                        }
                        if (c1[i] > brute) { std::printf("%s: point %d counts %d > brute %d\n", argv[a], i, c1[i], brute); failures++; }
                        if (c1[i] < brute && k == 1) fewer++;
                        const int kept = c1[i] < k ? c1[i] : k;
                        for (int j = 0; j < k; j++) {
                            const size_t e = (size_t)i * k + j;
                            bool ok;
                            if (j >= kept) {
                                ok = d1[e] == 1e30f && i1[e] == -1 && p1[e * 3] == 0 && p1[e * 3 + 1] == 0 && p1[e * 3 + 2] == 0;
                            } else {
                                ok = i1[e] >= 0 && d1[e] * d1[e] <= b2 * 1.000001f &&
                                     (j == 0 || d1[e - 1] < d1[e] || (d1[e - 1] == d1[e] && i1[e - 1] != i1[e]));
                            }
                            if (!ok) { std::printf("%s: k %d point %d entry %d is wrong\n", argv[a], k, i, j); failures++; }
                        }
                    }
                }
            }
        }
        std::printf("%s: %d points (%d finite), both bounds: %d rows count fewer than the brute force\n", argv[a], n, finite, fewer);
        if (fewer * 100 > 2 * finite) failures++;     // 1 % of the 2 * finite rows
        rt_scene_free(h);
    }
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
