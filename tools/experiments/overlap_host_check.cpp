// overlap_host_check.cpp — stand-alone driver of rt_scene_overlap_box (the host twin, csrc/cpu_query.hip) for sanitizer
// runs on the CPU: no GPU, no Python.
//
// For every scene file on the command line ("path" or "path:no_bvh") it loads the scene, makes 300 seeded boxes
// (centres uniform in the bounds inflated by 25 % or on triangles, half-extents log-uniform in [1e-4 D, 0.2 D] or zero,
// the whole extent, and boxes with a NaN, +inf, -inf or lo > hi), and runs the twin for K = 1, 8 and 64 with every output
// alone, all and none, into exactly sized heap arrays.  With all outputs it checks each row: count against a brute force
// over all primitives by the same functions (never more; rows with fewer are counted and printed), any == (count >= 1),
// the kept indices ascending and members by the same functions, the padding; with `any` alone (the first-member walk)
// the answer against the full walk's.
//
//   D=cuda-raytracer_amd; I="-Iinclude -I$D/host -I$D/csrc"; S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   hipcc -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt --offload-arch=gfx950 \
//     $(for f in $S; do echo -Xarch_host $f; done) $I -c $D/csrc/cpu_query.hip -o cpu_query.o
//   clang++ -std=c++17 -O1 -g -ffp-contract=off $S $I tools/experiments/overlap_host_check.cpp cpu_query.o \
//     $D/host/scene_load.cpp $D/host/image_io.cpp $D/host/bvh_records.cpp -lpthread -o overlap_host_check
//   RT_ASSETS=assets ./overlap_host_check assets/cornell.scene assets/cornell.scene:no_bvh assets/teapot.scene ...
// (clang++ = the clang hipcc drives, so that both objects carry the same sanitizer runtime.)
#include "rt_abi.h"
#include "box_overlap_math.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace ov = rtamd::ov;

namespace rtamd {
// the loader's device BVH build (csrc/bvh_build.hip) is not linked: this driver builds on the host only
int gpu_build_bvh(std::vector<rt_triangle> &, uint16_t *, std::vector<rt_bvh_node> &, int, int) { return RT_E_NODEVICE; }
}  // namespace rtamd

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

static bool member(const rt_scene *s, int idx, rt_vec3 lo, rt_vec3 hi) {
    if (idx < s->sphere_count) return ov::sphere_meets(s->spheres[idx].center, s->spheres[idx].radius, lo, hi);
    const rt_triangle &t = s->triangles[idx - s->sphere_count];
    return ov::triangle_meets(t.p1, t.p2p1, t.p3p1, lo, hi);
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
        // sets of 60: uniform, on triangles (small), thin, the extent, invalid
        const int per = 60, n = 5 * per;
        std::vector<float> boxes((size_t)n * 6);
        for (int i = 0; i < n; i++) {
            float *b = &boxes[(size_t)i * 6];
            const int set = i / per;
            const rt_triangle *t = s->triangle_count ? &s->triangles[(int)(rnd() * s->triangle_count)] : nullptr;
            double c[3], hf[3];
            for (int k = 0; k < 3; k++) {
                const double mid = 0.5 * (lo3[k] + hi3[k]), half = 0.625 * (hi3[k] - lo3[k]);
                c[k] = mid + (2 * rnd() - 1) * half;
                hf[k] = diag * std::exp(std::log(1e-4) + rnd() * (std::log(0.2) - std::log(1e-4)));
                if (set == 1) hf[k] *= 0.01;
                if (set == 3) { c[k] = mid; hf[k] = 0.5 * (hi3[k] - lo3[k]) * (1 + 0.25 * (i % 2)); }
            }
            if (t && (set == 1 || set == 2)) {
                double u = rnd(), v = rnd();
                if (u + v > 1) { u = 1 - u; v = 1 - v; }
                c[0] = t->p1.x + u * t->p2p1.x + v * t->p3p1.x;
                c[1] = t->p1.y + u * t->p2p1.y + v * t->p3p1.y;
                c[2] = t->p1.z + u * t->p2p1.z + v * t->p3p1.z;
            }
            if (set == 2) for (int k = 0; k <= i % 3; k++) hf[(i + k) % 3] = 0;
            for (int k = 0; k < 3; k++) {
                b[k] = (float)(c[k] - hf[k]);
                b[3 + k] = (float)(c[k] + hf[k]);
                if (b[k] > b[3 + k]) b[k] = b[3 + k];
            }
            if (set == 4 && i % 5 != 4) {
                const int k = (i / 5) % 3;
                if (i % 5 == 0) b[k] = NAN;
                if (i % 5 == 1) b[3 + k] = INFINITY;
                if (i % 5 == 2) b[k] = -INFINITY;
                if (i % 5 == 3) { const float x = b[k]; b[k] = std::nextafter(b[3 + k], INFINITY); b[3 + k] = x; }
            }
        }
        // every output alone, all and none, in arrays of exactly n rows
        int fewer = 0, valid = 0;
        std::vector<uint8_t> full_any(n, 2);
        for (int k : {1, 8, 64}) {
            for (int mask : {7, 1, 2, 4, 0}) {
                const size_t m = (size_t)n * k;
                std::vector<int32_t> i1(mask & 1 ? m : 0), c1(mask & 2 ? n : 0);
                std::vector<uint8_t> a1(mask & 4 ? n : 0);
                rt_overlap_out o{mask & 1 ? i1.data() : nullptr, mask & 2 ? c1.data() : nullptr, mask & 4 ? a1.data() : nullptr};
                if (rt_scene_overlap_box(s, boxes.data(), n, k, &o)) {
                    std::printf("%s: call failed: %s\n", argv[a], rt_last_error());
                    failures++;
                    continue;
                }
                if (mask == 4) {                            // the first-member walk against the full walk
                    for (int i = 0; i < n; i++)
                        if (a1[i] != full_any[i]) { std::printf("%s: box %d any-only %d != %d\n", argv[a], i, a1[i], full_any[i]); failures++; }
                    continue;
                }
                if (mask != 7) continue;
                for (int i = 0; i < n; i++) {
                    const float *b = &boxes[(size_t)i * 6];
                    const rt_vec3 qlo = {b[0], b[1], b[2]}, qhi = {b[3], b[4], b[5]};
                    int brute = 0;
                    if (ov::valid_box(qlo, qhi)) {
                        for (int j = 0; j < s->sphere_count + s->triangle_count; j++) brute += member(s, j, qlo, qhi);
                        if (k == 1) valid++;
                    }
                    full_any[i] = a1[i];
                    if (c1[i] > brute) { std::printf("%s: box %d counts %d > brute %d\n", argv[a], i, c1[i], brute); failures++; }
                    if (c1[i] < brute && k == 1) fewer++;
                    if (a1[i] != (c1[i] >= 1 ? 1 : 0)) { std::printf("%s: box %d any %d count %d\n", argv[a], i, a1[i], c1[i]); failures++; }
                    const int kept = c1[i] < k ? c1[i] : k;
                    for (int j = 0; j < k; j++) {
                        const size_t e = (size_t)i * k + j;
                        bool ok;
                        if (j >= kept) ok = i1[e] == -1;
                        else ok = i1[e] >= 0 && (j == 0 || i1[e - 1] < i1[e]) && member(s, i1[e], qlo, qhi);
                        if (!ok) { std::printf("%s: k %d box %d entry %d is wrong\n", argv[a], k, i, j); failures++; }
                    }
                }
            }
        }
        std::printf("%s: %d boxes (%d valid): %d rows count fewer than the brute force\n", argv[a], n, valid, fewer);
        if (fewer * 100 > valid) failures++;          // 1 % of the valid rows
        rt_scene_free(h);
    }
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
