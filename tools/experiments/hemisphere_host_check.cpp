// hemisphere_host_check.cpp — stand-alone driver of rt_scene_hemisphere and rt_hemisphere_rays (the host twin and the
// sample generator, csrc/cpu_query.hip) for sanitizer runs on the CPU: no GPU, no Python.
//
// For every scene file on the command line ("path" or "path:no_bvh") it loads the scene, makes seeded frames (triangle
// points with the triangle's normal, points inside the bounds with random normals, and zero, NaN, infinite and
// non-unit normals), and runs the twin in both modes for S in {1, 3, 64, 65} (and 4096 on the first 4 frames) with
// every filter member absent and present, with primitive masks and without, into exactly sized heap arrays -- both
// outputs, each alone -- and the rays of the same calls into an exactly sized n * S * 6 array.  It checks relation R1
// on every row (open_count == S - the filtered any-hit of the call's own rays under the row's filter), openness ==
// (float)count / (float)S, a split batch with point_offset against the whole, and the stats' sums.
//
//   D=cuda-raytracer_amd; I="-Iinclude -I$D/host -I$D/csrc"; S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   hipcc -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt --offload-arch=gfx950 \
//     $(for f in $S; do echo -Xarch_host $f; done) $I -c $D/csrc/cpu_query.hip -o cpu_query.o
//   clang++ -std=c++17 -O1 -g -ffp-contract=off $S $I tools/experiments/hemisphere_host_check.cpp cpu_query.o \
//     $D/host/scene_load.cpp $D/host/image_io.cpp $D/host/bvh_records.cpp -lpthread -o hemisphere_host_check
//   RT_ASSETS=assets ./hemisphere_host_check assets/cornell.scene assets/spheres.scene assets/teapot.scene
// (clang++ = the clang hipcc drives, so that both objects carry the same sanitizer runtime.)
#include "rt_abi.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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
        const int P = s->sphere_count + s->triangle_count;
        float lo3[3] = {-1, -1, -1}, hi3[3] = {1, 1, 1};
        if (s->triangle_count) {
            const rt_bvh_node &r = s->bvh[0];
            lo3[0] = r.min_bound.x; lo3[1] = r.min_bound.y; lo3[2] = r.min_bound.z;
            hi3[0] = r.max_bound.x; hi3[1] = r.max_bound.y; hi3[2] = r.max_bound.z;
        }
        const int n = 48;
        std::vector<float> frames((size_t)n * 6), tmin(n), tmax(n);
        std::vector<int32_t> skip(n);
        std::vector<uint32_t> rmask(n), masks(P);
        for (int p = 0; p < P; p++) masks[p] = 1u << (s->material_indices[p] % 32);
        const float diag = std::sqrt((hi3[0] - lo3[0]) * (hi3[0] - lo3[0]) + (hi3[1] - lo3[1]) * (hi3[1] - lo3[1]) +
                                     (hi3[2] - lo3[2]) * (hi3[2] - lo3[2]));
        for (int i = 0; i < n; i++) {
            float *f = &frames[(size_t)i * 6];
            skip[i] = -1;
            if (i % 2 == 0 && s->triangle_count) {              // a triangle point, the triangle's normal, skip = itself
                const int j = (int)(rnd() * s->triangle_count);
                const rt_triangle &t = s->triangles[j];
                double u = rnd(), v = rnd();
                if (u + v > 1) { u = 1 - u; v = 1 - v; }
                f[0] = (float)(t.p1.x + u * t.p2p1.x + v * t.p3p1.x); f[1] = (float)(t.p1.y + u * t.p2p1.y + v * t.p3p1.y);
                f[2] = (float)(t.p1.z + u * t.p2p1.z + v * t.p3p1.z);
                f[3] = t.normal.x; f[4] = t.normal.y; f[5] = t.normal.z;
                skip[i] = s->sphere_count + j;
            } else {
                for (int k = 0; k < 3; k++) {
                    f[k] = (float)(lo3[k] + rnd() * (hi3[k] - lo3[k]));
                    f[3 + k] = (float)(2 * rnd() - 1);
                }
            }
            if (i % 12 == 5) f[3] = f[4] = f[5] = 0;
            if (i % 12 == 7) f[3 + i % 3] = NAN;
            if (i % 12 == 9) f[3 + i % 3] = INFINITY;
            if (i % 12 == 11) for (int k = 3; k < 6; k++) f[k] *= 1e4f;
            tmin[i] = i % 5 == 0 ? NAN : (float)(rnd() * 0.01 * diag);
            tmax[i] = i % 7 == 0 ? INFINITY : (i % 7 == 1 ? -1.0f : (float)(rnd() * diag));
            rmask[i] = i % 4 == 0 ? 0xFFFFFFFFu : (uint32_t)(rnd() * 4294967296.0);
        }
        long rows = 0, samples_walked = 0, open_total = 0;
        const int sample_counts[5] = {1, 3, 64, 65, RT_HEMISPHERE_MAX_SAMPLES};
        for (int mode = 0; mode < 2; mode++)
            for (int sc = 0; sc < 5; sc++)
                for (int variant = 0; variant < 6; variant++) {
                    const int S = sample_counts[sc];
                    const int m = S == RT_HEMISPHERE_MAX_SAMPLES ? 4 : n;
                    // variant: 0 no filter, 1 skip, 2 tmax, 3 tmin + mask with primitive masks, 4 all, 5 all with masks
                    rt_ray_filter f{(variant == 3 || variant >= 4) ? tmin.data() : nullptr,
                                    (variant == 2 || variant >= 4) ? tmax.data() : nullptr,
                                    (variant == 1 || variant >= 4) ? skip.data() : nullptr,
                                    (variant == 3 || variant >= 4) ? rmask.data() : nullptr};
                    const uint32_t *pm = (variant == 3 || variant == 5) ? masks.data() : nullptr;
                    const rt_hemisphere_params hp{S, mode, 77u + (uint32_t)variant, 0xFFFFFFF0u};    // the offset wraps inside the batch
                    std::vector<int32_t> cnt(m), cnt_alone(m), cnt_split(m);
                    std::vector<float> opn(m), opn_alone(m);
                    std::vector<float> rays((size_t)m * S * 6);
                    rt_stats st;
                    const rt_hemisphere_out both{cnt.data(), opn.data()}, c_only{cnt_alone.data(), nullptr}, o_only{nullptr, opn_alone.data()};
                    const rt_ray_filter *fp = variant ? &f : nullptr;
                    int rc = rt_scene_hemisphere(s, pm, frames.data(), fp, m, &hp, &both, &st);
                    rc = rc || rt_scene_hemisphere(s, pm, frames.data(), fp, m, &hp, &c_only, nullptr);
                    rc = rc || rt_scene_hemisphere(s, pm, frames.data(), fp, m, &hp, &o_only, nullptr);
                    rc = rc || rt_hemisphere_rays(frames.data(), m, &hp, rays.data());
                    // the batch split at `cut`, the second part called with its own offset
                    const int cut = m / 3 + 1;
                    rt_hemisphere_params hp2 = hp;
                    hp2.point_offset = hp.point_offset + (uint32_t)cut;
                    const rt_ray_filter f2{f.tmin ? f.tmin + cut : nullptr, f.tmax ? f.tmax + cut : nullptr, f.skip ? f.skip + cut : nullptr,
                                           f.mask ? f.mask + cut : nullptr};
                    const rt_hemisphere_out s1{cnt_split.data(), nullptr}, s2{cnt_split.data() + cut, nullptr};
                    rc = rc || rt_scene_hemisphere(s, pm, frames.data(), fp, cut, &hp, &s1, nullptr);
                    if (m > cut)
                        rc = rc || rt_scene_hemisphere(s, pm, frames.data() + (size_t)cut * 6, variant ? &f2 : nullptr, m - cut, &hp2, &s2, nullptr);
                    if (rc) {
                        std::printf("%s: call failed: %s\n", argv[a], rt_last_error());
                        failures++;
                        continue;
                    }
                    uint64_t occ_sum = 0;
                    for (int i = 0; i < m; i++) {
                        // R1: the filtered any-hit of row i's own rays, the row's filter on every one of them
                        std::vector<float> tn(S, f.tmin ? tmin[i] : 0), tx(S, f.tmax ? tmax[i] : 0);
                        std::vector<int32_t> sk(S, f.skip ? skip[i] : 0);
                        std::vector<uint32_t> rm(S, f.mask ? rmask[i] : 0);
                        const rt_ray_filter fr{f.tmin ? tn.data() : nullptr, f.tmax ? tx.data() : nullptr, f.skip ? sk.data() : nullptr,
                                               f.mask ? rm.data() : nullptr};
                        std::vector<uint8_t> occ(S);
                        if (rt_scene_occluded_filtered(s, pm, rays.data() + (size_t)i * S * 6, &fr, S, occ.data(), nullptr)) {
                            std::printf("%s: call failed: %s\n", argv[a], rt_last_error());
                            failures++;
                            continue;
                        }
                        int open = 0;
                        for (int k = 0; k < S; k++) open += occ[k] ? 0 : 1;
                        occ_sum += (uint64_t)(S - open);
                        rows++;
                        samples_walked += S;
                        open_total += open;
                        const float want = (float)open / (float)S;
                        const bool ok = cnt[i] == open && cnt_alone[i] == open && cnt_split[i] == open &&
                                        std::memcmp(&opn[i], &want, 4) == 0 && std::memcmp(&opn_alone[i], &want, 4) == 0;
                        if (!ok) {
                            std::printf("%s: mode %d S %d variant %d row %d is wrong (count %d alone %d split %d want %d)\n", argv[a], mode, S,
                                        variant, i, cnt[i], cnt_alone[i], cnt_split[i], open);
                            failures++;
                        }
                    }
                    if (st.live_segments != (uint64_t)m * S || st.hits != occ_sum || st.misses != (uint64_t)m * S - occ_sum) {
                        std::printf("%s: mode %d S %d variant %d stats are wrong\n", argv[a], mode, S, variant);
                        failures++;
                    }
                }
        std::printf("%s: %d frames, %ld rows, %ld sample rays, %ld open\n", argv[a], n, rows, samples_walked, open_total);
        rt_scene_free(h);
    }
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
