// ray_filter_host_check.cpp — stand-alone driver of rt_scene_closest_filtered and rt_scene_occluded_filtered (the host
// twins, csrc/cpu_query.hip) for sanitizer runs on the CPU: no GPU, no Python.
//
// For every scene file on the command line ("path" or "path:no_bvh") it loads the scene, makes seeded rays (from the
// bounds' inflated box toward a point inside it, from triangle points along the normal, with zero and non-finite
// components), takes their unfiltered closest hits (t_c, i_c) and runs both twins over the filter classes of the
// tests -- tmin: none, 0, the floats below, at and above t_c, 2 t_c, NaN, +inf, negative; tmax: none, 1e30, t_c, the
// floats below and above it, 0.5 t_c, 0, -1, NaN, +inf; skip: none, -1, i_c, the next ray's i_c, out of range; ray
// masks: none, all ones, 0, all but the bit of i_c's material, only that bit, random, with primitive masks (bit
// material % 32) and without; and seeded combinations of all four -- into exactly sized heap arrays, with t alone, index
// alone, both, neither, and the stats.  It checks relation R1 on every row (index >= 0 <=> occluded), that a hit's t
// lies in [lo, B) unless it is NaN, that a hit is eligible, and the stats' sums.
//
//   D=cuda-raytracer_amd; I="-Iinclude -I$D/host -I$D/csrc"; S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   hipcc -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt --offload-arch=gfx950 \
//     $(for f in $S; do echo -Xarch_host $f; done) $I -c $D/csrc/cpu_query.hip -o cpu_query.o
//   clang++ -std=c++17 -O1 -g -ffp-contract=off $S $I tools/experiments/ray_filter_host_check.cpp cpu_query.o \
//     $D/host/scene_load.cpp $D/host/image_io.cpp $D/host/bvh_records.cpp -lpthread -o ray_filter_host_check
//   RT_ASSETS=assets ./ray_filter_host_check assets/cornell.scene assets/cornell.scene:no_bvh assets/teapot.scene ...
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

static const float kEps = 0x1.47ae16p-8f;

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
        const int S = s->sphere_count, P = S + s->triangle_count;
        float lo3[3] = {-1, -1, -1}, hi3[3] = {1, 1, 1};
        if (s->triangle_count) {
            const rt_bvh_node &r = s->bvh[0];
            lo3[0] = r.min_bound.x; lo3[1] = r.min_bound.y; lo3[2] = r.min_bound.z;
            hi3[0] = r.max_bound.x; hi3[1] = r.max_bound.y; hi3[2] = r.max_bound.z;
        }
        const int per = 60, n = 5 * per;
        std::vector<float> rays((size_t)n * 6);
        for (int i = 0; i < n; i++) {
            float *r = &rays[(size_t)i * 6];
            const int set = i / per;
            double o[3], to[3];
            for (int k = 0; k < 3; k++) {
                const double mid = 0.5 * (lo3[k] + hi3[k]), half = 0.5 * (hi3[k] - lo3[k]);
                o[k] = mid + (2 * rnd() - 1) * half * 1.5;
                to[k] = mid + (2 * rnd() - 1) * half * 0.8;
            }
            if (set == 1 && s->triangle_count) {                // from a triangle point, along its normal
                const rt_triangle &t = s->triangles[(int)(rnd() * s->triangle_count)];
                double u = rnd(), v = rnd();
                if (u + v > 1) { u = 1 - u; v = 1 - v; }
                o[0] = t.p1.x + u * t.p2p1.x + v * t.p3p1.x; o[1] = t.p1.y + u * t.p2p1.y + v * t.p3p1.y;
                o[2] = t.p1.z + u * t.p2p1.z + v * t.p3p1.z;
                to[0] = o[0] + t.normal.x; to[1] = o[1] + t.normal.y; to[2] = o[2] + t.normal.z;
            }
            double d[3] = {to[0] - o[0], to[1] - o[1], to[2] - o[2]};
            if (set == 2) d[i % 3] = 0;                         // a zero component: an infinite 1/d
            if (set == 3) { d[i % 3] = 0; d[(i + 1) % 3] = 0; }
            const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int k = 0; k < 3; k++) {
                r[k] = (float)o[k];
                r[3 + k] = (float)(len > 0 ? d[k] / len : (k == 0));
            }
            if (set == 4 && i % 4 != 3) r[(i / 4) % 6] = i % 4 == 0 ? NAN : (i % 4 == 1 ? INFINITY : -INFINITY);
        }
        std::vector<float> tc(n);
        std::vector<int32_t> ic(n);
        if (rt_scene_closest_filtered(s, nullptr, rays.data(), nullptr, n, tc.data(), ic.data(), nullptr)) {
            std::printf("%s: call failed: %s\n", argv[a], rt_last_error());
            failures++;
        }
        std::vector<uint32_t> masks(P);
        for (int p = 0; p < P; p++) masks[p] = 1u << (s->material_indices[p] % 32);
        auto bit_of = [&](int i) { return ic[i] >= 0 ? masks[ic[i]] : 1u; };
        long rows = 0, hits = 0, changed = 0;
        // class index 0 of every member = the member is not given; `combo` draws all four at random
        const int NT = 9, NX = 11, NS = 5, NM = 6;
        for (int run = 0; run < NT + NX + NS + 2 * NM + 8; run++) {
            std::vector<float> tmin(n), tmax(n);
            std::vector<int32_t> skip(n);
            std::vector<uint32_t> rmask(n);
            int ct = 0, cx = 0, cs = 0, cm = 0;
            bool prim = false, combo = false;
            if (run < NT) ct = run;
            else if (run < NT + NX) cx = run - NT;
            else if (run < NT + NX + NS) cs = run - NT - NX;
            else if (run < NT + NX + NS + 2 * NM) { cm = (run - NT - NX - NS) % NM; prim = run - NT - NX - NS >= NM; }
            else { combo = true; prim = run % 2; }
            for (int i = 0; i < n; i++) {
                const int kt = combo ? 1 + (int)(rnd() * (NT - 1)) : ct, kx = combo ? 1 + (int)(rnd() * (NX - 1)) : cx;
                const int ks = combo ? 1 + (int)(rnd() * (NS - 1)) : cs, km = combo ? 1 + (int)(rnd() * (NM - 1)) : cm;
                const float tmins[9] = {0, 0, std::nextafterf(tc[i], -INFINITY), tc[i], std::nextafterf(tc[i], INFINITY),
                                        2 * tc[i], NAN, INFINITY, -1};
                const float tmaxs[11] = {0, 1e30f, tc[i], std::nextafterf(tc[i], -INFINITY), std::nextafterf(tc[i], INFINITY),
                                         0.5f * tc[i], 0, -1, NAN, INFINITY, (float)(rnd() * 2 * tc[i])};
                const int32_t skips[5] = {0, -1, ic[i], ic[(i + 1) % n], P + 5};
                const uint32_t rms[6] = {0, 0xFFFFFFFFu, 0, ~bit_of(i), bit_of(i), (uint32_t)(rnd() * 4294967296.0)};
                tmin[i] = tmins[kt]; tmax[i] = tmaxs[kx]; skip[i] = skips[ks]; rmask[i] = rms[km];
            }
            rt_ray_filter f{(combo || ct) ? tmin.data() : nullptr, (combo || cx) ? tmax.data() : nullptr,
                            (combo || cs) ? skip.data() : nullptr, (combo || cm) ? rmask.data() : nullptr};
            const uint32_t *pm = prim ? masks.data() : nullptr;
            for (int outs = 0; outs < 4; outs++) {              // t alone, index alone, both, neither
                std::vector<float> t(outs == 0 || outs == 2 ? n : 0);
                std::vector<int32_t> idx(outs == 1 || outs == 2 ? n : 0);
                std::vector<uint8_t> occ(n);
                rt_stats st, sa;
                if (rt_scene_closest_filtered(s, pm, rays.data(), &f, n, t.empty() ? nullptr : t.data(),
                                              idx.empty() ? nullptr : idx.data(), &st) ||
                    rt_scene_occluded_filtered(s, pm, rays.data(), &f, n, occ.data(), outs == 3 ? nullptr : &sa)) {
                    std::printf("%s: call failed: %s\n", argv[a], rt_last_error());
                    failures++;
                    continue;
                }
                if (outs != 2) continue;
                uint64_t nh = 0, no = 0;
                for (int i = 0; i < n; i++) {
                    rows++;
                    const float lo_i = f.tmin && tmin[i] > kEps ? tmin[i] : kEps;
                    const float B = f.tmax && tmax[i] <= 1e30f ? tmax[i] : 1e30f;
                    const bool hit = idx[i] >= 0;
                    nh += hit; no += occ[i];
                    hits += hit;
                    changed += idx[i] != ic[i];
                    bool ok = hit == (occ[i] != 0) && idx[i] < P;                                  // R1
                    if (hit) {
                        ok = ok && (t[i] != t[i] || (!(t[i] < lo_i) && t[i] < B));
                        ok = ok && !(f.skip && skip[i] == idx[i]);
                        ok = ok && ((pm ? pm[idx[i]] : 0xFFFFFFFFu) & (f.mask ? rmask[i] : 0xFFFFFFFFu)) != 0;
                    } else {
                        ok = ok && t[i] == 1e30f && idx[i] == -1;
                    }
                    if (!ok) { std::printf("%s: run %d ray %d is wrong (t %g index %d occluded %d)\n", argv[a], run, i, t[i], idx[i], occ[i]); failures++; }
                }
                if (st.hits != nh || st.misses != (uint64_t)n - nh || st.live_segments != (uint64_t)n || sa.hits != no ||
                    st.sphere_tests != (uint64_t)n * S) {
                    std::printf("%s: run %d stats are wrong\n", argv[a], run);
                    failures++;
                }
            }
        }
        std::printf("%s: %d rays, %ld filtered rows, %ld hits, %ld rows whose index differs from the unfiltered one\n", argv[a], n,
                    rows, hits, changed);
        rt_scene_free(h);
    }
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
