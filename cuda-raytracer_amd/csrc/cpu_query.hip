// cpu_query.hip — rt_scene_multi_hit, the host twin of rt_query_multi_hit, host-only.
//
// The reference traversal (scene.cu:338-372, :134-241) with `closest` held at the ray's bound B and never
// updated, run to the end: every accepted primitive is a hit.  The per-ray arithmetic is the shared
// __host__ __device__ code in rt_device.h (ray_sphere, ray_triangle, slab), so the accepted set and every t
// are the device kernel's bit for bit; the node array is the scene's own (rt_scene.bvh), walked with a plain
// stack -- the set does not depend on the order.  The hits are then sorted by the key (t', index) of rt_abi.h.
//
// Also rt_scene_closest_point, the host twin of rt_query_closest_point: the pinned walk with the
// shrinking bound, every value from closest_point_math.h, which the device kernel compiles too.
// And rt_scene_nearest_k, the host twin of rt_query_nearest_k: the same arithmetic with the bound held,
// every member of the fixed set collected and sorted by the key (dist2 bits, index).
// And rt_scene_closest_filtered / rt_scene_occluded_filtered, the host twins of the filtered ray queries:
// the pinned near-first walk with the shrinking bound and the any-hit walk with the bound held, the filter's
// arithmetic from ray_filter_math.h.
// And rt_scene_hemisphere, the host twin of rt_query_hemisphere, and rt_hemisphere_rays: the sample
// generator of hemisphere_math.h over the filtered any-hit twin.
// And rt_scene_overlap_box, the host twin of rt_query_overlap_box: the set of primitives that meet a box, by
// box_overlap_math.h, which box_overlap_kernel compiles too.
#include "rt_abi.h"
#include "rt_device.h"
#include "closest_point_math.h"
#include "ray_filter_math.h"
#include "hemisphere_math.h"
#include "box_overlap_math.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace rtamd {
int fail(int code, const std::string &msg);
}

using namespace rtd;

namespace {

struct Hit { uint32_t key; int32_t index; float t; };

V3 vec(const rt_vec3 &v) { return v3(v.x, v.y, v.z); }

// t' of rt_abi.h: t's bits, every NaN as one pattern
uint32_t key_of(float t) {
    uint32_t b;
    std::memcpy(&b, &t, 4);
    return t != t ? 0x7FC00000u : b;
}

void all_hits(const rt_scene &s, V3 o, V3 d, float B, std::vector<Hit> &hits, std::vector<int32_t> &stack) {
    hits.clear();
    for (int i = 0; i < s.sphere_count; i++) {
        float t;
        if (ray_sphere(o, d, vec(s.spheres[i].center), s.spheres[i].radius, B, t)) hits.push_back({key_of(t), i, t});
    }
    if (0.0f >= B || s.bvh_node_count <= 0) return;
    const float ix = 1 / d.x, iy = 1 / d.y, iz = 1 / d.z;
    stack.clear();
    stack.push_back(0);
    while (!stack.empty()) {
        const rt_bvh_node &nd = s.bvh[stack.back()];
        stack.pop_back();
        if (nd.child2 <= nd.child1) {
            for (int i = nd.child2; i < nd.child1; i++) {
                const rt_triangle &tr = s.triangles[i];
                float t;
                if (ray_triangle(o, d, vec(tr.p1), vec(tr.p2p1), vec(tr.p3p1), B, t))
                    hits.push_back({key_of(t), s.sphere_count + i, t});
            }
            continue;
        }
        for (const int32_t c : {nd.child1, nd.child2}) {
            const rt_bvh_node &b = s.bvh[c];
            float entry;
            if (slab(b.min_bound.x, b.min_bound.y, b.min_bound.z, b.max_bound.x, b.max_bound.y, b.max_bound.z, o, ix, iy,
                     iz, B, entry) &&
                !(entry >= B))
                stack.push_back(c);
        }
    }
}

// rt_scene_closest_point's walk (rt_abi.h) for one finite point: closest_point_kernel's, over the
// scene's own node array.  The stack holds (node, box2) pairs; the walk pushes at most one per level.
struct Entry { int32_t node; float box2; };

void nearest(const rt_scene &s, rt_vec3 p, float &best2, int32_t &best, std::vector<Entry> &stack) {
    namespace cp = rtamd::cp;
    for (int i = 0; i < s.sphere_count; i++) {
        rt_vec3 w;
        float len;
        const float d2 = cp::sphere_dist2(p, s.spheres[i].center, s.spheres[i].radius, w, len);
        if (cp::accepts(d2, i, best2, best)) { best2 = d2; best = i; }
    }
    if (0.0f > best2) return;
    stack.clear();
    int32_t n = 0;
    while (true) {
        const rt_bvh_node &nd = s.bvh[n];
        bool descend = false;
        if (nd.child2 <= nd.child1) {
            for (int j = nd.child2; j < nd.child1; j++) {
                const rt_triangle &tr = s.triangles[j];
                const float d2 = cp::triangle(p, tr.p1, tr.p2p1, tr.p3p1).dist2;
                if (cp::accepts(d2, s.sphere_count + j, best2, best)) { best2 = d2; best = s.sphere_count + j; }
            }
        } else {
            const rt_bvh_node &c1 = s.bvh[nd.child1], &c2 = s.bvh[nd.child2];
            const float a = cp::box2(p, c1.min_bound, c1.max_bound), b = cp::box2(p, c2.min_bound, c2.max_bound);
            const bool e1 = !(a > best2), e2 = !(b > best2);
            if (e1 || e2) {
                const bool second = e2 && (!e1 || b < a);
                if (e1 && e2) stack.push_back(second ? Entry{nd.child1, a} : Entry{nd.child2, b});
                n = second ? nd.child2 : nd.child1;
                descend = true;
            }
        }
        if (descend) continue;
        bool found = false;
        while (!stack.empty() && !found) {
            const Entry e = stack.back();
            stack.pop_back();
            if (!(e.box2 > best2)) { n = e.node; found = true; }
        }
        if (!found) return;
    }
}

// rt_scene_nearest_k's set H (rt_abi.h) for one finite point: nearest_k_kernel's walk with the bound b2
// held, over the scene's own node array.  The stack holds nodes only -- every pushed child has passed the test it
// would meet at the pop -- and the set does not depend on the order.
struct Member { uint32_t key; int32_t index; float dist2; };

void members(const rt_scene &s, rt_vec3 p, float b2, std::vector<Member> &found, std::vector<int32_t> &stack) {
    namespace cp = rtamd::cp;
    found.clear();
    for (int i = 0; i < s.sphere_count; i++) {
        rt_vec3 w;
        float len;
        const float d2 = cp::sphere_dist2(p, s.spheres[i].center, s.spheres[i].radius, w, len);
        if (cp::within(d2, b2)) found.push_back({cp::key_bits(d2), i, d2});
    }
    if (0.0f > b2) return;
    stack.clear();
    stack.push_back(0);
    while (!stack.empty()) {
        const rt_bvh_node &nd = s.bvh[stack.back()];
        stack.pop_back();
        if (nd.child2 <= nd.child1) {
            for (int j = nd.child2; j < nd.child1; j++) {
                const rt_triangle &tr = s.triangles[j];
                const float d2 = cp::triangle(p, tr.p1, tr.p2p1, tr.p3p1).dist2;
                if (cp::within(d2, b2)) found.push_back({cp::key_bits(d2), s.sphere_count + j, d2});
            }
            continue;
        }
        const rt_bvh_node &c1 = s.bvh[nd.child1], &c2 = s.bvh[nd.child2];
        const float a = cp::box2(p, c1.min_bound, c1.max_bound), b = cp::box2(p, c2.min_bound, c2.max_bound);
        const bool e1 = !(a > b2), e2 = !(b > b2);
        const bool second = e2 && (!e1 || b < a);      // the nearer child first, a tie to child1: the kernel's order
        if (e1 && e2) stack.push_back(second ? nd.child1 : nd.child2);
        if (e1 || e2) stack.push_back(second ? nd.child2 : nd.child1);
    }
}

// rt_scene_overlap_box's set H (rt_abi.h) for one valid box: box_overlap_kernel's walk in its pinned order
// over the scene's own node array.  first_only: the any-only walk, which stops at the first member.
void overlapping(const rt_scene &s, rt_vec3 lo, rt_vec3 hi, bool first_only, std::vector<int32_t> &found,
                 std::vector<int32_t> &stack) {
    namespace ov = rtamd::ov;
    found.clear();
    for (int i = 0; i < s.sphere_count; i++) {
        if (!ov::sphere_meets(s.spheres[i].center, s.spheres[i].radius, lo, hi)) continue;
        found.push_back(i);
        if (first_only) return;
    }
    stack.clear();
    stack.push_back(0);
    while (!stack.empty()) {
        const rt_bvh_node &nd = s.bvh[stack.back()];
        stack.pop_back();
        if (nd.child2 <= nd.child1) {
            for (int j = nd.child2; j < nd.child1; j++) {
                const rt_triangle &tr = s.triangles[j];
                if (!ov::triangle_meets(tr.p1, tr.p2p1, tr.p3p1, lo, hi)) continue;
                found.push_back(s.sphere_count + j);
                if (first_only) return;
            }
            continue;
        }
        const rt_bvh_node &c1 = s.bvh[nd.child1], &c2 = s.bvh[nd.child2];
        if (ov::boxes_meet(c2.min_bound, c2.max_bound, lo, hi)) stack.push_back(nd.child2);
        if (ov::boxes_meet(c1.min_bound, c1.max_bound, lo, hi)) stack.push_back(nd.child1);   // child1 first
    }
}

// The filtered ray queries' walks (rt_abi.h) for one ray, over the scene's own node array: the per-ray
// arithmetic is rt_device.h's and ray_filter_math.h's, which filtered_closest_kernel and filtered_anyhit_kernel
// compile too.  Work counts the walk's Pn, Iv, Tt and sphere tests.
struct Filter { float lo, B; int32_t skip; uint32_t rm; const uint32_t *masks; };
struct Work { uint64_t pn = 0, iv = 0, tt = 0, st = 0; };
struct FarEntry { int32_t node; float entry; };

Filter filter_of(const rt_ray_filter *f, const uint32_t *masks, int32_t i) {
    namespace rf = rtamd::rf;
    Filter r{kEps, 1e30f, -1, rf::kAllBits, masks};
    if (!f) return r;
    if (f->tmin) r.lo = rf::lower(f->tmin[i]);
    if (f->tmax) r.B = rf::upper(f->tmax[i]);
    if (f->skip) r.skip = f->skip[i];
    if (f->mask) r.rm = f->mask[i];
    return r;
}

bool eligible(const Filter &f, int32_t p) { return rtamd::rf::eligible(p, f.skip, f.masks ? f.masks[p] : rtamd::rf::kAllBits, f.rm); }

bool accept_sphere(const rt_scene &s, const Filter &f, V3 o, V3 d, int k, float bound, float &t) {
    return rtamd::rf::ray_sphere_lo(o, d, vec(s.spheres[k].center), s.spheres[k].radius, f.lo, bound, t) && eligible(f, k);
}

bool accept_triangle(const rt_scene &s, const Filter &f, V3 o, V3 d, int j, float bound, float &t) {
    const rt_triangle &tr = s.triangles[j];
    return ray_triangle(o, d, vec(tr.p1), vec(tr.p2p1), vec(tr.p3p1), bound, t) && !(t < f.lo) && eligible(f, s.sphere_count + j);
}

bool child_entered(const rt_scene &s, int32_t c, V3 o, float ix, float iy, float iz, float bound, float &entry) {
    const rt_bvh_node &b = s.bvh[c];
    return slab(b.min_bound.x, b.min_bound.y, b.min_bound.z, b.max_bound.x, b.max_bound.y, b.max_bound.z, o, ix, iy, iz,
                bound, entry) &&
           !(entry >= bound);
}

void closest_filtered(const rt_scene &s, const Filter &f, V3 o, V3 d, float &closest, int32_t &index, Work &w,
                      std::vector<FarEntry> &stack) {
    closest = f.B;
    index = -1;
    for (int k = 0; k < s.sphere_count; k++) {
        float t;
        w.st++;
        if (accept_sphere(s, f, o, d, k, closest, t)) { closest = t; index = k; }
    }
    if (0.0f >= closest) return;
    const float ix = 1 / d.x, iy = 1 / d.y, iz = 1 / d.z;
    stack.clear();
    int32_t n = 0;
    w.pn++;
    while (true) {
        const rt_bvh_node &nd = s.bvh[n];
        bool descend = false;
        if (nd.child2 <= nd.child1) {
            for (int j = nd.child2; j < nd.child1; j++) {
                float t;
                w.tt++;
                if (accept_triangle(s, f, o, d, j, closest, t)) { closest = t; index = s.sphere_count + j; }
            }
        } else {
            w.iv++;
            float t1, t2;
            const bool e1 = child_entered(s, nd.child1, o, ix, iy, iz, closest, t1);
            const bool e2 = child_entered(s, nd.child2, o, ix, iy, iz, closest, t2);
            if (e1 || e2) {
                const bool second = e2 && (!e1 || t2 < t1);
                if (e1 && e2) stack.push_back(second ? FarEntry{nd.child1, t1} : FarEntry{nd.child2, t2});
                n = second ? nd.child2 : nd.child1;
                w.pn++;
                descend = true;
            }
        }
        if (descend) continue;
        bool found = false;
        while (!stack.empty() && !found) {
            const FarEntry e = stack.back();
            stack.pop_back();
            if (!(e.entry >= closest)) { n = e.node; w.pn++; found = true; }
        }
        if (!found) return;
    }
}

bool occluded_filtered(const rt_scene &s, const Filter &f, V3 o, V3 d, Work &w, std::vector<int32_t> &stack) {
    const float B = f.B;
    for (int k = 0; k < s.sphere_count; k++) {
        float t;
        w.st++;
        if (accept_sphere(s, f, o, d, k, B, t)) return true;
    }
    if (0.0f >= B) return false;
    const float ix = 1 / d.x, iy = 1 / d.y, iz = 1 / d.z;
    stack.clear();
    int32_t n = 0;
    w.pn++;
    while (true) {
        const rt_bvh_node &nd = s.bvh[n];
        bool descend = false;
        if (nd.child2 <= nd.child1) {
            for (int j = nd.child2; j < nd.child1; j++) {
                float t;
                w.tt++;
                if (accept_triangle(s, f, o, d, j, B, t)) return true;
            }
        } else {
            w.iv++;
            float t1, t2;
            const bool e1 = child_entered(s, nd.child1, o, ix, iy, iz, B, t1);
            const bool e2 = child_entered(s, nd.child2, o, ix, iy, iz, B, t2);
            if (e1 || e2) {
                const bool second = e2 && (!e1 || t2 < t1);
                if (e1 && e2) stack.push_back(second ? nd.child1 : nd.child2);
                n = second ? nd.child2 : nd.child1;
                w.pn++;
                descend = true;
            }
        }
        if (descend) continue;
        if (stack.empty()) return false;
        n = stack.back();
        stack.pop_back();
        w.pn++;
    }
}

// The checks shared by the two filtered twins; > 0: n == 0, nothing to do.
int filtered_twin_args(const char *fn, const rt_scene *s, const void *rays, int32_t n) {
    const std::string f(fn);
    if (!s) return rtamd::fail(RT_E_INVALID, f + ": null scene");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative ray count");
    if (n == 0) return 1;
    if (!rays) return rtamd::fail(RT_E_INVALID, f + ": null pointer");
    if (s->bvh_node_count < 1 || !s->bvh) return rtamd::fail(RT_E_INVALID, f + ": scene has no BVH root");
    return RT_OK;
}

void fill_stats(rt_stats *st, int32_t n, const Work &w, uint64_t hits, uint64_t hits_sphere) {
    if (!st) return;
    std::memset(st, 0, sizeof(*st));
    st->live_segments = (uint64_t)n;
    st->nodes_popped = w.pn; st->internal_visits = w.iv; st->triangle_tests = w.tt; st->sphere_tests = w.st;
    st->hits = hits; st->misses = (uint64_t)n - hits; st->hits_sphere = hits_sphere;
}

}  // namespace

extern "C" int rt_scene_closest_filtered(const rt_scene *s, const uint32_t *masks, const float *rays,
                                         const rt_ray_filter *filter, int32_t n, float *t_out, int32_t *index_out,
                                         rt_stats *stats) {
    const int rc = filtered_twin_args("rt_scene_closest_filtered", s, rays, n);
    if (rc) return rc > 0 ? RT_OK : rc;
    std::vector<FarEntry> stack;
    Work w;
    uint64_t hits = 0, hits_sphere = 0;
    for (int32_t i = 0; i < n; i++) {
        const float *r = rays + (size_t)i * 6;
        float closest;
        int32_t index;
        closest_filtered(*s, filter_of(filter, masks, i), v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]), closest, index, w, stack);
        if (t_out) t_out[i] = index < 0 ? 1e30f : closest;
        if (index_out) index_out[i] = index;
        hits += index >= 0;
        hits_sphere += index >= 0 && index < s->sphere_count;
    }
    fill_stats(stats, n, w, hits, hits_sphere);
    return RT_OK;
}

extern "C" int rt_scene_occluded_filtered(const rt_scene *s, const uint32_t *masks, const float *rays,
                                          const rt_ray_filter *filter, int32_t n, uint8_t *occluded, rt_stats *stats) {
    const int rc = filtered_twin_args("rt_scene_occluded_filtered", s, rays, n);
    if (rc) return rc > 0 ? RT_OK : rc;
    if (!occluded) return rtamd::fail(RT_E_INVALID, "rt_scene_occluded_filtered: null pointer");
    std::vector<int32_t> stack;
    Work w;
    uint64_t hits = 0;
    for (int32_t i = 0; i < n; i++) {
        const float *r = rays + (size_t)i * 6;
        const bool occ = occluded_filtered(*s, filter_of(filter, masks, i), v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]), w, stack);
        occluded[i] = occ ? 1 : 0;
        hits += occ;
    }
    fill_stats(stats, n, w, hits, 0);
    return RT_OK;
}

// rt_scene_hemisphere, the host twin of rt_query_hemisphere: the generator of hemisphere_math.h, which
// hemisphere_kernel compiles too, and the filtered any-hit twin above, per work item.
extern "C" int rt_scene_hemisphere(const rt_scene *s, const uint32_t *masks, const float *frames, const rt_ray_filter *filter,
                                   int32_t n, const rt_hemisphere_params *params, const rt_hemisphere_out *out,
                                   rt_stats *stats) {
    namespace hemi = rtamd::hemi;
    const std::string f("rt_scene_hemisphere");
    if (!s) return rtamd::fail(RT_E_INVALID, f + ": null scene");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative point count");
    if (n == 0) return RT_OK;
    if (!frames) return rtamd::fail(RT_E_INVALID, f + ": null frames");
    if (const char *why = hemi::params_error(params, n)) return rtamd::fail(RT_E_INVALID, f + ": " + why);
    if (!out || (!out->open_count && !out->openness)) return rtamd::fail(RT_E_INVALID, f + ": no output pointer");
    if (s->bvh_node_count < 1 || !s->bvh) return rtamd::fail(RT_E_INVALID, f + ": scene has no BVH root");
    const uint32_t ns = (uint32_t)params->samples;
    std::vector<int32_t> stack;
    Work w;
    uint64_t hits = 0;
    for (int32_t i = 0; i < n; i++) {
        const float *r = frames + (size_t)i * 6;
        const V3 p = v3(r[0], r[1], r[2]), nh = hemi::unit_normal(v3(r[3], r[4], r[5]));
        const Filter fl = filter_of(filter, masks, i);
        uint32_t open = 0;
        for (uint32_t k = 0; k < ns; k++) {
            const V3 d = hemi::direction(nh, hemi::work_item(params->point_offset, (uint32_t)i, ns, k), params->seed, params->mode);
            open += occluded_filtered(*s, fl, p, d, w, stack) ? 0u : 1u;
        }
        hits += ns - open;
        if (out->open_count) out->open_count[i] = (int32_t)open;
        if (out->openness) out->openness[i] = (float)open / (float)ns;
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        const uint64_t rays = (uint64_t)n * ns;
        stats->live_segments = rays;
        stats->nodes_popped = w.pn; stats->internal_visits = w.iv; stats->triangle_tests = w.tt; stats->sphere_tests = w.st;
        stats->hits = hits; stats->misses = rays - hits;
    }
    return RT_OK;
}

extern "C" int rt_hemisphere_rays(const float *frames, int32_t n, const rt_hemisphere_params *params, float *rays_out) {
    namespace hemi = rtamd::hemi;
    const std::string f("rt_hemisphere_rays");
    if (n < 0) return rtamd::fail(RT_E_INVALID, f + ": negative point count");
    if (n == 0) return RT_OK;
    if (!frames || !rays_out) return rtamd::fail(RT_E_INVALID, f + ": null pointer");
    if (const char *why = hemi::params_error(params, n)) return rtamd::fail(RT_E_INVALID, f + ": " + why);
    const uint32_t ns = (uint32_t)params->samples;
    for (int32_t i = 0; i < n; i++) {
        const float *r = frames + (size_t)i * 6;
        const V3 nh = hemi::unit_normal(v3(r[3], r[4], r[5]));
        for (uint32_t k = 0; k < ns; k++) {
            const V3 d = hemi::direction(nh, hemi::work_item(params->point_offset, (uint32_t)i, ns, k), params->seed, params->mode);
            float *o = rays_out + ((size_t)i * ns + k) * 6;
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
            o[3] = d.x; o[4] = d.y; o[5] = d.z;
        }
    }
    return RT_OK;
}

extern "C" int rt_scene_overlap_box(const rt_scene *s, const float *boxes, int32_t n, int32_t k, const rt_overlap_out *out) {
    namespace ov = rtamd::ov;
    if (!s) return rtamd::fail(RT_E_INVALID, "rt_scene_overlap_box: null scene");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_scene_overlap_box: negative box count");
    if (k < 1 || k > RT_OVERLAP_K_MAX)
        return rtamd::fail(RT_E_INVALID, "rt_scene_overlap_box: k " + std::to_string(k) + " is outside 1.." +
                                             std::to_string(RT_OVERLAP_K_MAX));
    if (n == 0) return RT_OK;
    if (!boxes || !out) return rtamd::fail(RT_E_INVALID, "rt_scene_overlap_box: null pointer");
    if ((int64_t)n * k > INT32_MAX)
        return rtamd::fail(RT_E_INVALID, "rt_scene_overlap_box: n * k = " + std::to_string((int64_t)n * k) + " does not fit int32");
    if (s->bvh_node_count < 1 || !s->bvh) return rtamd::fail(RT_E_INVALID, "rt_scene_overlap_box: scene has no BVH root");
    const bool first_only = !out->index && !out->count && out->any;
    std::vector<int32_t> found, stack;
    for (int32_t i = 0; i < n; i++) {
        const float *b = boxes + (size_t)i * 6;
        const rt_vec3 lo = {b[0], b[1], b[2]}, hi = {b[3], b[4], b[5]};
        found.clear();
        if (ov::valid_box(lo, hi)) overlapping(*s, lo, hi, first_only, found, stack);
        if (out->count) out->count[i] = (int32_t)found.size();
        if (out->any) out->any[i] = found.empty() ? 0 : 1;
        if (!out->index) continue;
        std::sort(found.begin(), found.end());
        for (int32_t j = 0; j < k; j++) out->index[(size_t)i * k + j] = (size_t)j < found.size() ? found[j] : -1;
    }
    return RT_OK;
}

extern "C" int rt_scene_nearest_k(const rt_scene *s, const float *points, const float *max_dist, int32_t n, int32_t k,
                                  const rt_nearest_k_out *out) {
    namespace cp = rtamd::cp;
    if (!s) return rtamd::fail(RT_E_INVALID, "rt_scene_nearest_k: null scene");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_scene_nearest_k: negative point count");
    if (k < 1 || k > RT_NEAREST_K_MAX)
        return rtamd::fail(RT_E_INVALID, "rt_scene_nearest_k: k " + std::to_string(k) + " is outside 1.." +
                                             std::to_string(RT_NEAREST_K_MAX));
    if (n == 0) return RT_OK;
    if (!points || !out) return rtamd::fail(RT_E_INVALID, "rt_scene_nearest_k: null pointer");
    if ((int64_t)n * k > INT32_MAX)
        return rtamd::fail(RT_E_INVALID, "rt_scene_nearest_k: n * k = " + std::to_string((int64_t)n * k) + " does not fit int32");
    if (s->bvh_node_count < 1 || !s->bvh) return rtamd::fail(RT_E_INVALID, "rt_scene_nearest_k: scene has no BVH root");
    std::vector<Member> found;
    std::vector<int32_t> stack;
    for (int32_t i = 0; i < n; i++) {
        const rt_vec3 p = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
        const float b2 = max_dist ? cp::bound2(max_dist[i]) : INFINITY;
        found.clear();
        if (cp::finite3(p)) members(*s, p, b2, found, stack);
        std::sort(found.begin(), found.end(),
                  [](const Member &a, const Member &b) { return cp::key_less(a.key, a.index, b.key, b.index); });
        if (out->count) out->count[i] = (int32_t)found.size();
        for (int32_t j = 0; j < k; j++) {
            const size_t e = (size_t)i * k + j;
            const bool have = (size_t)j < found.size();
            if (out->distance) out->distance[e] = have ? sqrtf(found[j].dist2) : 1e30f;
            if (out->index) out->index[e] = have ? found[j].index : -1;
            if (!out->point) continue;
            rt_vec3 q{0.0f, 0.0f, 0.0f};
            if (have && found[j].index < s->sphere_count) {
                q = cp::sphere(p, s->spheres[found[j].index].center, s->spheres[found[j].index].radius).point;
            } else if (have) {
                const rt_triangle &tr = s->triangles[found[j].index - s->sphere_count];
                q = cp::triangle(p, tr.p1, tr.p2p1, tr.p3p1).point;
            }
            out->point[e * 3] = q.x; out->point[e * 3 + 1] = q.y; out->point[e * 3 + 2] = q.z;
        }
    }
    return RT_OK;
}

extern "C" int rt_scene_closest_point(const rt_scene *s, const float *points, const float *max_dist, int32_t n,
                                      const rt_closest_point_out *out) {
    namespace cp = rtamd::cp;
    if (!s) return rtamd::fail(RT_E_INVALID, "rt_scene_closest_point: null scene");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_scene_closest_point: negative point count");
    if (n == 0) return RT_OK;
    if (!points || !out) return rtamd::fail(RT_E_INVALID, "rt_scene_closest_point: null pointer");
    if (s->bvh_node_count < 1 || !s->bvh) return rtamd::fail(RT_E_INVALID, "rt_scene_closest_point: scene has no BVH root");
    std::vector<Entry> stack;
    for (int32_t i = 0; i < n; i++) {
        const rt_vec3 p = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
        float best2 = max_dist ? cp::bound2(max_dist[i]) : INFINITY;
        int32_t best = INT32_MAX;
        if (cp::finite3(p)) nearest(*s, p, best2, best, stack);
        const bool hit = best != INT32_MAX;
        cp::Near nr{0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
        if (hit && best < s->sphere_count) {
            nr = cp::sphere(p, s->spheres[best].center, s->spheres[best].radius);
        } else if (hit) {
            const rt_triangle &tr = s->triangles[best - s->sphere_count];
            nr = cp::triangle(p, tr.p1, tr.p2p1, tr.p3p1);
        }
        if (out->distance) out->distance[i] = hit ? sqrtf(best2) : 1e30f;
        if (out->index) out->index[i] = hit ? best : -1;
        if (out->point) {
            float *q = out->point + (size_t)i * 3;
            q[0] = nr.point.x; q[1] = nr.point.y; q[2] = nr.point.z;
        }
        if (out->uv) {
            out->uv[(size_t)i * 2] = nr.u;
            out->uv[(size_t)i * 2 + 1] = nr.v;
        }
    }
    return RT_OK;
}

extern "C" int rt_scene_multi_hit(const rt_scene *s, const float *rays, const float *tmax, int32_t n, int32_t k,
                                  const rt_multi_hit_out *out) {
    if (!s) return rtamd::fail(RT_E_INVALID, "rt_scene_multi_hit: null scene");
    if (n < 0) return rtamd::fail(RT_E_INVALID, "rt_scene_multi_hit: negative ray count");
    if (k < 1 || k > RT_MULTI_HIT_MAX)
        return rtamd::fail(RT_E_INVALID, "rt_scene_multi_hit: k " + std::to_string(k) + " is outside 1.." +
                                             std::to_string(RT_MULTI_HIT_MAX));
    if (n == 0) return RT_OK;
    if (!rays || !out) return rtamd::fail(RT_E_INVALID, "rt_scene_multi_hit: null pointer");
    if ((int64_t)n * k > INT32_MAX)
        return rtamd::fail(RT_E_INVALID, "rt_scene_multi_hit: n * k = " + std::to_string((int64_t)n * k) + " does not fit int32");
    std::vector<Hit> hits;
    std::vector<int32_t> stack;
    for (int32_t i = 0; i < n; i++) {
        const float *r = rays + (size_t)i * 6;
        float B = 1e30f;
        if (tmax) B = tmax[i] <= 1e30f ? tmax[i] : 1e30f;
        all_hits(*s, v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]), B, hits, stack);
        std::sort(hits.begin(), hits.end(),
                  [](const Hit &a, const Hit &b) { return a.key != b.key ? a.key < b.key : a.index < b.index; });
        if (out->count) out->count[i] = (int32_t)hits.size();
        for (int32_t j = 0; j < k; j++) {
            const bool have = (size_t)j < hits.size();
            if (out->t) out->t[(size_t)i * k + j] = have ? hits[j].t : 1e30f;
            if (out->index) out->index[(size_t)i * k + j] = have ? hits[j].index : -1;
        }
    }
    return RT_OK;
}
