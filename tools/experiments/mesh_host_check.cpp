// mesh_host_check.cpp — stand-alone driver of rt_scene_from_mesh and rt_scene_face_index (host/scene_mesh.cpp,
// host/scene_load.cpp) for sanitizer runs on the CPU: no GPU, no Python.
//
// For every scene file on the command line it loads the scene, takes its triangles' vertices (p1, p1 + p2p1,
// p1 + p3p1), its spheres, materials and material indices, and builds the mesh scene twice, from a soup and from an
// indexed mesh (vertex rows de-duplicated on their bit patterns), every array in a heap block of exactly its size.
// Both must equal each other byte for byte; the face index must be a permutation that maps every scene triangle
// back to its input triangle and material.  Then every refusal of the entry is provoked, each on exactly sized
// arrays, and its message is checked.
//
//   D=cuda-raytracer_amd; I="-Iinclude -I$D/host -I$D/csrc"; S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   clang++ -std=c++17 -O1 -g -ffp-contract=off $S $I tools/experiments/mesh_host_check.cpp $D/host/scene_load.cpp \
//     $D/host/scene_mesh.cpp $D/host/scene_refit.cpp -lpthread -o mesh_host_check
//   RT_ASSETS=assets ./mesh_host_check assets/cornell.scene size_4097.scene      (tests/bvh_build_cases.write's file)
// The device builds are weak references of scene_load.cpp and stay unresolved here: bvh_device >= 0 is RT_E_NODEVICE.
#include "rt_abi.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <array>
#include <memory>
#include <string>
#include <vector>

static int failures = 0;

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {     // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

static rt_load_opts opts() {
    rt_load_opts lo;
    rt_default_load_opts(&lo);
    lo.quiet = 1;
    lo.asset_root = std::getenv("RT_ASSETS");
    lo.image_override = 1;
    lo.width = lo.height = 16;
    lo.ray_count = lo.bounces = 1;
    return lo;
}

static void expect_refusal(const char *what, const rt_mesh_desc *m, const rt_load_opts *lo, rt_scene_host **out,
                           const char *message) {
    const int rc = rt_scene_from_mesh(m, lo, out);
    if (rc != RT_E_INVALID || !std::strstr(rt_last_error(), message)) {
        std::printf("refusal '%s': rc %d, message '%s' (wanted '%s')\n", what, rc, rc ? rt_last_error() : "", message);
        failures++;
        if (rc == RT_OK && out && *out) rt_scene_free(*out);
    }
}

static bool same_scene(const rt_scene_host *a, const rt_scene_host *b) {
    const rt_scene *x = rt_scene_view(a), *y = rt_scene_view(b);
    if (x->triangle_count != y->triangle_count || x->sphere_count != y->sphere_count ||
        x->bvh_node_count != y->bvh_node_count || x->material_count != y->material_count)
        return false;
    const size_t prims = (size_t)x->sphere_count + x->triangle_count;
    if (std::memcmp(x->triangles, y->triangles, sizeof(rt_triangle) * x->triangle_count) ||
        std::memcmp(x->bvh, y->bvh, sizeof(rt_bvh_node) * x->bvh_node_count) ||
        std::memcmp(x->material_indices, y->material_indices, sizeof(uint16_t) * prims) ||
        std::memcmp(x->materials, y->materials, sizeof(rt_material) * x->material_count) ||
        (x->sphere_count && std::memcmp(x->spheres, y->spheres, sizeof(rt_sphere) * x->sphere_count)))
        return false;
    return !std::memcmp(&x->camera_position, &y->camera_position, sizeof(rt_scene) - offsetof(rt_scene, camera_position));
}

static void refusals() {
    const std::vector<float> v = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 2, 2, 2};
    const std::vector<int32_t> f = {0, 1, 2, 0, 1, 3, 1, 2, 3};
    const std::vector<rt_material> mats(5);
    const std::vector<rt_sphere> sph = {{{0, 0, 0}, 1}, {{1, 1, 1}, 1}};
    const rt_load_opts lo = opts();
    rt_scene_host *h = nullptr;
    auto V = exact(v);
    auto F = exact(f);
    auto M = exact(mats);
    auto S = exact(sph);
    rt_mesh_desc good{};
    good.vertices = V.get(); good.vertex_count = 5; good.indices = F.get(); good.triangle_count = 3;
    if (rt_scene_from_mesh(&good, &lo, &h)) { std::printf("good mesh refused: %s\n", rt_last_error()); failures++; }
    else rt_scene_free(h);
    expect_refusal("null mesh", nullptr, &lo, &h, "null argument");
    expect_refusal("null out", &good, &lo, nullptr, "null argument");
    rt_mesh_desc m = good;
    m.vertex_count = -1; expect_refusal("negative vertex count", &m, &lo, &h, "negative count");
    m = good; m.triangle_count = -1; expect_refusal("negative triangle count", &m, &lo, &h, "negative count");
    m = good; m.sphere_count = -1; expect_refusal("negative sphere count", &m, &lo, &h, "negative count");
    m = good; m.material_count = -1; expect_refusal("negative material count", &m, &lo, &h, "negative count");
    m = good; m.vertices = nullptr; expect_refusal("null vertices", &m, &lo, &h, "null vertices with 3 triangles");
    m = good; m.indices = nullptr; m.triangle_count = 1;
    expect_refusal("soup count", &m, &lo, &h, "a soup of 1 triangles needs 3 vertices, not 5");
    const std::vector<uint16_t> tm = {0, 4, 5}, sm = {4, 5};
    auto TM = exact(tm);
    auto SM = exact(sm);
    m = good; m.triangle_materials = TM.get();
    expect_refusal("indices without a table", &m, &lo, &h, "material indices without a material table");
    m.materials = M.get(); m.material_count = 5;
    expect_refusal("triangle material", &m, &lo, &h, "triangle 2 has a material index outside the table of 5 materials");
    m = good; m.materials = M.get(); m.material_count = 5; m.spheres = S.get(); m.sphere_count = 2; m.sphere_materials = SM.get();
    expect_refusal("sphere material", &m, &lo, &h, "sphere 1 has a material index outside the table of 5 materials");
    m = good; m.materials = M.get(); m.material_count = 65536;
    expect_refusal("too many materials", &m, &lo, &h, "more than 65535 materials");
    m = good; m.spheres = S.get(); m.sphere_count = 0x7fffffff - 2;
    expect_refusal("count overflow", &m, &lo, &h, "does not fit int32");
    rt_load_opts small = lo;
    small.width = 1;
    expect_refusal("image size", &good, &small, &h, "scene image must be at least 2x2");
    for (int32_t bad : {-1, 5, INT32_MIN, INT32_MAX})
        for (int t : {0, 2}) {
            std::vector<int32_t> f2 = f;
            f2[3 * t + 1] = bad;
            std::vector<float> v2 = v;
            v2[12] = NAN;                                   // vertex 4: referenced by nobody
            auto F2 = exact(f2);
            auto V2 = exact(v2);
            m = good; m.indices = F2.get(); m.vertices = V2.get();
            const std::string want = "triangle " + std::to_string(t) + " has a vertex index outside [0, 5)";
            expect_refusal("vertex index", &m, &lo, &h, want.c_str());
        }
    {
        std::vector<float> v2 = v;
        v2[12] = NAN;
        auto V2 = exact(v2);
        m = good; m.vertices = V2.get();
        if (rt_scene_from_mesh(&m, &lo, &h)) { std::printf("unreferenced NaN refused: %s\n", rt_last_error()); failures++; }
        else rt_scene_free(h);
        v2 = v;
        v2[10] = INFINITY;                                  // vertex 3: triangles 1 and 2
        auto V3 = exact(v2);
        m.vertices = V3.get();
        expect_refusal("referenced inf", &m, &lo, &h, "triangle 1 has a non-finite coordinate");
        std::vector<float> soup(18, 0.0f);
        soup[9] = soup[12] = 3e38f;
        auto V4 = exact(soup);
        rt_mesh_desc s2{};
        s2.vertices = V4.get(); s2.vertex_count = 6; s2.triangle_count = 2;
        expect_refusal("centroid overflow", &s2, &lo, &h, "triangle 1 has a non-finite centroid: the sum of its vertices overflows");
        std::vector<rt_sphere> bad_sphere = sph;
        bad_sphere[1].radius = NAN;
        auto S2 = exact(bad_sphere);
        m = good; m.spheres = S2.get(); m.sphere_count = 2;
        expect_refusal("sphere", &m, &lo, &h, "sphere 1 has a non-finite coordinate or radius");
    }
    rt_load_opts dev = lo;
    dev.bvh_device = 0;
    if (rt_scene_from_mesh(&good, &dev, &h) != RT_E_NODEVICE) { std::printf("device build was not RT_E_NODEVICE\n"); failures++; }
    std::printf("refusals: checked\n");
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        rt_load_opts lo = opts();
        rt_scene_host *src = nullptr;
        if (rt_scene_load(argv[a], &lo, &src)) {
            std::printf("%s: load failed: %s\n", argv[a], rt_last_error());
            failures++;
            continue;
        }
        const rt_scene *s = rt_scene_view(src);
        const int n = s->triangle_count, ns = s->sphere_count;
        std::vector<float> soup((size_t)n * 9);
        for (int i = 0; i < n; i++) {
            const rt_triangle &t = s->triangles[i];
            const float v[9] = {t.p1.x, t.p1.y, t.p1.z, t.p1.x + t.p2p1.x, t.p1.y + t.p2p1.y, t.p1.z + t.p2p1.z,
                                t.p1.x + t.p3p1.x, t.p1.y + t.p3p1.y, t.p1.z + t.p3p1.z};
            std::memcpy(&soup[(size_t)i * 9], v, sizeof(v));
        }
        std::map<std::array<uint32_t, 3>, int32_t> seen;    // indexed: rows de-duplicated on their bits
        std::vector<float> verts;
        std::vector<int32_t> faces((size_t)n * 3);
        for (size_t r = 0; r < (size_t)n * 3; r++) {
            std::array<uint32_t, 3> key;
            std::memcpy(key.data(), &soup[r * 3], 12);
            auto it = seen.find(key);
            if (it == seen.end()) {
                it = seen.emplace(key, (int32_t)(verts.size() / 3)).first;
                verts.insert(verts.end(), &soup[r * 3], &soup[r * 3] + 3);
            }
            faces[r] = it->second;
        }
        std::vector<rt_sphere> sph(s->spheres, s->spheres + ns);
        std::vector<rt_material> mats(s->materials, s->materials + s->material_count);
        std::vector<uint16_t> smat(s->material_indices, s->material_indices + ns), tmat(s->material_indices + ns, s->material_indices + ns + n);
        auto SOUP = exact(soup);
        auto V = exact(verts);
        auto F = exact(faces);
        auto SP = exact(sph);
        auto M = exact(mats);
        auto SM = exact(smat);
        auto TM = exact(tmat);
        const rt_camera_desc cam{{0, 0, -10}, {0.1f, 0, 1}, {0, 1, 0.2f}, 40};
        const rt_vec3 sky{0.6f, 0.7f, 0.9f};
        rt_mesh_desc m{};
        m.vertices = SOUP.get(); m.vertex_count = 3 * n; m.triangle_count = n; m.triangle_materials = TM.get();
        m.spheres = ns ? SP.get() : nullptr; m.sphere_count = ns; m.sphere_materials = ns ? SM.get() : nullptr;
        m.materials = M.get(); m.material_count = s->material_count; m.camera = &cam; m.sky = &sky;
        rt_scene_host *a1 = nullptr, *a2 = nullptr, *a3 = nullptr;
        rt_mesh_desc mi = m;
        mi.vertices = V.get(); mi.vertex_count = (int32_t)(verts.size() / 3); mi.indices = F.get();
        rt_load_opts flat = lo;
        flat.use_bvh = 0;
        if (rt_scene_from_mesh(&m, &lo, &a1) || rt_scene_from_mesh(&mi, &lo, &a2) || rt_scene_from_mesh(&mi, &flat, &a3)) {
            std::printf("%s: from_mesh failed: %s\n", argv[a], rt_last_error());
            failures++;
            continue;
        }
        if (!same_scene(a1, a2)) { std::printf("%s: soup and indexed mesh differ\n", argv[a]); failures++; }
        if (rt_scene_view(a3)->bvh_node_count != 1) { std::printf("%s: use_bvh = 0 is not one leaf\n", argv[a]); failures++; }
        for (rt_scene_host *h : {a1, a2, a3}) {
            const int32_t *fi = nullptr;
            int32_t count = -1;
            if (rt_scene_face_index(h, &fi, &count) || count != n) { std::printf("%s: face index count %d\n", argv[a], count); failures++; continue; }
            std::vector<char> hit(n, 0);
            const rt_scene *x = rt_scene_view(h);
            int wrong = 0;
            for (int j = 0; j < n; j++) {
                if (fi[j] < 0 || fi[j] >= n || hit[fi[j]]++) { wrong++; continue; }
                wrong += std::memcmp(&x->triangles[j].p1, &soup[(size_t)fi[j] * 9], 12) != 0;
                wrong += x->material_indices[ns + j] != tmat[fi[j]];
            }
            if (wrong) { std::printf("%s: %d face index entries are wrong\n", argv[a], wrong); failures++; }
        }
        // a refit leaves the face index alone
        const int32_t *fi = nullptr;
        int32_t count = 0;
        rt_scene_face_index(a1, &fi, &count);
        std::vector<int32_t> before(fi, fi + count);
        std::vector<float> moved((size_t)n * 9);
        for (int j = 0; j < n; j++)
            for (int k = 0; k < 9; k++) moved[(size_t)j * 9 + k] = soup[(size_t)fi[j] * 9 + k] * 1.5f + 0.25f;
        auto MV = exact(moved);
        if (rt_scene_refit(a1, MV.get(), n)) { std::printf("%s: refit failed: %s\n", argv[a], rt_last_error()); failures++; }
        rt_scene_face_index(a1, &fi, &count);
        if (count != n || (n && std::memcmp(fi, before.data(), sizeof(int32_t) * n))) { std::printf("%s: refit changed the face index\n", argv[a]); failures++; }
        std::printf("%s: %d triangles (%zu distinct vertices), %d spheres: soup, indexed, no_bvh, face index, refit checked\n",
                    argv[a], n, verts.size() / 3, ns);
        rt_scene_free(a1); rt_scene_free(a2); rt_scene_free(a3); rt_scene_free(src);
    }
    refusals();
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
