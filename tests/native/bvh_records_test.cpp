// bvh_records_test.cpp — the child-pair record layout (cuda-raytracer_amd/host/bvh_records.cpp) on
// hand-built trees: numbering, leaf refs, the depth limit, refused node arrays and the unpack round trip.
// Stand-alone (tests/test_bvh_records.py builds it with -fsanitize=address,undefined).
//   bvh_records_test            runs every case; prints "ok <n> checks" and exits 0, or the failed checks
#include "bvh_records.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace rtamd;
using records::Records;
using records::Row;

namespace {

int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        g_checks++;                                                            \
        if (!(cond)) {                                                         \
            g_failed++;                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
        }                                                                      \
    } while (0)

constexpr int kDepthLimit = 32;             // the library's kStackMax

// Bounds with awkward bit patterns, different for every node and plane.
rt_bvh_node node(int i, int child1, int child2) {
    const float odd[] = {-0.0f, std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::infinity(),
                         -std::numeric_limits<float>::infinity(), 1e-42f, -1.5f};
    rt_bvh_node n{};
    float *f[6] = {&n.min_bound.x, &n.min_bound.y, &n.min_bound.z, &n.max_bound.x, &n.max_bound.y, &n.max_bound.z};
    for (int k = 0; k < 6; k++) *f[k] = (i + k) % 3 == 0 ? odd[(i + k) / 3 % 6] : (float)(i * 6 + k) + 0.25f;
    n.child1 = child1;
    n.child2 = child2;
    return n;
}
rt_bvh_node leaf(int i, int begin, int count) { return node(i, begin + count, begin); }   // child2 <= child1

std::string build(const std::vector<rt_bvh_node> &bvh, Records &r, int depth_limit = kDepthLimit) {
    rt_scene sc{};
    sc.bvh = bvh.data();
    sc.bvh_node_count = (int)bvh.size();
    return records::build(&sc, depth_limit, r);
}

uint32_t ref(const Records &r, int rec, int child) {
    uint32_t v;
    std::memcpy(&v, child ? &r.rows[(size_t)rec * 4 + 3].y : &r.rows[(size_t)rec * 4 + 3].x, 4);
    return v;
}
uint32_t small_leaf(int begin, int count) { return kLeaf | ((uint32_t)count << 24) | (uint32_t)begin; }

// unpack(record of node i) == the children's bounds, bit for bit, for every record of an accepted tree
void round_trip(const std::vector<rt_bvh_node> &bvh, const Records &r) {
    int records_seen = 0;
    for (size_t i = 0; i < bvh.size(); i++) {
        if (r.node_rec[i] < 0) continue;
        records_seen++;
        rt_vec3 b[4];
        records::unpack(&r.rows[(size_t)r.node_rec[i] * 4], b[0], b[1], b[2], b[3]);
        const rt_bvh_node &l = bvh[bvh[i].child1], &rr = bvh[bvh[i].child2];
        CHECK(!std::memcmp(&b[0], &l.min_bound, sizeof(rt_vec3)) && !std::memcmp(&b[1], &l.max_bound, sizeof(rt_vec3)));
        CHECK(!std::memcmp(&b[2], &rr.min_bound, sizeof(rt_vec3)) && !std::memcmp(&b[3], &rr.max_bound, sizeof(rt_vec3)));
        const Row &refs = r.rows[(size_t)r.node_rec[i] * 4 + 3];
        CHECK(refs.z == 0.0f && refs.w == 0.0f);
    }
    CHECK(records_seen > 0 || bvh[0].child2 <= bvh[0].child1);
}

void root_leaf() {
    Records r;
    CHECK(build({leaf(0, 0, 5)}, r).empty());
    CHECK(r.node_rec == std::vector<int>{-1});
    CHECK(r.root_ref == small_leaf(0, 5));
    CHECK(r.rows.size() == 4);                  // one zero record, so the device array is never empty
    for (const Row &q : r.rows) CHECK(q.x == 0 && q.y == 0 && q.z == 0 && q.w == 0);
    CHECK(r.big.size() == 1 && r.big[0].begin == 0 && r.big[0].end == 0);
    // an empty root leaf (a scene without triangles)
    CHECK(build({leaf(0, 0, 0)}, r).empty() && r.root_ref == kLeaf);
}

void three_nodes() {
    const std::vector<rt_bvh_node> bvh{node(0, 1, 2), leaf(1, 0, 3), leaf(2, 3, 4)};
    Records r;
    CHECK(build(bvh, r).empty());
    CHECK((r.node_rec == std::vector<int>{0, -1, -1}));
    CHECK(r.root_ref == 0);
    CHECK(r.rows.size() == 8);                  // record 0 and its padding
    CHECK(ref(r, 0, 0) == small_leaf(0, 3) && ref(r, 0, 1) == small_leaf(3, 4));
    for (int k = 4; k < 8; k++) CHECK(r.rows[k].x == 0 && r.rows[k].y == 0 && r.rows[k].z == 0 && r.rows[k].w == 0);
    round_trip(bvh, r);
}

void seven_nodes() {
    //        0
    //     1     2          both internal: records 2 and 3
    //   3  4   5  6        leaves
    std::vector<rt_bvh_node> bvh{node(0, 1, 2), node(1, 3, 4), node(2, 5, 6),
                                 leaf(3, 0, 1), leaf(4, 1, 1), leaf(5, 2, 1), leaf(6, 3, 1)};
    Records r;
    CHECK(build(bvh, r).empty());
    CHECK((r.node_rec == std::vector<int>{0, 2, 3, -1, -1, -1, -1}));
    CHECK(ref(r, 0, 0) == 2 && ref(r, 0, 1) == 3);
    CHECK(ref(r, 2, 0) == small_leaf(0, 1) && ref(r, 3, 1) == small_leaf(3, 1));
    round_trip(bvh, r);
    // depth-first, child1's subtree first: with internal grandchildren under both children, node 1's
    // children get the pair after the root's, and node 2's children come after node 1's whole subtree
    //   0 -> (1, 2);  1 -> (3, 4);  2 -> (5, 6);  3 -> (7, 8);  5 -> (9, 10);  4, 6..10 leaves
    bvh = {node(0, 1, 2), node(1, 3, 4), node(2, 5, 6), node(3, 7, 8), leaf(4, 0, 1), node(5, 9, 10), leaf(6, 1, 1),
           leaf(7, 2, 1), leaf(8, 3, 1), leaf(9, 4, 1), leaf(10, 5, 1)};
    CHECK(build(bvh, r).empty());
    //                        node:  0  1  2  3   4  5   6 ...
    CHECK((r.node_rec == std::vector<int>{0, 2, 3, 4, -1, 6, -1, -1, -1, -1, -1}));
    CHECK(r.rows.size() == 8 * 4);             // records 0..7; 5 and 7 are the leaf siblings' unused halves
    round_trip(bvh, r);
    // only child2 internal: it still gets the odd record of its pair
    bvh = {node(0, 1, 2), leaf(1, 0, 1), node(2, 3, 4), leaf(3, 1, 1), leaf(4, 2, 1)};
    CHECK(build(bvh, r).empty());
    CHECK((r.node_rec == std::vector<int>{0, -1, 3, -1, -1}));
    round_trip(bvh, r);
}

void leaf_sizes() {
    const int far = 1 << 24;
    const std::vector<rt_bvh_node> bvh{node(0, 1, 2), node(1, 3, 4), leaf(2, 100, 63), leaf(3, 200, 64),
                                       leaf(4, far, 2)};
    Records r;
    CHECK(build(bvh, r).empty());
    CHECK(ref(r, 0, 1) == small_leaf(100, 63));                    // 63 triangles: inline
    CHECK(ref(r, 2, 0) == (kLeaf | kBigLeaf | 0u));                // 64: the table
    CHECK(ref(r, 2, 1) == (kLeaf | kBigLeaf | 1u));                // begin >= 2^24: the table
    CHECK(r.big.size() == 2);
    CHECK(r.big[0].begin == 200 && r.big[0].end == 264);
    CHECK(r.big[1].begin == far && r.big[1].end == far + 2);
    round_trip(bvh, r);
    // begin = 2^24 - 1 still fits a ref
    Records s;
    CHECK(build({node(0, 1, 2), leaf(1, far - 1, 1), leaf(2, 0, 1)}, s).empty());
    CHECK(ref(s, 0, 0) == small_leaf(far - 1, 1) && s.big.size() == 1 && s.big[0].end == 0);
    // a big root leaf
    CHECK(build({leaf(0, 0, 1000)}, s).empty());
    CHECK(s.root_ref == (kLeaf | kBigLeaf | 0u) && s.big.size() == 1 && s.big[0].begin == 0 && s.big[0].end == 1000);
}

// A left-deep chain: node d < n is the internal node at depth d (n = deepest + 1 of them), its child1 the next
// one (the last one's: leaf n), its child2 the leaf n + 1 + d.
std::vector<rt_bvh_node> chain(int deepest) {
    const int n = deepest + 1;
    std::vector<rt_bvh_node> bvh;
    for (int d = 0; d < n; d++) bvh.push_back(node(d, d + 1, n + 1 + d));
    for (int k = 0; k <= n; k++) bvh.push_back(leaf(n + k, k, 1));
    return bvh;
}

void depth() {
    Records r;
    const std::vector<rt_bvh_node> ok = chain(kDepthLimit - 1);
    CHECK(build(ok, r).empty());
    CHECK(r.node_rec[kDepthLimit - 1] == 2 * (kDepthLimit - 1));   // one pair per level, child1 internal: even
    round_trip(ok, r);
    CHECK(build(chain(kDepthLimit), r) == "BVH deeper than the traversal stack (32 internal levels)");
}

void bad_trees() {
    Records r;
    CHECK(build({node(0, -1, 2), leaf(1, 0, 1), leaf(2, 1, 1)}, r) == "BVH child index out of range");
    CHECK(build({node(0, 1, 3), leaf(1, 0, 1), leaf(2, 1, 1)}, r) == "BVH child index out of range");
    CHECK(build({node(0, 1, 2), leaf(1, 0, 1), node(2, 1, 3)}, r) == "BVH child index out of range");
    // node 2 is its own descendant (through its child 2), and so is the root
    CHECK(build({node(0, 1, 2), leaf(1, 0, 1), node(2, 1, 2)}, r) == "BVH is not a tree");
    CHECK(build({node(0, 1, 2), leaf(1, 0, 1), node(2, 0, 3), leaf(3, 0, 1)}, r) == "BVH is not a tree");
}

}  // namespace

int main() {
    root_leaf();
    three_nodes();
    seven_nodes();
    leaf_sizes();
    depth();
    bad_trees();
    if (g_failed) {
        std::printf("%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
