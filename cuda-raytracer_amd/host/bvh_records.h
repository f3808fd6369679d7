// bvh_records.h — the 64-B child-pair node records the traversal kernels read, laid out on
// the host from a scene's node array.  No HIP dependency.
//
// A record belongs to an internal node and holds both children: three 16-B rows with the children's
// bounds interleaved per plane, so one packed-fp32 op handles both boxes,
//   {lx0 lx1 ly0 ly1} {lz0 lz1 hx0 hx1} {hy0 hy1 hz0 hz1}      (0 = child1, 1 = child2)
// and a fourth row {ref0, ref1, 0, 0}.  A ref is the child's own record number, or for a leaf child
// kLeaf | count << 24 | begin (count < 64, begin < 2^24), or kLeaf | kBigLeaf | index into the table
// of {begin, end} ranges for leaves that do not fit.
#pragma once
#include "rt_abi.h"

#include <string>
#include <vector>

namespace rtamd {

constexpr uint32_t kLeaf = 0x80000000u, kBigLeaf = 0x40000000u;

namespace records {

struct Row { float x, y, z, w; };           // the device's float4
struct Range { int32_t begin, end; };       // the device's int2
static_assert(sizeof(Row) == 16 && sizeof(Range) == 8, "device layout");

struct Records {
    std::vector<int> node_rec;              // node -> its record, -1 for a leaf
    std::vector<Row> rows;                  // 4 per record; one zero record when the root is a leaf
    std::vector<Range> big;                 // never empty: {0, 0} when no leaf needs it
    uint32_t root_ref = kLeaf;
};

// Record numbering: record 0 is the root's and record 1 padding (the root has no sibling); the two
// children of a node get adjacent records (an even/odd pair, one 128-B line), so stepping into one child
// brings in its sibling's record too, which the stack usually visits next; pairs are handed out in
// depth-first order, child1's subtree first, so a subtree's records stay close.  Layout only: the
// traversal order is unchanged.
// A visit of an internal node at depth k can leave k + 1 entries on the traversal stack, so a tree with
// an internal node at depth >= max_depth is refused (the reference's MAX_BVH_DEPTH 30 gives at most 30,
// scene.cu:10).  Returns the empty string, or why the node array is refused.
std::string build(const rt_scene *sc, int max_depth, Records &out);

// The two children's boxes of one record (4 rows), bit for bit.
void unpack(const Row *rec, rt_vec3 &min1, rt_vec3 &max1, rt_vec3 &min2, rt_vec3 &max2);

}  // namespace records
}  // namespace rtamd
