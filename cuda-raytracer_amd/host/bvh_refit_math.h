// bvh_refit_math.h — the refit definition (include/rt_abi.h), shared by its host twin
// (host/scene_refit.cpp) and the gfx950 kernels (csrc/bvh_refit.hip) so both evaluate one text.
//
// A triangle's record is the loader's ray-tracing representation of its three vertices
// (scene_load.cpp: p1, p2 - p1, p3 - p1, normalise(cross(p3 - p1, p2 - p1)), no contraction); bounds are
// folds of the absolute vertices with the loader's fmin_/fmax_, which keep the earlier operand of a tie.
// "Earliest of the smallest" is associative, so a box may be folded hierarchically (vertices -> triangle
// -> leaf -> node) and still equals the builder's linear fold over the node's range, zero signs included.
// The compare is explicit: the hardware's v_min_f32 orders -0 below +0.
#pragma once
#include "rt_abi.h"

#include <math.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#define RT_REFIT_HD __host__ __device__ __forceinline__
#else
#define RT_REFIT_HD inline
#endif

namespace rtamd {
namespace refit {

// scene_load.cpp's fmin_/fmax_ (glibc's fminf/fmaxf): a NaN operand yields the other one
RT_REFIT_HD float fmin_(float a, float b) { if (a != a) return b; if (b != b) return a; return (b < a) ? b : a; }
RT_REFIT_HD float fmax_(float a, float b) { if (a != a) return b; if (b != b) return a; return (b > a) ? b : a; }

struct Box { rt_vec3 lo, hi; };

RT_REFIT_HD Box empty_box() { return {{1e30f, 1e30f, 1e30f}, {-1e30f, -1e30f, -1e30f}}; }
RT_REFIT_HD void grow(Box &b, rt_vec3 p) {
    b.lo = {fmin_(b.lo.x, p.x), fmin_(b.lo.y, p.y), fmin_(b.lo.z, p.z)};
    b.hi = {fmax_(b.hi.x, p.x), fmax_(b.hi.y, p.y), fmax_(b.hi.z, p.z)};
}
RT_REFIT_HD void grow(Box &b, const Box &o) {
    b.lo = {fmin_(b.lo.x, o.lo.x), fmin_(b.lo.y, o.lo.y), fmin_(b.lo.z, o.lo.z)};
    b.hi = {fmax_(b.hi.x, o.hi.x), fmax_(b.hi.y, o.hi.y), fmax_(b.hi.z, o.hi.z)};
}

// v: {a.xyz, b.xyz, c.xyz}
RT_REFIT_HD Box triangle_box(const float *v) {
    Box b = empty_box();
    grow(b, rt_vec3{v[0], v[1], v[2]});
    grow(b, rt_vec3{v[3], v[4], v[5]});
    grow(b, rt_vec3{v[6], v[7], v[8]});
    return b;
}

RT_REFIT_HD rt_triangle triangle_record(const float *v) {
    rt_triangle t;
    t.p1 = {v[0], v[1], v[2]};
    t.p2p1 = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
    t.p3p1 = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
    const rt_vec3 a = t.p3p1, b = t.p2p1;
    const rt_vec3 n{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
    const float s = 1.0f / sqrtf(n.x * n.x + n.y * n.y + n.z * n.z);
    t.normal = {s * n.x, s * n.y, s * n.z};
    return t;
}

}  // namespace refit
}  // namespace rtamd
