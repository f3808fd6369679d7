// closest_point_math.h — the closest-point definition (include/rt_abi.h), shared by its host twin
// (csrc/cpu_query.hip) and the gfx950 kernel (csrc/closest_point.hip) so both evaluate one text.
//
// float32 throughout, each operation rounded once, no contraction.  The triangle rule is Ericson's region test
// on the record's own edges in predicated form: every quantity is computed, the seven regions are tested in the
// definition's order and the first that applies selects (u, v).  The four regions that divide share one
// division: the selected numerator over the selected denominator is the definition's own quotient.
#pragma once
#include "rt_abi.h"

#include <math.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#define RT_CP_HD __host__ __device__ __forceinline__
#else
#define RT_CP_HD inline
#endif

namespace rtamd {
namespace cp {

struct Near {
    float dist2, u, v;
    rt_vec3 point;
};

RT_CP_HD float dot(rt_vec3 a, rt_vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RT_CP_HD rt_vec3 sub(rt_vec3 a, rt_vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

// max_dist R -> the squared bound: R * R for 0 <= R <= 1e18, -1 (nothing qualifies) for R < 0, otherwise
// (larger, +inf, NaN) +inf
RT_CP_HD float bound2(float r) {
    if (r < 0.0f) return -1.0f;
    return r <= 1e18f ? r * r : INFINITY;
}

RT_CP_HD bool finite3(rt_vec3 p) { return fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY; }

// The state (best2, best) takes primitive i at dist2 iff this holds; a NaN dist2 never does.
RT_CP_HD bool accepts(float dist2, int32_t i, float best2, int32_t best) {
    return dist2 < best2 || (dist2 == best2 && i < best);
}

// Range queries (rt_query_nearest_k): the bound b2 is held, a primitive at dist2 is a member iff this
// holds (a NaN dist2 never is), and so is a node whose box2 passes `!(box2 > b2)`.
RT_CP_HD bool within(float dist2, float b2) { return dist2 <= b2; }

// Their order: the key (dist2's bits as uint32, index), ascending.  A member's dist2 is a sum of squares, >= +0 and
// not NaN, so unsigned order is numeric order.
RT_CP_HD uint32_t key_bits(float dist2) {
    uint32_t u;
    __builtin_memcpy(&u, &dist2, sizeof(u));
    return u;
}
RT_CP_HD bool key_less(uint32_t ka, int32_t ia, uint32_t kb, int32_t ib) { return ka < kb || (ka == kb && ia < ib); }

// (u, v) of the point of triangle (p1, e1 = p2 - p1, e2 = p3 - p1) nearest to p
RT_CP_HD void triangle_uv(rt_vec3 p, rt_vec3 p1, rt_vec3 e1, rt_vec3 e2, float &u, float &v) {
    const rt_vec3 ap = sub(p, p1), bp = sub(ap, e1), cq = sub(ap, e2);
    const float d1 = dot(e1, ap), d2 = dot(e2, ap), d3 = dot(e1, bp), d4 = dot(e2, bp), d5 = dot(e1, cq), d6 = dot(e2, cq);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    const bool rA = d1 <= 0 && d2 <= 0;
    const bool rB = d3 >= 0 && d4 <= d3;
    const bool rAB = vc <= 0 && d1 >= 0 && d3 <= 0;
    const bool rC = d6 >= 0 && d5 <= d6;
    const bool rAC = vb <= 0 && d2 >= 0 && d6 <= 0;
    const bool rBC = va <= 0 && d43 >= 0 && d56 >= 0;
    // the quotient of the first dividing region in the order AB, AC, BC, face
    float num = 1.0f, den = (va + vb) + vc;
    num = rBC ? d43 : num;  den = rBC ? d43 + d56 : den;
    num = rAC ? d2 : num;   den = rAC ? d2 - d6 : den;
    num = rAB ? d1 : num;   den = rAB ? d1 - d3 : den;
    const float q = num / den;
    float uu = vb * q, vv = vc * q;             // face
    uu = rBC ? 1.0f - q : uu;  vv = rBC ? q : vv;
    uu = rAC ? 0.0f : uu;      vv = rAC ? q : vv;
    uu = rC ? 0.0f : uu;       vv = rC ? 1.0f : vv;
    uu = rAB ? q : uu;         vv = rAB ? 0.0f : vv;
    uu = rB ? 1.0f : uu;       vv = rB ? 0.0f : vv;
    uu = rA ? 0.0f : uu;       vv = rA ? 0.0f : vv;
    u = uu;
    v = vv;
}

RT_CP_HD Near triangle(rt_vec3 p, rt_vec3 p1, rt_vec3 e1, rt_vec3 e2) {
    Near n;
    triangle_uv(p, p1, e1, e2, n.u, n.v);
    n.point = {(p1.x + n.u * e1.x) + n.v * e2.x, (p1.y + n.u * e1.y) + n.v * e2.y, (p1.z + n.u * e1.z) + n.v * e2.z};
    const rt_vec3 w = sub(p, n.point);
    n.dist2 = dot(w, w);
    return n;
}

// squared distance to the sphere's surface alone (the traversal's test)
RT_CP_HD float sphere_dist2(rt_vec3 p, rt_vec3 c, float r, rt_vec3 &w, float &len) {
    w = sub(p, c);
    len = sqrtf(dot(w, w));
    const float g = len - r;
    return g * g;
}

RT_CP_HD Near sphere(rt_vec3 p, rt_vec3 c, float r) {
    Near n;
    rt_vec3 w;
    float len;
    n.dist2 = sphere_dist2(p, c, r, w, len);
    n.u = n.v = 0.0f;
    const float s = r / len;
    n.point = {c.x + s * w.x, c.y + s * w.y, c.z + s * w.z};
    if (len == 0) n.point = {c.x + r, c.y + 0.0f, c.z + 0.0f};
    return n;
}

// squared distance from p to the box (lo, hi); 0 inside
RT_CP_HD float box2(rt_vec3 p, rt_vec3 lo, rt_vec3 hi) {
    const float qx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
    const float qy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
    const float qz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
    return (qx * qx + qy * qy) + qz * qz;
}

}  // namespace cp
}  // namespace rtamd
