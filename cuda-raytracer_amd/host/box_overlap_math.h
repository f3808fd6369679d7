// box_overlap_math.h — the box-overlap definition (include/rt_abi.h), shared by its host twin
// (csrc/cpu_query.hip) and the gfx950 kernel (csrc/box_overlap.hip) so both evaluate one text.
//
// float32 throughout, each operation rounded once, no contraction.  A query is an axis-aligned box (lo, hi); a node
// box meets it by six comparisons, a triangle by a 13-axis separating-axis test on the record's own vertices
// (p1, p1 + e1, p1 + e2), a sphere's surface by the nearest and the farthest point of the box.  Every separating
// comparison is strict: a NaN never separates, and a zero axis projects everything to 0 and never separates.
// tests/overlap_ref.py restates this file operation for operation.
#pragma once
#include "closest_point_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rtamd {
namespace ov {

// All six numbers finite and lo <= hi on every axis.
RT_CP_HD bool valid_box(rt_vec3 lo, rt_vec3 hi) {
    return cp::finite3(lo) && cp::finite3(hi) && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
}

// Closed: touching boxes meet.  Comparisons only; an empty-box sentinel (lo > hi) meets nothing finite.
RT_CP_HD bool boxes_meet(rt_vec3 nlo, rt_vec3 nhi, rt_vec3 qlo, rt_vec3 qhi) {
    return nlo.x <= qhi.x && qlo.x <= nhi.x && nlo.y <= qhi.y && qlo.y <= nhi.y && nlo.z <= qhi.z && qlo.z <= nhi.z;
}

RT_CP_HD float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
RT_CP_HD float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

RT_CP_HD rt_vec3 vertex(rt_vec3 p1, rt_vec3 e) { return {p1.x + e.x, p1.y + e.y, p1.z + e.z}; }

// Axes 1-3, the box's own: the triangle's extent on each coordinate against [lo, hi].
RT_CP_HD bool box_axes_separate(rt_vec3 v0, rt_vec3 v1, rt_vec3 v2, rt_vec3 lo, rt_vec3 hi) {
    const bool sx = min3(v0.x, v1.x, v2.x) > hi.x || max3(v0.x, v1.x, v2.x) < lo.x;
    const bool sy = min3(v0.y, v1.y, v2.y) > hi.y || max3(v0.y, v1.y, v2.y) < lo.y;
    const bool sz = min3(v0.z, v1.z, v2.z) > hi.z || max3(v0.z, v1.z, v2.z) < lo.z;
    return sx || sy || sz;
}

// Axis 4, the triangle's plane: m = e1 x e2 (not the stored unit normal), the plane's offset against the box's
// interval on m.
RT_CP_HD bool normal_axis_separates(rt_vec3 v0, rt_vec3 e1, rt_vec3 e2, rt_vec3 lo, rt_vec3 hi) {
    const rt_vec3 m = {e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
    const float s = cp::dot(m, v0);
    const float ax = m.x * lo.x, bx = m.x * hi.x, ay = m.y * lo.y, by = m.y * hi.y, az = m.z * lo.z, bz = m.z * hi.z;
    const float bmin = (fminf(ax, bx) + fminf(ay, by)) + fminf(az, bz);
    const float bmax = (fmaxf(ax, bx) + fmaxf(ay, by)) + fmaxf(az, bz);
    return s < bmin || s > bmax;
}

// One of axes 5-13, a = edge x unit_i: its two non-zero components (a1 on coordinate c1, a2 on coordinate c2).  The
// arguments are the three vertices' and the box's coordinates c1 and c2.
RT_CP_HD bool edge_axis_separates(float a1, float a2, float p0, float q0, float p1, float q1, float p2, float q2, float lo1,
                                  float hi1, float lo2, float hi2) {
    const float t0 = a1 * p0 + a2 * q0, t1 = a1 * p1 + a2 * q1, t2 = a1 * p2 + a2 * q2;
    const float b1l = a1 * lo1, b1h = a1 * hi1, b2l = a2 * lo2, b2h = a2 * hi2;
    const float bmin = fminf(b1l, b1h) + fminf(b2l, b2h);
    const float bmax = fmaxf(b1l, b1h) + fmaxf(b2l, b2h);
    return min3(t0, t1, t2) > bmax || max3(t0, t1, t2) < bmin;
}

// The three axes of one edge f, i = x, y, z in that order: f x unit_x = (0, f.z, -f.y), f x unit_y = (-f.z, 0, f.x),
// f x unit_z = (f.y, -f.x, 0).
RT_CP_HD bool edge_axes_separate(rt_vec3 f, rt_vec3 v0, rt_vec3 v1, rt_vec3 v2, rt_vec3 lo, rt_vec3 hi) {
    const bool sx = edge_axis_separates(f.z, -f.y, v0.y, v0.z, v1.y, v1.z, v2.y, v2.z, lo.y, hi.y, lo.z, hi.z);
    const bool sy = edge_axis_separates(-f.z, f.x, v0.x, v0.z, v1.x, v1.z, v2.x, v2.z, lo.x, hi.x, lo.z, hi.z);
    const bool sz = edge_axis_separates(f.y, -f.x, v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, lo.x, hi.x, lo.y, hi.y);
    return sx || sy || sz;
}

// Axes 4-13: the plane, then the edges e1, e2 and e2 - e1.
RT_CP_HD bool tail_axes_separate(rt_vec3 v0, rt_vec3 v1, rt_vec3 v2, rt_vec3 e1, rt_vec3 e2, rt_vec3 lo, rt_vec3 hi) {
    const rt_vec3 e3 = cp::sub(e2, e1);
    return normal_axis_separates(v0, e1, e2, lo, hi) || edge_axes_separate(e1, v0, v1, v2, lo, hi) ||
           edge_axes_separate(e2, v0, v1, v2, lo, hi) || edge_axes_separate(e3, v0, v1, v2, lo, hi);
}

// Triangle (p1, e1 = p2 - p1, e2 = p3 - p1) against the box: a member iff none of the 13 axes separates.
RT_CP_HD bool triangle_meets(rt_vec3 p1, rt_vec3 e1, rt_vec3 e2, rt_vec3 lo, rt_vec3 hi) {
    const rt_vec3 v1 = vertex(p1, e1), v2 = vertex(p1, e2);
    return !box_axes_separate(p1, v1, v2, lo, hi) && !tail_axes_separate(p1, v1, v2, e1, e2, lo, hi);
}

// The sphere's surface against the box: the box's nearest point is within r and its farthest corner is not inside.
RT_CP_HD bool sphere_meets(rt_vec3 c, float r, rt_vec3 lo, rt_vec3 hi) {
    const float near2 = cp::box2(c, lo, hi);
    const float fx = fmaxf(fabsf(c.x - lo.x), fabsf(hi.x - c.x));
    const float fy = fmaxf(fabsf(c.y - lo.y), fabsf(hi.y - c.y));
    const float fz = fmaxf(fabsf(c.z - lo.z), fabsf(hi.z - c.z));
    const float far2 = (fx * fx + fy * fy) + fz * fz;
    const float r2 = r * r;
    return near2 <= r2 && far2 >= r2;
}

}  // namespace ov
}  // namespace rtamd
