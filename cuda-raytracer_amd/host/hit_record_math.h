// hit_record_math.h — the hit-record definition (include/rt_abi.h), shared by its host twin
// (host/scene_hit.cpp) and the gfx950 egest kernel (csrc/rt_query.hip) so both evaluate one text.
//
// Given a ray (o, d) and its closest hit (t, index), the record is what the reference forms after the
// traversal (scene.cu:398-418) plus the barycentrics its triangle test computes and drops
// (scene.cu:166-183): float32 throughout, each operation rounded once, no contraction.  The normal is the
// stored one, never flipped; front_face tells the side.
#pragma once
#include "rt_abi.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#define RT_HIT_HD __host__ __device__ __forceinline__
#else
#define RT_HIT_HD inline
#endif

namespace rtamd {
namespace hit {

struct Record {
    float u, v;
    rt_vec3 normal, position;
    int32_t material;
    uint8_t front_face;
};

RT_HIT_HD float dot(rt_vec3 a, rt_vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RT_HIT_HD rt_vec3 cross(rt_vec3 a, rt_vec3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// index < 0: every field +0, material -1
RT_HIT_HD Record miss() { return {0.0f, 0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, -1, 0}; }

// o + t * d (scene.cu:398)
RT_HIT_HD rt_vec3 position(rt_vec3 o, rt_vec3 d, float t) { return {o.x + t * d.x, o.y + t * d.y, o.z + t * d.z}; }

RT_HIT_HD uint8_t front_face(rt_vec3 normal, rt_vec3 d) { return dot(normal, d) < 0 ? 1 : 0; }   // scene.cu:418

// Triangle record (p1, e1 = p2 - p1, e2 = p3 - p1, normal): u and v are ray_triangle's (scene.cu:166-183),
// the hit lies at p1 + u e1 + v e2.  `material` is left to the caller.
RT_HIT_HD Record triangle(rt_vec3 o, rt_vec3 d, float t, rt_vec3 p1, rt_vec3 e1, rt_vec3 e2, rt_vec3 normal) {
    Record r = miss();
    const rt_vec3 h = cross(d, e2);
    const float a = dot(h, e1);
    const float f = 1 / a;
    const rt_vec3 s = {o.x - p1.x, o.y - p1.y, o.z - p1.z};
    r.u = dot(s, h) * f;
    const rt_vec3 q = cross(s, e1);
    r.v = dot(d, q) * f;
    r.normal = normal;
    r.position = position(o, d, t);
    r.front_face = front_face(normal, d);
    return r;
}

// Sphere: normal = (1 / radius) * (position - center) (scene.cu:405), uv = (+0, +0)
RT_HIT_HD Record sphere(rt_vec3 o, rt_vec3 d, float t, rt_vec3 center, float radius) {
    Record r = miss();
    r.position = position(o, d, t);
    const float inv = 1 / radius;
    r.normal = {inv * (r.position.x - center.x), inv * (r.position.y - center.y), inv * (r.position.z - center.z)};
    r.front_face = front_face(r.normal, d);
    return r;
}

}  // namespace hit
}  // namespace rtamd
