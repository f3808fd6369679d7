// ray_filter_math.h — the per-ray filter of the filtered ray queries (rt_query_closest_filtered,
// rt_query_occluded_filtered; rt_abi.h): the interval's two ends, the eligibility test and the sphere
// test with a caller-chosen lower bound.  Compiled by the kernels (csrc/ray_filter.hip) and by the host twins
// (csrc/cpu_query.hip), so both sides evaluate the same text.
#pragma once
#include "rt_device.h"

#pragma clang fp contract(off)

namespace rtamd {
namespace rf {

using namespace rtd;

constexpr uint32_t kAllBits = 0xFFFFFFFFu;   // the word of a primitive without masks, and of a ray without one

// lo of a caller's tmin: NaN, negative and small values give kEps (the unfiltered calls' bound), +inf stays.
RT_HD float lower(float tmin) { return tmin > kEps ? tmin : kEps; }
// B of a caller's tmax: rt_query_occluded's rule.
RT_HD float upper(float tmax) { return tmax <= 1e30f ? tmax : 1e30f; }

// eligible(p) for a ray with skip index `skip` and mask word `rm`, m = the primitive's mask word.
RT_HD bool eligible(int32_t p, int32_t skip, uint32_t m, uint32_t rm) { return p != skip && (m & rm) != 0; }

// ray_sphere (rt_device.h, scene.cu:340-371) with kEps replaced by lo: the near root if it lies in [lo, closest),
// otherwise the far root under the same test -- so a lo between the two roots returns the far one.  With lo = kEps
// this is ray_sphere bit for bit.
RT_HD bool ray_sphere_lo(V3 o, V3 d, V3 c, float radius, float lo, float closest, float &t) {
    const V3 off = c - o;
    const float mhb = dot(off, d);
    const float qc = magsq(off) - radius * radius;
    const float qd = mhb * mhb - qc;
    if (qd < 0) return false;
    const float hs = sqrtf(qd);
    t = mhb - hs;
    if (t < closest && !(t < lo)) return true;
    t = mhb + hs;
    return t < closest && !(t < lo);
}

}  // namespace rf
}  // namespace rtamd
