// hemisphere_math.h — the sample generator of the hemisphere visibility queries (rt_query_hemisphere; rt_abi.h,
// DESIGN §18): the unit normal of a frame, the seed of a work item and the sample direction of either mode.  Compiled
// by the kernels (csrc/hemisphere.hip) and by the host twin and rt_hemisphere_rays (csrc/cpu_query.hip), so both sides
// evaluate the same text.
#pragma once
#include "rt_abi.h"
#include "rt_device.h"

#pragma clang fp contract(off)

namespace rtamd {
namespace hemi {

using namespace rtd;

// n̂ of a frame's normal: rt_device.h's normalise, literally (a zero normal gives NaNs, an infinite one too).
RT_HD V3 unit_normal(V3 nrm) { return normalise(nrm); }

// w of work item (i, s) in uint32 arithmetic; base(point_offset, S) + i * S + s is the same number.
RT_HD uint32_t work_item(uint32_t point_offset, uint32_t i, uint32_t S, uint32_t s) { return (point_offset + i) * S + s; }
RT_HD uint32_t base(uint32_t point_offset, uint32_t S) { return point_offset * S; }

// The direction of work item w above the unit normal nh.
RT_HD V3 direction(V3 nh, uint32_t w, uint32_t seed, int32_t mode) {
    Rng rng = pcg_seed(w * 0x9E3779B1u + seed * 0x85EBCA6Bu);
    const V3 u = random_on_sphere(rng);
    if (mode == RT_HEMISPHERE_UNIFORM) return dot(u, nh) < 0 ? -u : u;
    const V3 v = nh + u;
    const float m = magsq(v);
    return !(m >= 0x1p-40f) ? nh : (1.0f / sqrtf(m)) * v;
}

// What the entry points refuse about params alone, and n * S; nullptr = fine.
inline const char *params_error(const rt_hemisphere_params *p, int32_t n) {
    if (!p) return "null params";
    if (p->samples < 1 || p->samples > RT_HEMISPHERE_MAX_SAMPLES) return "samples is outside 1..RT_HEMISPHERE_MAX_SAMPLES";
    if (p->mode != RT_HEMISPHERE_COSINE && p->mode != RT_HEMISPHERE_UNIFORM) return "unknown mode";
    if (n > 0 && (int64_t)n * p->samples > INT32_MAX) return "n * samples does not fit int32";
    return nullptr;
}

}  // namespace hemi
}  // namespace rtamd
