// mesh_ingest.h — launchers of csrc/mesh_ingest.hip's two kernels, called by the device build of a mesh
// (gpu_build_mesh, csrc/bvh_build.hip).  All pointers are device memory on the current device.
#pragma once
#include "rt_abi.h"

#include <hip/hip_runtime.h>

namespace rtamd {

// One triangle per lane: gathers the triangle's vertices (indices NULL = soup) into vrec (9 floats per triangle)
// and writes its box, centroid and input index into the build's blo/bhi/cen/idx.  err[0..2] (0xffffffff before the
// launch) take, by atomicMin, the smallest triangle with a vertex index outside [0, vertex_count), the smallest
// with a material index >= material_count, and 2 * i + c for the smallest triangle i with a non-finite coordinate
// (c = 0) or, its coordinates being finite, a non-finite centroid (c = 1).
void mesh_assemble_launch(const float *vertices, int32_t vertex_count, const int32_t *indices, const uint16_t *materials,
                          int32_t material_count, int32_t n, float4 *blo, float4 *bhi, float4 *cen, uint32_t *idx,
                          float *vrec, uint32_t *err, hipStream_t s);

// One output slot per lane: slot j takes source triangle idx[j]: its ray-tracing record, its material index
// (materials NULL = 0) and face_index[j] = idx[j].
void mesh_finalize_launch(const uint32_t *idx, const float *vrec, const uint16_t *materials, int32_t n,
                          rt_triangle *triangles, uint16_t *materials_out, int32_t *face_index, hipStream_t s);

}  // namespace rtamd
