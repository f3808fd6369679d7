// mesh_ingest.hip — the two ends of the device build of a mesh given as device arrays
// (rt_scene_from_mesh_device); the level loop between them is csrc/bvh_build.hip's.
//
//   * mesh_assemble_kernel stands in for the loader's `triangle` lines, its validation and the build's host
//     pre-pass: per triangle it bounds-checks the three indices (before any vertex load: a triangle with a bad
//     index loads nothing), gathers the vertices, forms the loader's centroid (1/3f) * ((a + b) + c) and the box
//     as the reference grows it (refit::triangle_box: the 1e30 start, the first of equal values), and writes the
//     build's blo/bhi/cen/idx and a 36-byte vertex record.  What the loader would refuse is reported as the
//     smallest offending triangle per rule, by atomicMin on three global words, so the report does not depend on
//     the schedule.
//   * mesh_finalize_kernel stands in for the host's permutation and its last loop: slot j gathers source triangle
//     idx[j] and writes refit::triangle_record of its vertices -- the text the loader's last loop evaluates, no
//     contraction, IEEE divide and sqrt -- with the permuted material index and face_index[j].
#include "mesh_ingest.h"
#include "bvh_refit_math.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

namespace rf = rtamd::refit;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;        // 8 workgroups per CU; the loops are grid-stride

__device__ __forceinline__ bool finite_bits(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(kThreads) void mesh_assemble_kernel(
    const float *__restrict__ vertices, int32_t vertex_count, const int32_t *__restrict__ indices,
    const uint16_t *__restrict__ materials, int32_t material_count, int32_t n, float4 *__restrict__ blo,
    float4 *__restrict__ bhi, float4 *__restrict__ cen, uint32_t *__restrict__ idx, float *__restrict__ vrec,
    uint32_t *__restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        if (materials && (int32_t)materials[i] >= material_count) atomicMin(&err[1], (uint32_t)i);
        int64_t q[3] = {3 * i, 3 * i + 1, 3 * i + 2};
        if (indices) {
            const int32_t a = indices[3 * i], b = indices[3 * i + 1], c = indices[3 * i + 2];
            q[0] = a; q[1] = b; q[2] = c;
        }
        // a soup's positions are checked like indices: nothing is loaded from outside [0, vertex_count)
        if (q[0] < 0 || q[0] >= vertex_count || q[1] < 0 || q[1] >= vertex_count || q[2] < 0 || q[2] >= vertex_count) {
            atomicMin(&err[0], (uint32_t)i);
            continue;
        }
        float v[9];
        bool finite = true;
        for (int k = 0; k < 3; k++)
            for (int c = 0; c < 3; c++) {
                const float f = vertices[3 * q[k] + c];
                v[3 * k + c] = f;
                finite = finite && finite_bits(f);
            }
        const float third = 1.0f / 3.0f;
        const float cx = third * ((v[0] + v[3]) + v[6]), cy = third * ((v[1] + v[4]) + v[7]),
                    cz = third * ((v[2] + v[5]) + v[8]);
        if (!finite) atomicMin(&err[2], 2u * (uint32_t)i);
        else if (!(finite_bits(cx) && finite_bits(cy) && finite_bits(cz))) atomicMin(&err[2], 2u * (uint32_t)i + 1u);
        const rf::Box box = rf::triangle_box(v);
        blo[i] = make_float4(box.lo.x, box.lo.y, box.lo.z, 0.0f);
        bhi[i] = make_float4(box.hi.x, box.hi.y, box.hi.z, 0.0f);
        cen[i] = make_float4(cx, cy, cz, 0.0f);
        idx[i] = (uint32_t)i;
        for (int k = 0; k < 9; k++) vrec[9 * i + k] = v[k];
    }
}

__global__ __launch_bounds__(kThreads) void mesh_finalize_kernel(
    const uint32_t *__restrict__ idx, const float *__restrict__ vrec, const uint16_t *__restrict__ materials, int32_t n,
    rt_triangle *__restrict__ triangles, uint16_t *__restrict__ materials_out, int32_t *__restrict__ face_index) {
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < n; j += (int64_t)gridDim.x * kThreads) {
        const uint32_t src = idx[j];
        float v[9];
        for (int k = 0; k < 9; k++) v[k] = vrec[9 * (int64_t)src + k];
        const rt_triangle t = rf::triangle_record(v);
        float4 *out = reinterpret_cast<float4 *>(triangles + j);     // 48-byte records: three 16-byte stores
        out[0] = make_float4(t.p1.x, t.p1.y, t.p1.z, t.p2p1.x);
        out[1] = make_float4(t.p2p1.y, t.p2p1.z, t.p3p1.x, t.p3p1.y);
        out[2] = make_float4(t.p3p1.z, t.normal.x, t.normal.y, t.normal.z);
        materials_out[j] = materials ? materials[src] : (uint16_t)0;
        face_index[j] = (int32_t)src;
    }
}

int blocks_for(int32_t n) { return (int)std::min<int64_t>(kMaxBlocks, ((int64_t)n + kThreads - 1) / kThreads); }

}  // namespace

namespace rtamd {

void mesh_assemble_launch(const float *vertices, int32_t vertex_count, const int32_t *indices, const uint16_t *materials,
                          int32_t material_count, int32_t n, float4 *blo, float4 *bhi, float4 *cen, uint32_t *idx,
                          float *vrec, uint32_t *err, hipStream_t s) {
    hipLaunchKernelGGL(mesh_assemble_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, vertices, vertex_count, indices,
                       materials, material_count, n, blo, bhi, cen, idx, vrec, err);
}

void mesh_finalize_launch(const uint32_t *idx, const float *vrec, const uint16_t *materials, int32_t n,
                          rt_triangle *triangles, uint16_t *materials_out, int32_t *face_index, hipStream_t s) {
    hipLaunchKernelGGL(mesh_finalize_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, idx, vrec, materials, n,
                       triangles, materials_out, face_index);
}

}  // namespace rtamd
