// Packed mesh batches, shared by the mesh kernels (mesh_in.hip, mesh_data.hip, render.hip, and mesh_rows.h for mesh_ops.hip and
// mesh_simplify.hip): the rows of a mesh in `offsets` and its triangles.
#pragma once
#include "common.h"

namespace pcd {

// mesh b of a packed batch as offsets[b * 2 .. b * 2 + 3] give it: first vertex row, first face row and the two row counts, unchecked.  What
// counts as an empty mesh differs from kernel to kernel and stays with the caller.
struct MeshRows { int64_t v0, f0, nv, nf; };

template <typename Index>                                      // int, or int64_t where b * 2 + 3 may pass 2^31
__device__ __forceinline__ MeshRows mesh_rows(const int64_t* __restrict__ offsets, Index b) {
    MeshRows m;
    m.v0 = offsets[b * 2];
    m.f0 = offsets[b * 2 + 1];
    m.nv = offsets[b * 2 + 2] - m.v0;
    m.nf = offsets[b * 2 + 3] - m.f0;
    return m;
}

#pragma clang fp contract(off)
struct MinTri {
    float ax, ay, az, bx, by, bz, cx, cy, cz;                  // index coordinates p = (v - lo) * inv_pitch, per component
    bool ok;                                                   // all three indices inside the mesh's vertex rows
};

__device__ __forceinline__ MinTri min_load_tri(const float* __restrict__ v, const int32_t* __restrict__ f, int t, int64_t nv, float lo, float ip) {
    MinTri q;
    const int i0 = f[(int64_t)t * 3], i1 = f[(int64_t)t * 3 + 1], i2 = f[(int64_t)t * 3 + 2];
    q.ok = (unsigned long long)i0 < (unsigned long long)nv && (unsigned long long)i1 < (unsigned long long)nv &&
           (unsigned long long)i2 < (unsigned long long)nv && i0 >= 0 && i1 >= 0 && i2 >= 0;
    q.ax = q.ay = q.az = q.bx = q.by = q.bz = q.cx = q.cy = q.cz = 0.f;
    if (q.ok) {
        const float* a = v + (int64_t)i0 * 3;
        const float* b = v + (int64_t)i1 * 3;
        const float* c = v + (int64_t)i2 * 3;
        q.ax = (a[0] - lo) * ip; q.ay = (a[1] - lo) * ip; q.az = (a[2] - lo) * ip;
        q.bx = (b[0] - lo) * ip; q.by = (b[1] - lo) * ip; q.bz = (b[2] - lo) * ip;
        q.cx = (c[0] - lo) * ip; q.cy = (c[1] - lo) * ip; q.cz = (c[2] - lo) * ip;
    }
    return q;
}
#pragma clang fp contract(fast)

// launch 1 of pcd_mesh_sample_points, also pcd_mesh_area_sums: the per-mesh inclusive running sums of the triangle areas into cdf (fp32 [sum F])
int mesh_area_scan_launch(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, float* cdf, hipStream_t stream);

}  // namespace pcd
