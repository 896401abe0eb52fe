// Packed mesh batches on the device, shared by mesh_ops.hip and mesh_simplify.hip: the rows of a mesh in `offsets` clamped to int, the
// valid-face test and the three-launch device scan (defined once, in mesh_ops.hip).  The rest sits in the unnamed namespace: each including
// file gets its own copy.  The workgroup scan is device_prims.h's block_scan_excl<MO_WAVES>.
#pragma once
#include "mesh_tri.h"

namespace pcd {

// out[i] = in[0] + ... + in[i - 1] for i < n, three launches: chunks of 1024, the chunk sums, the add.  partial: ceil(n / 1024) ints.
int mo_scan(const int32_t* in, int32_t* out, int64_t n, int32_t* partial, hipStream_t stream);

#pragma clang fp contract(off)

namespace {

constexpr int MO_THREADS = 256;                                  // flat kernels: one thread per packed row
constexpr int MO_WG = 1024;                                      // one-workgroup-per-mesh kernels
constexpr int MO_WAVES = MO_WG / 64;

struct MoMesh {
    int64_t v0, f0;                                              // first vertex row, first face row
    int nv, nf;
};

__device__ __forceinline__ MoMesh mo_mesh(const int64_t* __restrict__ offsets, int b) {
    const MeshRows r = mesh_rows(offsets, b);
    MoMesh m;
    m.v0 = r.v0;
    m.f0 = r.f0;
    m.nv = r.nv > 0 && r.nv <= 0x7fffffff ? (int)r.nv : 0;
    m.nf = r.nf > 0 && r.nf <= 0x7fffffff ? (int)r.nf : 0;
    return m;
}

// the mesh that holds packed row `row` of column col (0 vertices, 1 faces): the last b with offsets[b][col] <= row; at most 32 halvings
__device__ __forceinline__ int mo_find(const int64_t* __restrict__ offsets, int batch, int64_t row, int col) {
    int lo = 0, hi = batch - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid * 2 + col] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// face t of a mesh: valid iff the three indices are rows of the mesh and pairwise different
__device__ __forceinline__ bool mo_face(const int32_t* __restrict__ f, int t, int nv, int& a, int& b, int& c) {
    a = f[(int64_t)t * 3];
    b = f[(int64_t)t * 3 + 1];
    c = f[(int64_t)t * 3 + 2];
    return (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv && a != b && b != c && a != c;
}

bool mo_sizes_ok(int batch, int64_t total_vertices, int64_t total_faces) {
    return batch > 0 && batch <= 65535 && total_vertices >= 0 && total_vertices < 0x7fffffff && total_faces >= 0 &&
           total_faces <= (0x7fffffff - MO_WG) / 6;
}

}  // namespace

#pragma clang fp contract(fast)

}  // namespace pcd
