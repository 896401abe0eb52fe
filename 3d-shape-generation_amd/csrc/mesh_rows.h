// Packed mesh batches on the device, shared by mesh_ops.hip and mesh_simplify.hip: the rows of a mesh in `offsets`, the valid-face test, the
// workgroup scan and the three-launch device scan.  Everything sits in the unnamed namespace: each including file gets its own copy.
#pragma once
#include "common.h"

namespace pcd {

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
    MoMesh m;
    m.v0 = offsets[b * 2];
    m.f0 = offsets[b * 2 + 1];
    const int64_t nv = offsets[b * 2 + 2] - m.v0, nf = offsets[b * 2 + 3] - m.f0;
    m.nv = nv > 0 && nv <= 0x7fffffff ? (int)nv : 0;
    m.nf = nf > 0 && nf <= 0x7fffffff ? (int)nf : 0;
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

// exclusive running sum of one int per thread over the workgroup's MO_WG threads, in thread order; total = the sum.  Barriers inside.
__device__ __forceinline__ int mo_block_scan(int x, int* wsum /* [MO_WAVES] */, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MO_WAVES; ++w) {
        const int s = wsum[w];
        if (w < wave) before += s;
        all += s;
    }
    total = all;
    return before + incl - x;
}

// ---------------------------------------------------------------------------------------------------------------- device scan
// out[i] = in[0] + ... + in[i - 1] for i < n, three launches: chunks of MO_WG, the chunk sums, the add.
__global__ __launch_bounds__(MO_WG) void mo_scan_chunks_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t n,
                                                               int32_t* __restrict__ partial) {
    __shared__ int wsum[MO_WAVES];
    const int64_t i = (int64_t)blockIdx.x * MO_WG + threadIdx.x;
    const int x = i < n ? in[i] : 0;
    int total;
    const int e = mo_block_scan(x, wsum, total);
    if (i < n) out[i] = e;
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(MO_WG) void mo_scan_partials_kernel(int32_t* __restrict__ partial, int chunks) {
    __shared__ int wsum[MO_WAVES];
    int base = 0;
    for (int c0 = 0; c0 < chunks; c0 += MO_WG) {
        const int i = c0 + threadIdx.x;
        const int x = i < chunks ? partial[i] : 0;
        int total;
        const int e = mo_block_scan(x, wsum, total);
        if (i < chunks) partial[i] = base + e;
        base += total;
    }
}

__global__ __launch_bounds__(MO_WG) void mo_scan_add_kernel(int32_t* __restrict__ out, int64_t n, const int32_t* __restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * MO_WG + threadIdx.x;
    if (i < n) out[i] += partial[blockIdx.x];
}

int mo_scan(const int32_t* in, int32_t* out, int64_t n, int32_t* partial, hipStream_t stream) {
    const int chunks = (int)ceil_div(n, MO_WG);
    hipLaunchKernelGGL(mo_scan_chunks_kernel, dim3(chunks), dim3(MO_WG), 0, stream, in, out, n, partial);
    PCD_CHECK_LAUNCH();
    hipLaunchKernelGGL(mo_scan_partials_kernel, dim3(1), dim3(MO_WG), 0, stream, partial, chunks);
    PCD_CHECK_LAUNCH();
    hipLaunchKernelGGL(mo_scan_add_kernel, dim3(chunks), dim3(MO_WG), 0, stream, out, n, partial);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

bool mo_sizes_ok(int batch, int64_t total_vertices, int64_t total_faces) {
    return batch > 0 && batch <= 65535 && total_vertices >= 0 && total_vertices < 0x7fffffff && total_faces >= 0 &&
           total_faces <= (0x7fffffff - MO_WG) / 6;
}

}  // namespace

#pragma clang fp contract(fast)

}  // namespace pcd
