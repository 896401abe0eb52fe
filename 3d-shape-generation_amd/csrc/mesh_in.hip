// K13: triangle meshes in (DESIGN.md "Mesh input"; include/pcd_hip.h pcd_mesh_voxelize, pcd_mesh_sample_points): the inverse of mesh.hip.
//
//   voxelize: one workgroup per mesh.  Integer accumulators per mesh -- a bit per node for the surface, an int32 event per node for the interior --
//             in LDS up to R = 32 (128 KB + 4 KB of the CU's 160 KB), in the workspace above.  Triangles are taken 1024 at a time; a block scan of
//             their column counts spreads the (triangle, column of its bounding box) items evenly over the threads, so 3000 small triangles and
//             12 large ones keep the workgroup equally busy.  An item walks the column's nodes with the 13-axis triangle / cube test and places the
//             triangle's winding event by a binary search on the plane predicate.  One pass down every column turns events into windings and
//             writes the fp32 grid.  Integer atomics only: bitwise repeatable and independent of the rest of the batch.
//   sample:   areas and their inclusive running sum per mesh (one workgroup per mesh, fixed scan tree), then one thread per output point.
//
// The predicates are fp32 without contraction and without division: where every intermediate value is exactly representable they decide ties as
// the float64 statement (tests/mesh_in_statement.py) does.
#include "common.h"
#include "mesh_tri.h"
#include <cmath>

namespace pcd {

#pragma clang fp contract(off)

constexpr int MIN_THREADS = 1024;
constexpr int MIN_WAVES = MIN_THREADS / 64;
constexpr int MIN_LDS_R = 32;                                  // accumulators of a grid up to this extent live in LDS
constexpr int MIN_MAX_R = 64;

// nodes i of one axis whose closed unit interval [i - 1/2, i + 1/2] meets [mn, mx], cut to [0, r - 1]: first node and count (0 for none, also
// for NaN: fmaxf / fminf drop it and the clamp bounds the conversion)
__device__ __forceinline__ void min_axis_range(float a, float b, float c, int r, int& first, int& count) {
    const float mn = fminf(fminf(a, b), c), mx = fmaxf(fmaxf(a, b), c);
    const float l = fminf(fmaxf(ceilf(mn - 0.5f), 0.f), (float)r);
    const float h = fminf(fmaxf(floorf(mx + 0.5f), -1.f), (float)(r - 1));
    first = (int)l;
    count = max((int)h - first + 1, 0);
    if (!(mn <= mx)) count = 0;
}

__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// one separating-axis candidate: projections p0, p1, p2 of the vertices, radius rad of the cube; true = separated (touching is not)
__device__ __forceinline__ bool min_separates(float p0, float p1, float p2, float rad) {
    return min3(p0, p1, p2) > rad || max3(p0, p1, p2) < -rad;
}

// does the triangle meet the closed cube of side 1 centred on (x, y, z)?  13 axes: the cube's 3 normals, the triangle's normal n = (b - a) x (c - a),
// and e x X, e x Y, e x Z for the edges e = b - a, c - b, a - c.  A zero axis (a triangle of zero area, a zero edge) projects everything to 0 and
// separates nothing, so a segment or a point is tested as what it is.
__device__ __forceinline__ bool min_tri_meets_cube(const MinTri& q, float x, float y, float z) {
    const float ax = q.ax - x, ay = q.ay - y, az = q.az - z;
    const float bx = q.bx - x, by = q.by - y, bz = q.bz - z;
    const float cx = q.cx - x, cy = q.cy - y, cz = q.cz - z;
    if (min_separates(ax, bx, cx, 0.5f) || min_separates(ay, by, cy, 0.5f) || min_separates(az, bz, cz, 0.5f)) return false;
    const float ux = bx - ax, uy = by - ay, uz = bz - az;
    const float vx = cx - ax, vy = cy - ay, vz = cz - az;
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const float d = (nx * ax + ny * ay) + nz * az;
    const float rn = 0.5f * ((fabsf(nx) + fabsf(ny)) + fabsf(nz));
    if (d > rn || d < -rn) return false;
    const float ex[3] = {ux, cx - bx, ax - cx}, ey[3] = {uy, cy - by, ay - cy}, ez[3] = {uz, cz - bz, az - cz};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // e x X = (0, ez, -ey), e x Y = (-ez, 0, ex), e x Z = (ey, -ex, 0)
        if (min_separates(ez[k] * ay - ey[k] * az, ez[k] * by - ey[k] * bz, ez[k] * cy - ey[k] * cz, 0.5f * (fabsf(ez[k]) + fabsf(ey[k])))) return false;
        if (min_separates(ex[k] * az - ez[k] * ax, ex[k] * bz - ez[k] * bx, ex[k] * cz - ez[k] * cx, 0.5f * (fabsf(ex[k]) + fabsf(ez[k])))) return false;
        if (min_separates(ey[k] * ax - ex[k] * ay, ey[k] * bx - ex[k] * by, ey[k] * cx - ex[k] * cy, 0.5f * (fabsf(ey[k]) + fabsf(ex[k])))) return false;
    }
    return true;
}

// edge function of the directed edge p -> q (coordinates relative to the sample) with the top-left rule: the sample is taken at (+eps, +eps^2)
__device__ __forceinline__ bool min_edge_covers(float px, float py, float qx, float qy) {
    const float e = px * qy - py * qx;
    const float dx = qx - px, dy = qy - py;
    return e > 0.f || (e == 0.f && (dy < 0.f || (dy == 0.f && dx > 0.f)));
}

// Interior event of triangle q over the column (y, x): 0 when its projection does not cover the point or has zero area; otherwise sign(n_z), with
// `nodes` = how many nodes z = 0 .. nodes - 1 lie strictly below the plane (z* > z  <=>  sign(n_z) n . (a - p) > 0, monotone in z also in fp32)
__device__ __forceinline__ int min_column_event(const MinTri& q, float x, float y, int r, int& nodes) {
    const float ux = q.bx - q.ax, uy = q.by - q.ay, uz = q.bz - q.az;
    const float vx = q.cx - q.ax, vy = q.cy - q.ay, vz = q.cz - q.az;
    const float nz = ux * vy - uy * vx;
    if (!(nz != 0.f) || nz != nz) return 0;
    const float ax = q.ax - x, ay = q.ay - y;
    float bx = q.bx - x, by = q.by - y, cx = q.cx - x, cy = q.cy - y;
    if (nz < 0.f) { float t = bx; bx = cx; cx = t; t = by; by = cy; cy = t; }
    if (!(min_edge_covers(ax, ay, bx, by) && min_edge_covers(bx, by, cx, cy) && min_edge_covers(cx, cy, ax, ay))) return 0;
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz;
    const float t0 = nx * ax + ny * ay;
    const float s = nz > 0.f ? 1.f : -1.f;
    int l = 0, h = r;
    while (l < h) {
        const int m = (l + h) >> 1;
        if (s * (t0 + nz * (q.az - (float)m)) > 0.f) l = m + 1; else h = m;
    }
    nodes = l;
    return nz > 0.f ? 1 : -1;
}

static inline size_t min_bit_words(int r) { return ((size_t)r * r * r + 31) / 32; }
static inline size_t min_acc_bytes(int r) { return align_up((size_t)r * r * r * sizeof(int32_t) + min_bit_words(r) * sizeof(uint32_t)); }

// mode: 0 surface, 1 interior, 2 solid
template <bool IN_LDS>
__global__ __launch_bounds__(MIN_THREADS) void mesh_voxelize_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                     const int64_t* __restrict__ offsets, int r, float lo, float ip, int mode,
                                                                     char* workspace, size_t acc_bytes, float* __restrict__ vox) {
    extern __shared__ __attribute__((aligned(16))) char min_lds[];
    __shared__ int prefix[MIN_THREADS];
    __shared__ int wsum[MIN_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const MeshRows m = mesh_rows(offsets, b);
    const int64_t nv = m.nv;
    const int nf = nv > 0 && m.nf > 0 && m.nf <= 0x7fffffff ? (int)m.nf : 0;
    const float* v = vertices + m.v0 * 3;
    const int32_t* f = faces + m.f0 * 3;
    const int n3 = r * r * r, nw = (n3 + 31) >> 5;
    int* ev;
    unsigned* bits;
    if (IN_LDS) {
        ev = (int*)min_lds;
    } else {
        ev = (int*)(workspace + (size_t)b * acc_bytes);
    }
    bits = (unsigned*)(ev + n3);
    for (int i = tid; i < n3 + nw; i += MIN_THREADS) ev[i] = 0;               // events and bits are one run of words
    __syncthreads();
    const bool want_surface = mode != 1, want_interior = mode != 0;

    for (int c0 = 0; c0 < nf; c0 += MIN_THREADS) {
        int mine = 0;
        if (c0 + tid < nf) {
            const MinTri q = min_load_tri(v, f, c0 + tid, nv, lo, ip);
            if (q.ok) {
                int x0, xn, y0, yn;
                min_axis_range(q.ax, q.bx, q.cx, r, x0, xn);
                min_axis_range(q.ay, q.by, q.cy, r, y0, yn);
                mine = xn * yn;
            }
        }
        int total;
        prefix[tid] = block_scan_incl<MIN_WAVES>(mine, wsum, total);
        __syncthreads();
        for (int item = tid; item < total; item += MIN_THREADS) {
            const int l = first_above(prefix, MIN_THREADS - 1, item);         // the first triangle whose inclusive sum exceeds the item
            const MinTri q = min_load_tri(v, f, c0 + l, nv, lo, ip);          // l has items, so c0 + l < nf and q.ok
            int x0, xn, y0, yn, z0, zn;
            min_axis_range(q.ax, q.bx, q.cx, r, x0, xn);
            min_axis_range(q.ay, q.by, q.cy, r, y0, yn);
            min_axis_range(q.az, q.bz, q.cz, r, z0, zn);
            const int local = item - (l ? prefix[l - 1] : 0);
            if (xn <= 0 || local >= xn * yn) continue;                        // cannot happen: the counts above came from the same arithmetic
            const int y = y0 + local / xn, x = x0 + local % xn;
            const float fx = (float)x, fy = (float)y;
            if (want_surface) {
                for (int z = z0; z < z0 + zn; ++z) {
                    const int node = (z * r + y) * r + x;
                    const unsigned bit = 1u << (node & 31);
                    if (__hip_atomic_load(&bits[node >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) continue;
                    if (min_tri_meets_cube(q, fx, fy, (float)z)) atomicOr(&bits[node >> 5], bit);
                }
            }
            if (want_interior) {
                int nodes = 0;
                const int s = min_column_event(q, fx, fy, r, nodes);
                if (s != 0 && nodes > 0) atomicAdd(&ev[((nodes - 1) * r + y) * r + x], s);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    float* out = vox + (size_t)b * n3;
    for (int col = tid; col < r * r; col += MIN_THREADS) {
        int w = 0;
        for (int z = r - 1; z >= 0; --z) {
            const int node = z * r * r + col;
            w += __hip_atomic_load(&ev[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool surf = (__hip_atomic_load(&bits[node >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (node & 31)) & 1u;
            const bool on = (want_surface && surf) || (want_interior && w != 0);
            out[node] = on ? 1.f : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- sampling
__device__ __forceinline__ float min_tri_area(const float* __restrict__ v, const int32_t* __restrict__ f, int t, int64_t nv) {
    const MinTri q = min_load_tri(v, f, t, nv, 0.f, 1.f);
    if (!q.ok) return 0.f;
    const float ux = q.bx - q.ax, uy = q.by - q.ay, uz = q.bz - q.az;
    const float vx = q.cx - q.ax, vy = q.cy - q.ay, vz = q.cz - q.az;
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const float a = 0.5f * sqrtf((nx * nx + ny * ny) + nz * nz);
    return a == a && a <= 3.0e38f ? a : 0.f;                                  // a face with a non-finite area is never drawn
}

// cdf[f0 + i] = area_0 + ... + area_i of mesh b, added in a fixed tree: lanes of a wave, the 16 waves, then the chunks of 1024 in order.  The
// scan is block_scan_incl<MIN_WAVES, float> of device_prims.h written out: through the template the same 304 instructions come out in another
// order, and the launch measured 0.4 us slower than the parent's (profiles/mesh_family_isa.md).
__global__ __launch_bounds__(MIN_THREADS) void mesh_area_scan_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                      const int64_t* __restrict__ offsets, float* __restrict__ cdf) {
    __shared__ float wsum[MIN_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t v0 = offsets[b * 2], f0 = offsets[b * 2 + 1];
    const int64_t nv = offsets[b * 2 + 2] - v0, nf64 = offsets[b * 2 + 3] - f0;
    const int nf = nf64 > 0 && nf64 <= 0x7fffffff ? (int)nf64 : 0;
    const float* v = vertices + v0 * 3;
    const int32_t* f = faces + f0 * 3;
    float base = 0.f;
    for (int c0 = 0; c0 < nf; c0 += MIN_THREADS) {
        const int t = c0 + tid;
        float x = t < nf ? min_tri_area(v, f, t, nv) : 0.f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        if (wave == 0) {
            float s = lane < MIN_WAVES ? wsum[lane] : 0.f;
#pragma unroll
            for (int o = 1; o < MIN_WAVES; o <<= 1) {
                const float y = __shfl_up(s, o);
                if (lane >= o) s += y;
            }
            if (lane < MIN_WAVES) wsum[lane] = s;
        }
        __syncthreads();
        const float incl = base + ((wave ? wsum[wave - 1] : 0.f) + x);
        if (t < nf) cdf[f0 + t] = incl;
        base = base + wsum[MIN_WAVES - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void mesh_sample_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                           const int64_t* __restrict__ offsets, int n_points, uint64_t seed, uint64_t ctr0,
                                                           const float* __restrict__ u, const float* __restrict__ cdf,
                                                           float* __restrict__ points, float* __restrict__ normals, int32_t* __restrict__ face_index) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const MeshRows mr = mesh_rows(offsets, b);
    const int64_t v0 = mr.v0, f0 = mr.f0, nv = mr.nv, nf64 = mr.nf;
    const int64_t row = (int64_t)b * n_points + i;
    float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    int face = 0;
    if (nf64 > 0 && nf64 <= 0x7fffffff) {
        const int nf = (int)nf64;
        const float* v = vertices + v0 * 3;
        const int32_t* f = faces + f0 * 3;
        const float* c = cdf + f0;
        float u0, u1, u2;
        if (u != nullptr) {
            u0 = u[row * 3]; u1 = u[row * 3 + 1]; u2 = u[row * 3 + 2];
        } else {
            uint32_t w[4];
            philox_words4(ctr0 + (uint64_t)i, seed, w);
            u0 = (float)(w[0] >> 8) * (1.0f / 16777216.0f);
            u1 = (float)(w[1] >> 8) * (1.0f / 16777216.0f);
            u2 = (float)(w[2] >> 8) * (1.0f / 16777216.0f);
        }
        const float total = c[nf - 1];
        float s = 0.f, t = 0.f;                                                // total area 0: the first vertex of the first face
        if (total > 0.f) {
            const float target = u0 * total;
            int l = 0, h = nf - 1;                                             // the first face whose running sum exceeds the target (the last at most);
            while (l < h) {                                                    // first_above written out, as in mesh_data.hip, which draws the same bits
                const int m = (l + h) >> 1;
                if (c[m] > target) h = m; else l = m + 1;
            }
            face = l;
            s = sqrtf(fminf(fmaxf(u1, 0.f), 1.f));
            t = fminf(fmaxf(u2, 0.f), 1.f);
        }
        const MinTri q = min_load_tri(v, f, face, nv, 0.f, 1.f);
        if (q.ok) {
            const float wa = 1.f - s, wb = s * (1.f - t), wc = s * t;
            px = (wa * q.ax + wb * q.bx) + wc * q.cx;
            py = (wa * q.ay + wb * q.by) + wc * q.cy;
            pz = (wa * q.az + wb * q.bz) + wc * q.cz;
            const float ux = q.bx - q.ax, uy = q.by - q.ay, uz = q.bz - q.az;
            const float vx = q.cx - q.ax, vy = q.cy - q.ay, vz = q.cz - q.az;
            const float mx = uy * vz - uz * vy, my = uz * vx - ux * vz, mz = ux * vy - uy * vx;
            const float len = sqrtf((mx * mx + my * my) + mz * mz);
            if (len > 0.f && len <= 3.0e38f) { nx = mx / len; ny = my / len; nz = mz / len; }
        }
    }
    points[row * 3] = px; points[row * 3 + 1] = py; points[row * 3 + 2] = pz;
    if (normals != nullptr) { normals[row * 3] = nx; normals[row * 3 + 1] = ny; normals[row * 3 + 2] = nz; }
    if (face_index != nullptr) face_index[row] = face;
}
#pragma clang fp contract(fast)

static bool min_vox_args_ok(int batch, int r) { return batch > 0 && r >= 2 && r <= MIN_MAX_R; }

int mesh_area_scan_launch(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, float* cdf, hipStream_t stream) {
    hipLaunchKernelGGL(mesh_area_scan_kernel, dim3(batch), dim3(MIN_THREADS), 0, stream, vertices, faces, offsets, cdf);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

extern "C" size_t pcd_mesh_voxelize_workspace_bytes(int batch, int r) {
    if (!min_vox_args_ok(batch, r)) return 0;
    return (size_t)batch * min_acc_bytes(r);
}

extern "C" int pcd_mesh_voxelize(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int r, float lo,
                                 float inv_pitch, int mode, void* workspace, float* vox, void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && workspace && vox && min_vox_args_ok(batch, r));
    PCD_CHECK_ARG(mode == PCD_MESH_FILL_SURFACE || mode == PCD_MESH_FILL_INTERIOR || mode == PCD_MESH_FILL_SOLID);
    PCD_CHECK_ARG(std::isfinite(lo) && std::isfinite(inv_pitch) && inv_pitch > 0.f);
    const size_t acc = min_acc_bytes(r);
    if (r <= MIN_LDS_R) {
        static PcdLdsOnce once;
        PCD_CHECK_HIP(pcd_allow_lds(once, (const void*)mesh_voxelize_kernel<true>, (int)min_acc_bytes(MIN_LDS_R)));
        hipLaunchKernelGGL(mesh_voxelize_kernel<true>, dim3(batch), dim3(MIN_THREADS), acc, (hipStream_t)stream, vertices, faces, offsets, r, lo,
                           inv_pitch, mode, (char*)workspace, acc, vox);
    } else {
        hipLaunchKernelGGL(mesh_voxelize_kernel<false>, dim3(batch), dim3(MIN_THREADS), 0, (hipStream_t)stream, vertices, faces, offsets, r, lo,
                           inv_pitch, mode, (char*)workspace, acc, vox);
    }
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_mesh_sample_workspace_bytes(int batch, int64_t total_faces) {
    if (batch <= 0 || total_faces <= 0) return 0;
    return align_up((size_t)total_faces * sizeof(float));
}

extern "C" int pcd_mesh_sample_points(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int n_points, uint64_t seed,
                                      uint64_t philox_offset, const float* u, void* workspace, float* points, float* normals,
                                      int32_t* face_index, void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && workspace && points);
    PCD_CHECK_ARG(batch > 0 && batch <= 65535 && n_points > 0);
    int rc;
    PCD_RUN(mesh_area_scan_launch(vertices, faces, offsets, batch, (float*)workspace, (hipStream_t)stream));
    hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)ceil_div(n_points, 256), batch), dim3(256), 0, (hipStream_t)stream, vertices, faces,
                       offsets, n_points, seed, philox_offset, u, (const float*)workspace, points, normals, face_index);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
