// Closed meshes from point clouds by grid closing (DESIGN.md "Cloud to mesh"; include/pcd_hip.h pcd_cloud_spacing .. pcd_project_to_cloud).
// A cloud is dilated on an R^3 grid of nodes by a ball of radius r (the shell), the free nodes that the grid's surroundings reach through free
// nodes are the outside, everything else is solid, and the solid is eroded again by r through the exact squared distance to the outside; the
// surface-nets kernels of mesh.hip then run on the eroded field.  R <= 64: a grid row (z, y) is one 64-bit word, bit x = node x, so a whole grid of
// shell bits and a whole grid of outside bits (2 x 32 KB at R = 64) live in LDS, one workgroup per cloud.
//   * shell: a wave takes a point, walks the rows (z, y) of the box of nodes that can lie within r of it, a lane evaluates one node with the fp32
//     arithmetic of pcd_nearest_neighbors, the wave's ballot holds the rows' words, one LDS atomic OR per row stores them.
//   * fill: every sweep a thread ORs the four neighbouring rows of its row into it, masks with the free bits and closes the word along x with six
//     doubling shifts in each direction (the Kogge-Stone fill), until a sweep changes nothing.  Growth is monotone, so the order in which rows see
//     one another's updates does not matter for the fixed point.
//   * depth: x from the words with count-leading / trailing-zeros, y and z brute-force minima over a column staged in LDS -- the exact integer EDT.
//   * projection: one thread per vertex, in double, the eigen-solve of geo_prims.h.
// Everything that decides a bit is integer work or fp32 without contraction, so the outputs are bitwise repeatable and a cloud's result does not
// depend on the rest of the batch.
#include <math.h>

#include "common.h"
#include "geo_prims.h"

namespace pcd {

#pragma clang fp contract(off)

typedef unsigned long long u64;

constexpr int CM_THREADS = 1024;
constexpr int CM_WAVES = CM_THREADS / 64;
constexpr int CM_SCRATCH = 64;                 // bytes in front of the two masks: 3 "changed" flags, 3 counters
constexpr int CM_RMIN = 8, CM_RMAX = 64;
constexpr int CM_MAX_CLOUDS = 65535;           // gridDim.y
constexpr size_t CM_LDS_MAX = CM_SCRATCH + 2 * (size_t)CM_RMAX * CM_RMAX * sizeof(u64);

__device__ __forceinline__ u64 cm_full(int R) { return R == 64 ? ~0ull : ((1ull << R) - 1ull); }

// grid (P), 256 threads.  d2 given: the mean over the rows below the count whose last slot is valid of the fp32 root of that slot, summed in
// double and rounded once, times scale; else radii_in[p].  Then the clamp max(r, (2 - inset) h).
__global__ __launch_bounds__(256) void cm_spacing_kernel(const float* __restrict__ d2, const int* __restrict__ counts, int N, int k,
                                                         const float* __restrict__ radii_in, float scale, float h, float inset,
                                                         float* __restrict__ radii) {
    __shared__ double sd[4];
    __shared__ int si[4];
    const int p = blockIdx.x;
    float r = 0.f;
    if (d2) {
        const int n = clamped_count(counts, p, N);
        const float* last = d2 + (int64_t)p * N * k + (k - 1);
        double s = 0.0;
        int c = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const float v = last[(int64_t)i * k];
            if (v == v) { s += (double)sqrtf(v); c += 1; }
        }
        const int have = block_reduce<4>(c, SumOp(), si);
        const double total = block_reduce<4>(s, SumOp(), sd);
        if (have > 0) r = scale * (float)(total / (double)have);
    } else {
        r = radii_in[p];
    }
    const float floor_r = (2.f - inset) * h;
    if (threadIdx.x == 0) radii[p] = fmaxf(r, floor_r);      // a NaN radius takes the clamp value
}

// first and last node index of an axis that a point at coordinate c can reach with reach `mf` nodes: floats all the way, so that no value leaves
// the range of int; an empty range comes out as first > last
__device__ __forceinline__ void cm_range(float c, float lo, float h, float mf, int R, int& first, int& last) {
    const float f = (c - lo) / h;
    first = (int)fminf(fmaxf(floorf(f - mf), 0.f), (float)R);
    last = (int)fmaxf(fminf(ceilf(f + mf), (float)(R - 1)), -1.f);
}

// shell[z * R + y] |= bit x for every node within r of a finite point of the cloud.  The workgroup's 16 waves take the points in turn.  The nodes a
// point can reach fill a box of (2 ceil(r / h) + 3)^3 at the most; where the box is at most 16 (32) nodes wide along x, a wave's 64 lanes cover 4 (2)
// of its rows (z, y .. y + 3) at a time, 16 (32) lanes along x each, else one row.  The wave's ballot holds the rows' words side by side.
__device__ __forceinline__ void cm_shell(const float* __restrict__ pts, int n, int R, float lo, float h, float r, u64* shell) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float r2 = r * r;
    const float mf = ceilf(r / h) + 1.f;                          // nodes within r of a point lie within ceil(r / h) + 1 nodes of it on every axis
    for (int i = wave; i < n; i += CM_WAVES) {
        const float px = pts[(int64_t)i * 3], py = pts[(int64_t)i * 3 + 1], pz = pts[(int64_t)i * 3 + 2];
        if (!(isfinite(px) && isfinite(py) && isfinite(pz))) continue;
        int x0, x1, y0, y1, z0, z1;
        cm_range(px, lo, h, mf, R, x0, x1);
        cm_range(py, lo, h, mf, R, y0, y1);
        cm_range(pz, lo, h, mf, R, z0, z1);
        if (x0 > x1 || y0 > y1 || z0 > z1) continue;
        const int width = x1 - x0 + 1;
        const int shift = width <= 16 ? 4 : (width <= 32 ? 5 : 6);               // lanes per row = 1 << shift
        const int slot = lane >> shift, xi = lane & ((1 << shift) - 1), per_step = 64 >> shift;
        const int x = x0 + xi;
        const float dx = (lo + (float)x * h) - px, dxx = dx * dx;
        for (int z = z0; z <= z1; ++z) {
            const float dz = (lo + (float)z * h) - pz, dzz = dz * dz;
            for (int yb = y0; yb <= y1; yb += per_step) {
                const int y = yb + slot;
                const float dy = (lo + (float)y * h) - py, dyy = dy * dy;
                const u64 votes = __ballot(y <= y1 && x <= x1 && (dxx + dyy) + dzz <= r2);
                if (votes == 0ull) continue;
                const u64 word = shift == 6 ? votes : ((votes >> (slot << shift)) & ((1ull << (1 << shift)) - 1ull));
                if (xi == 0 && word != 0ull) atomicOr(&shell[z * R + y], word << x0);
            }
        }
    }
}

// the bits of `free` that `seed` (a subset of free) reaches along the word through free bits: Kogge-Stone fill towards the high and the low end
__device__ __forceinline__ u64 cm_fill_word(u64 seed, u64 free) {
    u64 up = seed, p = free;
    up |= p & (up << 1); p &= p << 1;
    up |= p & (up << 2); p &= p << 2;
    up |= p & (up << 4); p &= p << 4;
    up |= p & (up << 8); p &= p << 8;
    up |= p & (up << 16); p &= p << 16;
    up |= p & (up << 32);
    u64 down = seed;
    p = free;
    down |= p & (down >> 1); p &= p >> 1;
    down |= p & (down >> 2); p &= p >> 2;
    down |= p & (down >> 4); p &= p >> 4;
    down |= p & (down >> 8); p &= p >> 8;
    down |= p & (down >> 16); p &= p >> 16;
    down |= p & (down >> 32);
    return up | down;
}

// outside = the free nodes 6-connected through free nodes to the layer of free nodes round the grid.  shell, out: R * R words in LDS, shell
// masked to R bits; flag: 3 ints in LDS.  All threads of the workgroup call it and all return the same: the number of sweeps (the last one
// changed nothing), or -1 past R^3 sweeps -- more than the nodes there are to gain, so never for a monotone fill.
__device__ __forceinline__ int cm_fill(const u64* shell, u64* out, int R, int* flag) {
    const u64 full = cm_full(R), ends = 1ull | (1ull << (R - 1));
    const int rows = R * R;
    for (int row = threadIdx.x; row < rows; row += CM_THREADS) {
        const int z = row / R, y = row - z * R;
        const u64 free = ~shell[row] & full;
        const bool edge = z == 0 || z == R - 1 || y == 0 || y == R - 1;        // a row of the layer round the grid lies next to it
        out[row] = cm_fill_word(edge ? free : (free & ends), free);
    }
    if (threadIdx.x < 3) flag[threadIdx.x] = 0;
    __syncthreads();
    const int cap = rows * R;
    for (int s = 0; s < cap; ++s) {
        // three flags in turn: the one cleared here was last read behind the barrier of sweep s - 2, and every thread has passed that of s - 1
        if (threadIdx.x == 0) flag[(s + 1) % 3] = 0;
        bool changed = false;
        for (int row = threadIdx.x; row < rows; row += CM_THREADS) {
            const u64 free = ~shell[row] & full, own = out[row];
            if (own == free) continue;
            const int z = row / R, y = row - z * R;
            u64 seen = own;
            if (y > 0) seen |= out[row - 1];
            if (y < R - 1) seen |= out[row + 1];
            if (z > 0) seen |= out[row - R];
            if (z < R - 1) seen |= out[row + R];
            seen &= free;
            if (seen != own) {                                                   // own is closed along x already
                out[row] = cm_fill_word(seen, free);
                changed = true;
            }
        }
        if (changed) flag[s % 3] = 1;
        __syncthreads();
        if (flag[s % 3] == 0) return s + 1;
    }
    return -1;
}

// info[p] = (shell nodes, enclosed nodes, shell nodes on the six faces of the grid); the words to global memory
__device__ __forceinline__ void cm_finish(const u64* shell, const u64* out, int R, int sweeps_done, int* acc, u64* __restrict__ shell_out,
                                          u64* __restrict__ outside_out, int* __restrict__ info, int* __restrict__ sweeps) {
    const u64 full = cm_full(R), ends = 1ull | (1ull << (R - 1));
    const int rows = R * R, p = blockIdx.x;
    int n_shell = 0, n_enclosed = 0, n_border = 0;
    for (int row = threadIdx.x; row < rows; row += CM_THREADS) {
        const int z = row / R, y = row - z * R;
        const u64 s = shell[row], o = out[row];
        const bool edge = z == 0 || z == R - 1 || y == 0 || y == R - 1;
        n_shell += __popcll(s);
        n_enclosed += __popcll(~s & ~o & full);
        n_border += __popcll(edge ? s : (s & ends));
        if (shell_out) shell_out[(int64_t)p * rows + row] = s;
        outside_out[(int64_t)p * rows + row] = o;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_shell += __shfl_xor(n_shell, o);
        n_enclosed += __shfl_xor(n_enclosed, o);
        n_border += __shfl_xor(n_border, o);
    }
    if (threadIdx.x < 3) acc[threadIdx.x] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {                                               // integer sums: the order does not matter
        atomicAdd(&acc[0], n_shell);
        atomicAdd(&acc[1], n_enclosed);
        atomicAdd(&acc[2], n_border);
    }
    __syncthreads();
    if (threadIdx.x < 3) info[p * 3 + threadIdx.x] = acc[threadIdx.x];
    if (threadIdx.x == 0 && sweeps) sweeps[p] = sweeps_done;
}

// grid (P).  FROM_CLOUD: the shell from points [P][N][3] and radii [P]; else from the caller's words shell_in [P][R][R] (bits at and past R ignored).
template <bool FROM_CLOUD>
__global__ __launch_bounds__(CM_THREADS) void cm_fill_kernel(const float* __restrict__ points, const int* __restrict__ counts, int N, int R,
                                                             float lo, float h, const float* __restrict__ radii,
                                                             const u64* __restrict__ shell_in, u64* __restrict__ shell_out,
                                                             u64* __restrict__ outside_out, int* __restrict__ info,
                                                             int* __restrict__ sweeps) {
    extern __shared__ __attribute__((aligned(16))) char cm_lds[];
    int* flag = (int*)cm_lds;                                                    // [3], then the counters [3]
    int* acc = flag + 4;
    u64* shell = (u64*)(cm_lds + CM_SCRATCH);
    u64* out = shell + R * R;
    const int p = blockIdx.x, rows = R * R;
    if (FROM_CLOUD) {
        for (int row = threadIdx.x; row < rows; row += CM_THREADS) shell[row] = 0ull;
        __syncthreads();
        cm_shell(points + (int64_t)p * N * 3, clamped_count(counts, p, N), R, lo, h, radii[p], shell);
    } else {
        const u64 full = cm_full(R);
        for (int row = threadIdx.x; row < rows; row += CM_THREADS) shell[row] = shell_in[(int64_t)p * rows + row] & full;
    }
    __syncthreads();
    const int done = cm_fill(shell, out, R, flag);
    cm_finish(shell, out, R, done, acc, FROM_CLOUD ? shell_out : nullptr, outside_out, info, sweeps);
}

// squared distance, in nodes along x, from node x to the nearest set bit of the row's word, the nodes -1 and R counting as set
__device__ __forceinline__ int cm_row_d2(u64 word, int x, int R) {
    if ((word >> x) & 1ull) return 0;
    const u64 below = word & ((1ull << x) - 1ull), above = (word >> x) >> 1;
    const int dl = below ? x - (63 - __clzll((long long)below)) : x + 1;
    const int dr = above ? __ffsll((long long)above) : R - x;                    // ffs = index of the lowest set bit + 1 = the distance
    const int d = dl < dr ? dl : dr;
    return d * d;
}

// grid (R, P), 256 threads: layer z of cloud p.  gxy[p][z][y][x] = min over y' of (x pass of row y')[x] + (y - y')^2, the rows -1 and R all outside.
__global__ __launch_bounds__(256) void cm_depth_xy_kernel(const u64* __restrict__ outside, int R, int32_t* __restrict__ gxy) {
    __shared__ int gx[CM_RMAX * CM_RMAX];
    const int z = blockIdx.x, p = blockIdx.y, x = threadIdx.x & 63, y_first = threadIdx.x >> 6;
    const u64* words = outside + ((int64_t)p * R + z) * R;
    const u64 full = cm_full(R);
    if (x < R)
        for (int y = y_first; y < R; y += 4) gx[y * R + x] = cm_row_d2(words[y] & full, x, R);
    __syncthreads();
    if (x >= R) return;
    for (int y = y_first; y < R; y += 4) {
        const int up = (y + 1) * (y + 1), down = (R - y) * (R - y);
        int best = up < down ? up : down;
        for (int j = 0; j < R; ++j) {
            const int c = gx[j * R + x] + (y - j) * (y - j);
            best = c < best ? c : best;
        }
        gxy[(((int64_t)p * R + z) * R + y) * R + x] = best;
    }
}

// grid (R, P), 256 threads: the nodes (., y, .) of cloud p.  Reads gxy from the memory of v itself (the layer it then overwrites, staged in LDS
// first), D2 = min over z' of gxy[z'] + (z - z')^2, and the field v = 0 where D2 = 0, else 1 + ((sqrt(D2) h - r) - inset h).
__global__ __launch_bounds__(256) void cm_depth_z_field_kernel(int R, float h, const float* __restrict__ radii, float inset,
                                                               int32_t* __restrict__ d2_out, void* field) {
    __shared__ int col[CM_RMAX * CM_RMAX];
    const int y = blockIdx.x, p = blockIdx.y, x = threadIdx.x & 63, z_first = threadIdx.x >> 6;
    const int64_t base = (int64_t)p * R * R * R + (int64_t)y * R;
    const int64_t zs = (int64_t)R * R;
    const int32_t* gxy = (const int32_t*)field;      // the same memory under both types: every read of gxy is in front of the barrier, every write of v behind it
    float* v = (float*)field;
    if (x < R)
        for (int z = z_first; z < R; z += 4) col[z * R + x] = gxy[base + z * zs + x];
    __syncthreads();
    if (x >= R) return;
    const float r = radii[p], shift = inset * h;
    for (int z = z_first; z < R; z += 4) {
        const int up = (z + 1) * (z + 1), down = (R - z) * (R - z);
        int best = up < down ? up : down;
        for (int j = 0; j < R; ++j) {
            const int c = col[j * R + x] + (z - j) * (z - j);
            best = c < best ? c : best;
        }
        if (d2_out) d2_out[base + z * zs + x] = best;
        v[base + z * zs + x] = best == 0 ? 0.f : 1.0f + ((sqrtf((float)best) * h - r) - shift);
    }
}

// grid (ceil(V / 256), P): out = scale * vertex + offset per component, then, with neighbour lists, the projection onto the plane through the mean
// of the neighbours whose normal is the eigenvector of the least eigenvalue of their covariance; all of the projection in double from the
// differences to the vertex, rounded to fp32 once.  Rows at and past the vertex count are not touched.
__global__ __launch_bounds__(256) void cm_project_kernel(const float* __restrict__ verts, const int* __restrict__ vcounts, int V,
                                                         const float* __restrict__ points, const int* __restrict__ counts, int N,
                                                         const int* __restrict__ index, int k, float scale, float offset,
                                                         float* __restrict__ out) {
    const int p = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= clamped_count(vcounts, p, V)) return;
    const int64_t row = (int64_t)p * V + i;
    const float fx = verts[row * 3] * scale + offset, fy = verts[row * 3 + 1] * scale + offset, fz = verts[row * 3 + 2] * scale + offset;
    float ox = fx, oy = fy, oz = fz;
    if (index) {
        const int n = clamped_count(counts, p, N);
        const float* pts = points + (int64_t)p * N * 3;
        const int* idx = index + row * k;
        const double px = (double)fx, py = (double)fy, pz = (double)fz;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int m = 0;
        for (int s = 0; s < k; ++s) {
            const int j = idx[s];
            if (j < 0 || j >= n) continue;
            sx += (double)pts[(int64_t)j * 3] - px;
            sy += (double)pts[(int64_t)j * 3 + 1] - py;
            sz += (double)pts[(int64_t)j * 3 + 2] - pz;
            m += 1;
        }
        if (m >= 3) {
            const double mx = sx / (double)m, my = sy / (double)m, mz = sz / (double)m;      // the mean of the neighbours, relative to the vertex
            double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
            for (int s = 0; s < k; ++s) {
                const int j = idx[s];
                if (j < 0 || j >= n) continue;
                const double ex = ((double)pts[(int64_t)j * 3] - px) - mx, ey = ((double)pts[(int64_t)j * 3 + 1] - py) - my,
                             ez = ((double)pts[(int64_t)j * 3 + 2] - pz) - mz;
                a00 += ex * ex; a01 += ex * ey; a02 += ex * ez; a11 += ey * ey; a12 += ey * ez; a22 += ez * ez;
            }
            double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
            for (int sweep = 0; sweep < GEO_SWEEPS; ++sweep) {
                geo_rotate(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);
                geo_rotate(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);
                geo_rotate(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);
            }
            const bool c0 = a00 <= a11 && a00 <= a22, c1 = !c0 && a11 <= a22;
            const double ux = c0 ? v00 : (c1 ? v01 : v02), uy = c0 ? v10 : (c1 ? v11 : v12), uz = c0 ? v20 : (c1 ? v21 : v22);
            const double un = sqrt((ux * ux + uy * uy) + uz * uz);
            const double nx = ux / un, ny = uy / un, nz = uz / un;
            const double t = (mx * nx + my * ny) + mz * nz;                                  // (c - v) . n
            const double qx = px + t * nx, qy = py + t * ny, qz = pz + t * nz;
            if (isfinite(qx) && isfinite(qy) && isfinite(qz)) { ox = (float)qx; oy = (float)qy; oz = (float)qz; }
        }
    }
    out[row * 3] = ox; out[row * 3 + 1] = oy; out[row * 3 + 2] = oz;
}

#pragma clang fp contract(fast)

static bool cm_grid_ok(int clouds, int R) { return clouds > 0 && clouds <= CM_MAX_CLOUDS && R >= CM_RMIN && R <= CM_RMAX; }

static size_t cm_lds_bytes(int R) { return CM_SCRATCH + 2 * (size_t)R * R * sizeof(u64); }

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_cloud_spacing(const float* d2, const int* counts, int n_max, int clouds, int k, const float* radii_in, float radius_scale,
                                 float h, float inset, float* radii, void* stream) {
    PCD_CHECK_ARG(radii && (d2 != nullptr) != (radii_in != nullptr));
    PCD_CHECK_ARG(clouds > 0 && clouds <= CM_MAX_CLOUDS);
    PCD_CHECK_ARG(d2 == nullptr || (counts && n_max > 0 && k >= 1 && k <= PCD_KNN_MAX_K && isfinite(radius_scale) && radius_scale > 0.f));
    PCD_CHECK_ARG(isfinite(h) && h > 0.f && inset >= -1.f && inset <= 1.f);
    hipLaunchKernelGGL(cm_spacing_kernel, dim3(clouds), dim3(256), 0, (hipStream_t)stream, d2, counts, n_max, k, radii_in, radius_scale, h,
                       inset, radii);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_cloud_shell_fill(const float* points, const int* counts, int n_max, int clouds, int resolution, float lo, float h,
                                    const float* radii, uint64_t* shell, uint64_t* outside, int32_t* info, int32_t* sweeps, void* stream) {
    PCD_CHECK_ARG(points && counts && radii && shell && outside && info);
    PCD_CHECK_ARG(cm_grid_ok(clouds, resolution) && n_max > 0);
    PCD_CHECK_ARG(isfinite(lo) && isfinite(h) && h > 0.f);
    static PcdLdsOnce once;
    PCD_CHECK_HIP(pcd_allow_lds(once, (const void*)cm_fill_kernel<true>, (int)CM_LDS_MAX));
    hipLaunchKernelGGL(cm_fill_kernel<true>, dim3(clouds), dim3(CM_THREADS), cm_lds_bytes(resolution), (hipStream_t)stream, points, counts,
                       n_max, resolution, lo, h, radii, (const u64*)nullptr, (u64*)shell, (u64*)outside, info, sweeps);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_grid_fill_outside(const uint64_t* shell, int clouds, int resolution, uint64_t* outside, int32_t* info, int32_t* sweeps,
                                     void* stream) {
    PCD_CHECK_ARG(shell && outside && info && shell != outside);
    PCD_CHECK_ARG(cm_grid_ok(clouds, resolution));
    static PcdLdsOnce once;
    PCD_CHECK_HIP(pcd_allow_lds(once, (const void*)cm_fill_kernel<false>, (int)CM_LDS_MAX));
    hipLaunchKernelGGL(cm_fill_kernel<false>, dim3(clouds), dim3(CM_THREADS), cm_lds_bytes(resolution), (hipStream_t)stream,
                       (const float*)nullptr, (const int*)nullptr, 0, resolution, 0.f, 1.f, (const float*)nullptr, (const u64*)shell,
                       (u64*)nullptr, (u64*)outside, info, sweeps);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_grid_depth_field(const uint64_t* outside, int clouds, int resolution, float h, const float* radii, float inset,
                                    int32_t* d2, float* v, void* stream) {
    PCD_CHECK_ARG(outside && radii && v && (const void*)d2 != (const void*)v);
    PCD_CHECK_ARG(cm_grid_ok(clouds, resolution));
    PCD_CHECK_ARG(isfinite(h) && h > 0.f && inset >= -1.f && inset <= 1.f);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cm_depth_xy_kernel, dim3(resolution, clouds), dim3(256), 0, s, (const u64*)outside, resolution, (int32_t*)v);
    hipLaunchKernelGGL(cm_depth_z_field_kernel, dim3(resolution, clouds), dim3(256), 0, s, resolution, h, radii, inset, d2, (void*)v);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_project_to_cloud(const float* vertices, const int* vertex_counts, int v_max, const float* points, const int* counts,
                                    int n_max, int clouds, const int32_t* index, int k, float scale, float offset, float* out, void* stream) {
    PCD_CHECK_ARG(vertices && vertex_counts && out);
    PCD_CHECK_ARG(clouds > 0 && clouds <= CM_MAX_CLOUDS && v_max > 0);
    PCD_CHECK_ARG(index == nullptr || (points && counts && n_max > 0 && k >= 1 && k <= PCD_KNN_MAX_K));
    PCD_CHECK_ARG(isfinite(scale) && isfinite(offset));
    hipLaunchKernelGGL(cm_project_kernel, dim3((unsigned)ceil_div(v_max, 256), clouds), dim3(256), 0, (hipStream_t)stream, vertices,
                       vertex_counts, v_max, points, counts, n_max, index, k, scale, offset, out);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
