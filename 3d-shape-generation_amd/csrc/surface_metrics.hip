// Surface evaluation of P ragged cloud pairs (DESIGN.md "Surface metrics"): the nearest neighbour of every point WITH its index, the
// reductions behind accuracy / completeness / Chamfer-L1 / -L2 / F-score / Hausdorff / normal consistency, and the IoU of two
// occupancy grids.  Pair p: a[p][0..na[p]) and b[p][0..nb[p]) inside padded [P][NA][3] / [P][NB][3] arrays, as in metrics_pairs.hip.
//   * nearest neighbour: nearest_scan of pair_scan.h in its form with a running index.  The target range is split over
//     blockIdx.y; the partial results of a query meet in a 64-bit unsigned atomic min on (float bits of d^2) << 32 | j, which
//     orders by d^2 (>= 0, so its bits order as the value) and then by j: the result does not depend on the order of arrival or on
//     the number of splits, and equal minima go to the lowest j.
//   * reduction: one workgroup per pair walks both directions; sums in double (per-thread strided partials, then block_reduce),
//     counts in integers, one rounding to fp32 per mean.
//   * IoU: one workgroup per pair, integer counts, one fp32 division.
#include <math.h>

#include "pair_scan.h"

namespace pcd {

#pragma clang fp contract(off)

constexpr unsigned long long SURF_NONE = ~0ull;     // a key no candidate reaches: its d^2 bits would be a NaN's

struct SurfTaus { float t[PCD_SURF_MAX_THRESHOLDS]; };

// grid (query blocks of SCAN_QBLOCK, target splits, jobs); job z = pair z / dirs, direction z % dirs (0: a queries b, 1: b queries a).
// keys[z][q] (stride NQ, all ones before the launch) takes the least (d^2 bits, j) over the targets with a FINITE d^2 = (dx dx +
// dy dy) + dz dz; a query without one keeps the all-ones key.  Rows at or past a cloud's count are never read.
__global__ __launch_bounds__(256) void surf_nn_kernel(const float* __restrict__ a, const int* __restrict__ na, int NA,
                                                       const float* __restrict__ b, const int* __restrict__ nb, int NB, int dirs,
                                                       int NQ, unsigned long long* __restrict__ keys) {
    __shared__ float4 tile[SCAN_TILE];
    const int p = blockIdx.z / dirs, dir = blockIdx.z % dirs;
    const float* q = dir == 0 ? a + (int64_t)p * NA * 3 : b + (int64_t)p * NB * 3;
    const float* r = dir == 0 ? b + (int64_t)p * NB * 3 : a + (int64_t)p * NA * 3;
    const int ca = clamped_count(na, p, NA), cb = clamped_count(nb, p, NB);
    nearest_scan(q, dir == 0 ? ca : cb, r, dir == 0 ? cb : ca, keys + (int64_t)blockIdx.z * NQ, tile);
}

__device__ __forceinline__ void surf_decode(unsigned long long key, float& d2, int& index) {
    const bool none = key == SURF_NONE;
    d2 = none ? __builtin_nanf("") : __uint_as_float((unsigned)(key >> 32));
    index = none ? -1 : (int)(unsigned)key;
}

// grid (ceil(NQ / 256), P): d2 / index [P][NQ] of pcd_nearest_neighbors; rows at or past the pair's count get (NaN, -1)
__global__ __launch_bounds__(256) void surf_nn_decode_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ nq_,
                                                              int NQ, float* __restrict__ d2, int* __restrict__ index) {
    const int p = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NQ) return;
    const int64_t at = (int64_t)p * NQ + i;
    surf_decode(i < clamped_count(nq_, p, NQ) ? keys[at] : SURF_NONE, d2[at], index[at]);
}

// grid (P): rows[p][PCD_SURF_ROW_BASE + 3 K] from the keys of both directions ([2p] a queries b, [2p + 1] b queries a, stride NQ).
// Optional outputs d2_* / index_* [P][NA] / [P][NB]: the decoded neighbours, (NaN, -1) at and past the count.
__global__ __launch_bounds__(256) void surf_rows_kernel(const unsigned long long* __restrict__ keys, int NQ, const int* __restrict__ na,
                                                         int NA, const int* __restrict__ nb, int NB, const float* __restrict__ normals_a,
                                                         const float* __restrict__ normals_b, SurfTaus taus, int K,
                                                         float* __restrict__ rows, float* __restrict__ d2_a, int* __restrict__ index_a,
                                                         float* __restrict__ d2_b, int* __restrict__ index_b) {
    __shared__ double sd[4];
    __shared__ int si[4];
    __shared__ float sf[4];
    const int p = blockIdx.x, width = PCD_SURF_ROW_BASE + 3 * K;
    const bool with_normals = normals_a != nullptr && normals_b != nullptr;
    float tau2[PCD_SURF_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < PCD_SURF_MAX_THRESHOLDS; ++k) tau2[k] = taus.t[k] * taus.t[k];
    double mean_d[2], mean_d2[2], mean_nc[2];
    float far2 = 0.f, frac[2][PCD_SURF_MAX_THRESHOLDS];
    int lost = 0;
    for (int dir = 0; dir < 2; ++dir) {
        const int n = dir == 0 ? clamped_count(na, p, NA) : clamped_count(nb, p, NB), N = dir == 0 ? NA : NB;
        const unsigned long long* kq = keys + (int64_t)(2 * p + dir) * NQ;
        const float* nq = (dir == 0 ? normals_a : normals_b) + (with_normals ? (int64_t)p * N * 3 : 0);
        const float* nt = (dir == 0 ? normals_b : normals_a) + (with_normals ? (int64_t)p * (dir == 0 ? NB : NA) * 3 : 0);
        float* d2_out = dir == 0 ? d2_a : d2_b;
        int* index_out = dir == 0 ? index_a : index_b;
        double s_d = 0.0, s_d2 = 0.0, s_nc = 0.0;
        float far = 0.f;
        int within[PCD_SURF_MAX_THRESHOLDS] = {0, 0, 0, 0, 0, 0, 0, 0}, none = 0;
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            float d2;
            int j;
            surf_decode(i < n ? kq[i] : SURF_NONE, d2, j);
            if (d2_out) d2_out[(int64_t)p * N + i] = d2;
            if (index_out) index_out[(int64_t)p * N + i] = j;
            if (i >= n) continue;
            if (j < 0) { none += 1; continue; }
            s_d += (double)sqrtf(d2);
            s_d2 += (double)d2;
            far = fmaxf(far, d2);
#pragma unroll
            for (int k = 0; k < PCD_SURF_MAX_THRESHOLDS; ++k) within[k] += (k < K && d2 <= tau2[k]) ? 1 : 0;
            if (with_normals) {
                const float* u = nq + (int64_t)i * 3;
                const float* v = nt + (int64_t)j * 3;
                s_nc += (double)fabsf(u[0] * v[0] + u[1] * v[1] + u[2] * v[2]);
            }
        }
        lost += block_reduce<4>(none, SumOp(), si);
        mean_d[dir] = block_reduce<4>(s_d, SumOp(), sd) / (double)n;
        mean_d2[dir] = block_reduce<4>(s_d2, SumOp(), sd) / (double)n;
        mean_nc[dir] = block_reduce<4>(s_nc, SumOp(), sd) / (double)n;
        far2 = fmaxf(far2, block_reduce<4>(far, MaxOp(), sf));
        for (int k = 0; k < K; ++k) frac[dir][k] = (float)block_reduce<4>(within[k], SumOp(), si) / (float)n;
    }
    if (threadIdx.x != 0) return;
    float* row = rows + (int64_t)p * width;
    // a pair with an empty cloud, or with a point that has no finite distance to the other cloud (a coordinate that is not finite,
    // on either side), has no metrics
    if (clamped_count(na, p, NA) == 0 || clamped_count(nb, p, NB) == 0 || lost > 0) {
        for (int c = 0; c < width; ++c) row[c] = __builtin_nanf("");
        return;
    }
    const float acc = (float)mean_d[0], comp = (float)mean_d[1], acc2 = (float)mean_d2[0], comp2 = (float)mean_d2[1];
    row[PCD_SURF_ROW_ACC] = acc;
    row[PCD_SURF_ROW_COMP] = comp;
    row[PCD_SURF_ROW_CHAMFER_L1] = (acc + comp) / 2.f;
    row[PCD_SURF_ROW_ACC2] = acc2;
    row[PCD_SURF_ROW_COMP2] = comp2;
    row[PCD_SURF_ROW_CHAMFER_L2] = acc2 + comp2;
    row[PCD_SURF_ROW_HAUSDORFF] = sqrtf(far2);
    const float nc_a = with_normals ? (float)mean_nc[0] : __builtin_nanf(""), nc_b = with_normals ? (float)mean_nc[1] : __builtin_nanf("");
    row[PCD_SURF_ROW_NC_A] = nc_a;
    row[PCD_SURF_ROW_NC_B] = nc_b;
    row[PCD_SURF_ROW_NC] = (nc_a + nc_b) / 2.f;
    for (int k = 0; k < K; ++k) {
        const float pr = frac[0][k], rc = frac[1][k];
        row[PCD_SURF_ROW_BASE + 3 * k] = pr;
        row[PCD_SURF_ROW_BASE + 3 * k + 1] = rc;
        row[PCD_SURF_ROW_BASE + 3 * k + 2] = pr + rc > 0.f ? (2.f * pr * rc) / (pr + rc) : 0.f;
    }
}

// grid (P): out[p] = |A and B| / |A or B| with occupancy value > threshold; NaN for an empty union
__global__ __launch_bounds__(256) void surf_voxel_iou_kernel(const float* __restrict__ a, const float* __restrict__ b, int voxels,
                                                              float threshold, float* __restrict__ out) {
    __shared__ int si[4];
    const int p = blockIdx.x;
    const float* ga = a + (int64_t)p * voxels;
    const float* gb = b + (int64_t)p * voxels;
    int both = 0, either = 0;
    for (int i = threadIdx.x; i < voxels; i += blockDim.x) {
        const bool oa = ga[i] > threshold, ob = gb[i] > threshold;
        both += (oa && ob) ? 1 : 0;
        either += (oa || ob) ? 1 : 0;
    }
    both = block_reduce<4>(both, SumOp(), si);
    either = block_reduce<4>(either, SumOp(), si);
    if (threadIdx.x == 0) out[p] = either > 0 ? (float)both / (float)either : __builtin_nanf("");
}

#pragma clang fp contract(fast)

constexpr int SURF_MAX_JOBS = 65535;      // gridDim.z

static size_t surf_key_bytes(int jobs, int NQ) { return align_up((size_t)jobs * NQ * sizeof(unsigned long long)); }

}  // namespace pcd

using namespace pcd;

extern "C" size_t pcd_nearest_workspace_bytes(int pairs, int nq_max, int nt_max) {
    if (pairs <= 0 || pairs > SURF_MAX_JOBS || nq_max <= 0 || nt_max <= 0) return 0;
    return surf_key_bytes(pairs, nq_max);
}

extern "C" int pcd_nearest_neighbors(const float* q, const int* nq, int nq_max, const float* t, const int* nt, int nt_max, int pairs,
                                     float* d2, int32_t* index, void* workspace, size_t workspace_bytes, void* stream) {
    PCD_CHECK_ARG(q && nq && t && nt && d2 && index && workspace);
    PCD_CHECK_ARG(pairs > 0 && pairs <= SURF_MAX_JOBS && nq_max > 0 && nt_max > 0);
    PCD_CHECK_ARG(workspace_bytes >= surf_key_bytes(pairs, nq_max));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)workspace;
    PCD_CHECK_HIP(hipMemsetAsync(keys, 0xff, (size_t)pairs * nq_max * sizeof(unsigned long long), s));
    const dim3 grid((unsigned)ceil_div(nq_max, SCAN_QBLOCK), scan_splits(pairs, nq_max, nt_max), pairs);
    hipLaunchKernelGGL(surf_nn_kernel, grid, dim3(256), 0, s, q, nq, nq_max, t, nt, nt_max, 1, nq_max, keys);
    hipLaunchKernelGGL(surf_nn_decode_kernel, dim3((unsigned)ceil_div(nq_max, 256), pairs), dim3(256), 0, s, keys, nq, nq_max, d2, index);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_surface_metrics_workspace_bytes(int pairs, int na_max, int nb_max) {
    if (pairs <= 0 || 2 * (int64_t)pairs > SURF_MAX_JOBS || na_max <= 0 || nb_max <= 0) return 0;
    return surf_key_bytes(2 * pairs, na_max > nb_max ? na_max : nb_max);
}

extern "C" int pcd_surface_metrics(const float* a, const float* normals_a, const int* na, int na_max, const float* b, const float* normals_b,
                                   const int* nb, int nb_max, int pairs, const float* thresholds, int n_thresholds, float* rows, float* d2_a,
                                   int32_t* index_a, float* d2_b, int32_t* index_b, void* workspace, size_t workspace_bytes, void* stream) {
    PCD_CHECK_ARG(a && na && b && nb && rows && workspace);
    PCD_CHECK_ARG(pairs > 0 && 2 * (int64_t)pairs <= SURF_MAX_JOBS && na_max > 0 && nb_max > 0);
    PCD_CHECK_ARG(n_thresholds >= 0 && n_thresholds <= PCD_SURF_MAX_THRESHOLDS && (n_thresholds == 0 || thresholds));
    SurfTaus taus{};
    for (int k = 0; k < n_thresholds; ++k) {
        PCD_CHECK_ARG(isfinite(thresholds[k]) && thresholds[k] >= 0.f);
        taus.t[k] = thresholds[k];
    }
    const int NQ = na_max > nb_max ? na_max : nb_max;
    PCD_CHECK_ARG(workspace_bytes >= surf_key_bytes(2 * pairs, NQ));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)workspace;
    PCD_CHECK_HIP(hipMemsetAsync(keys, 0xff, (size_t)2 * pairs * NQ * sizeof(unsigned long long), s));
    const dim3 grid((unsigned)ceil_div(NQ, SCAN_QBLOCK), scan_splits(2 * pairs, NQ, NQ), 2 * pairs);
    hipLaunchKernelGGL(surf_nn_kernel, grid, dim3(256), 0, s, a, na, na_max, b, nb, nb_max, 2, NQ, keys);
    hipLaunchKernelGGL(surf_rows_kernel, dim3(pairs), dim3(256), 0, s, keys, NQ, na, na_max, nb, nb_max, normals_a, normals_b, taus,
                       n_thresholds, rows, d2_a, index_a, d2_b, index_b);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_voxel_iou(const float* a, const float* b, int pairs, int voxels, float threshold, float* out, void* stream) {
    PCD_CHECK_ARG(a && b && out && pairs > 0 && voxels > 0 && isfinite(threshold));
    hipLaunchKernelGGL(surf_voxel_iou_kernel, dim3(pairs), dim3(256), 0, (hipStream_t)stream, a, b, voxels, threshold, out);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
