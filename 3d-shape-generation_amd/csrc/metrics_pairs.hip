// K10-K12 for a BATCH of independent cloud pairs: what the reference's evaluation loop computes one pair at a time
// (test_point_ddpm.py:85-92 -> metrics.compute_metrics, metrics.py:160-183): normalize_to_cube of both clouds, Chamfer
// distance, Sinkhorn EMD (metrics.py:94-158) and the voxel-occupancy BCE, for P ragged pairs in one enqueue with no
// host synchronisation.  Pair p: a[p][0..na[p]) and b[p][0..nb[p]) inside padded [P][NA][3] / [P][NB][3] arrays.
//   * Chamfer: thread = query, targets streamed through LDS; the target range is split over blockIdx.y so that a
//     single pair still spreads over the chip (per-query minima meet in an atomicMin on the float bits of d^2 >= 0,
//     which is order independent), then one block per pair adds sqrt(min) in a fixed order.
//   * Sinkhorn: the log-domain dual updates of sinkhorn.hip with per-pair sizes, per-pair cost normalisation and the
//     reference's `if err < thresh: break` kept ON THE DEVICE: iteration k+1 of a pair is skipped when both of its
//     iteration-k errors are below the threshold (a skipped iteration leaves its error slots at zero, so the skip is
//     sticky), and the host enqueues all max_iter iterations without reading anything back.
//   * voxel BCE: both (un-normalised, as metrics.py:181 passes them) clouds are rasterised to 32^3 bit sets; F.binary_cross_entropy of two binary grids with torch's
//     log clamp at -100 is exactly 100 * (number of differing voxels) / 32768.
#include "pair_scan.h"

namespace pcd {

#pragma clang fp contract(off)

// grid (P, 2): cloud 0 = a, 1 = b of pair blockIdx.x
__global__ __launch_bounds__(256) void pair_normalize_kernel(const float* __restrict__ a, const int* __restrict__ na, int NA,
                                                              const float* __restrict__ b, const int* __restrict__ nb, int NB,
                                                              float* __restrict__ an, float* __restrict__ bn) {
    __shared__ float scratch[4];
    const int p = blockIdx.x, which = blockIdx.y;
    const int n = which ? nb[p] : na[p];
    const float* src = which ? b + (int64_t)p * NB * 3 : a + (int64_t)p * NA * 3;
    float* dst = which ? bn + (int64_t)p * NB * 3 : an + (int64_t)p * NA * 3;
    normalize_cloud(src, n, dst, scratch);
}

// grid (query blocks of SCAN_QBLOCK, target splits, 2 * P); mins[(2p + dir)][q] = min_j |q - t_j|^2 as float bits (init +inf)
__global__ __launch_bounds__(256) void pair_chamfer_min_kernel(const float* __restrict__ an, const int* __restrict__ na, int NA,
                                                                const float* __restrict__ bn, const int* __restrict__ nb, int NB,
                                                                int NQ, unsigned* __restrict__ mins) {
    __shared__ float4 tile[SCAN_TILE];
    const int p = blockIdx.z >> 1, dir = blockIdx.z & 1;
    const float* q = dir == 0 ? an + (int64_t)p * NA * 3 : bn + (int64_t)p * NB * 3;
    const float* r = dir == 0 ? bn + (int64_t)p * NB * 3 : an + (int64_t)p * NA * 3;
    const int nq = dir == 0 ? na[p] : nb[p], nr = dir == 0 ? nb[p] : na[p];
    nearest_scan(q, nq, r, nr, mins + (int64_t)blockIdx.z * NQ, tile);
}

// grid (P): cd[p] = sum_i sqrt(min_a[i]) / na + sum_j sqrt(min_b[j]) / nb, fixed summation order (metrics.py:41-46)
__global__ __launch_bounds__(256) void pair_chamfer_sum_kernel(const unsigned* __restrict__ mins, const int* __restrict__ na,
                                                                const int* __restrict__ nb, int NQ, float* __restrict__ rows) {
    __shared__ float w[4];
    const int p = blockIdx.x;
    float tot[2];
    for (int dir = 0; dir < 2; ++dir) {
        const int n = dir == 0 ? na[p] : nb[p];
        const unsigned* m = mins + (int64_t)(2 * p + dir) * NQ;
        float acc = 0.f;
        for (int i = threadIdx.x; i < n; i += blockDim.x) acc += sqrtf(__uint_as_float(m[i]));
        tot[dir] = block_reduce<4>(acc, SumOp(), w);
    }
    if (threadIdx.x == 0) rows[p * 3 + 0] = tot[0] / (float)na[p] + tot[1] / (float)nb[p];
}

#pragma clang fp contract(fast)

// ---- Sinkhorn, ragged.  grid (row blocks, P).
__global__ __launch_bounds__(256) void pair_cmax_kernel(const float* __restrict__ an, const int* __restrict__ na, int NA,
                                                         const float* __restrict__ bn, const int* __restrict__ nb, int NB,
                                                         unsigned* __restrict__ cmax_bits) {
    __shared__ float ty[SCAN_TILE * 3];
    const int p = blockIdx.y, n = na[p], m = nb[p];
    if ((int)(blockIdx.x * blockDim.x) >= n) return;
    const float best = max_dist_row(an + (int64_t)p * NA * 3, n, bn + (int64_t)p * NB * 3, m, ty);
    if ((threadIdx.x & 63) == 0) atomicMax(cmax_bits + p, __float_as_uint(best));
}

// one half-iteration for every pair: rows of `pc` (count np[p]) against `qc` (count nq[p]).
// err layout: err[parity][p][2] (alpha, beta) as float bits; `slot` = 0 (alpha update) or 1 (beta update).
// A pair whose two errors of the previous iteration are both below `thresh` is converged and skipped (metrics.py:147-150).
__global__ __launch_bounds__(256) void pair_sinkhorn_dual_kernel(const float* __restrict__ pc, const int* __restrict__ np_, int NP,
                                                                  const float* __restrict__ qc, const int* __restrict__ nq_, int NQc,
                                                                  const unsigned* __restrict__ cmax_bits, float lambda, float eps,
                                                                  const float* __restrict__ logmarg, const float* __restrict__ dq,
                                                                  float* __restrict__ dp, unsigned* __restrict__ err, int P,
                                                                  int iter, int slot, float thresh) {
    __shared__ float tq[SCAN_TILE * 4];
    const int p = blockIdx.y, n = np_[p], m = nq_[p];
    const unsigned* eprev = err + (int64_t)((iter + 1) & 1) * P * 2 + p * 2;
    unsigned* ecur = err + (int64_t)(iter & 1) * P * 2 + p * 2;
    if (iter > 0 && __uint_as_float(eprev[0]) < thresh && __uint_as_float(eprev[1]) < thresh) return;   // converged
    if ((int)(blockIdx.x * blockDim.x) >= n) return;
    const float e = sinkhorn_dual_row(pc + (int64_t)p * NP * 3, n, qc + (int64_t)p * NQc * 3, m, lambda / __uint_as_float(cmax_bits[p]), eps,
                                      logmarg[p], dq + (int64_t)p * NQc, dp + (int64_t)p * NP, tq);
    if ((threadIdx.x & 63) == 0) atomicMax(ecur + slot, __float_as_uint(e));
}

// clears the error slots the NEXT iteration will write (grid 1)
__global__ void pair_sinkhorn_clear_kernel(unsigned* __restrict__ err, int P, int next_iter) {
    unsigned* e = err + (int64_t)(next_iter & 1) * P * 2;
    for (int i = threadIdx.x; i < 2 * P; i += blockDim.x) e[i] = 0u;
}

__global__ __launch_bounds__(256) void pair_sinkhorn_cost_kernel(const float* __restrict__ an, const int* __restrict__ na, int NA,
                                                                  const float* __restrict__ bn, const int* __restrict__ nb, int NB,
                                                                  const unsigned* __restrict__ cmax_bits, float lambda,
                                                                  const float* __restrict__ alpha, const float* __restrict__ beta,
                                                                  float* __restrict__ row_cost) {
    __shared__ float tq[SCAN_TILE * 4];
    const int p = blockIdx.y, n = na[p], m = nb[p];
    if ((int)(blockIdx.x * blockDim.x) >= n) return;
    sinkhorn_cost_row(an + (int64_t)p * NA * 3, n, bn + (int64_t)p * NB * 3, m, 1.f / __uint_as_float(cmax_bits[p]), lambda,
                      alpha + (int64_t)p * NA, beta + (int64_t)p * NB, row_cost + (int64_t)p * NA, tq);
}

// rows[p][1] = sum_i row_cost[p][i], fixed order, double accumulation
__global__ __launch_bounds__(256) void pair_row_sum_kernel(const float* __restrict__ v, const int* __restrict__ na, int NA,
                                                            float* __restrict__ rows) {
    __shared__ double ws[4];
    const int p = blockIdx.x, n = na[p];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += (double)v[(int64_t)p * NA + i];
    acc = block_reduce<4>(acc, SumOp(), ws);
    if (threadIdx.x == 0) rows[p * 3 + 1] = (float)acc;
}

#pragma clang fp contract(off)
// ---- voxel BCE: 32^3 occupancy as 1024-word bit sets (index order [x][y][z], utils.py:488-509)
__global__ __launch_bounds__(256) void pair_voxelize_bits_kernel(const float* __restrict__ an, const int* __restrict__ na, int NA,
                                                                  const float* __restrict__ bn, const int* __restrict__ nb, int NB,
                                                                  unsigned* __restrict__ bits /* [P][2][1024], zeroed */) {
    const int p = blockIdx.y, which = blockIdx.z;
    const int n = which ? nb[p] : na[p];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* pt = (which ? bn + (int64_t)p * NB * 3 : an + (int64_t)p * NA * 3) + (int64_t)i * 3;
    int idx[3];
    voxel_cell(pt, 32, idx);
    const int lin = (idx[0] * 32 + idx[1]) * 32 + idx[2];
    atomicOr(bits + ((int64_t)p * 2 + which) * 1024 + (lin >> 5), 1u << (lin & 31));
}

__global__ __launch_bounds__(256) void pair_bce_kernel(const unsigned* __restrict__ bits, float* __restrict__ rows) {
    __shared__ int ws[4];
    const int p = blockIdx.x;
    const unsigned* ga = bits + (int64_t)p * 2 * 1024;
    const unsigned* gb = ga + 1024;
    int diff = 0;
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) diff += __popc(ga[i] ^ gb[i]);
    diff = block_reduce<4>(diff, SumOp(), ws);
    if (threadIdx.x == 0) rows[p * 3 + 2] = (100.f * (float)diff) / 32768.f;   // metrics.py:181
}
#pragma clang fp contract(fast)

// a pair with an empty cloud has no metrics (the reference's compute_metrics would raise on it): its row is NaN, explicitly --
// otherwise the Chamfer mean is 0/0 but the Sinkhorn scale divides by a zero cost maximum and the BCE of an empty grid is a number
__global__ void pair_empty_rows_kernel(const int* __restrict__ na, const int* __restrict__ nb, int P, float* __restrict__ rows) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P && (na[p] <= 0 || nb[p] <= 0)) rows[p * 3 + 0] = rows[p * 3 + 1] = rows[p * 3 + 2] = __builtin_nanf("");
}

static inline size_t pm_align(size_t v) { return (v + 255) / 256 * 256; }
struct PmWs { size_t an, bn, mins, alpha, beta, rowc, cmax, err, bits, total; };
static PmWs pm_carve(int P, int NA, int NB) {
    PmWs w{};
    const int NQ = NA > NB ? NA : NB;
    size_t o = 0;
    w.an = o; o += pm_align((size_t)P * NA * 3 * 4);
    w.bn = o; o += pm_align((size_t)P * NB * 3 * 4);
    w.mins = o; o += pm_align((size_t)P * 2 * NQ * 4);
    w.alpha = o; o += pm_align((size_t)P * NA * 4);
    w.beta = o; o += pm_align((size_t)P * NB * 4);
    w.rowc = o; o += pm_align((size_t)P * NA * 4);
    w.cmax = o; o += pm_align((size_t)P * 4);
    w.err = o; o += pm_align((size_t)P * 4 * 4);
    w.bits = o; o += pm_align((size_t)P * 2 * 1024 * 4);
    w.total = o;
    return w;
}

}  // namespace pcd

using namespace pcd;

extern "C" size_t pcd_pair_metrics_workspace_bytes(int pairs, int na_max, int nb_max) {
    if (pairs <= 0 || na_max <= 0 || nb_max <= 0) return 0;
    return pm_carve(pairs, na_max, nb_max).total;
}

// Byte offsets of the stage buffers pcd_pair_metrics leaves in its workspace, in the order of PCD_PAIR_WS_* (include/pcd_hip.h);
// host arithmetic only, the same carve the launch uses.
extern "C" int pcd_pair_metrics_workspace_layout(int pairs, int na_max, int nb_max, size_t* offsets) {
    PCD_CHECK_ARG(offsets && pairs > 0 && na_max > 0 && nb_max > 0);
    const PmWs w = pm_carve(pairs, na_max, nb_max);
    const size_t f[PCD_PAIR_WS_FIELDS] = {w.an, w.bn, w.mins, w.alpha, w.beta, w.rowc, w.cmax, w.err, w.bits, w.total};
    for (int i = 0; i < PCD_PAIR_WS_FIELDS; ++i) offsets[i] = f[i];
    return PCD_OK;
}

extern "C" int pcd_pair_metrics(const float* a, const int* na, int na_max, const float* b, const int* nb, int nb_max, int pairs,
                                int with_sinkhorn, float epsilon, float thresh, int max_iter, const float* log_mu,
                                const float* log_nu, float* rows, void* workspace, size_t workspace_bytes, void* stream) {
    PCD_CHECK_ARG(a && na && b && nb && rows && workspace && pairs > 0 && na_max > 0 && nb_max > 0);
    PCD_CHECK_ARG(!with_sinkhorn || (log_mu && log_nu && epsilon > 0.f && max_iter > 0));
    const int P = pairs, NA = na_max, NB = nb_max, NQ = NA > NB ? NA : NB;
    const PmWs w = pm_carve(P, NA, NB);
    if (workspace_bytes < w.total) {
        set_error("pcd_pair_metrics: workspace %zu < required %zu", workspace_bytes, w.total);
        return PCD_ERR_WORKSPACE;
    }
    char* ws = (char*)workspace;
    float *an = (float*)(ws + w.an), *bn = (float*)(ws + w.bn), *alpha = (float*)(ws + w.alpha), *beta = (float*)(ws + w.beta);
    float* rowc = (float*)(ws + w.rowc);
    unsigned *mins = (unsigned*)(ws + w.mins), *cmax = (unsigned*)(ws + w.cmax), *err = (unsigned*)(ws + w.err);
    unsigned* bits = (unsigned*)(ws + w.bits);
    hipStream_t s = (hipStream_t)stream;
    PCD_CHECK_HIP(hipMemsetAsync(mins, 0x7f, (size_t)P * 2 * NQ * 4, s));            // 0x7f7f7f7f = 3.39e38 > any d^2
    PCD_CHECK_HIP(hipMemsetAsync(bits, 0, (size_t)P * 2 * 1024 * 4, s));
    PCD_CHECK_HIP(hipMemsetAsync(rows, 0, (size_t)P * 3 * 4, s));
    hipLaunchKernelGGL(pair_normalize_kernel, dim3(P, 2), dim3(256), 0, s, a, na, NA, b, nb, NB, an, bn);
    // Chamfer: split the targets so that ~1024 blocks exist even for one pair
    const int qblocks = (int)ceil_div(NQ, 256);
    const dim3 cgrid((unsigned)ceil_div(NQ, SCAN_QBLOCK), scan_splits(2 * P, NQ, NQ), 2 * P);
    hipLaunchKernelGGL(pair_chamfer_min_kernel, cgrid, dim3(256), 0, s, an, na, NA, bn, nb, NB, NQ, mins);
    hipLaunchKernelGGL(pair_chamfer_sum_kernel, dim3(P), dim3(256), 0, s, mins, na, nb, NQ, rows);
    hipLaunchKernelGGL(pair_voxelize_bits_kernel, dim3(qblocks, P, 2), dim3(256), 0, s, a, na, NA, b, nb, NB, bits);   // the RAW clouds (metrics.py:181)
    hipLaunchKernelGGL(pair_bce_kernel, dim3(P), dim3(256), 0, s, bits, rows);
    PCD_CHECK_LAUNCH();
    if (with_sinkhorn) {
        PCD_CHECK_HIP(hipMemsetAsync(cmax, 0, (size_t)P * 4, s));
        PCD_CHECK_HIP(hipMemsetAsync(err, 0, (size_t)P * 4 * 4, s));
        PCD_CHECK_HIP(hipMemsetAsync(alpha, 0, (size_t)P * NA * 4, s));
        PCD_CHECK_HIP(hipMemsetAsync(beta, 0, (size_t)P * NB * 4, s));
        const int ablocks = (int)ceil_div(NA, 256), bblocks = (int)ceil_div(NB, 256);
        hipLaunchKernelGGL(pair_cmax_kernel, dim3(ablocks, P), dim3(256), 0, s, an, na, NA, bn, nb, NB, cmax);
        const float lambda = 1.f / epsilon;
        for (int it = 0; it < max_iter; ++it) {
            hipLaunchKernelGGL(pair_sinkhorn_dual_kernel, dim3(ablocks, P), dim3(256), 0, s, an, na, NA, bn, nb, NB, cmax, lambda,
                               epsilon, log_mu, beta, alpha, err, P, it, 0, thresh);
            hipLaunchKernelGGL(pair_sinkhorn_dual_kernel, dim3(bblocks, P), dim3(256), 0, s, bn, nb, NB, an, na, NA, cmax, lambda,
                               epsilon, log_nu, alpha, beta, err, P, it, 1, thresh);
            hipLaunchKernelGGL(pair_sinkhorn_clear_kernel, dim3(1), dim3(256), 0, s, err, P, it + 1);
        }
        hipLaunchKernelGGL(pair_sinkhorn_cost_kernel, dim3(ablocks, P), dim3(256), 0, s, an, na, NA, bn, nb, NB, cmax, lambda, alpha,
                           beta, rowc);
        hipLaunchKernelGGL(pair_row_sum_kernel, dim3(P), dim3(256), 0, s, rowc, na, NA, rows);
        PCD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pair_empty_rows_kernel, dim3((unsigned)ceil_div(P, 256)), dim3(256), 0, s, na, nb, P, rows);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
