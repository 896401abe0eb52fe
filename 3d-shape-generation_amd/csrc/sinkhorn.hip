// K12: log-domain Sinkhorn EMD (reference metrics.py:94-158) without ever storing the
// B x n x m cost matrix: every pass recomputes C_ij = |x_i - y_j| / Cmax from the 3-float
// points (12 bytes per point from LDS), so a pass is VALU/exp-bound, not HBM-bound.
//   alpha_i = eps * (log(mu + 1e-10) - logsumexp_j(-C_ij / eps + beta_j))     (and the mirror for beta)
// One thread per row, the other cloud + its dual streamed through LDS tiles, online logsumexp.
#include "pair_scan.h"

namespace pcd {

__global__ __launch_bounds__(256) void pair_max_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        int n, int m, unsigned* __restrict__ out_bits) {
    __shared__ float ty[SCAN_TILE * 3];
    const int b = blockIdx.y;
    const float best = max_dist_row(x + (int64_t)b * n * 3, n, y + (int64_t)b * m * 3, m, ty);
    if ((threadIdx.x & 63) == 0) atomicMax(out_bits, __float_as_uint(best));
}

// dual update for the rows of `p` against the cloud `q` with dual `dq`:
//   dp_new[i] = eps * (logmarg - lse_j(-lambda * |p_i - q_j| / cmax + dq[j])),  err = max |dp_new - dp_old|
__global__ __launch_bounds__(256) void sinkhorn_dual_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                             int np_, int nq, const float* __restrict__ cmax,
                                                             float lambda, float eps, float logmarg,
                                                             const float* __restrict__ dq, float* __restrict__ dp,
                                                             unsigned* __restrict__ err_bits) {
    __shared__ float tq[SCAN_TILE * 4];
    const int b = blockIdx.y;
    const float e = sinkhorn_dual_row(p + (int64_t)b * np_ * 3, np_, q + (int64_t)b * nq * 3, nq, lambda / cmax[0], eps, logmarg,
                                      dq + (int64_t)b * nq, dp + (int64_t)b * np_, tq);
    if ((threadIdx.x & 63) == 0) atomicMax(err_bits, __float_as_uint(e));
}

// row_cost[b][i] = sum_j exp(-lambda C_ij + alpha_i + beta_j) * C_ij
__global__ __launch_bounds__(256) void sinkhorn_cost_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             int n, int m, const float* __restrict__ cmax, float lambda,
                                                             const float* __restrict__ alpha,
                                                             const float* __restrict__ beta,
                                                             float* __restrict__ row_cost) {
    __shared__ float tq[SCAN_TILE * 4];
    const int b = blockIdx.y;
    sinkhorn_cost_row(x + (int64_t)b * n * 3, n, y + (int64_t)b * m * 3, m, 1.f / cmax[0], lambda, alpha + (int64_t)b * n,
                      beta + (int64_t)b * m, row_cost + (int64_t)b * n, tq);
}

// out[b] = sum_i row_cost[b][i], fixed order (one block per batch entry)
__global__ __launch_bounds__(256) void row_sum_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
    __shared__ double ws[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += (double)v[(int64_t)blockIdx.x * n + i];
    acc = block_reduce<4>(acc, SumOp(), ws);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)acc;
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_pairwise_max_dist(const float* x, const float* y, int batch, int n, int m, float* out_max,
                                     void* stream) {
    PCD_CHECK_ARG(x && y && out_max && batch > 0 && n > 0 && m > 0);
    hipStream_t s = (hipStream_t)stream;
    PCD_CHECK_HIP(hipMemsetAsync(out_max, 0, sizeof(float), s));
    hipLaunchKernelGGL(pair_max_kernel, dim3((unsigned)ceil_div(n, 256), batch), dim3(256), 0, s, x, y, n, m,
                       (unsigned*)out_max);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_sinkhorn_dual_update(const float* p, const float* q, int batch, int np_, int nq, const float* cmax,
                                        float epsilon, float log_marginal, const float* dual_q, float* dual_p,
                                        float* err_max, void* stream) {
    PCD_CHECK_ARG(p && q && cmax && dual_q && dual_p && err_max && batch > 0 && np_ > 0 && nq > 0 && epsilon > 0.f);
    hipStream_t s = (hipStream_t)stream;
    PCD_CHECK_HIP(hipMemsetAsync(err_max, 0, sizeof(float), s));
    hipLaunchKernelGGL(sinkhorn_dual_kernel, dim3((unsigned)ceil_div(np_, 256), batch), dim3(256), 0, s, p, q, np_, nq,
                       cmax, 1.f / epsilon, epsilon, log_marginal, dual_q, dual_p, (unsigned*)err_max);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_sinkhorn_cost(const float* x, const float* y, int batch, int n, int m, const float* cmax,
                                 float epsilon, const float* alpha, const float* beta, float* row_scratch,
                                 float* cost, void* stream) {
    PCD_CHECK_ARG(x && y && cmax && alpha && beta && row_scratch && cost && batch > 0 && n > 0 && m > 0 && epsilon > 0.f);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sinkhorn_cost_kernel, dim3((unsigned)ceil_div(n, 256), batch), dim3(256), 0, s, x, y, n, m, cmax,
                       1.f / epsilon, alpha, beta, row_scratch);
    PCD_CHECK_LAUNCH();
    hipLaunchKernelGGL(row_sum_kernel, dim3(batch), dim3(256), 0, s, row_scratch, n, cost);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
