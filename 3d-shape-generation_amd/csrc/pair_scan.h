// Row scans over a pair of point clouds, one definition each, for the kernels of metrics.hip, metrics_pairs.hip, sinkhorn.hip and
// surface_metrics.hip: the Sinkhorn dual-update, cost and largest-distance rows (one thread per row, the other cloud streamed through an LDS
// tile), the nearest-target scan (SCAN_Q queries per thread, targets as float4), normalize_to_cube and the voxel cell of a point.  A kernel
// keeps what is its own: which cloud and which counts, its early exits, and where the result goes.  The bodies take the clouds' base pointers
// and index them as their kernels did; the tile is the kernel's __shared__ array.  Each body carries the contraction mode its kernels had.
#pragma once
#include "common.h"

namespace pcd {

constexpr int SCAN_TILE = 512;      // points of the other cloud per LDS tile
constexpr int SCAN_Q = 4;           // queries per thread in the nearest-target scan: one LDS read of a target serves SCAN_Q distances
constexpr int SCAN_QBLOCK = 256 * SCAN_Q;

#pragma clang fp contract(off)

// normalize_to_cube (metrics.py:7-21) of the n points at src by one workgroup; scratch[blockDim / 64]
__device__ __forceinline__ void normalize_cloud(const float* src, int n, float* dst, float* scratch) {
    const int step = blockDim.x;      // read once: read again in every loop, the first read compiles to a vector load
    float mx[3] = {-INFINITY, -INFINITY, -INFINITY}, mn[3] = {INFINITY, INFINITY, INFINITY};
    for (int i = threadIdx.x; i < n; i += step)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = src[i * 3 + k];
            mx[k] = fmaxf(mx[k], v);
            mn[k] = fminf(mn[k], v);
        }
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float hi = block_reduce(mx[k], MaxOp(), scratch);
        const float lo = block_reduce(mn[k], MinOp(), scratch);
        c[k] = (hi + lo) / 2.f;   // metrics.py:17
    }
    float am = 0.f;
    for (int i = threadIdx.x; i < n; i += step)
#pragma unroll
        for (int k = 0; k < 3; ++k) am = fmaxf(am, fabsf(src[i * 3 + k] - c[k]));
    const float scale = block_reduce(am, MaxOp(), scratch);   // metrics.py:19
    for (int i = threadIdx.x; i < n; i += step)
#pragma unroll
        for (int k = 0; k < 3; ++k) dst[i * 3 + k] = (src[i * 3 + k] - c[k]) / scale;
}

// cell[k] of point pt in a res^3 grid over [-1, 1]^3: scale, truncate toward zero as .long() does, clamp (utils.py:501)
__device__ __forceinline__ void voxel_cell(const float* pt, int res, int (&cell)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = ((pt[k] + 1.f) * (float)(res - 1)) / 2.f;
        long long t = (v == v) ? (long long)v : 0;
        t = t < 0 ? 0 : (t > res - 1 ? res - 1 : t);
        cell[k] = (int)t;
    }
}

// Queries blockIdx.x * SCAN_QBLOCK .. of q[0..nq) against share blockIdx.y of the targets r[0..nr), in LDS as float4 (one ds_read_b128,
// broadcast to the wave); every thread keeps SCAN_Q queries in registers, so SCAN_Q distances cost 1 LDS read + 7 SCAN_Q VALU operations.
// The shares meet in an atomic min on out[query], which does not depend on the order of arrival or on the number of shares.
//   Key = unsigned            the float bits of the least d^2 (>= 0, so its bits order as the value), by fminf;
//   Key = unsigned long long  (bits of d^2) << 32 | j, the least FINITE d^2 and then the lowest j; a query without one stores nothing.
//                             Compare-and-select, two VALU operations per distance where fminf is one: 1.22 x the time of the other form.
template <typename Key>
__device__ __forceinline__ void nearest_scan(const float* q, int nq, const float* r, int nr, Key* out,
                                             float4* tile /* [SCAN_TILE] */) {
    constexpr bool INDEX = sizeof(Key) == 8;
    const int q0 = blockIdx.x * SCAN_QBLOCK;
    if (q0 >= nq) return;
    const int per = (nr + gridDim.y - 1) / gridDim.y;
    const int r_lo = blockIdx.y * per, r_hi = min(nr, r_lo + per);
    if (r_lo >= r_hi) return;
    float qx[SCAN_Q], qy[SCAN_Q], qz[SCAN_Q], best[SCAN_Q];
    int arg[SCAN_Q];
#pragma unroll
    for (int c = 0; c < SCAN_Q; ++c) {
        int qi = q0 + c * 256 + threadIdx.x;
        qi = qi < nq ? qi : nq - 1;                          // clamped duplicates are not stored
        qx[c] = q[(int64_t)qi * 3]; qy[c] = q[(int64_t)qi * 3 + 1]; qz[c] = q[(int64_t)qi * 3 + 2];
        best[c] = INFINITY;
        arg[c] = -1;
    }
    for (int r0 = r_lo; r0 < r_hi; r0 += SCAN_TILE) {
        const int cnt = min(SCAN_TILE, r_hi - r0);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
            const float* t = r + (int64_t)(r0 + i) * 3;
            tile[i] = make_float4(t[0], t[1], t[2], 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 t = tile[j];
            const int jj = r0 + j;
#pragma unroll
            for (int c = 0; c < SCAN_Q; ++c) {
                const float dx = qx[c] - t.x, dy = qy[c] - t.y, dz = qz[c] - t.z;
                const float d = dx * dx + dy * dy + dz * dz;
                if constexpr (INDEX) {
                    const bool closer = d < best[c];         // false for a NaN and for +inf: neither is ever a neighbour; ties keep the lower j
                    best[c] = closer ? d : best[c];
                    arg[c] = closer ? jj : arg[c];
                } else {
                    best[c] = fminf(best[c], d);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < SCAN_Q; ++c) {
        const int qi = q0 + c * 256 + threadIdx.x;
        if constexpr (INDEX) {
            if (qi < nq && arg[c] >= 0) atomicMin(out + qi, ((unsigned long long)__float_as_uint(best[c]) << 32) | (unsigned)arg[c]);
        } else {
            if (qi < nq) atomicMin(out + qi, __float_as_uint(best[c]));
        }
    }
}

#pragma clang fp contract(fast)

// Row i = blockIdx.x * blockDim.x + threadIdx.x of x[0..n) against y[0..m), for the three Sinkhorn rows below; a thread past n only helps to
// fill the tile.

// the wave's largest |x_i - y_j|; ty[SCAN_TILE * 3]
__device__ __forceinline__ float max_dist_row(const float* xb, int n, const float* yb, int m, float* ty) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = xb[i * 3]; py = xb[i * 3 + 1]; pz = xb[i * 3 + 2]; }
    float best = 0.f;
    for (int j0 = 0; j0 < m; j0 += SCAN_TILE) {
        const int cnt = min(SCAN_TILE, m - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt * 3; t += blockDim.x) ty[t] = yb[(int64_t)j0 * 3 + t];
        __syncthreads();
        if (live)
            for (int j = 0; j < cnt; ++j) {
                const float dx = px - ty[j * 3], dy = py - ty[j * 3 + 1], dz = pz - ty[j * 3 + 2];
                best = fmaxf(best, dx * dx + dy * dy + dz * dz);
            }
    }
    return wave_reduce(sqrtf(best), MaxOp());
}

// Dual update of row i of cloud p against cloud q with dual dq, online log-sum-exp over tiles of (x, y, z, dual):
//   dp[i] = eps * (logmarg - lse_j(dq[j] - scale * |p_i - q_j|)),  scale = lambda / cmax;  returns the wave's largest |new - old|.  tq[SCAN_TILE * 4]
__device__ __forceinline__ float sinkhorn_dual_row(const float* pb, int n, const float* qb, int m, float scale,
                                                   float eps, float logmarg, const float* dqb, float* dpb, float* tq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = pb[i * 3]; py = pb[i * 3 + 1]; pz = pb[i * 3 + 2]; }
    float mrun = -INFINITY, srun = 0.f;
    for (int j0 = 0; j0 < m; j0 += SCAN_TILE) {
        const int cnt = min(SCAN_TILE, m - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
            tq[t * 4] = qb[(int64_t)(j0 + t) * 3]; tq[t * 4 + 1] = qb[(int64_t)(j0 + t) * 3 + 1];
            tq[t * 4 + 2] = qb[(int64_t)(j0 + t) * 3 + 2]; tq[t * 4 + 3] = dqb[j0 + t];
        }
        __syncthreads();
        if (live)
            for (int j = 0; j < cnt; ++j) {
                const float dx = px - tq[j * 4], dy = py - tq[j * 4 + 1], dz = pz - tq[j * 4 + 2];
                const float v = tq[j * 4 + 3] - scale * sqrtf(dx * dx + dy * dy + dz * dz);
                if (v > mrun) { srun = srun * __expf(mrun - v) + 1.f; mrun = v; }
                else srun += __expf(v - mrun);
            }
    }
    float e = 0.f;
    if (live) {
        const float nv = eps * (logmarg - (mrun + logf(srun)));
        float* dst = dpb + i;
        e = fabsf(nv - *dst);
        *dst = nv;
    }
    return wave_reduce(e, MaxOp());
}

// row_cost[i] = sum_j exp(-lambda C_ij + alpha_i + beta_j) * C_ij,  C_ij = |x_i - y_j| * inv
__device__ __forceinline__ void sinkhorn_cost_row(const float* xb, int n, const float* yb, int m, float inv, float lambda,
                                                  const float* alphab, const float* betab,
                                                  float* row_cost, float* tq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    float px = 0.f, py = 0.f, pz = 0.f, a = 0.f;
    if (live) { px = xb[i * 3]; py = xb[i * 3 + 1]; pz = xb[i * 3 + 2]; a = alphab[i]; }
    float acc = 0.f;
    for (int j0 = 0; j0 < m; j0 += SCAN_TILE) {
        const int cnt = min(SCAN_TILE, m - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
            tq[t * 4] = yb[(int64_t)(j0 + t) * 3]; tq[t * 4 + 1] = yb[(int64_t)(j0 + t) * 3 + 1];
            tq[t * 4 + 2] = yb[(int64_t)(j0 + t) * 3 + 2]; tq[t * 4 + 3] = betab[j0 + t];
        }
        __syncthreads();
        if (live)
            for (int j = 0; j < cnt; ++j) {
                const float dx = px - tq[j * 4], dy = py - tq[j * 4 + 1], dz = pz - tq[j * 4 + 2];
                const float c = sqrtf(dx * dx + dy * dy + dz * dz) * inv;
                acc += __expf(-lambda * c + a + tq[j * 4 + 3]) * c;
            }
    }
    if (live) row_cost[i] = acc;
}

// Shares of the targets (gridDim.y of nearest_scan) so that ~1024 workgroups exist even for one job, never below 128 targets a share
static int scan_splits(int jobs, int NQ, int NT) {
    const int64_t qblocks = ceil_div(NQ, SCAN_QBLOCK);
    int64_t s = ceil_div(1024, qblocks * jobs);
    const int64_t max_split = ceil_div(NT, 128);
    s = s > max_split ? max_split : s;
    s = s > 65535 ? 65535 : s;
    return s < 1 ? 1 : (int)s;
}

}  // namespace pcd
