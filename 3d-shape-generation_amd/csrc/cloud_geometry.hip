// Local geometry of P ragged clouds (DESIGN.md "Cloud geometry"): the k nearest neighbours of every point, PCA normals from the neighbour
// lists, the statistical / radius outlier masks from the neighbour distances, and the stable compaction of a cloud by a mask.  Cloud p is
// points[p][0..counts[p]) inside a padded [P][N][3] array, as in surface_metrics.hip; rows at or past a count are never read as data.
//   * k nearest: a loop of its own next to nearest_scan of pair_scan.h (targets in LDS as float4, read as a wave-wide broadcast, d2 = (dx dx + dy dy) + dz dz without
//     contraction), one query per thread.  A thread keeps its K best (d2, j) in registers, sorted, K a template constant >= k, so the
//     insertion is a fully unrolled compare-and-shift and nothing is indexed at run time.  A target is a candidate while d2 < the thread's
//     K-th best.  Candidates are rare after the first few hundred targets, but among the 64 lanes of a wave some lane has one at almost
//     every target, so a candidate is not inserted on the spot: it is parked in a small per-thread queue in LDS, and the wave runs the
//     insertion only when a lane's queue is full (and once at the end), for all lanes at once.  The queue keeps the order of j, the
//     comparison is strict, so equal distances stay in the order of j: the list is the order of the key (d2 bits) << 32 | j.
//   * normals: one thread per point, all in double: the mean and the covariance of the differences to the point itself (exact in double
//     for fp32 coordinates), cyclic Jacobi rotations on the 3 x 3 matrix, the column of the smallest eigenvalue.
//   * outliers: one workgroup per cloud; the means and the deviation in double in a fixed order (per-thread strided partials, a butterfly
//     over each wave, the four waves in order).
//   * compaction: one workgroup per cloud walks the rows in blocks of 256 with a ballot prefix per wave and the four wave totals in LDS.
#include <math.h>

#include "common.h"
#include "geo_prims.h"

namespace pcd {

#pragma clang fp contract(off)

constexpr int KNN_TILE = 512;      // targets per LDS tile
constexpr int KNN_BLOCK = 256;     // queries per workgroup, one per thread
constexpr int KNN_STEP = 4;        // targets per step of the inner loop: one group of LDS reads, one look at the queues
constexpr int KNN_PEND = 8;        // parked candidates per thread; a queue is emptied before a step could overflow it

// the sorted list takes (d, j) if d is below its last entry; entries equal to d stay in front of it (they came with a lower j)
template <int K>
__device__ __forceinline__ void knn_insert(float (&bd)[K], int (&bi)[K], float d, int j) {
#pragma unroll
    for (int s = K - 1; s > 0; --s) {                    // selects on values already in registers: no branch per slot
        const float lo = bd[s - 1], cur = bd[s];
        const int ilo = bi[s - 1], icur = bi[s];
        const bool up = d < lo, here = d < cur;
        const float keep_d = here ? d : cur;
        const int keep_i = here ? j : icur;
        bd[s] = up ? lo : keep_d;
        bi[s] = up ? ilo : keep_i;
    }
    const float d0 = bd[0];
    const int i0 = bi[0];
    const bool first = d < d0;
    bd[0] = first ? d : d0;
    bi[0] = first ? j : i0;
}

// grid (ceil(NQ / 256), P).  d2 / index [P][NQ][k]: slot s of query i = the s-th smallest (d2 bits, j) over the targets j < nt[p] with a finite
// d2 (and j != i under exclude_self); (NaN, -1) in the slots past the number of such targets and in every slot of a row at or past nq[p].
template <int K>
__global__ __launch_bounds__(KNN_BLOCK) void knn_kernel(const float* __restrict__ q_, const int* __restrict__ nq_, int NQ,
                                                        const float* __restrict__ t_, const int* __restrict__ nt_, int NT, int k,
                                                        int exclude_self, float* __restrict__ d2, int* __restrict__ index) {
    __shared__ float4 tile[KNN_TILE];
    __shared__ uint2 pend[KNN_PEND][KNN_BLOCK];           // parked candidates: (bits of d2, j), one 8-byte write each
    const int p = blockIdx.y, tid = threadIdx.x;
    const int nq = clamped_count(nq_, p, NQ), nt = clamped_count(nt_, p, NT);
    const int q0 = blockIdx.x * KNN_BLOCK, qi = q0 + tid;
    const float* q = q_ + (int64_t)p * NQ * 3;
    const float* t = t_ + (int64_t)p * NT * 3;
    float bd[K];
    int bi[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bi[s] = -1; }
    if (q0 < nq) {
        const int qr = qi < nq ? qi : nq - 1;                // clamped duplicates are not stored
        const float qx = q[(int64_t)qr * 3], qy = q[(int64_t)qr * 3 + 1], qz = q[(int64_t)qr * 3 + 2];
        const int self = exclude_self ? qi : -1;
        float worst = INFINITY;                              // the K-th best at the last flush: a NaN or +inf d2 is never below it
        int cnt = 0;
        for (int t0 = 0; t0 < nt; t0 += KNN_TILE) {
            const int n_tile = min(KNN_TILE, nt - t0);
            const int n_pad = (n_tile + KNN_STEP - 1) / KNN_STEP * KNN_STEP;      // the slots up to a whole step: points at infinity, nobody's candidates
            __syncthreads();
            for (int i = tid; i < n_pad; i += KNN_BLOCK) {
                const float* r = t + (int64_t)(t0 + i) * 3;
                tile[i] = i < n_tile ? make_float4(r[0], r[1], r[2], 0.f) : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
            }
            __syncthreads();
            for (int j = 0; j < n_pad; j += KNN_STEP) {
                float4 r[KNN_STEP];
#pragma unroll
                for (int u = 0; u < KNN_STEP; ++u) r[u] = tile[j + u];
#pragma unroll
                for (int u = 0; u < KNN_STEP; ++u) {
                    const int jj = t0 + j + u;
                    const float dx = qx - r[u].x, dy = qy - r[u].y, dz = qz - r[u].z;
                    const float d = dx * dx + dy * dy + dz * dz;
                    if (d < worst && jj != self) {
                        pend[cnt][tid] = make_uint2(__float_as_uint(d), (unsigned)jj);
                        ++cnt;
                    }
                }
                if (__any(cnt > KNN_PEND - KNN_STEP)) {          // the next step could overflow some lane's queue
#pragma nounroll
                    for (int c = 0; c < KNN_PEND; ++c) {
                        if (!__any(c < cnt)) break;
                        const uint2 parked = pend[c][tid];
                        const float cd = c < cnt ? __uint_as_float(parked.x) : INFINITY;
                        knn_insert<K>(bd, bi, cd, (int)parked.y);
                    }
                    cnt = 0;
                    worst = bd[K - 1];
                }
            }
        }
#pragma nounroll
        for (int c = 0; c < KNN_PEND; ++c) {
            if (!__any(c < cnt)) break;
            const uint2 parked = pend[c][tid];
            const float cd = c < cnt ? __uint_as_float(parked.x) : INFINITY;
            knn_insert<K>(bd, bi, cd, (int)parked.y);
        }
    }
    if (qi >= NQ) return;
    const bool live = qi < nq;
    const int64_t at = ((int64_t)p * NQ + qi) * k;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        if (s < k) {
            const bool has = live && bi[s] >= 0;
            d2[at + s] = has ? bd[s] : __builtin_nanf("");
            index[at + s] = has ? bi[s] : -1;
        }
    }
}

// grid (P): centroid[p][3] = the mean in double of the rows below the count whose three coordinates are finite (0 without one)
__global__ __launch_bounds__(256) void geo_centroid_kernel(const float* __restrict__ points, const int* __restrict__ counts, int N,
                                                           double* __restrict__ centroid) {
    __shared__ double sd[4];
    __shared__ int si[4];
    const int p = blockIdx.x, n = clamped_count(counts, p, N);
    const float* pts = points + (int64_t)p * N * 3;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float x = pts[(int64_t)i * 3], y = pts[(int64_t)i * 3 + 1], z = pts[(int64_t)i * 3 + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) { sx += (double)x; sy += (double)y; sz += (double)z; c += 1; }
    }
    sx = block_reduce<4>(sx, SumOp(), sd);
    sy = block_reduce<4>(sy, SumOp(), sd);
    sz = block_reduce<4>(sz, SumOp(), sd);
    c = block_reduce<4>(c, SumOp(), si);
    if (threadIdx.x == 0) {
        double* out = centroid + (int64_t)p * 3;
        out[0] = c > 0 ? sx / (double)c : 0.0;
        out[1] = c > 0 ? sy / (double)c : 0.0;
        out[2] = c > 0 ? sz / (double)c : 0.0;
    }
}

// grid (ceil(N / 256), P): normals [P][N][3], curvature [P][N] or null.  mode 0: no orientation, 1: away from centroid[p], 2: toward view[p].
__global__ __launch_bounds__(256) void geo_normals_kernel(const float* __restrict__ points, const int* __restrict__ counts, int N,
                                                          const int* __restrict__ index, int k, int mode,
                                                          const double* __restrict__ centroid, const float* __restrict__ view,
                                                          float* __restrict__ normals, float* __restrict__ curvature) {
    const int p = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int n = clamped_count(counts, p, N);
    const int64_t row = (int64_t)p * N + i;
    float* out = normals + row * 3;
    float nx = 0.f, ny = 0.f, nz = 0.f, curv = __builtin_nanf("");
    if (i < n) {
        const float* pts = points + (int64_t)p * N * 3;
        const int* idx = index + row * k;
        const double px = (double)pts[(int64_t)i * 3], py = (double)pts[(int64_t)i * 3 + 1], pz = (double)pts[(int64_t)i * 3 + 2];
        // the neighbourhood: the point itself (difference 0) and the neighbours 0 <= j < count; differences of fp32 values are exact in double
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int m = 1;
        for (int s = 0; s < k; ++s) {
            const int j = idx[s];
            if (j < 0 || j >= n) continue;
            sx += (double)pts[(int64_t)j * 3] - px;
            sy += (double)pts[(int64_t)j * 3 + 1] - py;
            sz += (double)pts[(int64_t)j * 3 + 2] - pz;
            m += 1;
        }
        if (m >= 3) {
            const double mx = sx / (double)m, my = sy / (double)m, mz = sz / (double)m;
            double a00 = mx * mx, a01 = mx * my, a02 = mx * mz, a11 = my * my, a12 = my * mz, a22 = mz * mz;      // the point itself: (0 - mean)
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
            // the smallest eigenvalue, the lowest column on a tie
            const bool c0 = a00 <= a11 && a00 <= a22, c1 = !c0 && a11 <= a22;
            double ux = c0 ? v00 : (c1 ? v01 : v02), uy = c0 ? v10 : (c1 ? v11 : v12), uz = c0 ? v20 : (c1 ? v21 : v22);
            const double l0 = fmax(c0 ? a00 : (c1 ? a11 : a22), 0.0), trace = (a00 + a11) + a22;
            if (mode == 1) {
                const double* c = centroid + (int64_t)p * 3;
                if (ux * (px - c[0]) + uy * (py - c[1]) + uz * (pz - c[2]) < 0.0) { ux = -ux; uy = -uy; uz = -uz; }
            } else if (mode == 2) {
                const float* v = view + (int64_t)p * 3;
                if (ux * ((double)v[0] - px) + uy * ((double)v[1] - py) + uz * ((double)v[2] - pz) < 0.0) { ux = -ux; uy = -uy; uz = -uz; }
            }
            if (isfinite(ux) && isfinite(uy) && isfinite(uz)) {       // a neighbourhood with a coordinate that is not finite has no normal
                nx = (float)ux; ny = (float)uy; nz = (float)uz;
                curv = trace > 0.0 ? (float)(l0 / trace) : __builtin_nanf("");
            }
        }
    }
    out[0] = nx; out[1] = ny; out[2] = nz;
    if (curvature) curvature[row] = curv;
}

// the mean in double of the correctly rounded fp32 roots of the valid slots (d2 not NaN), in slot order; `slots` = how many there were
__device__ __forceinline__ double geo_dbar(const float* __restrict__ d2, int k, int& slots) {
    double s = 0.0;
    int c = 0;
    for (int t = 0; t < k; ++t) {
        const float v = d2[t];
        if (v == v) { s += (double)sqrtf(v); c += 1; }
    }
    slots = c;
    return c > 0 ? s / (double)c : 0.0;
}

// grid (P).  method 0 (statistical): keep iff dbar <= mu + ratio sigma over the points of the cloud that have a dbar; method 1 (radius): keep
// iff at least min_neighbors slots have d2 <= radius * radius.  mask [P][N] (0 at and past the count), mean_distance [P][N] or null.
__global__ __launch_bounds__(256) void geo_outlier_kernel(const float* __restrict__ d2, const int* __restrict__ counts, int N, int k,
                                                          int method, double ratio, float radius, int min_neighbors,
                                                          unsigned char* __restrict__ mask, float* __restrict__ mean_distance) {
    __shared__ double sd[4];
    __shared__ int si[4];
    const int p = blockIdx.x, n = clamped_count(counts, p, N);
    const float* rows = d2 + (int64_t)p * N * k;
    unsigned char* keep = mask + (int64_t)p * N;
    if (mean_distance) {
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            int slots = 0;
            const double dbar = i < n ? geo_dbar(rows + (int64_t)i * k, k, slots) : 0.0;
            mean_distance[(int64_t)p * N + i] = slots > 0 ? (float)dbar : __builtin_nanf("");
        }
    }
    if (method == 1) {
        const float r2 = radius * radius;
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            int within = 0;
            if (i < n)
                for (int t = 0; t < k; ++t) within += rows[(int64_t)i * k + t] <= r2 ? 1 : 0;
            keep[i] = (i < n && within >= min_neighbors) ? 1 : 0;
        }
        return;
    }
    double s = 0.0;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        int slots = 0;
        const double dbar = geo_dbar(rows + (int64_t)i * k, k, slots);
        if (slots > 0) { s += dbar; c += 1; }
    }
    const int have = block_reduce<4>(c, SumOp(), si);
    const double mu = block_reduce<4>(s, SumOp(), sd) / (double)(have > 0 ? have : 1);
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        int slots = 0;
        const double dbar = geo_dbar(rows + (int64_t)i * k, k, slots);
        if (slots > 0) v += (dbar - mu) * (dbar - mu);
    }
    const double sigma = sqrt(block_reduce<4>(v, SumOp(), sd) / (double)(have > 0 ? have : 1));
    const double limit = mu + ratio * sigma;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        int slots = 0;
        const double dbar = i < n ? geo_dbar(rows + (int64_t)i * k, k, slots) : 0.0;
        keep[i] = (slots > 0 && dbar <= limit) ? 1 : 0;
    }
}

// grid (P): the rows below the count with a mask byte != 0, in their order, to the front of points_out (and attr_out); zeros behind them
__global__ __launch_bounds__(256) void geo_compact_kernel(const float* __restrict__ points, const float* __restrict__ attr,
                                                          const unsigned char* __restrict__ mask, const int* __restrict__ counts, int N,
                                                          float* __restrict__ points_out, float* __restrict__ attr_out,
                                                          int* __restrict__ counts_out) {
    __shared__ int wave_total[4];
    const int p = blockIdx.x, n = clamped_count(counts, p, N), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)p * N;
    int kept = 0;                                            // the same in every thread
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool flag = i < n && mask[base + i] != 0;
        const unsigned long long votes = __ballot(flag);
        const int before = __popcll(votes & ((1ull << lane) - 1ull));
        __syncthreads();                                     // the totals of the block before have been read
        if (lane == 0) wave_total[wave] = __popcll(votes);
        __syncthreads();
        int at = kept + before;
        for (int w = 0; w < 4; ++w) {
            at += w < wave ? wave_total[w] : 0;
            kept += wave_total[w];
        }
        if (flag) {
            const float* src = points + (base + i) * 3;
            float* dst = points_out + (base + at) * 3;
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            if (attr_out) {
                const float* asrc = attr + (base + i) * 3;
                float* adst = attr_out + (base + at) * 3;
                adst[0] = asrc[0]; adst[1] = asrc[1]; adst[2] = asrc[2];
            }
        }
    }
    for (int64_t e = (int64_t)kept * 3 + threadIdx.x; e < (int64_t)N * 3; e += blockDim.x) {
        points_out[base * 3 + e] = 0.f;
        if (attr_out) attr_out[base * 3 + e] = 0.f;
    }
    if (threadIdx.x == 0) counts_out[p] = kept;
}

#pragma clang fp contract(fast)

constexpr int GEO_MAX_CLOUDS = 65535;      // gridDim.y

static size_t geo_centroid_bytes(int clouds) { return align_up((size_t)clouds * 3 * sizeof(double)); }

template <int K>
static void knn_launch(const float* q, const int* nq, int nq_max, const float* t, const int* nt, int nt_max, int clouds, int k,
                       int exclude_self, float* d2, int* index, hipStream_t s) {
    hipLaunchKernelGGL(knn_kernel<K>, dim3((unsigned)ceil_div(nq_max, KNN_BLOCK), clouds), dim3(KNN_BLOCK), 0, s, q, nq, nq_max, t, nt,
                       nt_max, k, exclude_self, d2, index);
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_knn(const float* q, const int* nq, int nq_max, const float* t, const int* nt, int nt_max, int clouds, int k,
                       int exclude_self, float* d2, int32_t* index, void* stream) {
    PCD_CHECK_ARG(q && nq && t && nt && d2 && index);
    PCD_CHECK_ARG(clouds > 0 && clouds <= GEO_MAX_CLOUDS && nq_max > 0 && nt_max > 0);
    PCD_CHECK_ARG(k >= 1 && k <= PCD_KNN_MAX_K);
    hipStream_t s = (hipStream_t)stream;
    if (k <= 8) knn_launch<8>(q, nq, nq_max, t, nt, nt_max, clouds, k, exclude_self != 0, d2, index, s);
    else if (k <= 16) knn_launch<16>(q, nq, nq_max, t, nt, nt_max, clouds, k, exclude_self != 0, d2, index, s);
    else knn_launch<32>(q, nq, nq_max, t, nt, nt_max, clouds, k, exclude_self != 0, d2, index, s);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_cloud_normals_workspace_bytes(int clouds) {
    if (clouds <= 0 || clouds > GEO_MAX_CLOUDS) return 0;
    return geo_centroid_bytes(clouds);
}

extern "C" int pcd_cloud_normals(const float* points, const int* counts, int n_max, int clouds, const int32_t* index, int k, int mode,
                                 const float* viewpoints, float* normals, float* curvature, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    PCD_CHECK_ARG(points && counts && index && normals);
    PCD_CHECK_ARG(clouds > 0 && clouds <= GEO_MAX_CLOUDS && n_max > 0 && k >= 1 && k <= PCD_KNN_MAX_K);
    PCD_CHECK_ARG(mode == PCD_NORMALS_UNORIENTED || mode == PCD_NORMALS_OUTWARD || mode == PCD_NORMALS_TOWARD_VIEW);
    PCD_CHECK_ARG(mode != PCD_NORMALS_TOWARD_VIEW || viewpoints);
    PCD_CHECK_ARG(mode != PCD_NORMALS_OUTWARD || (workspace && workspace_bytes >= geo_centroid_bytes(clouds)));
    hipStream_t s = (hipStream_t)stream;
    double* centroid = (double*)workspace;
    if (mode == PCD_NORMALS_OUTWARD) hipLaunchKernelGGL(geo_centroid_kernel, dim3(clouds), dim3(256), 0, s, points, counts, n_max, centroid);
    hipLaunchKernelGGL(geo_normals_kernel, dim3((unsigned)ceil_div(n_max, 256), clouds), dim3(256), 0, s, points, counts, n_max, index, k, mode,
                       centroid, viewpoints, normals, curvature);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_cloud_outlier_mask(const float* d2, const int* counts, int n_max, int clouds, int k, int method, double std_ratio,
                                      float radius, int min_neighbors, uint8_t* mask, float* mean_distance, void* stream) {
    PCD_CHECK_ARG(d2 && counts && mask);
    PCD_CHECK_ARG(clouds > 0 && clouds <= GEO_MAX_CLOUDS && n_max > 0 && k >= 1 && k <= PCD_KNN_MAX_K);
    PCD_CHECK_ARG(method == PCD_OUTLIER_STATISTICAL || method == PCD_OUTLIER_RADIUS);
    PCD_CHECK_ARG(method != PCD_OUTLIER_STATISTICAL || isfinite(std_ratio));
    PCD_CHECK_ARG(method != PCD_OUTLIER_RADIUS || (isfinite(radius) && radius >= 0.f && min_neighbors >= 1 && min_neighbors <= k));
    hipLaunchKernelGGL(geo_outlier_kernel, dim3(clouds), dim3(256), 0, (hipStream_t)stream, d2, counts, n_max, k, method, std_ratio, radius,
                       min_neighbors, mask, mean_distance);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_cloud_compact(const float* points, const float* attr, const uint8_t* mask, const int* counts, int n_max, int clouds,
                                 float* points_out, float* attr_out, int* counts_out, void* stream) {
    PCD_CHECK_ARG(points && mask && counts && points_out && counts_out);
    PCD_CHECK_ARG((attr == nullptr) == (attr_out == nullptr));
    PCD_CHECK_ARG(points_out != points && (attr_out == nullptr || attr_out != attr));
    PCD_CHECK_ARG(clouds > 0 && clouds <= GEO_MAX_CLOUDS && n_max > 0);
    hipLaunchKernelGGL(geo_compact_kernel, dim3(clouds), dim3(256), 0, (hipStream_t)stream, points, attr, mask, counts, n_max, points_out,
                       attr_out, counts_out);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
