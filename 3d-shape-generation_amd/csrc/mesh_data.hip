// Device-resident mesh dataset (include/pcd_hip.h: pcd_mesh_area_sums, pcd_mesh_batch_clouds; DESIGN.md "Mesh dataset"): a table of packed triangle
// meshes and their running area sums stays on the device, and one launch turns an index vector into a batch of freshly drawn surface clouds.
//
// pcd_mesh_batch_clouds: one workgroup of 1024 lanes per batch slot; lane t owns the points i = t, t + 1024, ... in every pass, so nothing a lane
// reads was written by another one and the passes need no barrier beyond those of the reductions.  A point is drawn as pcd_mesh_sample_points draws
// it (Philox counter -> u0, u1, u2 -> binary search of the mesh's running sums -> barycentric point); the mesh's slice of the sums is staged in LDS
// when it has at most 4096 faces.  The chain (rotate, jitter, normalize) is dataset.hip's.  Two forms, same bits: up to 8192 points the slot's cloud
// is kept in LDS (x[N], y[N], z[N]: lane-strided 4-byte accesses, conflict free) and rewritten in place by the augmentation; above that, or under
// pcd_mesh_data_config(0), every pass draws its points again from the counters, as dataset.hip does with its voxels.
#include "common.h"
#include "mesh_tri.h"
#include <cmath>

namespace pcd {

constexpr int MDT_THREADS = 1024;
constexpr int MDT_WAVES = MDT_THREADS / 64;
constexpr int MDT_LDS_POINTS = 8192;                           // 96 KB of the CU's 160 KB
constexpr int MDT_CDF_LDS = 4096;                              // running sums of a mesh up to this many faces are searched in LDS

static int g_mesh_data_resident = 1;


// the slot's mesh, uniform over the workgroup
struct MdtMesh {
    const float* v;
    const int32_t* f;
    const float* c;                                            // inclusive running sums of its nf areas (global memory or the LDS copy)
    int nf;
    int64_t nv;
    float total;
};

// what a slot's run is made of, uniform over the workgroup
struct MdtSlot {
    uint64_t seed, ctr0;                                       // ctr0: first counter of the slot's span
    int flags;
    float sigma, clip;
    float mean0[3], rad0;                                      // centroid and radius of the drawn cloud
    float cs, sn;                                              // rotation
    float mean1[3], rad1;                                      // centroid and radius of the augmented cloud
};

#pragma clang fp contract(off)
// point i of the slot, its face and that face's unit normal: mesh_sample_kernel's arithmetic, operation by operation (total > 0 here)
__device__ __forceinline__ int mdt_draw(const MdtMesh& m, uint64_t seed, uint64_t ctr, float (&p)[3], float (&n)[3]) {
    uint32_t w[4];
    philox_words4(ctr, seed, w);
    const float u0 = (float)(w[0] >> 8) * (1.0f / 16777216.0f);
    const float u1 = (float)(w[1] >> 8) * (1.0f / 16777216.0f);
    const float u2 = (float)(w[2] >> 8) * (1.0f / 16777216.0f);
    const float target = u0 * m.total;
    int l = 0, h = m.nf - 1;                                   // the first face whose running sum exceeds the target (the last at most)
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (m.c[mid] > target) h = mid; else l = mid + 1;
    }
    const float s = sqrtf(fminf(fmaxf(u1, 0.f), 1.f));
    const float t = fminf(fmaxf(u2, 0.f), 1.f);
    p[0] = p[1] = p[2] = 0.f;
    n[0] = n[1] = n[2] = 0.f;
    const MinTri q = min_load_tri(m.v, m.f, l, m.nv, 0.f, 1.f);
    if (q.ok) {
        const float wa = 1.f - s, wb = s * (1.f - t), wc = s * t;
        p[0] = (wa * q.ax + wb * q.bx) + wc * q.cx;
        p[1] = (wa * q.ay + wb * q.by) + wc * q.cy;
        p[2] = (wa * q.az + wb * q.bz) + wc * q.cz;
        const float ux = q.bx - q.ax, uy = q.by - q.ay, uz = q.bz - q.az;
        const float vx = q.cx - q.ax, vy = q.cy - q.ay, vz = q.cz - q.az;
        const float mx = uy * vz - uz * vy, my = uz * vx - ux * vz, mz = ux * vy - uy * vx;
        const float len = sqrtf((mx * mx + my * my) + mz * mz);
        if (len > 0.f && len <= 3.0e38f) { n[0] = mx / len; n[1] = my / len; n[2] = mz / len; }
    }
    return l;
}

// squared distance from m: (d0^2 + d1^2) + d2^2
__device__ __forceinline__ float mdt_dist2(const float (&p)[3], const float (&m)[3]) {
    const float a = p[0] - m[0], b = p[1] - m[1], c = p[2] - m[2];
    return (a * a + b * b) + c * c;
}

__device__ __forceinline__ void mdt_normalize(float (&p)[3], const float (&mean)[3], float rad) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = ((p[c] - mean[c]) / rad);
}

// right-multiplication by [[c, 0, s], [0, 1, 0], [-s, 0, c]]
__device__ __forceinline__ void mdt_rotate(const MdtSlot& s, float (&p)[3]) {
    const float p0 = p[0], p2 = p[2];
    p[0] = p0 * s.cs - p2 * s.sn;
    p[2] = p0 * s.sn + p2 * s.cs;
}

// drawn point i -> the point after rotation and jitter (before the last normalisation)
__device__ __forceinline__ void mdt_augment(const MdtSlot& s, int i, float (&p)[3]) {
    if (s.flags & PCD_VOXEL_ROTATE) {
        mdt_normalize(p, s.mean0, s.rad0);
        mdt_rotate(s, p);
    }
    if (s.flags & PCD_VOXEL_JITTER) {
        float v[4];
        philox_normals4(s.ctr0 + PCD_MESH_CTR_JITTER + (uint64_t)i, s.seed, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] += fminf(fmaxf(s.sigma * v[c], -s.clip), s.clip);
    }
}

// centroid and radius of the n points get(i, p): lane t adds its points t, t + 1024, ... in ascending i to a partial that starts at 0, the partials
// are added over the lanes of a wave by the xor butterfly 32, 16, 8, 4, 2, 1 and the 16 wave sums in ascending wave order; mean = sum / n;
// radius = sqrt(max of the squared distances)
template <class Get>
__device__ __forceinline__ void mdt_centroid_radius(Get get, int n, float* wave_f, float (&mean)[3], float& rad) {
    float acc[3] = {0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n; i += MDT_THREADS) {
        float p[3];
        get(i, p);
        acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2];
    }
    for (int c = 0; c < 3; ++c) mean[c] = (block_reduce(acc[c], SumOp(), wave_f)) / (float)n;
    float d2 = 0.f;
    for (int i = threadIdx.x; i < n; i += MDT_THREADS) {
        float p[3];
        get(i, p);
        d2 = fmaxf(d2, mdt_dist2(p, mean));
    }
    rad = sqrtf(block_reduce(d2, MaxOp(), wave_f));            // the correctly rounded root is monotonic: max of the roots = root of the max
}
#pragma clang fp contract(fast)

template <bool RESIDENT>
__global__ __launch_bounds__(MDT_THREADS) void mesh_batch_clouds_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                         const int64_t* __restrict__ offsets, int n_meshes,
                                                                         const float* __restrict__ area_sums, const int* __restrict__ index,
                                                                         int n_points, uint64_t seed, uint64_t offset, int flags, float sigma,
                                                                         float clip, float* __restrict__ out, float* __restrict__ normals,
                                                                         int32_t* __restrict__ face_index) {
    extern __shared__ __attribute__((aligned(16))) float mdt_cloud[];          // RESIDENT: x[N], y[N], z[N]
    __shared__ float cdf_lds[MDT_CDF_LDS];
    __shared__ float wave_f[MDT_WAVES];
    const int t = threadIdx.x, b = blockIdx.x, N = n_points;
    float* __restrict__ rows = out + (size_t)b * N * 3;
    float* __restrict__ nrm = normals != nullptr ? normals + (size_t)b * N * 3 : nullptr;
    int32_t* __restrict__ fidx = face_index != nullptr ? face_index + (size_t)b * N : nullptr;

    // ---------------------------------------------------------------- the slot's mesh (everything here is uniform over the workgroup)
    MdtMesh m;
    m.v = vertices; m.f = faces; m.c = area_sums; m.nf = 0; m.nv = 0; m.total = 0.f;
    const int g = index[b];
    int64_t f0 = 0;
    if (g >= 0 && g < n_meshes) {
        const int64_t v0 = offsets[(int64_t)g * 2];
        f0 = offsets[(int64_t)g * 2 + 1];
        const int64_t nv = offsets[(int64_t)g * 2 + 2] - v0, nf64 = offsets[(int64_t)g * 2 + 3] - f0;
        if (nv > 0 && nf64 > 0 && nf64 <= 0x7fffffff) {
            m.v = vertices + v0 * 3; m.f = faces + f0 * 3; m.c = area_sums + f0; m.nf = (int)nf64; m.nv = nv;
            m.total = area_sums[f0 + nf64 - 1];
        }
    }
    if (!(m.total > 0.f)) {                      // an index outside the table, a mesh without faces or without area: zero rows, zero normals, face -1
        for (int i = t; i < N * 3; i += MDT_THREADS) {
            rows[i] = 0.f;
            if (nrm != nullptr) nrm[i] = 0.f;
        }
        if (fidx != nullptr)
            for (int i = t; i < N; i += MDT_THREADS) fidx[i] = -1;
        return;
    }
    if (m.nf <= MDT_CDF_LDS) {
        for (int i = t; i < m.nf; i += MDT_THREADS) cdf_lds[i] = m.c[i];
        m.c = cdf_lds;
        __syncthreads();
    }

    MdtSlot s;
    s.seed = seed; s.ctr0 = offset + (uint64_t)b * PCD_MESH_CTR_SPAN; s.flags = flags; s.sigma = sigma; s.clip = clip;
    s.rad0 = s.rad1 = 1.f; s.cs = 1.f; s.sn = 0.f;
    for (int c = 0; c < 3; ++c) s.mean0[c] = s.mean1[c] = 0.f;
    if (flags & PCD_VOXEL_ROTATE) {
        uint32_t c[4];
        philox_words4(s.ctr0 + PCD_MESH_CTR_ANGLE, seed, c);
        const float u = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        sincosf(6.28318530717958647692f * u, &s.sn, &s.cs);
    }
    const uint64_t ctr_point = s.ctr0 + PCD_MESH_CTR_POINT;

    // ---------------------------------------------------------------- draw: faces and normals leave here, the points too when there is no chain
    for (int i = t; i < N; i += MDT_THREADS) {
        float p[3], n[3];
        const int face = mdt_draw(m, seed, ctr_point + (uint64_t)i, p, n);
        if (flags == 0) { rows[i * 3] = p[0]; rows[i * 3 + 1] = p[1]; rows[i * 3 + 2] = p[2]; }
        if (RESIDENT) { mdt_cloud[i] = p[0]; mdt_cloud[N + i] = p[1]; mdt_cloud[2 * N + i] = p[2]; }
        if (nrm != nullptr) {
            if (flags & PCD_VOXEL_ROTATE) mdt_rotate(s, n);
            nrm[i * 3] = n[0]; nrm[i * 3 + 1] = n[1]; nrm[i * 3 + 2] = n[2];
        }
        if (fidx != nullptr) fidx[i] = face;
    }
    if (flags == 0) return;

    auto drawn = [&](int i, float (&p)[3]) {
        if (RESIDENT) {
            p[0] = mdt_cloud[i]; p[1] = mdt_cloud[N + i]; p[2] = mdt_cloud[2 * N + i];
        } else {
            float n[3];
            mdt_draw(m, seed, ctr_point + (uint64_t)i, p, n);
        }
    };
    const bool augmented = (flags & (PCD_VOXEL_ROTATE | PCD_VOXEL_JITTER)) != 0;
    // ---------------------------------------------------------------- centroid and radius of the drawn cloud
    if ((flags & PCD_VOXEL_ROTATE) || !augmented) mdt_centroid_radius(drawn, N, wave_f, s.mean0, s.rad0);
    if (!augmented) {                            // normalize alone
        for (int i = t; i < N; i += MDT_THREADS) {
            float p[3];
            drawn(i, p);
            mdt_normalize(p, s.mean0, s.rad0);
            rows[i * 3] = p[0]; rows[i * 3 + 1] = p[1]; rows[i * 3 + 2] = p[2];
        }
        return;
    }
    // ---------------------------------------------------------------- rotate, jitter: in place in LDS, or again in every pass
    if (RESIDENT) {
        for (int i = t; i < N; i += MDT_THREADS) {
            float p[3];
            drawn(i, p);
            mdt_augment(s, i, p);
            mdt_cloud[i] = p[0]; mdt_cloud[N + i] = p[1]; mdt_cloud[2 * N + i] = p[2];
        }
    }
    auto augmented_point = [&](int i, float (&p)[3]) {
        drawn(i, p);
        if (!RESIDENT) mdt_augment(s, i, p);
    };
    if (flags & PCD_VOXEL_NORMALIZE) mdt_centroid_radius(augmented_point, N, wave_f, s.mean1, s.rad1);
    for (int i = t; i < N; i += MDT_THREADS) {
        float p[3];
        augmented_point(i, p);
        if (flags & PCD_VOXEL_NORMALIZE) mdt_normalize(p, s.mean1, s.rad1);
        rows[i * 3] = p[0]; rows[i * 3 + 1] = p[1]; rows[i * 3 + 2] = p[2];
    }
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_mesh_data_config(int code) {
    PCD_CHECK_ARG(code == 0 || code == 1);
    g_mesh_data_resident = code;
    return PCD_OK;
}

extern "C" int pcd_mesh_area_sums(const float* vertices, const int32_t* faces, const int64_t* offsets, int n_meshes, float* area_sums,
                                  void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && area_sums && n_meshes > 0);
    return mesh_area_scan_launch(vertices, faces, offsets, n_meshes, area_sums, (hipStream_t)stream);
}

extern "C" int pcd_mesh_batch_clouds(const float* vertices, const int32_t* faces, const int64_t* offsets, int n_meshes, const float* area_sums,
                                     const int* index, int batch, int num_points, uint64_t seed, uint64_t offset, int flags, float sigma,
                                     float clip, float* out, float* normals, int32_t* face_index, void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && area_sums && index && out);
    PCD_CHECK_ARG(n_meshes > 0 && batch > 0 && num_points > 0 && num_points <= PCD_MESH_MAX_POINTS);
    PCD_CHECK_ARG((flags & ~(PCD_VOXEL_NORMALIZE | PCD_VOXEL_ROTATE | PCD_VOXEL_JITTER)) == 0);
    PCD_CHECK_ARG(std::isfinite(sigma) && std::isfinite(clip));
    if (g_mesh_data_resident && flags != 0 && num_points <= MDT_LDS_POINTS) {
        static PcdLdsOnce once;
        PCD_CHECK_HIP(pcd_allow_lds(once, (const void*)mesh_batch_clouds_kernel<true>, MDT_LDS_POINTS * 3 * (int)sizeof(float)));
        hipLaunchKernelGGL(mesh_batch_clouds_kernel<true>, dim3(batch), dim3(MDT_THREADS), (size_t)num_points * 3 * sizeof(float),
                           (hipStream_t)stream, vertices, faces, offsets, n_meshes, area_sums, index, num_points, seed, offset, flags, sigma, clip,
                           out, normals, face_index);
    } else {
        hipLaunchKernelGGL(mesh_batch_clouds_kernel<false>, dim3(batch), dim3(MDT_THREADS), 0, (hipStream_t)stream, vertices, faces, offsets,
                           n_meshes, area_sums, index, num_points, seed, offset, flags, sigma, clip, out, normals, face_index);
    }
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
