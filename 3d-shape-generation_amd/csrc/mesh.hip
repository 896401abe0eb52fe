// K12: surface-nets mesh extraction from occupancy-probability grids (DESIGN.md "Mesh output"; include/pcd_hip.h pcd_mesh_*).
// One workgroup per grid, as voxels_to_points_kernel: the cells of the zero-padded field are walked in row-major order, 4 x 1024 per pass,
// and every index (a cell's vertex number, a quad's row) comes from wave ballots plus one block scan per pass of the 64 (sub-pass, wave) counts
// -- no atomics, so the packed outputs are bitwise repeatable and a grid's mesh does not depend on what else is in the batch.
//
//   count: 8 corners -> side mask -> active cell / crossing edges; leaves each cell's vertex number (or -1) in the workspace
//   emit:  reads those numbers for the four cells round a crossing edge, recomputes the corners for the crossing points
//
// STAGED = true: the workgroup copies its grid into LDS once (32^3 fp32 = 128 KB of the CU's 160 KB) and serves the 8-corner reads
// from there; STAGED = false reads the grid through the vector cache (any grid; what a grid that does not fit LDS takes).
// fp32 throughout, true division for the crossing parameter, contraction off so both forms give the same bits.
#include "common.h"
#include <float.h>

namespace pcd {

#pragma clang fp contract(off)

constexpr int MESH_THREADS = 1024;
constexpr int MESH_WAVES = MESH_THREADS / 64;
constexpr int MESH_SUB = 4;                                    // sub-passes of 1024 cells between two block scans
constexpr int MESH_SLOTS = MESH_SUB * MESH_WAVES;              // = 64: one wave scans them with shuffles
constexpr size_t MESH_LDS_SCRATCH = 512;                       // two slot arrays, in front of the field (keeps it 16-byte aligned)
constexpr size_t MESH_LDS_FIELD_MAX = 144 * 1024;              // field bytes a workgroup stages; + scratch < 160 KB

static int g_mesh_staged = 1;                                  // pcd_mesh_config

struct MeshGrid {
    int d, h, w;                                               // unpadded extents
    int cd, ch, cw;                                            // cells per axis = extent + 1
    int64_t nvox, ncell;
};

// value of padded node (pz, py, px): the field inside, 0 in the one-node border
template <class Ptr>
__device__ __forceinline__ float mesh_node(Ptr f, const MeshGrid& g, int pz, int py, int px) {
    const int z = pz - 1, y = py - 1, x = px - 1;
    if ((unsigned)z >= (unsigned)g.d || (unsigned)y >= (unsigned)g.h || (unsigned)x >= (unsigned)g.w) return 0.f;
    return f[((int64_t)z * g.h + y) * g.w + x];
}

// the 8 corners of cell (cz, cy, cx), corner index 4 a + 2 b + c = padded node (cz + a, cy + b, cx + c); returns the inside mask
template <class Ptr>
__device__ __forceinline__ unsigned mesh_corners(Ptr f, const MeshGrid& g, int cz, int cy, int cx, float thr, float (&v)[8]) {
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[k] = mesh_node(f, g, cz + (k >> 2), cy + ((k >> 1) & 1), cx + (k & 1));
        mask |= (v[k] > thr ? 1u : 0u) << k;
    }
    return mask;
}

// does the edge from the cell's corner 0 (the padded node with the cell's index) along axis a (0 z, 1 y, 2 x) change side?  The four cells round
// such an edge always exist: the inside end is a node of the grid, so the node's other two padded coordinates are >= 1 (checked all the same, so
// that no index can leave the workspace whatever the field holds).
__device__ __forceinline__ bool mesh_crossing(unsigned mask, int a, int cz, int cy, int cx) {
    const int bit = a == 0 ? 4 : (a == 1 ? 2 : 1);
    const bool cross = ((mask ^ (mask >> bit)) & 1u) != 0;
    const bool room = a == 0 ? (cy >= 1 && cx >= 1) : (a == 1 ? (cx >= 1 && cz >= 1) : (cz >= 1 && cy >= 1));
    return cross && room;
}

__device__ __forceinline__ void mesh_stage(const float* __restrict__ src, float* dst, int64_t n) {
    if ((n & 3) == 0 && (((uintptr_t)src) & 15) == 0) {
        const f32x4* s4 = (const f32x4*)src;
        f32x4* d4 = (f32x4*)dst;
        for (int64_t i = threadIdx.x; i < (n >> 2); i += MESH_THREADS) d4[i] = s4[i];
    } else {
        for (int64_t i = threadIdx.x; i < n; i += MESH_THREADS) dst[i] = src[i];
    }
    __syncthreads();
}

// wave 0, after the barrier behind the slot writes: slot[j * 16 + wave] = number of items of wave `wave` in sub-pass j -> the index of that wave's
// first item (running total before this pass + exclusive scan in (sub-pass, wave) order = row-major cell order); returns the new running total
__device__ __forceinline__ int mesh_scan_slots(int* slot, int lane, int base) {
    const int own = slot[lane];
    int x = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    slot[lane] = base + x - own;
    return base + __shfl(x, 63);
}

template <bool STAGED>
__global__ __launch_bounds__(MESH_THREADS) void mesh_count_kernel(const float* __restrict__ vox, MeshGrid g, float thr,
                                                                   int32_t* __restrict__ cellnum, int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char mesh_lds[];
    int* slot_v = (int*)mesh_lds;                              // [4][16] vertices per (sub-pass, wave), then their first numbers
    int* slot_q = slot_v + MESH_SLOTS;                         // [4][16] quads per (sub-pass, wave)
    float* field = (float*)(mesh_lds + MESH_LDS_SCRATCH);
    const float* v = vox + (int64_t)blockIdx.x * g.nvox;
    int32_t* num = cellnum + (int64_t)blockIdx.x * g.ncell;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncell = (int)g.ncell, plane = g.cw * g.ch;       // 32-bit cell arithmetic: ncell <= (2^31 - 1) / 6 (mesh_args_ok)
    if (STAGED) mesh_stage(v, field, g.nvox);
    int vbase = 0, qbase = 0;                                  // running totals, kept by wave 0
    for (int c0 = 0; c0 < ncell; c0 += MESH_SUB * MESH_THREADS) {
        int before[MESH_SUB];                                  // -1: not active, else active cells in lower lanes of the wave
#pragma unroll
        for (int j = 0; j < MESH_SUB; ++j) {
            const int c = c0 + j * MESH_THREADS + (int)threadIdx.x;
            bool active = false, q0 = false, q1 = false, q2 = false;
            if (c < ncell) {
                const int cz = c / plane, r = c - cz * plane, cy = r / g.cw, cx = r - cy * g.cw;
                float cv[8];
                const unsigned mask = STAGED ? mesh_corners((const float*)field, g, cz, cy, cx, thr, cv) : mesh_corners(v, g, cz, cy, cx, thr, cv);
                active = mask != 0u && mask != 255u;
                q0 = mesh_crossing(mask, 0, cz, cy, cx);
                q1 = mesh_crossing(mask, 1, cz, cy, cx);
                q2 = mesh_crossing(mask, 2, cz, cy, cx);
            }
            const unsigned long long mv = __ballot(active);
            const unsigned long long m0 = __ballot(q0), m1 = __ballot(q1), m2 = __ballot(q2);
            if (lane == 0) {
                slot_v[j * MESH_WAVES + wave] = __popcll(mv);
                slot_q[j * MESH_WAVES + wave] = __popcll(m0) + __popcll(m1) + __popcll(m2);
            }
            before[j] = active ? __popcll(mv & ((1ull << lane) - 1ull)) : -1;
        }
        __syncthreads();
        if (wave == 0) {
            vbase = mesh_scan_slots(slot_v, lane, vbase);
            qbase = mesh_scan_slots(slot_q, lane, qbase);
        }
        __syncthreads();
        // a wave reads and (next pass) writes only its own slots; wave 0 rewrites them all only behind the next pass's first barrier
#pragma unroll
        for (int j = 0; j < MESH_SUB; ++j) {
            const int c = c0 + j * MESH_THREADS + (int)threadIdx.x;
            if (c < ncell) num[c] = before[j] >= 0 ? slot_v[j * MESH_WAVES + wave] + before[j] : -1;
        }
    }
    if (threadIdx.x == 0) {
        counts[blockIdx.x * 2] = vbase;
        counts[blockIdx.x * 2 + 1] = 2 * qbase;
    }
}

template <bool STAGED>
__global__ __launch_bounds__(MESH_THREADS) void mesh_emit_kernel(const float* __restrict__ vox, MeshGrid g, float thr,
                                                                  const int32_t* __restrict__ cellnum, const int64_t* __restrict__ offsets,
                                                                  float* __restrict__ vertices, int32_t* __restrict__ faces) {
    extern __shared__ __attribute__((aligned(16))) char mesh_lds[];
    int* slot_q = (int*)mesh_lds;                              // [4][16] quads per (sub-pass, wave), then their first rows
    float* field = (float*)(mesh_lds + MESH_LDS_SCRATCH);
    const float* v = vox + (int64_t)blockIdx.x * g.nvox;
    const int32_t* num = cellnum + (int64_t)blockIdx.x * g.ncell;
    float* vout = vertices + offsets[blockIdx.x * 2] * 3;
    int32_t* fout = faces + offsets[blockIdx.x * 2 + 1] * 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncell = (int)g.ncell, plane = g.cw * g.ch;       // cell strides: 1 (x), g.cw (y), plane (z)
    if (STAGED) mesh_stage(v, field, g.nvox);
    const float fw = (float)(g.w - 1), fh = (float)(g.h - 1), fd = (float)(g.d - 1);
    int qbase = 0;                                             // running quad total, kept by wave 0
    for (int c0 = 0; c0 < ncell; c0 += MESH_SUB * MESH_THREADS) {
        int qbits[MESH_SUB], before[MESH_SUB];                 // bits 0-2: crossing edge along z, y, x; bit 3: the cell's own node is inside
#pragma unroll
        for (int j = 0; j < MESH_SUB; ++j) {
            const int c = c0 + j * MESH_THREADS + (int)threadIdx.x;
            bool q[3] = {false, false, false};
            unsigned mask = 0;
            if (c < ncell) {
                const int cz = c / plane, r = c - cz * plane, cy = r / g.cw, cx = r - cy * g.cw;
                float cv[8];
                mask = STAGED ? mesh_corners((const float*)field, g, cz, cy, cx, thr, cv) : mesh_corners(v, g, cz, cy, cx, thr, cv);
#pragma unroll
                for (int a = 0; a < 3; ++a) q[a] = mesh_crossing(mask, a, cz, cy, cx);
                if (mask != 0u && mask != 255u) {
                    // mean of the crossing points of the edges whose ends differ in side, in index coordinates of the unpadded grid (padded - 1);
                    // edges in the order axis z, y, x, and within an axis by the corner index of the low end
                    const float oz = (float)(cz - 1), oy = (float)(cy - 1), ox = (float)(cx - 1);
                    float sumz = 0.f, sumy = 0.f, sumx = 0.f, n = 0.f;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const int bit = a == 0 ? 4 : (a == 1 ? 2 : 1);
#pragma unroll
                        for (int ka = 0; ka < 8; ++ka) {
                            if (ka & bit) continue;
                            const int kb = ka | bit;
                            if ((((mask >> ka) ^ (mask >> kb)) & 1u) == 0) continue;
                            const float t = (thr - cv[ka]) / (cv[kb] - cv[ka]);
                            sumz += oz + (a == 0 ? t : (float)(ka >> 2));
                            sumy += oy + (a == 1 ? t : (float)((ka >> 1) & 1));
                            sumx += ox + (a == 2 ? t : (float)(ka & 1));
                            n += 1.f;
                        }
                    }
                    const int vn = num[c];                     // >= 0: the count call saw the same field
                    if (vn >= 0) {
                        float* o = vout + (int64_t)vn * 3;
                        o[0] = (2.f * (sumx / n)) / fw - 1.f;  // the map of voxels_to_points_kernel
                        o[1] = (2.f * (sumy / n)) / fh - 1.f;
                        o[2] = (2.f * (sumz / n)) / fd - 1.f;
                    }
                }
            }
            const unsigned long long m0 = __ballot(q[0]), m1 = __ballot(q[1]), m2 = __ballot(q[2]);
            if (lane == 0) slot_q[j * MESH_WAVES + wave] = __popcll(m0) + __popcll(m1) + __popcll(m2);
            const unsigned long long below = (1ull << lane) - 1ull;
            before[j] = __popcll(m0 & below) + __popcll(m1 & below) + __popcll(m2 & below);
            qbits[j] = (q[0] ? 1 : 0) | (q[1] ? 2 : 0) | (q[2] ? 4 : 0) | ((mask & 1u) ? 8 : 0);
        }
        __syncthreads();
        if (wave == 0) qbase = mesh_scan_slots(slot_q, lane, qbase);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MESH_SUB; ++j) {
            if ((qbits[j] & 7) == 0) continue;
            const int c = c0 + j * MESH_THREADS + (int)threadIdx.x;
            int row = slot_q[j * MESH_WAVES + wave] + before[j];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!((qbits[j] >> a) & 1)) continue;
                // (u, w) = the two axes that follow a cyclically; the cells (-1, -1), (0, -1), (0, 0), (-1, 0) on them
                const int su = a == 0 ? g.cw : (a == 1 ? 1 : plane), sw = a == 0 ? 1 : (a == 1 ? plane : g.cw);
                int n0 = num[c - su - sw], n1 = num[c - sw], n2 = num[c], n3 = num[c - su];
                if (qbits[j] & 8) { int t = n0; n0 = n3; n3 = t; t = n1; n1 = n2; n2 = t; }     // inside node: outward normals in the [x, y, z] rows that leave
                int32_t* o = fout + (int64_t)row * 6;
                o[0] = n0; o[1] = n1; o[2] = n2;
                o[3] = n0; o[4] = n2; o[5] = n3;
                ++row;
            }
        }
    }
}
#pragma clang fp contract(fast)

static bool mesh_args_ok(int batch, int d, int h, int w) {
    // vertex numbers and triangle counts are int32: 6 triangles per cell at the very most
    return batch > 0 && d > 1 && h > 1 && w > 1 && (int64_t)(d + 1) * (h + 1) * (w + 1) <= 0x7fffffff / 6;
}

static MeshGrid mesh_grid(int d, int h, int w) {
    MeshGrid g;
    g.d = d; g.h = h; g.w = w;
    g.cd = d + 1; g.ch = h + 1; g.cw = w + 1;
    g.nvox = (int64_t)d * h * w;
    g.ncell = (int64_t)g.cd * g.ch * g.cw;
    return g;
}

static bool mesh_fits_lds(const MeshGrid& g) { return g_mesh_staged && (size_t)g.nvox * sizeof(float) <= MESH_LDS_FIELD_MAX; }

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_mesh_config(int code) {
    PCD_CHECK_ARG(code == 0 || code == 1);
    g_mesh_staged = code;
    return PCD_OK;
}

extern "C" size_t pcd_mesh_workspace_bytes(int batch, int d, int h, int w) {
    if (!mesh_args_ok(batch, d, h, w)) return 0;
    return (size_t)batch * (size_t)(d + 1) * (h + 1) * (w + 1) * sizeof(int32_t);
}

extern "C" int pcd_mesh_count(const float* vox, int batch, int d, int h, int w, float threshold, void* workspace, int32_t* counts,
                              void* stream) {
    PCD_CHECK_ARG(vox && workspace && counts && mesh_args_ok(batch, d, h, w));
    PCD_CHECK_ARG(threshold > 0.f && threshold <= FLT_MAX);
    const MeshGrid g = mesh_grid(d, h, w);
    if (mesh_fits_lds(g)) {
        const size_t lds = MESH_LDS_SCRATCH + (size_t)g.nvox * sizeof(float);
        static PcdLdsOnce once;
        PCD_CHECK_HIP(pcd_allow_lds(once, (const void*)mesh_count_kernel<true>, (int)(MESH_LDS_SCRATCH + MESH_LDS_FIELD_MAX)));
        hipLaunchKernelGGL(mesh_count_kernel<true>, dim3(batch), dim3(MESH_THREADS), lds, (hipStream_t)stream, vox, g, threshold,
                           (int32_t*)workspace, counts);
    } else {
        hipLaunchKernelGGL(mesh_count_kernel<false>, dim3(batch), dim3(MESH_THREADS), MESH_LDS_SCRATCH, (hipStream_t)stream, vox, g,
                           threshold, (int32_t*)workspace, counts);
    }
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_mesh_emit(const float* vox, int batch, int d, int h, int w, float threshold, const void* workspace,
                             const int64_t* offsets, float* vertices, int32_t* faces, void* stream) {
    PCD_CHECK_ARG(vox && workspace && offsets && vertices && faces && mesh_args_ok(batch, d, h, w));
    PCD_CHECK_ARG(threshold > 0.f && threshold <= FLT_MAX);
    const MeshGrid g = mesh_grid(d, h, w);
    if (mesh_fits_lds(g)) {
        const size_t lds = MESH_LDS_SCRATCH + (size_t)g.nvox * sizeof(float);
        static PcdLdsOnce once;
        PCD_CHECK_HIP(pcd_allow_lds(once, (const void*)mesh_emit_kernel<true>, (int)(MESH_LDS_SCRATCH + MESH_LDS_FIELD_MAX)));
        hipLaunchKernelGGL(mesh_emit_kernel<true>, dim3(batch), dim3(MESH_THREADS), lds, (hipStream_t)stream, vox, g, threshold,
                           (const int32_t*)workspace, offsets, vertices, faces);
    } else {
        hipLaunchKernelGGL(mesh_emit_kernel<false>, dim3(batch), dim3(MESH_THREADS), MESH_LDS_SCRATCH, (hipStream_t)stream, vox, g,
                           threshold, (const int32_t*)workspace, offsets, vertices, faces);
    }
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
