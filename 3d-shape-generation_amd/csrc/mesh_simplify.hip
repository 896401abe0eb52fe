// Mesh simplification by vertex clustering with quadric-optimal representatives on packed mesh batches (definitions in DESIGN.md "Mesh
// simplification"; Lindstrom 2000).  Integer atomics only: the slot a key lands in and the order a row is filled in depend on arrival, nothing
// that is read back does -- roots are minima, rows are sorted by rank before they are summed, every floating-point sum runs in ascending
// index order and every loop is bounded by the sizes.  Tables that atomics wrote are read by plain loads only in a later launch.
#include "mesh_rows.h"
#include <cmath>

namespace pcd {

#pragma clang fp contract(off)

namespace {

constexpr int MS_MAX_R = PCD_MESH_SIMPLIFY_MAX_RESOLUTION;
constexpr int MS_MAX_V = PCD_MESH_SIMPLIFY_MAX_VERTICES;         // three roots fit one 64-bit key of the duplicate table
constexpr int MS_ROUNDS = 10;                                    // bisection rounds: 1 .. 1025 halves to one resolution
constexpr int MS_LONG_ROW = 1024;                                // member rows above this are sorted by a workgroup, the others by a wave
constexpr int MS_GRID_WORDS = 8;                                 // per mesh: lo[3], ext, h (float), R, bisection lo, hi (int)
constexpr uint32_t MS_EMPTY = 0xffffffffu;
constexpr unsigned long long MS_EMPTY64 = ~0ull;
enum { MS_PHASE_GIVEN = 0, MS_PHASE_MID = 1, MS_PHASE_FOUND = 2 };

// a mesh at or above the vertex limit is refused on the host; on the device it counts as empty, so no key can overflow
__device__ __forceinline__ MoMesh ms_mesh(const int64_t* __restrict__ offsets, int b) {
    MoMesh m = mo_mesh(offsets, b);
    if (m.nv >= MS_MAX_V) m.nv = m.nf = 0;
    return m;
}

__device__ __forceinline__ uint32_t ms_hash(uint32_t k) {
    k *= 2654435761u;
    return k ^ (k >> 15);
}

__device__ __forceinline__ uint32_t ms_hash64(unsigned long long k) {
    k *= 0x9e3779b97f4a7c15ull;
    return (uint32_t)(k >> 32);
}

// ---------------------------------------------------------------------------------------------------------------- incidence, boxes
// per valid face, one incidence per corner: cnt > 0 is "referenced", and the counts are the incidence rows' lengths
__global__ __launch_bounds__(MO_THREADS) void ms_inc_count_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ offsets,
                                                                  int batch, int32_t* __restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= offsets[batch * 2 + 1]) return;
    const MoMesh m = ms_mesh(offsets, mo_find(offsets, batch, t, 1));
    int a, b, c;
    if (t - m.f0 >= m.nf || !mo_face(faces + m.f0 * 3, (int)(t - m.f0), m.nv, a, b, c)) return;
    atomicAdd(&cnt[m.v0 + a], 1);
    atomicAdd(&cnt[m.v0 + b], 1);
    atomicAdd(&cnt[m.v0 + c], 1);
}

// lo, hi over the referenced vertices by comparisons that are false for NaN, from +inf / -inf; ext the largest hi - lo, from -inf
__global__ __launch_bounds__(MO_WG) void ms_box_kernel(const float* __restrict__ vertices, const int64_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ cnt, int32_t* __restrict__ grid,
                                                       int32_t* __restrict__ fcount) {
    __shared__ float part[MO_WAVES][6];
    const MoMesh m = ms_mesh(offsets, blockIdx.x);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
        if (cnt[m.v0 + v] <= 0) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = vertices[(m.v0 + v) * 3 + k];
            if (x < lo[k]) lo[k] = x;
            if (x > hi[k]) hi[k] = x;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                                // no NaN in here: fminf / fmaxf are plain minima
        lo[k] = wave_reduce(lo[k], MinOp());
        hi[k] = wave_reduce(hi[k], MaxOp());
        if ((threadIdx.x & 63) == 0) {
            part[threadIdx.x >> 6][k] = lo[k];
            part[threadIdx.x >> 6][3 + k] = hi[k];
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float ext = -INFINITY;
    float* g = (float*)(grid + (int64_t)blockIdx.x * MS_GRID_WORDS);
    for (int k = 0; k < 3; ++k) {
        float l = part[0][k], h = part[0][3 + k];
        for (int w = 1; w < MO_WAVES; ++w) {
            l = fminf(l, part[w][k]);
            h = fmaxf(h, part[w][3 + k]);
        }
        const float d = h - l;
        if (d > ext) ext = d;
        g[k] = l;
    }
    g[3] = ext;
    grid[(int64_t)blockIdx.x * MS_GRID_WORDS + 6] = 1;
    grid[(int64_t)blockIdx.x * MS_GRID_WORDS + 7] = MS_MAX_R + 1;
    fcount[blockIdx.x] = 0;
}

// the resolution and cell size of every mesh for the launches that follow
__global__ __launch_bounds__(MO_THREADS) void ms_grid_kernel(int batch, int mode, int phase, const void* __restrict__ params,
                                                             int32_t* __restrict__ grid) {
    const int b = blockIdx.x * MO_THREADS + threadIdx.x;
    if (b >= batch) return;
    int32_t* gi = grid + (int64_t)b * MS_GRID_WORDS;
    float* gf = (float*)gi;
    const float ext = gf[3];
    int r;
    float h;
    if (mode == PCD_MESH_SIMPLIFY_CELL_SIZE) {
        const float c = ((const float*)params)[b];
        if (!(c > 0.f) || !std::isfinite(c)) {                                   // refused before the call; bounded here all the same
            r = 1;
            h = 1.f;
        } else {
            h = c;
            const float e = ext / h;
            r = !std::isfinite(ext) ? 1 : (e >= (float)(MS_MAX_R - 1) ? MS_MAX_R : (int)floorf(e) + 1);
            r = r < 1 ? 1 : r;
        }
    } else {
        if (mode == PCD_MESH_SIMPLIFY_RESOLUTION) r = ((const int32_t*)params)[b];
        else r = phase == MS_PHASE_MID ? (gi[6] + gi[7]) / 2 : gi[6];
        r = r < 1 ? 1 : (r > MS_MAX_R ? MS_MAX_R : r);
        h = ext / (float)r;
        if (ext == 0.f || !std::isfinite(ext)) h = 1.f;
    }
    gf[4] = h;
    gi[5] = r;
}

__device__ __forceinline__ int ms_cell(float x, float lo, float h, int r) {
    const float q = (x - lo) / h;
    if (!(q >= 0.f)) return 0;
    if (q >= (float)r) return r - 1;
    return (int)floorf(q);
}

// ---------------------------------------------------------------------------------------------------------------- clusters
// Per referenced vertex the key of its cell, and the key's slot of the mesh's own table (2 V slots from 2 v0) takes the least vertex index.
// Only the values atomicCAS returns are looked at here; the table is read by the next launch.
__global__ __launch_bounds__(MO_THREADS) void ms_key_kernel(const float* __restrict__ vertices, const int64_t* __restrict__ offsets, int batch,
                                                            const int32_t* __restrict__ cnt, const int32_t* __restrict__ grid,
                                                            int32_t* __restrict__ key, uint32_t* __restrict__ tkey,
                                                            uint32_t* __restrict__ troot) {
    const int64_t g = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (g >= offsets[batch * 2]) return;
    const int b = mo_find(offsets, batch, g, 0);
    const MoMesh m = ms_mesh(offsets, b);
    if (g - m.v0 >= m.nv || cnt[g] <= 0) {
        key[g] = -1;
        return;
    }
    const float* gf = (const float*)(grid + (int64_t)b * MS_GRID_WORDS);
    const float h = gf[4];
    const int r = grid[(int64_t)b * MS_GRID_WORDS + 5];
    const int cx = ms_cell(vertices[g * 3], gf[0], h, r), cy = ms_cell(vertices[g * 3 + 1], gf[1], h, r),
              cz = ms_cell(vertices[g * 3 + 2], gf[2], h, r);
    const uint32_t k = (uint32_t)((cz * r + cy) * r + cx);
    key[g] = (int32_t)k;
    const uint32_t slots = 2u * (uint32_t)m.nv;
    uint32_t s = ms_hash(k) % slots;
    for (uint32_t i = 0; i < slots; ++i) {
        const uint32_t old = atomicCAS(&tkey[m.v0 * 2 + s], MS_EMPTY, k);
        if (old == MS_EMPTY || old == k) {
            atomicMin(&troot[m.v0 * 2 + s], (uint32_t)(g - m.v0));
            return;
        }
        s = s + 1 == slots ? 0 : s + 1;
    }
}

// the root of every vertex (the least index of its cluster, -1 unreferenced) and the flag the cluster numbers are scanned from;
// row sum V of the flags closes the scan
__global__ __launch_bounds__(MO_THREADS) void ms_root_kernel(const int64_t* __restrict__ offsets, int batch, const int32_t* __restrict__ key,
                                                             const uint32_t* __restrict__ tkey, const uint32_t* __restrict__ troot,
                                                             int32_t* __restrict__ root, int32_t* __restrict__ isroot) {
    const int64_t g = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    const int64_t total = offsets[batch * 2];
    if (g > total) return;
    if (g == total) {
        isroot[g] = 0;
        return;
    }
    const MoMesh m = ms_mesh(offsets, mo_find(offsets, batch, g, 0));
    int found = -1;
    const int32_t k = key[g];
    if (g - m.v0 < m.nv && k >= 0) {
        const uint32_t slots = 2u * (uint32_t)m.nv;
        uint32_t s = ms_hash((uint32_t)k) % slots;
        for (uint32_t i = 0; i < slots; ++i) {
            const uint32_t have = tkey[m.v0 * 2 + s];
            if (have == (uint32_t)k) {
                found = (int)troot[m.v0 * 2 + s];
                break;
            }
            if (have == MS_EMPTY) break;                                         // every referenced vertex was inserted: not reached
            s = s + 1 == slots ? 0 : s + 1;
        }
        if ((unsigned)found >= (unsigned)m.nv) found = -1;
    }
    root[g] = found;
    isroot[g] = found >= 0 && found == (int)(g - m.v0);
}

// ---------------------------------------------------------------------------------------------------------------- faces
// A valid face whose three roots differ survives; with `dedup` only the one of least index among those with the same rotated triple of
// roots (roots and cluster numbers are in the same order, so the smallest root in front is the smallest number in front).
// COUNT: adds the survivors to fcount (a new key in the table is one survivor).  Otherwise: keepf = 1 for a survivor so far, and with
// dedup the key's slot in fslot and the least face index in dmin, for ms_count_kernel.
template <bool COUNT>
__global__ __launch_bounds__(MO_THREADS) void ms_face_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ offsets, int batch,
                                                             const int32_t* __restrict__ root, int dedup,
                                                             unsigned long long* __restrict__ dkey, uint32_t* __restrict__ dmin,
                                                             int32_t* __restrict__ fslot, int32_t* __restrict__ keepf,
                                                             int32_t* __restrict__ fcount) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    int b = -1, keep = 0;
    if (t < offsets[batch * 2 + 1]) {
        b = mo_find(offsets, batch, t, 1);
        const MoMesh m = ms_mesh(offsets, b);
        int a, bb, c;
        if (t - m.f0 < m.nf && mo_face(faces + m.f0 * 3, (int)(t - m.f0), m.nv, a, bb, c)) {
            const int ra = root[m.v0 + a], rb = root[m.v0 + bb], rc = root[m.v0 + c];
            keep = ra >= 0 && rb >= 0 && rc >= 0 && ra != rb && rb != rc && ra != rc;
            if (keep && dedup) {
                int p = ra, q = rb, s3 = rc;
                if (rb < ra && rb < rc) { p = rb; q = rc; s3 = ra; }
                else if (rc < ra && rc < rb) { p = rc; q = ra; s3 = rb; }
                const unsigned long long k = ((unsigned long long)p << 42) | ((unsigned long long)q << 21) | (unsigned long long)s3;
                const uint32_t slots = 2u * (uint32_t)m.nf;
                uint32_t s = ms_hash64(k) % slots;
                bool fresh = false;
                for (uint32_t i = 0; i < slots; ++i) {
                    const unsigned long long old = atomicCAS(&dkey[m.f0 * 2 + s], MS_EMPTY64, k);
                    if (old == MS_EMPTY64 || old == k) {
                        fresh = old == MS_EMPTY64;
                        break;
                    }
                    s = s + 1 == slots ? 0 : s + 1;
                }
                if (COUNT) keep = fresh;
                else {
                    atomicMin(&dmin[m.f0 * 2 + s], (uint32_t)(t - m.f0));
                    fslot[t] = (int32_t)s;
                }
            }
        }
        if (!COUNT) keepf[t] = keep;
    }
    if (COUNT) {                                                                 // one add per wave where the wave lies in one mesh
        const int b0 = __shfl(b, 0);
        if (__all(!keep || b == b0)) {
            const int n = __popcll(__ballot(keep));
            if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(&fcount[b0], n);
        } else if (keep) {
            atomicAdd(&fcount[b], 1);
        }
    }
}

__global__ __launch_bounds__(MO_THREADS) void ms_bisect_kernel(int batch, const int32_t* __restrict__ target, int32_t* __restrict__ grid,
                                                               int32_t* __restrict__ fcount) {
    const int b = blockIdx.x * MO_THREADS + threadIdx.x;
    if (b >= batch) return;
    int32_t* gi = grid + (int64_t)b * MS_GRID_WORDS;
    const int mid = (gi[6] + gi[7]) / 2, want = target[b] < 0 ? 0 : target[b];
    if (fcount[b] <= want) gi[6] = mid; else gi[7] = mid;
    fcount[b] = 0;
}

// per mesh: the map vertex -> cluster number, the final keep flag of every face, counts = (clusters, surviving faces), the resolution
__global__ __launch_bounds__(MO_WG) void ms_count_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ root,
                                                         const int32_t* __restrict__ cscan, int dedup, const uint32_t* __restrict__ dmin,
                                                         const int32_t* __restrict__ fslot, const int32_t* __restrict__ grid,
                                                         int32_t* __restrict__ keepf, int32_t* __restrict__ map, int32_t* __restrict__ counts,
                                                         int32_t* __restrict__ resolutions) {
    __shared__ int wsum[MO_WAVES];
    const MoMesh m = ms_mesh(offsets, blockIdx.x);
    const int c0 = cscan[m.v0];
    for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
        const int r = root[m.v0 + v];
        map[m.v0 + v] = r >= 0 ? cscan[m.v0 + r] - c0 : -1;
    }
    int nf = 0;
    for (int f0 = 0; f0 < m.nf; f0 += MO_WG) {
        const int t = f0 + threadIdx.x;
        int k = 0, total;
        if (t < m.nf) {
            k = keepf[m.f0 + t];
            if (k && dedup) k = dmin[m.f0 * 2 + fslot[m.f0 + t]] == (uint32_t)t;
            keepf[m.f0 + t] = k;
        }
        block_scan_excl<MO_WAVES>(k, wsum, &total);
        nf += total;
    }
    if (threadIdx.x == 0) {
        counts[blockIdx.x * 2] = cscan[m.v0 + m.nv] - c0;
        counts[blockIdx.x * 2 + 1] = nf;
        resolutions[blockIdx.x] = grid[(int64_t)blockIdx.x * MS_GRID_WORDS + 5];
    }
}

// ---------------------------------------------------------------------------------------------------------------- rows
// rows in arrival order: the incident faces of a vertex (row g from start[g]) ...
__global__ __launch_bounds__(MO_THREADS) void ms_inc_fill_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ offsets,
                                                                 int batch, const int32_t* __restrict__ inc_start, int32_t* __restrict__ cursor,
                                                                 int32_t* __restrict__ inc_raw) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= offsets[batch * 2 + 1]) return;
    const MoMesh m = ms_mesh(offsets, mo_find(offsets, batch, t, 1));
    int q[3];
    const int fl = (int)(t - m.f0);
    if (t - m.f0 >= m.nf || !mo_face(faces + m.f0 * 3, fl, m.nv, q[0], q[1], q[2])) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t g = m.v0 + q[k];
        inc_raw[(int64_t)inc_start[g] + atomicAdd(&cursor[g], 1)] = fl;
    }
}

// ... and the members of a cluster (row c, the packed cluster number, holding packed vertex rows)
template <bool FILL>
__global__ __launch_bounds__(MO_THREADS) void ms_member_kernel(const int64_t* __restrict__ offsets, int batch, const int32_t* __restrict__ root,
                                                               const int32_t* __restrict__ cscan, const int32_t* __restrict__ cstart,
                                                               int32_t* __restrict__ ccount, int32_t* __restrict__ mem_raw) {
    const int64_t g = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (g >= offsets[batch * 2]) return;
    const MoMesh m = ms_mesh(offsets, mo_find(offsets, batch, g, 0));
    const int r = root[g];
    if (g - m.v0 >= m.nv || r < 0) return;
    const int c = cscan[m.v0 + r];
    const int at = atomicAdd(&ccount[c], 1);
    if (FILL) mem_raw[(int64_t)cstart[c] + at] = (int32_t)g;
}

// Row `row` sorted by rank over the T threads of the caller: entry i goes to the number of smaller entries (the entries are unique).
template <int T>
__device__ __forceinline__ void ms_rank_sort(const int32_t* __restrict__ raw, int32_t* __restrict__ sorted, int n, int tid) {
    for (int i = tid; i < n; i += T) {
        const int x = raw[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += raw[j] < x;
        sorted[r] = x;
    }
}

// one wave per row; with LONG_LIST rows above MS_LONG_ROW are left to ms_long_sort_kernel and listed for it (in arrival order, which only
// decides which workgroup sorts which row)
template <bool LONG_LIST>
__global__ __launch_bounds__(MO_THREADS) void ms_row_sort_kernel(const int32_t* __restrict__ nrows, int64_t rows, const int32_t* __restrict__ start,
                                                                 const int32_t* __restrict__ raw, int32_t* __restrict__ sorted,
                                                                 int32_t* __restrict__ nlong, int32_t* __restrict__ long_list) {
    const int64_t c = (int64_t)blockIdx.x * (MO_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= (LONG_LIST ? (int64_t)*nrows : rows)) return;                       // the clusters are counted on the device
    const int n = start[c + 1] - start[c];
    if (LONG_LIST && n > MS_LONG_ROW) {
        if ((threadIdx.x & 63) == 0) long_list[atomicAdd(nlong, 1)] = (int32_t)c;
        return;
    }
    ms_rank_sort<64>(raw + start[c], sorted + start[c], n, threadIdx.x & 63);
}

__global__ __launch_bounds__(MO_WG) void ms_long_sort_kernel(const int32_t* __restrict__ nlong, const int32_t* __restrict__ long_list,
                                                             const int32_t* __restrict__ start, const int32_t* __restrict__ raw,
                                                             int32_t* __restrict__ sorted) {
    if ((int)blockIdx.x >= *nlong) return;
    const int c = long_list[blockIdx.x];
    ms_rank_sort<MO_WG>(raw + start[c], sorted + start[c], start[c + 1] - start[c], threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------- quadrics
// q = A00 A01 A02 A11 A12 A22 b0 b1 b2 of one face, in double from the fp32 corners; false where the face has no area
__device__ __forceinline__ bool ms_face_quadric(const float* __restrict__ x, int a, int b, int c, double* q) {
    const double ax = x[(int64_t)a * 3], ay = x[(int64_t)a * 3 + 1], az = x[(int64_t)a * 3 + 2];
    const double e1x = (double)x[(int64_t)b * 3] - ax, e1y = (double)x[(int64_t)b * 3 + 1] - ay, e1z = (double)x[(int64_t)b * 3 + 2] - az;
    const double e2x = (double)x[(int64_t)c * 3] - ax, e2y = (double)x[(int64_t)c * 3 + 1] - ay, e2z = (double)x[(int64_t)c * 3 + 2] - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (len == 0.0) return false;
    const double ux = nx / len, uy = ny / len, uz = nz / len, w = 0.5 * len;
    const double d = (ux * ax + uy * ay) + uz * az;
    const double wx = w * ux, wy = w * uy, wz = w * uz, wd = w * d;
    q[0] = wx * ux; q[1] = wx * uy; q[2] = wx * uz;
    q[3] = wy * uy; q[4] = wy * uz; q[5] = wz * uz;
    q[6] = wd * ux; q[7] = wd * uy; q[8] = wd * uz;
    return true;
}

// the quadric of every vertex: its incident valid faces' in ascending face order, from +0
__global__ __launch_bounds__(MO_THREADS) void ms_vertex_quadric_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                       const int64_t* __restrict__ offsets, int batch,
                                                                       const int32_t* __restrict__ inc_start,
                                                                       const int32_t* __restrict__ inc_sorted, double* __restrict__ vq) {
    const int64_t g = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (g >= offsets[batch * 2]) return;
    const MoMesh m = ms_mesh(offsets, mo_find(offsets, batch, g, 0));
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (g - m.v0 < m.nv) {
        const float* x = vertices + m.v0 * 3;
        const int32_t* fc = faces + m.f0 * 3;
        const int r0 = inc_start[g], n = inc_start[g + 1] - r0;
        for (int i = 0; i < n; ++i) {
            const int t = inc_sorted[r0 + i];
            int a, b, c;
            double q[9];
            if ((unsigned)t >= (unsigned)m.nf || !mo_face(fc, t, m.nv, a, b, c) || !ms_face_quadric(x, a, b, c, q)) continue;
#pragma unroll
            for (int k = 0; k < 9; ++k) s[k] = s[k] + q[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) vq[g * 9 + k] = s[k];
}

// One thread per cluster: the members' quadrics, positions and count summed in ascending vertex order, then the representative.
__global__ __launch_bounds__(MO_THREADS) void ms_cluster_kernel(const float* __restrict__ vertices, const int64_t* __restrict__ offsets, int batch,
                                                                const int32_t* __restrict__ cscan, const int32_t* __restrict__ cstart,
                                                                const int32_t* __restrict__ members, const double* __restrict__ vq,
                                                                const int32_t* __restrict__ key, const int32_t* __restrict__ grid,
                                                                int placement, const int64_t* __restrict__ out_offsets,
                                                                float* __restrict__ out_vertices) {
    const int64_t total = offsets[batch * 2];
    const int64_t c = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (c >= cscan[total]) return;
    const int r0 = cstart[c], n = cstart[c + 1] - r0;
    if (n <= 0) return;
    const int64_t g0 = members[r0];                                              // the root
    if (g0 < 0 || g0 >= total) return;
    const int b = mo_find(offsets, batch, g0, 0);
    const int64_t v0 = offsets[b * 2];
    double s[3] = {0.0, 0.0, 0.0}, q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i) {
        const int64_t g = members[r0 + i];
        if (g < 0 || g >= total) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = s[k] + (double)vertices[g * 3 + k];
        if (placement == PCD_MESH_SIMPLIFY_QUADRIC) {
#pragma unroll
            for (int k = 0; k < 9; ++k) q[k] = q[k] + vq[g * 9 + k];
        }
    }
    const double cnt = (double)n;
    const double mean[3] = {s[0] / cnt, s[1] / cnt, s[2] / cnt};
    double p[3] = {mean[0], mean[1], mean[2]};
    const double tr = (q[0] + q[3]) + q[5];
    if (placement == PCD_MESH_SIMPLIFY_QUADRIC && tr > 0.0) {
        const double reg = 1e-3 * tr;
        const double a00 = q[0] + reg, a01 = q[1], a02 = q[2], a11 = q[3] + reg, a12 = q[4], a22 = q[5] + reg;
        const double b0 = q[6] + reg * mean[0], b1 = q[7] + reg * mean[1], b2 = q[8] + reg * mean[2];
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = (a00 * c00 + a01 * c01) + a02 * c02;
        const double sol[3] = {((c00 * b0 + c01 * b1) + c02 * b2) / det, ((c01 * b0 + c11 * b1) + c12 * b2) / det,
                               ((c02 * b0 + c12 * b1) + c22 * b2) / det};
        const float* gf = (const float*)(grid + (int64_t)b * MS_GRID_WORDS);
        const int r = grid[(int64_t)b * MS_GRID_WORDS + 5];
        const int k0 = key[g0];
        const int cell[3] = {k0 % r, (k0 / r) % r, k0 / (r * r)};
        const double h = (double)gf[4];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double low = (double)gf[k] + ((double)cell[k] - 0.5) * h, high = (double)gf[k] + ((double)cell[k] + 1.5) * h;
            ok = ok && std::isfinite(sol[k]) && sol[k] >= low && sol[k] <= high;
        }
        if (ok) {
            p[0] = sol[0]; p[1] = sol[1]; p[2] = sol[2];
        }
    }
    float* o = out_vertices + (out_offsets[b * 2] + (c - cscan[v0])) * 3;
    o[0] = (float)p[0];
    o[1] = (float)p[1];
    o[2] = (float)p[2];
}

// the surviving faces of a mesh in input order, corner by corner through the map
__global__ __launch_bounds__(MO_WG) void ms_emit_faces_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ keepf, const int32_t* __restrict__ root,
                                                              const int32_t* __restrict__ cscan, const int64_t* __restrict__ out_offsets,
                                                              int32_t* __restrict__ out_faces) {
    __shared__ int wsum[MO_WAVES];
    const MoMesh m = ms_mesh(offsets, blockIdx.x);
    const int64_t of = out_offsets[blockIdx.x * 2 + 1];
    const int32_t* fc = faces + m.f0 * 3;
    const int c0 = cscan[m.v0];
    int base = 0;
    for (int f0 = 0; f0 < m.nf; f0 += MO_WG) {
        const int t = f0 + threadIdx.x;
        int a = 0, b = 0, c = 0, total;
        const int k = t < m.nf && keepf[m.f0 + t] != 0 && mo_face(fc, t, m.nv, a, b, c);
        const int e = block_scan_excl<MO_WAVES>(k, wsum, &total);
        if (k) {
            int32_t* o = out_faces + (of + base + e) * 3;
            o[0] = cscan[m.v0 + root[m.v0 + a]] - c0;
            o[1] = cscan[m.v0 + root[m.v0 + b]] - c0;
            o[2] = cscan[m.v0 + root[m.v0 + c]] - c0;
        }
        base += total;
    }
}

// ---------------------------------------------------------------------------------------------------------------- workspace
struct MsWorkspace {
    size_t grid, fcount, nlong, cnt, cursor, ccount, zero_end, isroot, cscan, cstart, inc_start, key, root, members_raw, members, long_list,
        partial, keepf, fslot, inc_raw, inc_sorted, tkey, troot, table_end, dkey, dmin, dedup_end, vq, total;
};

MsWorkspace ms_workspace(int batch, int64_t total_vertices, int64_t total_faces) {
    MsWorkspace w;
    size_t o = 0;
    const size_t rows = (size_t)total_vertices + 1, tv = (size_t)total_vertices, tf = (size_t)total_faces, i4 = sizeof(int32_t);
    w.grid = o;         o += align_up((size_t)batch * MS_GRID_WORDS * i4);
    w.fcount = o;       o += align_up((size_t)batch * i4);
    w.nlong = o;        o += align_up(i4);                                        // nlong .. zero_end: cleared together
    w.cnt = o;          o += align_up(rows * i4);
    w.cursor = o;       o += align_up(rows * i4);
    w.ccount = o;       o += align_up(rows * i4);
    w.zero_end = o;
    w.isroot = o;       o += align_up(rows * i4);
    w.cscan = o;        o += align_up(rows * i4);
    w.cstart = o;       o += align_up(rows * i4);
    w.inc_start = o;    o += align_up(rows * i4);
    w.key = o;          o += align_up(rows * i4);
    w.root = o;         o += align_up(rows * i4);
    w.members_raw = o;  o += align_up(rows * i4);
    w.members = o;      o += align_up(rows * i4);
    w.long_list = o;    o += align_up((tv / MS_LONG_ROW + 1) * i4);
    w.partial = o;      o += align_up((size_t)ceil_div((int64_t)rows, MO_WG) * i4);
    w.keepf = o;        o += align_up((tf + 1) * i4);
    w.fslot = o;        o += align_up((tf + 1) * i4);
    w.inc_raw = o;      o += align_up((tf * 3 + 1) * i4);
    w.inc_sorted = o;   o += align_up((tf * 3 + 1) * i4);
    w.tkey = o;         o += align_up((tv * 2 + 1) * i4);                         // tkey .. table_end: set to all ones together
    w.troot = o;        o += align_up((tv * 2 + 1) * i4);
    w.table_end = o;
    w.dkey = o;         o += align_up((tf * 2 + 1) * sizeof(unsigned long long));  // dkey .. dedup_end likewise
    w.dmin = o;         o += align_up((tf * 2 + 1) * i4);
    w.dedup_end = o;
    w.vq = o;           o += align_up((tv * 9 + 1) * sizeof(double));
    w.total = o;
    return w;
}

bool ms_sizes_ok(int batch, int64_t total_vertices, int64_t total_faces, int64_t max_vertices) {
    return mo_sizes_ok(batch, total_vertices, total_faces) && max_vertices >= 0 && max_vertices <= total_vertices &&
           max_vertices < MS_MAX_V;
}

// keys, roots and the root flags at the resolutions ms_grid_kernel last wrote; with `dedup` the duplicate table is cleared for the faces
int ms_cluster(const float* vertices, const int64_t* offsets, int batch, int64_t tv, int dedup, char* ws, const MsWorkspace& w, hipStream_t s) {
    PCD_CHECK_HIP(hipMemsetAsync(ws + w.tkey, 0xff, w.table_end - w.tkey, s));
    if (dedup) PCD_CHECK_HIP(hipMemsetAsync(ws + w.dkey, 0xff, w.dedup_end - w.dkey, s));
    if (tv > 0) {
        hipLaunchKernelGGL(ms_key_kernel, dim3((unsigned)ceil_div(tv, MO_THREADS)), dim3(MO_THREADS), 0, s, vertices, offsets, batch,
                           (const int32_t*)(ws + w.cnt), (const int32_t*)(ws + w.grid), (int32_t*)(ws + w.key), (uint32_t*)(ws + w.tkey),
                           (uint32_t*)(ws + w.troot));
        PCD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ms_root_kernel, dim3((unsigned)ceil_div(tv + 1, MO_THREADS)), dim3(MO_THREADS), 0, s, offsets, batch,
                       (const int32_t*)(ws + w.key), (const uint32_t*)(ws + w.tkey), (const uint32_t*)(ws + w.troot), (int32_t*)(ws + w.root),
                       (int32_t*)(ws + w.isroot));
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

}  // namespace

#pragma clang fp contract(fast)

}  // namespace pcd

using namespace pcd;

extern "C" size_t pcd_mesh_simplify_workspace_bytes(int batch, int64_t total_vertices, int64_t total_faces) {
    if (!mo_sizes_ok(batch, total_vertices, total_faces)) return 0;
    return ms_workspace(batch, total_vertices, total_faces).total;
}

extern "C" int pcd_mesh_simplify_count(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices,
                                       int64_t total_faces, int64_t max_vertices, int mode, const void* params, int deduplicate,
                                       void* workspace, size_t workspace_bytes, int32_t* resolutions, int32_t* map, int32_t* counts,
                                       void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && params && workspace && resolutions && map && counts);
    PCD_CHECK_ARG(mode == PCD_MESH_SIMPLIFY_RESOLUTION || mode == PCD_MESH_SIMPLIFY_CELL_SIZE || mode == PCD_MESH_SIMPLIFY_TARGET_FACES);
    PCD_CHECK_ARG(deduplicate == 0 || deduplicate == 1);
    PCD_CHECK_ARG(ms_sizes_ok(batch, total_vertices, total_faces, max_vertices));
    const MsWorkspace w = ms_workspace(batch, total_vertices, total_faces);
    if (workspace_bytes < w.total) {
        set_error("pcd_mesh_simplify_count: workspace of %zu bytes, %zu needed", workspace_bytes, w.total);
        return PCD_ERR_WORKSPACE;
    }
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int32_t* grid = (int32_t*)(ws + w.grid);
    int32_t* fcount = (int32_t*)(ws + w.fcount);
    int32_t* cnt = (int32_t*)(ws + w.cnt);
    int32_t* root = (int32_t*)(ws + w.root);
    int32_t* keepf = (int32_t*)(ws + w.keepf);
    int32_t* fslot = (int32_t*)(ws + w.fslot);
    unsigned long long* dkey = (unsigned long long*)(ws + w.dkey);
    uint32_t* dmin = (uint32_t*)(ws + w.dmin);
    const int64_t tv = total_vertices, tf = total_faces;
    const unsigned fblocks = (unsigned)ceil_div(tf, MO_THREADS), bblocks = (unsigned)ceil_div(batch, MO_THREADS);
    int rc;
    PCD_CHECK_HIP(hipMemsetAsync(ws + w.nlong, 0, w.zero_end - w.nlong, s));
    if (tf > 0) {
        hipLaunchKernelGGL(ms_inc_count_kernel, dim3(fblocks), dim3(MO_THREADS), 0, s, faces, offsets, batch, cnt);
        PCD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ms_box_kernel, dim3(batch), dim3(MO_WG), 0, s, vertices, offsets, (const int32_t*)cnt, grid, fcount);
    PCD_CHECK_LAUNCH();
    if (mode == PCD_MESH_SIMPLIFY_TARGET_FACES) {
        for (int round = 0; round < MS_ROUNDS; ++round) {
            hipLaunchKernelGGL(ms_grid_kernel, dim3(bblocks), dim3(MO_THREADS), 0, s, batch, mode, (int)MS_PHASE_MID, params, grid);
            PCD_CHECK_LAUNCH();
            PCD_RUN(ms_cluster(vertices, offsets, batch, tv, deduplicate, ws, w, s));
            if (tf > 0) {
                hipLaunchKernelGGL(ms_face_kernel<true>, dim3(fblocks), dim3(MO_THREADS), 0, s, faces, offsets, batch, (const int32_t*)root,
                                   deduplicate, dkey, dmin, fslot, keepf, fcount);
                PCD_CHECK_LAUNCH();
            }
            hipLaunchKernelGGL(ms_bisect_kernel, dim3(bblocks), dim3(MO_THREADS), 0, s, batch, (const int32_t*)params, grid, fcount);
            PCD_CHECK_LAUNCH();
        }
    }
    hipLaunchKernelGGL(ms_grid_kernel, dim3(bblocks), dim3(MO_THREADS), 0, s, batch, mode,
                       (int)(mode == PCD_MESH_SIMPLIFY_TARGET_FACES ? MS_PHASE_FOUND : MS_PHASE_GIVEN), params, grid);
    PCD_CHECK_LAUNCH();
    PCD_RUN(ms_cluster(vertices, offsets, batch, tv, deduplicate, ws, w, s));
    PCD_RUN(mo_scan((const int32_t*)(ws + w.isroot), (int32_t*)(ws + w.cscan), tv + 1, (int32_t*)(ws + w.partial), s));
    if (tf > 0) {
        hipLaunchKernelGGL(ms_face_kernel<false>, dim3(fblocks), dim3(MO_THREADS), 0, s, faces, offsets, batch, (const int32_t*)root,
                           deduplicate, dkey, dmin, fslot, keepf, fcount);
        PCD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ms_count_kernel, dim3(batch), dim3(MO_WG), 0, s, offsets, (const int32_t*)root, (const int32_t*)(ws + w.cscan),
                       deduplicate, (const uint32_t*)dmin, (const int32_t*)fslot, (const int32_t*)grid, keepf, map, counts, resolutions);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_mesh_simplify_emit(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices,
                                      int64_t total_faces, int64_t max_vertices, int placement, void* workspace, size_t workspace_bytes,
                                      const int64_t* out_offsets, float* out_vertices, int32_t* out_faces, void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && workspace && out_offsets && out_vertices && out_faces);
    PCD_CHECK_ARG(placement == PCD_MESH_SIMPLIFY_QUADRIC || placement == PCD_MESH_SIMPLIFY_MEAN);
    PCD_CHECK_ARG(ms_sizes_ok(batch, total_vertices, total_faces, max_vertices));
    const MsWorkspace w = ms_workspace(batch, total_vertices, total_faces);
    if (workspace_bytes < w.total) {
        set_error("pcd_mesh_simplify_emit: workspace of %zu bytes, %zu needed", workspace_bytes, w.total);
        return PCD_ERR_WORKSPACE;
    }
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int64_t tv = total_vertices, tf = total_faces;
    const unsigned fblocks = (unsigned)ceil_div(tf, MO_THREADS), vblocks = (unsigned)ceil_div(tv, MO_THREADS),
                   wblocks = (unsigned)ceil_div(tv, MO_THREADS / 64);
    const int32_t* cnt = (const int32_t*)(ws + w.cnt);
    const int32_t* root = (const int32_t*)(ws + w.root);
    const int32_t* cscan = (const int32_t*)(ws + w.cscan);
    int32_t* cursor = (int32_t*)(ws + w.cursor);
    int32_t* ccount = (int32_t*)(ws + w.ccount);
    int32_t* cstart = (int32_t*)(ws + w.cstart);
    int32_t* inc_start = (int32_t*)(ws + w.inc_start);
    int32_t* members_raw = (int32_t*)(ws + w.members_raw);
    int32_t* members = (int32_t*)(ws + w.members);
    int32_t* nlong = (int32_t*)(ws + w.nlong);
    int32_t* long_list = (int32_t*)(ws + w.long_list);
    int32_t* partial = (int32_t*)(ws + w.partial);
    int32_t* inc_raw = (int32_t*)(ws + w.inc_raw);
    int32_t* inc_sorted = (int32_t*)(ws + w.inc_sorted);
    double* vq = (double*)(ws + w.vq);
    int rc;
    if (tv > 0) {
        PCD_CHECK_HIP(hipMemsetAsync(nlong, 0, w.cnt - w.nlong, s));
        PCD_CHECK_HIP(hipMemsetAsync(cursor, 0, w.zero_end - w.cursor, s));       // the counts of pcd_mesh_simplify_count stay
        if (placement == PCD_MESH_SIMPLIFY_QUADRIC) {
            PCD_RUN(mo_scan(cnt, inc_start, tv + 1, partial, s));
            if (tf > 0) {
                hipLaunchKernelGGL(ms_inc_fill_kernel, dim3(fblocks), dim3(MO_THREADS), 0, s, faces, offsets, batch, (const int32_t*)inc_start,
                                   cursor, inc_raw);
                PCD_CHECK_LAUNCH();
            }
            hipLaunchKernelGGL(ms_row_sort_kernel<false>, dim3(wblocks), dim3(MO_THREADS), 0, s, (const int32_t*)nullptr, tv,
                               (const int32_t*)inc_start, (const int32_t*)inc_raw, inc_sorted, nlong, long_list);
            PCD_CHECK_LAUNCH();
            hipLaunchKernelGGL(ms_vertex_quadric_kernel, dim3(vblocks), dim3(MO_THREADS), 0, s, vertices, faces, offsets, batch,
                               (const int32_t*)inc_start, (const int32_t*)inc_sorted, vq);
            PCD_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(ms_member_kernel<false>, dim3(vblocks), dim3(MO_THREADS), 0, s, offsets, batch, root, cscan, (const int32_t*)cstart,
                           ccount, members_raw);
        PCD_CHECK_LAUNCH();
        PCD_RUN(mo_scan(ccount, cstart, tv + 1, partial, s));
        PCD_CHECK_HIP(hipMemsetAsync(ccount, 0, w.zero_end - w.ccount, s));
        hipLaunchKernelGGL(ms_member_kernel<true>, dim3(vblocks), dim3(MO_THREADS), 0, s, offsets, batch, root, cscan, (const int32_t*)cstart,
                           ccount, members_raw);
        PCD_CHECK_LAUNCH();
        hipLaunchKernelGGL(ms_row_sort_kernel<true>, dim3(wblocks), dim3(MO_THREADS), 0, s, cscan + tv, tv, (const int32_t*)cstart,
                           (const int32_t*)members_raw, members, nlong, long_list);
        PCD_CHECK_LAUNCH();
        hipLaunchKernelGGL(ms_long_sort_kernel, dim3((unsigned)(tv / MS_LONG_ROW + 1)), dim3(MO_WG), 0, s, (const int32_t*)nlong,
                           (const int32_t*)long_list, (const int32_t*)cstart, (const int32_t*)members_raw, members);
        PCD_CHECK_LAUNCH();
        hipLaunchKernelGGL(ms_cluster_kernel, dim3(vblocks), dim3(MO_THREADS), 0, s, vertices, offsets, batch, cscan, (const int32_t*)cstart,
                           (const int32_t*)members, (const double*)vq, (const int32_t*)(ws + w.key), (const int32_t*)(ws + w.grid), placement,
                           out_offsets, out_vertices);
        PCD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ms_emit_faces_kernel, dim3(batch), dim3(MO_WG), 0, s, faces, offsets, (const int32_t*)(ws + w.keepf), root, cscan,
                       out_offsets, out_faces);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
