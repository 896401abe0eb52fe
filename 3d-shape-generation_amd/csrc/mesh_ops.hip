// Mesh processing on packed mesh batches (definitions in DESIGN.md "Mesh processing"): vertex rings, Taubin smoothing, vertex normals,
// connected components, compaction and measures.  Integer atomics only, every floating-point sum in a fixed order, every loop bounded
// by the sizes: bitwise repeatable, and a mesh gets in a batch what it gets alone.
#include "mesh_rows.h"
#include <cmath>

namespace pcd {

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------------------------- device scan
// out[i] = in[0] + ... + in[i - 1] for i < n, three launches: chunks of MO_WG, the chunk sums, the add.
__global__ __launch_bounds__(MO_WG) void mo_scan_chunks_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t n,
                                                               int32_t* __restrict__ partial) {
    __shared__ int wsum[MO_WAVES];
    const int64_t i = (int64_t)blockIdx.x * MO_WG + threadIdx.x;
    const int x = i < n ? in[i] : 0;
    int total;
    const int e = block_scan_excl<MO_WAVES>(x, wsum, &total);
    if (i < n) out[i] = e;
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(MO_WG) void mo_scan_partials_kernel(int32_t* __restrict__ partial, int chunks) {
    __shared__ int wsum[MO_WAVES];
    int base = 0;
    for (int c0 = 0; c0 < chunks; c0 += MO_WG) {
        const int i = c0 + threadIdx.x;
        const int x = i < chunks ? partial[i] : 0;
        int total;
        const int e = block_scan_excl<MO_WAVES>(x, wsum, &total);
        if (i < chunks) partial[i] = base + e;
        base += total;
    }
}

__global__ __launch_bounds__(MO_WG) void mo_scan_add_kernel(int32_t* __restrict__ out, int64_t n, const int32_t* __restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * MO_WG + threadIdx.x;
    if (i < n) out[i] += partial[blockIdx.x];
}

int mo_scan(const int32_t* in, int32_t* out, int64_t n, int32_t* partial, hipStream_t stream) {
    const int chunks = (int)ceil_div(n, MO_WG);
    hipLaunchKernelGGL(mo_scan_chunks_kernel, dim3(chunks), dim3(MO_WG), 0, stream, in, out, n, partial);
    PCD_CHECK_LAUNCH();
    hipLaunchKernelGGL(mo_scan_partials_kernel, dim3(1), dim3(MO_WG), 0, stream, partial, chunks);
    PCD_CHECK_LAUNCH();
    hipLaunchKernelGGL(mo_scan_add_kernel, dim3(chunks), dim3(MO_WG), 0, stream, out, n, partial);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

namespace {

constexpr int MO_FLAG_REFERENCED = 1, MO_FLAG_BOUNDARY = 2, MO_FLAG_IRREGULAR = 4;
constexpr int MO_NO_LABEL = 0x7fffffff;

int g_labels_form = 0;                                           // pcd_mesh_ops_config: 0 LDS where they fit, 1 always the workspace

// ---------------------------------------------------------------------------------------------------------------- adjacency
// launch 1: per valid face, one incidence per corner
__global__ __launch_bounds__(MO_THREADS) void mo_adj_count_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ offsets,
                                                                  int batch, int32_t* __restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= offsets[batch * 2 + 1]) return;
    const MoMesh m = mo_mesh(offsets, mo_find(offsets, batch, t, 1));
    int a, b, c;
    if (t - m.f0 >= m.nf || !mo_face(faces + m.f0 * 3, (int)(t - m.f0), m.nv, a, b, c)) return;
    atomicAdd(&cnt[m.v0 + a], 1);
    atomicAdd(&cnt[m.v0 + b], 1);
    atomicAdd(&cnt[m.v0 + c], 1);
}

// a raw ring entry of vertex a: neighbour u, the face, and whether the face holds u -> a (1) or a -> u (0); unique within a's row
__device__ __forceinline__ int64_t mo_key(int u, int face, int in) { return ((int64_t)u << 32) | ((int64_t)face << 1) | in; }

// launch 2: the rows in arrival order (sorted by the next launch): per corner the face, and the two ring entries the face gives it
__global__ __launch_bounds__(MO_THREADS) void mo_adj_fill_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ offsets,
                                                                 int batch, const int32_t* __restrict__ inc_start, int32_t* __restrict__ cursor,
                                                                 int32_t* __restrict__ inc_raw, int64_t* __restrict__ raw) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= offsets[batch * 2 + 1]) return;
    const MoMesh m = mo_mesh(offsets, mo_find(offsets, batch, t, 1));
    int q[3];
    const int fl = (int)(t - m.f0);
    if (t - m.f0 >= m.nf || !mo_face(faces + m.f0 * 3, fl, m.nv, q[0], q[1], q[2])) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t g = m.v0 + q[k];
        const int64_t slot = (int64_t)inc_start[g] + atomicAdd(&cursor[g], 1);
        inc_raw[slot] = fl;
        raw[slot * 2] = mo_key(q[(k + 1) % 3], fl, 0);
        raw[slot * 2 + 1] = mo_key(q[(k + 2) % 3], fl, 1);
    }
}

// launch 3: one wave per vertex sorts its rows by rank (entry i goes to the number of smaller entries: n^2 / 64 steps, any row length) and
// counts the distinct neighbours
__global__ __launch_bounds__(MO_THREADS) void mo_adj_sort_kernel(int64_t total_vertices, const int32_t* __restrict__ inc_start,
                                                                 const int32_t* __restrict__ inc_raw, const int64_t* __restrict__ raw,
                                                                 int32_t* __restrict__ inc_faces, int64_t* __restrict__ sorted,
                                                                 int32_t* __restrict__ deg) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (MO_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= total_vertices) return;
    const int64_t base = inc_start[g];
    const int n = inc_start[g + 1] - inc_start[g];
    for (int i = lane; i < n; i += 64) {
        const int fi = inc_raw[base + i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += inc_raw[base + j] < fi;
        inc_faces[base + r] = fi;
    }
    int heads = 0;
    for (int i = lane; i < 2 * n; i += 64) {
        const int64_t k = raw[base * 2 + i];
        int r = 0, head = 1;
        for (int j = 0; j < 2 * n; ++j) {
            const int64_t kj = raw[base * 2 + j];
            r += kj < k;
            if (kj < k && (kj >> 32) == (k >> 32)) head = 0;
        }
        sorted[base * 2 + r] = k;
        heads += head;
    }
    heads = wave_reduce(heads, SumOp());
    if (lane == 0) deg[g] = heads;
}

// launch 4: one thread per vertex walks its sorted ring and writes one entry per distinct neighbour, with the flags
__global__ __launch_bounds__(MO_THREADS) void mo_adj_emit_kernel(int64_t total_vertices, const int32_t* __restrict__ inc_start,
                                                                 const int64_t* __restrict__ sorted, const int32_t* __restrict__ nbr_start,
                                                                 int32_t* __restrict__ nbr_index, int32_t* __restrict__ nbr_counts,
                                                                 int32_t* __restrict__ flags) {
    const int64_t g = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (g >= total_vertices) return;
    const int64_t base = (int64_t)inc_start[g] * 2;
    const int n2 = (inc_start[g + 1] - inc_start[g]) * 2;
    int64_t o = nbr_start[g];
    int fl = n2 > 0 ? MO_FLAG_REFERENCED : 0;
    int cur = -1, out = 0, in = 0;
    for (int i = 0; i <= n2; ++i) {
        const int64_t k = i < n2 ? sorted[base + i] : -1;
        const int u = (int)(k >> 32);
        if (i == n2 || u != cur) {
            if (cur >= 0) {
                nbr_index[o] = cur;
                nbr_counts[o * 2] = out;
                nbr_counts[o * 2 + 1] = in;
                ++o;
                if (out + in == 1) fl |= MO_FLAG_BOUNDARY;
                if (out != 1 || in != 1) fl |= MO_FLAG_IRREGULAR;
            }
            cur = u;
            out = in = 0;
        }
        if (i < n2) { if (k & 1) ++in; else ++out; }
    }
    flags[g] = fl;
}

// ---------------------------------------------------------------------------------------------------------------- smoothing
// One umbrella step of one vertex: s = +0; s += x[u] over the row in order; m = s / n; x' = x + f (m - x), per component.
__device__ __forceinline__ void mo_umbrella(const float* x, int nv, int v, const int32_t* __restrict__ row, int n, float f, bool pinned,
                                            float* dst) {
    const float px = x[v * 3], py = x[v * 3 + 1], pz = x[v * 3 + 2];
    float ox = px, oy = py, oz = pz;
    if (n > 0 && !pinned) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int i = 0; i < n; ++i) {
            const int u = row[i];
            if ((unsigned)u >= (unsigned)nv) continue;                       // rows of pcd_mesh_adjacency never hold one
            sx = sx + x[u * 3];
            sy = sy + x[u * 3 + 1];
            sz = sz + x[u * 3 + 2];
        }
        const float d = (float)n;
        const float mx = sx / d, my = sy / d, mz = sz / d;
        ox = px + f * (mx - px);
        oy = py + f * (my - py);
        oz = pz + f * (mz - pz);
    }
    dst[v * 3] = ox;
    dst[v * 3 + 1] = oy;
    dst[v * 3 + 2] = oz;
}

// one step of the whole batch through HBM
__global__ __launch_bounds__(MO_THREADS) void mo_smooth_step_kernel(const float* __restrict__ in, const int64_t* __restrict__ offsets, int batch,
                                                                    const int32_t* __restrict__ nbr_start, const int32_t* __restrict__ nbr_index,
                                                                    const int32_t* __restrict__ flags, float f, int pin,
                                                                    float* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (g >= offsets[batch * 2]) return;
    const MoMesh m = mo_mesh(offsets, mo_find(offsets, batch, g, 0));
    if (g - m.v0 >= m.nv) return;
    const int r0 = nbr_start[g];
    mo_umbrella(in + m.v0 * 3, m.nv, (int)(g - m.v0), nbr_index + r0, nbr_start[g + 1] - r0, f, pin && (flags[g] & MO_FLAG_BOUNDARY),
                out + m.v0 * 3);
}

// ---------------------------------------------------------------------------------------------------------------- vertex normals
__global__ __launch_bounds__(MO_THREADS) void mo_normals_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                const int64_t* __restrict__ offsets, int batch,
                                                                const int32_t* __restrict__ inc_start, const int32_t* __restrict__ inc_faces,
                                                                float* __restrict__ normals) {
    const int64_t g = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (g >= offsets[batch * 2]) return;
    const MoMesh m = mo_mesh(offsets, mo_find(offsets, batch, g, 0));
    if (g - m.v0 >= m.nv) return;
    const float* x = vertices + m.v0 * 3;
    const int32_t* fc = faces + m.f0 * 3;
    const int r0 = inc_start[g], n = inc_start[g + 1] - r0;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int i = 0; i < n; ++i) {
        const int t = inc_faces[r0 + i];
        int a, b, c;
        if ((unsigned)t >= (unsigned)m.nf || !mo_face(fc, t, m.nv, a, b, c)) continue;   // rows of pcd_mesh_adjacency hold valid faces only
        const float e1x = x[b * 3] - x[a * 3], e1y = x[b * 3 + 1] - x[a * 3 + 1], e1z = x[b * 3 + 2] - x[a * 3 + 2];
        const float e2x = x[c * 3] - x[a * 3], e2y = x[c * 3 + 1] - x[a * 3 + 1], e2z = x[c * 3 + 2] - x[a * 3 + 2];
        nx = nx + (e1y * e2z - e1z * e2y);
        ny = ny + (e1z * e2x - e1x * e2z);
        nz = nz + (e1x * e2y - e1y * e2x);
    }
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    const bool ok = n > 0 && len != 0.f;
    normals[g * 3] = ok ? nx / len : 0.f;
    normals[g * 3 + 1] = ok ? ny / len : 0.f;
    normals[g * 3 + 2] = ok ? nz / len : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- components
// Labels are read while other threads lower them: in LDS a plain (volatile) read sees them; in the workspace the read has to pass the
// vector L1, which atomics at L2 do not refresh.
template <bool LDS>
__device__ __forceinline__ int mo_label(int* p) {
    if (LDS) return *(volatile int*)p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Min-label propagation with pointer jumping, one workgroup per mesh.  Labels only fall and always name a vertex of the same component, so
// any interleaving ends in the same fixed point, every vertex labelled by the least index of its component; after sweep k every vertex
// within k ring steps of that least vertex holds it, so nv sweeps suffice and the loop is bounded by them.
template <bool LDS>
__global__ __launch_bounds__(MO_WG) void mo_components_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ nbr_start, const int32_t* __restrict__ nbr_index,
                                                              const int32_t* __restrict__ flags, int lds_v, int32_t* __restrict__ workspace,
                                                              int32_t* __restrict__ labels, int32_t* __restrict__ counts,
                                                              int32_t* __restrict__ component_faces) {
    extern __shared__ __attribute__((aligned(16))) int mo_lab[];
    __shared__ int changed, roots;
    const MoMesh m = mo_mesh(offsets, blockIdx.x);
    if (LDS != (m.nv <= lds_v)) return;                                          // the other instance's mesh
    int* lab = LDS ? mo_lab : workspace + m.v0;
    if (threadIdx.x == 0) roots = 0;
    for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
        const int l = (flags[m.v0 + v] & MO_FLAG_REFERENCED) ? v : MO_NO_LABEL;
        if (LDS) lab[v] = l;
        else __hip_atomic_store(lab + v, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // where the atomics and the reads above go
    }
    __syncthreads();
    for (int sweep = 0; sweep < m.nv; ++sweep) {
        if (threadIdx.x == 0) changed = 0;
        __syncthreads();
        bool ch = false;
        for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
            const int l = mo_label<LDS>(lab + v);
            if (l == MO_NO_LABEL) continue;
            const int r0 = nbr_start[m.v0 + v], n = nbr_start[m.v0 + v + 1] - r0;
            int best = l;
            for (int i = 0; i < n; ++i) {
                const int u = nbr_index[r0 + i];
                if ((unsigned)u < (unsigned)m.nv) best = min(best, mo_label<LDS>(lab + u));
            }
            if (best < l) {
                atomicMin(lab + v, best);
                atomicMin(lab + l, best);                                        // hook the old representative too
                ch = true;
            }
        }
        if (ch) changed = 1;
        __syncthreads();
        const int any = changed;
        __syncthreads();
        if (!any) break;
        for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
            int l = mo_label<LDS>(lab + v);
            if (l == MO_NO_LABEL) continue;
            for (int k = 0; k < 64; ++k) {
                const int p = mo_label<LDS>(lab + l);
                if (p >= l) break;
                l = p;
            }
            atomicMin(lab + v, l);
        }
        __syncthreads();
    }
    int mine = 0;
    for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
        const int l = mo_label<LDS>(lab + v);
        labels[m.v0 + v] = l == MO_NO_LABEL ? -1 : l;
        mine += l == v;
    }
    mine = wave_reduce(mine, SumOp());
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&roots, mine);
    const int32_t* fc = faces + m.f0 * 3;
    for (int t = threadIdx.x; t < m.nf; t += MO_WG) {
        int a, b, c;
        if (mo_face(fc, t, m.nv, a, b, c)) atomicAdd(&component_faces[m.v0 + mo_label<LDS>(lab + a)], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = roots;
}

__global__ __launch_bounds__(MO_WG) void mo_keep_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ component_faces, int rule, int min_faces,
                                                        int32_t* __restrict__ keep) {
    __shared__ unsigned long long best;
    const MoMesh m = mo_mesh(offsets, blockIdx.x);
    if (threadIdx.x == 0) best = 0ull;
    __syncthreads();
    if (rule == PCD_MESH_KEEP_LARGEST) {
        unsigned long long mine = 0ull;                                          // most faces, then the smaller label
        for (int v = threadIdx.x; v < m.nv; v += MO_WG)
            if (labels[m.v0 + v] == v) {
                const unsigned long long k = ((unsigned long long)(unsigned)component_faces[m.v0 + v] << 32) | (unsigned)(0x7fffffff - v);
                mine = k > mine ? k : mine;
            }
        if (mine) atomicMax(&best, mine);
        __syncthreads();
    }
    const int winner = best ? 0x7fffffff - (int)(best & 0xffffffffull) : -1;
    for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
        const int l = labels[m.v0 + v];
        int k = 0;
        if (l >= 0 && l < m.nv) k = rule == PCD_MESH_KEEP_LARGEST ? l == winner : component_faces[m.v0 + l] >= min_faces;
        keep[m.v0 + v] = k;
    }
}

// ---------------------------------------------------------------------------------------------------------------- compaction
__device__ __forceinline__ bool mo_face_kept(const int32_t* __restrict__ fc, int t, int nv, const int32_t* __restrict__ remap, int& a, int& b,
                                             int& c) {
    if (!mo_face(fc, t, nv, a, b, c)) return false;
    a = remap[a]; b = remap[b]; c = remap[c];
    return a >= 0 && b >= 0 && c >= 0;
}

__global__ __launch_bounds__(MO_WG) void mo_compact_count_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ keep, int32_t* __restrict__ remap,
                                                                 int32_t* __restrict__ counts) {
    __shared__ int wsum[MO_WAVES];
    const MoMesh m = mo_mesh(offsets, blockIdx.x);
    int base = 0;
    for (int c0 = 0; c0 < m.nv; c0 += MO_WG) {
        const int v = c0 + threadIdx.x;
        const int k = v < m.nv && keep[m.v0 + v] != 0;
        int total;
        const int e = block_scan_excl<MO_WAVES>(k, wsum, &total);
        if (v < m.nv) remap[m.v0 + v] = k ? base + e : -1;
        base += total;
    }
    __syncthreads();                                                             // the workgroup's own remap rows are read below
    const int32_t* fc = faces + m.f0 * 3;
    int nf = 0;
    for (int c0 = 0; c0 < m.nf; c0 += MO_WG) {
        const int t = c0 + threadIdx.x;
        int a, b, c, total;
        const int k = t < m.nf && mo_face_kept(fc, t, m.nv, remap + m.v0, a, b, c);
        block_scan_excl<MO_WAVES>(k, wsum, &total);
        nf += total;
    }
    if (threadIdx.x == 0) {
        counts[blockIdx.x * 2] = base;
        counts[blockIdx.x * 2 + 1] = nf;
    }
}

__global__ __launch_bounds__(MO_WG) void mo_compact_emit_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                const int64_t* __restrict__ offsets, const int32_t* __restrict__ remap,
                                                                const int64_t* __restrict__ out_offsets, float* __restrict__ out_vertices,
                                                                int32_t* __restrict__ out_faces) {
    __shared__ int wsum[MO_WAVES];
    const MoMesh m = mo_mesh(offsets, blockIdx.x);
    const int64_t ov = out_offsets[blockIdx.x * 2], of = out_offsets[blockIdx.x * 2 + 1];
    for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
        const int r = remap[m.v0 + v];
        if (r < 0) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) out_vertices[(ov + r) * 3 + k] = vertices[(m.v0 + v) * 3 + k];
    }
    const int32_t* fc = faces + m.f0 * 3;
    int base = 0;
    for (int c0 = 0; c0 < m.nf; c0 += MO_WG) {
        const int t = c0 + threadIdx.x;
        int a = 0, b = 0, c = 0, total;
        const int k = t < m.nf && mo_face_kept(fc, t, m.nv, remap + m.v0, a, b, c);
        const int e = block_scan_excl<MO_WAVES>(k, wsum, &total);
        if (k) {
            int32_t* o = out_faces + (of + base + e) * 3;
            o[0] = a; o[1] = b; o[2] = c;
        }
        base += total;
    }
}

// ---------------------------------------------------------------------------------------------------------------- measures
// adds every thread's count to an LDS word: the wave's butterfly, then one integer atomic per wave (all lanes of the wave call it)
__device__ __forceinline__ void mo_acc(int* word, int mine) {
    const int s = wave_reduce(mine, SumOp());
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(word, s);
}

// Doubles are added in a fixed tree: the butterfly of a wave, the 16 waves in order, then the chunks of 1024 faces in order.
__global__ __launch_bounds__(MO_WG) void mo_measures_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                            const int64_t* __restrict__ offsets, const int32_t* __restrict__ nbr_start,
                                                            const int32_t* __restrict__ nbr_index, const int32_t* __restrict__ nbr_counts,
                                                            const int32_t* __restrict__ labels, double* __restrict__ real,
                                                            int32_t* __restrict__ whole) {
    __shared__ double scratch[MO_WAVES * 5];
    __shared__ int acc[7];                                                       // referenced, entries, faces, boundary, irregular, roots, open entries
    const MoMesh m = mo_mesh(offsets, blockIdx.x);
    if (threadIdx.x < 7) acc[threadIdx.x] = 0;
    __syncthreads();
    int ref = 0, ent = 0, bnd = 0, irr = 0, roots = 0, open = 0;
    for (int v = threadIdx.x; v < m.nv; v += MO_WG) {
        const int r0 = nbr_start[m.v0 + v], n = nbr_start[m.v0 + v + 1] - r0;
        ref += n > 0;
        ent += n;
        roots += labels[m.v0 + v] == v;
        for (int i = 0; i < n; ++i) {
            const int out = nbr_counts[(int64_t)(r0 + i) * 2], in = nbr_counts[(int64_t)(r0 + i) * 2 + 1];
            open += out != in;
            if (nbr_index[r0 + i] > v) {                                         // every undirected edge once
                bnd += out + in == 1;
                irr += out != 1 || in != 1;
            }
        }
    }
    mo_acc(acc + 0, ref);
    mo_acc(acc + 1, ent);
    mo_acc(acc + 3, bnd);
    mo_acc(acc + 4, irr);
    mo_acc(acc + 5, roots);
    mo_acc(acc + 6, open);
    const float* x = vertices + m.v0 * 3;
    const int32_t* fc = faces + m.f0 * 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                                   // area, volume, area-weighted centroid (thread 0's are used)
    int nfv = 0;
    for (int c0 = 0; c0 < m.nf; c0 += MO_WG) {
        const int t = c0 + threadIdx.x;
        double term[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        int a, b, c;
        if (t < m.nf && mo_face(fc, t, m.nv, a, b, c)) {
            ++nfv;
            const double ax = x[a * 3], ay = x[a * 3 + 1], az = x[a * 3 + 2];
            const double bx = x[b * 3], by = x[b * 3 + 1], bz = x[b * 3 + 2];
            const double cx = x[c * 3], cy = x[c * 3 + 1], cz = x[c * 3 + 2];
            const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            const double area = sqrt((nx * nx + ny * ny) + nz * nz) / 2.0;
            term[0] = area;
            term[1] = ((ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)) / 6.0;
            term[2] = area * (((ax + bx) + cx) / 3.0);
            term[3] = area * (((ay + by) + cy) / 3.0);
            term[4] = area * (((az + bz) + cz) / 3.0);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double w = wave_reduce(term[k], SumOp());
            if (lane == 0) scratch[wave * 5 + k] = w;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                double r = scratch[k];
#pragma unroll 1
                for (int w = 1; w < MO_WAVES; ++w) r = r + scratch[w * 5 + k];
                sum[k] = sum[k] + r;
            }
        }
        __syncthreads();
    }
    mo_acc(acc + 2, nfv);
    __syncthreads();
    if (threadIdx.x == 0) {
        double* r = real + (int64_t)blockIdx.x * 5;
        r[0] = sum[0];
        r[1] = sum[1];
        for (int k = 2; k < 5; ++k) r[k] = sum[0] > 0.0 ? sum[k] / sum[0] : 0.0;
        int32_t* w = whole + (int64_t)blockIdx.x * 8;
        w[0] = acc[0];
        w[1] = acc[1] / 2;
        w[2] = acc[2];
        w[3] = acc[3];
        w[4] = acc[4];
        w[5] = acc[5];
        w[6] = acc[0] - acc[1] / 2 + acc[2];
        w[7] = acc[6] == 0;
    }
}

struct MoAdjWorkspace { size_t raw, sorted, inc_raw, cnt, cursor, deg, partial, total; };

MoAdjWorkspace mo_adj_workspace(int64_t total_vertices, int64_t total_faces) {
    MoAdjWorkspace w;
    size_t o = 0;
    const size_t rows = (size_t)total_vertices + 1;
    w.raw = o;      o += align_up((size_t)total_faces * 6 * sizeof(int64_t));
    w.sorted = o;   o += align_up((size_t)total_faces * 6 * sizeof(int64_t));
    w.inc_raw = o;  o += align_up((size_t)total_faces * 3 * sizeof(int32_t));
    w.cnt = o;      o += align_up(rows * sizeof(int32_t));
    w.cursor = o;   o += align_up(rows * sizeof(int32_t));
    w.deg = o;      o += align_up(rows * sizeof(int32_t));
    w.partial = o;  o += align_up((size_t)ceil_div((int64_t)rows, MO_WG) * sizeof(int32_t));
    w.total = o;
    return w;
}

}  // namespace

#pragma clang fp contract(fast)

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_mesh_ops_config(int code) {
    PCD_CHECK_ARG(code == 0 || code == 1);
    g_labels_form = code;
    return PCD_OK;
}

extern "C" size_t pcd_mesh_adjacency_workspace_bytes(int batch, int64_t total_vertices, int64_t total_faces) {
    if (!mo_sizes_ok(batch, total_vertices, total_faces)) return 0;
    return mo_adj_workspace(total_vertices, total_faces).total;
}

extern "C" int pcd_mesh_adjacency(const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices, int64_t total_faces,
                                  void* workspace, int32_t* nbr_start, int32_t* nbr_index, int32_t* nbr_counts, int32_t* inc_start,
                                  int32_t* inc_faces, int32_t* flags, void* stream) {
    PCD_CHECK_ARG(faces && offsets && workspace && nbr_start && nbr_index && nbr_counts && inc_start && inc_faces && flags);
    PCD_CHECK_ARG(mo_sizes_ok(batch, total_vertices, total_faces));
    const MoAdjWorkspace w = mo_adj_workspace(total_vertices, total_faces);
    char* ws = (char*)workspace;
    int64_t* raw = (int64_t*)(ws + w.raw);
    int64_t* sorted = (int64_t*)(ws + w.sorted);
    int32_t* inc_raw = (int32_t*)(ws + w.inc_raw);
    int32_t* cnt = (int32_t*)(ws + w.cnt);
    int32_t* cursor = (int32_t*)(ws + w.cursor);
    int32_t* deg = (int32_t*)(ws + w.deg);
    int32_t* partial = (int32_t*)(ws + w.partial);
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = total_vertices + 1;
    int rc;
    PCD_CHECK_HIP(hipMemsetAsync(cnt, 0, (w.partial - w.cnt), s));                // cnt, cursor and deg, their closing rows included
    const unsigned fblocks = (unsigned)ceil_div(total_faces, MO_THREADS), vblocks = (unsigned)ceil_div(total_vertices, MO_THREADS);
    if (total_faces > 0) {
        hipLaunchKernelGGL(mo_adj_count_kernel, dim3(fblocks), dim3(MO_THREADS), 0, s, faces, offsets, batch, cnt);
        PCD_CHECK_LAUNCH();
    }
    PCD_RUN(mo_scan(cnt, inc_start, rows, partial, s));
    if (total_faces > 0) {
        hipLaunchKernelGGL(mo_adj_fill_kernel, dim3(fblocks), dim3(MO_THREADS), 0, s, faces, offsets, batch, inc_start, cursor, inc_raw, raw);
        PCD_CHECK_LAUNCH();
    }
    if (total_vertices > 0) {
        hipLaunchKernelGGL(mo_adj_sort_kernel, dim3((unsigned)ceil_div(total_vertices, MO_THREADS / 64)), dim3(MO_THREADS), 0, s, total_vertices,
                           inc_start, inc_raw, raw, inc_faces, sorted, deg);
        PCD_CHECK_LAUNCH();
    }
    PCD_RUN(mo_scan(deg, nbr_start, rows, partial, s));
    if (total_vertices > 0) {
        hipLaunchKernelGGL(mo_adj_emit_kernel, dim3(vblocks), dim3(MO_THREADS), 0, s, total_vertices, inc_start, sorted, nbr_start, nbr_index,
                           nbr_counts, flags);
        PCD_CHECK_LAUNCH();
    }
    return PCD_OK;
}

extern "C" size_t pcd_mesh_smooth_workspace_bytes(int64_t total_vertices) {
    if (total_vertices < 0 || total_vertices >= 0x7fffffff) return 0;
    return align_up((size_t)total_vertices * 3 * sizeof(float));
}

extern "C" int pcd_mesh_smooth(const float* vertices, const int64_t* offsets, int batch, int64_t total_vertices, const int32_t* nbr_start,
                               const int32_t* nbr_index, const int32_t* flags, int iterations, float lam, float mu, int pin_boundary,
                               void* workspace, float* out, void* stream) {
    PCD_CHECK_ARG(vertices && offsets && nbr_start && nbr_index && flags && workspace && out && out != vertices);
    PCD_CHECK_ARG(mo_sizes_ok(batch, total_vertices, 0));
    PCD_CHECK_ARG(iterations >= 0 && iterations <= (1 << 20));
    PCD_CHECK_ARG(std::isfinite(lam) && std::isfinite(mu) && lam > 0.f && lam <= 1.f && mu > -1.f && mu <= 0.f);
    hipStream_t s = (hipStream_t)stream;
    const int two = mu != 0.f, steps = iterations * (two ? 2 : 1);
    if (total_vertices == 0) return PCD_OK;
    if (steps == 0) {
        PCD_CHECK_HIP(hipMemcpyAsync(out, vertices, (size_t)total_vertices * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
        return PCD_OK;
    }
    float* other = (float*)workspace;                                            // the steps alternate between it and out, the last one into out
    const float* src = vertices;
    for (int k = 0; k < steps; ++k) {
        float* dst = ((steps - 1 - k) & 1) ? other : out;
        hipLaunchKernelGGL(mo_smooth_step_kernel, dim3((unsigned)ceil_div(total_vertices, MO_THREADS)), dim3(MO_THREADS), 0, s, src, offsets, batch,
                           nbr_start, nbr_index, flags, (two && (k & 1)) ? mu : lam, pin_boundary != 0, dst);
        PCD_CHECK_LAUNCH();
        src = dst;
    }
    return PCD_OK;
}

extern "C" int pcd_mesh_vertex_normals(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices,
                                       const int32_t* inc_start, const int32_t* inc_faces, float* normals, void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && inc_start && inc_faces && normals && mo_sizes_ok(batch, total_vertices, 0));
    if (total_vertices == 0) return PCD_OK;
    hipLaunchKernelGGL(mo_normals_kernel, dim3((unsigned)ceil_div(total_vertices, MO_THREADS)), dim3(MO_THREADS), 0, (hipStream_t)stream, vertices,
                       faces, offsets, batch, inc_start, inc_faces, normals);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_mesh_components_workspace_bytes(int64_t total_vertices) {
    if (total_vertices < 0 || total_vertices >= 0x7fffffff) return 0;
    return align_up((size_t)total_vertices * sizeof(int32_t));
}

extern "C" int pcd_mesh_components(const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices, int64_t max_vertices,
                                   const int32_t* nbr_start, const int32_t* nbr_index, const int32_t* flags, void* workspace, int32_t* labels,
                                   int32_t* counts, int32_t* component_faces, void* stream) {
    PCD_CHECK_ARG(faces && offsets && nbr_start && nbr_index && flags && workspace && labels && counts && component_faces);
    PCD_CHECK_ARG(mo_sizes_ok(batch, total_vertices, 0) && max_vertices >= 0 && max_vertices <= total_vertices);
    hipStream_t s = (hipStream_t)stream;
    if (total_vertices > 0) PCD_CHECK_HIP(hipMemsetAsync(component_faces, 0, (size_t)total_vertices * sizeof(int32_t), s));
    const int lds_v = g_labels_form == 1 ? -1 : (int)(max_vertices < PCD_MESH_LABELS_LDS_MAX_V ? max_vertices : PCD_MESH_LABELS_LDS_MAX_V);
    if (lds_v >= 0) {                                                            // empty meshes get their zero count here
        static PcdLdsOnce once;
        PCD_CHECK_HIP(pcd_allow_lds(once, (const void*)mo_components_kernel<true>, PCD_MESH_LABELS_LDS_MAX_V * (int)sizeof(int32_t)));
        hipLaunchKernelGGL(mo_components_kernel<true>, dim3(batch), dim3(MO_WG), (size_t)(lds_v > 0 ? lds_v : 1) * sizeof(int32_t), s, faces,
                           offsets, nbr_start, nbr_index, flags, lds_v, (int32_t*)workspace, labels, counts, component_faces);
        PCD_CHECK_LAUNCH();
    }
    if (max_vertices > lds_v) {
        hipLaunchKernelGGL(mo_components_kernel<false>, dim3(batch), dim3(MO_WG), 0, s, faces, offsets, nbr_start, nbr_index, flags, lds_v,
                           (int32_t*)workspace, labels, counts, component_faces);
        PCD_CHECK_LAUNCH();
    }
    return PCD_OK;
}

extern "C" int pcd_mesh_component_keep(const int64_t* offsets, int batch, const int32_t* labels, const int32_t* component_faces, int rule,
                                       int min_faces, int32_t* keep, void* stream) {
    PCD_CHECK_ARG(offsets && labels && component_faces && keep && batch > 0 && batch <= 65535);
    PCD_CHECK_ARG(rule == PCD_MESH_KEEP_LARGEST || (rule == PCD_MESH_KEEP_MIN_FACES && min_faces >= 0));
    hipLaunchKernelGGL(mo_keep_kernel, dim3(batch), dim3(MO_WG), 0, (hipStream_t)stream, offsets, labels, component_faces, rule, min_faces, keep);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_mesh_compact_workspace_bytes(int64_t total_vertices) {
    if (total_vertices < 0 || total_vertices >= 0x7fffffff) return 0;
    return align_up((size_t)total_vertices * sizeof(int32_t));
}

extern "C" int pcd_mesh_compact_count(const int32_t* faces, const int64_t* offsets, int batch, const int32_t* keep, void* workspace,
                                      int32_t* counts, void* stream) {
    PCD_CHECK_ARG(faces && offsets && keep && workspace && counts && batch > 0 && batch <= 65535);
    hipLaunchKernelGGL(mo_compact_count_kernel, dim3(batch), dim3(MO_WG), 0, (hipStream_t)stream, faces, offsets, keep, (int32_t*)workspace,
                       counts);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_mesh_compact_emit(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, const void* workspace,
                                     const int64_t* out_offsets, float* out_vertices, int32_t* out_faces, void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && workspace && out_offsets && out_vertices && out_faces && batch > 0 && batch <= 65535);
    hipLaunchKernelGGL(mo_compact_emit_kernel, dim3(batch), dim3(MO_WG), 0, (hipStream_t)stream, vertices, faces, offsets,
                       (const int32_t*)workspace, out_offsets, out_vertices, out_faces);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_mesh_measures(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, const int32_t* nbr_start,
                                 const int32_t* nbr_index, const int32_t* nbr_counts, const int32_t* labels, double* real, int32_t* whole,
                                 void* stream) {
    PCD_CHECK_ARG(vertices && faces && offsets && nbr_start && nbr_index && nbr_counts && labels && real && whole);
    PCD_CHECK_ARG(batch > 0 && batch <= 65535);
    hipLaunchKernelGGL(mo_measures_kernel, dim3(batch), dim3(MO_WG), 0, (hipStream_t)stream, vertices, faces, offsets, nbr_start, nbr_index,
                       nbr_counts, labels, real, whole);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
