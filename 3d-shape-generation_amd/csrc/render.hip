// K14: images out (DESIGN.md "Render"; include/pcd_hip.h pcd_render_points, pcd_render_meshes): a depth-buffered batch rasterizer for point
// clouds and triangle meshes, the third member of the mesh family (mesh.hip out, mesh_in.hip in).
//
//   One launch, one workgroup per (shape, view, tile).  The tile's visibility keys live in LDS as u64 (orderable(depth) << 32 | primitive): one
//   ds_min_u64 per covered pixel decides the least (depth, index) pair whatever the order of evaluation.  Every workgroup walks all primitives of
//   its shape, 1024 at a time; a block scan of their row counts spreads the (primitive, pixel row of its tile-clipped bounding box) items evenly
//   over the threads, as mesh_in.hip spreads its columns: 12 large triangles and 3000 small ones keep the workgroup equally busy.  No binning
//   pass, no workspace.  Resolve: a thread takes 4 pixels of a row, decodes the winners, recomputes depth and shading from the primitive and
//   stores 16 + 16 + 12 bytes where the width allows.
//
// Coverage, depth and shading are functions of (primitive, pixel) alone, fp32 without contraction and without a division in any coverage
// decision: the same bits for either tile shape, for a shape alone or in a batch, and -- where every intermediate value is exactly
// representable -- the decisions of the float64 statement (tests/render_statement.py).
#include "mesh_tri.h"
#include <cmath>

namespace pcd {

#pragma clang fp contract(off)

constexpr int REN_THREADS = 1024;
constexpr int REN_WAVES = REN_THREADS / 64;
constexpr int REN_TW = 128;                                    // tile width in pixels; the height is 64 or 128
constexpr int REN_MAX_SIDE = 2048;
constexpr unsigned long long REN_EMPTY = ~0ull;

struct RenArgs {
    const float* prims;                                        // points, or vertices
    const int32_t* faces;
    const int64_t* offsets;
    const float* views;
    const float* colors;
    int view_sets, n_views, height, width;
    float radius, lx, ly, lz, ambient, bg[3];
    int vec;                                                   // rows and pointers allow the 16 / 16 / 12 byte stores
    int32_t* ids;
    float* depth;
    uint8_t* rgb;
};

struct RenView { float m[12]; };

__device__ __forceinline__ void ren_project(const RenView& w, const float* __restrict__ p, float& x, float& y, float& z) {
    const float px = p[0], py = p[1], pz = p[2];
    x = ((w.m[0] * px + w.m[1] * py) + w.m[2] * pz) + w.m[3];
    y = ((w.m[4] * px + w.m[5] * py) + w.m[6] * pz) + w.m[7];
    z = ((w.m[8] * px + w.m[9] * py) + w.m[10] * pz) + w.m[11];
}

__device__ __forceinline__ bool ren_finite(float v) { return fabsf(v) <= 3.4028234e38f; }   // false for NaN

// pixels j of one axis whose centre j + 1/2 may lie in [mn, mx], cut to [t0, t1): first and count.  One pixel generous on either side (the
// coverage test decides); the clamp bounds the conversion, and the range depends on the pixel grid alone, not on the tile.
__device__ __forceinline__ void ren_axis_range(float mn, float mx, int t0, int t1, int& first, int& count) {
    const float l = fminf(fmaxf(floorf(mn - 0.5f), (float)t0), (float)t1);
    const float h = fminf(fmaxf(ceilf(mx - 0.5f), (float)(t0 - 1)), (float)(t1 - 1));
    first = (int)l;
    count = max((int)h - first + 1, 0);
    if (!(mn <= mx)) count = 0;
}

__device__ __forceinline__ unsigned long long ren_key(float depth, unsigned index) {
    const unsigned u = __float_as_uint(depth + 0.f);                               // -0 -> +0: ordered as fp32 compares
    const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)o << 32) | index;
}

__device__ __forceinline__ float ren_round255(float v) { return floorf(fminf(fmaxf(v, 0.f), 255.f) + 0.5f); }

// ------------------------------------------------------------------------------------------------------------------- points
struct RenPoint { float x, y, z; bool ok; };

__device__ __forceinline__ RenPoint ren_load_point(const RenView& w, const float* __restrict__ pts, int k) {
    RenPoint q;
    ren_project(w, pts + (int64_t)k * 3, q.x, q.y, q.z);
    q.ok = ren_finite(q.x) && ren_finite(q.y) && ren_finite(q.z);
    return q;
}

__device__ __forceinline__ void ren_point_box(const RenPoint& q, float r, int tx0, int tx1, int ty0, int ty1, int& x0, int& xn, int& y0, int& yn) {
    x0 = y0 = xn = yn = 0;
    if (!q.ok) return;
    ren_axis_range(q.x - r, q.x + r, tx0, tx1, x0, xn);
    ren_axis_range(q.y - r, q.y + r, ty0, ty1, y0, yn);
    if (xn <= 0 || yn <= 0) xn = yn = 0;
}

// ------------------------------------------------------------------------------------------------------------------- triangles
struct RenEdge { float ax, ay, dx, dy, s; bool tie; };
struct RenTri {
    float x0, y0, z0, x1, y1, z1, x2, y2, z2;
    float nx, ny, nz;                                          // u x v of the view-space edges
    RenEdge e[3];
    bool ok;
};

// edge P - Q with R the third vertex, from its canonical order: the neighbour across the edge computes the same d and the same e(c)
__device__ __forceinline__ RenEdge ren_edge(float px, float py, float qx, float qy, float rx, float ry) {
    if (qx < px || (qx == px && qy < py)) { float t = px; px = qx; qx = t; t = py; py = qy; qy = t; }
    RenEdge e;
    e.ax = px; e.ay = py; e.dx = qx - px; e.dy = qy - py;
    const float w = e.dx * (ry - py) - e.dy * (rx - px);
    e.s = w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f);
    const float nx = e.s * -e.dy, ny = e.s * e.dx;             // inward normal
    e.tie = nx > 0.f || (nx == 0.f && ny > 0.f);
    return e;
}

__device__ __forceinline__ bool ren_edge_covers(const RenEdge& e, float cx, float cy) {
    const float v = e.dx * (cy - e.ay) - e.dy * (cx - e.ax);
    return e.s * v > 0.f || (v == 0.f && e.tie);
}

template <bool FULL>                                           // FULL: with the edges (rasterize); otherwise plane and normal only (resolve)
__device__ __forceinline__ RenTri ren_load_tri(const RenView& w, const float* __restrict__ v, const int32_t* __restrict__ f, int t, int64_t nv) {
    RenTri q;
    const int i0 = f[(int64_t)t * 3], i1 = f[(int64_t)t * 3 + 1], i2 = f[(int64_t)t * 3 + 2];
    q.ok = i0 >= 0 && i1 >= 0 && i2 >= 0 && (int64_t)i0 < nv && (int64_t)i1 < nv && (int64_t)i2 < nv;
    if (!q.ok) return q;
    ren_project(w, v + (int64_t)i0 * 3, q.x0, q.y0, q.z0);
    ren_project(w, v + (int64_t)i1 * 3, q.x1, q.y1, q.z1);
    ren_project(w, v + (int64_t)i2 * 3, q.x2, q.y2, q.z2);
    q.ok = ren_finite(q.x0) && ren_finite(q.y0) && ren_finite(q.z0) && ren_finite(q.x1) && ren_finite(q.y1) && ren_finite(q.z1) &&
           ren_finite(q.x2) && ren_finite(q.y2) && ren_finite(q.z2);
    if (!q.ok) return q;
    const float ux = q.x1 - q.x0, uy = q.y1 - q.y0, uz = q.z1 - q.z0;
    const float vx = q.x2 - q.x0, vy = q.y2 - q.y0, vz = q.z2 - q.z0;
    q.nx = uy * vz - uz * vy; q.ny = uz * vx - ux * vz; q.nz = ux * vy - uy * vx;
    q.ok = q.nz != 0.f && q.nz == q.nz;
    if (FULL && q.ok) {
        q.e[0] = ren_edge(q.x0, q.y0, q.x1, q.y1, q.x2, q.y2);
        q.e[1] = ren_edge(q.x1, q.y1, q.x2, q.y2, q.x0, q.y0);
        q.e[2] = ren_edge(q.x2, q.y2, q.x0, q.y0, q.x1, q.y1);
        q.ok = q.e[0].s != 0.f && q.e[1].s != 0.f && q.e[2].s != 0.f;
    }
    return q;
}

__device__ __forceinline__ float ren_tri_depth(const RenTri& q, float cx, float cy) {
    return q.z0 - (q.nx * (cx - q.x0) + q.ny * (cy - q.y0)) / q.nz;
}

__device__ __forceinline__ void ren_tri_box(const RenTri& q, int tx0, int tx1, int ty0, int ty1, int& x0, int& xn, int& y0, int& yn) {
    x0 = y0 = xn = yn = 0;
    if (!q.ok) return;
    ren_axis_range(fminf(fminf(q.x0, q.x1), q.x2), fmaxf(fmaxf(q.x0, q.x1), q.x2), tx0, tx1, x0, xn);
    ren_axis_range(fminf(fminf(q.y0, q.y1), q.y2), fmaxf(fmaxf(q.y0, q.y1), q.y2), ty0, ty1, y0, yn);
    if (xn <= 0 || yn <= 0) xn = yn = 0;
}

template <bool MESH, int TH>
__global__ __launch_bounds__(REN_THREADS) void render_kernel(const RenArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ren_keys[];   // [TH][REN_TW]
    __shared__ int prefix[REN_THREADS];
    __shared__ int wsum[REN_WAVES];
    const int tid = threadIdx.x, b = blockIdx.z, view = blockIdx.y;
    const int tiles_x = (a.width + REN_TW - 1) / REN_TW;
    const int tx0 = (int)(blockIdx.x % tiles_x) * REN_TW, ty0 = (int)(blockIdx.x / tiles_x) * TH;
    const int tx1 = min(tx0 + REN_TW, a.width), ty1 = min(ty0 + TH, a.height);
    RenView w;
    {
        const float* m = a.views + ((int64_t)(a.view_sets == 1 ? 0 : b) * a.n_views + view) * 12;
#pragma unroll
        for (int i = 0; i < 12; ++i) w.m[i] = m[i];
    }
    const float* pv;
    const int32_t* f = nullptr;
    int64_t nv;
    int np;                                                    // primitives of this shape
    if (MESH) {
        const MeshRows m = mesh_rows(a.offsets, b);
        nv = m.nv;
        np = nv > 0 && m.nf > 0 && m.nf <= 0x7fffffff ? (int)m.nf : 0;
        pv = a.prims + m.v0 * 3;
        f = a.faces + m.f0 * 3;
    } else {
        const int64_t p0 = a.offsets[b];
        nv = a.offsets[b + 1] - p0;
        np = nv > 0 && nv <= 0x7fffffff ? (int)nv : 0;
        pv = a.prims + p0 * 3;
    }
    const float r = a.radius, r2 = r * r;

    for (int i = tid; i < TH * REN_TW; i += REN_THREADS) ren_keys[i] = REN_EMPTY;
    __syncthreads();

    for (int c0 = 0; c0 < np; c0 += REN_THREADS) {
        int mine = 0;
        if (c0 + tid < np) {
            int x0, xn, y0, yn;
            if (MESH) ren_tri_box(ren_load_tri<true>(w, pv, f, c0 + tid, nv), tx0, tx1, ty0, ty1, x0, xn, y0, yn);
            else ren_point_box(ren_load_point(w, pv, c0 + tid), r, tx0, tx1, ty0, ty1, x0, xn, y0, yn);
            mine = yn;
        }
        int total;
        prefix[tid] = block_scan_incl<REN_WAVES>(mine, wsum, total);
        __syncthreads();
        for (int item = tid; item < total; item += REN_THREADS) {
            const int l = first_above(prefix, REN_THREADS - 1, item);             // the first primitive whose inclusive sum exceeds the item
            const int local = item - (l ? prefix[l - 1] : 0);
            const unsigned index = (unsigned)(c0 + l);                            // l has items, so c0 + l < np and the primitive is ok
            int x0, xn, y0, yn;
            if (MESH) {
                const RenTri q = ren_load_tri<true>(w, pv, f, c0 + l, nv);
                ren_tri_box(q, tx0, tx1, ty0, ty1, x0, xn, y0, yn);
                if (local >= yn) continue;                                        // cannot happen: the counts came from the same arithmetic
                const int y = y0 + local;
                const float cy = (float)y + 0.5f;
                unsigned long long* row = ren_keys + (y - ty0) * REN_TW - tx0;
                for (int x = x0; x < x0 + xn; ++x) {
                    const float cx = (float)x + 0.5f;
                    if (!(ren_edge_covers(q.e[0], cx, cy) && ren_edge_covers(q.e[1], cx, cy) && ren_edge_covers(q.e[2], cx, cy))) continue;
                    const float d = ren_tri_depth(q, cx, cy);
                    if (ren_finite(d)) atomicMin(&row[x], ren_key(d, index));
                }
            } else {
                const RenPoint q = ren_load_point(w, pv, c0 + l);
                ren_point_box(q, r, tx0, tx1, ty0, ty1, x0, xn, y0, yn);
                if (local >= yn) continue;
                const int y = y0 + local;
                const float dy = ((float)y + 0.5f) - q.y;
                const unsigned long long key = ren_key(q.z, index);
                unsigned long long* row = ren_keys + (y - ty0) * REN_TW - tx0;
                for (int x = x0; x < x0 + xn; ++x) {
                    const float dx = ((float)x + 0.5f) - q.x;
                    if (dx * dx + dy * dy <= r2) atomicMin(&row[x], key);
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();

    // resolve: 4 pixels of a row per thread
    float col[3] = {0.27f, 0.51f, 0.71f};
    if (a.colors != nullptr) { col[0] = a.colors[b * 3]; col[1] = a.colors[b * 3 + 1]; col[2] = a.colors[b * 3 + 2]; }
    const float bgr = ren_round255(255.f * a.bg[0]), bgg = ren_round255(255.f * a.bg[1]), bgb = ren_round255(255.f * a.bg[2]);
    const int64_t image = ((int64_t)b * a.n_views + view) * a.height;
    for (int quad = tid; quad < TH * (REN_TW / 4); quad += REN_THREADS) {
        const int y = ty0 + quad / (REN_TW / 4), x = tx0 + (quad % (REN_TW / 4)) * 4;
        if (y >= ty1 || x >= tx1) continue;
        const int n = min(4, tx1 - x);
        int id[4];
        float dep[4];
        unsigned char c[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            id[k] = -1; dep[k] = INFINITY; c[k * 3] = (unsigned char)bgr; c[k * 3 + 1] = (unsigned char)bgg; c[k * 3 + 2] = (unsigned char)bgb;
            if (k >= n) continue;
            const unsigned long long key = ren_keys[(y - ty0) * REN_TW + (x - tx0) + k];
            if (key == REN_EMPTY) continue;
            const int index = (int)(unsigned)key;
            const float cx = (float)(x + k) + 0.5f, cy = (float)y + 0.5f;
            float L;
            if (MESH) {
                const RenTri q = ren_load_tri<false>(w, pv, f, index, nv);
                dep[k] = ren_tri_depth(q, cx, cy);
                const float len = sqrtf((q.nx * q.nx + q.ny * q.ny) + q.nz * q.nz);
                L = fabsf((q.nx * a.lx + q.ny * a.ly) + q.nz * a.lz) / len;
            } else {
                const RenPoint q = ren_load_point(w, pv, index);
                dep[k] = q.z;
                const float dx = cx - q.x, dy = cy - q.y;
                const float nz = -sqrtf(fmaxf(r2 - (dx * dx + dy * dy), 0.f));
                L = fmaxf(((dx * a.lx + dy * a.ly) + nz * a.lz) / r, 0.f);
            }
            id[k] = index;
            const float shade = a.ambient + (1.f - a.ambient) * L;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[k * 3 + ch] = (unsigned char)ren_round255((255.f * col[ch]) * shade);
        }
        const int64_t at = (image + y) * a.width + x;
        if (a.vec && n == 4) {
            if (a.ids != nullptr) *(int4*)(a.ids + at) = make_int4(id[0], id[1], id[2], id[3]);
            if (a.depth != nullptr) *(float4*)(a.depth + at) = make_float4(dep[0], dep[1], dep[2], dep[3]);
            if (a.rgb != nullptr) {
                unsigned* out = (unsigned*)(a.rgb + at * 3);
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    out[j] = (unsigned)c[j * 4] | ((unsigned)c[j * 4 + 1] << 8) | ((unsigned)c[j * 4 + 2] << 16) | ((unsigned)c[j * 4 + 3] << 24);
            }
        } else {
            for (int k = 0; k < n; ++k) {
                if (a.ids != nullptr) a.ids[at + k] = id[k];
                if (a.depth != nullptr) a.depth[at + k] = dep[k];
                if (a.rgb != nullptr) { a.rgb[(at + k) * 3] = c[k * 3]; a.rgb[(at + k) * 3 + 1] = c[k * 3 + 1]; a.rgb[(at + k) * 3 + 2] = c[k * 3 + 2]; }
            }
        }
    }
}
#pragma clang fp contract(fast)

static int g_render_tile = 2;                                  // pcd_render_config: 0 = 128 x 64, 1 = 128 x 128, 2 = by the size of the launch

// The 128 x 64 form wins while its launch is at most one workgroup per CU (more workgroups share the walk over a shape's primitives: 21 against
// 28 us for 32 clouds, 92 against 124 us for 32 meshes of 3 k triangles at 256 x 256, one view).  Beyond that the 128 x 128 form wins, which
// walks the primitives half as often: already at two views (30 against 33 us, 129 against 141 us; two workgroups of 1024 threads on a CU do
// not outrun one) and more so at eight (95 against 106 us, 322 against 435 us).  profiles/render_bench.json, render_bench_views_2_3_4.json.
static bool ren_tall_tile(const RenArgs& a, int batch) {
    if (g_render_tile != 2) return g_render_tile == 1;
    int dev = 0, n = 0;                                        // of the device this launch goes to; a failed query falls back to 256 CUs
    const int cus = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    return (int64_t)ceil_div(a.width, REN_TW) * ceil_div(a.height, 64) * a.n_views * batch > (int64_t)cus;
}

template <bool MESH, int TH>
static int ren_launch(const RenArgs& a, int batch, hipStream_t stream) {
    static PcdLdsOnce once;
    const int lds = TH * REN_TW * (int)sizeof(unsigned long long);
    PCD_CHECK_HIP(pcd_allow_lds(once, (const void*)render_kernel<MESH, TH>, lds));
    const unsigned tiles = (unsigned)(ceil_div(a.width, REN_TW) * ceil_div(a.height, TH));
    hipLaunchKernelGGL((render_kernel<MESH, TH>), dim3(tiles, a.n_views, batch), dim3(REN_THREADS), lds, stream, a);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

static int ren_run(bool mesh, RenArgs& a, int batch, const pcd_render_style_t* style, void* stream) {
    PCD_CHECK_ARG(a.prims && a.offsets && a.views && style && (!mesh || a.faces));
    PCD_CHECK_ARG(batch >= 1 && batch <= 65535 && a.n_views >= 1 && a.n_views <= 65535);
    PCD_CHECK_ARG(a.view_sets == 1 || a.view_sets == batch);
    PCD_CHECK_ARG(a.height >= 1 && a.height <= REN_MAX_SIDE && a.width >= 1 && a.width <= REN_MAX_SIDE);
    PCD_CHECK_ARG(a.radius > 0.f && a.radius <= 64.f);
    PCD_CHECK_ARG(style->ambient >= 0.f && style->ambient <= 1.f);
    a.colors = style->colors;
    a.lx = style->light[0]; a.ly = style->light[1]; a.lz = style->light[2];
    a.ambient = style->ambient;
    for (int k = 0; k < 3; ++k) a.bg[k] = style->background[k];
    a.vec = a.width % 4 == 0 && (uintptr_t)a.ids % 16 == 0 && (uintptr_t)a.depth % 16 == 0 && (uintptr_t)a.rgb % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    if (!ren_tall_tile(a, batch)) return mesh ? ren_launch<true, 64>(a, batch, s) : ren_launch<false, 64>(a, batch, s);
    return mesh ? ren_launch<true, 128>(a, batch, s) : ren_launch<false, 128>(a, batch, s);
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_render_points(const float* points, const int64_t* offsets, int batch, const float* views, int view_sets, int n_views,
                                 int height, int width, float radius, const pcd_render_style_t* style, int32_t* ids, float* depth,
                                 uint8_t* rgb, void* stream) {
    RenArgs a = {};
    a.prims = points; a.offsets = offsets; a.views = views; a.view_sets = view_sets; a.n_views = n_views; a.height = height; a.width = width;
    a.radius = radius; a.ids = ids; a.depth = depth; a.rgb = rgb;
    return ren_run(false, a, batch, style, stream);
}

extern "C" int pcd_render_meshes(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, const float* views,
                                 int view_sets, int n_views, int height, int width, const pcd_render_style_t* style, int32_t* ids,
                                 float* depth, uint8_t* rgb, void* stream) {
    RenArgs a = {};
    a.prims = vertices; a.faces = faces; a.offsets = offsets; a.views = views; a.view_sets = view_sets; a.n_views = n_views; a.height = height;
    a.width = width; a.radius = 1.f; a.ids = ids; a.depth = depth; a.rgb = rgb;
    return ren_run(true, a, batch, style, stream);
}

extern "C" int pcd_render_config(int code) {
    PCD_CHECK_ARG(code >= 0 && code <= 2);
    g_render_tile = code;
    return PCD_OK;
}
