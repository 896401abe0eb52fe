// Elementwise / small kernels of the sampler path (all HBM- or latency-bound):
//   time embedding + time_mlp + hoisted enc1 time bias (K3), enc1 xyz half (K=3),
//   output head (C=3), add/remove noise and DDIM/DDPM updates (K4), Philox normals (K5),
//   fp32<->fp16 converts, the row update of shape completion.
#include "common.h"

namespace pcd {

// ------------------------------------------------------------------ time path
// One block per time value.  fp32 throughout (this path defines per-step constants).
__global__ __launch_bounds__(256) void time_embed_kernel(
    const float* __restrict__ t, const float* __restrict__ freqs, int time_dim, int dim,
    const float* __restrict__ w0, const float* __restrict__ b0,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ temb,
    const float* __restrict__ e1w_t, const float* __restrict__ e1b, int c1, float* __restrict__ tbias) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* emb = sm;                 // [time_dim]
    float* hid = sm + time_dim;      // [dim]
    float* out = hid + dim;          // [dim]
    const int i = blockIdx.x;
    const float tv = t[i];
    const int half = time_dim / 2;
    for (int j = threadIdx.x; j < time_dim; j += blockDim.x) {
        float v = 0.f;
        if (j < half) v = sinf(tv * freqs[j]);
        else if (j < 2 * half) v = cosf(tv * freqs[j - half]);
        emb[j] = v;  // odd time_dim: trailing zero pad (networks.py:836-837)
    }
    __syncthreads();
    for (int c = threadIdx.x; c < dim; c += blockDim.x) {
        const float* wr = w0 + (int64_t)c * time_dim;
        float a = 0.f;
        for (int k = 0; k < time_dim; ++k) a = fmaf(wr[k], emb[k], a);
        a += b0[c];
        hid[c] = a / (1.f + expf(-a));  // SiLU
    }
    __syncthreads();
    for (int c = threadIdx.x; c < dim; c += blockDim.x) {
        const float* wr = w2 + (int64_t)c * dim;
        float a = 0.f;
        for (int k = 0; k < dim; ++k) a = fmaf(wr[k], hid[k], a);
        a += b2[c];
        out[c] = a;
        if (temb != nullptr) temb[(int64_t)i * dim + c] = a;
    }
    if (e1w_t == nullptr) return;
    __syncthreads();
    for (int c = threadIdx.x; c < c1; c += blockDim.x) {
        const float* wr = e1w_t + (int64_t)c * dim;
        float a = 0.f;
        for (int k = 0; k < dim; ++k) a = fmaf(wr[k], out[k], a);
        tbias[(int64_t)i * c1 + c] = a + e1b[c];
    }
}

__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ x, int rows, int k,
                                                          const float* __restrict__ w, const float* __restrict__ b,
                                                          int c, float* __restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)rows * c) return;
    const int r = (int)(idx / c), cc = (int)(idx - (int64_t)r * c);
    const float* xr = x + (int64_t)r * k;
    const float* wr = w + (int64_t)cc * k;
    float a = 0.f;
    for (int j = 0; j < k; ++j) a = fmaf(wr[j], xr[j], a);
    y[idx] = a + (b != nullptr ? b[cc] : 0.f);
}

// ------------------------------------------------------ enc1.conv1, xyz half
// thread = (point, 8-channel chunk): 16-B coalesced fp16 stores, x broadcast within 8 lanes
__global__ __launch_bounds__(256) void enc1_xyz_kernel(const float* __restrict__ x, int64_t m, int rows_per_shape,
                                                        const float* __restrict__ w, int c1,
                                                        const float* __restrict__ tbias, int tb_stride,
                                                        half_t* __restrict__ out) {
    const int chunks = c1 / 8;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * chunks) return;
    const int64_t pt = idx / chunks;
    const int ch = (int)(idx - pt * chunks);
    const float px = x[pt * 3 + 0], py = x[pt * 3 + 1], pz = x[pt * 3 + 2];
    const float* tb = tbias + (int64_t)(pt / rows_per_shape) * tb_stride * c1 + ch * 8;
    const float* wr = w + (int64_t)ch * 8 * 3;
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = tb[e];
        v = fmaf(wr[e * 3 + 0], px, v);
        v = fmaf(wr[e * 3 + 1], py, v);
        v = fmaf(wr[e * 3 + 2], pz, v);
        o[e] = to_half_sat(fmaxf(v, 0.f));
    }
    *(half8*)(out + pt * c1 + ch * 8) = o;
}

// ---------------------------------------------------------------- output head
// eps[m][0..2] = W3 . h[m] + b3; one thread per point, h row read as 16-B pieces
template <int K>
__global__ __launch_bounds__(256) void head3_kernel(const half_t* __restrict__ h, int64_t m,
                                                     const float* __restrict__ w, const float* __restrict__ b,
                                                     float* __restrict__ eps) {
    __shared__ float ws[3 * K];
    for (int i = threadIdx.x; i < 3 * K; i += blockDim.x) ws[i] = w[i];
    __syncthreads();
    const int64_t pt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= m) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const half8* row = (const half8*)(h + pt * K);
#pragma unroll
    for (int cidx = 0; cidx < K / 8; ++cidx) {
        const half8 v = row[cidx];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = (float)v[e];
            a0 = fmaf(ws[cidx * 8 + e], f, a0);
            a1 = fmaf(ws[K + cidx * 8 + e], f, a1);
            a2 = fmaf(ws[2 * K + cidx * 8 + e], f, a2);
        }
    }
    eps[pt * 3 + 0] = a0 + b[0];
    eps[pt * 3 + 1] = a1 + b[1];
    eps[pt * 3 + 2] = a2 + b[2];
}

// ------------------------------------------------------------ diffusion updates
// Expression order follows the reference's torch-CPU ops (no FMA contraction) so that,
// given the same eps, results are bit-identical to diffusion.py:151,167,255,287.
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void add_noise_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                         const float* __restrict__ n, const float* __restrict__ s,
                                                         int stride, int64_t total, int64_t per_shape,
                                                         float* __restrict__ xt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = (i / per_shape) * stride;
    const float a = s[b] * x0[i];
    const float c = n[b] * noise[i];
    xt[i] = a + c;
}

__global__ __launch_bounds__(256) void remove_noise_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                            const float* __restrict__ n, const float* __restrict__ s,
                                                            int stride, int64_t total, int64_t per_shape,
                                                            float* __restrict__ x0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = (i / per_shape) * stride;
    const float ne = n[b] * eps[i];
    x0[i] = (xt[i] - ne) / s[b];
}

__global__ __launch_bounds__(256) void ddim_update_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                           const float* __restrict__ n, const float* __restrict__ s,
                                                           const float* __restrict__ n2, const float* __restrict__ s2,
                                                           int stride, int64_t total, int64_t per_shape,
                                                           float* __restrict__ x0o, float* __restrict__ xn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = (i / per_shape) * stride;
    const float e = eps[i];
    const float ne = n[b] * e;
    const float x0 = (x[i] - ne) / s[b];
    if (x0o != nullptr) x0o[i] = x0;
    if (xn != nullptr) {
        const float a = s2[b] * x0;
        const float c = n2[b] * e;
        xn[i] = a + c;
    }
}

// one element of the DDPM update (diffusion.py:246-255), shared by ddpm_update_kernel and the Philox-fused form below
__device__ __forceinline__ void ddpm_elem(float xv, float ev, float zv, float nb, float sb, float cb, float s2b, bool next, float& x0, float& xn) {
    const float ne = nb * ev;
    x0 = (xv - ne) / sb;
    xn = 0.f;
    if (next) {
        const float a = s2b * x0;
        const float cn = cb * nb;          // (coefficient * noise_rates) * noise, diffusion.py:255
        const float c = cn * zv;
        xn = a + c;
    }
}

__global__ __launch_bounds__(256) void ddpm_update_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                           const float* __restrict__ z, const float* __restrict__ n,
                                                           const float* __restrict__ s, const float* __restrict__ coef,
                                                           const float* __restrict__ s2, int stride, int64_t total,
                                                           int64_t per_shape, float* __restrict__ x0o,
                                                           float* __restrict__ xn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = (i / per_shape) * stride;
    const float ne = n[b] * eps[i];
    const float x0 = (x[i] - ne) / s[b];
    if (x0o != nullptr) x0o[i] = x0;
    if (xn != nullptr) {
        const float a = s2[b] * x0;
        const float cn = coef[b] * n[b];   // (coefficient * noise_rates) * noise, diffusion.py:255
        const float c = cn * z[i];
        xn[i] = a + c;
    }
}
#pragma clang fp contract(fast)

// Philox (philox_round, philox_normals4): device_prims.h
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // 4 outputs per thread
    if (q * 4 >= n) return;
    const uint64_t ctr = (uint64_t)q + offset;
    float v[4];
    philox_normals4(ctr, seed, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (q * 4 + e < n) out[q * 4 + e] = v[e];
}

__global__ __launch_bounds__(256) void f32_to_f16_kernel(const float* __restrict__ s, half_t* __restrict__ d, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = to_half_sat(s[i]);
}
__global__ __launch_bounds__(256) void f16_to_f32_kernel(const half_t* __restrict__ s, float* __restrict__ d, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = (float)s[i];
}

// x[m][c] += e[m / rows_per_shape][c]   (additive per-level time embeddings, networks.py:669-698)
__global__ __launch_bounds__(256) void add_shape_bias_kernel(const half_t* __restrict__ x, int64_t m, int c,
                                                              int rows_per_shape, const float* __restrict__ e,
                                                              int64_t e_stride, half_t* __restrict__ out) {
    const int chunks = c / 8;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * chunks) return;
    const int64_t row = idx / chunks;
    const int ch = (int)(idx - row * chunks);
    const float* er = e + (row / rows_per_shape) * e_stride + ch * 8;
    half8 v = *(const half8*)(x + row * c + ch * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = to_half_sat((float)v[i] + er[i]);
    *(half8*)(out + row * c + ch * 8) = v;
}

// Tail of UNetAttentionPointExperimental (networks.py:647-650,700-702): dec1 = PointNetLayer(128,3,3)
// on cat[a (ka ch) | b (kb ch)] followed by output = Conv1d(3,3).  BN folded; fp32 math per point.
// w1 [3][ka+kb], w2/w3/w4 [3][3], biases [3].
__global__ __launch_bounds__(256) void tail3_kernel(const half_t* __restrict__ a, int ka, const half_t* __restrict__ b,
                                                     int kb, int64_t m, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, const float* __restrict__ w234,
                                                     const float* __restrict__ b234, float* __restrict__ out) {
    extern __shared__ float ws[];   // w1 [3][ka+kb]
    const int k = ka + kb;
    for (int i = threadIdx.x; i < 3 * k; i += blockDim.x) ws[i] = w1[i];
    __syncthreads();
    const int64_t pt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= m) return;
    float h[3] = {b1[0], b1[1], b1[2]};
    for (int cidx = 0; cidx < ka / 8; ++cidx) {
        const half8 v = *(const half8*)(a + pt * ka + cidx * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = (float)v[e];
#pragma unroll
            for (int j = 0; j < 3; ++j) h[j] = fmaf(ws[j * k + cidx * 8 + e], f, h[j]);
        }
    }
    for (int cidx = 0; cidx < kb / 8; ++cidx) {
        const half8 v = *(const half8*)(b + pt * kb + cidx * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = (float)v[e];
#pragma unroll
            for (int j = 0; j < 3; ++j) h[j] = fmaf(ws[j * k + ka + cidx * 8 + e], f, h[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) h[j] = fmaxf(h[j], 0.f);
#pragma unroll
    for (int layer = 0; layer < 3; ++layer) {
        float o[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float acc = b234[layer * 3 + j];
#pragma unroll
            for (int i = 0; i < 3; ++i) acc = fmaf(w234[layer * 9 + j * 3 + i], h[i], acc);
            o[j] = layer < 2 ? fmaxf(acc, 0.f) : acc;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) h[j] = o[j];
    }
    out[pt * 3 + 0] = h[0]; out[pt * 3 + 1] = h[1]; out[pt * 3 + 2] = h[2];
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void reparam_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                       const float* __restrict__ eps, float* __restrict__ z, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float sd = expf(0.5f * lv[i]);
    const float e = eps[i] * sd;
    z[i] = mu[i] + e;
}
#pragma clang fp contract(fast)

// Device-side step selection so that ONE captured HIP graph can be replayed for every timestep:
// k = counter[0]; copy row k of the time-bias table and column k of the `cols` rate tables (four for the
// samplers, seven for a completion row) to fixed buffers; counter[1] = k (for consumers later in the step);
// counter[0] = k + 1.
__global__ __launch_bounds__(256) void step_select_kernel(int* __restrict__ counter, int n_steps,
                                                           const float* __restrict__ tb_table, int tb_elems,
                                                           float* __restrict__ tb_cur,
                                                           const float* __restrict__ rate_tables, int cols, int width,
                                                           float* __restrict__ rates_cur) {
    int k = counter[0];
    k = k < n_steps ? k : n_steps - 1;
    for (int i = threadIdx.x; i < tb_elems; i += blockDim.x) tb_cur[i] = tb_table[(int64_t)k * tb_elems + i];
    for (int i = threadIdx.x; i < cols * width; i += blockDim.x) {
        const int tbl = i / width, j = i - tbl * width;
        rates_cur[i] = rate_tables[((int64_t)tbl * n_steps + k) * width + j];
    }
    __syncthreads();
    if (threadIdx.x == 0) { counter[1] = k; counter[0] = k + 1; }
}

__global__ __launch_bounds__(256) void randn_step_kernel(float* __restrict__ out, int64_t n, uint64_t seed,
                                                          uint64_t base, uint64_t stride,
                                                          const int* __restrict__ counter) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= n) return;
    const uint64_t ctr = (uint64_t)q + base + stride * (uint64_t)counter[1];
    float v[4];
    philox_normals4(ctr, seed, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (q * 4 + e < n) out[q * 4 + e] = v[e];
}

static inline unsigned nblk(int64_t n) { return (unsigned)ceil_div(n, 256); }

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_time_embed(const float* t, int n_t, const float* freqs, int time_dim, int dim,
                              const float* w0, const float* b0, const float* w2, const float* b2,
                              float* temb, const float* e1w_t, const float* e1b, int c1, float* tbias,
                              void* stream) {
    PCD_CHECK_ARG(t && freqs && w0 && b0 && w2 && b2);
    PCD_CHECK_ARG(n_t > 0 && time_dim >= 2 && dim > 0);
    PCD_CHECK_ARG(temb != nullptr || e1w_t != nullptr);
    PCD_CHECK_ARG(e1w_t == nullptr || (e1b != nullptr && tbias != nullptr && c1 > 0));
    const size_t sm = (size_t)(time_dim + 2 * dim) * sizeof(float);
    hipLaunchKernelGGL(time_embed_kernel, dim3(n_t), dim3(256), sm, (hipStream_t)stream, t, freqs, time_dim, dim,
                       w0, b0, w2, b2, temb, e1w_t, e1b, c1, tbias);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_linear_f32(const float* x, int rows, int k, const float* w, const float* b, int c,
                              float* y, void* stream) {
    PCD_CHECK_ARG(x && w && y && rows > 0 && k > 0 && c > 0);
    hipLaunchKernelGGL(linear_f32_kernel, dim3(nblk((int64_t)rows * c)), dim3(256), 0, (hipStream_t)stream,
                       x, rows, k, w, b, c, y);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_enc1_xyz(const float* x, int64_t m, int rows_per_shape, const float* w_xyz, int c1,
                            const float* tbias, int tbias_shape_stride, void* out, void* stream) {
    PCD_CHECK_ARG(x && w_xyz && tbias && out);
    PCD_CHECK_ARG(m > 0 && rows_per_shape > 0 && c1 > 0 && c1 % 8 == 0);
    PCD_CHECK_ARG(tbias_shape_stride >= 0);
    hipLaunchKernelGGL(enc1_xyz_kernel, dim3(nblk(m * (c1 / 8))), dim3(256), 0, (hipStream_t)stream,
                       x, m, rows_per_shape, w_xyz, c1, tbias, tbias_shape_stride, (half_t*)out);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_head3(const void* h, int64_t m, int k, const float* w, const float* b, float* eps, void* stream) {
    PCD_CHECK_ARG(h && w && b && eps && m > 0);
    PCD_CHECK_ARG(k == 64);
    hipLaunchKernelGGL((head3_kernel<64>), dim3(nblk(m)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)h, m, w, b, eps);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_add_noise(const float* x0, const float* noise, const float* n, const float* s, int stride,
                             int64_t total, int64_t per_shape, float* x_t, void* stream) {
    PCD_CHECK_ARG(x0 && noise && n && s && x_t && total > 0 && per_shape > 0 && (stride == 0 || stride == 1));
    hipLaunchKernelGGL(add_noise_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream,
                       x0, noise, n, s, stride, total, per_shape, x_t);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_remove_noise(const float* x_t, const float* eps, const float* n, const float* s, int stride,
                                int64_t total, int64_t per_shape, float* x0, void* stream) {
    PCD_CHECK_ARG(x_t && eps && n && s && x0 && total > 0 && per_shape > 0 && (stride == 0 || stride == 1));
    hipLaunchKernelGGL(remove_noise_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream,
                       x_t, eps, n, s, stride, total, per_shape, x0);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_ddim_update(const float* x, const float* eps, const float* n, const float* s,
                               const float* n2, const float* s2, int stride, int64_t total, int64_t per_shape,
                               float* x0, float* x_next, void* stream) {
    PCD_CHECK_ARG(x && eps && n && s && total > 0 && per_shape > 0 && (stride == 0 || stride == 1));
    PCD_CHECK_ARG(x0 != nullptr || x_next != nullptr);
    PCD_CHECK_ARG(x_next == nullptr || (n2 != nullptr && s2 != nullptr));
    hipLaunchKernelGGL(ddim_update_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream,
                       x, eps, n, s, n2, s2, stride, total, per_shape, x0, x_next);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_ddpm_update(const float* x, const float* eps, const float* z, const float* n, const float* s,
                               const float* coef, const float* s2, int stride, int64_t total, int64_t per_shape,
                               float* x0, float* x_next, void* stream) {
    PCD_CHECK_ARG(x && eps && n && s && total > 0 && per_shape > 0 && (stride == 0 || stride == 1));
    PCD_CHECK_ARG(x0 != nullptr || x_next != nullptr);
    PCD_CHECK_ARG(x_next == nullptr || (z != nullptr && coef != nullptr && s2 != nullptr));
    hipLaunchKernelGGL(ddpm_update_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream,
                       x, eps, z, n, s, coef, s2, stride, total, per_shape, x0, x_next);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    PCD_CHECK_ARG(out && n > 0);
    hipLaunchKernelGGL(randn_kernel, dim3(nblk(ceil_div(n, 4))), dim3(256), 0, (hipStream_t)stream,
                       out, n, seed, offset);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_fill_zero(void* p, size_t bytes, void* stream) {
    PCD_CHECK_ARG(p != nullptr);
    if (bytes == 0) return PCD_OK;
    PCD_CHECK_HIP(hipMemsetAsync(p, 0, bytes, (hipStream_t)stream));
    return PCD_OK;
}

extern "C" int pcd_f32_to_f16(const float* src, void* dst, int64_t n, void* stream) {
    PCD_CHECK_ARG(src && dst && n > 0);
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, src, (half_t*)dst, n);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_f16_to_f32(const void* src, float* dst, int64_t n, void* stream) {
    PCD_CHECK_ARG(src && dst && n > 0);
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, (const half_t*)src, dst, n);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_add_shape_bias_strided_f16(const void* x, int64_t m, int c, int rows_per_shape, const float* e,
                                              int64_t e_stride, void* out, void* stream) {
    PCD_CHECK_ARG(x && e && out && m > 0 && c > 0 && c % 8 == 0 && rows_per_shape > 0 && e_stride >= 0);
    hipLaunchKernelGGL(add_shape_bias_kernel, dim3(nblk(m * (c / 8))), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, m, c, rows_per_shape, e, e_stride, (half_t*)out);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_add_shape_bias_f16(const void* x, int64_t m, int c, int rows_per_shape, const float* e, void* out,
                                      void* stream) {
    return pcd_add_shape_bias_strided_f16(x, m, c, rows_per_shape, e, c, out, stream);
}

extern "C" int pcd_tail3(const void* a, int ka, const void* b, int kb, int64_t m, const float* w1, const float* b1,
                         const float* w234, const float* b234, float* out, void* stream) {
    PCD_CHECK_ARG(a && b && w1 && b1 && w234 && b234 && out && m > 0);
    PCD_CHECK_ARG(ka > 0 && kb > 0 && ka % 8 == 0 && kb % 8 == 0 && ka + kb <= 4096);
    hipLaunchKernelGGL(tail3_kernel, dim3(nblk(m)), dim3(256), (size_t)3 * (ka + kb) * sizeof(float),
                       (hipStream_t)stream, (const half_t*)a, ka, (const half_t*)b, kb, m, w1, b1, w234, b234, out);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_reparameterize(const float* mu, const float* logvar, const float* eps, float* z, int64_t n,
                                  void* stream) {
    PCD_CHECK_ARG(mu && logvar && eps && z && n > 0);
    hipLaunchKernelGGL(reparam_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, mu, logvar, eps, z, n);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

// DDPM update with its normal draw generated in place: thread = 4 consecutive elements = one Philox counter, the counter layout and
// the Box-Muller arithmetic of randn_step_kernel, the update arithmetic of ddpm_update_kernel (ddpm_elem): bitwise the two launches
__global__ __launch_bounds__(256) void ddpm_update_philox_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                                  const float* __restrict__ n, const float* __restrict__ s,
                                                                  const float* __restrict__ coef, const float* __restrict__ s2,
                                                                  int stride, int64_t total, int64_t per_shape,
                                                                  float* __restrict__ x0o, float* __restrict__ xn, uint64_t seed,
                                                                  uint64_t base, uint64_t pstride, const int* __restrict__ counter) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= total) return;
    const uint64_t ctr = (uint64_t)q + base + pstride * (uint64_t)counter[1];
    float v[4];
    philox_normals4(ctr, seed, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t i = q * 4 + e;
        if (i >= total) break;
        const int64_t b = (i / per_shape) * stride;
        float x0, xv;
        ddpm_elem(x[i], eps[i], v[e], n[b], s[b], coef[b], s2[b], xn != nullptr, x0, xv);
        if (x0o != nullptr) x0o[i] = x0;
        if (xn != nullptr) xn[i] = xv;
    }
}

extern "C" int pcd_step_select(int* counter, int n_steps, const float* tb_table, int tb_elems, float* tb_cur,
                               const float* rate_tables, int width, float* rates_cur, void* stream) {
    return pcd_step_select_cols(counter, n_steps, tb_table, tb_elems, tb_cur, rate_tables, 4, width, rates_cur, stream);
}

extern "C" int pcd_step_select_cols(int* counter, int n_steps, const float* tb_table, int tb_elems, float* tb_cur,
                                    const float* rate_tables, int cols, int width, float* rates_cur, void* stream) {
    PCD_CHECK_ARG(counter && tb_table && tb_cur && rate_tables && rates_cur && n_steps > 0 && tb_elems > 0 && width > 0);
    PCD_CHECK_ARG(cols > 0 && cols <= 16);
    hipLaunchKernelGGL(step_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, counter, n_steps, tb_table,
                       tb_elems, tb_cur, rate_tables, cols, width, rates_cur);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_ddpm_update_philox(const float* x, const float* eps, const float* n, const float* s, const float* coef,
                                      const float* s2, int stride, int64_t total, int64_t per_shape, float* x0, float* x_next,
                                      uint64_t seed, uint64_t base_offset, uint64_t per_step_stride, const int* counter, void* stream) {
    PCD_CHECK_ARG(x && eps && n && s && coef && s2 && counter && total > 0 && per_shape > 0 && (stride == 0 || stride == 1));
    PCD_CHECK_ARG(x0 != nullptr || x_next != nullptr);
    hipLaunchKernelGGL(ddpm_update_philox_kernel, dim3(nblk(ceil_div(total, 4))), dim3(256), 0, (hipStream_t)stream, x, eps, n, s, coef, s2,
                       stride, total, per_shape, x0, x_next, seed, base_offset, per_step_stride, counter);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_randn_step(float* out, int64_t n, uint64_t seed, uint64_t base_offset, uint64_t per_step_stride,
                              const int* counter, void* stream) {
    PCD_CHECK_ARG(out && counter && n > 0);
    hipLaunchKernelGGL(randn_step_kernel, dim3(nblk(ceil_div(n, 4))), dim3(256), 0, (hipStream_t)stream, out, n, seed,
                       base_offset, per_step_stride, counter);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

// ------------------------------------------------------------ shape completion
// One row of `PointCloudDiffusion.complete`: the DDPM step of sample2 on the rows a shape does not know, the known points noised
// forward to the step's time on the rows it does, then (rows that carry one) the RePaint forward jump of the whole cloud.
// rates = the row's seven per-shape scalars [7][width]: n, s, coef, s_prev, n_prev, ja, jb (ja = 0 marks a row without a jump).
// A shape knows its first counts[shape] rows of `row_elems` floats.  Expression order follows tests/completion_statement.py.
#pragma clang fp contract(off)
__device__ __forceinline__ void complete_elem(float xv, float ev, float zv, float pv, bool known, float nb, float sb, float cb,
                                              float s2b, float n2b, bool next, float& x0, float& xn) {
    ddpm_elem(xv, ev, zv, nb, sb, cb, s2b, next, x0, xn);      // unknown rows: bitwise pcd_ddpm_update
    if (known) {
        if (next) {
            const float a = s2b * pv;
            const float c = n2b * zv;
            xn = a + c;
        } else {
            x0 = pv;                                           // last row: the known points as given
        }
    }
}

__device__ __forceinline__ float jump_elem(float xv, float z2v, float ja, float jb) {
    const float a = ja * xv;
    const float c = jb * z2v;
    return a + c;
}

// start state: known rows of x (the start draw) become s * p + n * x
__global__ __launch_bounds__(256) void complete_start_kernel(float* x, const float* __restrict__ p,
                                                              const int* __restrict__ counts, const float* __restrict__ n,
                                                              const float* __restrict__ s, int stride, int64_t total,
                                                              int64_t per_shape, int row_elems) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t sh = i / per_shape;
    if ((i - sh * per_shape) / row_elems >= counts[sh]) return;
    const int64_t b = sh * stride;
    const float a = s[b] * p[i];
    const float c = n[b] * x[i];
    x[i] = a + c;
}

// x and xn may be the same buffer (every element is read before it is written by the one thread that owns it)
__global__ __launch_bounds__(256) void complete_update_kernel(const float* x, const float* __restrict__ eps,
                                                               const float* __restrict__ z, const float* __restrict__ z2,
                                                               const float* __restrict__ p, const int* __restrict__ counts,
                                                               const float* __restrict__ rates, int width, int stride,
                                                               int64_t total, int64_t per_shape, int row_elems,
                                                               float* __restrict__ x0o, float* xn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t sh = i / per_shape;
    const int64_t b = sh * stride;
    const bool known = (i - sh * per_shape) / row_elems < counts[sh];
    const bool next = xn != nullptr;
    float x0, xv;
    complete_elem(x[i], eps[i], next ? z[i] : 0.f, known ? p[i] : 0.f, known, rates[b], rates[width + b], rates[2 * width + b],
                  rates[3 * width + b], rates[4 * width + b], next, x0, xv);
    if (x0o != nullptr) x0o[i] = x0;
    if (next) {
        if (z2 != nullptr) {
            const float ja = rates[5 * width + b];
            if (ja != 0.f) xv = jump_elem(xv, z2[i], ja, rates[6 * width + b]);
        }
        xn[i] = xv;
    }
}

// One step of `sample_dpm` (DPM-Solver++ 2M in data-prediction form; tests/dpm_statement.py).  rates = the step's six per-shape
// scalars [6][width]: n, s, n_next, s_next, c, q.  hist holds the previous step's x0 and receives this step's (read, then written by the
// one thread that owns the element).  c = h_k / (2 h_{k-1}) is 0 on the first step and for order 1: the history is then not read and the
// update is bitwise ddim_update_kernel's.  x and xn may be the same buffer.
__global__ __launch_bounds__(256) void dpm_update_kernel(const float* x, const float* __restrict__ eps,
                                                          const float* __restrict__ rates, int width, int stride, int64_t total,
                                                          int64_t per_shape, float* __restrict__ hist, float* xn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = (i / per_shape) * stride;
    const float e = eps[i];
    const float ne = rates[b] * e;
    const float x0 = (x[i] - ne) / rates[width + b];
    const float c = rates[4 * width + b];
    float D = x0, eD = e;
    if (c != 0.f) {
        const float w = c * (x0 - hist[i]);
        const float qw = rates[5 * width + b] * w;
        D = x0 + w;
        eD = e - qw;
    }
    hist[i] = x0;
    if (xn != nullptr) {
        const float a = rates[3 * width + b] * D;
        const float cc = rates[2 * width + b] * eD;
        xn[i] = a + cc;
    }
}
#pragma clang fp contract(fast)

// The same row with its normal draws generated in place (thread = 4 consecutive elements = one Philox counter, as in
// ddpm_update_philox_kernel): z from counter base + pstride * row + element / 4, and -- only in a run with jumps, and only on a row
// that carries one -- z2 from that counter + z2_off.  Neither is stored.
__global__ __launch_bounds__(256) void complete_update_philox_kernel(const float* x, const float* __restrict__ eps,
                                                                      const float* __restrict__ p, const int* __restrict__ counts,
                                                                      const float* __restrict__ rates, int width, int stride,
                                                                      int64_t total, int64_t per_shape, int row_elems, int jumps,
                                                                      float* __restrict__ x0o, float* xn, uint64_t seed,
                                                                      uint64_t base, uint64_t pstride, uint64_t z2_off,
                                                                      const int* __restrict__ counter) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= total) return;
    const bool next = xn != nullptr;
    const uint64_t ctr = (uint64_t)q + base + pstride * (uint64_t)counter[1];
    float v[4] = {0.f, 0.f, 0.f, 0.f}, v2[4] = {0.f, 0.f, 0.f, 0.f};
    if (next) philox_normals4(ctr, seed, v);
    // the 4 elements of a thread can straddle two shapes (per-shape rates): draw z2 when either end jumps
    bool any_jump = false;
    if (next && jumps) {
        const int64_t last = q * 4 + 3 < total ? q * 4 + 3 : total - 1;
        any_jump = rates[5 * width + (q * 4 / per_shape) * stride] != 0.f || rates[5 * width + (last / per_shape) * stride] != 0.f;
        if (any_jump) philox_normals4(ctr + z2_off, seed, v2);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t i = q * 4 + e;
        if (i >= total) break;
        const int64_t sh = i / per_shape;
        const int64_t b = sh * stride;
        const bool known = (i - sh * per_shape) / row_elems < counts[sh];
        float x0, xv;
        complete_elem(x[i], eps[i], v[e], known ? p[i] : 0.f, known, rates[b], rates[width + b], rates[2 * width + b],
                      rates[3 * width + b], rates[4 * width + b], next, x0, xv);
        if (x0o != nullptr) x0o[i] = x0;
        if (next) {
            if (any_jump) {
                const float ja = rates[5 * width + b];
                if (ja != 0.f) xv = jump_elem(xv, v2[e], ja, rates[6 * width + b]);
            }
            xn[i] = xv;
        }
    }
}

extern "C" int pcd_complete_start(float* x, const float* p, const int* counts, const float* n, const float* s, int stride,
                                  int64_t total, int64_t per_shape, int row_elems, void* stream) {
    PCD_CHECK_ARG(x && p && counts && n && s && total > 0 && per_shape > 0 && row_elems > 0 && (stride == 0 || stride == 1));
    PCD_CHECK_ARG(total % per_shape == 0 && per_shape % row_elems == 0);
    hipLaunchKernelGGL(complete_start_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, x, p, counts, n, s, stride,
                       total, per_shape, row_elems);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_complete_update(const float* x, const float* eps, const float* z, const float* z2, const float* p,
                                   const int* counts, const float* rates, int width, int stride, int64_t total,
                                   int64_t per_shape, int row_elems, float* x0, float* x_next, void* stream) {
    PCD_CHECK_ARG(x && eps && p && counts && rates && width > 0 && total > 0 && per_shape > 0 && row_elems > 0);
    PCD_CHECK_ARG(total % per_shape == 0 && per_shape % row_elems == 0);
    PCD_CHECK_ARG(stride == 0 || (stride == 1 && width == total / per_shape));
    PCD_CHECK_ARG(x0 != nullptr || x_next != nullptr);
    PCD_CHECK_ARG(x_next == nullptr || z != nullptr);
    hipLaunchKernelGGL(complete_update_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, x, eps, z, z2, p, counts,
                       rates, width, stride, total, per_shape, row_elems, x0, x_next);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_complete_update_philox(const float* x, const float* eps, const float* p, const int* counts,
                                          const float* rates, int width, int stride, int64_t total, int64_t per_shape,
                                          int row_elems, int jumps, float* x0, float* x_next, uint64_t seed,
                                          uint64_t base_offset, uint64_t per_step_stride, uint64_t z2_offset,
                                          const int* counter, void* stream) {
    PCD_CHECK_ARG(x && eps && p && counts && rates && counter && width > 0 && total > 0 && per_shape > 0 && row_elems > 0);
    PCD_CHECK_ARG(total % per_shape == 0 && per_shape % row_elems == 0);
    PCD_CHECK_ARG(stride == 0 || (stride == 1 && width == total / per_shape));
    PCD_CHECK_ARG(x0 != nullptr || x_next != nullptr);
    hipLaunchKernelGGL(complete_update_philox_kernel, dim3(nblk(ceil_div(total, 4))), dim3(256), 0, (hipStream_t)stream, x, eps,
                       p, counts, rates, width, stride, total, per_shape, row_elems, jumps, x0, x_next, seed, base_offset,
                       per_step_stride, z2_offset, counter);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_dpm_update(const float* x, const float* eps, const float* rates, int width, int stride, int64_t total,
                              int64_t per_shape, float* hist, float* x_next, void* stream) {
    PCD_CHECK_ARG(x && eps && rates && hist && width > 0 && total > 0 && per_shape > 0 && total % per_shape == 0);
    PCD_CHECK_ARG(stride == 0 || (stride == 1 && width == total / per_shape));
    hipLaunchKernelGGL(dpm_update_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, x, eps, rates, width, stride, total,
                       per_shape, hist, x_next);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

// ------------------------------------------------------------ classifier-free guidance
// step_select_kernel for a class-conditional run: instead of one copy of row k of the time-bias table it writes batch + 1 rows,
// row b = tb_table[k] + class_bias[labels[b]] and row `batch` = tb_table[k] + class_bias[null_row] (one fp32 add per element), so
// the conditional forward reads row 0 with shape stride 1 and the unconditional forward row `batch` with stride 0.  A label outside
// [0, class_rows) is read as null_row.  Rates and counter exactly as step_select_kernel; one block (the counter has one writer).
__global__ __launch_bounds__(1024) void step_select_labels_kernel(int* __restrict__ counter, int n_steps,
                                                                   const float* __restrict__ tb_table, int tb_elems,
                                                                   float* __restrict__ tb_rows, const float* __restrict__ class_bias,
                                                                   int class_rows, const int* __restrict__ labels, int batch,
                                                                   int null_row, const float* __restrict__ rate_tables, int cols,
                                                                   int width, float* __restrict__ rates_cur) {
    int k = counter[0];
    k = k < n_steps ? k : n_steps - 1;
    for (int i = threadIdx.x; i < (batch + 1) * tb_elems; i += blockDim.x) {
        const int b = i / tb_elems, e = i - b * tb_elems;
        int c = null_row;
        if (b < batch) {
            const int l = labels[b];
            if (l >= 0 && l < class_rows) c = l;
        }
        tb_rows[i] = tb_table[(int64_t)k * tb_elems + e] + class_bias[(int64_t)c * tb_elems + e];
    }
    for (int i = threadIdx.x; i < cols * width; i += blockDim.x) {
        const int tbl = i / width, j = i - tbl * width;
        rates_cur[i] = rate_tables[((int64_t)tbl * n_steps + k) * width + j];
    }
    __syncthreads();
    if (threadIdx.x == 0) { counter[1] = k; counter[0] = k + 1; }
}

// eps = eps_u + w * (eps - eps_u) in place, w per shape (w_stride 1) or shared (0).  VEC as in the AdamW kernel: lane i owns the floats
// [4 i, 4 i + 4) (16-byte accesses, both pointers 16-byte aligned), lane n / 4 the n % 4 tail; not VEC: one element per lane.
#pragma clang fp contract(off)
__device__ __forceinline__ float cfg_elem(float ec, float eu, float w) {
    const float d = ec - eu;
    const float wd = w * d;
    return eu + wd;
}

template <bool VEC>
__global__ __launch_bounds__(256) void cfg_combine_kernel(float* eps, const float* __restrict__ eps_u, const float* __restrict__ w,
                                                           int w_stride, int64_t n, int64_t per_shape) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const int64_t n4 = n / 4;
        if (i < n4) {
            float4 c = reinterpret_cast<float4*>(eps)[i];
            const float4 u = reinterpret_cast<const float4*>(eps_u)[i];
            const int64_t j = i * 4;
            c.x = cfg_elem(c.x, u.x, w[(j / per_shape) * w_stride]);
            c.y = cfg_elem(c.y, u.y, w[((j + 1) / per_shape) * w_stride]);
            c.z = cfg_elem(c.z, u.z, w[((j + 2) / per_shape) * w_stride]);
            c.w = cfg_elem(c.w, u.w, w[((j + 3) / per_shape) * w_stride]);
            reinterpret_cast<float4*>(eps)[i] = c;
        } else if (i == n4) {
            for (int64_t j = n4 * 4; j < n; ++j) eps[j] = cfg_elem(eps[j], eps_u[j], w[(j / per_shape) * w_stride]);
        }
    } else {
        if (i >= n) return;
        eps[i] = cfg_elem(eps[i], eps_u[i], w[(i / per_shape) * w_stride]);
    }
}
#pragma clang fp contract(fast)

extern "C" int pcd_step_select_labels(int* counter, int n_steps, const float* tb_table, int tb_elems, float* tb_rows,
                                      const float* class_bias, int class_rows, const int* labels, int batch, int null_row,
                                      const float* rate_tables, int cols, int width, float* rates_cur, void* stream) {
    PCD_CHECK_ARG(counter && tb_table && tb_rows && class_bias && labels && rate_tables && rates_cur);
    PCD_CHECK_ARG(n_steps > 0 && tb_elems > 0 && width > 0 && cols > 0 && cols <= 16);
    PCD_CHECK_ARG(batch > 0 && class_rows > 0 && null_row >= 0 && null_row < class_rows);
    PCD_CHECK_ARG(((int64_t)batch + 1) * tb_elems <= (int64_t)1 << 30);
    hipLaunchKernelGGL(step_select_labels_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counter, n_steps, tb_table, tb_elems,
                       tb_rows, class_bias, class_rows, labels, batch, null_row, rate_tables, cols, width, rates_cur);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_cfg_combine(float* eps, const float* eps_u, const float* w, int w_stride, int64_t n, int64_t per_shape,
                               void* stream) {
    PCD_CHECK_ARG(eps && eps_u && w && n > 0 && per_shape > 0 && (w_stride == 0 || w_stride == 1));
    if ((((uintptr_t)eps | (uintptr_t)eps_u) & 15) == 0)
        hipLaunchKernelGGL((cfg_combine_kernel<true>), dim3(nblk(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, eps, eps_u, w, w_stride, n,
                           per_shape);
    else
        hipLaunchKernelGGL((cfg_combine_kernel<false>), dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, eps, eps_u, w, w_stride, n,
                           per_shape);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
