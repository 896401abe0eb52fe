// Training kernels of the set-attention block (reference networks.py:51-83 under autograd):
//   * the log-sum-exp of the forward's scores (what the backward recomputes P from),
//   * the flash-style attention backward: dQ, dK, dV from softmax(Q K^T / sqrt d) V without the N x N matrix,
//   * LayerNorm with saved statistics, and its backward.
//
// Attention backward (per shape b and head h; S = Q K^T, P = exp(S / sqrt d - lse), dP = dO V^T, dS = P o (dP - delta),
// delta = rowsum(dO o O)):  dV = P^T dO,  dK = dS^T Q / sqrt d,  dQ = dS K / sqrt d.
// Two kernels, each owning its output rows, so every sum runs in one workgroup in a fixed order (bitwise reproducible,
// no atomics): a key-block kernel (dK, dV) and a query-block kernel (dQ); both recompute S and dP.
// Products on v_mfma_f32_16x16x32_f16 (lane l: A[m = l%16][k = 8(l/16)+i], B[k = 8(l/16)+i][n = l%16],
// D[m = 4(l/16)+r][n = l%16]).  The key (dK/dV kernel) or the query (dQ kernel) sits on the MFMA lane: the S / dP
// accumulators of two stacked 16-row tiles are then the 8-element operand of the next product directly, with the
// reduction index permuted as k(g, i) = i < 4 ? 4g + i : 16 + 4g + (i - 4); the other operand is read from a transposed
// LDS copy in the same order.
#include "common.h"
#include "layernorm_rows.h"

namespace pcd {

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int AT = 64;                  // rows per workgroup and per streamed tile (4 waves x 16)

__device__ __forceinline__ f32x4 mfma16(const half8& a, const half8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// 8 halfs of a row at column k0 (zero past d: d = 16 runs the K = 32 product half empty)
template <int D>
__device__ __forceinline__ half8 row8(const half_t* p, int k0) {
    if (D < 32 && k0 >= D) return half8{0, 0, 0, 0, 0, 0, 0, 0};
    return *(const half8*)(p + k0);
}

// operand in the permuted reduction order from a transposed image row t (32 columns from c0): t[c0+4g .. +3], t[c0+16+4g .. +3]
__device__ __forceinline__ half8 perm8(const half_t* t, int c0, int g) {
    const half4 a = *(const half4*)(t + c0 + 4 * g), b = *(const half4*)(t + c0 + 16 + 4 * g);
    return half8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

__device__ __forceinline__ half8 pack8(const f32x4& a, const f32x4& b) {
    return half8{(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3], (half_t)b[0], (half_t)b[1], (half_t)b[2], (half_t)b[3]};
}

// stage AT rows x D halfs (global row stride ld) into LDS rows of stride RS; optionally also transposed, [D][AT + 8]
template <int D, int RS, bool TR>
__device__ __forceinline__ void stage_rows(const half_t* __restrict__ src, int64_t ld, half_t* rows, half_t* tr) {
    constexpr int CPR = D / 8;
    for (int i = threadIdx.x; i < AT * CPR; i += 256) {
        const int r = i / CPR, c = (i % CPR) * 8;
        const half8 v = *(const half8*)(src + (int64_t)r * ld + c);
        *(half8*)(rows + r * RS + c) = v;
        if (TR) {
#pragma unroll
            for (int e = 0; e < 8; ++e) tr[(c + e) * (AT + 8) + r] = v[e];
        }
    }
}

// ---------------------------------------------------------------- log-sum-exp of the scores
// lse[bh][q] = ln sum_k exp(q . k / sqrt d), exact (running max per lane, combined over the four lane groups at the end)
template <int D>
__global__ __launch_bounds__(256) void attn_lse_kernel(const half_t* __restrict__ qkv, int n, int c, int heads,
                                                       float* __restrict__ lse) {
    constexpr int KC = (D + 31) / 32, RS = D + 8;
    __shared__ __attribute__((aligned(16))) half_t ks[AT * RS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
    const int64_t ld = 3 * (int64_t)c;
    const half_t* base = qkv + (int64_t)b * n * ld + h * D;
    const int q = blockIdx.x * AT + wave * 16 + l16;
    half8 qf[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = row8<D>(base + (int64_t)q * ld, kc * 32 + g * 8);
    const float sc = kLog2e / sqrtf((float)D);
    float m = -INFINITY, s = 0.f;
    for (int k0 = 0; k0 < n; k0 += AT) {
        __syncthreads();
        stage_rows<D, RS, false>(base + c + (int64_t)k0 * ld, ld, ks, nullptr);
        __syncthreads();
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) acc[mt] = mfma16(row8<D>(ks + (mt * 16 + l16) * RS, kc * 32 + g * 8), qf[kc], acc[mt]);
        }
        float tm = m;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) tm = fmaxf(tm, acc[mt][r] * sc);
        float add = 0.f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) add += exp2f(acc[mt][r] * sc - tm);
        s = s * exp2f(m - tm) + add;
        m = tm;
    }
    // the four lane groups g hold disjoint keys of the same query
    float mm = fmaxf(m, __shfl_xor(m, 16));
    mm = fmaxf(mm, __shfl_xor(mm, 32));
    float ss = s * exp2f(m - mm);
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    if (g == 0) lse[(int64_t)bh * n + q] = (mm + log2f(ss)) * 0.6931471805599453f;
}

// ---------------------------------------------------------------- delta = rowsum(dO o O) per (row, head)
template <int D>
__global__ __launch_bounds__(256) void attn_delta_kernel(const half_t* __restrict__ out, const half_t* __restrict__ dout,
                                                         int64_t rows, int n, int c, int heads, float* __restrict__ delta) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * heads) return;
    const int64_t row = i / heads;
    const int h = (int)(i % heads);
    const half_t* o = out + row * c + h * D;
    const half_t* d = dout + row * c + h * D;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < D; k += 8) {
        const half8 a = *(const half8*)(o + k), bb = *(const half8*)(d + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += (float)a[e] * (float)bb[e];
    }
    const int64_t b = row / n, q = row % n;
    delta[(b * heads + h) * n + q] = acc;
}

// ---------------------------------------------------------------- dK, dV: a workgroup owns 64 keys, streams every query
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ dout,
                                                            const float* __restrict__ lse, const float* __restrict__ delta,
                                                            int n, int c, int heads, half_t* __restrict__ dqkv) {
    constexpr int KC = (D + 31) / 32, NT = D / 16, RS = D + 8, TS = AT + 8;
    __shared__ __attribute__((aligned(16))) half_t qs[AT * RS];
    __shared__ __attribute__((aligned(16))) half_t os[AT * RS];
    __shared__ __attribute__((aligned(16))) half_t qt[D * TS];
    __shared__ __attribute__((aligned(16))) half_t ot[D * TS];
    __shared__ __attribute__((aligned(16))) float ls[AT];
    __shared__ __attribute__((aligned(16))) float ds[AT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
    const int64_t ld = 3 * (int64_t)c;
    const half_t* base = qkv + (int64_t)b * n * ld + h * D;
    const half_t* dbase = dout + (int64_t)b * n * c + h * D;
    const int key = blockIdx.x * AT + wave * 16 + l16;
    half8 kf[KC], vf[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        kf[kc] = row8<D>(base + (int64_t)key * ld + c, kc * 32 + g * 8);
        vf[kc] = row8<D>(base + (int64_t)key * ld + 2 * c, kc * 32 + g * 8);
    }
    const float sc = kLog2e / sqrtf((float)D);
    f32x4 dv[NT], dk[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dv[t] = dk[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < n; q0 += AT) {
        __syncthreads();
        stage_rows<D, RS, true>(base + (int64_t)q0 * ld, ld, qs, qt);
        stage_rows<D, RS, true>(dbase + (int64_t)q0 * c, c, os, ot);
        if (threadIdx.x < AT) ls[threadIdx.x] = lse[(int64_t)bh * n + q0 + threadIdx.x] * kLog2e;
        else if (threadIdx.x < 2 * AT) ds[threadIdx.x - AT] = delta[(int64_t)bh * n + q0 + threadIdx.x - AT];
        __syncthreads();
        // S[q][key] and dP[q][key] for the 64 queries (4 tiles of 16), key on the lane
        half8 pf[2], dsf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f32x4 p2[2], d2[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int mt = 2 * ks + j;
                f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = s;
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) {
                    s = mfma16(row8<D>(qs + (mt * 16 + l16) * RS, kc * 32 + g * 8), kf[kc], s);
                    dp = mfma16(row8<D>(os + (mt * 16 + l16) * RS, kc * 32 + g * 8), vf[kc], dp);
                }
                const f32x4 l4 = *(const f32x4*)(ls + mt * 16 + 4 * g), d4 = *(const f32x4*)(ds + mt * 16 + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = exp2f(s[r] * sc - l4[r]);
                    p2[j][r] = p;
                    d2[j][r] = p * (dp[r] - d4[r]);
                }
            }
            pf[ks] = pack8(p2[0], p2[1]);
            dsf[ks] = pack8(d2[0], d2[1]);
        }
        // dV^T[dd][key] += dO^T P,  dK^T[dd][key] += Q^T dS   (reduction over the 64 queries: two K = 32 steps)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const half_t* orow = ot + (t * 16 + l16) * TS;
            const half_t* qrow = qt + (t * 16 + l16) * TS;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                dv[t] = mfma16(perm8(orow, 32 * ks, g), pf[ks], dv[t]);
                dk[t] = mfma16(perm8(qrow, 32 * ks, g), dsf[ks], dk[t]);
            }
        }
    }
    // lane: key, dd = 16t + 4g + r (four consecutive columns: one 8-byte store each)
    const float rs = 1.f / sqrtf((float)D);
    half_t* drow = dqkv + ((int64_t)b * n + key) * ld + h * D;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int dd = t * 16 + 4 * g;
        *(half4*)(drow + c + dd) = half4{to_half_sat(dk[t][0] * rs), to_half_sat(dk[t][1] * rs), to_half_sat(dk[t][2] * rs),
                                         to_half_sat(dk[t][3] * rs)};
        *(half4*)(drow + 2 * c + dd) = half4{to_half_sat(dv[t][0]), to_half_sat(dv[t][1]), to_half_sat(dv[t][2]), to_half_sat(dv[t][3])};
    }
}

// ---------------------------------------------------------------- dQ: a workgroup owns 64 queries, streams every key
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          int n, int c, int heads, half_t* __restrict__ dqkv) {
    constexpr int KC = (D + 31) / 32, NT = D / 16, RS = D + 8, TS = AT + 8;
    __shared__ __attribute__((aligned(16))) half_t kk[AT * RS];
    __shared__ __attribute__((aligned(16))) half_t vv[AT * RS];
    __shared__ __attribute__((aligned(16))) half_t kt[D * TS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
    const int64_t ld = 3 * (int64_t)c;
    const half_t* base = qkv + (int64_t)b * n * ld + h * D;
    const int q = blockIdx.x * AT + wave * 16 + l16;
    half8 qf[KC], of[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        qf[kc] = row8<D>(base + (int64_t)q * ld, kc * 32 + g * 8);
        of[kc] = row8<D>(dout + ((int64_t)b * n + q) * c + h * D, kc * 32 + g * 8);
    }
    const float sc = kLog2e / sqrtf((float)D);
    const float l2 = lse[(int64_t)bh * n + q] * kLog2e, dl = delta[(int64_t)bh * n + q];
    f32x4 dq[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < n; k0 += AT) {
        __syncthreads();
        stage_rows<D, RS, true>(base + c + (int64_t)k0 * ld, ld, kk, kt);
        stage_rows<D, RS, false>(base + 2 * c + (int64_t)k0 * ld, ld, vv, nullptr);
        __syncthreads();
        // S^T[key][q], dP^T[key][q] (query on the lane) -> dS as the A operand of dQ = dS K
        half8 dsf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f32x4 d2[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int mt = 2 * ks + j;
                f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = s;
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) {
                    s = mfma16(row8<D>(kk + (mt * 16 + l16) * RS, kc * 32 + g * 8), qf[kc], s);
                    dp = mfma16(row8<D>(vv + (mt * 16 + l16) * RS, kc * 32 + g * 8), of[kc], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) d2[j][r] = exp2f(s[r] * sc - l2) * (dp[r] - dl);
            }
            dsf[ks] = pack8(d2[0], d2[1]);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const half_t* krow = kt + (t * 16 + l16) * TS;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) dq[t] = mfma16(dsf[ks], perm8(krow, 32 * ks, g), dq[t]);
        }
    }
    // D[m = query 4g + r of this wave][n = dd 16t + l16]
    const float rs = 1.f / sqrtf((float)D);
    const int64_t row0 = (int64_t)b * n + blockIdx.x * AT + wave * 16 + 4 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dqkv[(row0 + r) * ld + h * D + t * 16 + l16] = to_half_sat(dq[t][r] * rs);
}

// ---------------------------------------------------------------- LayerNorm backward
// (the forward with saved statistics is layernorm_rows_kernel<LPR, true> of layernorm_rows.h)
// dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) [+ dx]; per-workgroup partial sums of dy xhat and dy into
// slab[blockIdx.x] = [dgamma C | dbeta C] (summed in a fixed order by ln_sum_slabs_kernel).  x - mean in fp32.
template <int LPR>
__global__ __launch_bounds__(256) void layernorm_backward_kernel(const half_t* __restrict__ dy, const half_t* __restrict__ x,
                                                                 int64_t rows, const float* __restrict__ mean_in,
                                                                 const float* __restrict__ rstd_in, const float* __restrict__ gamma,
                                                                 int accumulate, half_t* __restrict__ dx,
                                                                 float* __restrict__ slabs) {
    constexpr int C = LPR * 8, RPW = 64 / LPR;
    __shared__ __attribute__((aligned(16))) float red[4][2 * C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane % LPR;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = gamma[l * 8 + e];
    float pg[8], pb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) pg[e] = pb[e] = 0.f;
    const int64_t groups = (rows + RPW - 1) / RPW;           // row groups of RPW rows, one per wave step
    for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < groups; grp += (int64_t)gridDim.x * 4) {
        const int64_t row = grp * RPW + lane / LPR;
        const bool ok = row < rows;
        const int64_t rr = ok ? row : rows - 1;
        const half8 xv = *(const half8*)(x + rr * C + l * 8), gv = *(const half8*)(dy + rr * C + l * 8);
        const float mu = mean_in[rr], rs = rstd_in[rr];
        float xh[8], gd[8], a = 0.f, bsum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            xh[e] = ((float)xv[e] - mu) * rs;
            gd[e] = (float)gv[e] * f[e];
            a += gd[e];
            bsum += gd[e] * xh[e];
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) { a += __shfl_xor(a, o); bsum += __shfl_xor(bsum, o); }
        a /= (float)C;
        bsum /= (float)C;
        if (ok) {
            half8 o8;
            half8 prev = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (accumulate) prev = *(const half8*)(dx + row * C + l * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) o8[e] = to_half_sat(rs * (gd[e] - a - xh[e] * bsum) + (float)prev[e]);
            *(half8*)(dx + row * C + l * 8) = o8;
#pragma unroll
            for (int e = 0; e < 8; ++e) { pg[e] += (float)gv[e] * xh[e]; pb[e] += (float)gv[e]; }
        }
    }
    // lanes l, l + LPR, ... hold the same channels
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) { pg[e] += __shfl_xor(pg[e], o); pb[e] += __shfl_xor(pb[e], o); }
    if (lane < LPR) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { red[wave][l * 8 + e] = pg[e]; red[wave][C + l * 8 + e] = pb[e]; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256)
        slabs[(int64_t)blockIdx.x * 2 * C + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

__global__ __launch_bounds__(256) void ln_sum_slabs_kernel(const float* __restrict__ slabs, int nslabs, int c,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * c) return;
    float s = 0.f;
    for (int k = 0; k < nslabs; ++k) s += slabs[(int64_t)k * 2 * c + i];
    if (i < c) dgamma[i] = s;
    else dbeta[i - c] = s;
}

int ln_slabs(int64_t rows) {
    const int64_t blocks = ceil_div(rows, 64);
    return (int)(blocks < 256 ? blocks : 256);
}

}  // namespace

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_set_attention_lse_f16(const void* qkv, int batch, int n_points, int c, int heads, void* out, float* lse,
                                         void* stream) {
    PCD_CHECK_ARG(qkv && out && lse && batch > 0 && n_points > 0 && heads > 0 && c % heads == 0);
    PCD_CHECK_ARG(n_points % AT == 0);
    const int d = c / heads;
    PCD_CHECK_ARG(d == 16 || d == 32 || d == 64);
    int rc = pcd_set_attention_f16(qkv, batch, n_points, c, heads, out, nullptr, 0, stream);
    if (rc) return rc;
    const dim3 grid((unsigned)(n_points / AT), (unsigned)(batch * heads));
    hipStream_t s = (hipStream_t)stream;
    const half_t* q = (const half_t*)qkv;
    if (d == 16) hipLaunchKernelGGL(attn_lse_kernel<16>, grid, dim3(256), 0, s, q, n_points, c, heads, lse);
    else if (d == 32) hipLaunchKernelGGL(attn_lse_kernel<32>, grid, dim3(256), 0, s, q, n_points, c, heads, lse);
    else hipLaunchKernelGGL(attn_lse_kernel<64>, grid, dim3(256), 0, s, q, n_points, c, heads, lse);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_set_attention_backward_workspace_bytes(int batch, int n_points, int c, int heads) {
    if (batch <= 0 || n_points <= 0 || c <= 0 || heads <= 0) return 0;
    return sizeof(float) * (size_t)batch * (size_t)heads * (size_t)n_points;
}

extern "C" int pcd_set_attention_backward_f16(const void* qkv, const void* out, const void* dout, const float* lse, int batch,
                                              int n_points, int c, int heads, void* dqkv, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    PCD_CHECK_ARG(qkv && out && dout && lse && dqkv && workspace && batch > 0 && n_points > 0 && heads > 0 && c % heads == 0);
    PCD_CHECK_ARG(n_points % AT == 0);
    const int d = c / heads;
    PCD_CHECK_ARG(d == 16 || d == 32 || d == 64);
    PCD_CHECK_ARG((int64_t)batch * n_points <= 0x7fffffff && (int64_t)batch * heads <= 65535);
    if (workspace_bytes < pcd_set_attention_backward_workspace_bytes(batch, n_points, c, heads)) {
        set_error("pcd_set_attention_backward_f16: workspace %zu < required %zu", workspace_bytes,
                  pcd_set_attention_backward_workspace_bytes(batch, n_points, c, heads));
        return PCD_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)batch * n_points;
    float* delta = (float*)workspace;
    const half_t *q = (const half_t*)qkv, *o = (const half_t*)out, *dO = (const half_t*)dout;
    half_t* dq = (half_t*)dqkv;
    const dim3 dgrid((unsigned)ceil_div(rows * heads, 256));
    const dim3 grid((unsigned)(n_points / AT), (unsigned)(batch * heads));
#define PCD_ATTN_BWD(D)                                                                                                     \
    hipLaunchKernelGGL(attn_delta_kernel<D>, dgrid, dim3(256), 0, s, o, dO, rows, n_points, c, heads, delta);                \
    hipLaunchKernelGGL(attn_bwd_dkdv_kernel<D>, grid, dim3(256), 0, s, q, dO, lse, delta, n_points, c, heads, dq);           \
    hipLaunchKernelGGL(attn_bwd_dq_kernel<D>, grid, dim3(256), 0, s, q, dO, lse, delta, n_points, c, heads, dq);
    if (d == 16) { PCD_ATTN_BWD(16) }
    else if (d == 32) { PCD_ATTN_BWD(32) }
    else { PCD_ATTN_BWD(64) }
#undef PCD_ATTN_BWD
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_layernorm_train_f16(const void* x, int64_t rows, int c, const float* gamma, const float* beta, void* out,
                                       float* mean, float* rstd, void* stream) {
    PCD_CHECK_ARG(x && gamma && beta && out && mean && rstd && rows > 0);
    PCD_CHECK_ARG(c == 64 || c == 128 || c == 256);
    hipStream_t s = (hipStream_t)stream;
    const half_t* x16 = (const half_t*)x;
    half_t* o16 = (half_t*)out;
    ln_launch(c, [&](auto lpr) {
        hipLaunchKernelGGL((layernorm_rows_kernel<decltype(lpr)::value, true>), dim3(ln_row_blocks(rows, c)), dim3(256), 0, s, x16, rows, gamma, beta, o16, mean, rstd);
    });
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_layernorm_backward_workspace_bytes(int64_t rows, int c) {
    if (rows <= 0 || c <= 0) return 0;
    return sizeof(float) * 2 * (size_t)c * (size_t)ln_slabs(rows);
}

extern "C" int pcd_layernorm_backward_f16(const void* dy, const void* x, int64_t rows, int c, const float* mean, const float* rstd,
                                          const float* gamma, int accumulate, void* dx, float* dgamma, float* dbeta,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    PCD_CHECK_ARG(dy && x && mean && rstd && gamma && dx && dgamma && dbeta && workspace && rows > 0 && dy != dx);
    PCD_CHECK_ARG(c == 64 || c == 128 || c == 256);
    if (workspace_bytes < pcd_layernorm_backward_workspace_bytes(rows, c)) {
        set_error("pcd_layernorm_backward_f16: workspace %zu < required %zu", workspace_bytes,
                  pcd_layernorm_backward_workspace_bytes(rows, c));
        return PCD_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int nb = ln_slabs(rows);
    float* slabs = (float*)workspace;
    const half_t *g16 = (const half_t*)dy, *x16 = (const half_t*)x;
    half_t* d16 = (half_t*)dx;
    ln_launch(c, [&](auto lpr) {
        hipLaunchKernelGGL(layernorm_backward_kernel<decltype(lpr)::value>, dim3(nb), dim3(256), 0, s, g16, x16, rows, mean, rstd, gamma, accumulate, d16, slabs);
    });
    hipLaunchKernelGGL(ln_sum_slabs_kernel, dim3((unsigned)ceil_div(2 * c, 256)), dim3(256), 0, s, slabs, nb, c, dgamma, dbeta);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
