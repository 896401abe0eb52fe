// The vectorised LayerNorm row of the attention U-Net's widths, written once: attention.hip instantiates it without the saved
// statistics (pcd_layernorm_f16), attn_bwd.hip with them (pcd_layernorm_train_f16), and the two must give the same bits
// (tests/test_gpu_layernorm_rows.py) although the two files are compiled with different flags.
#pragma once
#include <type_traits>
#include "common.h"

namespace pcd {

// C = 8 * LPR (64 / 128 / 256): a row is LPR lanes x 16 bytes, read once and kept in registers through both statistics passes
// and the output (layernorm_kernel in attention.hip reads every element three times, two bytes per lane and access: 3x off the
// HBM time of this purely bandwidth-bound step); 64 / LPR rows per wave.  fp32 statistics, biased variance, eps inside the sqrt
// (torch semantics).  STATS: mean / rstd per row go out as well, for the backward.
// The fused multiply-adds of the variance are spelled out: left to contraction, `q += f[e] * f[e]` came out as a chain of
// v_fmac under one file's flags and as v_pk_mul + v_add (every square rounded) under the other's, rstd differed in its last
// bit and a few outputs by an fp16 ulp.
template <int LPR, bool STATS>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const half_t* __restrict__ x, int64_t rows,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              half_t* __restrict__ out, float* __restrict__ mean_out,
                                                              float* __restrict__ rstd_out) {
    constexpr int C = LPR * 8, RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, l = lane % LPR;
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const int64_t rr = row < rows ? row : rows - 1;                    // whole groups stay active for the shuffles
    const half8 v = *(const half8*)(x + rr * C + l * 8);
    float f[8];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { f[e] = (float)v[e]; s += f[e]; }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] -= mean;
    float q = f[1] * f[1];                           // f1^2 rounded, the others fused: the form the contracted sum had taken
    q = __builtin_fmaf(f[0], f[0], q);
#pragma unroll
    for (int e = 2; e < 8; ++e) q = __builtin_fmaf(f[e], f[e], q);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)C + 1e-5f);
    const f32x4 g0 = *(const f32x4*)(gamma + l * 8), g1 = *(const f32x4*)(gamma + l * 8 + 4);
    const f32x4 b0 = *(const f32x4*)(beta + l * 8), b1 = *(const f32x4*)(beta + l * 8 + 4);
    half8 o8;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o8[e] = to_half_sat(__builtin_fmaf(f[e] * rstd, g0[e], b0[e]));
        o8[4 + e] = to_half_sat(__builtin_fmaf(f[4 + e] * rstd, g1[e], b1[e]));
    }
    if (row < rows) {
        *(half8*)(out + row * C + l * 8) = o8;
        if (STATS && l == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    }
}

// blocks of 256 threads x 8 halfs: 2048 / c rows each
static inline unsigned ln_row_blocks(int64_t rows, int c) { return (unsigned)ceil_div(rows, 2048 / c); }

// The c == 64 / 128 / 256 ladder of every kernel templated on LPR = c / 8: launch(std::integral_constant<int, LPR>) makes
// the one launch; false (nothing launched) for any other c.
template <typename Launch>
static inline bool ln_launch(int c, Launch&& launch) {
    if (c == 64) launch(std::integral_constant<int, 8>{});
    else if (c == 128) launch(std::integral_constant<int, 16>{});
    else if (c == 256) launch(std::integral_constant<int, 32>{});
    else return false;
    return true;
}

}  // namespace pcd
