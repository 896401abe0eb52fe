// K9: the two degenerate layers of VAE3DLarge that are not GEMM shaped -- the first conv (Cin = 1,
// K = 27) and the last conv (Cout = 1) with its sigmoid.
#include "conv3d.h"

namespace pcd {

// first layer: x fp32 [B][D][H][W] (Cin = 1), k3 s1 p1 -> fp16 NDHWC [..][cout], ReLU.
// thread = (voxel, 8-channel chunk); w fp32 [cout][27], b fp32 [cout]
__global__ __launch_bounds__(256) void conv3d_first_kernel(const float* __restrict__ x, int B, int D, int H, int W,
                                                            int stride, const float* __restrict__ w,
                                                            const float* __restrict__ b, int cout,
                                                            half_t* __restrict__ out) {
    extern __shared__ float ws[];   // [cout][27] + [cout]
    for (int i = threadIdx.x; i < cout * 28; i += blockDim.x) ws[i] = i < cout * 27 ? w[i] : b[i - cout * 27];
    __syncthreads();
    const int chunks = cout / 8;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;   // k3, pad 1
    const int64_t nvox = (int64_t)B * Do * Ho * Wo;
    if (idx >= nvox * chunks) return;
    const int64_t vox = idx / chunks;
    const int ch = (int)(idx - vox * chunks);
    int xx = (int)(vox % Wo); int64_t t = vox / Wo;
    int yy = (int)(t % Ho); t /= Ho;
    int zz = (int)(t % Do); const int bb = (int)(t / Do);
    xx *= stride; yy *= stride; zz *= stride;
    float tap[27];
#pragma unroll
    for (int kz = 0; kz < 3; ++kz)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iz = zz + kz - 1, iy = yy + ky - 1, ix = xx + kx - 1;
                const bool ok = (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                tap[(kz * 3 + ky) * 3 + kx] = ok ? x[(((int64_t)bb * D + iz) * H + iy) * W + ix] : 0.f;
            }
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ch * 8 + e;
        float a = ws[cout * 27 + c];
#pragma unroll
        for (int k = 0; k < 27; ++k) a = fmaf(ws[c * 27 + k], tap[k], a);
        o[e] = to_half_sat(fmaxf(a, 0.f));
    }
    *(half8*)(out + vox * cout + ch * 8) = o;
}

// first layer, cout = 32 fast path: thread = voxel, all 32 output channels.  Weight indices are wave-uniform, so
// they are scalar loads and the 864 FMAs per voxel take an SGPR operand (the generic kernel above reads one LDS
// word per FMA, which is what bounds it).
__global__ __launch_bounds__(256) void conv3d_first32_kernel(const float* __restrict__ x, int B, int D, int H, int W,
                                                              int stride, const float* __restrict__ w,
                                                              const float* __restrict__ b, half_t* __restrict__ out) {
    constexpr int COUT = 32;
    const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;   // k3, pad 1
    const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vox >= (int64_t)B * Do * Ho * Wo) return;
    int xx = (int)(vox % Wo); int64_t t = vox / Wo;
    int yy = (int)(t % Ho); t /= Ho;
    int zz = (int)(t % Do); const int bb = (int)(t / Do);
    xx *= stride; yy *= stride; zz *= stride;
    float tap[27];
#pragma unroll
    for (int kz = 0; kz < 3; ++kz)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iz = zz + kz - 1, iy = yy + ky - 1, ix = xx + kx - 1;
                const bool ok = (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                const int cz = min(max(iz, 0), D - 1), cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
                const float v = x[(((int64_t)bb * D + cz) * H + cy) * W + cx];
                tap[(kz * 3 + ky) * 3 + kx] = ok ? v : 0.f;
            }
    half_t* o = out + vox * COUT;
#pragma unroll
    for (int c8 = 0; c8 < COUT / 8; ++c8) {
        half8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c8 * 8 + e;
            float a = b[c];
#pragma unroll
            for (int k = 0; k < 27; ++k) a = fmaf(w[c * 27 + k], tap[k], a);
            r[e] = to_half_sat(fmaxf(a, 0.f));
        }
        *(half8*)(o + c8 * 8) = r;
    }
}

// encoder.0 on the matrix cores (stride 1, cout = 32, D % 4 == H % 4 == W % 8 == 0).  The VALU form above spends 864 fp32 FMAs
// per voxel (27 taps x 32 channels): 57 us at B = 32, five times what writing the 67 MB of output takes.  Here the layer is
// the product D[channel][voxel] = W[channel][tap] . im2col[tap][voxel] with K = 27 taps padded to one 32-deep MFMA step:
// weights (rounded to fp16 like every other layer's) are the A operand, held in registers; a workgroup keeps the fp16 image of
// its 6 x 6 x 10 input halo in LDS (720 B) and a lane gathers the eight taps of its k chunk for its voxel from it; the
// accumulator of a lane is 4 consecutive channels of one voxel = an 8-byte piece of the NDHWC output row.
// TZ x TY x 8 output voxels per tile (4 x 4 x 8, or 8 x 8 x 8 where the grid divides: the kernel is bound by instruction ISSUE -- 470 instructions per wave and
// 4 x 4 x 8 tile, of which 120 stage the halo and 60 decode the tile index; with 512 voxels per tile they are spread over four times the MFMA groups: 31 -> ~20 us)
template <int TZ, int TY>
__global__ __launch_bounds__(256) void conv3d_first32_mfma_kernel(const float* __restrict__ x, int B, int D, int H, int W,
                                                                   const float* __restrict__ w,
                                                                   const float* __restrict__ bias, half_t* __restrict__ out,
                                                                   int ntz, int nty, int ntx, int ntiles) {
    constexpr int HTZ = TZ, HTY = TY, HHY = HTY + 2, HROWS = (HTZ + 2) * HHY * HHX, GROUPS = TZ * TY * 8 / 16 / 4, YB = TY == 8 ? 3 : 2;   // (shadow the file's 128-row geometry)
    __shared__ half_t halo[2][HROWS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    // weights and tap offsets once per workgroup (it walks several tiles)
    half8 wa[2];
    int off[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int tap = 8 * q + j;                         // taps 27..31 are K padding: zero weights, any finite input
        const bool real = tap < 27;
        const int tc = real ? tap : 0;
        wa[0][j] = real ? (half_t)w[r * 27 + tc] : (half_t)0.f;
        wa[1][j] = real ? (half_t)w[(16 + r) * 27 + tc] : (half_t)0.f;
        off[j] = ((tc / 9) * HHY + (tc / 3) % 3) * HHX + tc % 3;
    }
    const f32x4 b0 = *(const f32x4*)(bias + 4 * q), b1 = *(const f32x4*)(bias + 16 + 4 * q);
    int buf = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, buf ^= 1) {
        int t = tile;
        const int tx = t % ntx; t /= ntx;
        const int ty = t % nty; t /= nty;
        const int tz = t % ntz; const int b = t / ntz;
        const int z0 = tz * HTZ, y0 = ty * HTY, x0 = tx * HTX;
        constexpr int SIT = (HROWS + 255) / 256;
        float hv[SIT];
#pragma unroll
        for (int it = 0; it < SIT; ++it) {                 // every load of the halo in flight before the first LDS store
            const int i = it * 256 + tid;
            const int hx = i % HHX; const int r2 = i / HHX;
            const int hy = r2 % HHY, hz = r2 / HHY;
            const int iz = z0 - 1 + hz, iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            const bool ok = i < HROWS && (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
            const int cz = min(max(iz, 0), D - 1), cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
            const float v = x[(((int64_t)b * D + cz) * H + cy) * W + cx];
            hv[it] = ok ? v : 0.f;
        }
#pragma unroll
        for (int it = 0; it < SIT; ++it) {
            const int i = it * 256 + tid;
            if (i < HROWS) halo[buf][i] = (half_t)hv[it];
        }
        __syncthreads();                                   // two halo buffers: one barrier per tile is enough
#pragma unroll
        for (int i = 0; i < GROUPS; ++i) {
            const int m = (wave * GROUPS + i) * 16 + r;    // this lane's voxel: the MFMA column
            const int vx = m & 7, vy = (m >> 3) & (TY - 1), vz = m >> (3 + YB);
            const int base = (vz * HHY + vy) * HHX + vx;
            half8 col;
#pragma unroll
            for (int j = 0; j < 8; ++j) col[j] = halo[buf][base + off[j]];
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            const f32x4 a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[0], col, zero, 0, 0, 0);
            const f32x4 a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[1], col, zero, 0, 0, 0);
            // lane (voxel, q) holds channels 4q..4q+3 of each 16-channel block; the two blocks exchange halves between the
            // 16-lane groups (v_permlane16_swap, as in the GEMM epilogue): group q then owns 8 consecutive channels
            unsigned pk[2][2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                half2_ h0, h1;
                h0[0] = (half_t)__builtin_amdgcn_fmed3f(a0[2 * e] + b0[2 * e], 0.f, 65504.f);
                h0[1] = (half_t)__builtin_amdgcn_fmed3f(a0[2 * e + 1] + b0[2 * e + 1], 0.f, 65504.f);
                h1[0] = (half_t)__builtin_amdgcn_fmed3f(a1[2 * e] + b1[2 * e], 0.f, 65504.f);
                h1[1] = (half_t)__builtin_amdgcn_fmed3f(a1[2 * e + 1] + b1[2 * e + 1], 0.f, 65504.f);
                pk[0][e] = __builtin_bit_cast(unsigned, h0);
                pk[1][e] = __builtin_bit_cast(unsigned, h1);
            }
            const auto s0 = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
            const auto s1 = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
            half_t* orow = out + ((((int64_t)b * D + z0 + vz) * H + y0 + vy) * W + x0 + vx) * 32;
            *(u32x4*)(orow + (q & 1) * 16 + (q >> 1) * 8) = o;
        }
    }
}

// last layer: fp16 NDHWC [..][CIN] -> fp32 [B][D][H][W], k3 s1 p1, Cout = 1, sigmoid.
// w fp32 [27][CIN], one thread per output voxel.
template <int CIN>
__global__ __launch_bounds__(256) void conv3d_last_kernel(const half_t* __restrict__ in, int B, int D, int H, int W,
                                                           const float* __restrict__ w, float bias,
                                                           float* __restrict__ out) {
    __shared__ float ws[27 * CIN];
    for (int i = threadIdx.x; i < 27 * CIN; i += blockDim.x) ws[i] = w[i];
    __syncthreads();
    const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vox >= (int64_t)B * D * H * W) return;
    const int xx = (int)(vox % W); int64_t t = vox / W;
    const int yy = (int)(t % H); t /= H;
    const int zz = (int)(t % D); const int bb = (int)(t / D);
    float a = bias;
    for (int kz = 0; kz < 3; ++kz)
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const int iz = zz + kz - 1, iy = yy + ky - 1, ix = xx + kx - 1;
                if ((unsigned)iz >= (unsigned)D || (unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
                const half8* src = (const half8*)(in + ((((int64_t)bb * D + iz) * H + iy) * W + ix) * CIN);
                const float* wk = ws + ((kz * 3 + ky) * 3 + kx) * CIN;
#pragma unroll
                for (int c8 = 0; c8 < CIN / 8; ++c8) {
                    const half8 v = src[c8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) a = fmaf(wk[c8 * 8 + e], (float)v[e], a);
                }
            }
    out[vox] = 1.f / (1.f + expf(-a));
}

// last layer with the halo in LDS: a workgroup owns 4 x 4 x 8 output voxels; thread = (voxel, half of the 27
// taps); the direct kernel above re-reads every input voxel 27 times from L2 (1.8 GB at B = 32).
// Requires D % 4 == H % 4 == W % 8 == 0.  Weights fp32 [27][32] are wave-uniform -> scalar loads.
__global__ __launch_bounds__(256) void conv3d_last_halo_kernel(const half_t* __restrict__ in, int B, int D, int H, int W,
                                                               const float* __restrict__ w, float bias,
                                                               float* __restrict__ out, int ntz, int nty, int ntx) {
    constexpr int CIN = 32, RB = CIN * 2, P = RB + 16, CPR = RB / 16;
    constexpr int HIT = (HROWS * CPR + 255) / 256;
    __shared__ __attribute__((aligned(16))) char smem[HROWS * P];
    __shared__ float part[128];
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % ntx; t /= ntx;
    const int ty = t % nty; t /= nty;
    const int tz = t % ntz; const int b = t / ntz;
    const int z0 = tz * HTZ, y0 = ty * HTY, x0 = tx * HTX;
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int c = it * 256 + tid;
        const int row = c / CPR, ch = c - row * CPR;
        const int hx = row % HHX; const int r2 = row / HHX;
        const int hy = r2 % HHY, hz = r2 / HHY;
        const int iz = z0 - 1 + hz, iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < HROWS) {
            if (ok) v = *(const half8*)(in + ((((int64_t)b * D + iz) * H + iy) * W + ix) * CIN + ch * 8);
            *(half8*)(smem + row * P + ch * 16) = v;
        }
    }
    __syncthreads();
    const int vox = tid & 127, half = __builtin_amdgcn_readfirstlane(tid >> 7);   // waves 0,1: taps 0-13; 2,3: 14-26
    const int x = vox & 7, y = (vox >> 3) & 3, z = vox >> 5;
    const char* base = smem + ((z * HHY + y) * HHX + x) * P;
    float a = 0.f;
    const int t0 = half * 14, t1 = half ? 27 : 14;
    for (int tap = t0; tap < t1; ++tap) {
        const int toff = ((tap / 9) * HHY + (tap / 3) % 3) * HHX + tap % 3;
        const float* wk = w + tap * CIN;                          // uniform address: s_load
#pragma unroll
        for (int c8 = 0; c8 < CIN / 8; ++c8) {
            const half8 v = *(const half8*)(base + toff * P + c8 * 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) a = fmaf(wk[c8 * 8 + e], (float)v[e], a);
        }
    }
    if (half) part[vox] = a;
    __syncthreads();
    if (!half) {
        a += part[vox] + bias;
        out[(((int64_t)b * D + z0 + z) * H + y0 + y) * W + x0 + x] = 1.f / (1.f + expf(-a));
    }
}

// The same layer with an 8 x 8 x 8 output block per workgroup (512 threads = 512 voxels, all 27 taps per thread).  The 4 x 4 x 8 form above
// fetches every input voxel 2.8 times (6 x 6 x 10 halo per 128 outputs: 188 MB of L2 -> LDS traffic at B = 32) and that, not its arithmetic,
// is what bounds it (a packed-fp16 dot-product form ran in the same 61 us: profiles/r04_j); here the halo is 10 x 10 x 10 per 512 outputs = 1.95 x.
template <int TZ>
__global__ __launch_bounds__(64 * TZ) void conv3d_last_halo8_kernel(const half_t* __restrict__ in, int B, int D, int H, int W,
                                                                    const float* __restrict__ w, float bias,
                                                                    float* __restrict__ out, int ntz, int nty, int ntx) {
    // rows padded to 80 bytes (conflict-free 16-byte reads of x-adjacent voxels).  Unpadded 64-byte rows with an XOR swizzle (64 KB per workgroup: two
    // per CU) measured the same (52.9 v. 51.8 us): the layer is VALU-bound now (864 v_fma_mix_f32 per voxel = ~48 us at B = 32), profiles/r04_j
    constexpr int CIN = 32, RB = CIN * 2, P = RB + 16, CPR = RB / 16, T = 8, HH = T + 2, ROWS = (TZ + 2) * HH * HH, NTH = 64 * TZ;
    constexpr int HIT = (ROWS * CPR + NTH - 1) / NTH;
    __shared__ __attribute__((aligned(16))) char smem[ROWS * P];
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % ntx; t /= ntx;
    const int ty = t % nty; t /= nty;
    const int tz = t % ntz; const int b = t / ntz;
    const int z0 = tz * TZ, y0 = ty * T, x0 = tx * T;
    half8 hv[HIT];
#pragma unroll
    for (int it = 0; it < HIT; ++it) {                           // every load of the halo in flight before the first LDS store
        const int c = it * NTH + tid;
        const int row = c / CPR, ch = c - row * CPR;
        const int hx = row % HH; const int r2 = row / HH;
        const int hy = r2 % HH, hz = r2 / HH;
        const int iz = z0 - 1 + hz, iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = row < ROWS && (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        hv[it] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        if (ok) hv[it] = *(const half8*)(in + ((((int64_t)b * D + iz) * H + iy) * W + ix) * CIN + ch * 8);
    }
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int c = it * NTH + tid;
        const int row = c / CPR, ch = c - row * CPR;
        if (row < ROWS) *(half8*)(smem + row * P + ch * 16) = hv[it];
    }
    __syncthreads();
    const int x = tid & 7, y = (tid >> 3) & 7, z = tid >> 6;
    const int r0 = (z * HH + y) * HH + x;
    float a = bias;
#pragma unroll 3
    for (int tap = 0; tap < 27; ++tap) {
        const int row = r0 + ((tap / 9) * HH + (tap / 3) % 3) * HH + tap % 3;
        const float* wk = w + tap * CIN;                          // uniform address: s_load
#pragma unroll
        for (int c8 = 0; c8 < CIN / 8; ++c8) {
            const half8 v = *(const half8*)(smem + row * P + c8 * 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) a = fmaf(wk[c8 * 8 + e], (float)v[e], a);
        }
    }
    out[(((int64_t)b * D + z0 + z) * H + y0 + y) * W + x0 + x] = 1.f / (1.f + expf(-a));
}

// fp32 weights [27][32] -> the MFMA A operand of every tap for conv3d_last_mfma8_kernel: [27][64 lanes][8 halfs]
__global__ __launch_bounds__(64) void conv3d_last_pack_kernel(const float* __restrict__ w, half_t* __restrict__ wfrag) {
    const int tap = blockIdx.x, lane = threadIdx.x, m = lane & 15, kq = lane >> 4;
    half8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float wf = w[tap * 32 + kq * 8 + e];
        const half_t hi = (half_t)wf;
        const half_t lo = (half_t)(wf - (float)hi);
        const half_t lo2 = (half_t)((wf - (float)hi) - (float)lo);
        v[e] = m == 0 ? hi : (m == 1 ? lo : (m == 2 ? lo2 : (half_t)0.f));
    }
    *(half8*)(wfrag + (tap * 64 + lane) * 8) = v;
}

// The same 8 x 8 x 8 block with the 864 multiply-adds per voxel on the MATRIX pipe (round 5).  The layer has ONE output channel, so as a product it is
// D[3][voxel] = Wt[3][K = 27 x 32] . X[K][voxel] with the three rows = the fp16 head of the fp32 weights and two successive fp16 rounding residuals (hi + lo + lo2: the
// fp32 weights to their last bit, fp32 accumulation; the other 13 rows of the 16 x 16 x 32 MFMA are zeros -- wasted, and still 4 x faster than 864 v_fma_mix per voxel:
// 108 MFMAs of 16 cycles per wave and 64 voxels against ~3500 VALU cycles).  A k step is one tap: the B operand of voxel n is its 32 input channels at the tap's
// halo row (the same 16-byte LDS reads as the VALU form); the A operand of tap t is 1 KB of a fragment-order copy of the weights (pcd_conv3d_last_pack, made once).
// Lanes 0-15 hold rows 0-2 (the three partial sums) of their voxel: out = sigmoid(hi + (lo + lo2) + bias).
__global__ __launch_bounds__(512, 4) void conv3d_last_mfma8_kernel(const half_t* __restrict__ in, int B, int D, int H, int W, const half_t* __restrict__ wfrag,
                                                                   float bias, float* __restrict__ out, int ntz, int nty, int ntx) {
    constexpr int CIN = 32, RB = CIN * 2, P = RB + 16, CPR = RB / 16, T = 8, TZ = 8, HH = T + 2, ROWS = (TZ + 2) * HH * HH, NTH = 64 * TZ;
    constexpr int HIT = (ROWS * CPR + NTH - 1) / NTH;
    __shared__ __attribute__((aligned(16))) char smem[ROWS * P];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    int t = blockIdx.x;
    const int tx = t % ntx; t /= ntx;
    const int ty = t % nty; t /= nty;
    const int tz = t % ntz; const int b = t / ntz;
    const int z0 = tz * TZ, y0 = ty * T, x0 = tx * T;
    {
        half8 hv[HIT];
#pragma unroll
        for (int it = 0; it < HIT; ++it) {                       // every load of the halo in flight before the first LDS store
            const int c = it * NTH + tid;
            const int row = c / CPR, ch = c - row * CPR;
            const int hx = row % HH; const int r2 = row / HH;
            const int hy = r2 % HH, hz = r2 / HH;
            const int iz = z0 - 1 + hz, iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            const bool ok = row < ROWS && (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
            hv[it] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (ok) hv[it] = *(const half8*)(in + ((((int64_t)b * D + iz) * H + iy) * W + ix) * CIN + ch * 8);
        }
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int c = it * NTH + tid;
            const int row = c / CPR, ch = c - row * CPR;
            if (row < ROWS) *(half8*)(smem + row * P + ch * 16) = hv[it];
        }
    }
    // A operand of tap t: wfrag[t][lane][8] (conv3d_last_pack_kernel: lane (m = lane & 15, k = 8 (lane >> 4) .. + 7), rows 0-2 = hi / lo / lo2, rows 3-15 zero),
    // one coalesced 1-KB load per tap and wave from 27 KB that every workgroup reads (L1 / L2 resident)
    const int m = lane & 15, kq = lane >> 4;
    const half_t* wl = wfrag + lane * 8;
    __syncthreads();
    const int z = tid >> 6;                                       // the wave's z slice: 64 voxels = four groups of 16 (two x rows of 8 each)
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 3
    for (int tap = 0; tap < 27; ++tap) {
        const int toff = ((tap / 9) * HH + (tap / 3) % 3) * HH + tap % 3;
        const half8 wa = *(const half8*)(wl + tap * 512);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int v = g * 16 + m, x = v & 7, y = v >> 3;
            const half8 xb = *(const half8*)(smem + ((z * HH + y) * HH + x + toff) * P + kq * 16);
            acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, xb, acc[g], 0, 0, 0);
        }
    }
    if (kq == 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int v = g * 16 + m, x = v & 7, y = v >> 3;
            const float a = (acc[g][0] + (acc[g][1] + acc[g][2])) + bias;
            out[(((int64_t)b * D + z0 + z) * H + y0 + y) * W + x0 + x] = 1.f / (1.f + expf(-a));
        }
    }
}

// The same layer as PER-TAP PARTIAL PRODUCTS (round 5, default).  The form above reads one 1-KB B fragment from LDS per MFMA: 108 KB per wave and 64 voxels, the LDS
// port is busy 3.2 us per workgroup of a 2048-workgroup grid (26 us) and the layer took 51-56 us for 0.9 GFLOP.  Here a wave owns one 8 x 8 output slice and turns the
// product inside out: for each of the three input slices above it (dz = -1, 0, +1) it forms, for every voxel u of that slice's 10 x 10 halo,
//       p[u][t] = sum_c w[dz][t][c] x[u][c]        for the nine taps t = 3 dy + dx of that dz
// as D[tap][voxel] = W[tap][K = 32 c] . X[c][voxel] on v_mfma_f32_16x16x32_f16 -- the A operand holds nine tap rows (the fp32 weights as hi + lo + lo2 fp16 parts,
// three MFMAs into one accumulator), the B operand 16 voxels x 32 channels straight from global memory (64 contiguous bytes per voxel: no input staging) -- writes
// the 16 x 9 partials to a WAVE-PRIVATE 5-KB LDS tile and gathers out[y][x] += p[(y + dy, x + dx)][3 dy + dx]: nine 4-byte reads per dz and lane, a fixed
// summation order.  21 B-fragment loads (all in flight), 63 MFMAs, 27 + 21 LDS operations per wave; no workgroup barrier (LDS operations of one wave execute in order).
// Each input slice is read by the three waves around it: L1 / L2 absorb that.  d a multiple of 4, h and w of 8.
template <int TZ, int ABL = 0>  // TZ: output slices = waves per workgroup (4: three workgroups per CU at this kernel's 131 registers); ABL (tools/bench_last_layer.py,
                                // outputs wrong): 1 = loads only (their sum instead of products and gathers), 2 = no loads
__global__ __launch_bounds__(64 * TZ, 4) void conv3d_last_taps_kernel(const half_t* __restrict__ in, int B, int D, int H, int W, const half_t* __restrict__ wfrag, float bias,
                                                               float* __restrict__ out, int ntz, int nty, int ntx) {
    constexpr int CIN = 32, HH = 10, NV = HH * HH, NG = (NV + 15) / 16, PITCH = 12;
    __shared__ __attribute__((aligned(16))) float psm[TZ][NG * 16][PITCH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int t = blockIdx.x;
    const int tx = t % ntx; t /= ntx;
    const int ty = t % nty; t /= nty;
    const int tz = t % ntz; const int b = t / ntz;
    const int z0 = tz * TZ, y0 = ty * 8, x0 = tx * 8;
    const int n = lane & 15, q = lane >> 4;
    // A operands: row m = n is tap 3 dy + dx of slice dz (rows 9 .. 15 zero), k = 8 q .. 8 q + 7; three fp16 parts of the fp32 weight
    // (from pcd_conv3d_last_pack's copy [27 taps][64 lanes][8]: there lane part + 16 q of tap t holds part `part` of w[t][8 q .. 8 q + 7]); one slice's set at a time
    half8 wa[3];
    auto load_w = [&](int dz) __attribute__((always_inline)) {
#pragma unroll
        for (int part = 0; part < 3; ++part) {
            wa[part] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (n < 9) wa[part] = *(const half8*)(wfrag + ((dz * 9 + n) * 64 + part + 16 * q) * 8);
        }
    };
    load_w(0);
    float (*pw)[PITCH] = psm[wave];
    const int oy = lane >> 3, ox = lane & 7;
    float o = bias;
    // the B fragments of the first two input slices are requested before the first is used; the third slice's take the first slice's registers behind its MFMAs
    // (56 + 12 weight registers: four waves per SIMD).  A lane's in-plane offsets and bounds are the same for the three slices: formed once; the loads are raw
    // buffer loads over the slice (a lane outside the grid carries an offset past its end and receives zeros: no branch, no per-load address arithmetic).
    half8 xb[3][NG];
    unsigned voff[NG];                                               // byte offset inside a slice, or past the end of every slice: the buffer load returns zeros there
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int v = g * 16 + n, hy = v / HH, hx = v - hy * HH;
        const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = !(ABL & 2) && v < NV && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        voff[g] = ok ? (unsigned)(((iy * W + ix) * CIN + 8 * q) * 2) : 0xffffffffu;
    }
    auto request = [&](int dz) __attribute__((always_inline)) {
        const int iz = z0 + wave - 1 + dz;
        const bool zok = (unsigned)iz < (unsigned)D;                 // wave-uniform: a slice outside the grid is a buffer of zero bytes
        const half_t* slice = in + ((int64_t)b * D + (zok ? iz : 0)) * H * W * CIN;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)slice, 0, zok ? H * W * CIN * 2 : 0, 0x00020000);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
            const u32x4_ r = __builtin_amdgcn_raw_buffer_load_b128(rs, voff[g], 0, 0);
            xb[dz][g] = __builtin_bit_cast(half8, r);
        }
    };
    request(0);
    request(1);
    if constexpr ((ABL & 1) != 0) request(2);
    if constexpr ((ABL & 1) != 0) {
#pragma unroll
        for (int dz = 0; dz < 3; ++dz)
#pragma unroll
            for (int g = 0; g < NG; ++g) o += (float)xb[dz][g][0] + (float)xb[dz][g][7];
        out[(((int64_t)b * D + z0 + wave) * H + y0 + oy) * W + x0 + ox] = o;
        return;
    }
#pragma unroll
    for (int dz = 0; dz < 3; ++dz) {
        f32x4 accs[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[2], xb[dz][g], acc, 0, 0, 0);      // smallest part first
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[1], xb[dz][g], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[0], xb[dz][g], acc, 0, 0, 0);
            accs[g] = acc;
        }
        // lane (voxel n, q) holds taps 4 q .. 4 q + 3 of voxel g * 16 + n (taps 9 .. 11 are zero rows of the A operand; taps 12 .. 15 have no place in the tile)
        if (q < 3) {
#pragma unroll
            for (int g = 0; g < NG; ++g) *(f32x4*)&pw[g * 16 + n][4 * q] = accs[g];
        }
        if (dz < 2) {
            __builtin_amdgcn_sched_barrier(0);                       // (not earlier: the compiler would hoist these loads to the top and need 50 more registers)
            load_w(dz + 1);
            if (dz == 0) request(2);
            __builtin_amdgcn_sched_barrier(0);
        }
        // Lanes exchange data through the tile: to the language that is communication between threads and needs synchronisation, or the compiler may (and did)
        // keep a lane's reads in front of stores the lane itself does not execute.  Within one wave the hardware needs nothing (its LDS operations execute in
        // order): wavefront-scope fences + a wave barrier emit no instruction and pin the order.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) o += pw[(oy + dy) * HH + ox + dx][3 * dy + dx];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // the next slice's stores stay behind these reads
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    out[(((int64_t)b * D + z0 + wave) * H + y0 + oy) * W + x0 + ox] = 1.f / (1.f + expf(-o));
}

// The same per-tap partial products with every input slice read ONCE: a wave owns TZ consecutive output slices of one 8 x 8 tile and walks the TZ + 2 input
// slices around them; for a slice it forms ALL 27 taps' partials (two MFMA row groups: taps 0-15 and 16-26, three weight parts each: six MFMAs per 16 voxels),
// writes them to its LDS tile ([112 voxels][28 taps]) and every output slice the slice touches (z = s + 1 - dz) gathers its nine.  The kernel above issues ~650
// instructions per output slice (it is bound by instruction issue); here the loads, their offsets and the prologue are shared by TZ slices: ~300 per slice at TZ = 4
// (22.7 us against 32; TZ = 2: 26.6, TZ = 8: 24.4 -- 2048 waves do not fill the chip).
// The next slice's B fragments are requested before the current slice's MFMAs.  Summation order per output: input slice ascending, then (dy, dx): deterministic.
template <int TZ>
__global__ __launch_bounds__(256, 2) void conv3d_last_roll_kernel(const half_t* __restrict__ in, int B, int D, int H, int W, const half_t* __restrict__ wfrag, float bias,
                                                                  float* __restrict__ out, int ntz, int nty, int ntx, int nwork) {
    constexpr int CIN = 32, HH = 10, NV = HH * HH, NG = (NV + 15) / 16, PITCH = 28;
    __shared__ __attribute__((aligned(16))) float psm[4][NG * 16][PITCH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int t = blockIdx.x * 4 + wave;                                   // one (sample, z chunk, y tile, x tile) per wave; no workgroup-level synchronisation below
    if (t >= nwork) return;
    const int tx = t % ntx; t /= ntx;
    const int ty = t % nty; t /= nty;
    const int tz = t % ntz; const int b = t / ntz;
    const int z0 = tz * TZ, y0 = ty * 8, x0 = tx * 8;
    const int n = lane & 15, q = lane >> 4;
    // A operands: row group rg, row m = n is tap 16 rg + n (taps 27 .. 31: zero rows), k = 8 q ..; from pcd_conv3d_last_pack's copy (lane part + 16 q of tap t)
    half8 wa[2][3];
#pragma unroll
    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int part = 0; part < 3; ++part) {
            wa[rg][part] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (16 * rg + n < 27) wa[rg][part] = *(const half8*)(wfrag + ((16 * rg + n) * 64 + part + 16 * q) * 8);
        }
    unsigned voff[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int v = g * 16 + n, hy = v / HH, hx = v - hy * HH;
        const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = v < NV && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        voff[g] = ok ? (unsigned)(((iy * W + ix) * CIN + 8 * q) * 2) : 0xffffffffu;
    }
    half8 xb[2][NG];
    auto request = [&](int s, half8 (&dst)[NG]) __attribute__((always_inline)) {      // input slice z0 - 1 + s
        const int iz = z0 - 1 + s;
        const bool zok = (unsigned)iz < (unsigned)D;                 // wave-uniform: a slice outside the grid is a buffer of zero bytes
        const half_t* slice = in + ((int64_t)b * D + (zok ? iz : 0)) * H * W * CIN;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)slice, 0, zok ? H * W * CIN * 2 : 0, 0x00020000);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
            dst[g] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[g], 0, 0));
        }
    };
    float (*pw)[PITCH] = psm[wave];
    const int oy = lane >> 3, ox = lane & 7;
    float o[TZ];
#pragma unroll
    for (int z = 0; z < TZ; ++z) o[z] = bias;
    request(0, xb[0]);
#pragma unroll
    for (int s = 0; s < TZ + 2; ++s) {
        if (s + 1 < TZ + 2) request(s + 1, xb[(s + 1) & 1]);
        // lane (voxel n, q) holds taps 16 rg + 4 q .. + 3 of voxel g * 16 + n; taps 28 .. 31 (rg 1, q 3) have no place in the tile
        f32x4 acc1[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[0][2], xb[s & 1][g], acc, 0, 0, 0);      // smallest part first
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[0][1], xb[s & 1][g], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[0][0], xb[s & 1][g], acc, 0, 0, 0);
            *(f32x4*)&pw[g * 16 + n][4 * q] = acc;
            acc = (f32x4){0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[1][2], xb[s & 1][g], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[1][1], xb[s & 1][g], acc, 0, 0, 0);
            acc1[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[1][0], xb[s & 1][g], acc, 0, 0, 0);
        }
        if (q < 3) {
#pragma unroll
            for (int g = 0; g < NG; ++g) *(f32x4*)&pw[g * 16 + n][16 + 4 * q] = acc1[g];
        }
        // lanes exchange data through the tile: wavefront-scope fences + a wave barrier pin the order for the compiler (conv3d_last_taps_kernel)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int dz = 0; dz < 3; ++dz) {
            const int z = s - dz;                                    // output slice z0 + z reads input slice z0 - 1 + s with its taps of dz
            if (z >= 0 && z < TZ) {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) o[z] += pw[(oy + dy) * HH + ox + dx][9 * dz + 3 * dy + dx];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // the next slice's stores stay behind these reads
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
#pragma unroll
    for (int z = 0; z < TZ; ++z) out[(((int64_t)b * D + z0 + z) * H + y0 + oy) * W + x0 + ox] = 1.f / (1.f + expf(-o[z]));
}

// VAE3D's last layer (networks.py:2018-2019): ConvTranspose3d(CIN, 1, k3, s2, p1, output_padding 1) + Sigmoid.
// o = 2 i - 1 + k per dimension: even o takes (k=1, i=o/2); odd o takes (k=0, i=(o+1)/2) and (k=2, i=(o-1)/2).
// in fp16 NDHWC [B][D][H][W][CIN]; w fp32 [27][CIN] (tap-major); out fp32 [B][2D][2H][2W].
template <int CIN>
__global__ __launch_bounds__(256) void convT3d_last_kernel(const half_t* __restrict__ in, int B, int D, int H, int W,
                                                            const float* __restrict__ w, float bias,
                                                            float* __restrict__ out) {
    __shared__ float ws[27 * CIN];
    for (int i = threadIdx.x; i < 27 * CIN; i += blockDim.x) ws[i] = w[i];
    __syncthreads();
    const int OD = 2 * D, OH = 2 * H, OW = 2 * W;
    const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vox >= (int64_t)B * OD * OH * OW) return;
    const int ox = (int)(vox % OW); int64_t t = vox / OW;
    const int oy = (int)(t % OH); t /= OH;
    const int oz = (int)(t % OD); const int bb = (int)(t / OD);
    float a = bias;
    for (int kz = (oz & 1) ? 0 : 1; kz < 3; kz += 2) {
        const int iz = (oz + 1 - kz) >> 1;
        if ((unsigned)iz >= (unsigned)D) continue;
        for (int ky = (oy & 1) ? 0 : 1; ky < 3; ky += 2) {
            const int iy = (oy + 1 - ky) >> 1;
            if ((unsigned)iy >= (unsigned)H) continue;
            for (int kx = (ox & 1) ? 0 : 1; kx < 3; kx += 2) {
                const int ix = (ox + 1 - kx) >> 1;
                if ((unsigned)ix >= (unsigned)W) continue;
                const half8* src = (const half8*)(in + ((((int64_t)bb * D + iz) * H + iy) * W + ix) * CIN);
                const float* wk = ws + ((kz * 3 + ky) * 3 + kx) * CIN;
#pragma unroll
                for (int c8 = 0; c8 < CIN / 8; ++c8) {
                    const half8 v = src[c8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) a = fmaf(wk[c8 * 8 + e], (float)v[e], a);
                }
            }
        }
    }
    out[vox] = 1.f / (1.f + expf(-a));
}

// ---- the first layer: which kernel (read top down; a tiled row also needs its tile count to fit 32 bits)
//   cout  stride  first8  dims                         form
//   32    1       1       d, h, w % 8 == 0             Mfma8   (conv3d_first32_mfma_kernel<8, 8>, 512-voxel tiles)
//   32    1       any     d % 4, h % 4, w % 8 == 0     Mfma4   (conv3d_first32_mfma_kernel<4, 4>, 128-voxel tiles)
//   32    any     any     any                          First32 (conv3d_first32_kernel)
//   else                                               Generic (conv3d_first_kernel, weights in dynamic LDS)
enum class FirstForm { Mfma8, Mfma4, First32, Generic };
static FirstForm first_form(int d, int h, int w, int stride, int cout, int64_t ovox_total, const Conv3dConfig& cfg) {
    if (cout != 32) return FirstForm::Generic;
    if (stride == 1 && cfg.first8 && d % 8 == 0 && h % 8 == 0 && w % 8 == 0 && ovox_total / 512 <= 0x7fffffff) return FirstForm::Mfma8;
    if (stride == 1 && d % HTZ == 0 && h % HTY == 0 && w % HTX == 0 && ovox_total / 128 <= 0x7fffffff) return FirstForm::Mfma4;
    return FirstForm::First32;
}

// ---- the last layer: which kernel (read top down; a tiled row also needs its workgroup-unit count, total / 256, / 512 or / 128, to fit 32 bits).
// "packed" = a pcd_conv3d_last_pack copy was passed; /8 = d, h, w % 8 == 0; /488 = d % 4, h % 8, w % 8 == 0; /448 = d % 4, h % 4, w % 8 == 0
//   packed  last8  last_roll  dims    form
//   yes     3      1          /488    Roll    (conv3d_last_roll_kernel<4>)
//   yes     3      0          /488    Taps    (conv3d_last_taps_kernel<4, last_abl>)
//   yes     2      any        /8      Mfma8   (conv3d_last_mfma8_kernel)
//   any     1-3    any        /8      Halo8   (conv3d_last_halo8_kernel<8>, fp32 weights)
//   any     any    any        /448    Halo4   (conv3d_last_halo_kernel)
//   any     any    any        any     Direct  (conv3d_last_kernel<32>)
enum class LastForm { Roll, Taps, Mfma8, Halo8, Halo4, Direct };
static LastForm last_form(int d, int h, int w, int64_t total, bool packed, const Conv3dConfig& cfg) {
    const bool by8 = d % 8 == 0 && h % 8 == 0 && w % 8 == 0 && total / 512 <= 0x7fffffff;
    if (packed && cfg.last8 == 3 && d % 4 == 0 && h % 8 == 0 && w % 8 == 0 && total / 256 <= 0x7fffffff)
        return cfg.last_roll ? LastForm::Roll : LastForm::Taps;
    if (packed && cfg.last8 == 2 && by8) return LastForm::Mfma8;
    if (cfg.last8 != 0 && by8) return LastForm::Halo8;
    if (d % HTZ == 0 && h % HTY == 0 && w % HTX == 0 && total / 128 <= 0x7fffffff) return LastForm::Halo4;
    return LastForm::Direct;
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_conv3d_first(const float* x, int batch, int d, int h, int w, int stride, const float* wgt,
                                const float* bias, int cout, void* out, void* stream) {
    PCD_CHECK_ARG(x && wgt && bias && out && batch > 0 && d > 0 && h > 0 && w > 0 && cout > 0 && cout % 8 == 0);
    PCD_CHECK_ARG(stride == 1 || stride == 2);
    const int64_t total = (int64_t)batch * ((d - 1) / stride + 1) * ((h - 1) / stride + 1) * ((w - 1) / stride + 1);   // output voxels
    hipStream_t s = (hipStream_t)stream;
    half_t* o = (half_t*)out;
    const auto tgrid = [](int64_t tiles) { return dim3((unsigned)(tiles < 2048 ? tiles : 2048)); };   // the tiled forms: persistent over at most 2048 workgroups
    switch (first_form(d, h, w, stride, cout, total, g_conv3d)) {
    case FirstForm::Mfma8:
        hipLaunchKernelGGL((conv3d_first32_mfma_kernel<8, 8>), tgrid(total / 512), dim3(256), 0, s, x, batch, d, h, w, wgt, bias, o, d / 8, h / 8, w / 8, (int)(total / 512));
        break;
    case FirstForm::Mfma4:
        hipLaunchKernelGGL((conv3d_first32_mfma_kernel<4, 4>), tgrid(total / 128), dim3(256), 0, s, x, batch, d, h, w, wgt, bias, o, d / HTZ, h / HTY, w / HTX, (int)(total / 128));
        break;
    case FirstForm::First32:
        hipLaunchKernelGGL(conv3d_first32_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x, batch, d, h, w, stride, wgt, bias, o);
        break;
    case FirstForm::Generic:
        hipLaunchKernelGGL(conv3d_first_kernel, dim3((unsigned)ceil_div(total * (cout / 8), 256)), dim3(256), (size_t)cout * 28 * sizeof(float), s,
                           x, batch, d, h, w, stride, wgt, bias, cout, o);
        break;
    }
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_conv3d_last_packed_bytes(void) { return (size_t)27 * 64 * 8 * sizeof(half_t); }

extern "C" int pcd_conv3d_last_pack(const float* wgt, void* wfrag, void* stream) {
    PCD_CHECK_ARG(wgt && wfrag);
    hipLaunchKernelGGL(conv3d_last_pack_kernel, dim3(27), dim3(64), 0, (hipStream_t)stream, wgt, (half_t*)wfrag);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

// Conv3d(32 -> 1, k3, p1) + sigmoid; wfrag = pcd_conv3d_last_pack's copy of the weights for the matrix-pipe forms, or null (the forms that read the fp32 weights)
extern "C" int pcd_conv3d_last_sigmoid_packed(const void* in, int batch, int d, int h, int w, int cin, const float* wgt, const void* wfrag, float bias, float* out,
                                              void* stream) {
    PCD_CHECK_ARG(in && wgt && out && batch > 0 && d > 0 && h > 0 && w > 0 && cin == 32);
    const int64_t total = (int64_t)batch * d * h * w;
    hipStream_t s = (hipStream_t)stream;
    const half_t* x = (const half_t*)in;
    const half_t* wf = (const half_t*)wfrag;
    switch (last_form(d, h, w, total, wfrag != nullptr, g_conv3d)) {
    case LastForm::Roll:       // total / 256 (sample, 4 output slices, 8 x 8 tile) units, one per wave
        hipLaunchKernelGGL(conv3d_last_roll_kernel<4>, dim3((unsigned)ceil_div(total / 256, 4)), dim3(256), 0, s, x, batch, d, h, w, wf, bias, out, d / 4, h / 8, w / 8, (int)(total / 256));
        break;
    case LastForm::Taps:
        dispatch_int<0, 1, 2>(g_conv3d.last_abl, [&](auto abl) {
            hipLaunchKernelGGL((conv3d_last_taps_kernel<4, decltype(abl)::value>), dim3((unsigned)(total / 256)), dim3(256), 0, s, x, batch, d, h, w, wf, bias, out, d / 4, h / 8, w / 8);
        });
        break;
    case LastForm::Mfma8:
        hipLaunchKernelGGL(conv3d_last_mfma8_kernel, dim3((unsigned)(total / 512)), dim3(512), 0, s, x, batch, d, h, w, wf, bias, out, d / 8, h / 8, w / 8);
        break;
    case LastForm::Halo8:
        hipLaunchKernelGGL(conv3d_last_halo8_kernel<8>, dim3((unsigned)(total / 512)), dim3(512), 0, s, x, batch, d, h, w, wgt, bias, out, d / 8, h / 8, w / 8);
        break;
    case LastForm::Halo4:
        hipLaunchKernelGGL(conv3d_last_halo_kernel, dim3((unsigned)(total / 128)), dim3(256), 0, s, x, batch, d, h, w, wgt, bias, out, d / HTZ, h / HTY, w / HTX);
        break;
    case LastForm::Direct:
        hipLaunchKernelGGL((conv3d_last_kernel<32>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, x, batch, d, h, w, wgt, bias, out);
        break;
    }
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_conv3d_last_sigmoid(const void* in, int batch, int d, int h, int w, int cin, const float* wgt, float bias, float* out, void* stream) {
    return pcd_conv3d_last_sigmoid_packed(in, batch, d, h, w, cin, wgt, nullptr, bias, out, stream);
}

extern "C" int pcd_convt3d_last_sigmoid(const void* in, int batch, int d, int h, int w, int cin, const float* wgt,
                                        float bias, float* out, void* stream) {
    PCD_CHECK_ARG(in && wgt && out && batch > 0 && d > 0 && h > 0 && w > 0);
    PCD_CHECK_ARG(cin == 32);
    const int64_t total = (int64_t)batch * d * h * w * 8;
    hipLaunchKernelGGL((convT3d_last_kernel<32>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const half_t*)in, batch, d, h, w, wgt, bias, out);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
