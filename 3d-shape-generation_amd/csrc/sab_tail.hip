// The tail of SetAttentionBlock.forward (reference networks.py:78-83) behind the attention kernel, for C = 128 and C = 64, as ONE launch:
//     x1 = x + out_proj(a) ;  y = x1 + W2 relu(W1 LN2(x1) + b1) + b2          (a = the heads' outputs, x = the block's input)
// As four launches (out_proj GEMM + residual, LayerNorm, W1 GEMM + ReLU, W2 GEMM + residual) the tail costs 145 / 70 us per block at
// B = 64, N = 2048 for 39 / 9.7 GFLOP: K = 64 .. 512 GEMMs are latency / HBM bound, and the 4C-wide hidden tensor (134 / 67 MB) is written and
// read back.  Here a wave owns 32 points for the whole tail and nothing leaves its REGISTERS between the layers (the scheme of
// pw_wide_chain_kernel, csrc/widechain.hip):
//   * every product is transposed, D[channel][point] = W[channel][k] . act[point][k] on v_mfma_f32_32x32x16_f16 (weights = A operand,
//     activations = B operand); an accumulator group holds 4 consecutive channels of one point, and one v_permlane32_swap per register turns two
//     groups of the two lane halves into the 8 consecutive k of the next product's B fragment;
//   * x1 stays in fp32 in the accumulators: the residual x is added there, the LayerNorm statistics of a point are a per-lane sum over its
//     C / 2 channels + one exchange with lane ^ 32 (two passes: mean, then squared deviations), and the same registers then take
//     b2 and are the C operand of the W2 products -- y accumulates onto x1;
//   * the FFN streams over its 4C hidden channels in chunks of 64: h = relu(W1[chunk] . LN + b1) (two accumulator tiles) -> fp16 B fragments
//     -> y += W2[:, chunk] . h.  The hidden tensor never exists;
//   * only the weights move: packed once per block (pcd_sab_tail_pack) into stage images in fragment order -- [W_out] and, per chunk,
//     [W1 chunk | W2 chunk] -- they arrive by LDS-DMA in a three-stage ring shared by the workgroup's eight waves (256 points), one barrier
//     per stage, 262 FLOP per byte of LDS fill.
// sab_head_kernel below does the block's first half in the same form (LN1 + in_proj).  Rows must be a multiple of 256 (otherwise the caller keeps the
// separate launches).  Arithmetic: fp16 operands, fp32 accumulation; x1 and the
// LayerNorm in fp32 (the four-launch form rounds x1 and LN2(x1) to fp16 in between: this form is the closer one to the reference's fp32).
// Host side: the block's packed buffer is st_layout below; stage_images.h has the packer (stage_pack) and the launch (ring_launch).
#include "common.h"
#include "stage_images.h"

namespace pcd {

constexpr int ST_WAVES = 8, ST_THREADS = 64 * ST_WAVES, ST_TILE = 32 * ST_WAVES, ST_RING = 3;

template <int C>
struct StCfg {
    static constexpr int NT = C / 32;                  // 32-channel tiles of a C-wide output
    static constexpr int KS = C / 16;                  // 16-deep k steps of a C-wide input
    static constexpr int NCH = C / 16;                 // 64-wide chunks of the 4C hidden channels
    static constexpr int STAGE = C == 128 ? 32768 : 16384;      // bytes: [W1 chunk: 2 tiles x KS pieces | W2 chunk: NT tiles x 4 pieces] of 1 KB
    static constexpr int NSTG = 1 + NCH;               // stage images per tile of points: W_out, then the chunks
    static constexpr int PPW = STAGE / 1024 / ST_WAVES;         // LDS-DMA pieces per wave and stage
    static constexpr int W2OFF = 2 * KS * 1024;        // the W2 part of a chunk image
    // fp32 parameters behind the images: b_out [C] | ln2 gamma [C] | ln2 beta [C] | b_ff2 [C] | b_ff1 [4C]
    static constexpr int BO = 0, GA = C, BE = 2 * C, B2 = 3 * C, B1 = 4 * C, NPAR = 8 * C;
    // the head (LN1 + in_proj, sab_head_kernel) behind the tail's image: three stage images of W_in (one C-wide output pass each), then b_in [3C] | ln1 gamma [C] |
    // ln1 beta [C]
    static constexpr int HSTAGE = NT * KS * 1024;      // one pass of W_in: C x C fp16
    static constexpr int HPPW = HSTAGE / 1024 / ST_WAVES;
    static constexpr int HB = 0, HGA = 3 * C, HBE = 4 * C, HNPAR = 5 * C;
    static_assert(C == 64 || C == 128, "the tail kernel is built for C = 64 and C = 128");
    static_assert((2 * KS + 4 * NT) * 1024 == STAGE && NT * KS * 1024 <= STAGE, "stage image layout");
};

struct SabTailParams {
    const half_t* a;          // [M][C] attention output (heads concatenated)
    const half_t* x;          // [M][C] the block's input (residual)
    const char* packed;       // NSTG stage images, then NPAR floats
    half_t* y;                // [M][C]
    int64_t m;
    // the attention U-Net's additive per-level time embeddings (networks.py:669-698) inside the launch: x is read as fp16(x + pre_e[shape]) (the block
    // runs on x + emb), y leaves as fp16(y + post_e[shape]) (the skip tensor is block(x) + emb); each exactly as pcd_add_shape_bias_strided_f16 rounds it
    const float* pre_e; const float* post_e; int64_t estride; int rps;
    int split;                // 1: one wave per SIMD requests a stage's LDS-DMA pieces (pcd_sab_tail_config bit 1)
};

template <int C>
__global__ __launch_bounds__(ST_THREADS, 2) void sab_tail_kernel(SabTailParams p) {
    using K = StCfg<C>;
    constexpr int NT = K::NT, KS = K::KS;
    extern __shared__ __attribute__((aligned(16))) char st_smem[];          // [ST_RING][STAGE] | parameters
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pnt = lane & 31, hh = lane >> 5;
    float* par = (float*)(st_smem + ST_RING * K::STAGE);
    {
        const float* src = (const float*)(p.packed + (size_t)K::NSTG * K::STAGE);
        for (int i = threadIdx.x; i < K::NPAR; i += ST_THREADS) par[i] = src[i];
    }
    const int64_t ntiles = p.m / ST_TILE;
    const int my_tiles = (int)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
    const int total_stages = my_tiles * K::NSTG;
    // stage n of this workgroup's run = image n % NSTG (StageRing, device_prims.h; the request form is chosen at run time)
    const bool split = p.split != 0;
    int n = 0;                                                 // next stage to consume
    const StageRing<K::STAGE, K::PPW, ST_RING> ring{p.packed, st_smem, total_stages, wave, lane, K::NSTG, split};
    ring.issue(0);
    ring.issue(1);
    // (a closure over n: with ring.acquire(n) at the sites themselves the kernels' register numbering changes, profiles/device_prims_isa.md)
    auto acquire = [&]() __attribute__((always_inline)) -> const char* { return ring.acquire(n); };
    for (int ti = 0; ti < my_tiles; ++ti) {
        const int64_t tile = blockIdx.x + (int64_t)ti * gridDim.x;
        const int64_t pt = tile * ST_TILE + wave * 32 + pnt;
        // B fragments of a: lane (point, half) takes the 8 channels 16 s + 8 half of every k step; the residual in accumulator layout
        half8 bf[KS];
        {
            const half_t* row = p.a + pt * C + 8 * hh;
#pragma unroll
            for (int s = 0; s < KS; ++s) bf[s] = *(const half8*)(row + 16 * s);
        }
        half4 xr[NT][4];
        {
            const half_t* row = p.x + pt * C + 4 * hh;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) xr[t][g] = *(const half4*)(row + 32 * t + 8 * g);
        }
        if (p.pre_e != nullptr) {
            const float* er = p.pre_e + (pt / p.rps) * p.estride + 4 * hh;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 ev = *(const f32x4*)(er + 32 * t + 8 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) xr[t][g][e] = to_half_sat((float)xr[t][g][e] + ev[e]);
                }
        }
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
        // ---- out_proj
        {
            const char* img = acquire();
#pragma unroll
            for (int q = 0; q < KS; ++q) {
                half8 af[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) af[t] = *(const half8*)(img + (t * KS + q) * 1024);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t], bf[q], acc[t], 0, 0, 0);
            }
            ++n;
        }
        // ---- x1 = x + out_proj(a) + b_out (fp32), its LayerNorm statistics over the point's C channels (this lane's C / 2 + lane ^ 32's)
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bo = *(const f32x4*)&par[K::BO + 32 * t + 8 * g + 4 * hh];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[t][4 * g + e] += bo[e] + (float)xr[t][g][e];
                    sum += acc[t][4 * g + e];
                }
            }
        sum += __shfl_xor(sum, 32);
        const float mean = sum * (1.f / C);
        float ssq = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) { const float dv = acc[t][e] - mean; ssq += dv * dv; }
        ssq += __shfl_xor(ssq, 32);
        const float rstd = rsqrtf(ssq * (1.f / C) + 1e-5f);
        // ---- LN2(x1) -> B fragments (k step 2 t + gp), from the fp32 accumulators (PCD_LN_FRAGMENTS normalises fp16 B fragments); then the accumulators take b_ff2 and go on as y
        half8 lnf[KS];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float v[2][4];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int g = 2 * gp + u;
                    const f32x4 ga = *(const f32x4*)&par[K::GA + 32 * t + 8 * g + 4 * hh];
                    const f32x4 be = *(const f32x4*)&par[K::BE + 32 * t + 8 * g + 4 * hh];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[u][e] = __builtin_amdgcn_fmed3f((acc[t][4 * g + e] - mean) * rstd * ga[e] + be[e], -65504.f, 65504.f);
                }
                lnf[2 * t + gp] = regroup_swap(v[0], v[1]);
            }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 b2 = *(const f32x4*)&par[K::B2 + 32 * t + 8 * g + 4 * hh];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t][4 * g + e] += b2[e];
            }
        // ---- the FFN, 64 hidden channels at a time
#pragma unroll 1
        for (int ch = 0; ch < K::NCH; ++ch) {
            const char* img = acquire();
            f32x16 h[2];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 16; ++e) h[u][e] = 0.f;
#pragma unroll
            for (int q = 0; q < KS; ++q) {
                half8 af[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) af[u] = *(const half8*)(img + (u * KS + q) * 1024);
#pragma unroll
                for (int u = 0; u < 2; ++u) h[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[u], lnf[q], h[u], 0, 0, 0);
            }
            half8 hf[4];
            const float* b1 = par + K::B1 + 64 * ch + 4 * hh;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    float v[2][4];
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        const int g = 2 * gp + w;
                        const f32x4 bb = *(const f32x4*)&b1[32 * u + 8 * g];
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[w][e] = __builtin_amdgcn_fmed3f(h[u][4 * g + e] + bb[e], 0.f, 65504.f);
                    }
                    hf[2 * u + gp] = regroup_swap(v[0], v[1]);
                }
            const char* img2 = img + K::W2OFF;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                half8 af[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) af[t] = *(const half8*)(img2 + (t * 4 + q) * 1024);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t], hf[q], acc[t], 0, 0, 0);
            }
            ++n;
        }
        // ---- y rows leave as 16-byte pieces (8 consecutive channels per lane)
        half_t* orow = p.y + pt * C + 8 * hh;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float v[2][4];
#pragma unroll
                for (int w = 0; w < 2; ++w)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[w][e] = __builtin_amdgcn_fmed3f(acc[t][4 * (2 * gp + w) + e], -65504.f, 65504.f);
                if (p.post_e != nullptr) {
                    const float* er = p.post_e + (pt / p.rps) * p.estride + 32 * t + 4 * hh;
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        const f32x4 ev = *(const f32x4*)(er + 8 * (2 * gp + w));
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[w][e] = __builtin_amdgcn_fmed3f((float)(half_t)v[w][e] + ev[e], -65504.f, 65504.f);
                    }
                }
                *(half8*)(orow + 32 * t + 16 * gp) = regroup_swap(v[0], v[1]);
            }
    }
}

// The head of the block for C <= 128: qkv = in_proj(LN1(x)) (reference networks.py:81) in one launch of the same form -- the B fragments of x are normalised
// as they are loaded (statistics by v_dot2_f32_f16 over the lane's C / 2 channels + lane ^ 32, fp32; result fp16 like pcd_layernorm_f16's), then three
// C-wide output passes over them, one stage image of W_in each, bias, no activation, 16-byte stores into the [rows][3C] qkv tensor.
struct SabHeadParams {
    const half_t* x;          // [M][C] the block's input
    const char* packed;       // the head part of the block's image: 3 stage images, then HNPAR floats
    half_t* qkv;              // [M][3C]
    int64_t m;
    const float* pre_e; int64_t estride; int rps;      // x is read as fp16(x + pre_e[shape]) (see SabTailParams)
    int split;                // as SabTailParams
};

template <int C>
__global__ __launch_bounds__(ST_THREADS, 2) void sab_head_kernel(SabHeadParams p) {
    using K = StCfg<C>;
    constexpr int NT = K::NT, KS = K::KS;
    extern __shared__ __attribute__((aligned(16))) char st_smem[];          // [ST_RING][HSTAGE] | parameters
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pnt = lane & 31, hh = lane >> 5;
    float* par = (float*)(st_smem + ST_RING * K::HSTAGE);
    {
        const float* src = (const float*)(p.packed + (size_t)3 * K::HSTAGE);
        for (int i = threadIdx.x; i < K::HNPAR; i += ST_THREADS) par[i] = src[i];
    }
    const int64_t ntiles = p.m / ST_TILE;
    const int my_tiles = (int)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
    const int total_stages = my_tiles * 3;
    const bool split = p.split != 0;
    int n = 0;
    const StageRing<K::HSTAGE, K::HPPW, ST_RING> ring{p.packed, st_smem, total_stages, wave, lane, 3, split};
    ring.issue(0);
    ring.issue(1);
    __syncthreads();                                           // the LayerNorm affine is read before the first stage barrier
    auto acquire = [&]() __attribute__((always_inline)) -> const char* { return ring.acquire(n); };
    for (int ti = 0; ti < my_tiles; ++ti) {
        const int64_t tile = blockIdx.x + (int64_t)ti * gridDim.x;
        const int64_t pt = tile * ST_TILE + wave * 32 + pnt;
        half8 bf[KS];
        {
            const half_t* row = p.x + pt * C + 8 * hh;
#pragma unroll
            for (int s = 0; s < KS; ++s) bf[s] = *(const half8*)(row + 16 * s);
        }
        if (p.pre_e != nullptr) {
            const float* er = p.pre_e + (pt / p.rps) * p.estride + 8 * hh;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const f32x4 e0 = *(const f32x4*)(er + 16 * s), e1 = *(const f32x4*)(er + 16 * s + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bf[s][e] = to_half_sat((float)bf[s][e] + e0[e]);
                    bf[s][4 + e] = to_half_sat((float)bf[s][4 + e] + e1[e]);
                }
            }
        }
        PCD_LN_FRAGMENTS(bf, C, par, K::HGA, par, K::HBE, hh);
        half_t* orow = p.qkv + pt * (3 * C) + 8 * hh;
#pragma unroll 1
        for (int pass = 0; pass < 3; ++pass) {
            const char* img = acquire();
            f32x16 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
#pragma unroll
            for (int q = 0; q < KS; ++q) {
                half8 af[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) af[t] = *(const half8*)(img + (t * KS + q) * 1024);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t], bf[q], acc[t], 0, 0, 0);
            }
            ++n;
            const float* bb = par + K::HB + pass * C + 4 * hh;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    float v[2][4];
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        const int g = 2 * gp + w;
                        const f32x4 b4 = *(const f32x4*)&bb[32 * t + 8 * g];
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[w][e] = __builtin_amdgcn_fmed3f(acc[t][4 * g + e] + b4[e], -65504.f, 65504.f);
                    }
                    *(half8*)(orow + pass * C + 32 * t + 16 * gp) = regroup_swap(v[0], v[1]);
                }
        }
    }
}

static int g_sab_split = 1;     // pcd_sab_tail_config + 2 switches it off: one wave per SIMD requests a stage's LDS-DMA pieces
static int g_sab_tail = 1;      // pcd_sab_tail_config: 0 = pcd_sab_forward keeps the four launches even where the descriptor carries a packed tail

// The block's buffer = the tail's part, then the head's; each is images | parameters, in the order StCfg gives the kernels.  Weights and parameters by index:
enum { ST_W_OUT, ST_W_FF1, ST_W_FF2, ST_W_IN };
enum { ST_B_OUT, ST_LN2_G, ST_LN2_B, ST_B_FF2, ST_B_FF1, ST_B_IN, ST_LN1_G, ST_LN1_B };
constexpr StageLayout st_layout(int C, bool head) {
    const int nt = C / 32, ks = C / 16;
    StageLayout L{};
    if (head) {                                                // W_in as three C-wide passes | b_in [3C] | ln1 gamma | ln1 beta
        for (int i = 0; i < 3; ++i) sl_frag(L, ST_W_IN, C, i * C, 3 * C, 0, nt, ks);
        sl_row(L, ST_B_IN, 0, 3 * C, 3 * C);
        for (int i = ST_LN1_G; i <= ST_LN1_B; ++i) sl_row(L, i, 0, C, C);
        return L;
    }
    sl_frag(L, ST_W_OUT, C, 0, C, 0, nt, ks);
    L.bytes = L.par = (2 * ks + 4 * nt) * 1024;                // a whole stage image: at C = 64 W_out fills half of it, the rest stays zero
    for (int ch = 0; ch < C / 16; ++ch) {                      // per 64-wide chunk of the hidden channels [W1 chunk | W2 chunk]
        sl_frag(L, ST_W_FF1, C, 64 * ch, 4 * C, 0, 2, ks);
        sl_frag(L, ST_W_FF2, 4 * C, 0, C, 64 * ch, nt, 4);
    }
    for (int i = ST_B_OUT; i <= ST_B_FF2; ++i) sl_row(L, i, 0, C, C);
    sl_row(L, ST_B_FF1, 0, 4 * C, 4 * C);
    return L;
}
template <int C>
constexpr bool st_layout_ok() {
    using K = StCfg<C>;
    constexpr StageLayout T = st_layout(C, false), H = st_layout(C, true);
    return T.par == (size_t)K::NSTG * K::STAGE && T.bytes - T.par == K::NPAR * sizeof(float) && T.block[1].off == (size_t)K::STAGE &&
           T.block[2].off == (size_t)K::STAGE + K::W2OFF && T.row[0].off == K::BO && T.row[1].off == K::GA && T.row[2].off == K::BE &&
           T.row[3].off == K::B2 && T.row[4].off == K::B1 && H.par == (size_t)3 * K::HSTAGE && H.bytes - H.par == K::HNPAR * sizeof(float) &&
           H.row[0].off == K::HB && H.row[1].off == K::HGA && H.row[2].off == K::HBE;
}
static_assert(st_layout_ok<64>() && st_layout_ok<128>(), "StCfg (what the kernels read) and the packed layout disagree");

template <int C>
static int head_launch(const void* packed, const void* x, int64_t m, void* qkv, const float* pre_e, int64_t estride, int rps, hipStream_t s) {
    constexpr StageLayout T = st_layout(C, false), H = st_layout(C, true);
    SabHeadParams p{};
    p.x = (const half_t*)x; p.packed = (const char*)packed + T.bytes; p.qkv = (half_t*)qkv; p.m = m;
    p.pre_e = pre_e; p.estride = estride; p.rps = rps > 0 ? rps : 1;
    p.split = g_sab_split;
    PCD_CHECK_HIP((ring_launch<sab_head_kernel<C>, sab_head_kernel<C>>(m / ST_TILE, C == 64 ? RING_CAP_HEAD64 : RING_CAP_CU, ST_THREADS,
                                                                      ST_RING * StCfg<C>::HSTAGE + H.bytes - H.par, false, s, p)));
    return PCD_OK;
}

template <int C>
static int tail_launch(const void* packed, const void* a, const void* x, int64_t m, void* y, const float* pre_e, const float* post_e, int64_t estride, int rps,
                       hipStream_t s) {
    constexpr StageLayout T = st_layout(C, false);
    SabTailParams p{};
    p.a = (const half_t*)a; p.x = (const half_t*)x; p.packed = (const char*)packed; p.y = (half_t*)y; p.m = m;
    p.pre_e = pre_e; p.post_e = post_e; p.estride = estride; p.rps = rps > 0 ? rps : 1;
    p.split = g_sab_split;
    PCD_CHECK_HIP((ring_launch<sab_tail_kernel<C>, sab_tail_kernel<C>>(m / ST_TILE, C == 64 ? RING_CAP_TAIL64 : RING_CAP_CU, ST_THREADS,
                                                                      ST_RING * StCfg<C>::STAGE + T.bytes - T.par, false, s, p)));
    return PCD_OK;
}

}  // namespace pcd

using namespace pcd;

extern "C" size_t pcd_sab_tail_packed_bytes(int dim) {
    return (dim == 64 || dim == 128) ? st_layout(dim, false).bytes + st_layout(dim, true).bytes : 0;
}

extern "C" int pcd_sab_tail_supported(int dim, int64_t rows) {
    return (dim == 64 || dim == 128) && rows > 0 && rows % ST_TILE == 0 && rows * dim <= 0x7fffffff ? 1 : 0;
}

extern "C" int pcd_sab_tail_config(int fused) {
    PCD_CHECK_ARG(fused >= 0 && fused <= 3);
    g_sab_tail = fused & 1;
    g_sab_split = (fused & 2) ? 0 : 1;
    return PCD_OK;
}

extern "C" int pcd_sab_tail_enabled(void) { return g_sab_tail; }

extern "C" int pcd_sab_tail_pack(const pcd_sab_desc_t* d, void* packed, void* stream) {
    PCD_CHECK_ARG(d && packed && (d->dim == 64 || d->dim == 128));
    PCD_CHECK_ARG(d->w_out && d->b_out && d->ln2_g && d->ln2_b && d->w_ff1 && d->b_ff1 && d->w_ff2 && d->b_ff2);
    PCD_CHECK_ARG(d->w_in && d->b_in && d->ln1_g && d->ln1_b);
    const void* const weights[] = {d->w_out, d->w_ff1, d->w_ff2, d->w_in};                                     // ST_W_*
    const float* const params[] = {d->b_out, d->ln2_g, d->ln2_b, d->b_ff2, d->b_ff1, d->b_in, d->ln1_g, d->ln1_b};     // ST_B_OUT ..
    const StageLayout tail = st_layout(d->dim, false);
    int rc = stage_pack(tail, weights, params, packed, (hipStream_t)stream);
    if (rc == PCD_OK) rc = stage_pack(st_layout(d->dim, true), weights, params, (char*)packed + tail.bytes, (hipStream_t)stream);
    return rc;
}

extern "C" int pcd_sab_tail_bias_f16(int dim, const void* packed, const void* a, const void* x, int64_t rows, int rows_per_shape, const float* pre_e,
                                     const float* post_e, int64_t e_stride, void* y, void* stream) {
    PCD_CHECK_ARG(packed && a && x && y && y != a && y != x);
    PCD_CHECK_ARG(pcd_sab_tail_supported(dim, rows));
    PCD_CHECK_ARG((pre_e == nullptr && post_e == nullptr) || (rows_per_shape > 0 && e_stride >= 0 && e_stride % 4 == 0));
    PCD_CHECK_ARG((((uintptr_t)pre_e | (uintptr_t)post_e) & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    return dim == 128 ? tail_launch<128>(packed, a, x, rows, y, pre_e, post_e, e_stride, rows_per_shape, s)
                      : tail_launch<64>(packed, a, x, rows, y, pre_e, post_e, e_stride, rows_per_shape, s);
}

extern "C" int pcd_sab_tail_f16(int dim, const void* packed, const void* a, const void* x, int64_t rows, void* y, void* stream) {
    return pcd_sab_tail_bias_f16(dim, packed, a, x, rows, 0, nullptr, nullptr, 0, y, stream);
}

extern "C" int pcd_sab_head_bias_f16(int dim, const void* packed, const void* x, int64_t rows, int rows_per_shape, const float* pre_e, int64_t e_stride,
                                     void* qkv, void* stream) {
    PCD_CHECK_ARG(packed && x && qkv && qkv != x);
    PCD_CHECK_ARG(pcd_sab_tail_supported(dim, rows));
    PCD_CHECK_ARG(pre_e == nullptr || (rows_per_shape > 0 && e_stride >= 0 && e_stride % 4 == 0 && ((uintptr_t)pre_e & 15) == 0));
    hipStream_t s = (hipStream_t)stream;
    return dim == 128 ? head_launch<128>(packed, x, rows, qkv, pre_e, e_stride, rows_per_shape, s)
                      : head_launch<64>(packed, x, rows, qkv, pre_e, e_stride, rows_per_shape, s);
}

extern "C" int pcd_sab_head_f16(int dim, const void* packed, const void* x, int64_t rows, void* qkv, void* stream) {
    return pcd_sab_head_bias_f16(dim, packed, x, rows, 0, nullptr, 0, qkv, stream);
}
