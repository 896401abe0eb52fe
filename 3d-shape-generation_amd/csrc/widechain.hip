// Chains of 256-channel pointwise layers of UNetPointNetLarge (reference networks.py:16-49, 779-818) as one launch each:
//   E3: x2 [M][256] -> enc3.conv1 256->256 -> conv2 256->256 -> conv3 256->512 -> x3
//   D2: [dec3 out [M][256] | x2 [M][256]] -> dec2.conv1 512->256 -> conv2 256->256 -> conv3 256->128
// As separate GEMMs these layers are HBM / latency bound (K = 256: four K tiles per output tile; 33-57 us per layer against a
// 22 us traffic floor) and write + re-read a 67 MB intermediate each.  Here a wave owns 32 points for the whole chain and the
// activations never leave its REGISTERS between layers:
//   * every layer is the transposed product D[channel][point] = W[channel][k] . act[point][k] on v_mfma_f32_32x32x16_f16 (weights
//     = A operand, activations = B operand); the B fragments of all 16 k-steps of a 256-wide input are 64 registers per lane;
//   * an accumulator group holds 4 consecutive channels of one point; after bias + ReLU + fp16 rounding, one v_permlane32_swap per
//     register turns two such groups of the two lane halves into the 8 consecutive k of the NEXT layer's B fragment: no LDS, no
//     barrier, no memory traffic between layers;
//   * only the weights stream: packed once into 32-KB stage images ([8 channel tiles][4 k-steps][64 lanes][16 B] = 256 channels x
//     64 k in fragment order), they arrive by LDS-DMA into a 3-deep ring, one barrier per 64-deep K tile for the 8 waves
//     (256 points) of a workgroup; a 256 x 256 tile of work per 32 KB of LDS fill = 256 FLOP per filled byte, twice the GEMM's.
// Output rows leave as 16-byte pieces (8 consecutive channels per lane after the same swap).  M must be a multiple of 256.
// Further down, the same engine with a shape per segment takes the narrow layers next to these chains along (pw_wide_ends_kernel: E23, D21).
// Host side: each packed buffer is one StageLayout (wc_layout, wl_layout, we_layout); stage_images.h has the packer (stage_pack) and the launch (ring_launch).
#include "common.h"
#include "stage_images.h"

namespace pcd {

constexpr int WC_WAVES = 8, WC_THREADS = 64 * WC_WAVES, WC_TILE = 32 * WC_WAVES;
constexpr int WC_STAGE = 32768, WC_RING = 3;
constexpr int WC_MAXSEG = 8;

// one 256-channel output pass: 4 K tiles of the current B fragments (accumulating onto the previous segment when `cont`)
struct WcSeg {
    int src;          // 0: the registers hold the previous layer's output; 1 / 2: load the B fragments from in1 / in2
    int cont;         // 1: keep accumulating (second K half of a two-source layer), 0: start from zero
    int finish;       // 0: more K to come; 1: epilogue -> next layer's fragments (registers); 2: epilogue -> global at channel offset `coff`
    int coff;         // finish 2: first output channel of this pass
    int cvalid;       // finish 2: channels of this pass that exist (256, or 128 for a padded last layer)
    int bias_off;     // offset into the bias array
    int keep_b;       // 1: the B fragments are needed by the next segment too (second output pass of a 512-channel layer)
    int linear;       // 1: no ReLU in this pass's epilogue (a plain Linear: attention in_proj); 0: bias + ReLU
};

struct WcParams {
    const half_t* in1; const half_t* in2;     // [M][256]
    const char* wpacked;                       // stage images, segment after segment, 4 per segment
    const float* bias;                         // fp32, indexed by bias_off + channel
    const float* ln;                           // optional LayerNorm over the 256 input channels of in1 (gamma [256] | beta [256], eps 1e-5) applied to the B
                                               // fragments as they are loaded: LN + Linear(256, 256 P) [+ ReLU] in one launch (pcd_pw_wide_ln_linear)
    half_t* out; int ldo;                      // [M][ldo]
    int64_t m;
    int nseg;
    WcSeg seg[WC_MAXSEG];
};

// LN = false: the chains of UNetPointNetLarge; LN = true: LayerNorm + Linear (pcd_pw_wide_ln_linear) -- its own instantiation so that the chains keep their
// register allocation (246 registers, no spill)
// SPLIT: the request form of the weight-image ring (StageRing, device_prims.h)
template <bool LN, bool SPLIT>
__global__ __launch_bounds__(WC_THREADS, 2) void pw_wide_chain_kernel(WcParams p) {
    extern __shared__ __attribute__((aligned(16))) char wc_smem[];          // [WC_RING][WC_STAGE] | bias copy
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pnt = lane & 31, hh = lane >> 5;
    float* bias_lds = (float*)(wc_smem + WC_RING * WC_STAGE);
    const int nbias = p.nseg * 256;
    for (int i = threadIdx.x; i < nbias; i += WC_THREADS) bias_lds[i] = p.bias[i];
    float* ln_lds = bias_lds + WC_MAXSEG * 256;                // (present when p.ln: the host sizes the allocation)
    if constexpr (LN)
        for (int i = threadIdx.x; i < 512; i += WC_THREADS) ln_lds[i] = p.ln[i];
    const int64_t ntiles = p.m / WC_TILE;
    const int my_tiles = (int)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
    const int nstage_seq = p.nseg * 4;                         // stages per tile of points
    const int total_stages = my_tiles * nstage_seq;
    // stage n of this workgroup's run = image (n % nstage_seq)
    const StageRing<WC_STAGE, 4, WC_RING> ring{p.wpacked, wc_smem, total_stages, wave, lane, nstage_seq, SPLIT};
    ring.issue(0);
    ring.issue(1);
    if constexpr (LN) __syncthreads();                         // ln_lds is read before the first stage barrier
    int n = 0;                                                 // next stage to consume
    for (int ti = 0; ti < my_tiles; ++ti) {
        const int64_t tile = blockIdx.x + (int64_t)ti * gridDim.x;
        const int64_t pt = tile * WC_TILE + wave * 32 + pnt;
        half8 bf[16];
        f32x16 acc[8];
#pragma unroll 1
        for (int sg = 0; sg < p.nseg; ++sg) {
            const WcSeg S = p.seg[sg];
            if (S.src != 0) {
                // B fragments straight from the [point][256] rows: lane (point, half) takes the 8 channels 16 s + 8 half of every k-step
                const half_t* row = (S.src == 1 ? p.in1 : p.in2) + pt * 256 + 8 * hh;
#pragma unroll
                for (int s = 0; s < 16; ++s) bf[s] = *(const half8*)(row + 16 * s);
                // LayerNorm of the point's 256 channels.  (The first barrier below orders these reads of ln_lds behind its fill; at the first tile of a
                // workgroup the fill is ordered by the __syncthreads() in front of the tile loop.)
                if constexpr (LN) PCD_LN_FRAGMENTS(bf, 256, ln_lds, 0, ln_lds, 256, hh);
            }
            if (!S.cont) {
#pragma unroll
                for (int t = 0; t < 8; ++t)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
            }
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const char* img = ring.acquire(n);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    half8 af[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t) af[t] = *(const half8*)(img + (t * 4 + q) * 1024);
#pragma unroll
                    for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t], bf[4 * kt + q], acc[t], 0, 0, 0);
                }
                ++n;
            }
            if (S.finish == 0) continue;
            const float* bseg = bias_lds + S.bias_off;
            const float lo = LN && S.linear ? -65504.f : 0.f;
            if (S.finish == 1) {
                // -> the next layer's B fragments: k-step s = 2 t + gp of the new input
#pragma unroll
                for (int t = 0; t < 8; ++t)
#pragma unroll
                    for (int gp = 0; gp < 2; ++gp) bf[2 * t + gp] = regroup_bias_clamp(acc[t], gp, bseg + 32 * t, hh, lo);
            } else {
                half_t* orow = p.out + pt * p.ldo + S.coff + 8 * hh;
#pragma unroll
                for (int t = 0; t < 8; ++t)
#pragma unroll
                    for (int gp = 0; gp < 2; ++gp) {
                        const half8 v = regroup_bias_clamp(acc[t], gp, bseg + 32 * t, hh, lo);
                        if (32 * t + 16 * gp < S.cvalid) *(half8*)(orow + 32 * t + 16 * gp) = v;
                    }
            }
        }
    }
}

// the LN + Linear launches' dynamic LDS: the ring, then ln_lds where the kernel puts it (behind the bias rows of WC_MAXSEG passes)
constexpr size_t WC_LDS_MAX = (size_t)WC_RING * WC_STAGE + (size_t)(WC_MAXSEG * 256 + 512) * sizeof(float);

// E3 / D2: w[0..2] / b[0..2] as four 256-channel passes of four images (256 channels x 64 k each), then one bias row of 256 floats per pass
constexpr StageLayout wc_layout(int chain) {
    // per pass: layer, ldw, first channel, channel limit, first k, channels with a bias (0: the pass has no epilogue)
    constexpr int pass[2][4][6] = {{{0, 256, 0, 256, 0, 256}, {1, 256, 0, 256, 0, 256}, {2, 256, 0, 512, 0, 256}, {2, 256, 256, 512, 0, 256}},
                                   {{0, 512, 0, 256, 0, 0}, {0, 512, 0, 256, 256, 256}, {1, 256, 0, 256, 0, 256}, {2, 256, 0, 128, 0, 128}}};
    StageLayout L{};
    for (const auto& p : pass[chain]) sl_frag(L, p[0], p[1], p[2], p[3], p[4], 8, 4, 4);
    for (const auto& p : pass[chain]) sl_row(L, p[0], p[2], p[5], 256);
    return L;
}
constexpr StageLayout WC_LAYOUT[2] = {wc_layout(0), wc_layout(1)};

// LN + Linear: w [256 P][256] as P passes | b [256 P] | gamma [256] | beta [256]
constexpr StageLayout wl_layout(int passes) {
    StageLayout L{};
    for (int i = 0; i < passes; ++i) sl_frag(L, 0, 256, 256 * i, 256 * passes, 0, 8, 4, 4);
    sl_row(L, 0, 0, 256 * passes, 256 * passes);
    for (int i = 1; i < 3; ++i) sl_row(L, i, 0, 256, 256);
    return L;
}
constexpr StageLayout WL_LAYOUT[4] = {wl_layout(1), wl_layout(2), wl_layout(3), wl_layout(4)};

// ------------------------------------------------------------------------------------------------ the narrow ends: enc2 + enc3 and dec2 + dec1.conv1
// The same engine with a shape per segment: K in {128, 256} input channels (K / 16 B fragments) x C in {128, 256} output channels (C / 32 accumulator
// tiles).  A stage image is always 32 pieces of 1 KiB = [C / 32 channel tiles][NQ k-steps], NQ = 1024 / C: 256 channels x 64 k or 128 channels x 128 k,
// so a stage is 32 MFMAs at any shape.  A chain's segment list is a compile-time constant and its segments are unrolled: every register-array index is a
// constant, and a 128-wide segment leaves the registers it does not use free (profiles/wide_chain_ends.md has what a run-time table cost).
//   E23: x1 [M][128] -> enc2.conv1 -> conv2 -> conv3 (x2 [M][256] stored AND kept as fragments) -> enc3.conv1 -> conv2 -> conv3 -> x3 [M][512]
//   D21: [dec3 out [M][256] | x2 [M][256]] -> dec2.conv1 -> conv2 -> conv3 -> dec1.conv1 on [registers 128 | x1 [M][128]] -> [M][128]
// A hi / lo layer is two segments on the same accumulators and the same B fragments: all hi K passes, then all lo passes (the order of pcd_gemm_f16_hilo).
constexpr int WE_MAXSEG = 8;
enum { WE_K128_C128 = 0, WE_K128_C256 = 1, WE_K256_C128 = 2, WE_K256_C256 = 3 };

struct WeSeg {
    int kind;         // WE_K*_C*: 1, 2, 2, 4 stage images
    int src;          // 0: the registers hold the input; 1 / 2: all K channels from in1 / in2 ([M][K]); 3: the first 128 stay in registers, the second 128 from in3 ([M][128])
    int cont;         // 1: keep accumulating (second source of a two-source layer, lo pass of a hi / lo layer)
    int finish;       // 0: more K to come; 1: epilogue -> next layer's fragments; 2: -> out at channel offset `coff`; 3: -> next layer's fragments and out2
    int coff;
    int bias_off;
};

// A chain as its segments in execution order: one description for the kernel (a constant there: the segments are unrolled, so that a register no segment of
// the moment needs is free), for the packer (which weights each segment's images hold) and for the launcher
struct WeSegSrc { int layer; int ldw; int c0; int k0; };      // index into w[] / b[]; row stride of w; first output channel and first k of the segment
struct WePlan {
    int nseg, nstage, nbias, nlayer;
    WeSeg seg[WE_MAXSEG];
    WeSegSrc from[WE_MAXSEG];
    int layer_c[6], layer_bias[6];                             // channels and bias offset of every layer
};
constexpr int we_kind_images(int kind) { return kind == WE_K128_C128 ? 1 : (kind == WE_K256_C256 ? 4 : 2); }
constexpr void we_add(WePlan& P, int kind, int src, int cont, int finish, int coff, int layer, int ldw, int c0, int k0) {
    P.seg[P.nseg] = WeSeg{kind, src, cont, finish, coff, P.layer_bias[layer] + c0};
    P.from[P.nseg] = WeSegSrc{layer, ldw, c0, k0};
    P.nstage += we_kind_images(kind);
    ++P.nseg;
}
constexpr WePlan we_plan(int chain, int hilo) {
    WePlan P{};
    if (chain == 0) {
        const int c[6] = {128, 128, 256, 256, 256, 512};
        P.nlayer = 6;
        for (int i = 0; i < 6; ++i) { P.layer_c[i] = c[i]; P.layer_bias[i] = P.nbias; P.nbias += c[i]; }
        we_add(P, WE_K128_C128, 1, 0, 1, 0, 0, 128, 0, 0);                             // enc2.conv1
        we_add(P, WE_K128_C128, 0, 0, 1, 0, 1, 128, 0, 0);                             // enc2.conv2
        if (hilo) {                                                                    // enc2.conv3 -> x2 (stored, and on into enc3)
            we_add(P, WE_K128_C256, 0, 0, 0, 0, 2, 256, 0, 0);
            we_add(P, WE_K128_C256, 0, 1, 3, 0, 2, 256, 0, 128);
        } else {
            we_add(P, WE_K128_C256, 0, 0, 3, 0, 2, 128, 0, 0);
        }
        we_add(P, WE_K256_C256, 0, 0, 1, 0, 3, 256, 0, 0);                             // enc3.conv1
        we_add(P, WE_K256_C256, 0, 0, 1, 0, 4, 256, 0, 0);                             // enc3.conv2
        we_add(P, WE_K256_C256, 0, 0, 2, 0, 5, 256, 0, 0);                             // enc3.conv3, channels 0 .. 255
        we_add(P, WE_K256_C256, 0, 0, 2, 256, 5, 256, 256, 0);                         //             channels 256 .. 511 (same B fragments)
    } else {
        const int c[4] = {256, 256, 128, 128};
        P.nlayer = 4;
        for (int i = 0; i < 4; ++i) { P.layer_c[i] = c[i]; P.layer_bias[i] = P.nbias; P.nbias += c[i]; }
        we_add(P, WE_K256_C256, 1, 0, 0, 0, 0, 512, 0, 0);                             // dec2.conv1, dec3's half
        we_add(P, WE_K256_C256, 2, 1, 1, 0, 0, 512, 0, 256);                           //             x2's half
        we_add(P, WE_K256_C256, 0, 0, 1, 0, 1, 256, 0, 0);                             // dec2.conv2
        we_add(P, WE_K256_C128, 0, 0, 1, 0, 2, 256, 0, 0);                             // dec2.conv3
        if (hilo) {                                                                    // dec1.conv1 on [registers | x1]
            we_add(P, WE_K256_C128, 3, 0, 0, 0, 3, 512, 0, 0);
            we_add(P, WE_K256_C128, 0, 1, 2, 0, 3, 512, 0, 256);
        } else {
            we_add(P, WE_K256_C128, 3, 0, 2, 0, 3, 256, 0, 0);
        }
    }
    return P;
}

struct WeParams {
    const half_t* in1; const half_t* in2; const half_t* in3;
    const char* wpacked;                       // stage images in execution order
    const float* bias;                         // fp32, indexed by bias_off + channel
    half_t* out;                               // E23: x3 [M][512], D21: [M][128]
    half_t* out2;                              // E23: x2 [M][256]
    int64_t m;
};

// segment SG of the chain, then the ones behind it
template <int CHAIN, bool HILO, int SG, typename Ring>
__device__ __forceinline__ void we_segments(const WeParams& p, const Ring& ring, int& n, int64_t row0, int lrow, int hh, const float* bias_lds, half8 (&bf)[16],
                                            f32x16 (&acc)[8]) {
    constexpr WePlan P = we_plan(CHAIN, HILO);
    if constexpr (SG < P.nseg) {
        constexpr WeSeg S = P.seg[SG];
        constexpr int K = (S.kind == WE_K128_C128 || S.kind == WE_K128_C256) ? 128 : 256, C = (S.kind == WE_K128_C128 || S.kind == WE_K256_C128) ? 128 : 256;
        constexpr int NT = C / 32, NQ = 32 / NT, NS = K / (16 * NQ);       // channel tiles; k-steps per stage; stages
        // row addresses as a wave-uniform tile base (scalar registers) + a 32-bit lane offset: 64-bit lane addresses of three matrices carried through
        // the chain do not fit next to 64 + 128 + 32 registers of fragments and accumulators
        auto at = [&row0, &lrow, &hh](auto* base, int ld, int col) { return base + row0 * ld + (unsigned)(lrow * ld + col + 8 * hh); };
        if constexpr (S.src == 1 || S.src == 2) {
            const half_t* row = at(S.src == 1 ? p.in1 : p.in2, K, 0);
#pragma unroll
            for (int s = 0; s < K / 16; ++s) bf[s] = *(const half8*)(row + 16 * s);
        }
        if constexpr (S.src == 3) {
            const half_t* row = at(p.in3, 128, 0);
#pragma unroll
            for (int s = 0; s < 8; ++s) bf[8 + s] = *(const half8*)(row + 16 * s);
        }
        if constexpr (!S.cont) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
        }
#pragma unroll
        for (int ks = 0; ks < NS; ++ks) {
            // (the stage counter kept opaque: with the segments unrolled, n % period is a constant per stage, and the compiler then keeps every stage's
            // per-lane request address live over the whole tile loop -- in scratch)
            asm volatile("" : "+s"(n));
            const char* img = ring.acquire(n);
#pragma unroll
            for (int f0 = 0; f0 < 32; f0 += 8) {                                       // fragment f of the stage: k-step f / NT, channel tile f % NT
                half8 af[8];
#pragma unroll
                for (int f = f0; f < f0 + 8; ++f) af[f - f0] = *(const half8*)(img + ((f % NT) * NQ + f / NT) * 1024);
#pragma unroll
                for (int f = f0; f < f0 + 8; ++f)
                    acc[f % NT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[f - f0], bf[NQ * ks + f / NT], acc[f % NT], 0, 0, 0);
            }
            ++n;
        }
        // (opaque for the same reason: one base register per epilogue and small immediate offsets, as with a run-time segment table, not a hoisted
        // register per 32-channel tile of every layer)
        int boff = S.bias_off;
        asm volatile("" : "+s"(boff));
        const float* bseg = bias_lds + boff;
        if constexpr (S.finish == 1) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) bf[2 * t + gp] = regroup_bias_clamp(acc[t], gp, bseg + 32 * t, hh, 0.f);
        } else if constexpr (S.finish == 2) {
            half_t* orow = at(p.out, CHAIN == 0 ? 512 : 128, S.coff);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) *(half8*)(orow + 32 * t + 16 * gp) = regroup_bias_clamp(acc[t], gp, bseg + 32 * t, hh, 0.f);
        } else if constexpr (S.finish == 3) {
            half_t* orow = at(p.out2, 256, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    bf[2 * t + gp] = regroup_bias_clamp(acc[t], gp, bseg + 32 * t, hh, 0.f);
                    *(half8*)(orow + 32 * t + 16 * gp) = bf[2 * t + gp];
                }
        }
        we_segments<CHAIN, HILO, SG + 1>(p, ring, n, row0, lrow, hh, bias_lds, bf, acc);
    }
}

// CHAIN 0: E23, 1: D21; HILO: the chain's narrow layer has hi | lo weights; SPLIT: the request form of the ring, as above
template <int CHAIN, bool HILO, bool SPLIT>
__global__ __launch_bounds__(WC_THREADS, 2) void pw_wide_ends_kernel(WeParams p) {
    extern __shared__ __attribute__((aligned(16))) char wc_smem[];          // [WC_RING][WC_STAGE] | bias copy
    constexpr WePlan P = we_plan(CHAIN, HILO);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pnt = lane & 31, hh = lane >> 5;
    float* bias_lds = (float*)(wc_smem + WC_RING * WC_STAGE);
    for (int i = threadIdx.x; i < P.nbias; i += WC_THREADS) bias_lds[i] = p.bias[i];      // (first read behind the first stage barrier)
    const int64_t ntiles = p.m / WC_TILE;
    const int my_tiles = (int)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
    const int nstage_seq = P.nstage;
    const int total_stages = my_tiles * nstage_seq;
    const StageRing<WC_STAGE, 4, WC_RING> ring{p.wpacked, wc_smem, total_stages, wave, lane, nstage_seq, SPLIT};
    ring.issue(0);
    ring.issue(1);
    int n = 0;
#pragma unroll 1
    for (int ti = 0; ti < my_tiles; ++ti) {
        const int64_t tile = blockIdx.x + (int64_t)ti * gridDim.x;
        int64_t row0 = tile * WC_TILE;
        asm volatile("" : "+s"(row0));                        // (opaque: no per-lane 64-bit row pointers stepped from tile to tile)
        half8 bf[16];
        f32x16 acc[8];
        we_segments<CHAIN, HILO, 0>(p, ring, n, row0, wave * 32 + pnt, hh, bias_lds, bf, acc);
    }
}

// the ends' buffer from the plan: every segment's images in execution order (32 pieces each: 8 channel tiles x 4 k-steps or 4 x 8), then the layers' biases
constexpr StageLayout we_layout(const WePlan& P) {
    StageLayout L{};
    for (int sg = 0; sg < P.nseg; ++sg) {
        const WeSegSrc& f = P.from[sg];
        const int kind = P.seg[sg].kind, nt = (kind == WE_K128_C128 || kind == WE_K256_C128) ? 4 : 8;
        sl_frag(L, f.layer, f.ldw, f.c0, P.layer_c[f.layer], f.k0, nt, 32 / nt, we_kind_images(kind));
    }
    for (int i = 0; i < P.nlayer; ++i) sl_row(L, i, 0, P.layer_c[i], P.layer_c[i]);
    return L;
}
// ... holds what the kernel takes from the plan itself: the stage count in front of the biases, and every layer's bias offset
constexpr bool we_layout_ok(int chain, int hilo) {
    const WePlan P = we_plan(chain, hilo);
    const StageLayout L = we_layout(P);
    bool ok = L.par == (size_t)P.nstage * WC_STAGE && L.bytes - L.par == P.nbias * sizeof(float);
    for (int i = 0; i < P.nlayer; ++i) ok = ok && L.row[i].off == P.layer_bias[i];
    return ok;
}
static_assert(we_layout_ok(0, 0) && we_layout_ok(0, 1) && we_layout_ok(1, 0) && we_layout_ok(1, 1), "ends: plan and packed layout disagree");

template <int CHAIN, bool HILO>
static hipError_t we_launch(bool split, hipStream_t s, WeParams& p) {
    constexpr StageLayout L = we_layout(we_plan(CHAIN, HILO));
    p.bias = (const float*)(p.wpacked + L.par);
    return ring_launch<pw_wide_ends_kernel<CHAIN, HILO, false>, pw_wide_ends_kernel<CHAIN, HILO, true>>(p.m / WC_TILE, RING_CAP_CU, WC_THREADS,
                                                                                                        WC_RING * WC_STAGE + L.bytes - L.par, split, s, p);
}

}  // namespace pcd

using namespace pcd;

static int g_wc_split = 1;         // pcd_pw_wide_config: which waves request the weight images (0: every wave 4 pieces; 1, default: one wave per SIMD 8 in the chains;
                                    // 2: in the LN + Linear launches too)
extern "C" int pcd_pw_wide_config(int split) { g_wc_split = split < 0 ? 0 : (split > 2 ? 2 : split); return PCD_OK; }

extern "C" size_t pcd_pw_wide_packed_bytes(int chain) { return (chain == 0 || chain == 1) ? WC_LAYOUT[chain].bytes : 0; }

// chain 0 (E3): w[0..2] = enc3.conv1 [256][256], conv2 [256][256], conv3 [512][256]; chain 1 (D2): dec2.conv1 [256][512], conv2 [256][256],
// conv3 [128][256].  Writes the stage images followed by the per-pass bias rows (4 x 256 fp32) into `packed` (wc_layout).
extern "C" int pcd_pw_wide_pack(int chain, const void* const* w, const float* const* b, void* packed, void* stream) {
    PCD_CHECK_ARG((chain == 0 || chain == 1) && w && b && packed && w[0] && w[1] && w[2] && b[0] && b[1] && b[2]);
    return stage_pack(WC_LAYOUT[chain], w, b, packed, (hipStream_t)stream);
}

extern "C" int pcd_pw_wide_chain(int chain, const void* in1, const void* in2, int64_t m, const void* packed, void* out, void* stream) {
    PCD_CHECK_ARG((chain == 0 || chain == 1) && in1 && packed && out && m > 0 && m % WC_TILE == 0);
    PCD_CHECK_ARG(chain == 0 || in2 != nullptr);
    const StageLayout& L = WC_LAYOUT[chain];
    WcParams p{};
    p.in1 = (const half_t*)in1; p.in2 = (const half_t*)in2; p.m = m;
    p.wpacked = (const char*)packed;
    p.bias = (const float*)(p.wpacked + L.par);
    p.out = (half_t*)out;
    p.nseg = 4;
    p.ldo = chain == 0 ? 512 : 128;
    // how the kernel walks wc_layout's passes: {src, cont, finish, keep_b}; a pass's channels and bias row come from the layout
    static const int walk[2][4][4] = {{{1, 0, 1, 0}, {0, 0, 1, 0}, {0, 0, 2, 1}, {0, 0, 2, 0}}, {{1, 0, 0, 0}, {2, 1, 1, 0}, {0, 0, 1, 0}, {0, 0, 2, 0}}};
    for (int i = 0; i < 4; ++i) {
        const FragBlock& b = L.block[i];
        const int* w = walk[chain][i];
        const int valid = b.row_limit - b.row0;
        p.seg[i] = WcSeg{w[0], w[1], w[2], b.row0, valid < 256 ? valid : 256, L.row[i].off, w[3], 0};
    }
    PCD_CHECK_HIP((ring_launch<pw_wide_chain_kernel<false, false>, pw_wide_chain_kernel<false, true>>(
        m / WC_TILE, RING_CAP_CU, WC_THREADS, WC_RING * WC_STAGE + L.bytes - L.par, g_wc_split != 0, (hipStream_t)stream, p)));
    return PCD_OK;
}

// ---- LayerNorm(256) + Linear(256, 256 P) [+ ReLU] as one launch of the same kernel (P <= 4 output passes over B fragments that are normalised as they are
// loaded): the in_proj and the first FFN layer of the C = 256 attention blocks (reference networks.py:61-66, 81-82) without the LayerNorm launch and its
// 67 + 67 MB.  packed = P x 4 stage images | bias [P][256] fp32 | gamma [256] | beta [256] (wl_layout).
extern "C" size_t pcd_pw_wide_ln_linear_packed_bytes(int passes) { return (passes >= 1 && passes <= 4) ? WL_LAYOUT[passes - 1].bytes : 0; }

extern "C" int pcd_pw_wide_ln_linear_pack(const void* w, const float* b, int passes, const float* ln_g, const float* ln_b, void* packed, void* stream) {
    PCD_CHECK_ARG(w && b && ln_g && ln_b && packed && passes >= 1 && passes <= 4);
    const float* const params[3] = {b, ln_g, ln_b};
    return stage_pack(WL_LAYOUT[passes - 1], &w, params, packed, (hipStream_t)stream);
}

extern "C" int pcd_pw_wide_ln_linear_supported(int dim, int64_t rows) { return dim == 256 && rows > 0 && rows % WC_TILE == 0 ? 1 : 0; }

extern "C" int pcd_pw_wide_ln_linear(const void* packed, int passes, int relu, const void* x, int64_t m, void* out, void* stream) {
    PCD_CHECK_ARG(packed && x && out && x != out && passes >= 1 && passes <= 4 && m > 0 && m % WC_TILE == 0);
    const StageLayout& L = WL_LAYOUT[passes - 1];
    WcParams p{};
    p.in1 = (const half_t*)x; p.in2 = nullptr; p.m = m;
    p.wpacked = (const char*)packed;
    p.bias = (const float*)(p.wpacked + L.par);
    p.ln = p.bias + L.row[1].off;
    p.out = (half_t*)out; p.ldo = 256 * passes;
    p.nseg = passes;
    for (int i = 0; i < passes; ++i) p.seg[i] = WcSeg{i == 0 ? 1 : 0, 0, 2, 256 * i, 256, L.row[0].off + 256 * i, i + 1 < passes ? 1 : 0, relu ? 0 : 1};
    // (the LN + Linear launches store a 256-wide output piece per pass: a requesting wave's vmcnt(0) would wait for those stores at every stage -- measured neutral to
    // slightly slower in the attention U-Net's forward, so they keep "every wave requests" unless pcd_pw_wide_config(2) asks for the split form)
    PCD_CHECK_HIP((ring_launch<pw_wide_chain_kernel<true, false>, pw_wide_chain_kernel<true, true>>(m / WC_TILE, RING_CAP_CU, WC_THREADS, WC_LDS_MAX, g_wc_split == 2,
                                                                                                    (hipStream_t)stream, p)));
    return PCD_OK;
}

// ---- the narrow ends of UNetPointNetLarge as one launch each (pw_wide_ends_kernel): chain 0 = E23, enc2.conv1-3 + enc3.conv1-3 (w[0..5], b[0..5]: x1 [M][128] ->
// x2 [M][256] and x3 [M][512]); chain 1 = D21, dec2.conv1-3 + dec1.conv1 (w[0..3]: [in1 [M][256] | in2 [M][256]] -> ... -> [. | in3 [M][128]] -> out [M][128]).
// hilo: the chain's narrow layer (enc2.conv3 / dec1.conv1) carries [c][2 k] hi | lo weights.  packed = the stage images in execution order | the layers' biases
// (we_layout).
extern "C" size_t pcd_pw_wide_ends_packed_bytes(int chain, int hilo) {
    return (chain == 0 || chain == 1) ? we_layout(we_plan(chain, hilo ? 1 : 0)).bytes : 0;
}

extern "C" int pcd_pw_wide_ends_pack(int chain, int hilo, const void* const* w, const float* const* b, void* packed, void* stream) {
    PCD_CHECK_ARG((chain == 0 || chain == 1) && w && b && packed);
    const WePlan P = we_plan(chain, hilo ? 1 : 0);
    for (int i = 0; i < P.nlayer; ++i) PCD_CHECK_ARG(w[i] != nullptr && b[i] != nullptr);
    return stage_pack(we_layout(P), w, b, packed, (hipStream_t)stream);
}

extern "C" int pcd_pw_wide_ends(int chain, int hilo, const void* in1, const void* in2, const void* in3, int64_t m, const void* packed, void* out, void* out2,
                                void* stream) {
    PCD_CHECK_ARG((chain == 0 || chain == 1) && in1 && packed && out && m > 0 && m % WC_TILE == 0 && m <= 0x7fffffff);
    PCD_CHECK_ARG(chain == 0 ? out2 != nullptr : (in2 != nullptr && in3 != nullptr));
    WeParams p{};
    p.in1 = (const half_t*)in1; p.in2 = (const half_t*)in2; p.in3 = (const half_t*)in3; p.m = m;
    p.wpacked = (const char*)packed;
    p.out = (half_t*)out;
    p.out2 = (half_t*)out2;
    hipStream_t s = (hipStream_t)stream;
    const bool split = g_wc_split != 0;
    hipError_t e;
    if (chain == 0) e = hilo ? we_launch<0, true>(split, s, p) : we_launch<0, false>(split, s, p);
    else e = hilo ? we_launch<1, true>(split, s, p) : we_launch<1, false>(split, s, p);
    PCD_CHECK_HIP(e);
    return PCD_OK;
}
