// K9: the k3 / k4 convolutions of VAE3DLarge with an LDS-resident input halo (the layers whose implicit-GEMM form,
// csrc/conv3d_igemm.hip, is bound by its gather): k3 s1 with the weights through an LDS ring or in registers,
// Conv3d(k4, s2) 64 -> 64 and ConvTranspose3d(k4, s2) 128 -> 64.
#include "conv3d.h"

namespace pcd {

// ---------------------------------------------------------------------------------------------------
// k3 / stride 1 / pad 1 with an LDS-resident input halo.  The implicit GEMM (conv3d_igemm.hip) re-gathers every input
// voxel once per tap (27x) from L2; at C_out <= 64 that gather traffic (24 KB per 1 MFLOP tile step) is
// what bounds the 32^3 layers.  Here a workgroup owns a 4 x 4 x 8 block of output voxels (128 GEMM rows),
// loads the 6 x 6 x 10 input halo ONCE into LDS and reads the A fragments of all 27 taps from it; only the
// weights stream (G taps per stage, LDS-DMA, three buffers).
// Halo image: voxel v = (hz * 6 + hy) * 10 + hx at v * C_in * 2 bytes, its 16-byte chunk c stored at chunk c ^ s(hx, hy):
//   C_in = 64 (8 chunks, two voxels per 256-B bank row):   s = ((hx >> 1) & 1) << 1 | (hy & 1) << 2
//   C_in = 32 (4 chunks, four voxels per bank row):        s = (hy & 1) << 1
// A ds_read_b128 is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32
// (MI355X_MICROARCH.md, LDS): a group holds all 16 rows of an MFMA block (two y rows of 8 x), rows 0-3 and 12-15 with
// k chunk q, rows 4-11 with q ^ 1, and is conflict-free when the 16 lanes hit 16 distinct 16-B slots of the bank row.
// With these s they do, for every tap shift (checked exhaustively; the round-1 layout, rows padded to C_in * 2 + 16
// bytes, was a 3-way conflict on every A read: SQ_LDS_BANK_CONFLICT 54 % of the LDS cycles).
struct HaloParams {
    const half_t* in; int B, D, H, W;
    const half_t* w; int kpad;        // [Cout][kpad], k = tap * CIN + c, taps in (kz, ky, kx) order
    const float* bias;
    const half_t* resid;
    half_t* out; int Cout;
    int relu;
    int tiles_n, tz, ty, tx;          // tiles per dimension
    int nblocks;
    const half_t* in2;                // CIN2 > 0: second source [B][D][H][W][CIN2] (the block input of a projection shortcut), K columns 27 * CIN ..
};

// NW waves per workgroup: 4 (2 x 2 or 4 x 1 wave grid, 64 x 32 / 32 x 32 wave tiles; what the launcher uses) or, for
// C_out = 64, 2 waves of 64 x 64 (8 fragment reads per 16 MFMAs instead of 6 per 8, but one wave per SIMD: measured
// slower, kept as a template parameter only).
// TY = 4: 4 x 4 x 8 output voxels (128 rows) per workgroup of four waves.  TY = 8: 4 x 8 x 8 voxels (256 rows) per workgroup of
// eight waves with the same wave tiles: the weights of a tap (and a smaller share of halo) are filled once per 256 rows.
// Used for 32 -> 32, where two such workgroups still fit a CU (64 KB of LDS each): 77 -> 69 us.  At C_in = 64 (94-110 KB,
// one workgroup per CU) it measured equal or slower, also as a persistent kernel that prefetches its next halo.
// CIN2 = 32: one more 32-deep k step behind the 27 taps -- the rows of a SECOND tensor (the residual block's input x, 32 channels) against
// weight columns 27 * CIN .. + 32: ResidualBlock3D's 1x1x1 projection shortcut summed into conv2's accumulators (pcd_conv3d_desc_t.in2).
// x's 128 rows (8 KB) and those 32 weight columns (4 KB) are requested with the halo, wait in registers and pass through the weight ring
// after the last tap (no LDS of their own: two workgroups must still fit a CU).
template <int CIN, int BN, int G, int NSTAGE, int NW, int TY = 4, int CIN2 = 0>
__global__ __launch_bounds__(64 * NW) void conv3d_halo_kernel(HaloParams p) {
    constexpr int NT = 64 * NW;
    constexpr int HHY = TY + 2, HROWS = (HTZ + 2) * HHY * HHX, ROWS = HTZ * TY * HTX, YSH = TY == 8 ? 3 : 2;   // shadow the 128-row geometry
    constexpr int RB = CIN * 2, P = RB, CPR = RB / 16, KS = CIN / 32;
    constexpr int NXV = CIN == 64 ? 3 : 1;                      // address variants per k_x (the swizzle of C_in = 64 depends on hx)
    constexpr int HALO_BYTES = HROWS * P;
    constexpr int BST = G * BN * RB;                          // bytes per weight stage
    constexpr int WAVES_N = (NW >= 4) ? BN / 32 : 1, WAVES_M = NW / WAVES_N, WMR = ROWS / WAVES_M, MI = WMR / 16;
    constexpr int WNC = BN / WAVES_N, NI = WNC / 16;
    constexpr int OUT_LD = BN * 2 + 16;
    constexpr int NS = 27 / G;
    constexpr int HIT = (HROWS * CPR + NT - 1) / NT;          // halo chunks per thread
    constexpr int RPI = 1024 / RB;                            // weight rows per wave-wide DMA instruction
    constexpr int NINSTR = G * BN / RPI;
    constexpr int U = (NINSTR + NW - 1) / NW;                       // DMA instructions per wave and stage (uniform, so
    constexpr int DUMP = (NINSTR % NW) ? 1024 : 0;             // the vmcnt arithmetic is: spare ones hit a dump KB)
    static_assert(27 % G == 0 && ROWS * OUT_LD <= HALO_BYTES && HALO_BYTES % 16 == 0 && NS >= NSTAGE, "layout");
    // second source: its rows and weight columns take over the weight ring once the 27 taps are done (two workgroups per CU need <= 80 KB each)
    constexpr int X2_OFF = HALO_BYTES, W2_OFF = X2_OFF + ROWS * 64;
    static_assert(CIN2 == 0 || (CIN2 == 32 && ROWS * 4 % NT == 0 && BN * 4 <= NT && (ROWS + BN) * 64 <= NSTAGE * BST),
                  "second source: 64-byte rows, one k step, inside the weight ring");
    __shared__ __attribute__((aligned(16))) char smem[HALO_BYTES + NSTAGE * BST + DUMP];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // consecutive workgroups go round-robin over the 8 XCDs: give each XCD a contiguous run of tiles so that
    // neighbouring tiles (which share halo voxels) meet in the same L2
    int bid = blockIdx.x;
    if ((p.nblocks & 7) == 0) bid = (bid & 7) * (p.nblocks >> 3) + (bid >> 3);
    const int tn = bid % p.tiles_n; int t = bid / p.tiles_n;
    const int tx = t % p.tx; t /= p.tx;
    const int ty = t % p.ty; t /= p.ty;
    const int tz = t % p.tz; const int b = t / p.tz;
    const int z0 = tz * HTZ, y0 = ty * TY, x0 = tx * HTX, n0 = tn * BN;

    // ---- halo: global -> registers -> LDS (once)
    // (loads are unconditional from a clamped address and zeroed afterwards: no divergent branches,
    //  all HIT loads in flight together)
    half8 hv[HIT];
    unsigned okmask = 0;
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int c = it * NT + tid;
        const int row = c / CPR, ch = c - row * CPR;
        const int hx = row % HHX; const int r2 = row / HHX;
        const int hy = r2 % HHY, hz = r2 / HHY;
        const int iz = z0 - 1 + hz, iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = row < HROWS && (unsigned)iz < (unsigned)p.D && (unsigned)iy < (unsigned)p.H &&
                        (unsigned)ix < (unsigned)p.W;
        okmask |= ok ? 1u << it : 0u;
        const int cz = min(max(iz, 0), p.D - 1), cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);
        hv[it] = *(const half8*)(p.in + ((((int64_t)b * p.D + cz) * p.H + cy) * p.W + cx) * CIN + ch * 8);
    }

    // rows of the second source and its 32 weight columns: requested with the halo, stored behind it
    constexpr int X2IT = CIN2 ? ROWS * 4 / NT : 1;
    half8 x2v[X2IT], w2v;
    if constexpr (CIN2 > 0) {
#pragma unroll
        for (int it = 0; it < X2IT; ++it) {
            const int c = it * NT + tid, m = c >> 2, ch = c & 3;
            const int x = m & 7, y = (m >> 3) & (TY - 1), z = m >> (3 + YSH);
            x2v[it] = *(const half8*)(p.in2 + ((((int64_t)b * p.D + z0 + z) * p.H + y0 + y) * p.W + x0 + x) * CIN2 + ch * 8);
        }
        int nn = n0 + (tid >> 2);
        nn = nn < p.Cout ? nn : p.Cout - 1;
        w2v = *(const half8*)(p.w + (int64_t)nn * p.kpad + 27 * CIN + (tid & 3) * 8);
    }

    auto stageB = [&](int s, int buf) {
        char* base = smem + HALO_BYTES + buf * BST;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int it = wave + NW * u;
            const bool real = it < NINSTR;
            const int row = (real ? it : 0) * RPI + lane / CPR;
            const int g = row / BN, n = row % BN;
            const int lch = (lane % CPR) ^ (RB == 128 ? (n >> 1) & 7 : (-(n >> 2)) & 3);
            int nn = n0 + n;
            nn = nn < p.Cout ? nn : p.Cout - 1;
            lds_dma16(p.w + (int64_t)nn * p.kpad + (s * G + g) * CIN + lch * 8,
                        real ? base + it * 1024 : smem + HALO_BYTES + NSTAGE * BST);
        }
    };
    stageB(0, 0);
    if (NS > 1) stageB(1, 1);
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int c = it * NT + tid;
        const int row = c / CPR, ch = c - row * CPR;
        const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const int hx = row % HHX, hy = (row / HHX) % HHY;
        const int sw = CIN == 64 ? (((hx >> 1) & 1) << 1) | ((hy & 1) << 2) : (hy & 1) << 1;
        if (row < HROWS) *(half8*)(smem + row * P + ((ch ^ sw) << 4)) = (okmask >> it) & 1 ? hv[it] : zero8;
    }

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int q = lane >> 4;
    // A fragment address of row block i for a tap (kz, ky, kx) and k step ks: areg[i][kx][ks ^ (ky & 1)] + the tap's
    // voxel offset (a compile-time immediate); the low bits carry the swizzle of the voxel the tap lands on
    int areg[MI][NXV][2], boff[NI][KS];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int m = wm * WMR + i * 16 + (lane & 15);
        const int x = m & 7, y = (m >> 3) & (TY - 1), z = m >> (3 + YSH);
        const int vrow = ((z * HHY + y) * HHX + x) * P;
#pragma unroll
        for (int kx = 0; kx < NXV; ++kx)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int hyb = (e ^ y) & 1;                                     // (ks ^ hy) & 1
                areg[i][kx][e] = vrow + (CIN == 64 ? (hyb << 6) | ((q ^ ((((x + kx) >> 1) & 1) << 1)) << 4)
                                                   : (q ^ (hyb << 1)) << 4);
            }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int n = wn * WNC + j * 16 + (lane & 15);
        const int sw = RB == 128 ? (n >> 1) & 7 : (-(n >> 2)) & 3;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) boff[j][ks] = HALO_BYTES + n * RB + (((ks * 4 + q) ^ sw) << 4);
    }

    // Fragment registers are double buffered per 32-wide k step: while the MFMAs of step u run, the fragments
    // of step u+1 are on their way from LDS (A from the halo, which never changes; B from the weight stage).
    // One step ahead, not one tap: a wave can have at most 15 LDS reads outstanding (lgkmcnt is 4 bits).
    half8 af[2][MI], bf[2][NI];
    auto readA = [&](int par, int tap, int ks) {
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const int voff = ((kz * HHY + ky) * HHX + kx) * P;
#pragma unroll
        for (int i = 0; i < MI; ++i)
            af[par][i] = *(const half8*)(smem + areg[i][NXV == 3 ? kx : 0][(ks ^ ky) & 1] + voff);
    };
    auto readB = [&](int par, const char* bbuf, int g, int ks) {
#pragma unroll
        for (int j = 0; j < NI; ++j) bf[par][j] = *(const half8*)(bbuf + boff[j][ks] + g * BN * RB);
    };
    // Weight stages: buffer s % NSTAGE.  The barrier of stage s publishes stage s+1 (every wave waited for its own
    // DMAs of it; with four buffers the DMAs of stage s+2 stay in flight behind a counted vmcnt) and frees the buffer
    // of stage s-1 for stage s+NSTAGE-1.  A stage is therefore requested NSTAGE-2 taps before the barrier that needs
    // it: one tap of MFMAs (~500 cycles per wave) does not cover an L2 round trip, two do.  The fragment prefetch runs
    // one k step ahead, also across a stage boundary.  Fully unrolled (27 taps): with a loop back-edge the compiler's
    // waitcnt pass falls back to lgkmcnt(0) in front of the MFMAs, which drains the prefetch it is meant to overlap.
    static_assert(NSTAGE == 3 || NSTAGE == 4, "the prefetch protocol below is written for three or four weight buffers");
    if (NSTAGE == 4 && NS > 2) {
        stageB(2, 2);
        wait_vmcnt<2 * U>();
    } else {
        wait_vmcnt<(NS > 1) ? U : 0>();
    }
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    readA(0, 0, 0);
    readB(0, smem, 0, 0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) {
            if (NSTAGE == 4 && s + 2 < NS) wait_vmcnt<U>(); else wait_vmcnt<0>();
            wait_lgkm0();
            __builtin_amdgcn_s_barrier();   // raw: __syncthreads() adds its own waits
            if (s + NSTAGE - 1 < NS) stageB(s + NSTAGE - 1, (s + NSTAGE - 1) % NSTAGE);
        }
        const char* bcur = smem + (s % NSTAGE) * BST;
        const char* bnxt = smem + ((s + 1) % NSTAGE) * BST;
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int par = ((s * G + g) * KS + ks) & 1;
                if (ks + 1 < KS) {
                    readA(par ^ 1, s * G + g, ks + 1);
                    readB(par ^ 1, bcur, g, ks + 1);
                } else if (g + 1 < G) {
                    readA(par ^ 1, s * G + g + 1, 0);
                    readB(par ^ 1, bcur, g + 1, 0);
                } else if (s + 1 < NS) {
                    readA(par ^ 1, (s + 1) * G, 0);
                    readB(par ^ 1, bnxt, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[par][i], bf[par][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
    }

    if constexpr (CIN2 > 0) {
        // the 28th k step: second-source rows x the shortcut's weight columns, through the weight ring (every tap has been read and no
        // DMA is in flight: the last stage was waited for two taps ago).  64-byte rows, chunk c of row r at c ^ ((-(r >> 2)) & 3) (swz<32>)
        __syncthreads();
#pragma unroll
        for (int it = 0; it < X2IT; ++it) {
            const int c = it * NT + tid, m = c >> 2, ch = c & 3;
            *(half8*)(smem + X2_OFF + m * 64 + ((ch ^ ((-(m >> 2)) & 3)) << 4)) = x2v[it];
        }
        if (tid < BN * 4) *(half8*)(smem + W2_OFF + (tid >> 2) * 64 + (((tid & 3) ^ ((-(tid >> 4)) & 3)) << 4)) = w2v;
        __syncthreads();
        half8 a2[MI], b2[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = wm * WMR + i * 16 + (lane & 15);
            a2[i] = *(const half8*)(smem + X2_OFF + m * 64 + ((q ^ ((-(m >> 2)) & 3)) << 4));
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int n = wn * WNC + j * 16 + (lane & 15);
            b2[j] = *(const half8*)(smem + W2_OFF + n * 64 + ((q ^ ((-(n >> 2)) & 3)) << 4));
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[i], b2[j], acc[i][j], 0, 0, 0);
    }

    // epilogue (same rounding points as conv3d_igemm_kernel): bias -> fp16 in LDS -> 16-B row stores
    const int colq = lane & 15;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int lcol = wn * WNC + j * 16 + colq;
        const float bc = (p.bias != nullptr && n0 + lcol < p.Cout) ? p.bias[n0 + lcol] : 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lrow = wm * WMR + i * 16 + q * 4 + r;
                float v = acc[i][j][r] + bc;
                if (p.relu && p.resid == nullptr) v = fmaxf(v, 0.f);
                *(half_t*)(smem + lrow * OUT_LD + lcol * 2) = to_half_sat(v);
            }
    }
    __syncthreads();
    constexpr int OCPR = BN / 8, TOTAL = ROWS * OCPR;
#pragma unroll
    for (int it = 0; it < TOTAL / NT; ++it) {
        const int idx = it * NT + tid;
        const int lrow = idx / OCPR, ch = idx - lrow * OCPR;
        const int col = n0 + ch * 8;
        if (col < p.Cout) {
            const int x = lrow & 7, y = (lrow >> 3) & (TY - 1), z = lrow >> (3 + YSH);
            const int64_t orow = (((int64_t)b * p.D + z0 + z) * p.H + y0 + y) * p.W + x0 + x;
            half8 v = *(const half8*)(smem + lrow * OUT_LD + ch * 16);
            if (p.resid != nullptr) {
                const half8 rs = *(const half8*)(p.resid + orow * p.Cout + col);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float f = (float)v[e] + (float)rs[e];
                    if (p.relu) f = fmaxf(f, 0.f);
                    v[e] = to_half_sat(f);
                }
            }
            *(half8*)(p.out + orow * p.Cout + col) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// ConvTranspose3d(k4, s2, p1) + ReLU, C_in = 128 -> C_out = 64 (decoder.6, reference networks.py:2253), with the input halo in LDS.
// As eight output-parity classes through the implicit GEMM (conv3d_igemm.hip) this layer is a 128 x 64 tile per class (43 FLOP per gathered
// byte) and every input voxel is fetched 8 x 8 times: 556 TFLOP/s.  Here a workgroup owns 4 x 4 x 8 INPUT voxels, loads their
// 6 x 6 x 10 halo (offsets -1 .. +1 cover every class: o = 2 i - 1 + k) ONCE -- 92 KB -- and computes all eight classes
// (8 x 128 output voxels x 64 channels) from it; only the weights stream (1 MB per workgroup, 16-KB stages in a ring of four).
//   * eight waves: two classes at a time (px = 0 / 1 of one (pz, py) pair), four waves per class as 2 voxel halves x 2 channel
//     halves, wave tile 64 voxels x 32 channels;
//   * the product is taken TRANSPOSED, D[channel][voxel] (weights = MFMA A operand, voxels = B), so a lane's accumulators are
//     four consecutive channels of one voxel: two 16-channel blocks trade halves (v_permlane16_swap) and every lane stores
//     16 contiguous bytes of an output row -- no LDS staging, so the weight ring keeps streaming through the epilogues;
//   * halo image: voxel v = (hz * 6 + hy) * 10 + hx at v * 256 B (one 64-bank row per voxel), its 16-byte chunk c at slot
//     c ^ ((hx & 7) << 1): a ds_read_b128 lane group holds 8 voxels with chunk c and 8 with chunk c ^ 1 (MI355X_MICROARCH.md, LDS),
//     the 16 voxels of an MFMA block have 8 distinct x twice, so the slots are 16 distinct ones for every tap shift;
//   * weight stage = one tap x one 64-channel half of K x two classes (2 x 64 rows of 128 B, the swz<64> of the GEMM),
//     requested three stages ahead, counted vmcnt (the epilogue's four stores per wave are counted too).
struct ConvTHaloParams {
    const half_t* in; int B, D, H, W;
    const half_t* w[8];               // class 4 pz + 2 py + px: [64][8 * 128], tap t = (tz * 2 + ty) * 2 + tx reads input offset p - t per axis
    const float* bias;
    half_t* out;                      // [B][2D][2H][2W][64]
    int tz, ty, tx, nblocks;
};

__global__ __launch_bounds__(512) void convT3d_halo_kernel(ConvTHaloParams p) {
    constexpr int CIN = 128, COUT = 64, VB = CIN * 2, NW = 8, NT = 512, NSTAGE = 4;
    constexpr int HALO_BYTES = HROWS * VB;                   // 360 voxels x 256 B
    constexpr int BST = 2 * COUT * 128;                      // stage: 2 classes x 64 rows x 64 k
    constexpr int U = BST / 1024 / NW;                       // DMA instructions per wave and stage (2)
    constexpr int NSTG = 64;                                 // 4 class pairs x 8 taps x 2 K halves
    constexpr int HIT = (HROWS * 16 + NT - 1) / NT;
    constexpr int NSTORE = 4;                                // epilogue stores per wave and class pair
    static_assert(U * NW * 1024 == BST && HALO_BYTES + NSTAGE * BST <= 160 * 1024, "layout");
    __shared__ __attribute__((aligned(16))) char smem[HALO_BYTES + NSTAGE * BST];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = wave >> 2, wv = (wave >> 1) & 1, wc = wave & 1;   // class in the pair (= px), voxel half, channel half
    int bid = blockIdx.x;
    if ((p.nblocks & 7) == 0) bid = (bid & 7) * (p.nblocks >> 3) + (bid >> 3);
    int t = bid;
    const int tx = t % p.tx; t /= p.tx;
    const int ty = t % p.ty; t /= p.ty;
    const int tz = t % p.tz; const int b = t / p.tz;
    const int z0 = tz * HTZ, y0 = ty * HTY, x0 = tx * HTX;

    // ---- halo: global -> registers (all loads in flight) -> LDS
    half8 hv[HIT];
    unsigned okmask = 0;
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int c = it * NT + tid;
        const int row = c >> 4, ch = c & 15;
        const int hx = row % HHX; const int r2 = row / HHX;
        const int hy = r2 % HHY, hz = r2 / HHY;
        const int iz = z0 - 1 + hz, iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = row < HROWS && (unsigned)iz < (unsigned)p.D && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        okmask |= ok ? 1u << it : 0u;
        const int cz = min(max(iz, 0), p.D - 1), cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);
        hv[it] = *(const half8*)(p.in + ((((int64_t)b * p.D + cz) * p.H + cy) * p.W + cx) * CIN + ch * 8);
    }

    const int q = lane >> 4, n16 = lane & 15;
    float bv[2][4];                                    // bias of this lane's channels (requested before any DMA: older in vmcnt order)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[i][r] = p.bias != nullptr ? p.bias[wc * 32 + i * 16 + q * 4 + r] : 0.f;

    // stage S = (pair, tap, K half): instruction it = wave + 8 u covers rows it * 8 .. + 7 of the 128 (class u, channels (wave * 8 ..) + lane / 8)
    auto stageW = [&](int S, int buf) {
        const int pair = S >> 4, tap = (S >> 1) & 7, kh = S & 1;
        char* base = smem + HALO_BYTES + buf * BST;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = wave * 8 + (lane >> 3);
            const int lch = (lane & 7) ^ ((n >> 1) & 7);
            lds_dma16(p.w[2 * pair + u] + n * (8 * CIN) + tap * CIN + kh * 64 + lch * 8, base + (wave + NW * u) * 1024);
        }
    };
    stageW(0, 0);
    stageW(1, 1);
    stageW(2, 2);
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int c = it * NT + tid;
        const int row = c >> 4, ch = c & 15;
        const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const int hx = row % HHX;
        if (row < HROWS) *(half8*)(smem + row * VB + ((ch ^ ((hx & 7) << 1)) << 4)) = (okmask >> it) & 1 ? hv[it] : zero8;
    }

    // voxel blocks of this wave: j -> (z = 2 wv + (j >> 1), y = 2 (j & 1) + (n16 >> 3), x = n16 & 7); halo voxel without a tap = + (1, 1, 1)
    const int vx = n16 & 7;
    int vrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) vrow[j] = (((2 * wv + (j >> 1) + 1) * HHY + 2 * (j & 1) + (n16 >> 3) + 1) * HHX + vx + 1) * VB;
    // weight rows of this wave in a stage: class cw, channels wc * 32 + i * 16 + n16
    int wrow[2], wsw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = wc * 32 + i * 16 + n16;
        wrow[i] = HALO_BYTES + (cw * COUT + n) * 128;
        wsw[i] = (n >> 1) & 7;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    wait_vmcnt<2 * U>();                          // stage 0 (and, before it, the halo loads) landed; stages 1, 2 in flight
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();

    const int OD = 2 * p.D, OH = 2 * p.H, OW = 2 * p.W;
#pragma unroll 1
    for (int pair = 0; pair < 4; ++pair) {
        const int pz = pair >> 1, py = pair & 1, px = cw;
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int S = pair * 16 + st;
            if (S + 1 < NSTG) {
                // publish stage S + 1: behind it at most stage S + 2 (and, right after a pair's epilogue, that epilogue's stores) may stay in flight
                if (st < 2) {
                    if (pair > 0) wait_vmcnt<U + NSTORE>(); else wait_vmcnt<U>();
                } else if (st == 14 && pair == 3) {
                    wait_vmcnt<0>();
                } else {
                    wait_vmcnt<U>();
                }
                wait_lgkm0();
                __builtin_amdgcn_s_barrier();
                if (S + 3 < NSTG) stageW(S + 3, (S + 3) & 3);
            }
            const int tap = st >> 1, kh = st & 1;
            const int dz = pz - (tap >> 2), dy = py - ((tap >> 1) & 1), dx = px - (tap & 1);
            const int voff = ((dz * HHY + dy) * HHX + dx) * VB;
            const int sw = ((vx + 1 + dx) & 7) << 1;
            const char* wb = smem + (S & 3) * BST;
#pragma unroll
            for (int ksl = 0; ksl < 2; ++ksl) {
                half8 af[2], bf[4];
                const int kc = (kh * 2 + ksl) * 4 + q;                     // 16-byte chunk of the voxel's 128 channels
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *(const half8*)(wb + wrow[i] + (((ksl * 4 + q) ^ wsw[i]) << 4));
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = *(const half8*)(smem + vrow[j] + voff + ((kc ^ sw) << 4));
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
        // epilogue of the pair: bias, ReLU, fp16; channel blocks 0 / 1 trade halves, lane group q stores 8 consecutive channels of
        // block (q & 1) at offset 8 * (q >> 1) of its voxel's output row
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned pk[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
                half2_t lo2, hi2;
                lo2[0] = to_half_sat(fmaxf(acc[i][j][0] + bv[i][0], 0.f)); lo2[1] = to_half_sat(fmaxf(acc[i][j][1] + bv[i][1], 0.f));
                hi2[0] = to_half_sat(fmaxf(acc[i][j][2] + bv[i][2], 0.f)); hi2[1] = to_half_sat(fmaxf(acc[i][j][3] + bv[i][3], 0.f));
                pk[i][0] = __builtin_bit_cast(unsigned, lo2);
                pk[i][1] = __builtin_bit_cast(unsigned, hi2);
                acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            const auto s0 = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
            const auto s1 = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
            const int z = 2 * wv + (j >> 1), y = 2 * (j & 1) + (n16 >> 3);
            const int64_t orow = (((int64_t)b * OD + 2 * (z0 + z) + pz) * OH + 2 * (y0 + y) + py) * OW + 2 * (x0 + vx) + px;
            *(u32x4*)(p.out + orow * COUT + wc * 32 + (q & 1) * 16 + (q >> 1) * 8) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Conv3d(k4, s2, p1) + ReLU, C_in = 64 -> C_out = 64 (encoder.3, reference networks.py:2229), with LDS-resident input.
// Through the implicit GEMM this layer is a 128 x 64 tile at 43 FLOP per gathered byte (every input voxel fetched 8 times, every
// tile re-gathering its 64 taps): 584 TFLOP/s, the slowest large layer of the encoder.  The stride-2 kernel splits by INPUT parity:
// out(o) = sum_k in(2 o - 1 + k) w(k), and per axis the even inputs are reached by k = 1, 3 at sub-grid index o, o + 1, the odd ones
// by k = 0, 2 at o - 1, o -- eight classes, each a 2 x 2 x 2 stride-1 convolution of one sub-sampled grid, all summed into the SAME
// output.  A workgroup owns 4 x 4 x 8 output voxels; per class it holds the 5 x 5 x 9 sub-grid halo (input voxel 2 (o0 + h) - parity,
// in the 6 x 10 pitch and with the swizzle of conv3d_halo_kernel's C_in = 64 image, so the same conflict-free fragment reads)
// and runs the class's 8 taps from it; the next class's halo is requested at the class's first tap (into registers) and swapped in
// behind one barrier; the weights stream through the same ring of four 8-KB stages over all 64 (class, tap) stages; the product
// is taken transposed with 16-byte direct stores like convT3d_halo_kernel.  70 KB of LDS: two workgroups per CU, the other one
// computes through this one's halo swaps.
struct ConvS2HaloParams {
    const half_t* in; int B, D, H, W;    // input grid (even dims); output grid D/2 x H/2 x W/2
    const half_t* w; int kpad;            // [64][kpad], k = ((kz * 4 + ky) * 4 + kx) * 64 + c
    const float* bias;
    half_t* out;
    int relu;
    int tz, ty, tx, nblocks;
};

__global__ __launch_bounds__(256) void conv3d_k4s2_halo_kernel(ConvS2HaloParams p) {
    constexpr int CIN = 64, COUT = 64, P = CIN * 2, NW = 4, NT = 256, NSTAGE = 4;
    constexpr int HALO_BYTES = HROWS * P;                    // the 6 x 6 x 10 pitch of the stride-1 kernels (5 x 5 x 9 voxels used)
    constexpr int BST = COUT * P;                            // one tap: 64 rows x 128 B
    constexpr int U = BST / 1024 / NW;                       // DMA instructions per wave and stage (2)
    constexpr int NSTG = 64;                                 // 8 classes x 8 taps
    constexpr int SV = 5 * 5 * 9, HIT = (SV * 8 + NT - 1) / NT;   // sub-halo voxels; 16-byte chunks per thread (8)
    __shared__ __attribute__((aligned(16))) char smem[HALO_BYTES + NSTAGE * BST];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;                 // voxel half (64 of the 128), channel half
    int bid = blockIdx.x;
    if ((p.nblocks & 7) == 0) bid = (bid & 7) * (p.nblocks >> 3) + (bid >> 3);
    int t = bid;
    const int tx = t % p.tx; t /= p.tx;
    const int ty = t % p.ty; t /= p.ty;
    const int tz = t % p.tz; const int b = t / p.tz;
    const int z0 = tz * HTZ, y0 = ty * HTY, x0 = tx * HTX;   // output block origin

    // this thread's chunks of a class's sub-halo: chunk c = it * 256 + tid -> voxel c >> 3 = (hz * 5 + hy) * 9 + hx, 16-byte piece c & 7.
    // Everything that does not depend on the class is worked out once: the chunk's element offset for class (0, 0, 0) (input voxel 2 (o0 + h)),
    // its LDS address, and six validity bits (per axis: index 2 (o0 + h) inside the grid for an even class / 2 (o0 + h) - 1 for an odd one);
    // class (cz, cy, cx) then reads (cz H W + cy W + cx) C_in elements earlier
    half8 hv[HIT];
    int hoff[HIT], hlds[HIT];
    unsigned hflags = 0;                                     // 6 bits per chunk... packed 4 chunks per word would not fit: one word per axis pair below
    unsigned fz = 0, fy = 0, fx = 0;                         // bit 2 it: even class valid, bit 2 it + 1: odd class valid
    (void)hflags;
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int c = it * NT + tid;
        const int v = c >> 3, ch = c & 7;
        const int hx = v % 9; const int r2 = v / 9;
        const int hy = r2 % 5, hz = r2 / 5;
        const int iz = 2 * (z0 + hz), iy = 2 * (y0 + hy), ix = 2 * (x0 + hx);
        const bool real = v < SV;
        fz |= ((real && iz < p.D) ? 1u : 0u) << (2 * it) | ((real && iz >= 1 && iz - 1 < p.D) ? 2u : 0u) << (2 * it);
        fy |= ((iy < p.H) ? 1u : 0u) << (2 * it) | ((iy >= 1 && iy - 1 < p.H) ? 2u : 0u) << (2 * it);
        fx |= ((ix < p.W) ? 1u : 0u) << (2 * it) | ((ix >= 1 && ix - 1 < p.W) ? 2u : 0u) << (2 * it);
        hoff[it] = (((b * p.D + iz) * p.H + iy) * p.W + ix) * CIN + ch * 8;
        const int sw = (((hx >> 1) & 1) << 1) | ((hy & 1) << 2);
        hlds[it] = real ? ((hz * HHY + hy) * HHX + hx) * P + ((ch ^ sw) << 4) : -1;
    }
    unsigned okmask = 0;
    auto halo_request = [&](int cls) __attribute__((always_inline)) {
        const int cz = cls >> 2, cy = (cls >> 1) & 1, cx = cls & 1;
        const int delta = ((cz * p.H + cy) * p.W + cx) * CIN;
        const unsigned m = (fz >> cz) & (fy >> cy) & (fx >> cx);
        okmask = 0;
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const bool ok = (m >> (2 * it)) & 1;
            okmask |= ok ? 1u << it : 0u;
            const half_t* g = p.in + (ok ? hoff[it] - delta : 0);
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(hv[it]) : "v"(g) : "memory");      // (the kernel owns every vmcnt wait)
        }
    };
    auto halo_store = [&]() __attribute__((always_inline)) {
        // the loads above are asm: to the compiler their registers were defined at the request.  Re-define them HERE, behind the wait that retired
        // the loads, so that nothing computed from them (the zero-fill select below) can be scheduled ahead of their landing
#pragma unroll
        for (int it = 0; it < HIT; ++it) asm volatile("" : "+v"(hv[it]));
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
            if (hlds[it] >= 0) *(half8*)(smem + hlds[it]) = (okmask >> it) & 1 ? hv[it] : zero8;
        }
    };
    // stage S = class * 8 + tap (tz, ty, tx): the k4 tap (2 t + 1 - parity) per axis; rows wave * 16 + 8 u + lane / 8 of the 64
    auto stageW = [&](int S, int buf) __attribute__((always_inline)) {
        const int cls = S >> 3, st = S & 7;
        const int kz = 2 * (st >> 2) + 1 - (cls >> 2), ky = 2 * ((st >> 1) & 1) + 1 - ((cls >> 1) & 1), kx = 2 * (st & 1) + 1 - (cls & 1);
        const int t4 = (kz * 4 + ky) * 4 + kx;
        char* base = smem + HALO_BYTES + buf * BST;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = (wave * U + u) * 8 + (lane >> 3);
            const int lch = (lane & 7) ^ ((n >> 1) & 7);
            lds_dma16(p.w + (int64_t)n * p.kpad + t4 * CIN + lch * 8, base + (wave * U + u) * 1024);
        }
    };

    const int q = lane >> 4, n16 = lane & 15;
    float bv[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[i][r] = p.bias != nullptr ? p.bias[wn * 32 + i * 16 + q * 4 + r] : 0.f;
    halo_request(0);
    wait_vmcnt<0>();
    halo_store();
    stageW(0, 0);
    stageW(1, 1);
    stageW(2, 2);

    // voxel blocks of this wave: j -> local (z = 2 wm + (j >> 1), y = 2 (j & 1) + (n16 >> 3), x = n16 & 7); halo voxel of tap t = + t
    const int vx = n16 & 7, vyp = n16 >> 3;
    int vrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) vrow[j] = (((2 * wm + (j >> 1)) * HHY + 2 * (j & 1) + vyp) * HHX + vx) * P;
    int wrow[2], wsw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = wn * 32 + i * 16 + n16;
        wrow[i] = HALO_BYTES + n * P;
        wsw[i] = (n >> 1) & 7;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    wait_vmcnt<2 * U>();                          // stage 0 landed; stages 1, 2 in flight
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();

#pragma unroll 1
    for (int cls = 0; cls < 8; ++cls) {
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            const int S = cls * 8 + st;
            if (S + 1 < NSTG) {
                // publish stage S + 1: behind it stage S + 2 may stay in flight -- and, at a class's taps 1 and 2, the next class's eight halo loads,
                // issued behind stage S + 3 at tap 0
                if ((st == 1 || st == 2) && cls < 7) wait_vmcnt<U + HIT>();
                else if (S + 2 < NSTG) wait_vmcnt<U>();
                else wait_vmcnt<0>();
                wait_lgkm0();
                __builtin_amdgcn_s_barrier();
                if (S + 3 < NSTG) stageW(S + 3, (S + 3) & 3);
            }
            if (st == 0 && cls < 7) halo_request(cls + 1);
            const int voff = (((st >> 2) * HHY + ((st >> 1) & 1)) * HHX + (st & 1)) * P;
            const int sw = ((((vx + (st & 1)) >> 1) & 1) << 1) | (((vyp + ((st >> 1) & 1)) & 1) << 2);
            const char* wb = smem + (S & 3) * BST;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                half8 af[2], bf[4];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *(const half8*)(wb + wrow[i] + (((ks * 4 + q) ^ wsw[i]) << 4));
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = *(const half8*)(smem + vrow[j] + voff + (((ks * 4 + q) ^ sw) << 4));
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
        if (cls < 7) {
            // swap the halo: every wave has read the last tap's fragments; the next class's chunks landed long ago (tap 3's wait retired them)
            wait_lgkm0();
            __builtin_amdgcn_s_barrier();
            halo_store();
            wait_lgkm0();     // (published by the next tap's barrier)
        }
    }
    // epilogue: bias, ReLU, fp16; channel blocks 0 / 1 trade halves, lane group q stores 8 consecutive channels of block (q & 1) at offset 8 (q >> 1)
    const int OD = p.D >> 1, OH = p.H >> 1, OW = p.W >> 1;
    const float lo = p.relu ? 0.f : -65504.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned pk[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
            half2_t lo2, hi2;
            lo2[0] = (half_t)__builtin_amdgcn_fmed3f(acc[i][j][0] + bv[i][0], lo, 65504.f); lo2[1] = (half_t)__builtin_amdgcn_fmed3f(acc[i][j][1] + bv[i][1], lo, 65504.f);
            hi2[0] = (half_t)__builtin_amdgcn_fmed3f(acc[i][j][2] + bv[i][2], lo, 65504.f); hi2[1] = (half_t)__builtin_amdgcn_fmed3f(acc[i][j][3] + bv[i][3], lo, 65504.f);
            pk[i][0] = __builtin_bit_cast(unsigned, lo2);
            pk[i][1] = __builtin_bit_cast(unsigned, hi2);
        }
        const auto s0 = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
        const int z = 2 * wm + (j >> 1), y = 2 * (j & 1) + vyp;
        const int64_t orow = (((int64_t)b * OD + z0 + z) * OH + y0 + y) * OW + x0 + vx;
        *(u32x4*)(p.out + orow * COUT + wn * 32 + (q & 1) * 16 + (q >> 1) * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------
// k3 / s1 / p1, C_in = 64, with the WEIGHTS IN REGISTERS: conv3d_halo_kernel above reads, per 32-deep k step and wave, four voxel
// fragments and two weight fragments from LDS for eight MFMAs -- with eight waves per CU the LDS pipe is busy 384 cycles per 256 MFMA
// cycles, which caps the matrix pipe at two thirds (and it streams every tap's weights through an LDS ring behind a barrier per tap).
// Here a workgroup owns 4 x 8 x 8 output voxels (256 rows; halo 6 x 10 x 10 = 76.8 KB: two workgroups per CU, nothing else in LDS), a
// wave 128 voxels x 32 channels, and the weight fragments never touch LDS: they are stored once per model in MFMA-fragment order
// (pcd_conv3d_pack_wfrag: [tile][tap][channel half][k step][16-channel block][lane][8]) so that a wave's fragment is ONE coalesced
// 1-KB global load straight into the registers the MFMA reads, two taps ahead.  Per k step and wave: eight voxel fragment reads (LDS)
// + two weight loads (L1/L2: 32 B per cycle and CU, half the L1 rate) for 16 MFMAs -- the LDS pipe is busy 512 cycles per 512 MFMA
// cycles at two waves per SIMD -- and there is NO barrier after the halo is in place: the 27 taps are straight-line code that the
// compiler pipelines (counted vmcnt / lgkmcnt of its own).  Transposed product, 16-byte direct stores (+ residual), as convT3d_halo_kernel.
struct HaloWregParams {
    const half_t* in; int B, D, H, W;
    const half_t* in2; int cin2;      // optional second source (pcd_conv3d_desc_t.in2, 32 or 64 channels): one or two more 32-deep k steps behind the taps, its
                                      // voxel fragments straight from global memory (a lane's 16 bytes = 8 of a row's channels), its weights = the stage
                                      // behind the last tap's
    const half_t* wfrag;              // [tiles_n][27 SPT + 1 stages][NWC][KSS][2][64][8]: a stage = up to 64 channels of one tap (SPT per tap), + the second source's
    const float* bias;
    const half_t* resid;
    half_t* out; int Cout;
    int relu;
    int tiles_n, tz, ty, tx, nblocks;
};

// CIN = 64 or 32 (32: one k step per tap, 64-byte voxel rows, 38.4 KB of halo: four workgroups per CU); NWC = wave columns: a tile is 32 NWC channels
// wide and a workgroup NWR x NWC waves (C_out = 32 layers: NWC = 1).  CIN = 128: 256-byte voxel rows (the swizzle of convT3d_halo_kernel), a 153.6-KB halo
// = ONE workgroup per CU, so it runs eight waves (tiles of 128 channels, NWC = 4); a tap is then two weight stages of 64 channels.
// ABL: timing ablations of the <64, 2> instance (pcd_conv3d_config + 32768 x bits; OUTPUTS WRONG): 1 = the halo is not loaded (zeros are written to LDS), 2 = no halo staging
// at all, 4 = no taps (no fragment reads, no MFMAs, no weight loads)
template <int CIN, int NWC, int NWR = 2, int ABL = 0>
__global__ __launch_bounds__(64 * NWR * NWC, 2) void conv3d_halo_wreg_kernel(HaloWregParams p) {      // >= two waves per SIMD: at most 256 registers
    constexpr int P = CIN * 2, CPV = CIN / 8, NT = 64 * NWR * NWC, TY8 = 8, HHY8 = TY8 + 2, TC = 32 * NWC;
    constexpr int SPT = CIN > 64 ? CIN / 64 : 1, KSS = (CIN > 64 ? 64 : CIN) / 32, NSTG = 27 * SPT;      // weight stages per tap, k steps per stage, stages
    constexpr int NB = 16 / NWR;                               // 16-voxel blocks per wave: NWR = 2 wave rows of 128 voxels, or 4 of 64 (C_in 64 -> C_out 32: four waves)
    constexpr int HV = (HTZ + 2) * HHY8 * HHX;                 // 600 halo voxels
    constexpr int HIT = (HV * CPV + NT - 1) / NT;              // 16-byte chunks per thread
    static_assert(HIT <= 32, "one validity bit per chunk in a 32-bit mask");
    __shared__ __attribute__((aligned(16))) char smem[HV * P];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / NWC, wc = wave - wr * NWC;           // voxel rows wr * 16 NB .. of the 256, 32-channel column of the tile
    int bid = blockIdx.x;
    if ((p.nblocks & 7) == 0) bid = (bid & 7) * (p.nblocks >> 3) + (bid >> 3);
    const int tn = bid % p.tiles_n; int t = bid / p.tiles_n;
    const int tx = t % p.tx; t /= p.tx;
    const int ty = t % p.ty; t /= p.ty;
    const int tz = t % p.tz; const int b = t / p.tz;
    const int z0 = tz * HTZ, y0 = ty * TY8, x0 = tx * HTX;

    // ---- halo: global -> registers (all loads in flight) -> LDS, chunk c of voxel (hz, hy, hx) at slot c ^ s(hx, hy) (the C_in = 64 image above)
    if constexpr (!(ABL & 2)) {
        half8 hv[HIT];
        unsigned okmask = 0;
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int c = it * NT + tid;
            const int row = c / CPV, ch = c - row * CPV;
            const int hx = row % HHX; const int r2 = row / HHX;
            const int hy = r2 % HHY8, hz = r2 / HHY8;
            const int iz = z0 - 1 + hz, iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            const bool ok = row < HV && (unsigned)iz < (unsigned)p.D && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            okmask |= ok ? 1u << it : 0u;
            const int cz = min(max(iz, 0), p.D - 1), cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);
            if constexpr ((ABL & 1) != 0) hv[it] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            else hv[it] = *(const half8*)(p.in + ((((int64_t)b * p.D + cz) * p.H + cy) * p.W + cx) * CIN + ch * 8);
        }
#pragma unroll
        for (int it = 0; it < HIT; ++it) {
            const int c = it * NT + tid;
            const int row = c / CPV, ch = c - row * CPV;
            const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
            const int hx = row % HHX, hy = (row / HHX) % HHY8;
            const int sw = CIN == 128 ? (hx & 7) << 1 : (CIN == 64 ? (((hx >> 1) & 1) << 1) | ((hy & 1) << 2) : (hy & 1) << 1);
            if (row < HV) *(half8*)(smem + row * P + ((ch ^ sw) << 4)) = (okmask >> it) & 1 ? hv[it] : zero8;
        }
    }
    const int q = lane >> 4, n16 = lane & 15;
    // this wave's weight fragments: stage g, k step ks, channel block j at wf + (((g * NWC + wc) * KSS + ks) * 2 + j) * 512 halfs (+ lane * 8)
    const half_t* wf = p.wfrag + (int64_t)tn * (NSTG + 1) * NWC * KSS * 2 * 512 + lane * 8;
    float bv[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[j][r] = p.bias != nullptr ? p.bias[tn * TC + wc * 32 + j * 16 + q * 4 + r] : 0.f;
    // voxel blocks of this wave: block g = wr * NB + i -> local (z = g >> 2, y = 2 (g & 3) + (n16 >> 3), x = n16 & 7)
    const int vx = n16 & 7, vyp = n16 >> 3;
    int vrow[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) vrow[i] = ((((wr * NB + i) >> 2) * HHY8 + 2 * ((wr * NB + i) & 3) + vyp) * HHX + vx) * P;
    f32x4 acc[2][NB];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    half8 wq[3][KSS][2];                                       // weight fragments of stages g, g + 1, g + 2 (ring of three)
    auto wload = [&](int slot, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < KSS; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j) wq[slot][ks][j] = *(const half8*)(wf + (((g * NWC + wc) * KSS + ks) * 2 + j) * 512);
    };
    wload(0, 0);
    wload(1, 1);
    __syncthreads();                                           // the halo is in place; no barrier from here on

#pragma unroll
    for (int g = 0; g < ((ABL & 4) ? 0 : NSTG); ++g) {
        if (g + 2 < NSTG) wload((g + 2) % 3, g + 2);
        __builtin_amdgcn_sched_barrier(0);                     // the loads stay HERE, two stages ahead of their use (left alone the scheduler sinks them to it)
        const int tap = g / SPT, kh = g % SPT;                 // kh: which 64 channels of the tap
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const int voff = ((kz * HHY8 + ky) * HHX + kx) * P;
        const int sw = CIN == 128 ? ((vx + kx) & 7) << 1
                                  : (CIN == 64 ? ((((vx + kx) >> 1) & 1) << 1) | (((vyp + ky) & 1) << 2) : ((vyp + ky) & 1) << 1);
#pragma unroll
        for (int ks = 0; ks < KSS; ++ks) {
            half8 vf[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) vf[i] = *(const half8*)(smem + vrow[i] + voff + ((((kh * KSS + ks) * 4 + q) ^ sw) << 4));
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < NB; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[g % 3][ks][j], vf[i], acc[j][i], 0, 0, 0);
        }
    }
    if (CIN >= 64 && p.in2 != nullptr) {
        // the second source's k steps (cin2 / 32 of them): weights = the stage behind the last tap's, voxel fragments from global memory (row m of in2,
        // channels 32 ks + 8 q .. + 7)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (ks * 32 < p.cin2) {
                half8 w2[2], x2[NB];
#pragma unroll
                for (int j = 0; j < 2; ++j) w2[j] = *(const half8*)(wf + (((NSTG * NWC + wc) * KSS + ks) * 2 + j) * 512);
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const int z = (wr * NB + i) >> 2, y = 2 * ((wr * NB + i) & 3) + vyp;
                    x2[i] = *(const half8*)(p.in2 + ((((int64_t)b * p.D + z0 + z) * p.H + y0 + y) * p.W + x0 + vx) * p.cin2 + ks * 32 + q * 8);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < NB; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2[j], x2[i], acc[j][i], 0, 0, 0);
            }
        }
    }
    // epilogue: bias -> fp16 (the rounding point of the other kernels) (+ residual) (+ ReLU); channel blocks 0 / 1 trade halves, lane group q stores
    // 8 consecutive channels of block (q & 1) at offset 8 (q >> 1)
    const float lo = (p.relu && p.resid == nullptr) ? 0.f : -65504.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        unsigned pk[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
            half2_t lo2, hi2;
            lo2[0] = (half_t)__builtin_amdgcn_fmed3f(acc[j][i][0] + bv[j][0], lo, 65504.f); lo2[1] = (half_t)__builtin_amdgcn_fmed3f(acc[j][i][1] + bv[j][1], lo, 65504.f);
            hi2[0] = (half_t)__builtin_amdgcn_fmed3f(acc[j][i][2] + bv[j][2], lo, 65504.f); hi2[1] = (half_t)__builtin_amdgcn_fmed3f(acc[j][i][3] + bv[j][3], lo, 65504.f);
            pk[j][0] = __builtin_bit_cast(unsigned, lo2);
            pk[j][1] = __builtin_bit_cast(unsigned, hi2);
        }
        const auto s0 = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
        const int z = (wr * NB + i) >> 2, y = 2 * ((wr * NB + i) & 3) + vyp;
        const int64_t orow = (((int64_t)b * p.D + z0 + z) * p.H + y0 + y) * p.W + x0 + vx;
        const int col = tn * TC + wc * 32 + (q & 1) * 16 + (q >> 1) * 8;
        if (p.resid != nullptr) {
            half8 ov = __builtin_bit_cast(half8, o);
            const half8 rs = *(const half8*)(p.resid + orow * p.Cout + col);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float f = (float)ov[e] + (float)rs[e];
                if (p.relu) f = fmaxf(f, 0.f);
                ov[e] = to_half_sat(f);
            }
            o = __builtin_bit_cast(u32x4, ov);
        }
        *(u32x4*)(p.out + orow * p.Cout + col) = o;
    }
}

// one thread per 16-byte fragment piece: out[tile][stage][wc][ks][j][lane][8] = w[tile * tc + wc * 32 + j * 16 + (lane & 15)][k ..], k = tap * cin + kh * 64 + ks * 32 +
// (lane >> 4) * 8 for stage = tap * spt + kh (spt = stages per tap: cin / 64, or 1); the LAST stage = the cin2 weight columns of a second source behind the 27 taps
__global__ __launch_bounds__(256) void conv3d_pack_wfrag_kernel(const half_t* __restrict__ w, int kpad, int cin, int cout, int cin2, int nwc, half_t* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int spt = cin > 64 ? cin / 64 : 1, kss = (cin > 64 ? 64 : cin) / 32, nstg = 27 * spt + 1, tc = 32 * nwc;
    const int total = (cout / tc) * nstg * nwc * kss * 2 * 64;
    if (idx >= total) return;
    const int lane = idx & 63; int r = idx >> 6;
    const int j = r & 1; r >>= 1;
    const int ks = r % kss; r /= kss;
    const int wc = r % nwc; r /= nwc;
    const int g = r % nstg; const int tile = r / nstg;
    const int n = tile * tc + wc * 32 + j * 16 + (lane & 15);
    const int kk = ks * 32 + (lane >> 4) * 8;
    const bool extra = g == nstg - 1;
    const int k = extra ? 27 * cin + kk : (g / spt) * cin + (g % spt) * 64 + kk;
    const bool real = !extra || kk + 8 <= cin2;
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    *(half8*)(out + (int64_t)idx * 8) = (real && k + 8 <= kpad) ? *(const half8*)(w + (int64_t)n * kpad + k) : zero8;
}

// tiles per dimension -> the parameter struct's tz, ty, tx and nblocks (the launch's workgroup count, which the kernels index in 32 bits)
template <class P>
static int halo_grid(P& p, int batch, int tz, int ty, int tx, int tiles_n = 1) {
    p.tz = tz; p.ty = ty; p.tx = tx;
    const int64_t blocks = (int64_t)batch * tz * ty * tx * tiles_n;
    PCD_CHECK_ARG(blocks <= 0x7fffffff);
    p.nblocks = (int)blocks;
    return PCD_OK;
}

// k3 / stride 1 / pad 1 on the input's own grid, whole 4 x ty x 8 blocks, no output offset: what both stride-1 halo forms need
static bool halo_grid_ok(const pcd_conv3d_desc_t* d, int ty) {
    return d->ntaps == 27 && d->stride == 1 && d->out_scale == 1 &&
           d->rows_d == d->in_d && d->rows_h == d->in_h && d->rows_w == d->in_w && d->out_d == d->in_d &&
           d->out_h == d->in_h && d->out_w == d->in_w && d->in_d % HTZ == 0 && d->in_h % ty == 0 &&
           d->in_w % HTX == 0 && d->out_off_z == 0 && d->out_off_y == 0 && d->out_off_x == 0;
}

static bool halo_supported(const pcd_conv3d_desc_t* d) {
    return halo_grid_ok(d, HTY) && (d->cin == 32 || d->cin == 64) && d->cout % 8 == 0 && d->kpad >= 27 * d->cin &&
           (d->in2 == nullptr || (d->cin == 64 && d->cout % 64 == 0 && d->cin2 == 32));
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_conv3d_k3s1_supported(const pcd_conv3d_desc_t* d) { return d != nullptr && conv_check(d) == PCD_OK && halo_supported(d) ? 1 : 0; }

extern "C" int pcd_conv3d_k3s1_f16(const pcd_conv3d_desc_t* d, void* stream) {
    PCD_CHECK_ARG(d != nullptr);
    int rc;
    PCD_RUN(conv_check(d));
    PCD_CHECK_ARG(halo_supported(d));
    HaloParams p{};
    p.in = (const half_t*)d->in; p.B = d->batch; p.D = d->in_d; p.H = d->in_h; p.W = d->in_w;
    p.w = (const half_t*)d->w; p.kpad = d->kpad; p.bias = d->bias; p.resid = (const half_t*)d->resid;
    p.out = (half_t*)d->out; p.Cout = d->cout; p.relu = d->relu;
    p.in2 = (const half_t*)d->in2;
    const int bn = d->cout <= 32 ? 32 : 64;
    p.tiles_n = (int)ceil_div(d->cout, bn);
    // 32 -> 32: 256-row workgroups (4 x 8 x 8 voxels, eight waves) where they still give every CU two rounds of work
    const int64_t blocks256 = (int64_t)d->batch * (d->in_d / HTZ) * (d->in_h / 8) * (d->in_w / HTX) * p.tiles_n;
    const bool tall = d->cin == 32 && bn == 32 && d->in_h % 8 == 0 &&
                      (g_conv3d.halo_tall == 2 || (g_conv3d.halo_tall == 1 && blocks256 >= 512));
    PCD_RUN(halo_grid(p, d->batch, d->in_d / HTZ, d->in_h / (tall ? 8 : HTY), d->in_w / HTX, p.tiles_n));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nblocks), blk(tall ? 512 : 256);
    // weight stage = one tap (three taps for 32 -> 32, where a tap is only 4 MFMAs per wave); 4 waves: the
    // 2-wave / 64 x 64 wave-tile form (fewer LDS reads per MFMA, but one wave per SIMD) measured 345 vs 304 us
    if (tall) hipLaunchKernelGGL((conv3d_halo_kernel<32, 32, 3, 4, 8, 8>), grid, blk, 0, s, p);
    else if (d->in2 != nullptr) hipLaunchKernelGGL((conv3d_halo_kernel<64, 64, 1, 4, 4, 4, 32>), grid, blk, 0, s, p);
    else if (d->cin == 64 && bn == 64) hipLaunchKernelGGL((conv3d_halo_kernel<64, 64, 1, 4, 4>), grid, blk, 0, s, p);
    else if (d->cin == 64) hipLaunchKernelGGL((conv3d_halo_kernel<64, 32, 1, 4, 4>), grid, blk, 0, s, p);
    else if (bn == 64) hipLaunchKernelGGL((conv3d_halo_kernel<32, 64, 1, 4, 4>), grid, blk, 0, s, p);
    else hipLaunchKernelGGL((conv3d_halo_kernel<32, 32, 3, 4, 4>), grid, blk, 0, s, p);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

// wave columns of a tile: C_out = 32 layers run 32-wide tiles, C_in = 128 layers 128-wide tiles on eight waves, everything else 64-wide tiles on four
static int wreg_nwc(int cin, int cout) { return cin == 128 ? 4 : (cout == 32 ? 1 : 2); }
static bool wreg_shape_ok(int cin, int cout) {
    return cout > 0 && (((cin == 64 || cin == 32) && (cout == 32 || cout % 64 == 0)) || (cin == 128 && cout % 128 == 0));
}
static int wreg_stages(int cin) { return 27 * (cin > 64 ? cin / 64 : 1) + 1; }

extern "C" size_t pcd_conv3d_wfrag_bytes(int cin, int cout) {
    return wreg_shape_ok(cin, cout) ? (size_t)wreg_stages(cin) * (cin > 64 ? 64 : cin) * cout * sizeof(half_t) : 0;
}

extern "C" int pcd_conv3d_pack_wfrag(const void* w, int kpad, int cin, int cout, int cin2, void* wfrag, void* stream) {
    PCD_CHECK_ARG(w && wfrag && wreg_shape_ok(cin, cout) && (cin2 == 0 || (cin >= 64 && (cin2 == 32 || cin2 == 64))));
    PCD_CHECK_ARG(kpad >= 27 * cin + cin2 && kpad % 8 == 0);
    const int nwc = wreg_nwc(cin, cout);
    const int total = (cout / (32 * nwc)) * wreg_stages(cin) * nwc * ((cin > 64 ? 64 : cin) / 32) * 2 * 64;
    hipLaunchKernelGGL(conv3d_pack_wfrag_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, (const half_t*)w, kpad, cin, cout,
                       cin2, nwc, (half_t*)wfrag);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

static bool wreg_supported(const pcd_conv3d_desc_t* d) {
    return halo_grid_ok(d, 8) && wreg_shape_ok(d->cin, d->cout) &&
           (d->in2 == nullptr || (d->cin >= 64 && (d->cin2 == 32 || d->cin2 == 64)));
}

extern "C" int pcd_conv3d_k3s1_wreg_supported(const pcd_conv3d_desc_t* d) { return d != nullptr && conv_check(d) == PCD_OK && wreg_supported(d) ? 1 : 0; }

extern "C" int pcd_conv3d_k3s1_wreg_f16(const pcd_conv3d_desc_t* d, const void* wfrag, void* stream) {
    PCD_CHECK_ARG(d != nullptr && wfrag != nullptr);
    int rc;
    PCD_RUN(conv_check(d));
    PCD_CHECK_ARG(wreg_supported(d));
    HaloWregParams p{};
    p.in = (const half_t*)d->in; p.B = d->batch; p.D = d->in_d; p.H = d->in_h; p.W = d->in_w;
    p.in2 = (const half_t*)d->in2; p.cin2 = d->in2 ? d->cin2 : 0;
    p.wfrag = (const half_t*)wfrag; p.bias = d->bias; p.resid = (const half_t*)d->resid;
    p.out = (half_t*)d->out; p.Cout = d->cout; p.relu = d->relu;
    const int nwc = wreg_nwc(d->cin, d->cout);
    p.tiles_n = d->cout / (32 * nwc);
    PCD_RUN(halo_grid(p, d->batch, d->in_d / HTZ, d->in_h / 8, d->in_w / HTX, p.tiles_n));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nblocks);
    if (d->cin == 128) hipLaunchKernelGGL((conv3d_halo_wreg_kernel<128, 4>), grid, dim3(512), 0, s, p);              // eight waves, one workgroup per CU
    else if (d->cin == 64 && nwc == 2)
        dispatch_int<0, 1, 2, 4, 6>(g_conv3d.wreg_abl, [&](auto abl) {
            hipLaunchKernelGGL((conv3d_halo_wreg_kernel<64, 2, 2, decltype(abl)::value>), grid, dim3(256), 0, s, p);
        });
    else if (d->cin == 64) hipLaunchKernelGGL((conv3d_halo_wreg_kernel<64, 1, 4>), grid, dim3(256), 0, s, p);     // C_out 32: four waves of 64 voxels
    else if (nwc == 2) hipLaunchKernelGGL((conv3d_halo_wreg_kernel<32, 2>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((conv3d_halo_wreg_kernel<32, 1>), grid, dim3(128), 0, s, p);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_conv3d_k4s2_halo_supported(int batch, int d, int h, int w, int cin, int cout, int kpad) {
    return batch > 0 && cin == 64 && cout == 64 && kpad >= 64 * 64 && kpad % 8 == 0 && d > 0 && h > 0 && w > 0 && d % (2 * HTZ) == 0 &&
           h % (2 * HTY) == 0 && w % (2 * HTX) == 0 && d <= 64 && h <= 64 && w <= 64 && ((int64_t)batch + 1) * d * h * w * cin <= 0x7fffffff ? 1 : 0;      // (+ 1: the kernel forms offsets one plane past the end)
}

extern "C" int pcd_conv3d_k4s2_halo_f16(const void* in, int batch, int d, int h, int w, int cin, const void* wgt, int kpad, const float* bias,
                                        int relu, int cout, void* out, void* stream) {
    PCD_CHECK_ARG(in && wgt && out);
    PCD_CHECK_ARG(pcd_conv3d_k4s2_halo_supported(batch, d, h, w, cin, cout, kpad));
    ConvS2HaloParams p{};
    p.in = (const half_t*)in; p.B = batch; p.D = d; p.H = h; p.W = w;
    p.w = (const half_t*)wgt; p.kpad = kpad; p.bias = bias; p.out = (half_t*)out; p.relu = relu;
    int rc;
    PCD_RUN(halo_grid(p, batch, d / 2 / HTZ, h / 2 / HTY, w / 2 / HTX));
    hipLaunchKernelGGL(conv3d_k4s2_halo_kernel, dim3((unsigned)p.nblocks), dim3(256), 0, (hipStream_t)stream, p);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" int pcd_convt3d_k4s2_halo_supported(int batch, int d, int h, int w, int cin, int cout) {
    return batch > 0 && cin == 128 && cout == 64 && d > 0 && h > 0 && w > 0 && d % HTZ == 0 && h % HTY == 0 && w % HTX == 0 &&
           (int64_t)batch * d * h * w * 8 * cout <= 0x7fffffff ? 1 : 0;
}

extern "C" int pcd_convt3d_k4s2_halo_f16(const void* in, int batch, int d, int h, int w, int cin, const void* const* w8, const float* bias,
                                         int cout, void* out, void* stream) {
    PCD_CHECK_ARG(in && w8 && out);
    PCD_CHECK_ARG(pcd_convt3d_k4s2_halo_supported(batch, d, h, w, cin, cout));
    ConvTHaloParams p{};
    p.in = (const half_t*)in; p.B = batch; p.D = d; p.H = h; p.W = w;
    for (int k = 0; k < 8; ++k) {
        PCD_CHECK_ARG(w8[k] != nullptr);
        p.w[k] = (const half_t*)w8[k];
    }
    p.bias = bias; p.out = (half_t*)out;
    int rc;
    PCD_RUN(halo_grid(p, batch, d / HTZ, h / HTY, w / HTX));
    hipLaunchKernelGGL(convT3d_halo_kernel, dim3((unsigned)p.nblocks), dim3(512), 0, (hipStream_t)stream, p);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
