// K9: 3-D convolutions of VAE3DLarge (reference networks.py:2225-2264, 471-504) as implicit GEMM
// on MFMA.  Activations are NDHWC fp16, so the Cin channels of one input voxel are contiguous
// and an im2col row is a list of (tap, voxel) segments: the A-tile loader below gathers those
// segments with the same 16-B global_load_lds + source-side XOR swizzle as the dense GEMM
// (csrc/gemm_f16.hip); out-of-range taps (padding, K padding) read from a zero page.
// Conv3d (any k/stride/pad) and each output-parity class of ConvTranspose3d(k4,s2,p1) are the
// same kernel with different tap tables and output row maps.  Eval-mode BatchNorm3d is folded
// into W/bias on the host; epilogue = bias (+ residual) (+ ReLU).
// The LDS-halo forms of the same layers: csrc/conv3d_halo.hip; the first and the last layer (not GEMM shaped): csrc/conv3d_ends.hip.
#include "conv3d.h"

namespace pcd {

// what differs between the problems of one launch (blockIdx.y): tap table, weights, output parity
struct ConvVariant {
    const int* taps;                  // device [ntaps] packed (dz & 0xff) | (dy & 0xff) << 8 | (dx & 0xff) << 16
    const half_t* w;                  // [Cout][kpad]
    int pz, py, px, pad_;
};

struct ConvParams {
    const half_t* in; int D, H, W, Cin, cin_shift;
    int Do, Ho, Wo, stride;           // row space: m = ((b*Do+oz)*Ho+oy)*Wo+ox ; input coord = o*stride + d
    int ntaps, kpad;
    const float* bias;
    const half_t* resid;              // optional, indexed like out
    half_t* out; int Cout;
    int OD, OH, OW, os;               // output voxel = (oz*os+pz, oy*os+py, ox*os+px) in an OD x OH x OW grid
    int relu;
    int M;
    const half_t* zero;               // >= 128 B of zeros
    int tiles_n;
    int splits;                       // split-K (blockIdx.z); > 1 -> fp32 partials into slabs, conv3d_finish_kernel
    float* slabs;                     // [splits][nvar][M][Cout]
    int nvar;
    const half_t* in2;                // optional second source on the row grid (pcd_conv3d_desc_t.in2): K tiles kt >= kt2 read it
    int cin2_shift, kt2;              // log2(cin2); first K tile of the second source (INT_MAX without one)
    ConvVariant var[MAX_VARIANTS];
};

// K tile BKT (64 or 32 halfs: 128- or 64-byte LDS rows) in a ring of NST stages.  A stage is requested NST - 1 K tiles before
// the barrier that publishes it and NST - 2 younger stages stay in flight behind that barrier's counted vmcnt: with two
// stages the gather of K tile kt+1 has one K tile of MFMAs (~500 cycles per wave) to come back from L2, and the waves
// spend more than half their time at the wait (SQ_WAIT_ANY 56 % of SQ_WAVE_CYCLES on the 128 -> 128 layers).
// ABL: timing ablations (pcd_conv3d_config + 1024 x bits; OUTPUTS WRONG): 1 = the weight rows are staged for the first NST - 1 K tiles only, 2 = the same for the gathered rows,
// 4 = every fragment read takes the first fragment's address, 8 = no MFMAs
template <int BM, int BN, int BKT, int NST, int ABL = 0>
__global__ __launch_bounds__(256) void conv3d_igemm_kernel(ConvParams p) {
    constexpr int CBK = BKT, CROWB = BKT * 2;                 // shadow the file-level K tile
    constexpr int LPR = BKT / 8, RPW = 64 / LPR, RPI = 4 * RPW;   // lanes per staged row, rows per wave instruction / per round
    constexpr int KS = BKT / 32;
    constexpr int WM = BM / 2, WN = BN / 2, MI = WM / 16, NI = WN / 16;
    constexpr int STAGE_BYTES = (BM + BN) * CROWB;
    constexpr int OUT_LD = BN * 2 + 16;
    constexpr int LDS_BYTES = (NST * STAGE_BYTES > BM * OUT_LD) ? NST * STAGE_BYTES : BM * OUT_LD;
    constexpr int AR = BM / RPI, BR = BN / RPI, LPT = AR + BR;  // LPT: LDS-DMA instructions per thread and stage
    static_assert(ABL == 0 || NST == 2, "the ablations drop LDS-DMA instructions: only the two-stage form, whose waits are vmcnt(0)");
    static_assert(BM % RPI == 0 && BN % RPI == 0 && NST >= 2 && NST <= 4, "stage layout");
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    __shared__ int4 taps_s[TAP_SLOTS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // consecutive workgroups go round-robin over the 8 XCDs: give each XCD a contiguous run of row tiles, so that the
    // tiles that gather the same input voxels (neighbouring output rows, all 27 taps) meet in one L2
    int bid = blockIdx.x;
    if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
    const int tm = bid / p.tiles_n, tn = bid - tm * p.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nk_all = p.kpad / BKT;
    const int cls = blockIdx.y, sp = blockIdx.z;
    const int kt0 = (int)((int64_t)sp * nk_all / p.splits), kt1 = (int)((int64_t)(sp + 1) * nk_all / p.splits);
    const ConvVariant& cv = p.var[cls];
    const half_t* __restrict__ wgt = cv.w;
    // Tap table -> LDS once, in the form the gather wants (the address arithmetic of a K tile is what bounds this
    // kernel's issue slots, not the MFMAs): x, y = the tap's (dz, dy, dx) as three biased byte fields, +64 + d and
    // 64 - d; z = its offset in elements of the NDHWC input.  A row keeps (z, y, x) + 64 and (D-1-z, H-1-y, W-1-x) + 64
    // in the same byte fields, so "input voxel inside the grid" is: bit 7 of every field of both sums set -- two
    // adds, two ands and one compare for all six bounds (dims <= 64, |d| < 64: no carry between fields).  Slots past
    // ntaps (K padding) hold 0 and fail that test.
    if (tid < TAP_SLOTS) {
        int4 e = {0, 0, 0, 0};
        if (tid < p.ntaps) {
            const int pk = cv.taps[tid];
            const int dz = (int)(signed char)(pk & 0xff), dy = (int)(signed char)((pk >> 8) & 0xff),
                      dx = (int)(signed char)((pk >> 16) & 0xff);
            e.x = (dz + 64) | (dy + 64) << 8 | (dx + 64) << 16;
            e.y = (64 - dz) | (64 - dy) << 8 | (64 - dx) << 16;
            e.z = ((dz * p.H + dy) * p.W + dx) * p.Cin;
        }
        taps_s[tid] = e;
    }
    __syncthreads();

    // the rows this thread stages (fixed for the whole K loop): decode the output voxel once
    const int srow = wave * RPW + lane / LPR;                // + r*RPI
    // logical 16-B chunk (same for every r): the XOR swizzles of gemm_f16.hip for 128- and 64-byte rows
    const int lchunk = (lane % LPR) ^ (BKT == 64 ? (srow >> 1) & 7 : (-(srow >> 2)) & 3);
    int rp1[AR], rp2[AR], rbase[AR];
#pragma unroll
    for (int r = 0; r < AR; ++r) {
        int m = m0 + r * RPI + srow;
        m = m < p.M ? m : p.M - 1;
        const int ox = m % p.Wo; int t = m / p.Wo;
        const int oy = t % p.Ho; t /= p.Ho;
        const int oz = t % p.Do;
        const int b = t / p.Do;
        const int rz = oz * p.stride, ry = oy * p.stride, rx = ox * p.stride;
        rp1[r] = (rz + 64) | (ry + 64) << 8 | (rx + 64) << 16;
        rp2[r] = (p.D - 1 - rz + 64) | (p.H - 1 - ry + 64) << 8 | (p.W - 1 - rx + 64) << 16;
        rbase[r] = (((b * p.D + rz) * p.H + ry) * p.W + rx) * p.Cin;
    }
    const half_t* wrow[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) {
        int n = n0 + r * RPI + srow;
        n = n < p.Cout ? n : p.Cout - 1;
        wrow[r] = wgt + (int64_t)n * p.kpad;
    }
    const half_t* zlane = p.zero + (lane % LPR) * 8;

    // LDS-DMA from asm (the compiler would serialise every later wait behind the builtin form); the K loop owns vmcnt
    auto stage = [&](int kt, int buf) {
        char* base = smem + buf * STAGE_BYTES;
        const int kidx = kt * CBK + lchunk * 8;
        const bool first = kt < kt0 + NST - 1;
        if ((ABL & 2) && !first) {
        } else
        if (kt >= p.kt2) {
            // second source (uniform per K tile): row m of in2, channels kidx - kt2 * CBK .. ; the row grid IS in2's grid (stride 1), so its
            // voxel index is rbase / Cin and no bound can fail
            const int c2 = kidx - p.kt2 * CBK;
#pragma unroll
            for (int r = 0; r < AR; ++r)
                lds_dma16(p.in2 + (((rbase[r] >> p.cin_shift) << p.cin2_shift) + c2), base + (r * RPI + wave * RPW) * CROWB);
        } else {
            const int4 te = taps_s[kidx >> p.cin_shift];
            const int dc = te.z + (kidx & (p.Cin - 1));
#pragma unroll
            for (int r = 0; r < AR; ++r) {
                const bool ok = (((rp1[r] + te.x) & (rp2[r] + te.y)) & 0x808080) == 0x808080;
                const half_t* g = p.in + (rbase[r] + dc);
                g = ok ? g : zlane;
                lds_dma16(g, base + (r * RPI + wave * RPW) * CROWB);
            }
        }
        if ((ABL & 1) && !first) return;
#pragma unroll
        for (int r = 0; r < BR; ++r) lds_dma16(wrow[r] + kidx, base + BM * CROWB + (r * RPI + wave * RPW) * CROWB);
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int ra = wm * WM + (lane & 15), rbw = wn * WN + (lane & 15);
    const int swa = BKT == 64 ? (ra >> 1) & 7 : (-(ra >> 2)) & 3, swb = BKT == 64 ? (rbw >> 1) & 7 : (-(rbw >> 2)) & 3;
    const int q = lane >> 4;
    int offa[KS], offb[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        offa[ks] = ra * CROWB + (((ks * 4 + q) ^ swa) << 4);
        offb[ks] = BM * CROWB + rbw * CROWB + (((ks * 4 + q) ^ swb) << 4);
    }

#pragma unroll
    for (int t = 0; t < NST - 1; ++t)
        if (kt0 + t < kt1) stage(kt0 + t, t);
    int buf = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        // stage kt must have landed; up to NST - 2 younger stages stay in flight
        const int younger = min(NST - 2, kt1 - 1 - kt);
        if (NST >= 4 && younger == 2) wait_vmcnt<2 * LPT>();
        else if (NST >= 3 && younger == 1) wait_vmcnt<LPT>();
        else wait_vmcnt<0>();
        wait_lgkm0();
        __builtin_amdgcn_s_barrier();      // every wave's share of K tile kt is in LDS; the buffer of K tile kt-1 is free
        if (kt + NST - 1 < kt1) {
            int nb = buf + NST - 1;
            nb = nb >= NST ? nb - NST : nb;
            stage(kt + NST - 1, nb);
        }
        const char* base = smem + buf * STAGE_BYTES;
        buf = buf + 1 == NST ? 0 : buf + 1;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            half8 af[MI], bf[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *(const half8*)(base + offa[ks] + ((ABL & 4) ? 0 : i * 16 * CROWB));
#pragma unroll
            for (int j = 0; j < NI; ++j) bf[j] = *(const half8*)(base + offb[ks] + ((ABL & 4) ? 0 : j * 16 * CROWB));
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    if constexpr ((ABL & 8) != 0) acc[i][j][0] += (float)af[i][0] * (float)bf[j][0];
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
                }
        }
    }

    // epilogue: bias -> LDS (fp16) -> row-contiguous 16-B stores (+ residual, ReLU) through the row map
    const int colq = lane & 15;
    if (p.splits > 1) {
        // split-K partial: raw fp32 accumulators to this split's slab; bias/residual/ReLU/row map in the finish
        float* slab = p.slabs + ((int64_t)sp * p.nvar + cls) * p.M * p.Cout;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int col = n0 + wn * WN + j * 16 + colq;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm * WM + i * 16 + q * 4 + r;
                    if (m < p.M && col < p.Cout) slab[(int64_t)m * p.Cout + col] = acc[i][j][r];
                }
        }
        return;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int lcol = wn * WN + j * 16 + colq;
        const float bc = (p.bias != nullptr && n0 + lcol < p.Cout) ? p.bias[n0 + lcol] : 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lrow = wm * WM + i * 16 + q * 4 + r;
                float v = acc[i][j][r] + bc;
                if (p.relu && p.resid == nullptr) v = fmaxf(v, 0.f);
                *(half_t*)(smem + lrow * OUT_LD + lcol * 2) = to_half_sat(v);
            }
    }
    __syncthreads();
    constexpr int CPR = BN / 8, TOTAL = BM * CPR;
#pragma unroll
    for (int it = 0; it < TOTAL / 256; ++it) {
        const int idx = it * 256 + tid;
        const int lrow = idx / CPR, ch = idx - lrow * CPR;
        const int m = m0 + lrow, col = n0 + ch * 8;
        if (m < p.M && col < p.Cout) {
            const int ox = m % p.Wo; int t = m / p.Wo;
            const int oy = t % p.Ho; t /= p.Ho;
            const int oz = t % p.Do; const int b = t / p.Do;
            const int64_t orow = (((int64_t)b * p.OD + oz * p.os + cv.pz) * p.OH + oy * p.os + cv.py) * p.OW +
                                 ox * p.os + cv.px;
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

// split-K finish: sum the slabs in split order (deterministic), then the same epilogue as above.
// thread = (variant, row, 8-column chunk)
__global__ __launch_bounds__(256) void conv3d_finish_kernel(ConvParams p) {
    // grid = (chunks of a variant, variant): 32-bit index arithmetic (64-bit divisions by run-time values were most of this kernel)
    const unsigned cpr = (unsigned)p.Cout / 8;
    const unsigned rem = blockIdx.x * blockDim.x + threadIdx.x;
    if (rem >= (unsigned)p.M * cpr) return;
    const int cls = blockIdx.y;
    const int m = (int)(rem / cpr), col = (int)(rem - (unsigned)m * cpr) * 8;
    const ConvVariant& cv = p.var[cls];
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    // slabs added in split order (deterministic), eight splits' loads in flight together: the small-grid layers that
    // split K deepest (up to 64 ways) have the fewest threads here, so this loop is pure load latency
    const int64_t sstride = (int64_t)p.nvar * p.M * p.Cout;
    const float* sp = p.slabs + ((int64_t)cls * p.M + m) * p.Cout + col;
    constexpr int FL = 8;
    for (int s = 0; s < p.splits; s += FL) {
        float4 u[FL], v[FL];
#pragma unroll
        for (int j = 0; j < FL; ++j) {
            const int sj = s + j < p.splits ? s + j : s;
            const float4* q = (const float4*)(sp + (int64_t)sj * sstride);
            u[j] = q[0]; v[j] = q[1];
        }
#pragma unroll
        for (int j = 0; j < FL; ++j)
            if (s + j < p.splits) {
                a[0] += u[j].x; a[1] += u[j].y; a[2] += u[j].z; a[3] += u[j].w;
                a[4] += v[j].x; a[5] += v[j].y; a[6] += v[j].z; a[7] += v[j].w;
            }
    }
    const int ox = m % p.Wo; int t = m / p.Wo;
    const int oy = t % p.Ho; t /= p.Ho;
    const int oz = t % p.Do; const int b = t / p.Do;
    const int64_t orow = (((int64_t)b * p.OD + oz * p.os + cv.pz) * p.OH + oy * p.os + cv.py) * p.OW + ox * p.os + cv.px;
    half8 o;
    float bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = 0.f;
    if (p.bias != nullptr) {
        const f32x4 b0 = *(const f32x4*)(p.bias + col), b1 = *(const f32x4*)(p.bias + col + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bv[e] = b0[e]; bv[4 + e] = b1[e]; }
    }
    if (p.resid != nullptr) {
        const half8 rs = *(const half8*)(p.resid + orow * p.Cout + col);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            // same rounding points as the unsplit epilogue: fp16(acc + bias), then + residual in fp32
            float f = (float)to_half_sat(a[e] + bv[e]) + (float)rs[e];
            if (p.relu) f = fmaxf(f, 0.f);
            o[e] = to_half_sat(f);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float f = a[e] + bv[e];
            if (p.relu) f = fmaxf(f, 0.f);
            o[e] = to_half_sat(f);
        }
    }
    *(half8*)(p.out + orow * p.Cout + col) = o;
}

Conv3dConfig g_conv3d;            // (hidden: declared PCD_INTERNAL in conv3d.h)

// split-K factor for a launch of `blocks` workgroups over `nk` K tiles: aim for ~2 workgroups per CU
static int conv_splits(int64_t blocks, int nk) {
    if (blocks >= g_conv3d.split_target || nk < 8) return 1;
    int s = (int)ceil_div((int64_t)g_conv3d.split_target, blocks);
    s = s < nk / 4 ? s : nk / 4;
    s = s < 64 ? s : 64;
    return s < 1 ? 1 : s;
}

int conv_check(const pcd_conv3d_desc_t* d) {
    PCD_CHECK_ARG(d->in && d->w && d->out && d->taps && d->zero_page);
    PCD_CHECK_ARG(d->batch > 0 && d->in_d > 0 && d->in_h > 0 && d->in_w > 0);
    PCD_CHECK_ARG(d->cin >= 8 && (d->cin & (d->cin - 1)) == 0);
    PCD_CHECK_ARG(d->cout > 0 && d->cout % 8 == 0);
    PCD_CHECK_ARG(d->ntaps > 0 && d->ntaps <= MAX_TAPS && d->kpad % CBK == 0 && d->kpad >= d->ntaps * d->cin);
    PCD_CHECK_ARG(d->kpad / d->cin <= TAP_SLOTS);
    // the gather tests all six grid bounds in packed byte fields (conv3d_igemm_kernel): coordinates below 64
    PCD_CHECK_ARG(d->in_d <= 64 && d->in_h <= 64 && d->in_w <= 64);
    PCD_CHECK_ARG((d->rows_d - 1) * d->stride < 64 && (d->rows_h - 1) * d->stride < 64 && (d->rows_w - 1) * d->stride < 64);
    PCD_CHECK_ARG((int64_t)d->batch * d->in_d * d->in_h * d->in_w * d->cin <= 0x7fffffff);
    PCD_CHECK_ARG(d->rows_d > 0 && d->rows_h > 0 && d->rows_w > 0 && d->stride > 0);
    PCD_CHECK_ARG(d->out_scale > 0 && d->out_d > 0 && d->out_h > 0 && d->out_w > 0);
    PCD_CHECK_ARG((int64_t)d->batch * d->rows_d * d->rows_h * d->rows_w <= 0x7fffffff);
    if (d->in2 != nullptr) {
        // second source: the row grid is its grid, its K columns start on a K-tile boundary behind the taps
        PCD_CHECK_ARG(d->cin2 >= 32 && (d->cin2 & (d->cin2 - 1)) == 0 && d->resid == nullptr);
        PCD_CHECK_ARG(d->stride == 1 && d->out_scale == 1 && d->rows_d == d->in_d && d->rows_h == d->in_h && d->rows_w == d->in_w);
        PCD_CHECK_ARG((d->ntaps * d->cin) % CBK == 0 && d->kpad >= d->ntaps * d->cin + d->cin2);
        PCD_CHECK_ARG((int64_t)d->batch * d->in_d * d->in_h * d->in_w * d->cin2 <= 0x7fffffff);
    }
    return PCD_OK;
}

// rows, column tiles and split-K factor of a launch of n variants; returns the bytes of its split-K slabs (0 when unsplit)
static size_t conv_shape(const pcd_conv3d_desc_t* d, int n, int64_t* m, int* tiles_n, int* splits) {
    *m = (int64_t)d->batch * d->rows_d * d->rows_h * d->rows_w;
    *tiles_n = (int)ceil_div(d->cout, d->cout <= 64 ? 64 : 128);
    *splits = conv_splits(ceil_div(*m, 128) * *tiles_n * n, d->kpad / CBK);
    return *splits > 1 ? (size_t)*splits * n * *m * d->cout * sizeof(float) : 0;
}

}  // namespace pcd

using namespace pcd;

extern "C" size_t pcd_conv3d_workspace_bytes(const pcd_conv3d_desc_t* d, int n) {
    if (d == nullptr || n < 1 || n > MAX_VARIANTS || conv_check(d) != PCD_OK) return 0;
    int64_t m; int tiles_n, splits;
    return conv_shape(d, n, &m, &tiles_n, &splits);
}

extern "C" int pcd_conv3d_f16_multi(const pcd_conv3d_desc_t* descs, int n, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    PCD_CHECK_ARG(descs != nullptr && n >= 1 && n <= MAX_VARIANTS);
    const pcd_conv3d_desc_t* d = descs;
    for (int i = 0; i < n; ++i) {
        const pcd_conv3d_desc_t* e = descs + i;
        const int rc = conv_check(e);
        if (rc != PCD_OK) return rc;
        // one launch: everything except the tap table, the weights and the output parity is shared
        PCD_CHECK_ARG(e->in == d->in && e->batch == d->batch && e->in_d == d->in_d && e->in_h == d->in_h &&
                      e->in_w == d->in_w && e->cin == d->cin && e->rows_d == d->rows_d && e->rows_h == d->rows_h &&
                      e->rows_w == d->rows_w && e->stride == d->stride && e->ntaps == d->ntaps && e->kpad == d->kpad &&
                      e->bias == d->bias && e->resid == d->resid && e->relu == d->relu && e->out == d->out &&
                      e->cout == d->cout && e->out_d == d->out_d && e->out_h == d->out_h && e->out_w == d->out_w &&
                      e->out_scale == d->out_scale && e->in2 == d->in2 && e->cin2 == d->cin2);
    }
    // the implicit GEMM reads a second source in whole K tiles, with no padding behind it
    PCD_CHECK_ARG(d->in2 == nullptr || (d->cin2 % CBK == 0 && d->kpad == d->ntaps * d->cin + d->cin2));
    ConvParams p{};
    p.in = (const half_t*)d->in; p.D = d->in_d; p.H = d->in_h; p.W = d->in_w; p.Cin = d->cin;
    p.cin_shift = __builtin_ctz((unsigned)d->cin);
    p.Do = d->rows_d; p.Ho = d->rows_h; p.Wo = d->rows_w; p.stride = d->stride;
    p.ntaps = d->ntaps; p.kpad = d->kpad;
    p.bias = d->bias; p.resid = (const half_t*)d->resid;
    p.out = (half_t*)d->out; p.Cout = d->cout;
    p.OD = d->out_d; p.OH = d->out_h; p.OW = d->out_w; p.os = d->out_scale;
    p.relu = d->relu;
    p.zero = (const half_t*)d->zero_page;
    p.in2 = (const half_t*)d->in2;
    p.cin2_shift = d->in2 ? __builtin_ctz((unsigned)d->cin2) : 0;
    p.kt2 = d->in2 ? d->ntaps * d->cin / CBK : 0x7fffffff;
    p.nvar = n;
    for (int i = 0; i < n; ++i) {
        p.var[i].taps = descs[i].taps; p.var[i].w = (const half_t*)descs[i].w;
        p.var[i].pz = descs[i].out_off_z; p.var[i].py = descs[i].out_off_y; p.var[i].px = descs[i].out_off_x;
    }
    int64_t m; int splits;
    const size_t need = conv_shape(d, n, &m, &p.tiles_n, &splits);
    p.M = (int)m;
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) splits = 1;   // no scratch: unsplit launch
    p.splits = splits;
    p.slabs = splits > 1 ? (float*)workspace : nullptr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(ceil_div(m, 128) * p.tiles_n), (unsigned)n, (unsigned)splits);
    // C_out <= 64, long K (the k4 s2 down-convolutions): three stages, the gather of K tile kt+2 in flight behind the
    // barrier of kt (enc.3 141 -> 112 us); short K and the 128-wide tile measured equal or slower with deeper rings
    if (d->cout <= 64) {
        if (d->kpad / CBK >= 32) hipLaunchKernelGGL((conv3d_igemm_kernel<128, 64, 64, 3>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((conv3d_igemm_kernel<128, 64, 64, 2>), grid, dim3(256), 0, s, p);
    } else {
        dispatch_int<0, 1, 2, 3, 4, 7, 8, 15>(g_conv3d.igemm_abl, [&](auto abl) {
            hipLaunchKernelGGL((conv3d_igemm_kernel<128, 128, 64, 2, decltype(abl)::value>), grid, dim3(256), 0, s, p);
        });
    }
    PCD_CHECK_LAUNCH();
    if (splits > 1) {
        const int64_t per = m * (d->cout / 8);                       // < 2^31: conv_check bounds the rows, cout / 8 <= 2^12 here
        PCD_CHECK_ARG(per <= 0x7fffffff);
        hipLaunchKernelGGL(conv3d_finish_kernel, dim3((unsigned)ceil_div(per, 256), (unsigned)n), dim3(256), 0, s, p);
        PCD_CHECK_LAUNCH();
    }
    return PCD_OK;
}

extern "C" int pcd_conv3d_f16(const pcd_conv3d_desc_t* d, void* stream) {
    PCD_CHECK_ARG(d != nullptr);
    return pcd_conv3d_f16_multi(d, 1, nullptr, 0, stream);
}

// TEST / BENCHMARK ONLY, process-global.  The bit fields are tabulated at the prototype in include/pcd_hip.h.
extern "C" int pcd_conv3d_config(int v) {
    PCD_CHECK_ARG(v >= 0 && (v & 7) <= 2 && v < 262144);
    static const int kSplitTarget[4] = {512, 768, 384, 1024};        // bits 5-6: 0, + 32, + 64, + 96
    static const int kLast8[4] = {3, 0, 1, 2};                       // bits 3-4: 0, + 8, + 16, + 24
    Conv3dConfig c;
    c.halo_tall = v & 7;
    c.last8 = kLast8[(v >> 3) & 3];
    c.split_target = kSplitTarget[(v >> 5) & 3];
    c.last_abl = (v >> 7) & 3;
    c.first8 = (v & 512) ? 0 : 1;
    c.igemm_abl = (v >> 10) & 15;
    c.last_roll = (v & 16384) ? 0 : 1;
    c.wreg_abl = (v >> 15) & 7;
    g_conv3d = c;
    return PCD_OK;
}
