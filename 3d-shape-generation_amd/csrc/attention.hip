// K6/K7: set attention over the N points of each shape (reference networks.py:51-83,
// nn.MultiheadAttention explicit bmm/softmax/bmm path) as a flash-style fused kernel:
// the N x N score matrix is never written.
//
// Formulation (everything K-major for v_mfma_f32_32x32x16_f16):
//   S^T[key][query] = sum_d K[key][d] Q[query][d]       A = K rows,  B = Q rows
//   O^T[dd][query]  = sum_key Vt[dd][key] P^T[key][query]  A = Vt rows, B = P^T straight from
//                                                           the S^T accumulators (no LDS trip)
// With queries on the MFMA lane index, the softmax row reduction is in-lane max3/adds plus one
// exchange between lane l and l+32 (v_permlane32_swap), and the O^T rescale is a per-lane scalar.
// V stays row-major [key][d] in LDS (staged like K, straight from qkv); the Vt fragments come from
// the hardware transpose read ds_read_b64_tr_b16, so there is no transpose pass and no workspace.
#include <type_traits>
#include "common.h"
#include "layernorm_rows.h"

namespace pcd {

// ---------------------------------------------------------------- LayerNorm
// one wave per row; fp32 statistics, biased variance, eps inside the sqrt (torch semantics)
__global__ __launch_bounds__(256) void layernorm_kernel(const half_t* __restrict__ x, int64_t rows, int c,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         half_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const half_t* xr = x + row * c;
    float s = 0.f;
    for (int i = lane; i < c; i += 64) s += (float)xr[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)c;
    float v = 0.f;
    for (int i = lane; i < c; i += 64) { const float d = (float)xr[i] - mean; v += d * d; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const float rstd = rsqrtf(v / (float)c + 1e-5f);
    half_t* orow = out + row * c;
    for (int i = lane; i < c; i += 64) orow[i] = to_half_sat(((float)xr[i] - mean) * rstd * gamma[i] + beta[i]);
}

// C = 64 / 128 / 256, the widths of the attention U-Net, take layernorm_rows_kernel<C / 8, false> of layernorm_rows.h instead

// ------------------------------------------------------------ flash attention
// block = 4 waves, each wave owns 32 (generic kernel) or 2 x 32 (pipelined kernels) queries of one (shape, head); K [64][D] and Vt [D][64]
// tiles arrive by LDS-DMA (global_load_lds 16 B/lane) into a 2-deep ring, XOR-swizzled through the
// source address so the ds_read_b128 fragment reads are bank-conflict free.
constexpr int KT = 64;              // keys per K/V tile (128 measured neutral: fewer barriers, but 2 workgroups/CU)
constexpr float RESCALE_THR = 8.0f;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// fmaxf pair -> one v_max3_f32 (attention.o is built with -fno-honor-nans, so no canonicalising
// v_max is needed on MFMA outputs).  NOT inline asm: an asm VALU reading an MFMA result gets none of
// the hazard wait states hipcc inserts for its own instructions (wrong maxima at d = 16).
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// max of lane l and lane l^32 in every lane, via v_permlane32_swap (VALU, no LDS)
__device__ __forceinline__ float xhalf_max(float v) {
    const unsigned u = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

// Swizzles (applied to the LDS-DMA source address and again on the reads).  K tile (ds_read_b128
// fragment reads, rows = lanes): chunk ^ f(row) makes the four 16-lane groups conflict free.
// V tile (ds_read_b64_tr_b16: 4 rows x 4 chunks per 32-lane half): with 128-B rows, rows r and r+2
// share a bank half, so bit 1 of the row flips the 64-B half of the row.
template <int RB>
__device__ __forceinline__ int k_swz(int row, int ch) {
    constexpr int CPR = RB / 16, LPR = 128 / RB;
    return ch ^ ((row / (2 * LPR)) & (CPR - 1));
}
template <int RB>
__device__ __forceinline__ int v_swz(int row, int ch) {
    return RB == 128 ? (ch ^ ((row & 2) << 1)) : ch;
}

// stage ROWS rows of RB bytes (global row stride ld halfs) with 4 waves; VSW selects the swizzle
template <int ROWS, int RB, bool VSW, int NW = 4, bool ASM = false>
__device__ __forceinline__ void stage_tile(const half_t* __restrict__ src, int64_t ld, int row0, int row_limit,
                                           char* lds, int wave, int lane) {
    constexpr int CPR = RB / 16, LPR = 128 / RB;
    constexpr int ROWS_PER_INSTR = 8 * LPR;                 // 64 lanes x 16 B = 1 KB
    constexpr int INSTRS = ROWS / ROWS_PER_INSTR;
    constexpr int PER_WAVE = (INSTRS + NW - 1) / NW;
#pragma unroll
    for (int r = 0; r < PER_WAVE; ++r) {
        const int ins = r * NW + wave;
        if (INSTRS % NW != 0 && ins >= INSTRS) break;
        const int row = ins * ROWS_PER_INSTR + lane / CPR;
        const int logical = VSW ? v_swz<RB>(row, lane % CPR) : k_swz<RB>(row, lane % CPR);
        int grow = row0 + row;
        grow = grow < row_limit ? grow : row_limit - 1;
        if (ASM) lds_dma16(src + (int64_t)grow * ld + logical * 8, lds + ins * 1024);
        else lds_dma16_builtin(src + (int64_t)grow * ld + logical * 8, lds + ins * 1024);
    }
}

// ------------------------------------------------------------ pieces every kernel of the family is built from
#define SP_SB() __builtin_amdgcn_sched_barrier(0)
#define SP_MF(a, b, cacc) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, cacc, 0, 0, 0)
constexpr unsigned SP_BIG_BITS = 0x70007000u;          // both halves hold the same fp16 sum T: T > 8192 (0x7000), inf, NaN

__device__ __forceinline__ half2_ sp_pk(float a, float b) { half2_ r; r.x = (half_t)a; r.y = (half_t)b; return r; }

// row max of a 32 x 32 score tile (7 v_max3 + one half-wave exchange)
__device__ __forceinline__ float sp_rowmax(const f32x16& s) {
    float mx = max3(s[0], s[1], s[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) mx = max3(mx, s[r], s[r + 1]);
    return xhalf_max(fmaxf(mx, s[15]));
}

// lane-partial row sum of the fp16 P of one tile, both halves of the result hold the total
__device__ __forceinline__ half2_ sp_tile_sum(const half8& p0, const half8& p1) {
    const half8 a = p0 + p1;
    const half4 b4 = a.lo + a.hi;
    const half2_ c2 = b4.lo + b4.hi;
    return c2 + c2.yx;
}

// Q fragments (B operand) of one 32-query block from its row qp: lane (query qr, half hh) holds Q[query][16*s + 8*hh + j],
// pre-scaled by log2(e)/sqrt(d) (one fp16 rounding) so the MFMA output is already in the exp2 domain
template <int KSTEPS>
__device__ __forceinline__ void attn_load_q(const half_t* qp, int hh, float scale_log2e, half8 (&qf)[KSTEPS]) {
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        const half8 raw = *(const half8*)(qp + 16 * s + 8 * hh);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[s][e] = (half_t)((float)raw[e] * scale_log2e);
    }
}

// the same for the two blocks A and B of a wave of the pipelined kernels, load by load
template <int KSTEPS>
__device__ __forceinline__ void attn_load_q2(const half_t* qpA, const half_t* qpB, int hh, float scale_log2e, half8 (&qA)[KSTEPS],
                                             half8 (&qB)[KSTEPS]) {
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        const half8 ra = *(const half8*)(qpA + 16 * s + 8 * hh), rb = *(const half8*)(qpB + 16 * s + 8 * hh);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            qA[s][e] = (half_t)((float)ra[e] * scale_log2e);
            qB[s][e] = (half_t)((float)rb[e] * scale_log2e);
        }
    }
}

// one LDS-DMA instruction (1 KiB per wave): wave-uniform source base and LDS address (through m0), lane-constant 32-bit offset
__device__ __forceinline__ void sp_dma(const char* sbase, unsigned voff, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr)
                 : "memory", "m0");
}

// Tail of a phase of the pipelined kernels (c0 .. c7: the tile's fp16 P in pairs, b1: the sum tree so far).  On gfx950 a
// packed (VOP3P) result needs one wait state before any VALU reads it, so the compiler puts an s_nop behind each of the three
// dependent v_pk_add_f16 of this tail.  Written out by hand, the OTHER block's pending row sum (its tile was checked a phase
// ago) is folded into its fp32 l in those slots instead:
//   a3 = c3 + c7 | lo = f32(t_other) | t = b1 + a3 | l_other += lo | tt = t + swap(t)   (the compiler adds the one
//   wait state between the asm block and its own compare of tt)
// Packs P into the two MFMA operands and returns the tile's lane-partial row sum (fp16, in both halves).
__device__ __forceinline__ half2_ sp_phase_tail(half2_ c0, half2_ c1, half2_ c2, half2_ c3, half2_ c4, half2_ c5, half2_ c6,
                                                half2_ c7, half2_ b1, half2_ t_other, float& l_other, half8& p0, half8& p1) {
    half2_ a3, t, tt;
    float lo;
    asm volatile("v_pk_add_f16 %0, %5, %6\n\t"
                 "v_cvt_f32_f16_e32 %3, %8\n\t"
                 "v_pk_add_f16 %1, %7, %0\n\t"
                 "v_add_f32_e32 %4, %4, %3\n\t"
                 "v_pk_add_f16 %2, %1, %1 op_sel:[0,1] op_sel_hi:[1,0]"
                 : "=&v"(a3), "=&v"(t), "=&v"(tt), "=&v"(lo), "+v"(l_other)
                 : "v"(c3), "v"(c7), "v"(b1), "v"(t_other));
    p0 = __builtin_shufflevector(__builtin_shufflevector(c0, c1, 0, 1, 2, 3), __builtin_shufflevector(c2, c3, 0, 1, 2, 3),
                                 0, 1, 2, 3, 4, 5, 6, 7);
    p1 = __builtin_shufflevector(__builtin_shufflevector(c4, c5, 0, 1, 2, 3), __builtin_shufflevector(c6, c7, 0, 1, 2, 3),
                                 0, 1, 2, 3, 4, 5, 6, 7);
    return tt;
}

// ------------------------------------------------------------ generic kernel (d = 16 / 32 / 64, any n)
// One 32-query block per wave, 2-deep K/V ring, masked last tile.  The frame is written once; the softmax between the score
// MFMAs and the PV MFMAs comes in two forms:
//   RunningMax  the round-1 form, a running row max with a deferred rescale: the tests' comparator and pcd_set_attention_config(1)
//   MaxFree     the softmax of set_attention_sp_kernel: every shape the pipelined kernels do not take
enum class AttnSoftmax { RunningMax, MaxFree };

__device__ __forceinline__ float lane_row_sum(float l) { return l; }
__device__ __forceinline__ float lane_row_sum(f32x2 l) { return l[0] + l[1]; }

template <int D, AttnSoftmax SOFTMAX>
__global__ __launch_bounds__(256, SOFTMAX == AttnSoftmax::MaxFree ? 2 : 1) void set_attention_generic_kernel(
    const half_t* __restrict__ qkv, int n, int c, int heads, float scale_log2e, half_t* __restrict__ out) {
    constexpr bool MAX_FREE = SOFTMAX == AttnSoftmax::MaxFree;
    constexpr int DP = (D < 32) ? 32 : D;        // O^T rows padded to the 32-row MFMA tile
    constexpr int KSTEPS = D / 16;               // MFMA k-steps of the S^T product
    constexpr int OT = DP / 32;                  // 32-row O^T tiles
    constexpr int KRB = D * 2;                   // bytes per K row
    constexpr int KBYTES = KT * KRB, STAGE = 2 * KBYTES;   // K tile + V tile, both [64 keys][D]
    constexpr int ZERO_OFF = 2 * STAGE;                      // 64 zero bytes: O^T rows >= D (d = 16 only)
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE + 64];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = lane & 31, hh = lane >> 5;
    const int bh = blockIdx.y, b = bh / heads, head = bh - b * heads;
    const int q0 = blockIdx.x * 128 + wave * 32;
    const int64_t row_base = (int64_t)b * n;
    const int ld = 3 * c;

    half8 qf[KSTEPS];
    {
        int qi = q0 + qr;
        qi = qi < n ? qi : n - 1;                // rows past n compute a copy of the last one and store nothing
        attn_load_q(qkv + (row_base + qi) * ld + head * D, hh, scale_log2e, qf);
    }
    // negm: 16 registers all holding -m (running row max of query qr, exp2 domain).  It is the C input of the first S^T MFMA
    // of every tile (D != C), so the accumulator comes out as s*c - m with no VALU work.  (For d <= 32 the compiler rebuilds it
    // with 15 v_mov per tile; carrying -m through an extra MFMA k-step instead -- constant K fragment [1, 1, 0..], Q fragment
    // [-m_hi, -m_lo, 0..] -- removes the moves and measured SLOWER: 696 v. 734 TFLOP/s at d = 32, 388 v. 410 at d = 16.)
    f32x16 oacc[OT], negm;
    std::conditional_t<MAX_FREE, float, f32x2> l = {};       // lane-partial row sum (RunningMax: two at a time, v_pk_add_f32)
#pragma unroll
    for (int r = 0; r < 16; ++r) negm[r] = 0.f;
#pragma unroll
    for (int o = 0; o < OT; ++o)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[o][r] = 0.f;
    if (tid < 16) *(float*)(smem + ZERO_OFF + tid * 4) = 0.f;

    const half_t* kbase = qkv + row_base * ld + c + head * D;
    const half_t* vbase = qkv + row_base * ld + 2 * c + head * D;
    const int ntiles = (n + KT - 1) / KT;

    // transpose-read addressing (ds_read_b64_tr_b16): in each 16-lane group, lane 4q+p supplies the
    // address of key row q, d columns 4p..4p+3 of the group's 4 x 16 block and receives column (lane&15).
    // Group g = lane>>4 covers O^T rows dd0 = 16*(g&1) .. +16 of a 32-row tile for key half hh = g>>1.
    const int tq = (lane >> 2) & 3, tp = lane & 3, tg = lane >> 4;
    const int tr_dd0 = 16 * (tg & 1);

    auto stage = [&](int kt, int buf) {
        char* base = smem + buf * STAGE;
        // LDS-DMA from asm: with the builtin pending the compiler drains vmcnt and lgkmcnt in front of every fragment read
        stage_tile<KT, KRB, false, 4, true>(kbase, ld, kt * KT, n, base, wave, lane);
        stage_tile<KT, KRB, true, 4, true>(vbase, ld, kt * KT, n, base + KBYTES, wave, lane);
    };

    // one KV tile; MASK only for the last, partial tile (keys >= n get -inf) so full tiles carry no
    // compare/select code at all
    auto tile_body = [&](int kt, auto mask_tag) {
        constexpr bool MASK = decltype(mask_tag)::value;
        const char* kb = smem + (kt & 1) * STAGE;
        const char* vb = kb + KBYTES;
#pragma unroll
        for (int sub = 0; sub < KT / 32; ++sub) {
            half8 kf[KSTEPS];
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                const int row = sub * 32 + qr;
                kf[s] = *(const half8*)(kb + row * KRB + (k_swz<KRB>(row, 2 * s + hh) << 4));
            }
            // Vt fragments: element j of lane half hh must be key 16*s2 + 8*(j>>2) + 4*hh + (j&3) (the k order
            // in which the S^T accumulators hand over P^T): two transposed 4-key reads per fragment.
            half8 vf[2][OT];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int o = 0; o < OT; ++o) {
                    const int dd0 = o * 32 + tr_dd0;
                    fp16x4 lo, hi;
                    if (D >= 32 || dd0 < D) {
                        const int key = sub * 32 + 16 * s2 + 4 * (tg >> 1) + tq;
                        const int ch = (dd0 >> 3) + (tp >> 1);
                        const char* a0 = vb + key * KRB + (v_swz<KRB>(key, ch) << 4) + (tp & 1) * 8;
                        const char* a1 = vb + (key + 8) * KRB + (v_swz<KRB>(key + 8, ch) << 4) + (tp & 1) * 8;
                        lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)a0);
                        hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)a1);
                    } else {   // d = 16: O^T rows 16..31 do not exist; every lane still issues the read (EXEC all ones)
                        const char* z = smem + ZERO_OFF + (tp & 1) * 8;
                        lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)z);
                        hi = lo;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) { vf[s2][o][e] = (half_t)lo[e]; vf[s2][o][4 + e] = (half_t)hi[e]; }
                }
            // S'^T tile: 32 keys x 32 queries, already relative to the running max
            f32x16 sacc = SP_MF(kf[0], qf[0], negm);
#pragma unroll
            for (int s = 1; s < KSTEPS; ++s) sacc = SP_MF(kf[s], qf[s], sacc);
            if constexpr (MASK) {   // register r of lane (qr, hh) is key (r&3) + 8*(r>>2) + 4*hh of this sub-tile
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kt * KT + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    if (key >= n) sacc[r] = -INFINITY;
                }
            }
            const bool first = (kt == 0) && (sub == 0);
            half8 p0, p1;                        // P^T of this tile, the B operands of the two PV k-steps
            if constexpr (MAX_FREE) {
                // The running-max form below spends 66 VALU instructions per 32 x 32 score tile, 50 of them around the 16 v_exp_f32
                // (row max chain, half-wave exchange, compare, fp32 row sums); at d = 32 / 16 a tile is only 4 / 3 MFMAs (128 / 96
                // matrix cycles), so it is VALU bound at 25.6 % / 14.2 % of the MFMA peak.  This form: m is fixed exactly by the first
                // 32 keys (every row then has a P = 1 term); afterwards a tile is exponentiated against the old m, its lane-partial
                // row sum is formed from the fp16 P by a packed-fp16 tree and only a sum >= 2^13 (or inf) sends the wave down the rare
                // path (exact maxima, rescale O / l, redo the tile).  Softmax is invariant to m: the same function as the
                // reference's.  ~36 VALU instructions per tile.  The bound that remains is the exponentials themselves: 16 v_exp_f32
                // (8 cycles each) + 8 packs + 8 packed adds = ~200 issue cycles per tile and wave against 128 / 96 cycles of MFMA,
                // i.e. <= ~42 % / ~21 % of the MFMA peak for d = 32 / 16 however the rest is arranged.  Measured (B = 64, N = 2048):
                // d = 32 734 v. 641 TFLOP/s, d = 16 410 v. 367.
                if (first) {                     // the first 32 keys fix the running max exactly
                    const float mx = sp_rowmax(sacc);
#pragma unroll
                    for (int r = 0; r < 16; ++r) { negm[r] = -mx; sacc[r] -= mx; }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    p0[j] = (half_t)__builtin_amdgcn_exp2f(sacc[j]);
                    p1[j] = (half_t)__builtin_amdgcn_exp2f(sacc[8 + j]);
                }
                half2_ tt = sp_tile_sum(p0, p1);
                if (__builtin_expect(__any(__builtin_bit_cast(unsigned, tt) > SP_BIG_BITS), 0)) {
                    // rare: some score is ~9 or more above the running max (or P overflowed fp16): exact maxima, rescale, redo the tile
                    const float delta = fmaxf(sp_rowmax(sacc), 0.f);
                    const float alpha = __builtin_amdgcn_exp2f(-delta);
                    l *= alpha;
#pragma unroll
                    for (int r = 0; r < 16; ++r) { negm[r] -= delta; sacc[r] -= delta; }
#pragma unroll
                    for (int o = 0; o < OT; ++o)
#pragma unroll
                        for (int r = 0; r < 16; ++r) oacc[o][r] *= alpha;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        p0[j] = (half_t)__builtin_amdgcn_exp2f(sacc[j]);
                        p1[j] = (half_t)__builtin_amdgcn_exp2f(sacc[8 + j]);
                    }
                    tt = sp_tile_sum(p0, p1);
                }
                l += (float)tt.x;
            } else {
                // Deferred max: move m only when some row's scores exceed it by more than RESCALE_THR (then
                // P <= 2^THR, exact in fp16's exponent range; row sums and O are fp32).  The very first tile
                // always sets m to its true row max (which may be negative).
                const float mx = sp_rowmax(sacc);
                if (first || __any(mx > RESCALE_THR)) {          // wave-uniform, rare after the first tiles
                    const float delta = first ? mx : fmaxf(mx, 0.f);
                    const float alpha = __builtin_amdgcn_exp2f(-delta);
                    l *= (f32x2){alpha, alpha};
#pragma unroll
                    for (int r = 0; r < 16; ++r) { negm[r] -= delta; sacc[r] -= delta; }
#pragma unroll
                    for (int o = 0; o < OT; ++o)
#pragma unroll
                        for (int r = 0; r < 16; ++r) oacc[o][r] *= alpha;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[r] = __builtin_amdgcn_exp2f(sacc[r]);
                // per-lane partial row sums, two at a time (v_pk_add_f32); halves combined in the epilogue
#pragma unroll
                for (int r = 0; r < 16; r += 2) l += (f32x2){sacc[r], sacc[r + 1]};
#pragma unroll
                for (int j = 0; j < 8; ++j) { p0[j] = (half_t)sacc[j]; p1[j] = (half_t)sacc[8 + j]; }
            }
#pragma unroll
            for (int o = 0; o < OT; ++o) {
                oacc[o] = SP_MF(vf[0][o], p0, oacc[o]);
                oacc[o] = SP_MF(vf[1][o], p1, oacc[o]);
            }
        }
    };

    const int full_tiles = n / KT;
    stage(0, 0);
    for (int kt = 0; kt < full_tiles; ++kt) {
        wait_vmcnt<0>();
        __syncthreads();
        if (kt + 1 < ntiles) stage(kt + 1, (kt + 1) & 1);
        tile_body(kt, std::false_type{});
    }
    if (full_tiles < ntiles) {
        wait_vmcnt<0>();
        __syncthreads();
        tile_body(full_tiles, std::true_type{});
    }

    const int qi = q0 + qr;
    const float l_lane = lane_row_sum(l);
    const float l_tot = l_lane + __shfl_xor(l_lane, 32);     // the other half of the row sum sits in lane ^ 32
    if (qi < n) {
        // lane (query qr, half hh) holds O^T rows dd = o*32 + (r&3) + 8*(r>>2) + 4*hh
        const float inv = 1.f / l_tot;
        half_t* orow = out + (row_base + qi) * c + head * D;
#pragma unroll
        for (int o = 0; o < OT; ++o)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = o * 32 + 8 * g + 4 * hh;
                if (dd < D) {
                    half4 ov;
#pragma unroll
                    for (int e = 0; e < 4; ++e) ov[e] = to_half_sat(oacc[o][4 * g + e] * inv);
                    *(half4*)(orow + dd) = ov;
                }
            }
    }
}


// ------------------------------------------------------------ software-pipelined kernel (d = 64, n % 256 == 0)
// The generic kernel (figures of its running-max form) keeps one 32-query block per wave and leaves the MFMA / softmax overlap to whichever waves share
// a SIMD; measured, the two add up (583 cycles per 32 x 32 score tile for 256 cycles of MFMA, 66 VALU instructions per
// tile).  Here a wave owns TWO 32-query blocks A and B and interleaves them by hand, half a step apart:
//
//   phase 1 of key sub-tile i:   MFMA  O_B += V(i-1)^T P_B(i-1),  S_A(i+1) = K(i+1) Q_A^T   |  VALU  P_A(i) = 2^S_A(i)
//   phase 2 of key sub-tile i:   MFMA  S_B(i+1) = K(i+1) Q_B^T,   O_A += V(i)^T P_A(i)      |  VALU  P_B(i) = 2^S_B(i)
//
// so every basic block holds 8 independent MFMAs beside the 16 v_exp_f32 + packing of the other block, written out
// gap by gap.  The per-score VALU work is exp2, fp16 pack and HALF a packed-fp16 add: the running max is not tracked
// per tile.  m is set exactly by the first 32 keys (every row then has a P = 1 term, l >= 1); afterwards a tile is
// exponentiated against the old m optimistically, its lane-partial row sum is formed from the fp16 P (the numbers the
// PV MFMA really multiplies) by a packed-fp16 tree, and only if some lane's sum reaches 2^13 (a score ~9 or more above
// the running max; an fp16 overflow shows up as +inf in the sum) the wave takes the rare path: exact row maxima,
// rescale O / l / the pending S(i+1), redo the tile.  Softmax is invariant to m, so the result is the same function
// as the reference's; P < 2^13 keeps every product inside fp16 / fp32 range.
// Registers: single K and V fragment sets (the four MFMAs that read the operand about to be reloaded come first in
// their phase, the LDS reads that overwrite it are issued behind them) keep the kernel at 256 registers = two waves
// per SIMD, which hide each other's LDS / branch / dependency stalls.  K/V tiles (64 keys) arrive by LDS-DMA into a
// 4-slot ring, two tiles ahead; the tile loop is unrolled by the ring so every LDS address is a lane-constant base
// plus an immediate: no address arithmetic in the loop.

// rare path: raise the running max of the rows that need it, rescale everything that was formed against the old one
// (O, l, the -m accumulator seed, the pending next score tile) and redo this tile's exponentials
__device__ __forceinline__ half2_ sp_fix(f32x16& s_cur, f32x16& s_nxt, f32x16& negm, f32x16 (&o)[2], float& l,
                                         half8& p0, half8& p1) {
    const float delta = fmaxf(sp_rowmax(s_cur), 0.f);
    const float alpha = __builtin_amdgcn_exp2f(-delta);
    l *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        negm[r] -= delta; s_cur[r] -= delta; s_nxt[r] -= delta;
        o[0][r] *= alpha; o[1][r] *= alpha;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        p0[j] = (half_t)__builtin_amdgcn_exp2f(s_cur[j]);
        p1[j] = (half_t)__builtin_amdgcn_exp2f(s_cur[8 + j]);
    }
    return sp_tile_sum(p0, p1);
}

// One phase, gap by gap (sched_barrier(0) between gaps pins the order): MFMA k of the 8, then the two v_exp_f32 of the
// pair the sum tree needs next, then the pack / tree adds whose inputs are a gap old.  Per gap: 8 (MFMA issue) + 16
// (2 exp) + 4..8 (1-2 VALU) cycles against the MFMA's 32.
//   PV_FIRST: O += V^T P_other (gaps 0-3), mid() reloads V, then sn = K Q^T + negm (gaps 4-7)
//   else    : sn = K Q^T + negm (gaps 0-3), mid() reloads K, then O += V^T P_other (gaps 4-7)
// Returns the tile's lane-partial row sum (fp16, in both halves).
template <bool PV_FIRST, typename Mid>
__device__ __forceinline__ half2_ sp_phase(const f32x16& s, half8& p0, half8& p1, const half8 (&kf)[4],
                                           const half8 (&qf)[4], const f32x16& negm, f32x16& sn, f32x16 (&o)[2],
                                           const half8 (&vf)[2][2], const half8& y0, const half8& y1, half2_ t_other,
                                           float& l_other, Mid&& mid) {
#define SP_M(k)                                                                                    \
    do {                                                                                           \
        constexpr int j = (k) & 3;                                                                 \
        if (((k) < 4) == PV_FIRST) o[j & 1] = SP_MF(vf[j >> 1][j & 1], (j >> 1) ? y1 : y0, o[j & 1]); \
        else sn = SP_MF(kf[j], qf[j], j == 0 ? negm : sn);                                         \
    } while (0)
    SP_SB();
    SP_M(0);
    const float e0 = __builtin_amdgcn_exp2f(s[0]), e1 = __builtin_amdgcn_exp2f(s[1]);
    SP_SB();
    SP_M(1);
    const float e8 = __builtin_amdgcn_exp2f(s[8]), e9 = __builtin_amdgcn_exp2f(s[9]);
    const half2_ c0 = sp_pk(e0, e1);
    SP_SB();
    SP_M(2);
    const float e2 = __builtin_amdgcn_exp2f(s[2]), e3 = __builtin_amdgcn_exp2f(s[3]);
    const half2_ c4 = sp_pk(e8, e9);
    SP_SB();
    SP_M(3);
    const float e10 = __builtin_amdgcn_exp2f(s[10]), e11 = __builtin_amdgcn_exp2f(s[11]);
    const half2_ c1 = sp_pk(e2, e3);
    const half2_ a0 = c0 + c4;
    SP_SB();
    mid();
    SP_SB();
    SP_M(4);
    const float e4 = __builtin_amdgcn_exp2f(s[4]), e5 = __builtin_amdgcn_exp2f(s[5]);
    const half2_ c5 = sp_pk(e10, e11);
    SP_SB();
    SP_M(5);
    const float e12 = __builtin_amdgcn_exp2f(s[12]), e13 = __builtin_amdgcn_exp2f(s[13]);
    const half2_ c2 = sp_pk(e4, e5);
    const half2_ a1 = c1 + c5;
    SP_SB();
    SP_M(6);
    const float e6 = __builtin_amdgcn_exp2f(s[6]), e7 = __builtin_amdgcn_exp2f(s[7]);
    const half2_ c6 = sp_pk(e12, e13);
    const half2_ b0 = a0 + a1;
    SP_SB();
    SP_M(7);
    const float e14 = __builtin_amdgcn_exp2f(s[14]), e15 = __builtin_amdgcn_exp2f(s[15]);
    const half2_ c3 = sp_pk(e6, e7);
    const half2_ a2 = c2 + c6;
    const half2_ b1 = b0 + a2;
    SP_SB();
#undef SP_M
    return sp_phase_tail(c0, c1, c2, c3, c4, c5, c6, sp_pk(e14, e15), b1, t_other, l_other, p0, p1);
}

// ABL: timing ablations (pcd_set_attention_config(16 + bits), outputs wrong while set): 1 = no K/V restaging in the loop, 2 = no rare-path test
// NW: waves per workgroup (4 or 8): the workgroup's 64 NW queries share one K/V ring -- restaging K/V costs 10 % of the kernel at NW = 4 (tools/bench_attn_small_d.py),
// and at NW = 8 every wave moves 2 pieces per tile instead of 4
template <int ABL = 0, int NW = 4>
__global__ __launch_bounds__(64 * NW, 2) void set_attention_sp_kernel(const half_t* __restrict__ qkv, int n, int c, int heads,
                                                                   float scale_log2e, half_t* __restrict__ out) {
    constexpr int D = 64, KSTEPS = 4, KRB = 128, NSLOT = 4;
    constexpr int KBYTES = KT * KRB, STAGE = 2 * KBYTES;
    constexpr int AHEAD = NSLOT - 2;                          // tiles in flight beyond the one being consumed
    __shared__ __attribute__((aligned(16))) char smem[NSLOT * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = lane & 31, hh = lane >> 5;
    // XCD-aware block -> (shape, head, query block) map.  Workgroups are dealt round-robin over the 8 XCDs
    // (block L runs on XCD L % 8, speed only, never correctness), and the n/256 query blocks of one (shape, head)
    // all stream the same K/V: give them to ONE XCD, next to each other in time, so its L2 fetches that K/V once
    // instead of 8 L2s fetching it once each.
    const int nqb = n / (64 * NW);                            // query blocks per (shape, head)
    int bh, qb;
    {
        const int L = blockIdx.x, total_bh = gridDim.x / nqb;
        const int xcd = L & 7, i = L >> 3;                    // i-th block of this XCD
        const int j = i / nqb;
        bh = xcd + 8 * j;
        qb = i - j * nqb;
        if (bh >= total_bh || (total_bh & 7)) { bh = L / nqb; qb = L - bh * nqb; }   // batch*heads not a multiple of 8: plain order
    }
    const int b = bh / heads, head = bh - b * heads;
    const int q0 = qb * (64 * NW) + wave * 64;
    const int64_t row_base = (int64_t)b * n;
    const int ld = 3 * c;

    const half_t* kbase = qkv + row_base * ld + c + head * D;
    const half_t* vbase = qkv + row_base * ld + 2 * c + head * D;
    const int ntiles = n / KT;                                // a multiple of NSLOT (n % 256 == 0)
    // LDS-DMA staging (global_load_lds_dwordx4, 1 KiB per wave-instruction = 8 rows of a [64 keys][64] tile): a tile is
    // 8 K pieces + 8 V pieces, wave w moves K pieces w, w+4 and V pieces w, w+4.  Source = wave-uniform SGPR base
    // (tile, piece rows, K or V) + a lane-constant 32-bit offset that carries the XOR swizzles of the generic kernel
    // (they only depend on the row inside the piece and on w & 1): no vector arithmetic per piece, so the four pieces
    // of a tile are issued one per phase, in an MFMA gap each.
    const unsigned lrow = lane >> 3, lch = lane & 7;
    const unsigned koff32 = lrow * (unsigned)ld * 2u + ((lch ^ ((4u * (wave & 1) + (lane >> 4)) & 7u)) << 4);
    const unsigned voff32 = lrow * (unsigned)ld * 2u + ((lch ^ ((lrow & 2u) << 1)) << 4);
    const unsigned lds0 = (unsigned)(size_t)smem;
    const size_t tile_bytes = (size_t)KT * ld * 2, half_bytes = (size_t)32 * ld * 2;
    const char* kwave = (const char*)kbase + (size_t)(8 * wave) * ld * 2;     // this wave's first piece of tile 0
    const char* vwave = (const char*)vbase + (size_t)(8 * wave) * ld * 2;
    // piece j (0..3) of tile kt into ring slot `slot`: K rows 8w.., K rows 8w+32.., V rows 8w.., V rows 8w+32..
    auto stage_piece = [&](int kt, int slot, int j) __attribute__((always_inline)) {
        if constexpr (NW == 4) {
            const char* src = ((j & 2) ? vwave : kwave) + (size_t)kt * tile_bytes + ((j & 1) ? half_bytes : 0);
            const unsigned dst = lds0 + slot * STAGE + ((j & 2) ? KBYTES : 0) + (wave + 4 * (j & 1)) * 1024;
            sp_dma(src, (j & 2) ? voff32 : koff32, dst);
        } else {                                               // eight waves: piece 0 = K rows 8 w .., piece 2 = V rows 8 w .. (one in front of each sub-tile)
            if (j == 0 || j == 2) {
                const char* src = (j ? vwave : kwave) + (size_t)kt * tile_bytes;
                sp_dma(src, j ? voff32 : koff32, lds0 + slot * STAGE + (j ? KBYTES : 0) + wave * 1024);
            }
        }
    };
    // K/V tiles 0 .. AHEAD go out first (4 LDS-DMA instructions per wave and tile), the Q rows behind them
#pragma unroll
    for (int t = 0; t <= AHEAD; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) stage_piece(t, t, j);

    half8 qA[KSTEPS], qB[KSTEPS];
    {
        const half_t* qpA = qkv + (row_base + q0 + qr) * ld + head * D;
        attn_load_q2(qpA, qpA + (int64_t)32 * ld, hh, scale_log2e, qA, qB);
    }

    // lane-constant LDS addresses (slot 0, key sub-tile 0); every read adds a compile-time offset.
    //   K fragment s: row qr (+32 per sub-tile), 16-byte chunk (2s + hh) ^ swizzle(row): the swizzle only depends
    //   on qr (row bits 1..3), so sub-tile and slot are pure offsets.
    //   V^T fragments (ds_read_b64_tr_b16, see the generic kernel): key 4*(tg>>1) + tq (+8, +16 per MFMA k-step,
    //   +32 per sub-tile), chunk (dd0>>3) + (tp>>1) ^ swizzle(key & 2): one base per 32-row O^T tile.
    const int tq = (lane >> 2) & 3, tp = lane & 3, tg = lane >> 4;
    const char* kaddr[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) kaddr[s] = smem + qr * KRB + (k_swz<KRB>(qr, 2 * s + hh) << 4);
    const char* vaddr[2];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const int key = 4 * (tg >> 1) + tq;
        const int ch = ((o * 32 + 16 * (tg & 1)) >> 3) + (tp >> 1);
        vaddr[o] = smem + KBYTES + key * KRB + (v_swz<KRB>(key, ch) << 4) + (tp & 1) * 8;
    }
    auto load_k = [&](int off, half8 (&kf)[KSTEPS]) __attribute__((always_inline)) {         // off = slot * STAGE + sub * 32 * KRB
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) kf[s] = *(const half8*)(kaddr[s] + off);
    };
    auto load_v = [&](int off, half8 (&vf)[2][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const char* a0 = vaddr[o] + off + 16 * s2 * KRB;
                const fp16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)a0);
                const fp16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)(a0 + 8 * KRB));
#pragma unroll
                for (int e = 0; e < 4; ++e) { vf[s2][o][e] = (half_t)lo[e]; vf[s2][o][4 + e] = (half_t)hi[e]; }
            }
    };

    f32x16 oA[2], oB[2], negmA, negmB, sA, sB, sAn, sBn;
    float lA = 0.f, lB = 0.f;
    half8 pA0, pA1, pB0, pB1, kf[KSTEPS], vf[2][2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { oA[0][r] = oA[1][r] = oB[0][r] = oB[1][r] = 0.f; negmA[r] = negmB[r] = 0.f; }
#pragma unroll
    for (int e = 0; e < 8; ++e) {                              // the first phase's O_B += V(-1)^T P_B(-1) adds zero
        pB0[e] = pB1[e] = (half_t)0.f;
        vf[0][0][e] = vf[0][1][e] = vf[1][0][e] = vf[1][1][e] = (half_t)0.f;
    }

    wait_vmcnt<0>();
    __syncthreads();
    // the first 32 keys fix the running max exactly: S(0) - rowmax, seed accumulators = -rowmax
    load_k(0, kf);
    sA = SP_MF(kf[0], qA[0], negmA);
    sB = SP_MF(kf[0], qB[0], negmB);
#pragma unroll
    for (int s = 1; s < KSTEPS; ++s) { sA = SP_MF(kf[s], qA[s], sA); sB = SP_MF(kf[s], qB[s], sB); }
    {
        const float ma = sp_rowmax(sA), mb = sp_rowmax(sB);
#pragma unroll
        for (int r = 0; r < 16; ++r) { negmA[r] = -ma; sA[r] -= ma; negmB[r] = -mb; sB[r] -= mb; }
    }
    load_k(32 * KRB, kf);                                     // K(1) for the first sub-tile's S(i+1) products

    // one key sub-tile i (32 keys): kf holds K(i+1) and vf V(i-1) on entry; V(i) at voff, K(i+2) at koff; pieces j0 and
    // j0 + 1 of tile st (if any) leave for ring slot sslot, one in front of each phase
    half2_ tA, tB;                                              // row sums of the last tile of A / B, not yet in lA / lB
    tA.x = tA.y = tB.x = tB.y = (half_t)0.f;
    // one key sub-tile i (32 keys): kf holds K(i+1) and vf V(i-1) on entry; V(i) at voff, K(i+2) at koff; when STAGE_ON,
    // pieces j0 and j0 + 1 of tile st leave for ring slot sslot, one in front of each phase
    auto sub_iter = [&](int voff, int koff, bool stage_on, int st, int sslot, int j0) __attribute__((always_inline)) {
        if (!(ABL & 1) && stage_on) stage_piece((ABL & 8) ? (st & 3) : st, sslot, j0);
        tA = sp_phase<true>(sA, pA0, pA1, kf, qA, negmA, sAn, oB, vf, pB0, pB1, tB, lB, [&]() { load_v(voff, vf); });
        if (!(ABL & 2) && __builtin_expect(__any(__builtin_bit_cast(unsigned, tA) > SP_BIG_BITS), 0)) tA = sp_fix(sA, sAn, negmA, oA, lA, pA0, pA1);
        if (!(ABL & 1) && stage_on) stage_piece((ABL & 8) ? (st & 3) : st, sslot, j0 + 1);
        tB = sp_phase<false>(sB, pB0, pB1, kf, qB, negmB, sBn, oA, vf, pA0, pA1, tA, lA, [&]() { load_k(koff, kf); });
        if (!(ABL & 2) && __builtin_expect(__any(__builtin_bit_cast(unsigned, tB) > SP_BIG_BITS), 0)) tB = sp_fix(sB, sBn, negmB, oB, lB, pB0, pB1);
        sA = sAn; sB = sBn;
    };
    // NSLOT tiles, tile t0 + u in ring slot u.  LAST = the final group: only its first tile still has a tile to stage
    // (t0 + 3 = ntiles - 1), and the waits drain instead of leaving the youngest stage in flight.
    auto tile_group = [&](int t0, auto last_tag) __attribute__((always_inline)) {
        constexpr bool LAST = decltype(last_tag)::value;
#pragma unroll
        for (int u = 0; u < NSLOT; ++u) {
            // tile t+1 has landed (all but the youngest stage's 4 LDS-DMA) and every wave is done with tile t-1
            // (lgkmcnt(0): this wave's own fragment reads have RETURNED before the barrier behind which another wave's LDS-DMA refills a slot --
            // the compiler's barrier fence says so at three of the four barriers of a group, not at the loop-carried one: tools/check_barrier_reads.py)
            if (!LAST || u < 2) {
                if constexpr (NW == 4) wait_vmcnt_lgkm0<4>();
                else wait_vmcnt_lgkm0<2>();
            }
            else wait_vmcnt_lgkm0<0>();
            __syncthreads();
            const int cur = u * STAGE, nxt = ((u + 1) % NSLOT) * STAGE;   // last tile: nxt holds stale bytes, S(i+1) unused
            const int st = t0 + u + AHEAD + 1, sslot = (u + AHEAD + 1) % NSLOT;   // tile to stage; its slot == slot of tile t-1
            const bool on = !LAST || u == 0;
            sub_iter(cur, nxt, on, st, sslot, 0);                       // sub-tile 2t:   V(2t),   K(2t+2) = tile t+1 rows 0..31
            sub_iter(cur + 32 * KRB, nxt + 32 * KRB, on, st, sslot, 2); // sub-tile 2t+1: V(2t+1), K(2t+3) = tile t+1 rows 32..63
        }
    };
    int t0 = 0;
    for (; t0 + NSLOT < ntiles; t0 += NSLOT) tile_group(t0, std::false_type{});
    tile_group(t0, std::true_type{});
#pragma unroll
    for (int oo = 0; oo < 2; ++oo) {                          // O_B += V(last)^T P_B(last)
        oB[oo] = SP_MF(vf[0][oo], pB0, oB[oo]);
        oB[oo] = SP_MF(vf[1][oo], pB1, oB[oo]);
    }

    // epilogue: lane (query qr, half hh) holds O^T rows dd = oo*32 + (r&3) + 8*(r>>2) + 4*hh
    auto store = [&](const f32x16 (&o)[2], float l, int qi) {
        const float l_tot = l + __shfl_xor(l, 32);
        const float inv = 1.f / l_tot;
        half_t* orow = out + (row_base + qi) * c + head * D;
#pragma unroll
        for (int oo = 0; oo < 2; ++oo)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half4 ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = to_half_sat(o[oo][4 * g + e] * inv);
                *(half4*)(orow + oo * 32 + 8 * g + 4 * hh) = ov;
            }
    };
    store(oA, lA, q0 + qr);
    store(oB, lB + (float)tB.x, q0 + 32 + qr);                 // B's last tile sum is still pending (A's went in with B's last phase)
}


// ------------------------------------------------------------ software-pipelined kernel for d = 32 / 16 (n % 256 == 0)
// The max-free form of the generic kernel keeps ONE 32-query block per wave: the score MFMAs, the 16 v_exp_f32, the packs, the row sum, the any() branch and the
// PV MFMAs of a 32 x 32 score tile are one dependent chain, and two waves per SIMD do not hide it -- 441 cycles per tile and SIMD at d = 32 for 128 cycles of
// MFMA and ~200 of VALU issue (profiles/r05_b: the matrix pipe and the VALU overlap, so the floor is the LARGER of the two, not their sum).  Here a wave
// owns TWO 32-query blocks half a step apart, exactly as in set_attention_sp_kernel: while block A's scores are exponentiated the matrix pipe holds block
// B's PV product and A's next score tile.  At d <= 32 a phase has 4 (d = 32) or 3 (d = 16) MFMAs beside the same 16 exponentials, so the VALU is the
// busy unit (~205 issue cycles per phase: 16 x 8 v_exp_f32 + 8 packs + 8 packed adds) and the MFMAs ride in its shadow.
//   d = 32: K / V tile rows are 64 bytes (4 + 4 one-KB LDS-DMA pieces per 64-key tile, two per wave), one O^T block of 32 rows;
//   d = 16: 32-byte rows (2 + 2 pieces, one per wave); O^T rows 16 .. 31 multiply zeros: the lanes that would read them point into a zeroed LDS region
//           as large as the ring, so the same immediate offsets apply and no lane needs a branch.
// Softmax, rare path, ring, barriers and the XCD-aware block map are set_attention_sp_kernel's.
// rare path: the tile's scores were overwritten by the next tile's (see spn_phase), so they are formed again from K(i), which is still in its ring slot;
// then as sp_fix: raise the running max of the rows that need it, rescale everything that was formed against the old one (O, l, the -m accumulator seed, the
// pending next score tile) and redo this tile's exponentials
template <int D>
__device__ __forceinline__ half2_ spn_fix(const char* (&kaddr)[D / 16], int koff_cur, const half8 (&qf)[D / 16], f32x16& s_nxt, f32x16& negm,
                                          f32x16& o, float& l, half8& p0, half8& p1) {
    f32x16 s_cur = SP_MF(*(const half8*)(kaddr[0] + koff_cur), qf[0], negm);
    if constexpr (D == 32) s_cur = SP_MF(*(const half8*)(kaddr[1] + koff_cur), qf[1], s_cur);
    const float delta = fmaxf(sp_rowmax(s_cur), 0.f);
    const float alpha = __builtin_amdgcn_exp2f(-delta);
    l *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        negm[r] -= delta; s_cur[r] -= delta; s_nxt[r] -= delta;
        o[r] *= alpha;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        p0[j] = (half_t)__builtin_amdgcn_exp2f(s_cur[j]);
        p1[j] = (half_t)__builtin_amdgcn_exp2f(s_cur[8 + j]);
    }
    return sp_tile_sum(p0, p1);
}

// One phase: the VALU work of sp_phase in its eight slices; the OTHER block's PV MFMAs (and mid(), the reload of V behind them) in front of fixed slices, and
// this block's NEXT score tile last, INTO the registers the exponentials have just read (the matrix pipe works on it under the next phase; a separate
// register set for it costs 32 registers = the third wave per SIMD):
//   d = 32:  PV0 | . | PV1 | . | mid | . | . | . | S0 S1           d = 16:  PV0 | . | . | PV1 | . | mid | . | . | S0
template <int D, typename Mid>
__device__ __forceinline__ half2_ spn_phase(f32x16& s, half8& p0, half8& p1, const half8 (&kf)[D / 16], const half8 (&qf)[D / 16],
                                            const f32x16& negm, f32x16& o, const half8 (&vf)[2], const half8& y0, const half8& y1,
                                            half2_ t_other, float& l_other, Mid&& mid) {
#define SPN_PV(j) o = SP_MF(vf[j], (j) ? y1 : y0, o)
#define SPN_SLOT(k)                                                            \
    do {                                                                       \
        SP_SB();                                                               \
        if constexpr ((k) == 0) SPN_PV(0);                                     \
        if constexpr ((k) == (D == 32 ? 2 : 3)) SPN_PV(1);                     \
        if constexpr ((k) == (D == 32 ? 4 : 5)) { mid(); SP_SB(); }            \
    } while (0)
    SPN_SLOT(0);
    const float e0 = __builtin_amdgcn_exp2f(s[0]), e1 = __builtin_amdgcn_exp2f(s[1]);
    SPN_SLOT(1);
    const float e8 = __builtin_amdgcn_exp2f(s[8]), e9 = __builtin_amdgcn_exp2f(s[9]);
    const half2_ c0 = sp_pk(e0, e1);
    SPN_SLOT(2);
    const float e2 = __builtin_amdgcn_exp2f(s[2]), e3 = __builtin_amdgcn_exp2f(s[3]);
    const half2_ c4 = sp_pk(e8, e9);
    SPN_SLOT(3);
    const float e10 = __builtin_amdgcn_exp2f(s[10]), e11 = __builtin_amdgcn_exp2f(s[11]);
    const half2_ c1 = sp_pk(e2, e3);
    const half2_ a0 = c0 + c4;
    SPN_SLOT(4);
    const float e4 = __builtin_amdgcn_exp2f(s[4]), e5 = __builtin_amdgcn_exp2f(s[5]);
    const half2_ c5 = sp_pk(e10, e11);
    SPN_SLOT(5);
    const float e12 = __builtin_amdgcn_exp2f(s[12]), e13 = __builtin_amdgcn_exp2f(s[13]);
    const half2_ c2 = sp_pk(e4, e5);
    const half2_ a1 = c1 + c5;
    SPN_SLOT(6);
    const float e6 = __builtin_amdgcn_exp2f(s[6]), e7 = __builtin_amdgcn_exp2f(s[7]);
    const half2_ c6 = sp_pk(e12, e13);
    const half2_ b0 = a0 + a1;
    SPN_SLOT(7);
    const float e14 = __builtin_amdgcn_exp2f(s[14]), e15 = __builtin_amdgcn_exp2f(s[15]);
    const half2_ c3 = sp_pk(e6, e7);
    const half2_ a2 = c2 + c6;
    const half2_ b1 = b0 + a2;
    SP_SB();
    s = SP_MF(kf[0], qf[0], negm);                             // every score of this tile has been read: the next tile's take their place
    if constexpr (D == 32) s = SP_MF(kf[1], qf[1], s);
    SP_SB();
#undef SPN_SLOT
#undef SPN_PV
    return sp_phase_tail(c0, c1, c2, c3, c4, c5, c6, sp_pk(e14, e15), b1, t_other, l_other, p0, p1);
}

// ABL: timing ablations for tools/bench_attn_small_d.py (pcd_set_attention_config(16 + bits); outputs are wrong while set): 1 = no K/V restaging in the loop,
// 2 = no rare-path test, 4 = no waits / barriers in the loop, 8 = restaging reads the first four tiles over and over (cache-resident sources)
template <int D, int ABL = 0>
__global__ __launch_bounds__(256, 3) void set_attention_spn_kernel(const half_t* __restrict__ qkv, int n, int c, int heads,
                                                                    float scale_log2e, half_t* __restrict__ out) {
    static_assert(D == 32 || D == 16, "d = 64 has set_attention_sp_kernel");
    constexpr int KSTEPS = D / 16, KRB = 2 * D, NSLOT = 4;
    constexpr int KBYTES = KT * KRB, STAGE = 2 * KBYTES;
    constexpr int AHEAD = NSLOT - 2;                          // tiles in flight beyond the one being consumed
    constexpr int RPP = 1024 / KRB;                           // rows of a K / V tile per 1-KB LDS-DMA piece (16 / 32)
    constexpr int CPR = KRB / 16;                             // 16-byte chunks per row (4 / 2)
    constexpr int PPW = 2 * (KT / RPP) / 4;                   // pieces per wave and tile (2 / 1)
    constexpr int ZERO_BYTES = D == 16 ? NSLOT * STAGE : 0;   // d = 16: what the lanes of O^T rows 16 .. 31 read (every ring offset stays inside it)
    __shared__ __attribute__((aligned(16))) char smem[NSLOT * STAGE + ZERO_BYTES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = lane & 31, hh = lane >> 5;
    // XCD-aware block -> (shape, head, query block) map of set_attention_sp_kernel: the n / 256 query blocks of one (shape, head) run on one XCD
    const int nqb = n >> 8;
    int bh, qb;
    {
        const int L = blockIdx.x, total_bh = gridDim.x / nqb;
        const int xcd = L & 7, i = L >> 3;
        const int j = i / nqb;
        bh = xcd + 8 * j;
        qb = i - j * nqb;
        if (bh >= total_bh || (total_bh & 7)) { bh = L / nqb; qb = L - bh * nqb; }
    }
    const int b = bh / heads, head = bh - b * heads;
    const int q0 = qb * 256 + wave * 64;
    const int64_t row_base = (int64_t)b * n;
    const int ld = 3 * c;

    if constexpr (D == 16) {
        typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
        for (int i = tid * 16; i < ZERO_BYTES; i += 256 * 16) *(u32x4_*)(smem + NSLOT * STAGE + i) = (u32x4_){0u, 0u, 0u, 0u};
    }

    const half_t* kbase = qkv + row_base * ld + c + head * D;
    const half_t* vbase = qkv + row_base * ld + 2 * c + head * D;
    const int ntiles = n / KT;                                // a multiple of NSLOT (n % 256 == 0)
    // LDS-DMA staging: a 1-KB piece is RPP rows; lane -> (row lane / CPR of the piece, chunk lane % CPR).  The K swizzle of a row only depends on the row
    // inside its piece (pieces start at multiples of 16 rows), V rows are not swizzled at these row widths: one lane-constant offset each.
    const unsigned lrow = lane / CPR, lch = lane % CPR;
    const unsigned koff32 = lrow * (unsigned)ld * 2u + ((unsigned)k_swz<KRB>((int)lrow, (int)lch) << 4);
    const unsigned voff32 = lrow * (unsigned)ld * 2u + (lch << 4);
    const unsigned lds0 = (unsigned)(size_t)smem;
    const size_t tile_bytes = (size_t)KT * ld * 2;
    // d = 32: wave w moves K piece w and V piece w of a tile (rows 16 w ..); d = 16: waves 0, 1 move K pieces 0, 1, waves 2, 3 V pieces 0, 1 (rows 32 (w & 1) ..)
    const int prow = D == 32 ? 16 * wave : 32 * (wave & 1);
    const char* kwave = (const char*)kbase + (size_t)prow * ld * 2;
    const char* vwave = (const char*)vbase + (size_t)prow * ld * 2;
    // piece j of this wave's PPW pieces of tile kt into ring slot `slot`
    auto stage_piece = [&](int kt, int slot, int j) __attribute__((always_inline)) {
        if constexpr (D == 32) {
            const char* src = (j ? vwave : kwave) + (size_t)kt * tile_bytes;
            sp_dma(src, j ? voff32 : koff32, lds0 + slot * STAGE + (j ? KBYTES : 0) + wave * 1024);
        } else {
            if (j == 0) {
                const bool is_v = wave >= 2;
                const char* src = (is_v ? vwave : kwave) + (size_t)kt * tile_bytes;
                sp_dma(src, is_v ? voff32 : koff32, lds0 + slot * STAGE + (is_v ? KBYTES : 0) + (wave & 1) * 1024);
            }
        }
    };
#pragma unroll
    for (int t = 0; t <= AHEAD; ++t)
#pragma unroll
        for (int j = 0; j < PPW; ++j) stage_piece(t, t, j);

    half8 qA[KSTEPS], qB[KSTEPS];
    {
        const half_t* qpA = qkv + (row_base + q0 + qr) * ld + head * D;
        attn_load_q2(qpA, qpA + (int64_t)32 * ld, hh, scale_log2e, qA, qB);
    }

    // lane-constant LDS addresses (slot 0, key sub-tile 0); every read adds a compile-time offset (the K swizzle of row qr + 32 i is that of row qr)
    const int tq = (lane >> 2) & 3, tp = lane & 3, tg = lane >> 4;
    const char* kaddr[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) kaddr[s] = smem + qr * KRB + (k_swz<KRB>(qr, 2 * s + hh) << 4);
    const char* vaddr;
    {
        const int key = 4 * (tg >> 1) + tq;
        const int ch = ((16 * (tg & 1)) >> 3) + (tp >> 1);
        vaddr = smem + KBYTES + key * KRB + (ch << 4) + (tp & 1) * 8;
        if (D == 16 && (tg & 1)) vaddr = smem + NSLOT * STAGE + (tp & 1) * 8;
    }
    auto load_k = [&](int off, half8 (&kf)[KSTEPS]) __attribute__((always_inline)) {         // off = slot * STAGE + sub * 32 * KRB
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) kf[s] = *(const half8*)(kaddr[s] + off);
    };
    auto load_v = [&](int off, half8 (&vf)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const char* a0 = vaddr + off + 16 * s2 * KRB;
            const fp16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)a0);
            const fp16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)(a0 + 8 * KRB));
#pragma unroll
            for (int e = 0; e < 4; ++e) { vf[s2][e] = (half_t)lo[e]; vf[s2][4 + e] = (half_t)hi[e]; }
        }
    };

    f32x16 oA, oB, negmA, negmB, sA, sB;
    float lA = 0.f, lB = 0.f;
    half8 pA0, pA1, pB0, pB1, kf[KSTEPS], vf[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { oA[r] = oB[r] = 0.f; negmA[r] = negmB[r] = 0.f; }
#pragma unroll
    for (int e = 0; e < 8; ++e) {                              // the first phase's O_B += V(-1)^T P_B(-1) adds zero
        pB0[e] = pB1[e] = (half_t)0.f;
        vf[0][e] = vf[1][e] = (half_t)0.f;
    }

    wait_vmcnt<0>();
    __syncthreads();
    // the first 32 keys fix the running max exactly: S(0) - rowmax, seed accumulators = -rowmax
    load_k(0, kf);
    sA = SP_MF(kf[0], qA[0], negmA);
    sB = SP_MF(kf[0], qB[0], negmB);
#pragma unroll
    for (int s = 1; s < KSTEPS; ++s) { sA = SP_MF(kf[s], qA[s], sA); sB = SP_MF(kf[s], qB[s], sB); }
    {
        const float ma = sp_rowmax(sA), mb = sp_rowmax(sB);
#pragma unroll
        for (int r = 0; r < 16; ++r) { negmA[r] = -ma; sA[r] -= ma; negmB[r] = -mb; sB[r] -= mb; }
    }
    load_k(32 * KRB, kf);                                     // K(1) for the first sub-tile's S(i+1) products

    half2_ tA, tB;                                              // row sums of the last tile of A / B, not yet in lA / lB
    tA.x = tA.y = tB.x = tB.y = (half_t)0.f;
    // one key sub-tile i (32 keys): kf holds K(i+1), vf V(i-1), sA / sB the scores S(i) on entry; V(i) (and K(i), for the rare path) at voff, K(i+2) at koff;
    // when stage_on, piece j of tile st leaves for ring slot sslot in front of the first phase
    auto sub_iter = [&](int voff, int koff, bool stage_on, int st, int sslot, int j) __attribute__((always_inline)) {
        if (!(ABL & 1) && stage_on && j < PPW) stage_piece((ABL & 8) ? (st & 3) : st, sslot, j);
        tA = spn_phase<D>(sA, pA0, pA1, kf, qA, negmA, oB, vf, pB0, pB1, tB, lB, [&]() { load_v(voff, vf); });
        asm volatile("" : "+v"(vf[0]), "+v"(vf[1]));           // V(i) is read HERE (the compiler would sink the reads to their use, the first MFMA of the next phase)
        if (!(ABL & 2) && __builtin_expect(__any(__builtin_bit_cast(unsigned, tA) > SP_BIG_BITS), 0)) tA = spn_fix<D>(kaddr, voff, qA, sA, negmA, oA, lA, pA0, pA1);
        tB = spn_phase<D>(sB, pB0, pB1, kf, qB, negmB, oA, vf, pA0, pA1, tA, lA, [&]() {});
        load_k(koff, kf);                                      // behind the last product that reads K(i+1)
        if (!(ABL & 2) && __builtin_expect(__any(__builtin_bit_cast(unsigned, tB) > SP_BIG_BITS), 0)) tB = spn_fix<D>(kaddr, voff, qB, sB, negmB, oB, lB, pB0, pB1);
    };
    auto tile_group = [&](int t0, auto last_tag) __attribute__((always_inline)) {
        constexpr bool LAST = decltype(last_tag)::value;
#pragma unroll
        for (int u = 0; u < NSLOT; ++u) {
            // tile t+1 has landed (all but the youngest stage's PPW LDS-DMA pieces of this wave), this wave's own fragment reads have returned
            if constexpr (!(ABL & 4)) {
                if (!LAST || u < 2) {
                    if constexpr (PPW == 2) wait_vmcnt_lgkm0<2>();
                    else wait_vmcnt_lgkm0<1>();
                } else {
                    wait_vmcnt_lgkm0<0>();
                }
                __syncthreads();
            }
            const int cur = u * STAGE, nxt = ((u + 1) % NSLOT) * STAGE;   // last tile: nxt holds stale bytes, S(i+1) unused
            const int st = t0 + u + AHEAD + 1, sslot = (u + AHEAD + 1) % NSLOT;   // tile to stage; its slot == slot of tile t-1
            const bool on = !LAST || u == 0;
            sub_iter(cur, nxt, on, st, sslot, 0);
            sub_iter(cur + 32 * KRB, nxt + 32 * KRB, on, st, sslot, 1);
        }
    };
    int t0 = 0;
    for (; t0 + NSLOT < ntiles; t0 += NSLOT) tile_group(t0, std::false_type{});
    tile_group(t0, std::true_type{});
    oB = SP_MF(vf[0], pB0, oB);                               // O_B += V(last)^T P_B(last)
    oB = SP_MF(vf[1], pB1, oB);

    // epilogue: lane (query qr, half hh) holds O^T rows dd = (r & 3) + 8 (r >> 2) + 4 hh
    auto store = [&](const f32x16& o, float l, int qi) {
        const float l_tot = l + __shfl_xor(l, 32);
        const float inv = 1.f / l_tot;
        half_t* orow = out + (row_base + qi) * c + head * D;
#pragma unroll
        for (int g = 0; g < D / 8; ++g) {
            half4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = to_half_sat(o[4 * g + e] * inv);
            *(half4*)(orow + 8 * g + 4 * hh) = ov;
        }
    };
    store(oA, lA, q0 + qr);
    store(oB, lB + (float)tB.x, q0 + 32 + qr);                 // B's last tile sum is still pending (A's went in with B's last phase)
}


}  // namespace pcd

using namespace pcd;

extern "C" int pcd_layernorm_f16(const void* x, int64_t rows, int c, const float* gamma, const float* beta,
                                 void* out, void* stream) {
    PCD_CHECK_ARG(x && gamma && beta && out && rows > 0 && c > 0);
    hipStream_t s = (hipStream_t)stream;
    const half_t* x16 = (const half_t*)x; half_t* o16 = (half_t*)out;
    const bool vec = ln_launch(c, [&](auto lpr) {
        hipLaunchKernelGGL((layernorm_rows_kernel<decltype(lpr)::value, false>), dim3(ln_row_blocks(rows, c)), dim3(256), 0, s, x16, rows, gamma, beta, o16,
                           (float*)nullptr, (float*)nullptr);
    });
    if (!vec) hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, x16, rows, c, gamma, beta, o16);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

extern "C" size_t pcd_set_attention_workspace_bytes(int batch, int n_points, int c) {
    (void)batch; (void)n_points; (void)c;
    return 0;   // V is transposed on the fly by ds_read_b64_tr_b16: no workspace needed any more
}

// tuning / testing hooks, set through pcd_set_attention_config
struct AttnConfig {
    int force_generic = 0;   // 1 = always the round-1 generic kernel (running max), 2 = always the max-free generic kernel
    int abl = 0;             // timing ablations of the pipelined kernels (code 16 + bits); outputs are wrong while set
    int sp_waves = 4;        // codes 5 / 6: set_attention_sp_kernel with 4 / 8 waves per workgroup
    int spn = 1;             // codes 3 / 4: d = 32 / 16 on the software-pipelined kernel: off / on (default)
};
static AttnConfig g_attn_config;

extern "C" int pcd_set_attention_config(int force_generic) {
    AttnConfig& cfg = g_attn_config;
    if (force_generic == 3 || force_generic == 4) { cfg.spn = force_generic == 4; return PCD_OK; }
    if (force_generic == 5 || force_generic == 6) { cfg.sp_waves = force_generic == 6 ? 8 : 4; return PCD_OK; }
    if (force_generic >= 16 && force_generic < 32) { cfg.abl = force_generic - 16; return PCD_OK; }
    cfg.force_generic = force_generic < 0 ? 0 : (force_generic > 2 ? 2 : force_generic);
    return PCD_OK;
}

static const char* g_attn_last_kernel = "";   // which kernel the last pcd_set_attention_f16 call launched (bench.py reports it)

extern "C" const char* pcd_set_attention_last_kernel(void) { return g_attn_last_kernel; }

// Every kernel of the family takes (qkv, n, c, heads, scale_log2e, out): which one runs, on what grid and under which name
// is a function of the shape and the hooks alone.
typedef void (*AttnKernel)(const half_t*, int, int, int, float, half_t*);
struct AttnPlan { AttnKernel kernel; dim3 grid, block; const char* name; };

// the timing-ablation instantiations of the pipelined kernels; a (d, code) without an entry runs the default kernel
struct AttnAblation { int d, code; AttnKernel kernel; };
static const AttnAblation kAttnAblations[] = {
    {64, 1, set_attention_sp_kernel<1>}, {64, 2, set_attention_sp_kernel<2>}, {64, 3, set_attention_sp_kernel<3>}, {64, 8, set_attention_sp_kernel<8>},
    {32, 1, set_attention_spn_kernel<32, 1>}, {32, 2, set_attention_spn_kernel<32, 2>}, {32, 3, set_attention_spn_kernel<32, 3>},
    {32, 7, set_attention_spn_kernel<32, 7>}, {32, 8, set_attention_spn_kernel<32, 8>},
    {16, 1, set_attention_spn_kernel<16, 1>}, {16, 2, set_attention_spn_kernel<16, 2>}, {16, 3, set_attention_spn_kernel<16, 3>},
    {16, 7, set_attention_spn_kernel<16, 7>}, {16, 8, set_attention_spn_kernel<16, 8>},
};

static AttnPlan attn_plan(int batch, int n, int d, int heads, const AttnConfig& cfg) {
    const int di = d == 16 ? 0 : d == 32 ? 1 : 2;
    if (cfg.force_generic == 0 && n % 256 == 0 && (d == 64 || cfg.spn)) {
        // software-pipelined kernels: 64 queries per wave, 256 per workgroup of four waves
        static const AttnKernel kernels[3] = {set_attention_spn_kernel<16>, set_attention_spn_kernel<32>, set_attention_sp_kernel<0, 4>};
        static const char* const names[3] = {"set_attention_spn_kernel<16>", "set_attention_spn_kernel<32>", "set_attention_sp_kernel"};
        const dim3 grid((unsigned)((n / 256) * batch * heads));
        for (const AttnAblation& a : kAttnAblations)
            if (a.d == d && a.code == cfg.abl) return {a.kernel, grid, dim3(256), d == 64 ? names[2] : "set_attention_spn_kernel (timing ablation)"};
        if (d == 64 && cfg.sp_waves == 8 && n % 512 == 0) return {set_attention_sp_kernel<0, 8>, dim3(grid.x / 2), dim3(512), names[2]};
        return {kernels[di], grid, dim3(256), names[di]};
    }
    // every other shape (n not a multiple of 256, or the pipelined kernels switched off): one 32-query block per wave, 128 per workgroup.
    // (Two blocks per wave measured slower here, 764 v. 836 TFLOP/s at d = 64: 256 VGPRs, and the shared K/V fragments do not pay for the lost occupancy.)
    static const AttnKernel kernels[2][3] = {
        {set_attention_generic_kernel<16, AttnSoftmax::MaxFree>, set_attention_generic_kernel<32, AttnSoftmax::MaxFree>,
         set_attention_generic_kernel<64, AttnSoftmax::MaxFree>},
        {set_attention_generic_kernel<16, AttnSoftmax::RunningMax>, set_attention_generic_kernel<32, AttnSoftmax::RunningMax>,
         set_attention_generic_kernel<64, AttnSoftmax::RunningMax>}};
    static const char* const names[2][3] = {{"set_attention_om_kernel<16>", "set_attention_om_kernel<32>", "set_attention_om_kernel<64>"},
                                            {"set_attention_kernel<16>", "set_attention_kernel<32>", "set_attention_kernel<64>"}};
    const int round1 = cfg.force_generic == 1;
    return {kernels[round1][di], dim3((unsigned)ceil_div(n, 128), (unsigned)(batch * heads)), dim3(256), names[round1][di]};
}

extern "C" int pcd_set_attention_f16(const void* qkv, int batch, int n_points, int c, int heads, void* out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    PCD_CHECK_ARG(qkv && out && batch > 0 && n_points > 0 && heads > 0 && c % heads == 0);
    const int d = c / heads;
    PCD_CHECK_ARG(d == 16 || d == 32 || d == 64);
    PCD_CHECK_ARG(c % 8 == 0);
    const float scale_log2e = 1.4426950408889634f / sqrtf((float)d);
    const AttnPlan plan = attn_plan(batch, n_points, d, heads, g_attn_config);
    hipLaunchKernelGGL(plan.kernel, plan.grid, plan.block, 0, (hipStream_t)stream, (const half_t*)qkv, n_points, c, heads, scale_log2e, (half_t*)out);
    g_attn_last_kernel = plan.name;
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}
