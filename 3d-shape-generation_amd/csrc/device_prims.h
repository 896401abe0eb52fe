// Device primitives shared by the kernels of this library (included from common.h): the LDS-DMA instruction, counted waits, the weight-image ring
// of the register-resident chains, LayerNorm and regrouping on MFMA fragments, the swizzled 32 x 128-byte image, block reductions and scans, Philox.  One definition
// of each: an invariant found in one kernel is kept for all of them here.
#pragma once

namespace pcd {

// ------------------------------------------------------------------------------------------------ LDS-DMA
// 16 bytes per lane (1 KiB per wave-instruction): global `g` (per-lane address) -> LDS at the wave-uniform byte address `lds_addr` + lane * 16.
// Issued from inline asm.  The compiler models the builtin form (lds_dma16_builtin) as a FLAT access that may touch both memory and LDS: while one
// is pending it turns every later s_waitcnt into vmcnt(0) / lgkmcnt(0) and puts a vmcnt(0) in front of LDS reads it cannot prove disjoint
// (ds_read_b64_tr_b16), which drains a DMA meant to stay in flight over several stages (+25 % on the implicit-GEMM convolution, where it was found;
// +0.7-1 % on the point U-Net's step).  From asm the DMA is invisible to that bookkeeping: the caller owns the `s_waitcnt vmcnt` and the barrier
// that make the bytes visible.
__device__ __forceinline__ void lds_dma16(const void* g, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds_addr) : "memory", "m0");
}
// the same with an LDS pointer the compiler does not know to be wave-uniform
__device__ __forceinline__ void lds_dma16(const void* g, const void* lds_wave_base) {
    lds_dma16(g, (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(size_t)lds_wave_base));
}
// the builtin form: the compiler tracks the DMA and places the waits itself
__device__ __forceinline__ void lds_dma16_builtin(const void* g, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// ------------------------------------------------------------------------------------------------ counted waits
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// Before a barrier behind which ANOTHER wave's LDS-DMA refills the ring stage this wave has just read: the wave's own ds_reads must have
// RETURNED, not just been issued.  The compiler sinks a stage's last MFMAs (and the lgkmcnt wait in front of them) below the raw s_barrier,
// so a wave would pass it with fragment reads of that stage still queued in the LDS pipe; nothing orders them against the DMA's write, and with
// two workgroups per CU queueing reads and L1-resident weights coming back fast the write did win now and then (conv3d_k4s2_halo_kernel, batch 16:
// one encode in seven differed from the others by 1e-3..5e-3; tools/diag_vae_batch.py).  tools/check_barrier_reads.py scans the built code for it.
__device__ __forceinline__ void wait_lgkm0() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmcnt_lgkm0() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// ------------------------------------------------------------------------------------------------ the weight-image ring
// A workgroup of eight waves streams a cyclic sequence of `period` stage images of STAGE bytes (fragment order, 1-KiB pieces) from `images` through
// RING LDS slots at the start of its dynamic LDS; stage n of the workgroup's run is image n % period in slot n % RING.  Protocol, per stage n:
//     wait(n)       this wave's share of stage n has landed and its LDS reads of stage n - 1 have RETURNED (wait_lgkm0 above: the refill of that slot is
//                   issued right behind the barrier, by any wave); the barrier publishes stage n and retires stage n - 1 for all waves;
//     issue(n + 2)  refills the slot of stage n - 1; stage n + 1 stays in flight;
//     slot(n)       this lane's 16 bytes of piece 0 of stage n (piece i is i * 1024 bytes further).
// acquire(n) is the three in that order; issue(0) and issue(1) prime the ring.  Who requests a piece does not enter the arithmetic:
//     split == false  every wave requests PPW pieces of every stage and waits with PPW pieces (those of stage n + 1) in flight, vmcnt(0) at the last stage;
//     split == true   ONE wave of each SIMD requests 2 PPW pieces (waves 0-3 for even stages, 4-7 for odd ones), so that its SIMD partner issues MFMAs
//                     meanwhile: a piece holds its wave's issue for 60-180 cycles.  The group that requested stage n waits for all its loads, the other
//                     group's pieces (stage n + 1) stay in flight.
// `split` is a constant in the kernels that choose the form at compile time.  The members mirror the closures this struct replaced (what they captured by
// reference is a reference here), and a kernel whose acquire was a closure over its stage counter keeps one around acquire(n): with anything else the kernels
// compile to other register numbers or instruction orders (profiles/device_prims_isa.md).  wide_ffn_kernel (wideffn.hip) spells the protocol out itself.
template <int STAGE, int PPW, int RING = 3>
struct StageRing {
    const char* const& images;              // the kernel parameter: re-read from the kernarg segment where a stage is requested
    char* const& lds;                       // the kernel's dynamic LDS array
    const int& total;                       // stages of this workgroup's run
    const int& wave; const int& lane;
    int period;                             // images per cycle
    const bool& split;

    __device__ __forceinline__ void issue(int n) const {
        if (n < total) {
            if (split) {
                if ((wave >> 2) == (n & 1)) {
                    const int w4 = wave & 3;
                    const char* src = images + (size_t)(n % period) * STAGE + (size_t)(2 * PPW * w4) * 1024 + lane * 16;
                    const unsigned dst = (unsigned)(size_t)lds + (n % RING) * STAGE + (2 * PPW * w4) * 1024;
#pragma unroll
                    for (int i = 0; i < 2 * PPW; ++i) lds_dma16(src + i * 1024, dst + i * 1024);
                }
            } else {
                const char* src = images + (size_t)(n % period) * STAGE + (size_t)(PPW * wave) * 1024 + lane * 16;
                const unsigned dst = (unsigned)(size_t)lds + (n % RING) * STAGE + (PPW * wave) * 1024;
#pragma unroll
                for (int i = 0; i < PPW; ++i) lds_dma16(src + i * 1024, dst + i * 1024);
            }
        }
    }
    __device__ __forceinline__ void wait(int n) const {
        if (split) {
            if ((wave >> 2) == (n & 1)) wait_vmcnt_lgkm0<0>();
            else wait_lgkm0();
        } else if (n + 1 < total) wait_vmcnt_lgkm0<PPW>();
        else wait_vmcnt_lgkm0<0>();
        __syncthreads();
    }
    __device__ __forceinline__ const char* slot(int n) const { return lds + (n % RING) * STAGE + lane * 16; }
    __device__ __forceinline__ const char* acquire(int n) const {
        wait(n);
        issue(n + 2);
        return slot(n);
    }
};

// ------------------------------------------------------------------------------------------------ MFMA fragments: regroup, LayerNorm
// v0 / v1: the four values (already biased / normalised / clamped) of accumulator groups 2 gp and 2 gp + 1 of one 32-channel tile of a transposed
// product D[channel][point] on v_mfma_f32_32x32x16_f16 (register 4 g + e = channel 8 g + 4 hh + e of the tile, point = lane & 31, hh = lane >> 5).
// Lane half 0 ends with the tile's channels 16 gp .. + 7, lane half 1 with 16 gp + 8 .. + 15: the next product's B fragment / one 16-byte output piece.
__device__ __forceinline__ void swap_halves(unsigned p, unsigned q, unsigned& lo, unsigned& hi) {
    // registers P = (half 0: X0, half 1: X1), Q = (half 0: Y0, half 1: Y1)  ->  (X0, Y0) and (X1, Y1): swap P's upper lanes with Q's lower lanes
    const auto r = __builtin_amdgcn_permlane32_swap(p, q, false, false);
    lo = r[0];                  // half 0: X0, half 1: Y0
    hi = r[1];                  // half 0: X1, half 1: Y1
}
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ half8 regroup_swap(const float (&v0)[4], const float (&v1)[4]) {
    unsigned f[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        half2_ pa, pb;
        pa.x = (half_t)v0[2 * h]; pa.y = (half_t)v0[2 * h + 1];
        pb.x = (half_t)v1[2 * h]; pb.y = (half_t)v1[2 * h + 1];
        swap_halves(__builtin_bit_cast(unsigned, pa), __builtin_bit_cast(unsigned, pb), f[h], f[2 + h]);
    }
    return __builtin_bit_cast(half8, (u32x4_t){f[0], f[1], f[2], f[3]});
}
// the same with the groups' values as packed fp16 pairs
__device__ __forceinline__ half8 regroup_swap(const unsigned (&p)[2], const unsigned (&q)[2]) {
    unsigned f[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) swap_halves(p[h], q[h], f[h], f[2 + h]);
    return __builtin_bit_cast(half8, (u32x4_t){f[0], f[1], f[2], f[3]});
}

// from the accumulators of the tile: + bias_t[channel of the tile], clamped to [lo, 65504] (lo = 0: ReLU)
__device__ __forceinline__ half8 regroup_bias_clamp(const f32x16& acc, int gp, const float* bias_t, int hh, float lo) {
    const int g0 = 2 * gp, g1 = 2 * gp + 1;
    unsigned p[2], q[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float a0 = acc[4 * g0 + 2 * h] + bias_t[8 * g0 + 4 * hh + 2 * h], a1 = acc[4 * g0 + 2 * h + 1] + bias_t[8 * g0 + 4 * hh + 2 * h + 1];
        const float b0 = acc[4 * g1 + 2 * h] + bias_t[8 * g1 + 4 * hh + 2 * h], b1 = acc[4 * g1 + 2 * h + 1] + bias_t[8 * g1 + 4 * hh + 2 * h + 1];
        half2_ pa, pb;
        pa.x = (half_t)__builtin_amdgcn_fmed3f(a0, lo, 65504.f); pa.y = (half_t)__builtin_amdgcn_fmed3f(a1, lo, 65504.f);
        pb.x = (half_t)__builtin_amdgcn_fmed3f(b0, lo, 65504.f); pb.y = (half_t)__builtin_amdgcn_fmed3f(b1, lo, 65504.f);
        p[h] = __builtin_bit_cast(unsigned, pa);
        q[h] = __builtin_bit_cast(unsigned, pb);
    }
    return regroup_swap(p, q);
}

// LayerNorm (eps 1e-5) of a point's C channels held as B fragments: lane (point, hh = lane >> 5) holds the 8 channels 16 s + 8 hh .. + 7 of every k-step s, lane ^ 32
// the others.  fp32 statistics, result in fp16 like pcd_layernorm_f16's.
// Two passes, the variance about the mean: sum(x^2) - C mean^2 cancels when |mean| >> std (post-ReLU rows near the fp16 range).  The sum straight from the
// packed fp16 pairs by v_dot2_f32_f16 with fp32 accumulation.  The second pass forms x - mean in fp32, element by element, the arithmetic of the plain kernels
// (attention.hip, attn_bwd.hip): |x - mean| reaches 131008 on finite rows (all +65504, one -65504), so no fp16 holds it.  A packed x - fp16(mean) is inf from
// 65520 on, which made sq inf, rstd 0 and the whole row beta (three quarters of a row near -30000, one quarter near +60000 did that); halved inside a packed
// fma it stays finite but is rounded to 11 bits, and on a row that is one outlier above a flat bulk that rounding alone moves rstd by 2.4e-4 and the row of
// a following Linear by 9.5e-4 (tests/test_gpu_layernorm_rows.py holds every row to 1e-3 of fp64).
// The pass streams: each difference is used once, one v_fma_mix_f32 (x - sum / C, the conversion inside it; sum / C is exact) and one v_fmac_f32 per
// element.  It reads the sum through `sum2`, an identity DPP move: the same bits, but not the same value to the compiler, which would otherwise keep the
// differences for the third pass, where x - mean appears again: no converted copy of the fragments stays alive (C / 2 more registers, a spill at C = 256).
// A move, not an empty asm: the timing ablations of wide_ffn_kernel that drop the MFMAs must still lose the whole LayerNorm as dead code.
// A macro, not a function: a function is simplified on its own before it is inlined (with hh a parameter of unknown range, the 4 C / 16 reads of the affine
// each get an address register: 92 more instructions at C = 256), and even with that mended the kernels' instruction streams come out reordered.
// frag: half8 [C / 16], normalised in place; gamma + goff, beta + boff: const float* (LDS), C floats each, base and offset apart because the two
// spellings of the same address do not compile to the same stream; hh = lane >> 5.
#define PCD_LN_FRAGMENTS(frag, C, gamma, goff, beta, boff, hh)                                                                                        \
    do {                                                                                                                                              \
        float sum = 0.f, sq = 0.f;                                                                                                                    \
        half2_ one2; one2.x = one2.y = (half_t)1.f;                                                                                                   \
        _Pragma("unroll") for (int s = 0; s < (C) / 16; ++s)                                                                                          \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                                           \
                half2_ v; v.x = (frag)[s][2 * e]; v.y = (frag)[s][2 * e + 1];                                                                         \
                sum = __builtin_amdgcn_fdot2(v, one2, sum, false);                                                                                    \
            }                                                                                                                                         \
        sum += __shfl_xor(sum, 32);                                                                                                                   \
        const float mean = sum * (1.f / (C));                                                                                                         \
        const float sum2 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, sum), 0xE4, 0xF, 0xF, false));                  \
        _Pragma("unroll") for (int s = 0; s < (C) / 16; ++s)                                                                                          \
            _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                                           \
                const float d = (float)(frag)[s][e] - sum2 * (1.f / (C));                                                                             \
                sq = __builtin_fmaf(d, d, sq);                                                                                                        \
            }                                                                                                                                         \
        sq += __shfl_xor(sq, 32);                                                                                                                     \
        const float rstd = rsqrtf(sq * (1.f / (C)) + 1e-5f);                                                                                          \
        _Pragma("unroll") for (int s = 0; s < (C) / 16; ++s) {                                                                                        \
            const f32x4 g0 = *(const f32x4*)&(gamma)[(goff) + 16 * s + 8 * (hh)], g1 = *(const f32x4*)&(gamma)[(goff) + 16 * s + 8 * (hh) + 4];                         \
            const f32x4 b0 = *(const f32x4*)&(beta)[(boff) + 16 * s + 8 * (hh)], b1 = *(const f32x4*)&(beta)[(boff) + 16 * s + 8 * (hh) + 4];                           \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                                           \
                (frag)[s][e] = (half_t)__builtin_amdgcn_fmed3f(((float)(frag)[s][e] - mean) * rstd * g0[e] + b0[e], -65504.f, 65504.f);               \
                (frag)[s][4 + e] = (half_t)__builtin_amdgcn_fmed3f(((float)(frag)[s][4 + e] - mean) * rstd * g1[e] + b1[e], -65504.f, 65504.f);       \
            }                                                                                                                                         \
        }                                                                                                                                             \
    } while (0)

// ------------------------------------------------------------------------------------------------ the swizzled [32 rows][128 B] image
// A 64-deep K chunk of 32 rows of a row-major fp16 matrix as a 4-KiB LDS image filled by four 1-KiB LDS-DMA instructions in full 128-byte lines (8 rows
// each), with the XOR swizzle of the attention K tile on the source address so that the ds_read_b128 fragment reads are conflict free.
__device__ __forceinline__ int swz128(int row, int ch) { return ch ^ ((row >> 1) & 7); }

// instruction i of 4 (rows 8 i .. 8 i + 7) of rows [row0, row0 + 32) at halfs column k0 of base[rows][ld] into the image at `img`
__device__ __forceinline__ void stage_rows32x128(const half_t* base, int64_t ld, int row0, int k0, char* img, int i, int lane) {
    const int row = 8 * i + (lane >> 3), ch = lane & 7;
    lds_dma16(base + (int64_t)(row0 + row) * ld + k0 + swz128(row, ch) * 8, img + i * 1024);
}
// the same with the rows clamped to `row_limit - 1`
__device__ __forceinline__ void stage_rows32x128(const half_t* base, int64_t ld, int row0, int row_limit, int k0, char* img, int i, int lane) {
    const int row = 8 * i + (lane >> 3), ch = lane & 7;
    int gr = row0 + row;
    gr = gr < row_limit ? gr : row_limit - 1;
    lds_dma16(base + (int64_t)gr * ld + k0 + swz128(row, ch) * 8, img + i * 1024);
}

// the 8 halfs of row `row`, chunk 4 hh + j: the 32x32x16 operand fragment of k-step j (lane = row + 32 hh)
__device__ __forceinline__ half8 frag128(const char* img, int row, int hh, int j) {
    return *(const half8*)(img + row * 128 + (swz128(row, 4 * hh + j) << 4));
}

// ------------------------------------------------------------------------------------------------ block reductions
struct MaxOp { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct MinOp { __device__ float operator()(float a, float b) const { return fminf(a, b); } };
struct SumOp { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };

// butterfly over the wave: every lane ends with the same bits
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}

// Fixed order: the butterfly, then the waves in order, ((w0 op w1) op w2) op ...; every thread gets the result.  The barrier in front lets a kernel
// use one scratch array for reduction after reduction.  WAVES = 0 reads the wave count from blockDim; a kernel launched with 64 WAVES threads
// may name it, which unrolls the last loop.
template <int WAVES = 0, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* scratch /* [waves] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    T r = scratch[0];
    for (int w = 1; w < (WAVES > 0 ? WAVES : (int)(blockDim.x >> 6)); ++w) r = op(r, scratch[w]);
    return r;
}

// ------------------------------------------------------------------------------------------------ block scans
// Running sums of one value per thread over a workgroup of 64 WAVES threads, in thread order; wsum: WAVES values of LDS.  Two forms: their
// barriers and their costs differ, and a caller relies on the one it has.
//
// Inclusive; total = the sum.  Wave 0 scans the wave sums.  Two barriers inside; the caller puts one more between the last use of `total` and
// the next call.  A fixed tree: the lanes of a wave, then the waves, then (sum within this wave) + (wave sums before it).
template <int WAVES, typename T>
__device__ __forceinline__ T block_scan_incl(T v, T* wsum, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    if (wave == 0) {
        T t = lane < WAVES ? wsum[lane] : T(0);
#pragma unroll
        for (int o = 1; o < WAVES; o <<= 1) {
            const T y = __shfl_up(t, o);
            if (lane >= o) t += y;
        }
        if (lane < WAVES) wsum[lane] = t;
    }
    __syncthreads();
    total = wsum[WAVES - 1];
    return x + (wave ? wsum[wave - 1] : T(0));
}

// Exclusive; *total (if given) = the sum.  A barrier in front and every thread adds the wave sums itself: safe to call back to back.
template <int WAVES, typename T>
__device__ __forceinline__ T block_scan_excl(T v, T* wsum, T* total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T s = wsum[w];
        if (w < wave) before += s;
        all += s;
    }
    if (total) *total = all;
    return before + incl - v;
}

// the least l in [0, last] with c[l] > target, `last` if there is none: the owner of `target` in the non-decreasing running sums c
template <typename T>
__device__ __forceinline__ int first_above(const T* c, int last, T target) {
    int l = 0, h = last;
    while (l < h) {
        const int m = (l + h) >> 1;
        if (c[m] > target) h = m; else l = m + 1;
    }
    return l;
}

// the count of ragged cloud p, clamped to its padded rows
__device__ __forceinline__ int clamped_count(const int* n, int p, int cap) {
    const int v = n[p];
    return v < 0 ? 0 : (v > cap ? cap : v);
}

// ------------------------------------------------------------------------------------------------ Philox4x32-10
// One round; counter c, key (k0, k1).  The stream of a 64-bit counter `ctr` under a 64-bit `seed`: c = {lo(ctr), hi(ctr), 0, 0}, key = {lo(seed), hi(seed)},
// ten rounds with the key bumped by (0x9E3779B9, 0xBB67AE85) after each.
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// the four 32-bit words of counter `ctr`
__device__ __forceinline__ void philox_words4(uint64_t ctr, uint64_t seed, uint32_t (&c)[4]) {
    c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = 0u; c[3] = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// Philox4x32-10 on counter `ctr` + Box-Muller: the 4 standard normals of one counter
__device__ __forceinline__ void philox_normals4(uint64_t ctr, uint64_t seed, float (&v)[4]) {
    uint32_t c[4];
    philox_words4(ctr, seed, c);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);      // (0,1)
        const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float r = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincosf(6.28318530717958647692f * u2, &sn, &cs);
        v[2 * h] = r * cs;
        v[2 * h + 1] = r * sn;
    }
}

}  // namespace pcd
