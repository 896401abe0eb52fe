// Row-panel chains: consecutive 512-channel-input store layers of the point U-Net as ONE launch, with the activations of a 128-row panel resident in
// LDS from the chain's input to its last layer.
//
//   E4   enc4.conv1 512->512, conv2 512->512, conv3 512->1024     x3 [M][512] -> x4 [M][1024]     (lin 8, 9, 10)
//   D3T  dec3.conv2 512->512, conv3 512->256                      [M][512]    -> [M][256]         (lin 17, 18)
//   D43  dec4.conv3 1024->512, dec3.conv1 [. | x3] 1024->512, dec3.conv2, conv3      [M][1024], x3 [M][512] -> [M][256]     (lin 15, 16, 17, 18)
//
// As per-layer launches (gemm_xs_kernel) each of these layers ends every round of tiles in a store burst and the next layer reads the same bytes back:
// at K = 512 a tile is 8 K tiles long and the layers run nearer their HBM bound than their MFMA bound.  Here a workgroup (8 waves, one per CU,
// persistent) owns 128 rows and ALL 512 output channels of a layer:
//   panel     [8 K tiles][128 rows][128 B] fp16 = 128 KB, the K-tile images of the staged GEMMs (chunk ^ ((row >> 1) & 7)), filled once per tile by 128
//             LDS-DMA pieces (16 per wave, whole 1-KB input rows).  Every layer reads its activation fragments from it: no fills and no barrier inside
//             a K loop.
//   waves     1 x 8: wave w owns all 128 rows x columns 64 w .. + 63 (MI = 8, NI = 4: 128 accumulators, the wave tile of the 256 x 256 kernels).  The
//             256-channel layer runs 2 x 4 (64 rows x 64 columns, MI = 4) so that no wave idles; the 1024-channel layer is two passes of 512 columns.
//   weights   straight from global memory into the MFMA operand registers, from pcd_gemm_pack_wfrag's fragment-order copies: wave w reads column tile
//             w >> 2, wave column w & 3 -- 8 KB per wave and K tile, each line once per CU.  One set of registers: a k step's four are reloaded with the
//             same k step of the NEXT K tile (of the next pass, of the next tile's first pass) as soon as its MFMAs are issued; counted vmcnt waits.
//   hand-over barrier (every wave has read the panel), bias + ReLU + clamp-and-pack on the accumulators, ds_write_b128 of the fp16 rows into K-tile image w
//             of the SAME panel (wave w's 64 columns are K tile w of the next layer), barrier.  In place because the accumulators hold the whole panel.
//   output    the last layer's passes leave through a 2-KB LDS slot per wave that turns sixteen rows x two 64-byte halves into two runs of eight whole
//             128-byte lines (the drip layout of gemm_xs_kernel), stored behind the next tile's panel request.
//   rolling   a K-tile image is free once every wave has read it; a pass that "rolls" has a barrier in front of each K tile (the wave's LDS reads
//             drained first), and behind the barrier of K tile kt every wave refills ITS two 1-KB pieces of image kt - 1 with K tile kt - 1 of the next
//             consumer.  Two uses.  (a) The last pass of a tile refills the panel with the NEXT tile's rows (image 7 at the pass's end), so the tile
//             boundary has no panel-sized burst to wait for; a workgroup's last tile re-requests its own rows, so that every wait keeps its count.
//             (b) A layer with K = 1024 (D43's first two) reads K tiles 0-7 from the resident images while K tiles 8-15 -- columns 512 .. 1023 of the
//             same input rows, or x3 -- roll into the freed images, and reads those from there: K tile 8 + j is image j.  A piece is requested one K
//             tile before the wave's next counted wait retires it (vmcnt is in order) and is published by the barrier after that.
// The products are v_mfma_f32_16x16x32_f16 with the weights as A and the activations as B (an accumulator = 4 consecutive channels of one point), k
// ascending in k steps of 32, then bias, ReLU and the fp16 clamp as in gemm_xs_kernel: every stored value is bitwise what the per-layer launches give.
//
// Issue order per wave, which the counted waits name (vmcnt retires loads and stores in order):
//   k step s:  [wait: step s landed]  MFMAs  [step s + 2 requested]
//   a rolling K tile:  barrier | pieces x 2 | k step | k step
//   a storing pass ends:  ... step next0 x 4 | step next1 x 4 | (tile end: pieces x 2) | stores x NST
// so a k step waits with the 4 loads of the following step outstanding (6 in a K tile that requested pieces), and the first two k steps behind a storing
// pass with 4 + NST.
//
// Registers (hipcc --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): no AGPRs, no scratch (192 VGPRs are accumulators and operands); the counts
// per instance are in profiles/panel_chain_dec.md.  LDS: 128 KB panel + 16 KB output slots + the biases (8 / 3 / 7 KB).  Measurements: profiles/panel_chain.md,
// profiles/panel_chain_dec.md.
#include <type_traits>
#include "common.h"

namespace pcd {

namespace {

constexpr int PC_ROWS = 128, PC_K = 512, PC_NK = 8, PC_THREADS = 512;
constexpr int PC_PANEL = PC_ROWS * PC_K * 2;               // 131072
constexpr int PC_SLOTS = 8 * 2048;                         // the waves' output slots
constexpr int PC_MAXL = 4, PC_NCHAIN = 3;
constexpr bool PC_ROLL_NEXT = true;                        // the last pass of a tile rolls the next tile's panel in (see "rolling" above)

// a pass: 512 (or 256) output columns of one layer over the resident panel.  half2: where K tiles 8 .. 15 of a K = 1024 layer come from (0: K = 512)
enum { PC_H2_NONE = 0, PC_H2_XHI = 1, PC_H2_X2 = 2 };       // columns 512 .. 1023 of the input rows | the second input [m][512]
struct PcPass { int layer, col0, two_by_four, store, half2; };
struct PcChain { int nlayers, c[PC_MAXL], k[PC_MAXL], npass; PcPass pass[4]; int c_out, ldx; };
constexpr PcChain PC_CHAIN[PC_NCHAIN] = {
    {3, {512, 512, 1024, 0}, {512, 512, 512, 0}, 4, {{0, 0, 0, 0, 0}, {1, 0, 0, 0, 0}, {2, 0, 0, 1, 0}, {2, 512, 0, 1, 0}}, 1024, 512},               // E4
    {2, {512, 256, 0, 0}, {512, 512, 0, 0}, 2, {{0, 0, 0, 0, 0}, {1, 0, 1, 1, 0}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}}, 256, 512},                       // D3T
    {4, {512, 512, 512, 256}, {1024, 1024, 512, 512}, 4,
     {{0, 0, 0, 0, PC_H2_XHI}, {1, 0, 0, 0, PC_H2_X2}, {2, 0, 0, 0, 0}, {3, 0, 1, 1, 0}}, 256, 1024},                                                 // D43
};
constexpr int pc_bias_off(int chain, int layer) {
    int o = 0;
    for (int l = 0; l < layer; ++l) o += PC_CHAIN[chain].c[l];
    return o;
}
constexpr int pc_lds_bytes(int chain) { return PC_PANEL + PC_SLOTS + pc_bias_off(chain, PC_CHAIN[chain].nlayers) * 4; }

struct PcParams {
    const half_t* x;                    // [m][ldx]: 512 wide, or 1024 (D43: the panel is its columns 0 .. 511, the second K half of the first layer the rest)
    const half_t* x2;                   // D43: [m][512], the second K half of the second layer
    const half_t* frag[PC_MAXL];        // pcd_gemm_pack_wfrag copies
    const float* bias[PC_MAXL];
    half_t* out; int ldo;               // [m][ldo]
    int tiles;
};

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ const half_t* pc_uniform(const half_t* q) {
    const uint64_t v = (uint64_t)q;
    return (const half_t*)(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v));
}
// LDS-DMA, 16 bytes per lane: scalar base + the lane's 32-bit offset -> LDS at lds_addr + lane * 16.  (No immediate offset: the instruction adds it to the
// LDS address as well as to the global one.)
__device__ __forceinline__ void pc_dma16(unsigned voff, const half_t* sbase, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory", "m0");
}
__device__ __forceinline__ void pc_store16(unsigned voff, u32x4_t data, const half_t* sbase) {
    // (s_nop 1: on gfx940 and later a VALU write of the data registers needs TWO wait states behind a > 8-byte store, and the compiler does not look into
    // the asm.  With one, the passes whose stores are followed at once by the next chunk's arithmetic in the same registers stored a few wrong 16-byte
    // pieces per tile.)
    asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(voff), "v"(data), "s"(sbase) : "memory");
}
// four fp32 values clamped to [0, 65504] -> two packed fp16 pairs: the arithmetic of PCD_GEMM_CLAMP_PACK (gemm_f16.hip) with ReLU
__device__ __forceinline__ void pc_relu_pack(const f32x4 v, unsigned (&pk)[2]) {
    half2_ lo2, hi2;
    lo2[0] = (half_t)__builtin_amdgcn_fmed3f(v[0], 0.f, 65504.f);
    lo2[1] = (half_t)__builtin_amdgcn_fmed3f(v[1], 0.f, 65504.f);
    hi2[0] = (half_t)__builtin_amdgcn_fmed3f(v[2], 0.f, 65504.f);
    hi2[1] = (half_t)__builtin_amdgcn_fmed3f(v[3], 0.f, 65504.f);
    pk[0] = __builtin_bit_cast(unsigned, lo2);
    pk[1] = __builtin_bit_cast(unsigned, hi2);
}

template <int CHAIN>
__global__ __launch_bounds__(PC_THREADS) void panel_chain_kernel(PcParams p) {
    constexpr PcChain CH = PC_CHAIN[CHAIN];
    constexpr int NP = CH.npass;
    constexpr int NI = 4;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* const panel = lds;
    float* const bias_lds = reinterpret_cast<float*>(lds + PC_PANEL + PC_SLOTS);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    int tile = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    if (tile >= p.tiles) return;

    // the layers' biases, once per workgroup (compiler-visible loads: finished before the first counted wait is set up)
#pragma unroll
    for (int l = 0; l < CH.nlayers; ++l)
        for (int i = tid; i < CH.c[l]; i += PC_THREADS) bias_lds[pc_bias_off(CHAIN, l) + i] = p.bias[l][i];
    __syncthreads();

    // panel request: wave w moves rows 16 w .. + 15 (two row groups of 8) of all 8 K tiles: piece (rg, kt) = rows 8 rg + lane / 8, 16-byte chunk
    // swz(row, lane % 8) of K tile kt, to image kt at rg * 1024.  (row >> 1) & 7 = (4 (rg & 1) + (lane >> 4)) & 7.  A scalar base per row group, the
    // lane's 32-bit offset formed here from an opaque copy of its slot (not carried across the K loops).
    const unsigned vlane16 = (unsigned)(lane * 16);
    constexpr int LDX = CH.ldx;
    auto request_panel = [&](int t) __attribute__((always_inline)) {
        unsigned l16 = vlane16;
        asm volatile("" : "+v"(l16));
        const unsigned r8 = l16 >> 7, c8 = (l16 >> 4) & 7;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned voff = r8 * (LDX * 2) + ((c8 ^ ((4 * h + (r8 >> 1)) & 7)) << 4);
            const half_t* g = pc_uniform(p.x + ((int64_t)t * PC_ROWS + wave * 16 + h * 8) * LDX);
            const unsigned dst = (unsigned)(size_t)panel + (unsigned)((wave * 2 + h) * 1024);
#pragma unroll
            for (int kt = 0; kt < PC_NK; ++kt) pc_dma16(voff, g + kt * 64, dst + kt * 16384);
        }
    };
    // the wave's two pieces of ONE image: the same rows and places as above, from rows of LD halfs; src = the tile's first row at the K tile's first column
    auto request_image = [&](auto ldc, const half_t* src, int img) __attribute__((always_inline)) {
        constexpr int LD = decltype(ldc)::value;
        unsigned l16 = vlane16;
        asm volatile("" : "+v"(l16));
        const unsigned r8 = l16 >> 7, c8 = (l16 >> 4) & 7;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned voff = r8 * (LD * 2) + ((c8 ^ ((4 * h + (r8 >> 1)) & 7)) << 4);
            const half_t* g = pc_uniform(src + (int64_t)(wave * 16 + h * 8) * LD);
            pc_dma16(voff, g, (unsigned)(size_t)panel + (unsigned)((wave * 2 + h) * 1024) + (unsigned)(img * 16384));
        }
    };
    // this wave's fragments of K tile 0 of a pass: [column tile][K tile][wave column][4096 halfs]
    auto pass_weights = [&](auto pc) __attribute__((always_inline)) {
        constexpr int P = decltype(pc)::value;
        constexpr PcPass D = CH.pass[P];
        const int tn = D.col0 / 256 + (D.two_by_four ? 0 : (wave >> 2));
        return pc_uniform(p.frag[D.layer] + ((int64_t)tn * (CH.k[D.layer] / 64) * 4 + (wave & 3)) * 4096);
    };
    auto wload = [&](const half_t* wks, auto jc) __attribute__((always_inline)) {
        constexpr int J = decltype(jc)::value;
        half8 v;
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(v) : "v"(vlane16), "s"(wks), "n"(J * 1024) : "memory");
        return v;
    };
    auto wload4 = [&](half8 (&dst)[NI], const half_t* wks) __attribute__((always_inline)) {
        dst[0] = wload(wks, std::integral_constant<int, 0>{});
        dst[1] = wload(wks, std::integral_constant<int, 1>{});
        dst[2] = wload(wks, std::integral_constant<int, 2>{});
        dst[3] = wload(wks, std::integral_constant<int, 3>{});
    };

    char* const slot = lds + PC_PANEL + wave * 2048;       // the wave's output slot: 16 rows x 128 B

    f32x4 acc[8][NI];
    half8 wq[2][NI];

    // prologue: the first tile's panel and the first pass's first K tile
    request_panel(tile);
    {
        const half_t* w0 = pass_weights(std::integral_constant<int, 0>{});
        wload4(wq[0], w0);
        wload4(wq[1], w0 + 2048);
    }
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();

    for (;;) {
        const int next = tile + (int)gridDim.x;
        const bool has_next = next < p.tiles;

        auto run_pass = [&](auto pc) __attribute__((always_inline)) {
            constexpr int P = decltype(pc)::value;
            constexpr PcPass D = CH.pass[P];
            constexpr int PN = (P + 1) % NP, PP = (P + NP - 1) % NP;
            constexpr int MI = D.two_by_four ? 4 : 8;
            // stores of the pass in front of this one (they sit behind this pass's first two k steps in the issue order)
            constexpr int NST_PREV = CH.pass[PP].store ? (CH.pass[PP].two_by_four ? 8 : 16) : 0;
            const int row0 = D.two_by_four ? (wave >> 2) * 64 : 0;           // the wave's first row of the panel
            const int wcol = D.two_by_four ? (wave & 3) : wave;               // its 64-column block of the pass
            const half_t* wcur = pass_weights(pc);
            const half_t* wnp = pass_weights(std::integral_constant<int, PN>{});
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // activation fragment of k step ks: row pr (+ 16 i), 16-byte chunk 4 ks + q, swizzled.  Formed per pass from an opaque copy of the lane's slot,
            // and the K tile's addresses from an opaque copy of the counter: hoisted out of the tile loop they are more live values than there are registers.
            int offa[2];
            {
                unsigned l16 = vlane16;
                asm volatile("" : "+v"(l16));
                const int pr = (l16 >> 4) & 15, q = l16 >> 8;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) offa[ks] = pr * 128 + (((ks * 4 + q) ^ ((pr >> 1) & 7)) << 4);
            }
            // one K tile; WAITC = what may be outstanding behind this k step's weights: the following k step's 4 loads (+ the previous pass's stores, + the K tile's 2 pieces).  Every
            // wait has a fixed count at a fixed place (the first K tile behind a storing pass is its own copy of the body), so the counts can be checked on
            // the built code (tools/check_barrier_reads.py).
            // BAR: a barrier in front of the K tile (it retires image kt - 1 and publishes the pieces whose waits lie before it); ROLL: behind it the
            // wave requests its pieces of image kt - 1 from K tile kt - 1 of the rows at roll_src, and the k steps wait with those 2 outstanding as well.
            constexpr bool LAST = P + 1 == NP;
            constexpr bool ROLL_NEXT = LAST && PC_ROLL_NEXT;
            constexpr int NKT = D.half2 != PC_H2_NONE ? 2 * PC_NK : PC_NK;
            static_assert(!(ROLL_NEXT && D.half2 != PC_H2_NONE), "a pass rolls one source");
            constexpr int RLD = D.half2 == PC_H2_X2 ? PC_K : LDX;
            const half_t* roll_src = nullptr;
            if constexpr (D.half2 == PC_H2_XHI) roll_src = pc_uniform(p.x + (int64_t)tile * PC_ROWS * LDX + PC_K);
            else if constexpr (D.half2 == PC_H2_X2) roll_src = pc_uniform(p.x2 + (int64_t)tile * PC_ROWS * PC_K);
            else if constexpr (ROLL_NEXT) roll_src = pc_uniform(p.x + (int64_t)(has_next ? next : tile) * PC_ROWS * LDX);
            auto k_tile = [&](int kt, auto waitc, auto barc, auto rollc) __attribute__((always_inline)) {
                constexpr int WAITC = decltype(waitc)::value;
                constexpr bool BAR = decltype(barc)::value, ROLL = decltype(rollc)::value;
                int ktv = kt;
                asm volatile("" : "+s"(ktv));
                if constexpr (BAR) {
                    wait_lgkm0();
                    __builtin_amdgcn_s_barrier();
                }
                if constexpr (ROLL) request_image(std::integral_constant<int, RLD>{}, roll_src + (ktv - 1) * 64, ktv - 1);
                const half_t* wnext = pc_uniform(ktv + 1 < NKT ? wcur + (int64_t)(ktv + 1) * 16384 : wnp);
                const char* base = panel + (ktv & (PC_NK - 1)) * 16384 + row0 * 128;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    half8 af[MI];
#pragma unroll
                    for (int i = 0; i < MI; ++i) af[i] = *(const half8*)(base + offa[ks] + i * 2048);
                    wait_vmcnt<WAITC>();
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq[ks][j], af[i], acc[i][j], 0, 0, 0);
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
                    wload4(wq[ks], wnext + ks * 2048);     // the same k step of the next K tile (the MFMAs that read the registers have been issued)
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            using yes = std::true_type;
            using no = std::false_type;
            constexpr bool ROLLS = ROLL_NEXT || D.half2 != PC_H2_NONE;
            if constexpr (NST_PREV > 0 || ROLLS) k_tile(0, std::integral_constant<int, 4 + NST_PREV>{}, no{}, no{});
            if constexpr (D.half2 != PC_H2_NONE) {
                // K tiles 1 .. 8 free images 0 .. 7 and request K tiles 8 .. 15 into them; image 7's pieces are retired by the wait of K tile 9 and
                // published by the barrier of K tile 10, long before K tile 15 reads them
#pragma unroll 1
                for (int kt = 1; kt <= PC_NK; ++kt) k_tile(kt, std::integral_constant<int, 6>{}, yes{}, yes{});
#pragma unroll 1
                for (int kt = PC_NK + 1; kt <= PC_NK + 2; ++kt) k_tile(kt, std::integral_constant<int, 4>{}, yes{}, no{});
#pragma unroll 1
                for (int kt = PC_NK + 3; kt < NKT; ++kt) k_tile(kt, std::integral_constant<int, 4>{}, no{}, no{});
            } else if constexpr (ROLL_NEXT) {
#pragma unroll 1
                for (int kt = 1; kt < PC_NK; ++kt) k_tile(kt, std::integral_constant<int, 6>{}, yes{}, yes{});
            } else {
#pragma unroll 1
                for (int kt = NST_PREV > 0 ? 1 : 0; kt < PC_NK; ++kt) k_tile(kt, std::integral_constant<int, 4>{}, no{}, no{});
            }
            // ---- the pass's end: bias + ReLU + fp16 on the accumulators.  The lane's places are formed here from an opaque copy of its slot: carried
            // across the K loops they would cost registers that the accumulators and operands do not leave.
            unsigned l16 = vlane16;
            asm volatile("" : "+v"(l16));
            const int pr = (l16 >> 4) & 15, q = l16 >> 8;
            // after the half swap a lane holds row pr (+ 16 i), channels 16 (2 jp + (q & 1)) + 8 (q >> 1) .. + 7 of the wave's 64 = 16-byte chunk
            // 4 jp + seg of that row; jp = 1 is the address ^ 64
            const int seg = 2 * (q & 1) + (q >> 1);
            f32x4 bv[NI];
#pragma unroll
            for (int j = 0; j < NI; ++j) bv[j] = *(const f32x4*)&bias_lds[pc_bias_off(CHAIN, D.layer) + D.col0 + wcol * 64 + j * 16 + q * 4];
            if constexpr (!D.store) {
                // hand-over: image `wave` of the panel (the wave's 64 columns are K tile `wave` of the next layer), chunk swizzled as the fills are
                const int hand_off = wave * 16384 + pr * 128 + ((seg ^ ((pr >> 1) & 7)) << 4);
                wait_lgkm0();
                __builtin_amdgcn_s_barrier();              // every wave has read the panel for the last time
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; j += 2) {
                        unsigned pk[2][2];
                        pc_relu_pack(acc[i][j] + bv[j], pk[0]);
                        pc_relu_pack(acc[i][j + 1] + bv[j + 1], pk[1]);
                        const auto s0 = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
                        const auto s1 = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
                        const u32x4_t o = {s0[0], s1[0], s0[1], s1[1]};
                        *(u32x4_t*)(panel + ((hand_off ^ ((j >> 1) * 64)) + i * 2048)) = o;
                    }
                wait_lgkm0();
                __builtin_amdgcn_s_barrier();              // the next layer's panel is complete
            } else {
                if constexpr (LAST) {
                    wait_lgkm0();
                    __builtin_amdgcn_s_barrier();          // every wave has read the panel for the last time: the next tile's may land
                    if constexpr (ROLL_NEXT) request_image(std::integral_constant<int, LDX>{}, roll_src + (PC_NK - 1) * 64, PC_NK - 1);
                    else if (has_next) request_panel(next);
                }
                // the slot: row pr at chunk (4 jp + seg) ^ (pr & 7); read back as two runs of 8 rows, lane L = row L / 8, chunk L % 8: whole 128-byte lines
                const int slot_wr = pr * 128 + ((seg ^ (pr & 7)) << 4);
                const int slot_rd = (l16 >> 7) * 128 + ((((l16 >> 4) & 7) ^ (l16 >> 7)) << 4);
                const unsigned vline = (unsigned)(((l16 >> 7) * p.ldo + ((l16 >> 4) & 7) * 8) * 2);
                const half_t* orow = p.out + ((int64_t)tile * PC_ROWS + row0) * p.ldo + D.col0 + wcol * 64;
#pragma unroll
                for (int i = 0; i < MI; ++i) {
#pragma unroll
                    for (int j = 0; j < NI; j += 2) {
                        unsigned pk[2][2];
                        pc_relu_pack(acc[i][j] + bv[j], pk[0]);
                        pc_relu_pack(acc[i][j + 1] + bv[j + 1], pk[1]);
                        const auto s0 = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
                        const auto s1 = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
                        const u32x4_t o = {s0[0], s1[0], s0[1], s1[1]};
                        *(u32x4_t*)(slot + (slot_wr ^ ((j >> 1) * 64))) = o;
                    }
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const u32x4_t dv = *(const u32x4_t*)(slot + h * 1024 + slot_rd);
                        pc_store16(vline, dv, pc_uniform(orow + (int64_t)(i * 16 + h * 8) * p.ldo));
                    }
                }
                if constexpr (LAST) {
                    if (has_next) {
                        // the panel's pieces are older than this pass's stores
                        wait_vmcnt<D.two_by_four ? 8 : 16>();
                        __builtin_amdgcn_s_barrier();
                    }
                }
            }
        };
        run_pass(std::integral_constant<int, 0>{});
        run_pass(std::integral_constant<int, 1>{});
        if constexpr (NP > 2) run_pass(std::integral_constant<int, 2>{});
        if constexpr (NP > 3) run_pass(std::integral_constant<int, 3>{});
        if (!has_next) break;
        tile = next;
    }
    wait_vmcnt<0>();                                       // the look-ahead's loads and the stores: nothing may land after the wave has gone
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < NI; ++j) asm volatile("" ::"v"(wq[ks][j]));
}

}  // namespace

}  // namespace pcd

using namespace pcd;

// what both entry points check and launch: chain 0 / 1 / 2 = E4 / D3T / D43
static int pc_launch(int chain, const void* x, const void* x2, int64_t m, const void* const* frag, const float* const* bias, int hilo, void* out,
                     int64_t ld, int cap, void* stream) {
    PCD_CHECK_ARG(x != nullptr && frag != nullptr && bias != nullptr && out != nullptr && x != out);
    PCD_CHECK_ARG(m > 0 && m % PC_ROWS == 0 && m <= 0x7fffffff);
    PCD_CHECK_ARG(cap >= 1 && cap <= 256);
    PCD_CHECK_ARG(hilo == 0);
    const PcChain& ch = PC_CHAIN[chain];
    PCD_CHECK_ARG(ld >= ch.c_out && ld % 8 == 0 && (7 * ld + 64) * 2 < 0x7fffffffLL);
    PcParams p{};
    for (int l = 0; l < ch.nlayers; ++l) {
        PCD_CHECK_ARG(frag[l] != nullptr && bias[l] != nullptr);
        p.frag[l] = (const half_t*)frag[l]; p.bias[l] = bias[l];
    }
    p.x = (const half_t*)x; p.x2 = (const half_t*)x2; p.out = (half_t*)out; p.ldo = (int)ld; p.tiles = (int)(m / PC_ROWS);
    static PcdLdsOnce once[PC_NCHAIN];
    const void* kernel = chain == 0 ? (const void*)panel_chain_kernel<0> : chain == 1 ? (const void*)panel_chain_kernel<1> : (const void*)panel_chain_kernel<2>;
    const int lds = pc_lds_bytes(chain);
    PCD_CHECK_HIP(pcd_allow_lds(once[chain], kernel, lds));
    const dim3 grid((unsigned)(p.tiles < cap ? p.tiles : cap));
    if (chain == 0) hipLaunchKernelGGL(panel_chain_kernel<0>, grid, dim3(PC_THREADS), lds, (hipStream_t)stream, p);
    else if (chain == 1) hipLaunchKernelGGL(panel_chain_kernel<1>, grid, dim3(PC_THREADS), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(panel_chain_kernel<2>, grid, dim3(PC_THREADS), lds, (hipStream_t)stream, p);
    PCD_CHECK_LAUNCH();
    return PCD_OK;
}

// chain 0 = E4 (frag / bias: lin 8, 9, 10; out [m][ld], ld >= 1024), chain 1 = D3T (lin 17, 18; ld >= 256).  x: [m][512] fp16, dense.  frag[l]:
// pcd_gemm_pack_wfrag of layer l's [C][512] weights.  hilo: bit l set = layer l has hi / lo weights, which this kernel does not take.  cap: the most
// workgroups (1 .. 256; one per CU); a workgroup walks tiles b, b + grid, ...  Refuses what the kernel does not take and launches nothing then.
extern "C" int pcd_panel_chain(int chain, const void* x, int64_t m, const void* const* frag, const float* const* bias, int hilo, void* out, int64_t ld,
                               int cap, void* stream) {
    PCD_CHECK_ARG(chain == 0 || chain == 1);
    return pc_launch(chain, x, nullptr, m, frag, bias, hilo, out, ld, cap, stream);
}

// D43 (frag / bias: lin 15, 16, 17, 18; out [m][ld], ld >= 256).  x: [m][1024] fp16, dense; x3: [m][512], the second K half of the second layer
// ([the first layer's output | x3]).  frag[0], frag[1]: pcd_gemm_pack_wfrag of [512][1024] weights; frag[2], frag[3]: of [512][512] and [256][512].
extern "C" int pcd_panel_chain_dec(const void* x, const void* x3, int64_t m, const void* const* frag, const float* const* bias, int hilo, void* out,
                                   int64_t ld, int cap, void* stream) {
    PCD_CHECK_ARG(x3 != nullptr && x3 != out);
    return pc_launch(2, x, x3, m, frag, bias, hilo, out, ld, cap, stream);
}
