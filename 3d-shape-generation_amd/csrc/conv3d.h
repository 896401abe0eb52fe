// What the three convolution files share (internal; included by conv3d_igemm.hip, conv3d_halo.hip and conv3d_ends.hip only).
#pragma once
#include <type_traits>
#include "common.h"

namespace pcd {

constexpr int CBK = 64;
constexpr int CROWB = CBK * 2;

constexpr int MAX_VARIANTS = 8;      // the 2x2x2 output-parity classes of a stride-2 ConvTranspose3d
constexpr int MAX_TAPS = 64;
constexpr int TAP_SLOTS = 128;     // LDS tap table of the implicit GEMM: ntaps real entries + the K padding's (kpad / Cin <= 128)

// the 4 x 4 x 8 output block of the LDS-halo kernels and its 6 x 6 x 10 input halo
constexpr int HTZ = 4, HTY = 4, HTX = 8, HHY = HTY + 2, HHX = HTX + 2, HROWS = (HTZ + 2) * HHY * HHX;

// shared between the three files only: kept out of the library's dynamic symbol table
#define PCD_INTERNAL __attribute__((visibility("hidden")))

PCD_INTERNAL int conv_check(const pcd_conv3d_desc_t* d);     // what every entry point that takes a descriptor requires of it (conv3d_igemm.hip)

// pcd_conv3d_config, decoded (the table of codes is in include/pcd_hip.h).  TEST / BENCHMARK ONLY, process-global.
struct Conv3dConfig {
    int halo_tall = 1;        // 32 -> 32 LDS-ring layers on 256-row workgroups: 0 never, 1 where that leaves >= 512 workgroups, 2 wherever the shape allows
    int last8 = 3;            // the last layer: 3 = per-tap partial products, 2 = 8 x 8 x 8 blocks with one MFMA per tap and 16 voxels, 1 = 8 x 8 x 8 on the VALU, 0 = 4 x 4 x 8 blocks
    int split_target = 512;   // split-K aims at this many workgroups (VAE3DLarge encode at B = 32: 834 / 913 / 888 us at 384 / 768 / 1024 against 817 at 512)
    int last_abl = 0;         // timing ablations of conv3d_last_taps_kernel (outputs wrong)
    int first8 = 1;           // the first layer: 8 x 8 x 8 tiles where the grid divides; 0 = 4 x 4 x 8 tiles
    int igemm_abl = 0;        // timing ablations of the 128 x 128 implicit GEMM (outputs wrong)
    int last_roll = 1;        // per-tap last layer: a wave owns four output slices and reads every input slice once; 0 = a wave per output slice
    int wreg_abl = 0;         // timing ablations of conv3d_halo_wreg_kernel<64, 2> (outputs wrong)
};
PCD_INTERNAL extern Conv3dConfig g_conv3d;

// `call(std::integral_constant<int, V>)` for the V among Vs... that equals v, for V0 otherwise: an ablation ladder whose rungs differ in one
// template integer, written once (the instances are exactly V0, Vs...).
template <int V0, int... Vs, class F>
static inline void dispatch_int(int v, F&& call) {
    if (!((v == Vs && (call(std::integral_constant<int, Vs>{}), true)) || ...)) call(std::integral_constant<int, V0>{});
}

}  // namespace pcd
