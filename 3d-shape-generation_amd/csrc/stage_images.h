// Host side of the register-resident chains (widechain.hip, wideffn.hip, sab_tail.hip), once: what a packed weight buffer holds (StageLayout), the
// one kernel and the one function that write it, and the one launch of a kernel that streams it through the three-slot LDS-DMA ring.
// A buffer is stage images -- 1-KiB pieces in MFMA fragment order -- followed by a block of fp32 parameters.  Each family states its buffer as ONE
// constexpr layout function; its *_packed_bytes, its *_pack and its launcher read that, and its kernel's own constants are asserted against it.
#pragma once
#include "common.h"

namespace pcd {

// W [.][ldw] fp16 -> ntile x nq pieces: piece (t * nq + q) * 64 + lane = the 8 halfs W[row0 + 32 t + (lane & 31)][k0 + 16 q + 8 (lane >> 5) .. + 7],
// rows at or past row_limit read as zero
static __global__ __launch_bounds__(256) void stage_pack_kernel(const half_t* __restrict__ w, int64_t ldw, int row0, int row_limit, int k0, int ntile, int nq,
                                                                char* __restrict__ dst) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= ntile * nq * 64) return;
    const int lane = id & 63, tq = id >> 6, t = tq / nq, q = tq - t * nq;
    const int row = row0 + 32 * t + (lane & 31);
    half8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (half_t)0.f;
    if (row < row_limit) v = *(const half8*)(w + (int64_t)row * ldw + k0 + 16 * q + 8 * (lane >> 5));
    *(half8*)(dst + (size_t)id * 16) = v;
}

// nimg consecutive images of ntile x nq pieces of weights[w]: image j starts at column k0 + 16 nq j
struct FragBlock { int w, ldw, row0, row_limit, k0, ntile, nq, nimg; size_t off; };
// n floats of params[src] from its float src_off on (src < 0 or n = 0: no source, the row stays zero), at float `off` of the parameter block
struct ParamRow { int src, src_off, n, off; };
struct StageLayout {
    int nblock, nrow;
    size_t par;                    // bytes in front of the parameter block
    size_t bytes;                  // the whole buffer; what no block or row covers is zero
    FragBlock block[20];
    ParamRow row[8];
};
constexpr void sl_frag(StageLayout& L, int w, int ldw, int row0, int row_limit, int k0, int ntile, int nq, int nimg = 1) {
    L.block[L.nblock++] = FragBlock{w, ldw, row0, row_limit, k0, ntile, nq, nimg, L.bytes};
    L.bytes += (size_t)nimg * ntile * nq * 1024;
    L.par = L.bytes;
}
// a row of `width` floats of which the first n come from params[src]
constexpr void sl_row(StageLayout& L, int src, int src_off, int n, int width) {
    L.row[L.nrow++] = ParamRow{src, src_off, n, (int)((L.bytes - L.par) / sizeof(float))};
    L.bytes += width * sizeof(float);
}

static inline int stage_pack(const StageLayout& L, const void* const* weights, const float* const* params, void* packed, hipStream_t s) {
    char* dst = (char*)packed;
    PCD_CHECK_HIP(hipMemsetAsync(dst, 0, L.bytes, s));
    for (int i = 0; i < L.nblock; ++i) {
        const FragBlock& b = L.block[i];
        const int pieces = b.ntile * b.nq * 64;
        for (int j = 0; j < b.nimg; ++j)
            hipLaunchKernelGGL(stage_pack_kernel, dim3((pieces + 255) / 256), dim3(256), 0, s, (const half_t*)weights[b.w], (int64_t)b.ldw, b.row0, b.row_limit,
                               b.k0 + 16 * b.nq * j, b.ntile, b.nq, dst + b.off + (size_t)j * pieces * 16);
    }
    PCD_CHECK_LAUNCH();
    for (int i = 0; i < L.nrow; ++i) {
        const ParamRow& r = L.row[i];
        if (r.src >= 0 && r.n > 0)
            PCD_CHECK_HIP(hipMemcpyAsync(dst + L.par + r.off * sizeof(float), params[r.src] + r.src_off, r.n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return PCD_OK;
}

// Grid caps of the ring kernels: workgroups that walk the tiles of points (256 CUs)
enum RingCap : int {
    RING_CAP_CU = 256,             // one workgroup per CU: the chains, the ends, LN + Linear, the FFN, the C = 128 tail and head (a 96-KB ring fills a CU's LDS once)
    RING_CAP_TAIL64 = 512,         // the C = 64 tail: 128 registers and 50 KB of LDS let two workgroups share a CU, and it is closer to its HBM bound than to the matrix pipe's
    RING_CAP_HEAD64 = 768,         // the C = 64 head: 74 registers, 26 KB of LDS: three workgroups per CU (HBM-bound: 67 MB per launch at cfg2)
};

// The launch of a ring kernel: min(tiles, cap) workgroups; EVERY / SPLIT = its "every wave requests" / "one wave per SIMD requests" instantiation (the same
// kernel twice where the form is a run-time parameter).  Dynamic LDS above 64 KB is allowed once per kernel and device.
template <auto EVERY, auto SPLIT, class Params>
static hipError_t ring_launch(int64_t tiles, RingCap cap, int threads, size_t lds, bool split, hipStream_t s, const Params& p) {
    static PcdLdsOnce once[2];
    hipError_t e = pcd_allow_lds(once[split], (const void*)(split ? SPLIT : EVERY), (int)lds);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
    if (split) hipLaunchKernelGGL(SPLIT, grid, dim3(threads), lds, s, p);
    else hipLaunchKernelGGL(EVERY, grid, dim3(threads), lds, s, p);
    return hipGetLastError();
}

}  // namespace pcd
