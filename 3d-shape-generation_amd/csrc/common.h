// Shared helpers for the gfx950 library (internal; the public ABI is include/pcd_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/pcd_hip.h"

namespace pcd {

void set_error(const char* fmt, ...);

#define PCD_CHECK_ARG(cond)                                                        \
    do {                                                                           \
        if (!(cond)) {                                                             \
            ::pcd::set_error("%s:%d: bad argument: %s", __FILE__, __LINE__, #cond); \
            return PCD_ERR_ARG;                                                    \
        }                                                                          \
    } while (0)

#define PCD_CHECK_HIP(expr)                                                              \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess) {                                                         \
            ::pcd::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,               \
                             hipGetErrorString(e__));                                    \
            return PCD_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

#define PCD_CHECK_LAUNCH() PCD_CHECK_HIP(hipGetLastError())

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2_ __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

__device__ __forceinline__ half_t to_half_sat(float v) {
    // keep fp16 activations finite: clamp to the largest normal instead of +-inf
    v = __builtin_fminf(__builtin_fmaxf(v, -65504.f), 65504.f);
    return (half_t)v;
}

// host: run a step that returns a PCD_* code and leave with it on failure (`int rc` in scope)
#define PCD_RUN(expr) do { rc = (expr); if (rc) return rc; } while (0)

static inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Dynamic LDS above 64 KB has to be allowed per kernel AND per device: once per (device, kernel), whichever device is current at the launch.
struct PcdLdsOnce { unsigned long long done = 0; };          // one bit per device ordinal below 64 (above: set every time)
static inline hipError_t pcd_allow_lds(PcdLdsOnce& once, const void* kernel, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && ((once.done >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev >= 0 && dev < 64) once.done |= 1ull << dev;
    return e;
}

// Device copy of packed weights, made when a handle is created.  `src` points into the source weights: the copy is allocated on the CURRENT
// device, and only if that is where they live (one process per GPU sets it so).  `pack(buf)` enqueues the packer on the null stream and returns a
// PCD_* code; the copy is finished before this returns.  Any failure frees the buffer, clears the sticky HIP error and returns null: the caller
// keeps the kernel that reads the unpacked weights.
template <class Pack>
static inline void* pcd_packed_copy(const void* src, size_t bytes, Pack pack) {
    hipPointerAttribute_t at;
    int cur = -1;
    void* buf = nullptr;
    if (bytes == 0) return nullptr;
    if (hipGetDevice(&cur) == hipSuccess && hipPointerGetAttributes(&at, src) == hipSuccess && at.device == cur &&
        hipMalloc(&buf, bytes) == hipSuccess && pack(buf) == PCD_OK && hipStreamSynchronize(nullptr) == hipSuccess)
        return buf;
    (void)hipGetLastError();
    if (buf != nullptr) (void)hipFree(buf);
    return nullptr;
}

// gemm_f16.hip: would pcd_gemm_f16_colmax_wfrag take this column-max product (a fragment-order copy held, the path switched on, a shape of gemm_xw_kernel)?
// It refuses the others, and the caller then goes to pcd_gemm_f16_colmax.
bool gemm_colmax_takes_wfrag(const pcd_gemm_desc_t* d, int rows_per_shape, const void* wfrag);

}  // namespace pcd

#include "device_prims.h"
