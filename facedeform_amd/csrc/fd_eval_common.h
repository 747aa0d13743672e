// fd_eval_common.h -- helpers the evaluation translation units share (fd_eval.hip, fd_eval_shared.hip, fd_vectors_shared.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "fd_internal.h"

namespace fd {
namespace {

constexpr unsigned kMaxCUs = 1024;     // bound of the diagnostics' per-CU tables

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// ---- fp32 epilogue, same operation order as the reference -------------------
__device__ __forceinline__ void normalize3(float &x, float &y, float &z)
{
    const float l2 = x * x + y * y + z * z;
    if (l2 > 0.f) {
        const float inv = 1.f / sqrtf(l2);
        x *= inv; y *= inv; z *= inv;
    }
}

// d2 * log2|d2| with the DX9 multiply (0 * anything = 0): rounding can leave a vertex that sits
// on a centre at exactly zero or at a tiny negative d2; the first gives 0 * -inf = 0 here and the
// second an error of order 1e-7 * 23, the size of the rounding of d2 itself.  No clamp needed.
extern "C" __device__ float fd_fmul_legacy(float, float) __asm("llvm.amdgcn.fmul.legacy");
__device__ __forceinline__ float d2_log_d2(float d)
{
    return fd_fmul_legacy(d, __builtin_amdgcn_logf(__builtin_fabsf(d)));
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE property of a kernel: one process may hold contexts on
// several GPUs (fd_config.device), so "done" is remembered per (kernel, device), not per process.  (Host code: the shared-rig
// launches, fd_eval_shared.hip and fd_vectors_shared.hip.)
constexpr int kMaxDevices = 64;
struct LdsAttrOnce {
    bool done[kMaxDevices] = {};
    hipError_t ensure(const void *fn, int bytes)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < kMaxDevices && done[dev]) return hipSuccess;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess && dev >= 0 && dev < kMaxDevices) done[dev] = true;
        return e;
    }
};

}  // namespace
}  // namespace fd
