// fd_shared_common.h -- what the shot launches of fd_eval_shared.hip and fd_eval_shared_ml.hip share: the frame record, the
// split of an fp32 pair into its two fp16 pieces, the 12-byte position stores and the constants both are sized by.  Moved here
// from fd_eval_shared.hip word for word (its kernels' generated code is unchanged: DESIGN.md 4.1f).
#pragma once
#include <hip/hip_runtime.h>

#include "fd_eval_common.h"
#include "fd_shared_plan.h"       // kSharedLdsBudget, kGaussShift

namespace fd {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

struct SharedFrame {              // one per frame slot (nT * 4), written by k_pack_shared
    float inv_scale;              // 2^-k: undoes the scaling of the frame's weights and polynomial
    int built;                    // terminationtype == 1
    int pad[2];
    float *P_out, *falloff_out;   // the frame's outputs (read from LDS inside the frame loop: 64 pointers
                                  // as kernel arguments end up hoisted into SGPRs all at once and spilled)
};
static_assert(sizeof(SharedFrame) == 32, "frame record");

// fp32 pair -> its two fp16 pieces, packed: hi = RN16(v), lo = RN16(v - hi).  One v_cvt_pk_f16_f32 and
// two mixed-precision fmas that subtract the fp16 piece from the fp32 value and round the
// remainder to fp16 in the same instruction (v_fma_mixlo/hi_f16 write one half of the destination
// and keep the other) -- three instructions for two values, no unpacking, no repacking.
// PLAIN: the same two pieces from instructions the compiler sees (conversions and a subtraction: about twice as
// many).  The Gaussian kinds take this form: there the inputs come straight from v_exp_f32, and a vector
// instruction hidden in an asm string that reads a transcendental's result gets none of the wait states the
// compiler pads that pair with (hipcc pads nothing inside or around asm strings).
template <bool PLAIN = false, bool NOP = true>
__device__ __forceinline__ void split_pair_f16(float v0, float v1, unsigned &hi, unsigned &lo)
{
    if constexpr (PLAIN) {
        const _Float16 h0 = (_Float16)v0, h1 = (_Float16)v1;
        const _Float16 l0 = (_Float16)(v0 - (float)h0), l1 = (_Float16)(v1 - (float)h1);
        hi = __builtin_bit_cast(unsigned, (f16x2){h0, h1});
        lo = __builtin_bit_cast(unsigned, (f16x2){l0, l1});
        return;
    }
    const f16x2 hh = __builtin_convertvector((f32x2){v0, v1}, f16x2);
    hi = __builtin_bit_cast(unsigned, hh);
    unsigned l;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(hi), "v"(v0));
    // (s_nop 1 inside the string: a register written by a vector instruction needs two wait states before a matrix
    // instruction reads it as an operand, and the compiler pads only producers it can see; no measurable cost:
    // 218-229 us per C2 x 32 launch with it, 210-237 without, same box)
    // (NOP = false: the caller fences a whole block of pairs with ONE s_nop behind the last of them, fence_operands below)
    if constexpr (NOP) asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\ts_nop 1" : "+v"(l) : "v"(hi), "v"(v1));
    else asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(hi), "v"(v1));
    lo = l;
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x8 __attribute__((ext_vector_type(8)));
// one vertex position as a single 12-byte store (dword-aligned: global_store_dwordx3)
struct __attribute__((packed, aligned(4))) Pos3 { float x, y, z; };
__device__ __forceinline__ void store_pos3(Pos3 FD_GLOBAL *dst, float x, float y, float z)
{
    dst->x = x; dst->y = y; dst->z = z;      // member-wise: a struct assignment through an address-space pointer does not compile on the host pass
}

// the same with the non-temporal hint: the 512 MB a launch writes need not displace what else lives in L2
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef f32x3 f32x3_a4 __attribute__((aligned(4)));
typedef f32x4 f32x4_a16 __attribute__((aligned(16)));
typedef f32x2 f32x2_a8 __attribute__((aligned(8)));
__device__ __forceinline__ void store_pos3_nt(Pos3 FD_GLOBAL *dst, float x, float y, float z)
{
    __builtin_nontemporal_store((f32x3){x, y, z}, (f32x3_a4 FD_GLOBAL *)dst);
}
}  // namespace
}  // namespace fd
