// fd_shared64.h -- what the two fp64 shot launches share (fd_eval_shared64.hip: positions, fd_vectors_shared64.hip: the
// Jacobian and the vectors): the layout of the batch's fp64 scratch as k_pack_shared64 writes it, and the dealing of
// (frame, component) rows onto the 16-row output tiles of v_mfma_f64_16x16x4_f64.  ONE copy: the vector launch reads
// the scratch the position launch's pack kernel wrote, so the two must agree on every offset.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "fd_internal.h"

namespace fd {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kS64Waves = 8;
constexpr int kS64Threads = 64 * kS64Waves;
constexpr size_t kS64LdsBudget = 158 * 1024;

// head of the scratch (and of LDS): per-frame status and outputs
struct S64Head {
    int built[kMaxBatch];
    float *P_out[kMaxBatch];
    float *fall[kMaxBatch];
};
static_assert(sizeof(S64Head) % 16 == 0, "the tiles behind the head stay 16-byte aligned");

// scratch, in doubles behind the head: [affine tiles NT x 64][centre records Mpad x 4][weights nks x NT x 64]
__host__ __device__ inline size_t s64_aff_at() { return sizeof(S64Head) / 8; }
__host__ __device__ inline size_t s64_cen_at(int NT) { return s64_aff_at() + (size_t)NT * 64; }
__host__ __device__ inline size_t s64_w_at(int NT, int Mpad) { return s64_cen_at(NT) + (size_t)Mpad * 4; }

inline int s64_tiles(int nF) { return nF > 12 ? 3 * ((nF + 15) / 16) : (nF + 3) / 4; }

// (frame, component) of row `row` of row tile T; component 3 or a frame past nF: padding
__device__ __forceinline__ void s64_row(bool dense, int T, int row, int &f, int &c)
{
    const int g = row & 3, r = row >> 2;
    if (dense) {
        const int s = 4 * (T % 3) + r;
        f = 16 * (T / 3) + 4 * g + s / 3; c = s % 3;
    } else {
        f = 4 * T + g; c = r;
    }
}

}  // namespace fd
