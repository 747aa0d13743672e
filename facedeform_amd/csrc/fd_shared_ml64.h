// fd_shared_ml64.h -- what the two fp64 shot launches of the MULTILAYER model share (fd_eval_shared_ml64.hip: positions,
// fd_vectors_shared_ml64.hip: the Jacobian and the vectors): the layout of the batch's multilayer-fp64 scratch as
// k_pack_shared_ml64 writes it.  ONE copy: the vector launch reads the scratch the position launch's pack kernel wrote,
// so the two must agree on every offset.  Head, affine tiles and row dealing are fd_shared64.h's.
#pragma once
#include <cstddef>

#include "fd_shared64.h"

namespace fd {

constexpr int kMl64Restart = 4;                           // layers per chain: three quadruplings at most
constexpr int kMl64Cen = 6;                               // doubles per centre record {cx, cy, cz, s_0, s_4, 0}

// scratch, in doubles behind the head (S64Head): [affine tiles NT x 64][centre records Mc4 x 6][weights nkc x L x NT x 64]
__host__ __device__ inline size_t ml64_cen_at(int NT) { return s64_aff_at() + (size_t)NT * 64; }
__host__ __device__ inline size_t ml64_w_at(int NT, int Mc4) { return ml64_cen_at(NT) + (size_t)Mc4 * kMl64Cen; }
__host__ __device__ inline size_t ml64_step_w(int NT, int L) { return (size_t)L * NT * 64; }        // weights of one centre step

}  // namespace fd
