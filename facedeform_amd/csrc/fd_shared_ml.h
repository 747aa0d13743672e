// fd_shared_ml.h -- what the two fp32 shot launches of the MULTILAYER model share (fd_eval_shared_ml.hip: positions,
// fd_vectors_shared_ml.hip: the Jacobian and the vectors): the layout of the batch's multilayer scratch as k_pack_shared_ml
// writes it.  ONE copy: the vector launch reads the scratch the position launch's pack kernel wrote, so the two must agree
// on every offset.
#pragma once
#include "fd_shared_common.h"

namespace fd {
namespace {

constexpr int kMlMinFrames = 2;                   // fewer frames: the per-context launches

// Rows of the stack of 32-row output tiles: row 3 f + c is component c of frame f (as the wide kernel packs them).
constexpr int ml_tiles(int nF) { return (3 * nF + 31) / 32; }          // 1 up to 10 frames, 2 up to 21, else 3
constexpr int ml_share(int L) { return L % 4 == 0 ? 4 : (L % 2 == 0 ? 2 : 1); }

// scratch, in 16-byte words: [frame records 32 x 2][normalisation][polynomial tiles NT x 64][records nkb x 32]
//                            [weight tiles nkb x NT x (K step 2 x (hi, lo) x 64 lanes)]
constexpr size_t kMlNormAt = kMaxBatch * sizeof(SharedFrame) / 16;
constexpr size_t kMlPolyAt = kMlNormAt + 1;
constexpr size_t ml_rec_at(int nt) { return kMlPolyAt + (size_t)nt * 64; }
constexpr size_t ml_w_at(int nt, int nkb) { return ml_rec_at(nt) + (size_t)nkb * 32; }
constexpr size_t ml_w16(int nt) { return (size_t)nt * 256; }           // words of weight tiles per K block

}  // namespace
}  // namespace fd
