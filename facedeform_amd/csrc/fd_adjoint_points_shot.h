// fd_adjoint_points_shot.h -- the operand dealing and the scratch layout of the shot form of the positional adjoint
// (fd_adjoint_points_shot.hip, fd_batch_deform_adjoint_points_shared_dev).  Plain C++, callable on the host:
// the pack kernel and the main launch take every offset from here, and so do tests/tools/adjoint_points_shot_dealing.cpp and
// through it tests/test_adjoint_points_shot_abi.py.
//
// The product s = W R on v_mfma_f64_16x16x4_f64 has 16 centres as rows, 16 vertices as columns and (frame, component) as
// depth.  One instruction takes four depth slots, slot k from lane group k.  Depth is dealt so that a lane group holds whole
// frames: frames go in quads, a quad takes three steps, step 3 q + b carries component b of frames 4 q .. 4 q + 3 and slot k
// of it frame 4 q + k.  Lane (k, j) then forms r of vertex j for frames k, 4 + k, ... and nothing else: G is read once per
// (frame, vertex).  A shot of F frames has NQ = ceil(F / 4) quads and 3 NQ steps; the frames past F carry zeros.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define FD_APS_HD __host__ __device__
#else
#define FD_APS_HD
#endif

namespace fd {

FD_APS_HD inline int aps_quads(int nF) { return (nF + 3) / 4; }
FD_APS_HD inline int aps_steps(int nq) { return 3 * nq; }

// (frame, component) of depth slot k of step `step`
FD_APS_HD inline void aps_frame(int step, int k, int &f, int &b)
{
    f = 4 * (step / 3) + k;
    b = step % 3;
}

// ... and back: where component b of frame f goes
FD_APS_HD inline void aps_slot(int f, int b, int &step, int &k)
{
    step = 3 * (f / 4) + b;
    k = f % 4;
}

// Scratch, in doubles: [head: built[32] as ints][the affine tile: steps x 64][centre records Mpad x 4 {cx, cy, cz, s}]
// [weights: (Mpad / 16) centre tiles x steps x 64].  A tile of a step is the A operand as the 64 lanes read it: lane l
// holds row l & 15 and depth slot l >> 4.
constexpr size_t kApsHead = 16;
FD_APS_HD inline size_t aps_aff_at() { return kApsHead; }
FD_APS_HD inline size_t aps_cen_at(int nq) { return aps_aff_at() + (size_t)aps_steps(nq) * 64; }
FD_APS_HD inline size_t aps_w_at(int nq, int Mpad) { return aps_cen_at(nq) + (size_t)Mpad * 4; }
FD_APS_HD inline size_t aps_doubles(int nq, int Mpad) { return aps_w_at(nq, Mpad) + (size_t)(Mpad / 16) * aps_steps(nq) * 64; }

// Entry q of the weights: the centre, frame and component whose weight stands there (a frame >= nF: zero)
FD_APS_HD inline void aps_weight_source(int nq, size_t q, int &centre, int &f, int &b)
{
    const int l = (int)(q & 63);
    const size_t ts = q >> 6;
    const int step = (int)(ts % (size_t)aps_steps(nq)), tile = (int)(ts / (size_t)aps_steps(nq));
    centre = 16 * tile + (l & 15);
    aps_frame(step, l >> 4, f, b);
}

// Entry q of the affine tile: row `dir` (< 3: the direction of grad_P; the rows from 3 on are zero) holds L_f[b][dir], the
// coefficient of coordinate `dir` in output b of frame f, so that the tile's product with R is sum_f L_f^T r_f
FD_APS_HD inline void aps_affine_source(size_t q, int &dir, int &f, int &b)
{
    const int l = (int)(q & 63);
    dir = l & 15;
    aps_frame((int)(q >> 6), l >> 4, f, b);
}

// LDS of the main launch: the head and the affine tile stay; centre tiles are staged `tchunk` at a time
FD_APS_HD inline size_t aps_lds_fixed(int nq) { return 8 * aps_cen_at(nq); }
FD_APS_HD inline size_t aps_lds_per_tile(int nq) { return 8 * (size_t)(64 + aps_steps(nq) * 64); }
constexpr size_t kApsLdsBudget = 158 * 1024;         // fd_shared64.h's kS64LdsBudget
FD_APS_HD inline int aps_lds_tiles(int nq) { return (int)((kApsLdsBudget - aps_lds_fixed(nq)) / aps_lds_per_tile(nq)); }

}  // namespace fd
