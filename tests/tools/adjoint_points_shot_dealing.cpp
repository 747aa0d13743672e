// The operand dealing of the shot form of the positional adjoint (facedeform_amd/csrc/fd_adjoint_points_shot.h) as a table, for
// tests/test_adjoint_points_shot_abi.py: the very inline functions the pack kernel and the main launch call, compiled for the
// host.  Usage: adjoint_points_shot_dealing NQ MPAD
//   W q centre f b     entry q of the weights holds component b of frame f's weight of `centre`
//   A q dir f b        entry q of the affine tile holds L_f[b][dir] (dir >= 3: zero)
//   S f b step k       component b of frame f is depth slot k of step `step`
//   L nq fixed per_tile tiles      LDS bytes that stay, bytes per tile of 16 centres, tiles that fit beside them
#include <cstdio>
#include <cstdlib>

#include "fd_adjoint_points_shot.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int nq = atoi(argv[1]), Mpad = atoi(argv[2]);
    const size_t nw = fd::aps_doubles(nq, Mpad) - fd::aps_w_at(nq, Mpad);
    for (size_t q = 0; q < nw; ++q) {
        int centre, f, b;
        fd::aps_weight_source(nq, q, centre, f, b);
        printf("W %zu %d %d %d\n", q, centre, f, b);
    }
    for (size_t q = 0; q < fd::aps_cen_at(nq) - fd::aps_aff_at(); ++q) {
        int dir, f, b;
        fd::aps_affine_source(q, dir, f, b);
        printf("A %zu %d %d %d\n", q, dir, f, b);
    }
    for (int f = 0; f < 4 * nq; ++f)
        for (int b = 0; b < 3; ++b) {
            int step, k;
            fd::aps_slot(f, b, step, k);
            int f2, b2;
            fd::aps_frame(step, k, f2, b2);
            if (f2 != f || b2 != b) return 3;
            printf("S %d %d %d %d\n", f, b, step, k);
        }
    for (int q = 1; q <= 8; ++q)
        printf("L %d %zu %zu %d\n", q, fd::aps_lds_fixed(q), fd::aps_lds_per_tile(q), fd::aps_lds_tiles(q));
    return 0;
}
