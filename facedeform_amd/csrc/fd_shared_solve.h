// fd_shared_solve.h -- what the two shared-factor solve kernels of a shot have in common: k_ml_solve_shared
// (fd_build_ml_shared.hip, the Cholesky factors of the multilayer model's layers) and k_qnn_solve_shared
// (fd_build_qnn_shared.hip, the LU of the QNN model's kernel block).  Both cut the 3 F right-hand-side columns of the shot into
// tiles of 16, keep one workgroup's rows x 16 fp64 block in LDS, remove the least-squares polynomial from it and take it through
// triangular factors in 32-row blocks: the diagonal step a product with a stored inverse block, the update of the other rows
// rank-32 products on v_mfma_f64_16x16x4_f64, right-looking, the row tiles dealt to the four waves (no sum crosses a wave) with
// the next tile's operands in flight under the current one.  No atomics, fixed summation orders.
#pragma once

#include "fd_internal.h"

namespace fd {
namespace shared_solve {

typedef double double4_t __attribute__((ext_vector_type(4)));

// one 128-VGPR slot: these kernels run beside evaluation launches (see fd_nullspace.hip)
#define FD_FIT_BESIDE_EVAL __attribute__((amdgpu_waves_per_eu(4, 8)))

constexpr int kTile = 16;               // right-hand-side columns per workgroup: one MFMA tile
constexpr int kNB = 32;                 // the block width of the factorisations (fd_nullspace.hip, fd_build.hip)
constexpr int kMaxRows = 1024;          // 128 bytes of LDS per row of the block

// the eight A operands of one 16-row tile against a 32-column block: -op[c][g + 4 s], element (row, col) at base[col * lda + row].
// `base` is wave-uniform (column kb, row 0), the lane's part a 32-bit offset: scalar base + one address register per load
__device__ __forceinline__ void load_ops(double (&a)[8], gcdouble *base, int lda, unsigned lane_off)
{
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = -(base + (size_t)(4 * s) * lda)[lane_off];
}

// rows r0 .. r0+15 of the block take the contribution of the 32 solved rows whose values wait in yb (B operands)
__device__ __forceinline__ void update_tile(double *Bs, int r0, int c, int g, const double (&a)[8], const double (&yb)[8])
{
    double *p = Bs + (size_t)(r0 + g) * kTile + c;
    double4_t acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = p[4 * r * kTile];
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], yb[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) p[4 * r * kTile] = acc[r];
}

// The diagonal step, wave 0: rows kb .. kb+31 of the block <- Z (forward) or Z^T (backward) times themselves, in two parts.
// inv: row-major [k][j] = Z[k][j], lower triangular -- the half that is zero is skipped, which leaves twelve A operands:
// forward, rows 0..15 see columns 0..15 only; backward, rows 16..31 see rows 16..31 of the stored block only.
// load_inv fetches them (the sweeps do that one block ahead, under the update of the other rows: a step of the chain then
// waits for no load of its own), diag_apply is the products.
__device__ __forceinline__ void load_inv(double (&iv)[12], gcdouble *inv, int c, int g, bool transposed)
{
    int q = 0;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if ((!transposed && t == 0 && s >= 4) || (transposed && t == 1 && s < 4)) continue;
            const unsigned at = transposed ? (unsigned)((g + 4 * s) * kNB + 16 * t + c) : (unsigned)((16 * t + c) * kNB + g + 4 * s);
            iv[q++] = inv[at];
        }
}

__device__ __forceinline__ void diag_apply(double *Bs, int kb, int c, int g, const double (&iv)[12], bool transposed)
{
    double yb[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) yb[s] = Bs[(size_t)(kb + g + 4 * s) * kTile + c];
    double4_t acc[2];
    int q = 0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if ((!transposed && t == 0 && s >= 4) || (transposed && t == 1 && s < 4)) continue;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(iv[q++], yb[s], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) Bs[(size_t)(kb + 16 * t + g + 4 * r) * kTile + c] = acc[t][r];
}

// Which column of the shot a thread owns while the block is filled and handed off: thread (j, rg) has column j of the tile
// in the rows rg, rg + 16, ...; column gc = 3 f + comp is component comp of frame f.
struct Column {
    int j, rg, f, comp;
    bool live;
};
__device__ __forceinline__ Column own_column(int tid, int nF)
{
    Column o;
    o.j = tid & 15; o.rg = tid >> 4;
    const int gc = (int)blockIdx.x * kTile + o.j;
    o.live = gc < 3 * nF;
    o.f = o.live ? gc / 3 : 0; o.comp = o.live ? gc % 3 : 0;
    return o;
}

// Prologue: the deltas widened into the block (zeros below row M and in the columns past the shot's); then, T > 0, Q^T f
// through the shared reflectors V in place, the polynomial from its pivot rows, f - P a from the deltas anew -- k_ml_affine's
// arithmetic per column, the sixteen partial sums added in fixed order -- and the polynomial into `mine` (the owning frame's
// small block, where k_ml_finish / k_qnn_finish look for it).  small: the shared small block (tau, R); s_red: [16][kTile].
__device__ __forceinline__ void fit_polynomial(double *Bs, double *s_red, const Column &o, const float FD_GLOBAL *delta, gcdouble *V,
                                               gcdouble *small, gcdouble *centres, gdouble *mine, int M, int T, int rows,
                                               const MlSharedLayout &at)
{
    const int j = o.j, rg = o.rg, comp = o.comp;
    const bool live = o.live;
    for (int i = rg; i < rows; i += 16) Bs[(size_t)i * kTile + j] = (live && i < M) ? (double)delta[3 * (size_t)i + comp] : 0.0;
    if (T > 0) {
        for (int k = 0; k < T; ++k) {
            const int piv = M - 1 - k;
            const double tau = small[at.tau + k];
            double d = 0.0;
            for (int i = rg; i <= piv; i += 16) d = fma(V[4 * (size_t)i + k], Bs[(size_t)i * kTile + j], d);
            s_red[rg * kTile + j] = d;
            __syncthreads();
            d = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) d += s_red[q * kTile + j];
            for (int i = rg; i <= piv; i += 16) Bs[(size_t)i * kTile + j] = fma(-tau * d, V[4 * (size_t)i + k], Bs[(size_t)i * kTile + j]);
            __syncthreads();
        }
        double pa[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = T - 1; k >= 0; --k) {
            if (M - 1 - k < 0) continue;
            double v = Bs[(size_t)(M - 1 - k) * kTile + j];
            for (int cc = k + 1; cc < T; ++cc) v = fma(-small[at.R + 4 * k + cc], pa[cc], v);
            pa[k] = v / small[at.R + 4 * k + k];
        }
        __syncthreads();                  // everyone has read the pivot rows
        for (int i = rg; i < M; i += 16) {
            const double px = centres[3 * (size_t)i], py = centres[3 * (size_t)i + 1], pz = centres[3 * (size_t)i + 2];
            double v = live ? (double)delta[3 * (size_t)i + comp] : 0.0;
            v -= fma(pa[3], pz, fma(pa[2], py, fma(pa[1], px, pa[0])));
            Bs[(size_t)i * kTile + j] = live ? v : 0.0;
        }
        if (live && rg == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) mine[at.aff + 3 * k + comp] = pa[k];
        }
    }
    __syncthreads();
}

// The lower factor, top down over the rows [0, rows): block kb solved by the product with its inverse block (inv0 +
// (kb / 32) inv_stride, row-major, lower triangular), the rows below it updated from the 32 columns of A under the block.
__device__ __forceinline__ void sweep_down(double *Bs, gcdouble *A, int lda, int rows, gcdouble *inv0, size_t inv_stride, int wave,
                                           int c, int g)
{
    const unsigned goff = (unsigned)(g * lda + c);        // the lane's place in a 16-row, 4-column piece of the factor
    double iv[12];
    if (wave == 0) load_inv(iv, inv0, c, g, false);
#pragma unroll 1
    for (int kb = 0; kb < rows; kb += kNB) {
        const int nt = (rows - kb - kNB) / 16;            // row tiles below the block
        int t = wave;
        double an[8];
        if (t < nt) load_ops(an, A + (size_t)kb * lda, lda, goff + (unsigned)(kb + kNB + 16 * t));     // in flight under the diagonal step
        if (wave == 0) {
            diag_apply(Bs, kb, c, g, iv, false);
            if (kb + kNB < rows) load_inv(iv, inv0 + (size_t)(kb / kNB + 1) * inv_stride, c, g, false);  // the next block's, in flight under the update
        }
        __syncthreads();
        if (nt > 0) {
            double yb[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) yb[s] = Bs[(size_t)(kb + g + 4 * s) * kTile + c];
            while (t < nt) {
                double ac[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) ac[s] = an[s];
                const int tn = t + 4;
                if (tn < nt) load_ops(an, A + (size_t)kb * lda, lda, goff + (unsigned)(kb + kNB + 16 * tn));
                update_tile(Bs, kb + kNB + 16 * t, c, g, ac, yb);
                t = tn;
            }
            __syncthreads();
        }
    }
}

// The upper factor, bottom up: block kb solved by the product with the TRANSPOSE of the stored block at inv0 + (kb / 32)
// inv_stride (so the stored block is lower triangular here too), the rows above it updated from the 32 columns of A over the
// block -- the Cholesky factor's mirrored triangle, or the U of an LU.
__device__ __forceinline__ void sweep_up(double *Bs, gcdouble *A, int lda, int rows, gcdouble *inv0, size_t inv_stride, int wave,
                                         int c, int g)
{
    const unsigned goff = (unsigned)(g * lda + c);
    double iv[12];
    if (wave == 0) load_inv(iv, inv0 + (size_t)(rows / kNB - 1) * inv_stride, c, g, true);
#pragma unroll 1
    for (int kb = rows - kNB; kb >= 0; kb -= kNB) {
        const int nt = kb / 16;
        int t = wave;
        double an[8];
        if (t < nt) load_ops(an, A + (size_t)kb * lda, lda, goff + (unsigned)(16 * t));
        if (wave == 0) {
            diag_apply(Bs, kb, c, g, iv, true);
            if (kb > 0) load_inv(iv, inv0 + (size_t)(kb / kNB - 1) * inv_stride, c, g, true);
        }
        __syncthreads();
        if (nt > 0) {
            double yb[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) yb[s] = Bs[(size_t)(kb + g + 4 * s) * kTile + c];
            while (t < nt) {
                double ac[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) ac[s] = an[s];
                const int tn = t + 4;
                if (tn < nt) load_ops(an, A + (size_t)kb * lda, lda, goff + (unsigned)(16 * tn));
                update_tile(Bs, 16 * t, c, g, ac, yb);
                t = tn;
            }
            __syncthreads();
        }
    }
}

// What the shared factorisations in the scratch slots [0, nslots) reported -- coincident centres, a pivot or multiplier out of
// bounds, the pivot extremes, max |A|, the elimination steps done (the last slot's, as a per-context chain leaves them) -- into
// the DevModel of one frame, where k_pack looks for them.
__device__ __forceinline__ void hand_flags(DevModel *m, const BatchSlot *slots, int nslots)
{
    int dup = m->dup_flag, sing = m->sing_flag;
    unsigned long long amax = m->amax_bits, pmin = m->pivmin_bits, pmax = m->pivmax_bits;    // non-negative doubles: ordered as their bits
    for (int l = 0; l < nslots; ++l) {
        const DevModel *s = slots[l].model;
        dup |= s->dup_flag;
        sing |= s->sing_flag;
        amax = s->amax_bits > amax ? s->amax_bits : amax;
        pmin = s->pivmin_bits < pmin ? s->pivmin_bits : pmin;
        pmax = s->pivmax_bits > pmax ? s->pivmax_bits : pmax;
    }
    m->dup_flag = dup; m->sing_flag = sing;
    m->amax_bits = amax; m->pivmin_bits = pmin; m->pivmax_bits = pmax;
    m->iterations = slots[nslots - 1].model->iterations;
}

}  // namespace shared_solve
}  // namespace fd
