// fd_morph.hip -- next row N1: morph-space reprojection on the device.
//
// Replaces DirectBSEdit (reference src/dbse.hpp:7-33, src/dbse.cpp:9-87) and the loop that
// applies it (src/SOP_FaceDeform.cpp:444-473):
//   init            shapes matrix A (3N x S, fp64, column-major) of fp32 deltas shape - rest, and
//                   its Householder QR in Eigen's packed form (dbse.cpp:9-37)
//   compute weights w_s = sum_i float(P_i - rest_i) * QR[i][s]        (dbse.cpp:39-60)
//   displace        P = rest + sum_s float(A[.][s]) * clamp(float(3 w_s)) [+ (P - rest) * falloffradius]
//                                                                      (dbse.cpp:62-77, SOP :458-473)
// Everything is HBM-bound streaming over the 3N x S matrix: rows run along lanes (coalesced),
// columns are walked in order.  The per-cook passes read the matrix once each: 8 B per entry
// for the weights (the packed QR, fp64 as the reference keeps it) and 4 B per entry for the
// displacement (the unfactored deltas are fp32 values by construction; an fp32 copy is kept).
// The QR itself runs once per change of the blendshape set.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "facedeform_hip.h"
#include "fd_owned.h"
#include "fd_tuning.h"

namespace {

constexpr int kT = 256;             // threads per workgroup everywhere in this file
constexpr int kRowsPerWg = 4096;    // rows of the 3N x S matrix one workgroup walks (16 per thread)
constexpr int kR = kRowsPerWg / kT;

__device__ __forceinline__ double wg_sum(double v, double *scratch)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

// dbse.cpp:16-31: column s of the shapes matrix, fp32 delta widened (and its fp32 twin)
__global__ __launch_bounds__(kT) void k_shape_column(const float *rest, const float *shape, int64_t rows,
                                                      double *col64, float *col32)
{
    const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (e >= rows) return;
    const float d = shape[e] - rest[e];
    col64[e] = (double)d;
    col32[e] = d;
}

// ---- Householder QR, one column at a time (Eigen's unblocked order = LAPACK dgeqr2) ----------
// hh[0] = beta, hh[1] = tau, hh[2] = c0 - beta (0 when the reflector is the identity)

// partial sums of squares of x[k+1:]
__global__ __launch_bounds__(kT) void k_qr_tail_norm(const double *x, int64_t rows, int k, double *partial)
{
    __shared__ double scratch[4];
    const int64_t base = (int64_t)blockIdx.x * kRowsPerWg;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        const int64_t i = base + r * kT + threadIdx.x;
        if (i > k && i < rows) { const double v = x[i]; acc = fma(v, v, acc); }
    }
    acc = wg_sum(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// makeHouseholderInPlace (Eigen/src/Householder/Householder.h): beta, tau, the divisor of the tail
__global__ __launch_bounds__(kT) void k_qr_reflector(double *x, int k, const double *partial, int npartial,
                                                      double *hh, double *tau_out)
{
    __shared__ double scratch[4];
    double acc = 0.0;
    for (int q = threadIdx.x; q < npartial; q += kT) acc += partial[q];
    const double tail2 = wg_sum(acc, scratch);
    if (threadIdx.x == 0) {
        const double c0 = x[k];
        double beta, tau, denom;
        if (tail2 <= DBL_MIN) { tau = 0.0; beta = c0; denom = 0.0; }
        else {
            beta = sqrt(c0 * c0 + tail2);
            if (c0 >= 0.0) beta = -beta;
            denom = c0 - beta;
            tau = (beta - c0) / beta;
        }
        x[k] = beta;
        hh[0] = beta; hh[1] = tau; hh[2] = denom;
        tau_out[k] = tau;
    }
}

// scale the tail into the essential part v (in place) and form the partial dots v . a_j of every
// trailing column j: partial[wg * ld + (j - k - 1)].  Waves reduce their own column sums and park
// them in LDS; the workgroup synchronises once at the end.
__global__ __launch_bounds__(kT) void k_qr_dots(double *A, int64_t rows, int S, int k, const double *hh,
                                                 double *partial, int ld)
{
    extern __shared__ double s_part[];       // [4][S - k - 1]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nt = S - k - 1;
    const double denom = hh[2];
    double *x = A + (size_t)k * rows;
    const int64_t base = (int64_t)blockIdx.x * kRowsPerWg;
    double v[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        const int64_t i = base + r * kT + threadIdx.x;
        v[r] = 0.0;
        if (i > k && i < rows) {
            v[r] = denom != 0.0 ? x[i] / denom : 0.0;
            x[i] = v[r];
        }
    }
    for (int j = k + 1; j < S; ++j) {
        const double *a = A + (size_t)j * rows;
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int64_t i = base + r * kT + threadIdx.x;
            if (i > k && i < rows) acc = fma(v[r], a[i], acc);
        }
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) s_part[wave * nt + (j - k - 1)] = acc;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nt; q += kT)
        partial[(size_t)blockIdx.x * ld + q] = (s_part[q] + s_part[nt + q]) + (s_part[2 * nt + q] + s_part[3 * nt + q]);
}

// tmp_j = essential^T a_j + a_j[k]; the row-k update of applyHouseholderOnTheLeft happens here too
__global__ __launch_bounds__(kT) void k_qr_dots_reduce(double *A, int64_t rows, int k, const double *hh,
                                                        const double *partial, int npartial, int ld, double *tmp)
{
    __shared__ double scratch[4];
    const int j = k + 1 + blockIdx.x;
    double acc = 0.0;
    for (int q = threadIdx.x; q < npartial; q += kT) acc += partial[(size_t)q * ld + blockIdx.x];
    acc = wg_sum(acc, scratch);
    if (threadIdx.x == 0) {
        double *a = A + (size_t)j * rows;
        const double t = acc + a[k];
        tmp[blockIdx.x] = t;
        a[k] -= hh[1] * t;
    }
}

// bottom -= tau * essential * tmp
__global__ __launch_bounds__(kT) void k_qr_apply(double *A, int64_t rows, int S, int k, const double *hh,
                                                  const double *tmp)
{
    const double tau = hh[1];
    const double *x = A + (size_t)k * rows;
    const int64_t base = (int64_t)blockIdx.x * kRowsPerWg;
    double v[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        const int64_t i = base + r * kT + threadIdx.x;
        v[r] = (i > k && i < rows) ? x[i] : 0.0;
    }
    for (int j = k + 1; j < S; ++j) {
        double *a = A + (size_t)j * rows;
        const double t = tmp[j - k - 1];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int64_t i = base + r * kT + threadIdx.x;
            if (i > k && i < rows) a[i] -= tau * v[r] * t;
        }
    }
}

// ---- Householder QR, blocked (default) --------------------------------------------------------
// Same reflectors as the column-by-column form above (Eigen's HouseholderQR is itself a panel
// factorisation followed by a block-reflector update: Eigen/src/QR/HouseholderQR.h,
// householder_qr_inplace_blocked), far fewer passes over the 3N x S matrix:
//   inside a panel of kNB columns ONE pass per column: it applies reflector k to the panel's later
//     columns and, while their updated values are in registers, forms the tail norm of column k+1
//     and its dot products with the columns after it -- everything the next reflector needs;
//   behind a panel the kNB reflectors go through the trailing columns together (compact WY:
//     C -= V T^T (V^T C)): one read-only pass for V^T C and V^T V, one read-write pass that also
//     forms the first column's sums for the next panel.
// Passes over a column: ~(kNB + 1) S inside panels + 3 S^2 / (2 kNB) behind them, instead of 1.5 S^2.
constexpr int kNB = 8;              // panel width
constexpr int kBR = 4;              // rows per lane
constexpr int kBRows = kBR * kT;    // rows per workgroup
constexpr int kSlices = 16;         // first-stage slices of the reduction over workgroups

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// acc[0..nq) summed over the workgroup -> out[0..nq)
__device__ __forceinline__ void wg_reduce_store(const double (&acc)[kNB], int nq, double *s_red /* [4][kNB] */, double *out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < kNB; ++q) {
        if (q < nq) {
            const double t = wave_sum(acc[q]);
            if (lane == 0) s_red[wave * kNB + q] = t;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nq)
        out[threadIdx.x] = (s_red[threadIdx.x] + s_red[kNB + threadIdx.x]) + (s_red[2 * kNB + threadIdx.x] + s_red[3 * kNB + threadIdx.x]);
}

// sums of column k against itself and the nq - 1 columns after it over the rows below k (first panel only)
__global__ __launch_bounds__(kT) void k_qr_gram(const double *A, int64_t rows, int k, int nq, double *partial)
{
    __shared__ double s_red[4 * kNB];
    const int64_t base = (int64_t)blockIdx.x * kBRows;
    double acc[kNB];
#pragma unroll
    for (int q = 0; q < kNB; ++q) acc[q] = 0.0;
#pragma unroll
    for (int r = 0; r < kBR; ++r) {
        const int64_t i = base + r * kT + threadIdx.x;
        if (i > k && i < rows) {
            const double u = A[(size_t)k * rows + i];
#pragma unroll
            for (int q = 0; q < kNB; ++q)
                if (q < nq) acc[q] = fma(u, q == 0 ? u : A[(size_t)(k + q) * rows + i], acc[q]);
        }
    }
    wg_reduce_store(acc, nq, s_red, partial + (size_t)blockIdx.x * kNB);
}

// One workgroup: the sums of the nwg workgroups -> reflector k (makeHouseholderInPlace), the
// products tmp_l = essential . a_l + a_l[k] of the panel's later columns, and their row-k update.
constexpr int kSetupT = 1024;
__global__ __launch_bounds__(kSetupT) void k_qr_col_setup(double *A, int64_t rows, int k, int nq, const double *partial, int nwg,
                                                           double *hh, double *tau_out, double *tmp)
{
    __shared__ double s_acc[kSetupT];
    __shared__ double tot[kNB];
    __shared__ double sh[2];
    const int q = threadIdx.x & (kNB - 1), w0 = threadIdx.x / kNB;       // 128 workgroups' sums per sweep
    constexpr int kSweep = kSetupT / kNB;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;                       // four loads in flight per lane
    int w = w0;
    for (; w + 3 * kSweep < nwg; w += 4 * kSweep) {
        a0 += partial[(size_t)w * kNB + q];
        a1 += partial[(size_t)(w + kSweep) * kNB + q];
        a2 += partial[(size_t)(w + 2 * kSweep) * kNB + q];
        a3 += partial[(size_t)(w + 3 * kSweep) * kNB + q];
    }
    for (; w < nwg; w += kSweep) a0 += partial[(size_t)w * kNB + q];
    s_acc[threadIdx.x] = q < nq ? (a0 + a1) + (a2 + a3) : 0.0;
    __syncthreads();
    if (threadIdx.x < 64) {                                              // 8 lanes per quantity, 16 sums each
        const int qq = threadIdx.x & (kNB - 1), part = threadIdx.x / kNB;
        double t = 0.0;
        for (int j = part; j < kSweep; j += 8) t += s_acc[j * kNB + qq];
        t += __shfl_xor(t, 8); t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
        if (threadIdx.x < kNB) tot[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *x = A + (size_t)k * rows;
        const double c0 = x[k], tail2 = tot[0];
        double beta, tau, denom;
        if (tail2 <= DBL_MIN) { tau = 0.0; beta = c0; denom = 0.0; }
        else {
            beta = sqrt(c0 * c0 + tail2);
            if (c0 >= 0.0) beta = -beta;
            denom = c0 - beta;
            tau = (beta - c0) / beta;
        }
        x[k] = beta;
        hh[0] = beta; hh[1] = tau; hh[2] = denom;
        tau_out[k] = tau;
        sh[0] = tau; sh[1] = denom;
    }
    __syncthreads();
    if (threadIdx.x >= 1 && (int)threadIdx.x < nq) {
        double *a = A + (size_t)(k + threadIdx.x) * rows + k;
        const double t = (sh[1] != 0.0 ? tot[threadIdx.x] / sh[1] : 0.0) + *a;
        tmp[threadIdx.x - 1] = t;
        *a -= sh[0] * t;
    }
}

// The pass of column k inside its panel [.., pend): scale the tail into the essential part, apply
// the reflector to the panel's later columns, and form column k+1's sums from the updated values.
__global__ __launch_bounds__(kT) void k_qr_panel_apply(double *A, int64_t rows, int k, int pend, const double *hh,
                                                        const double *tmp, double *partial)
{
    __shared__ double s_red[4 * kNB];
    const double tau = hh[1], denom = hh[2];
    const int nl = pend - k - 1;                         // later columns of the panel: 0 .. kNB-1
    double t[kNB - 1];
#pragma unroll
    for (int l = 0; l < kNB - 1; ++l) t[l] = l < nl ? tmp[l] : 0.0;
    const int64_t base = (int64_t)blockIdx.x * kBRows;
    double acc[kNB];
#pragma unroll
    for (int q = 0; q < kNB; ++q) acc[q] = 0.0;
    double *x = A + (size_t)k * rows;
#pragma unroll
    for (int r = 0; r < kBR; ++r) {
        const int64_t i = base + r * kT + threadIdx.x;
        if (i > k && i < rows) {
            const double v = denom != 0.0 ? x[i] / denom : 0.0;
            x[i] = v;
            double val[kNB - 1];
#pragma unroll
            for (int l = 0; l < kNB - 1; ++l) {
                if (l < nl) {
                    double *a = A + (size_t)(k + 1 + l) * rows + i;
                    val[l] = *a - tau * v * t[l];
                    *a = val[l];
                } else val[l] = 0.0;
            }
            if (i > k + 1) {
#pragma unroll
                for (int l = 0; l < kNB - 1; ++l)
                    if (l < nl) acc[l] = fma(val[0], val[l], acc[l]);
            }
        }
    }
    if (nl > 0) wg_reduce_store(acc, nl, s_red, partial + (size_t)blockIdx.x * kNB);
}

// V of the panel [k0, k0 + nb) as the block reflector sees it: unit diagonal, zeros above it
__device__ __forceinline__ double wy_v(const double *A, int64_t rows, int col, int64_t i)
{
    return i > col && i < rows ? A[(size_t)col * rows + i] : (i == col ? 1.0 : 0.0);
}

// 8 per-lane values, summed over the 64 lanes, for 8 different quantities at once: halve the set at
// each of the first three exchange steps (10 exchanges instead of 48).  The sum of quantity
// p = 4 b5 + 2 b4 + b3 ends in every lane whose bits 5, 4, 3 are (b5, b4, b3).
__device__ __forceinline__ double wave_sum8(const double (&a)[kNB])
{
    const int lane = threadIdx.x & 63;
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
    double b[4], c[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double keep = h5 ? a[4 + i] : a[i], send = h5 ? a[i] : a[4 + i];
        b[i] = keep + __shfl_xor(send, 32);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double keep = h4 ? b[2 + i] : b[i], send = h4 ? b[i] : b[2 + i];
        c[i] = keep + __shfl_xor(send, 16);
    }
    double d = (h3 ? c[1] : c[0]) + __shfl_xor(h3 ? c[0] : c[1], 8);
    d += __shfl_xor(d, 4);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 1);
    return d;
}

// partial[wg][c * kNB + p] = sum over the workgroup's rows of V[.][p] C[.][c]   (c < ntrail), then
// partial[wg][ntrail * kNB + q (q - 1) / 2 + p] = V[.][p] . V[.][q]            (p < q < nb)
__global__ __launch_bounds__(kT) void k_qr_wy_dots(const double *A, int64_t rows, int k0, int nb, int S, double *partial, int ld)
{
    extern __shared__ double s_part[];       // [4][ld]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pend = k0 + nb, ntrail = S - pend;
    const int64_t base = (int64_t)blockIdx.x * kBRows;
    double V[kBR][kNB];
#pragma unroll
    for (int r = 0; r < kBR; ++r)
#pragma unroll
        for (int p = 0; p < kNB; ++p) V[r][p] = p < nb ? wy_v(A, rows, k0 + p, base + r * kT + threadIdx.x) : 0.0;
    const int myp = ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
    double cur[kBR], nxt[kBR];
    auto load = [&](int c, double (&dst)[kBR]) {
        const double *col = A + (size_t)(pend + c) * rows;
#pragma unroll
        for (int r = 0; r < kBR; ++r) {
            const int64_t i = base + r * kT + threadIdx.x;
            dst[r] = i >= k0 && i < rows ? col[i] : 0.0;
        }
    };
    if (ntrail > 0) load(0, cur);
    for (int c = 0; c < ntrail; ++c) {
        if (c + 1 < ntrail) load(c + 1, nxt);
        double acc[kNB];
#pragma unroll
        for (int p = 0; p < kNB; ++p) {
            acc[p] = 0.0;
#pragma unroll
            for (int r = 0; r < kBR; ++r) acc[p] = fma(V[r][p], cur[r], acc[p]);
        }
        const double d = wave_sum8(acc);
        if ((lane & 7) == 0) s_part[wave * ld + c * kNB + myp] = d;
#pragma unroll
        for (int r = 0; r < kBR; ++r) cur[r] = nxt[r];
    }
    // V^T V, strictly upper part, in groups of 8 quantities
    {
        double acc[kNB];
        int filled = 0, first = 0;
#pragma unroll
        for (int q = 1; q < kNB; ++q)
#pragma unroll
            for (int p = 0; p < q; ++p) {
                double a = 0.0;
#pragma unroll
                for (int r = 0; r < kBR; ++r) a = fma(V[r][p], V[r][q], a);
                acc[filled++] = a;
                if (filled == kNB || (q == kNB - 1 && p == q - 1)) {
                    for (int z = filled; z < kNB; ++z) acc[z] = 0.0;
                    const double d = wave_sum8(acc);
                    if ((lane & 7) == 0 && myp < filled) s_part[wave * ld + ntrail * kNB + first + myp] = d;
                    first += filled;
                    filled = 0;
                }
            }
    }
    __syncthreads();
    const int nvals = ntrail * kNB + kNB * (kNB - 1) / 2;
    for (int q = threadIdx.x; q < nvals; q += kT)
        partial[(size_t)blockIdx.x * ld + q] = (s_part[q] + s_part[ld + q]) + (s_part[2 * ld + q] + s_part[3 * ld + q]);
}

// first stage of the sum over workgroups: slice y of them, 32 consecutive values per workgroup
__global__ __launch_bounds__(kT) void k_qr_wy_reduce(const double *partial, int nwg, int ld, int nvals, double *partial2)
{
    __shared__ double s[kT];
    const int idx = blockIdx.x * 32 + (threadIdx.x & 31), wl = threadIdx.x >> 5;
    const int per = (nwg + kSlices - 1) / kSlices;
    const int w_lo = blockIdx.y * per, w_hi = min(nwg, w_lo + per);
    double acc = 0.0;
    if (idx < nvals)
        for (int w = w_lo + wl; w < w_hi; w += kT / 32) acc += partial[(size_t)w * ld + idx];
    s[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < 32 && idx < nvals) {
        double t = 0.0;
        for (int j = 0; j < kT / 32; ++j) t += s[j * 32 + threadIdx.x];
        partial2[(size_t)blockIdx.y * ld + idx] = t;
    }
}

// One workgroup: W = V^T C and V^T V from the slices, the triangular factor T of the block
// reflector H_0 .. H_{nb-1} = I - V T V^T (T_jj = tau_j, T[0:j][j] = -tau_j T[0:j][0:j] V[:, 0:j]^T v_j),
// and Y = T^T W for the update C -= V Y.
__global__ __launch_bounds__(kT) void k_qr_wy_T(const double *partial2, int ld, int k0, int nb, int ntrail, const double *tau,
                                                 double *Y)
{
    extern __shared__ double s_w[];          // [ld] sums, then [kNB * kNB] T
    double *T = s_w + ld;
    const int nvals = ntrail * kNB + kNB * (kNB - 1) / 2;
    for (int q = threadIdx.x; q < nvals; q += kT) {
        double t = 0.0;
        for (int y = 0; y < kSlices; ++y) t += partial2[(size_t)y * ld + q];
        s_w[q] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double *vtv = s_w + ntrail * kNB;           // (p < q) at q (q - 1) / 2 + p
        for (int j = 0; j < kNB; ++j)
            for (int i = 0; i < kNB; ++i) T[i * kNB + j] = 0.0;
        for (int j = 0; j < nb; ++j) {
            const double tj = tau[k0 + j];
            for (int i = 0; i < j; ++i) {
                double acc = 0.0;
                for (int z = i; z < j; ++z) acc = fma(T[i * kNB + z], vtv[j * (j - 1) / 2 + z], acc);
                T[i * kNB + j] = -tj * acc;
            }
            T[j * kNB + j] = tj;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nb * ntrail; e += kT) {
        const int p = e / ntrail, c = e - p * ntrail;
        double acc = 0.0;
        for (int q = 0; q <= p; ++q) acc = fma(T[q * kNB + p], s_w[c * kNB + q], acc);
        Y[(size_t)p * ntrail + c] = acc;
    }
}

// C -= V Y over the trailing columns; the next panel's first column leaves its sums behind
__global__ __launch_bounds__(kT) void k_qr_wy_apply(double *A, int64_t rows, int k0, int nb, int S, const double *Y,
                                                     int next_nq, double *partial)
{
    extern __shared__ double s_y[];          // [nb][ntrail], then 4 * kNB of reduction scratch
    const int pend = k0 + nb, ntrail = S - pend;
    for (int e = threadIdx.x; e < nb * ntrail; e += kT) s_y[e] = Y[e];
    double *s_red = s_y + kNB * ntrail;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kBRows;
    double V[kBR][kNB];
#pragma unroll
    for (int r = 0; r < kBR; ++r)
#pragma unroll
        for (int p = 0; p < kNB; ++p) V[r][p] = p < nb ? wy_v(A, rows, k0 + p, base + r * kT + threadIdx.x) : 0.0;
    double acc[kNB], u[kBR];
#pragma unroll
    for (int q = 0; q < kNB; ++q) acc[q] = 0.0;
    double cur[kBR], nxt[kBR];
    auto load = [&](int c, double (&dst)[kBR]) {
        const double *col = A + (size_t)(pend + c) * rows;
#pragma unroll
        for (int r = 0; r < kBR; ++r) {
            const int64_t i = base + r * kT + threadIdx.x;
            dst[r] = i >= k0 && i < rows ? col[i] : 0.0;
        }
    };
    load(0, cur);
    for (int c = 0; c < ntrail; ++c) {
        if (c + 1 < ntrail) load(c + 1, nxt);
        double *col = A + (size_t)(pend + c) * rows;
        double y[kNB];
#pragma unroll
        for (int p = 0; p < kNB; ++p) y[p] = p < nb ? s_y[p * ntrail + c] : 0.0;
        double dot = 0.0;
#pragma unroll
        for (int r = 0; r < kBR; ++r) {
            const int64_t i = base + r * kT + threadIdx.x;
            double d = 0.0;
#pragma unroll
            for (int p = 0; p < kNB; ++p) d = fma(V[r][p], y[p], d);
            const double x = cur[r] - d;
            if (i >= k0 && i < rows) col[i] = x;
            if (c == 0) u[r] = i > pend && i < rows ? x : 0.0;
            dot = fma(u[r], x, dot);
        }
#pragma unroll
        for (int q = 0; q < kNB; ++q)
            if (q == c && c < next_nq) acc[q] = dot;
#pragma unroll
        for (int r = 0; r < kBR; ++r) cur[r] = nxt[r];
    }
    wg_reduce_store(acc, next_nq, s_red, partial + (size_t)blockIdx.x * kNB);
}

// ---- per cook --------------------------------------------------------------------------------
// dbse.cpp:39-60: partial[wg * S + s] = sum over the workgroup's rows of float(P - rest) * QR[.][s].
// A lane keeps its kWR deltas in registers and walks the columns; a wave reduces each column by
// itself and parks the result in LDS, so nothing but the last step synchronises the workgroup
// (with a workgroup-wide reduction per column this pass ran at 2.9 TB/s).
constexpr int kWR = 8;                       // rows per lane
constexpr int kWRows = kWR * kT;             // rows per workgroup
__global__ __launch_bounds__(kT) void k_morph_weights(const double *QR, int64_t rows, int S, const float *P,
                                                       const float *rest, double *partial)
{
    extern __shared__ double s_part[];       // [4][S]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kWRows;
    double d[kWR];
#pragma unroll
    for (int r = 0; r < kWR; ++r) {
        const int64_t i = base + r * kT + threadIdx.x;
        d[r] = i < rows ? (double)(P[i] - rest[i]) : 0.0;          // fp32 subtraction, then widened (:49-51)
    }
    const bool full = base + kWRows <= rows;
    for (int s = 0; s < S; ++s) {
        const double *q = QR + (size_t)s * rows + base + threadIdx.x;
        double v[kWR];
        if (full) {
#pragma unroll
            for (int r = 0; r < kWR; ++r) v[r] = __builtin_nontemporal_load(q + r * kT);
        } else {
#pragma unroll
            for (int r = 0; r < kWR; ++r) v[r] = base + r * kT + threadIdx.x < rows ? q[r * kT] : 0.0;
        }
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < kWR; ++r) acc = fma(d[r], v[r], acc);
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) s_part[wave * S + s] = acc;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += kT)
        partial[(size_t)blockIdx.x * S + s] = (s_part[s] + s_part[S + s]) + (s_part[2 * S + s] + s_part[3 * S + s]);
}

__global__ __launch_bounds__(kT) void k_morph_weights_reduce(const double *partial, int npartial, int S, double *w)
{
    __shared__ double scratch[4];
    const int s = blockIdx.x;
    double acc = 0.0;
    for (int q = threadIdx.x; q < npartial; q += kT) acc += partial[(size_t)q * S + s];
    acc = wg_sum(acc, scratch);
    if (threadIdx.x == 0) w[s] = acc;
}

// dbse.cpp:62-77 and SOP_FaceDeform.cpp:458-473, fp32 in the reference's order (this file is
// built with -ffp-contract=off: multiply and add stay separate roundings, as in unfused CPU code)
__global__ __launch_bounds__(kT) void k_morph_displace(const float *S32, int64_t N, int S, const double *w,
                                                        float clamp_lo, float clamp_hi, int do_clamp, int add_delta,
                                                        float falloffradius, const float *rest, float *P)
{
    extern __shared__ float s_cw[];
    for (int s = threadIdx.x; s < S; s += kT) {
        const float ws = (float)(w[s] * 3);                        // :70
        s_cw[s] = do_clamp ? (ws < clamp_lo ? clamp_lo : (ws > clamp_hi ? clamp_hi : ws)) : ws;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= N) return;
    const int64_t rows = 3 * N;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    for (int s = 0; s < S; ++s) {
        const float *c = S32 + (size_t)s * rows + 3 * i;
        const float cw = s_cw[s];
        dx = dx + c[0] * cw; dy = dy + c[1] * cw; dz = dz + c[2] * cw;
    }
    const float rx = rest[3 * i], ry = rest[3 * i + 1], rz = rest[3 * i + 2];
    if (add_delta) {
        dx = dx + (P[3 * i] - rx) * falloffradius;
        dy = dy + (P[3 * i + 1] - ry) * falloffradius;
        dz = dz + (P[3 * i + 2] - rz) * falloffradius;
    }
    P[3 * i] = rx + dx; P[3 * i + 1] = ry + dy; P[3 * i + 2] = rz + dz;
}

// ---- per group of frames (a shot) -------------------------------------------------------------
// Neither matrix depends on the frame, so the F frames of a group share one pass over each:
//   weights       W^T (S x F) = QR^T (S x 3N) . D (3N x F),  D[i][f] = double(float(P_f[i] - rest[i])),  fp64
//   displacement  d_f[i] = sum_s delta[i][s] * cw[f][s],  fp32 in the one-frame kernel's operation order
struct MorphFrames { const float *p[FD_MAX_BATCH]; };
struct MorphFramesRW { float *p[FD_MAX_BATCH]; };

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int kBK = 64;              // rows of a staged chunk (one per lane of the wave that fetches a column span)
constexpr int kBLd = kBK + 2;        // its LDS row stride, in doubles
constexpr int kBCols = 64;           // columns per workgroup: four 16-wide tiles
constexpr int kBFr = FD_MAX_BATCH;   // frames: two 16-wide tiles
constexpr int kBMaxWg = 512;         // row partitions at most (the length of the second launch's sums)
static_assert(kBFr == 32 && kBFr <= kBLd, "two frame tiles; the tile of sums reuses the staged columns");

// v_mfma_f64_16x16x4_f64 with the columns as M, the frames as N and the rows of the matrix as K: lane l gives
// QR[k + (l >> 4)][16 t + (l & 15)] and D[k + (l >> 4)][16 u + (l & 15)] and holds the sums of column
// 16 t + (l >> 4) + 4 r, frame 16 u + (l & 15) in element r.  Workgroup (x, y): rows [x * chunks_per_wg * kBK, ..),
// columns [y * kBCols, ..).  A chunk is fetched one 512-byte column span per wave instruction (row = lane),
// parked in LDS and read back in operand order; every wave multiplies its own 16 of the chunk's rows into all
// eight tiles while the next chunk's loads are in flight.  Columns past S, frames past F and rows past 3N are
// zero operands, never loads.  partial[(x * F + f) * ldp + column], summed by k_morph_weights_batch_reduce in a fixed
// order: no atomics.
__global__ __launch_bounds__(kT) void k_morph_weights_batch(const double *QR, int64_t rows, int S, int F, MorphFrames fr,
                                                             const float *rest, int chunks_per_wg, double *partial, int ldp)
{
    __shared__ double sQ[kBCols * kBLd];
    __shared__ double sD[kBFr * kBLd];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col0 = blockIdx.y * kBCols;
    const int ncols = S - col0 < kBCols ? S - col0 : kBCols;
    const int nst = (ncols + 15) >> 4, nft = (F + 15) >> 4;
    const int64_t nchunks = (rows + kBK - 1) / kBK;
    const int64_t chunk_lo = (int64_t)blockIdx.x * chunks_per_wg;
    const int64_t chunk_hi = chunk_lo + chunks_per_wg < nchunks ? chunk_lo + chunks_per_wg : nchunks;

    double q[kBCols / 4];            // columns wave, wave + 4, ..: row lane of the chunk
    float dl[kBFr / 4];              // frames wave, wave + 4, ..: float(P - rest) of that row (:49-51)
    auto fetch = [&](int64_t chunk) {
        const int64_t i = chunk * kBK + lane;
        const bool in = i < rows;
#pragma unroll
        for (int j = 0; j < kBCols / 4; ++j) {
            const int c = wave + 4 * j;
            q[j] = in && c < ncols ? __builtin_nontemporal_load(QR + (size_t)(col0 + c) * rows + i) : 0.0;
        }
        const float r = in ? rest[i] : 0.f;
#pragma unroll
        for (int j = 0; j < kBFr / 4; ++j) {
            const int f = wave + 4 * j;
            dl[j] = in && f < F ? fr.p[f][i] - r : 0.f;
        }
    };

    double4_t acc[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[t][u] = double4_t{0.0, 0.0, 0.0, 0.0};

    fetch(chunk_lo);
    for (int64_t chunk = chunk_lo; chunk < chunk_hi; ++chunk) {
        __syncthreads();             // the previous chunk has been read
#pragma unroll
        for (int j = 0; j < kBCols / 4; ++j) sQ[(wave + 4 * j) * kBLd + lane] = q[j];
#pragma unroll
        for (int j = 0; j < kBFr / 4; ++j) sD[(wave + 4 * j) * kBLd + lane] = (double)dl[j];
        __syncthreads();
        if (chunk + 1 < chunk_hi) fetch(chunk + 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int k = 16 * wave + 4 * ks + (lane >> 4);
            const double b0 = sD[(lane & 15) * kBLd + k];
            const double b1 = nft > 1 ? sD[(16 + (lane & 15)) * kBLd + k] : 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < nst) {
                    const double a = sQ[(16 * t + (lane & 15)) * kBLd + k];
                    acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[t][0], 0, 0, 0);
                    if (nft > 1) acc[t][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[t][1], 0, 0, 0);
                }
            }
        }
    }
    // the four waves' sums, added in wave order into one tile [frame][column]
    double *sOut = sQ;
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double *o = sOut + (16 * u + (lane & 15)) * kBCols + 16 * t + (lane >> 4) + 4 * r;
                        *o = w == 0 ? acc[t][u][r] : *o + acc[t][u][r];
                    }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < F * kBCols; e += kT)
        partial[((size_t)blockIdx.x * F + (e >> 6)) * ldp + col0 + (e & 63)] = sOut[e];
}

// w[f * S + column]: the row partitions' sums in four slices of consecutive partitions, then the slices in order
__global__ __launch_bounds__(kT) void k_morph_weights_batch_reduce(const double *partial, int nwg, int S, int F, int ldp, double *w)
{
    __shared__ double s[kT];
    const int f = blockIdx.y, c = blockIdx.x * kBCols + (threadIdx.x & 63), slice = threadIdx.x >> 6;
    const int per = (nwg + 3) / 4, lo = slice * per, hi = lo + per < nwg ? lo + per : nwg;
    const double *p = partial + (size_t)f * ldp + c;
    const size_t stride = (size_t)F * ldp;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;       // four loads in flight per lane
    int x = lo;
    for (; x + 3 < hi; x += 4) {
        a0 += p[x * stride];
        a1 += p[(x + 1) * stride];
        a2 += p[(x + 2) * stride];
        a3 += p[(x + 3) * stride];
    }
    for (; x < hi; ++x) a0 += p[x * stride];
    s[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (threadIdx.x < 64 && c < S)
        w[(size_t)f * S + c] = (s[threadIdx.x] + s[64 + threadIdx.x]) + (s[128 + threadIdx.x] + s[192 + threadIdx.x]);
}

// k_morph_displace for F frames at once: a lane owns a vertex, reads the three deltas of column s once and updates
// every frame's sum with it -- the same `d = d + c * cw` per frame, columns in order, multiply and add rounded
// separately, so frame f's result is the one-frame kernel's bit for bit.  The clamped weights of kDCols columns at
// a time sit in LDS as [column][FT]; all lanes read the same four frames with one broadcast load.  FT: the frame
// count rounded up (the sums are registers, 3 FT of them); frames past F carry a zero weight and are not stored.
constexpr int kDCols = 64;
constexpr int kDAhead = 4;           // columns whose deltas are requested ahead of the one being applied
template <int FT>
__global__ __launch_bounds__(kT) void k_morph_displace_batch(const float *S32, int64_t N, int S, int F, const double *w,
                                                              float clamp_lo, float clamp_hi, int do_clamp, int add_delta,
                                                              float falloffradius, const float *rest, MorphFramesRW fr)
{
    __shared__ float4 s_cw[kDCols * FT / 4];
    const int64_t i0 = (int64_t)blockIdx.x * kT + threadIdx.x;
    const bool live = i0 < N;
    const int64_t i = live ? i0 : N - 1;                   // idle lanes of the last workgroup: valid loads, no stores
    const int64_t rows = 3 * N;
    float dx[FT], dy[FT], dz[FT];
#pragma unroll
    for (int f = 0; f < FT; ++f) dx[f] = dy[f] = dz[f] = 0.f;
    for (int s0 = 0; s0 < S; s0 += kDCols) {
        const int ns = S - s0 < kDCols ? S - s0 : kDCols;
        __syncthreads();
        for (int e = threadIdx.x; e < ns * FT; e += kT) {
            const int s = e / FT, f = e % FT;
            float v = 0.f;
            if (f < F) {
                const float ws = (float)(w[(size_t)f * S + s0 + s] * 3);                   // :70
                v = do_clamp ? (ws < clamp_lo ? clamp_lo : (ws > clamp_hi ? clamp_hi : ws)) : ws;
            }
            reinterpret_cast<float *>(s_cw)[e] = v;
        }
        __syncthreads();
        const float *col = S32 + (size_t)s0 * rows + 3 * i;
        float c[kDAhead][3];                               // the deltas of columns s .. s + kDAhead - 1, in flight
        auto fetch = [&](int s, float (&dst)[3]) {
            const float *p = col + (size_t)(s < ns ? s : ns - 1) * rows;
            dst[0] = __builtin_nontemporal_load(p);
            dst[1] = __builtin_nontemporal_load(p + 1);
            dst[2] = __builtin_nontemporal_load(p + 2);
        };
#pragma unroll
        for (int j = 0; j < kDAhead; ++j) fetch(j, c[j]);
#pragma unroll 1
        for (int s = 0; s < ns; ++s) {
            const float cx = c[0][0], cy = c[0][1], cz = c[0][2];
#pragma unroll
            for (int j = 0; j + 1 < kDAhead; ++j) { c[j][0] = c[j + 1][0]; c[j][1] = c[j + 1][1]; c[j][2] = c[j + 1][2]; }
            fetch(s + kDAhead, c[kDAhead - 1]);
#pragma unroll
            for (int b = 0; b < FT / 4; ++b) {
                if (4 * b < F) {
                    const float4 cw = s_cw[s * (FT / 4) + b];
                    const float cwv[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        dx[4 * b + a] = dx[4 * b + a] + cx * cwv[a];
                        dy[4 * b + a] = dy[4 * b + a] + cy * cwv[a];
                        dz[4 * b + a] = dz[4 * b + a] + cz * cwv[a];
                    }
                }
            }
        }
    }
    const float rx = rest[3 * i], ry = rest[3 * i + 1], rz = rest[3 * i + 2];
#pragma unroll
    for (int f = 0; f < FT; ++f) {
        if (f < F && live) {
            float *P = fr.p[f];
            float ax = dx[f], ay = dy[f], az = dz[f];
            if (add_delta) {
                ax = ax + (P[3 * i] - rx) * falloffradius;
                ay = ay + (P[3 * i + 1] - ry) * falloffradius;
                az = az + (P[3 * i + 2] - rz) * falloffradius;
            }
            P[3 * i] = rx + ax; P[3 * i + 1] = ry + ay; P[3 * i + 2] = rz + az;
        }
    }
}

thread_local char g_merr[512] = {0};

}  // namespace

using fd::DevBuf;
using fd::Event;
using fd::Stream;

struct fd_morph {
    int device = 0;
    int64_t N = 0;
    int S = 0;
    bool initialised = false, computed = false;
    Stream stream;                // in front of what is enqueued on it: it outlives the buffers and events below
    DevBuf<float> d_rest, d_S32, d_stage, d_P;
    // the `rest` point attribute the cook passes use (SOP_FaceDeform.cpp:178-184,445); NULL: the
    // init rest pose (they differ only when input 0 carries its own rest attribute)
    DevBuf<float> d_rest_attr;
    bool use_rest_attr = false;
    DevBuf<double> d_QR, d_tau, d_w, d_partial, d_hh, d_tmp;
    DevBuf<double> d_bpartial, d_bpartial2, d_Y;    // blocked factorisation
    size_t cap_entries = 0;       // 3N * S capacity of d_QR / d_S32
    int64_t cap_N = 0;
    int cap_S = 0;
    // a group of frames (fd_morph_*_batch*): weights F x S and the row partitions' sums, apart from d_w / computed
    DevBuf<double> d_bw, d_bwpartial;
    int batch_F = 0;              // frames of the last batched compute; 0: none since fd_morph_init
    Event ev0, ev1;
    float last_init_ms = 0.f;
    char err[512] = {0};
};

static void merr(fd_morph *m, const char *fmt, ...)
{
    char *dst = m ? m->err : g_merr;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
}

#define FDM_HIP(m, call)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            merr(m, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return FD_E_DEVICE;                                                              \
        }                                                                                    \
    } while (0)

// DevBuf's alloc -- with kGrow its grow: a scratch that grows on demand and never shrinks -- and the handle's error text
constexpr bool kGrow = true;
template <typename T>
static int mrealloc(fd_morph *m, DevBuf<T> &b, size_t count, bool grow = false)
{
    if ((grow ? b.grow(count) : b.alloc(count)) == hipSuccess) return FD_OK;
    merr(m, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(hipGetLastError()));
    return FD_E_NOMEM;
}

// row length of the per-workgroup sums the block-reflector pass leaves: kNB per trailing column + V^T V
static size_t wy_ld(int S) { return (size_t)(S > 0 ? S : 1) * kNB + 32; }

static int morph_reserve(fd_morph *m, int64_t N, int S)
{
    int rc;
    const size_t rows = 3 * (size_t)N;
    const size_t nwg = (rows + kWRows - 1) / kWRows;        // the finer of the two row partitions
    if (N > m->cap_N) {
        if ((rc = mrealloc(m, m->d_rest, rows)) || (rc = mrealloc(m, m->d_stage, rows)) ||
            (rc = mrealloc(m, m->d_P, rows))) return rc;
        m->d_rest_attr.reset();
        m->cap_N = N;
    }
    if (rows * (size_t)S > m->cap_entries) {
        if ((rc = mrealloc(m, m->d_QR, rows * (size_t)S)) || (rc = mrealloc(m, m->d_S32, rows * (size_t)S))) return rc;
        m->cap_entries = rows * (size_t)S;
    }
    if (S > m->cap_S) {
        if ((rc = mrealloc(m, m->d_tau, (size_t)S)) || (rc = mrealloc(m, m->d_w, (size_t)S)) ||
            (rc = mrealloc(m, m->d_tmp, (size_t)S)) || (rc = mrealloc(m, m->d_Y, (size_t)kNB * (size_t)S)) ||
            (rc = mrealloc(m, m->d_bpartial2, (size_t)kSlices * wy_ld(S)))) return rc;
        m->cap_S = S;
    }
    {   // blocked factorisation: per-workgroup sums of V^T C and V^T V, their slices, Y
        const size_t nwg_b = (rows + kBRows - 1) / kBRows, ld = wy_ld(S);
        if ((rc = mrealloc(m, m->d_bpartial, nwg_b * ld, kGrow))) return rc;
    }
    if ((rc = mrealloc(m, m->d_partial, nwg * (size_t)(S ? S : 1), kGrow))) return rc;
    return FD_OK;
}

static int morph_factor_blocked(fd_morph *m)
{
    const int64_t rows = 3 * m->N;
    const int S = m->S;
    const unsigned nwg = (unsigned)((rows + kBRows - 1) / kBRows);
    hipStream_t st = m->stream;
    double *A = m->d_QR;
    for (int k0 = 0; k0 < S; k0 += kNB) {
        const int nb = S - k0 < kNB ? S - k0 : kNB, pend = k0 + nb, ntrail = S - pend;
        if (k0 == 0) hipLaunchKernelGGL(k_qr_gram, dim3(nwg), dim3(kT), 0, st, A, rows, 0, nb, m->d_bpartial.p);
        for (int k = k0; k < pend; ++k) {
            hipLaunchKernelGGL(k_qr_col_setup, dim3(1), dim3(kSetupT), 0, st, A, rows, k, pend - k, m->d_bpartial.p, (int)nwg, m->d_hh.p,
                               m->d_tau.p, m->d_tmp.p);
            hipLaunchKernelGGL(k_qr_panel_apply, dim3(nwg), dim3(kT), 0, st, A, rows, k, pend, m->d_hh.p, m->d_tmp.p, m->d_bpartial.p);
        }
        if (ntrail > 0) {
            const int ld = ntrail * kNB + 32, nvals = ntrail * kNB + kNB * (kNB - 1) / 2;
            hipLaunchKernelGGL(k_qr_wy_dots, dim3(nwg), dim3(kT), sizeof(double) * 4 * (size_t)ld, st, A, rows, k0, nb, S,
                               m->d_bpartial.p, ld);
            hipLaunchKernelGGL(k_qr_wy_reduce, dim3((nvals + 31) / 32, kSlices), dim3(kT), 0, st, m->d_bpartial.p, (int)nwg, ld,
                               nvals, m->d_bpartial2.p);
            hipLaunchKernelGGL(k_qr_wy_T, dim3(1), dim3(kT), sizeof(double) * ((size_t)ld + kNB * kNB), st, m->d_bpartial2.p, ld, k0,
                               nb, ntrail, m->d_tau.p, m->d_Y.p);
            hipLaunchKernelGGL(k_qr_wy_apply, dim3(nwg), dim3(kT), sizeof(double) * ((size_t)kNB * ntrail + 4 * kNB), st, A, rows,
                               k0, nb, S, m->d_Y.p, ntrail < kNB ? ntrail : kNB, m->d_bpartial.p);
        }
    }
    FDM_HIP(m, hipGetLastError());
    return FD_OK;
}

static int morph_factor(fd_morph *m)
{
    // the column-by-column form: what very wide shape sets take, whose per-workgroup sums would not fit the
    // LDS of the block-reflector pass
    if (m->S <= 256) return morph_factor_blocked(m);
    const int64_t rows = 3 * m->N;
    const int S = m->S;
    const unsigned nwg = (unsigned)((rows + kRowsPerWg - 1) / kRowsPerWg);
    hipStream_t st = m->stream;
    for (int k = 0; k < S; ++k) {
        double *x = m->d_QR + (size_t)k * rows;
        hipLaunchKernelGGL(k_qr_tail_norm, dim3(nwg), dim3(kT), 0, st, x, rows, k, m->d_partial.p);
        hipLaunchKernelGGL(k_qr_reflector, dim3(1), dim3(kT), 0, st, x, k, m->d_partial.p, (int)nwg, m->d_hh.p, m->d_tau.p);
        if (k + 1 < S) {
            const int nt = S - k - 1;
            hipLaunchKernelGGL(k_qr_dots, dim3(nwg), dim3(kT), sizeof(double) * 4 * (size_t)nt, st, m->d_QR.p, rows, S, k,
                               m->d_hh.p, m->d_partial.p, nt);
            hipLaunchKernelGGL(k_qr_dots_reduce, dim3(nt), dim3(kT), 0, st, m->d_QR.p, rows, k, m->d_hh.p, m->d_partial.p,
                               (int)nwg, nt, m->d_tmp.p);
            hipLaunchKernelGGL(k_qr_apply, dim3(nwg), dim3(kT), 0, st, m->d_QR.p, rows, S, k, m->d_hh.p, m->d_tmp.p);
        } else {
            // last column: only its own tail is scaled
            hipLaunchKernelGGL(k_qr_dots, dim3(nwg), dim3(kT), sizeof(double) * 4, st, m->d_QR.p, rows, S, k, m->d_hh.p,
                               m->d_partial.p, 1);
        }
    }
    FDM_HIP(m, hipGetLastError());
    return FD_OK;
}

extern "C" {

const char *fd_morph_last_error(const fd_morph *m) { return m ? m->err : g_merr; }

fd_morph *fd_morph_create(const fd_config *cfg)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        merr(nullptr, "fd_morph_create: no HIP device visible; this engine has no CPU path");
        return nullptr;
    }
    fd_morph *m = new (std::nothrow) fd_morph();
    if (!m) { merr(nullptr, "fd_morph_create: out of host memory"); return nullptr; }
    int dev = cfg ? cfg->device : -1;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    hipDeviceProp_t prop;
    if (dev >= ndev || hipSetDevice(dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        merr(nullptr, "fd_morph_create: cannot use device %d", dev);
        delete m;
        return nullptr;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        merr(nullptr, "fd_morph_create: device %d is %s; kernels are built for gfx950 (MI355X) only", dev, prop.gcnArchName);
        delete m;
        return nullptr;
    }
    m->device = dev;
    bool ok = m->stream.create() == hipSuccess;
    ok = ok && m->ev0.create(hipEventDefault) == hipSuccess && m->ev1.create(hipEventDefault) == hipSuccess;
    ok = ok && m->d_hh.alloc(4) == hipSuccess;
    if (!ok) {
        merr(nullptr, "fd_morph_create: device resource allocation failed: %s", hipGetErrorString(hipGetLastError()));
        fd_morph_destroy(m);
        return nullptr;
    }
    return m;
}

void fd_morph_destroy(fd_morph *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    delete m;                   // the members release what they own, the stream last
}

static int morph_init_common(fd_morph *m, int64_t N, int S, const float *rest, const float *const *shapes, bool on_device)
{
    if (!m) return FD_E_INVALID;
    if (N <= 0 || S < 0 || !rest || (S > 0 && !shapes)) { merr(m, "fd_morph_init: need N > 0, S >= 0 and the arrays"); return FD_E_INVALID; }
    if ((int64_t)S > 3 * N) { merr(m, "fd_morph_init: more blendshapes (%d) than rows (%lld)", S, (long long)(3 * N)); return FD_E_INVALID; }
    // every launch's dynamic LDS within the 64 KB a kernel gets without asking for more: k_morph_weights 32 S bytes,
    // k_qr_dots 32 (S - 1), k_morph_displace 4 S; the blocked form (S <= 256) 64 512 at most
    static_assert(sizeof(double) * 4 * (size_t)FD_MORPH_MAX_SHAPES <= 65536, "k_morph_weights keeps [4][S] doubles in LDS");
    if (S > FD_MORPH_MAX_SHAPES) {
        merr(m, "fd_morph_init: %d blendshapes, at most %d (FD_MORPH_MAX_SHAPES) are supported", S, FD_MORPH_MAX_SHAPES);
        return FD_E_INVALID;
    }
    for (int s = 0; s < S; ++s)
        if (!shapes[s]) { merr(m, "fd_morph_init: shape %d is NULL", s); return FD_E_INVALID; }
    FDM_HIP(m, hipSetDevice(m->device));
    int rc = morph_reserve(m, N, S);
    if (rc) return rc;
    m->N = N; m->S = S;
    m->initialised = false; m->computed = false;
    m->batch_F = 0;
    m->use_rest_attr = false;
    const size_t rows = 3 * (size_t)N, bytes = rows * sizeof(float);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipStream_t st = m->stream;
    FDM_HIP(m, hipMemcpyAsync(m->d_rest, rest, bytes, kind, st));
    FDM_HIP(m, hipEventRecord(m->ev0, st));
    const unsigned g = (unsigned)((rows + kT - 1) / kT);
    for (int s = 0; s < S; ++s) {
        const float *src = shapes[s];
        if (!on_device) {
            FDM_HIP(m, hipMemcpyAsync(m->d_stage, shapes[s], bytes, hipMemcpyHostToDevice, st));
            src = m->d_stage;
        }
        hipLaunchKernelGGL(k_shape_column, dim3(g), dim3(kT), 0, st, m->d_rest.p, src, (int64_t)rows,
                           m->d_QR.p + (size_t)s * rows, m->d_S32.p + (size_t)s * rows);
    }
    if ((rc = morph_factor(m))) return rc;
    FDM_HIP(m, hipEventRecord(m->ev1, st));
    FDM_HIP(m, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&m->last_init_ms, m->ev0, m->ev1);
    m->initialised = true;
    return FD_OK;
}

int fd_morph_init(fd_morph *m, int64_t N, int S, const float *rest_xyz, const float *const *shapes_xyz)
{
    return morph_init_common(m, N, S, rest_xyz, shapes_xyz, false);
}

int fd_morph_init_dev(fd_morph *m, int64_t N, int S, const float *d_rest_xyz, const float *const *d_shapes_xyz)
{
    return morph_init_common(m, N, S, d_rest_xyz, d_shapes_xyz, true);
}

int fd_morph_set_rest(fd_morph *m, const float *rest_xyz, int on_device)
{
    if (!m) return FD_E_INVALID;
    if (!m->initialised) { merr(m, "fd_morph_set_rest: fd_morph_init has not succeeded"); return FD_E_NOT_BUILT; }
    if (!rest_xyz) { m->use_rest_attr = false; return FD_OK; }
    FDM_HIP(m, hipSetDevice(m->device));
    const size_t rows = 3 * (size_t)m->N;
    if (!m->d_rest_attr) {
        int rc = mrealloc(m, m->d_rest_attr, 3 * (size_t)m->cap_N);
        if (rc) return rc;
    }
    FDM_HIP(m, hipMemcpyAsync(m->d_rest_attr, rest_xyz, rows * sizeof(float),
                              on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, m->stream));
    if (!on_device) FDM_HIP(m, hipStreamSynchronize(m->stream));
    m->use_rest_attr = true;
    return FD_OK;
}

int fd_morph_is_initialised(const fd_morph *m) { return m && m->initialised && m->N > 0; }   // dbse.hpp:16 isInitialized
int fd_morph_is_computed(const fd_morph *m) { return m && m->computed; }                      // dbse.hpp:18 isComputed
int fd_morph_shape_count(const fd_morph *m) { return m ? m->S : 0; }
float fd_morph_last_init_ms(const fd_morph *m) { return m ? m->last_init_ms : 0.f; }

int fd_morph_compute_weights_dev(fd_morph *m, const float *d_P_xyz, void *hip_stream)
{
    if (!m || !d_P_xyz) return FD_E_INVALID;
    if (!m->initialised) { merr(m, "fd_morph_compute_weights: fd_morph_init has not succeeded"); return FD_E_NOT_BUILT; }
    FDM_HIP(m, hipSetDevice(m->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : m->stream;
    const int64_t rows = 3 * m->N;
    const unsigned nwg = (unsigned)((rows + kWRows - 1) / kWRows);
    if (m->S > 0) {
        hipLaunchKernelGGL(k_morph_weights, dim3(nwg), dim3(kT), sizeof(double) * 4 * (size_t)m->S, st, m->d_QR.p, rows, m->S,
                           d_P_xyz, m->use_rest_attr ? m->d_rest_attr.p : m->d_rest.p, m->d_partial.p);
        hipLaunchKernelGGL(k_morph_weights_reduce, dim3(m->S), dim3(kT), 0, st, m->d_partial.p, (int)nwg, m->S, m->d_w.p);
    }
    FDM_HIP(m, hipGetLastError());
    m->computed = true;
    return FD_OK;
}

int fd_morph_displace_dev(fd_morph *m, float *d_P_xyz, const float *clamp_lo_hi, int add_delta, float falloffradius,
                          void *hip_stream)
{
    if (!m || !d_P_xyz) return FD_E_INVALID;
    if (!m->initialised || !m->computed) { merr(m, "fd_morph_displace: weights have not been computed"); return FD_E_NOT_BUILT; }
    FDM_HIP(m, hipSetDevice(m->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : m->stream;
    const unsigned g = (unsigned)((m->N + kT - 1) / kT);
    hipLaunchKernelGGL(k_morph_displace, dim3(g), dim3(kT), sizeof(float) * (size_t)(m->S ? m->S : 1), st, m->d_S32.p, m->N,
                       m->S, m->d_w.p, clamp_lo_hi ? clamp_lo_hi[0] : 0.f, clamp_lo_hi ? clamp_lo_hi[1] : 0.f,
                       clamp_lo_hi ? 1 : 0, add_delta ? 1 : 0, falloffradius, m->use_rest_attr ? m->d_rest_attr.p : m->d_rest.p,
                       d_P_xyz);
    FDM_HIP(m, hipGetLastError());
    return FD_OK;
}

int fd_morph_get_weights(fd_morph *m, double *w)
{
    if (!m || !w) return FD_E_INVALID;
    if (!m->computed) { merr(m, "fd_morph_get_weights: weights have not been computed"); return FD_E_NOT_BUILT; }
    FDM_HIP(m, hipSetDevice(m->device));
    FDM_HIP(m, hipMemcpyAsync(w, m->d_w, sizeof(double) * (size_t)m->S, hipMemcpyDeviceToHost, m->stream));
    FDM_HIP(m, hipStreamSynchronize(m->stream));
    return FD_OK;
}

// argument checks of the batched calls: before any device work
static int morph_batch_args(fd_morph *m, const char *fn, int F, const float *const *tab, bool distinct)
{
    if (!m) { merr(nullptr, "%s: NULL fd_morph", fn); return FD_E_INVALID; }
    if (F < 1 || F > FD_MAX_BATCH) { merr(m, "%s: F = %d, need 1..%d frames", fn, F, FD_MAX_BATCH); return FD_E_INVALID; }
    if (!tab) { merr(m, "%s: the table of frame pointers is NULL", fn); return FD_E_INVALID; }
    for (int f = 0; f < F; ++f) {
        if (!tab[f]) { merr(m, "%s: frame %d is NULL", fn, f); return FD_E_INVALID; }
        for (int g = 0; distinct && g < f; ++g)
            if (tab[g] == tab[f]) { merr(m, "%s: frames %d and %d are the same array", fn, g, f); return FD_E_INVALID; }
    }
    return FD_OK;
}

// computeWeights (dbse.cpp:39-60) for the F frames of a group: one pass over the packed QR
int fd_morph_compute_weights_batch_dev(fd_morph *m, int F, const float *const *d_P_xyz, void *hip_stream)
{
    int rc = morph_batch_args(m, "fd_morph_compute_weights_batch_dev", F, d_P_xyz, false);
    if (rc) return rc;
    if (!m->initialised) { merr(m, "fd_morph_compute_weights_batch_dev: fd_morph_init has not succeeded"); return FD_E_NOT_BUILT; }
    FDM_HIP(m, hipSetDevice(m->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : m->stream;
    const int64_t rows = 3 * m->N, nchunks = (rows + kBK - 1) / kBK;
    const int S = m->S, ngroups = (S + kBCols - 1) / kBCols, ldp = ngroups * kBCols;
    const int cpw = (int)((nchunks + kBMaxWg - 1) / kBMaxWg), nwg = (int)((nchunks + cpw - 1) / cpw);
    const size_t need_w = (size_t)FD_MAX_BATCH * (size_t)(S ? S : 1), need_p = (size_t)nwg * FD_MAX_BATCH * (size_t)(ldp ? ldp : 1);
    if ((rc = mrealloc(m, m->d_bw, need_w, kGrow)) || (rc = mrealloc(m, m->d_bwpartial, need_p, kGrow))) return rc;
    if (S > 0) {
        MorphFrames fr = {};
        for (int f = 0; f < F; ++f) fr.p[f] = d_P_xyz[f];
        hipLaunchKernelGGL(k_morph_weights_batch, dim3(nwg, ngroups), dim3(kT), 0, st, m->d_QR.p, rows, S, F, fr,
                           m->use_rest_attr ? m->d_rest_attr.p : m->d_rest.p, cpw, m->d_bwpartial.p, ldp);
        hipLaunchKernelGGL(k_morph_weights_batch_reduce, dim3(ngroups, F), dim3(kT), 0, st, m->d_bwpartial.p, nwg, S, F, ldp, m->d_bw.p);
    }
    FDM_HIP(m, hipGetLastError());
    m->batch_F = F;
    return FD_OK;
}

static int morph_batch_state(fd_morph *m, const char *fn, int F)
{
    if (!m->initialised || m->batch_F == 0) { merr(m, "%s: no batched weights have been computed", fn); return FD_E_NOT_BUILT; }
    if (F != m->batch_F) { merr(m, "%s: F = %d, the batched weights hold %d frames", fn, F, m->batch_F); return FD_E_INVALID; }
    return FD_OK;
}

// displaceVector + the loop at SOP_FaceDeform.cpp:458-473 for the F frames of a group: one pass over the deltas
int fd_morph_displace_batch_dev(fd_morph *m, int F, float *const *d_P_xyz, const float *clamp_lo_hi, int add_delta,
                                float falloffradius, void *hip_stream)
{
    int rc = morph_batch_args(m, "fd_morph_displace_batch_dev", F, d_P_xyz, true);
    if (rc || (rc = morph_batch_state(m, "fd_morph_displace_batch_dev", F))) return rc;
    FDM_HIP(m, hipSetDevice(m->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : m->stream;
    MorphFramesRW fr = {};
    for (int f = 0; f < F; ++f) fr.p[f] = d_P_xyz[f];
    const unsigned g = (unsigned)((m->N + kT - 1) / kT);
    const float lo = clamp_lo_hi ? clamp_lo_hi[0] : 0.f, hi = clamp_lo_hi ? clamp_lo_hi[1] : 0.f;
    const float *rest = m->use_rest_attr ? m->d_rest_attr.p : m->d_rest.p;
#define FD_MORPH_DISPLACE_BATCH(FT)                                                                                      \
    hipLaunchKernelGGL(k_morph_displace_batch<FT>, dim3(g), dim3(kT), 0, st, m->d_S32.p, m->N, m->S, F, m->d_bw.p, lo, hi, \
                       clamp_lo_hi ? 1 : 0, add_delta ? 1 : 0, falloffradius, rest, fr)
    if (F <= 8) FD_MORPH_DISPLACE_BATCH(8);
    else if (F <= 16) FD_MORPH_DISPLACE_BATCH(16);
    else FD_MORPH_DISPLACE_BATCH(32);
#undef FD_MORPH_DISPLACE_BATCH
    FDM_HIP(m, hipGetLastError());
    return FD_OK;
}

int fd_morph_get_weights_batch(fd_morph *m, int F, double *w)
{
    if (!m) { merr(nullptr, "fd_morph_get_weights_batch: NULL fd_morph"); return FD_E_INVALID; }
    if (F < 1 || F > FD_MAX_BATCH || !w) { merr(m, "fd_morph_get_weights_batch: need F in 1..%d and an array", FD_MAX_BATCH); return FD_E_INVALID; }
    int rc = morph_batch_state(m, "fd_morph_get_weights_batch", F);
    if (rc) return rc;
    FDM_HIP(m, hipSetDevice(m->device));
    if (m->S > 0) FDM_HIP(m, hipMemcpyAsync(w, m->d_bw, sizeof(double) * (size_t)F * (size_t)m->S, hipMemcpyDeviceToHost, m->stream));
    FDM_HIP(m, hipStreamSynchronize(m->stream));
    return FD_OK;
}

int fd_morph_get_qr(fd_morph *m, double *qr, double *tau)
{
    if (!m || !qr) return FD_E_INVALID;
    if (!m->initialised) { merr(m, "fd_morph_get_qr: fd_morph_init has not succeeded"); return FD_E_NOT_BUILT; }
    FDM_HIP(m, hipSetDevice(m->device));
    FDM_HIP(m, hipMemcpyAsync(qr, m->d_QR, sizeof(double) * 3 * (size_t)m->N * (size_t)m->S, hipMemcpyDeviceToHost, m->stream));
    if (tau) FDM_HIP(m, hipMemcpyAsync(tau, m->d_tau, sizeof(double) * (size_t)m->S, hipMemcpyDeviceToHost, m->stream));
    FDM_HIP(m, hipStreamSynchronize(m->stream));
    return FD_OK;
}

int fd_morph_apply(fd_morph *m, float *P_xyz, const float *clamp_lo_hi, int add_delta, float falloffradius, double *w_out)
{
    if (!m || !P_xyz) return FD_E_INVALID;
    if (!m->initialised) { merr(m, "fd_morph_apply: fd_morph_init has not succeeded"); return FD_E_NOT_BUILT; }
    FDM_HIP(m, hipSetDevice(m->device));
    const size_t bytes = sizeof(float) * 3 * (size_t)m->N;
    FDM_HIP(m, hipMemcpyAsync(m->d_P, P_xyz, bytes, hipMemcpyHostToDevice, m->stream));
    int rc = fd_morph_compute_weights_dev(m, m->d_P, m->stream);
    if (!rc) rc = fd_morph_displace_dev(m, m->d_P, clamp_lo_hi, add_delta, falloffradius, m->stream);
    if (rc) return rc;
    FDM_HIP(m, hipMemcpyAsync(P_xyz, m->d_P, bytes, hipMemcpyDeviceToHost, m->stream));
    if (w_out && m->S > 0) FDM_HIP(m, hipMemcpyAsync(w_out, m->d_w, sizeof(double) * (size_t)m->S, hipMemcpyDeviceToHost, m->stream));
    FDM_HIP(m, hipStreamSynchronize(m->stream));
    return FD_OK;
}

}  // extern "C"
