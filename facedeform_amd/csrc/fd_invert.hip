// fd_invert.hip -- the inverse of the deformation (fd_invert*): per vertex, Newton on F(x) = x + f Pi d(x) - y in one launch.
//
// x0 = y; while |F(x)|_2 > tol: x <- x - A(x)^-1 F(x), A = I + f Pi J(x) as fd_vectors defines it (include/facedeform_hip.h
// states the contract).  No line search, no damping; the 3x3 solve is cofactors and one division by det A.
//
// Mapping to the hardware: k_vectors64_<kind>'s (fd_vectors.hip).  256-thread workgroups, two vertices per lane; the 64 B
// records are wave-uniform and come through the scalar unit; x - c is formed directly in raw coordinates; everything is fp64.
// Per Newton step one pass over the Mpad records accumulates the field (3 sums) and its Jacobian (9 sums) per vertex, phi and
// g of a record from ONE transcendental.  The step loop's exit is wave-uniform; a lane that has converged, is gated or lies past
// N keeps its x under a mask (its arithmetic runs on and is dropped) and no lane returns early.  max_iter bounds the loop.
// No LDS, no atomics.  Built with -ffp-contract=off like fd_vectors.hip: every fused multiply-add is written out.
#include "fd_operator.h"

namespace fd {

namespace {

constexpr int kBlock = 256;
constexpr int kV = 2;        // vertices per lane

using packing::grad_scale64;
using packing::phi_grad64;       // phi and g of grad phi = grad_scale64 g (x - c) from the kind's one transcendental (fd_pack.h)

typedef const __attribute__((address_space(4))) Rec64 *ConstRec64;

struct InvParams : op::Mesh {            // P: the deformed points y
    int Mpad, max_iter;                  // the inputs first, in the order that adds no SGPR spill
    double tol;                          // > 0: every vertex's; otherwise 2^-25 max(|y|_inf, s) per vertex
    const Rec64 *rec64;
    const DevModel *model;
    float *X;                            // may alias P
    float *residual;                     // N or null
    int *iters;                          // N or null
};

__device__ __forceinline__ bool finite3(const double v[3]) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

template <int KIND>
__device__ __forceinline__ void invert64_body(const InvParams &p)
{
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * kV);
    const bool built = p.model->terminationtype == 1;
    const bool proj = p.tu != nullptr;
    const double scale = 1.0 / (double)p.model->norm32[3];      // the model's normalisation scale, a power of two

    float yf[kV][3];
    double x[kV][3], best[kV][3], bestres[kV], res[kV], tol[kV], f[kV];
    double a1[kV][3], a2[kV][3];
    int status[kV];              // steps taken once converged, -1, -2
    bool active[kV], solve[kV];  // still iterating; takes part in the solve at all (in range, not gated, model built)
#pragma unroll
    for (int v = 0; v < kV; ++v) {
        const int64_t i = base + v * kBlock + tid;
        const int64_t ic = i < p.N ? i : p.N - 1;
        solve[v] = op::vertex(p, i, ic, p.N, built, x[v], f[v]);
        active[v] = solve[v];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            yf[v][c] = p.P[3 * ic + c];       // x0 = y; the fp32 value is what a vertex outside the solve is given back
            best[v][c] = x[v][c];
            a1[v][c] = 0.0; a2[v][c] = 0.0;
        }
        if (proj) transport::axes<double>(p.tu, p.tv, p.nrm, ic, a1[v], a2[v]);
        const double ymax = fmax(fabs(x[v][0]), fmax(fabs(x[v][1]), fabs(x[v][2])));
        tol[v] = p.tol > 0.0 ? p.tol : 2.98023223876953125e-08 * fmax(ymax, scale);      // 2^-25
        bestres[v] = INFINITY;
        res[v] = 0.0;
        status[v] = 0;
    }

    const double gs = grad_scale64(KIND);
    const double *af = p.model->affine64;   // {const, x, y, z} per output
    // Step k evaluates F and A at the k-th iterate: max_iter steps are max_iter + 1 evaluations.  Once no lane of the wave
    // iterates any more, a wave with a lane left at -1 or -2 makes ONE more pass (`report`, wave-uniform): such a lane's best
    // iterate is rounded to fp32 first and the residual is taken at that value, the one that is written, so that residual_out
    // describes what the caller holds.  The bound k <= max_iter + 1 holds whatever the data.
    bool report = false;
    for (int k = 0; k <= p.max_iter + 1; ++k) {
        if (!report && !__any(active[0] || active[1])) {
            const bool failed0 = solve[0] && status[0] < 0, failed1 = solve[1] && status[1] < 0;
            if (!__any(failed0 || failed1)) break;
            report = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[0][c] = failed0 ? (double)(float)best[0][c] : x[0][c];
                x[1][c] = failed1 ? (double)(float)best[1][c] : x[1][c];
            }
        }
        double D[kV][3], S[kV][9];
#pragma unroll
        for (int v = 0; v < kV; ++v) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                D[v][c] = fma(af[4 * c + 3], x[v][2], fma(af[4 * c + 2], x[v][1], fma(af[4 * c + 1], x[v][0], af[4 * c])));
#pragma unroll
            for (int q = 0; q < 9; ++q) S[v][q] = 0.0;
        }
#pragma unroll 2
        for (int j = 0; j < p.Mpad; ++j) {
            ConstRec64 r = (ConstRec64)(uintptr_t)(p.rec64 + j);
            const double cx = r->cx, cy = r->cy, cz = r->cz, s = r->s;
            const double wx = r->wx, wy = r->wy, wz = r->wz;
#pragma unroll
            for (int v = 0; v < kV; ++v) {
                const double dx = x[v][0] - cx, dy = x[v][1] - cy, dz = x[v][2] - cz;
                const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                double t, g;
                phi_grad64<KIND>(d2, s, t, g);
                D[v][0] = fma(t, wx, D[v][0]); D[v][1] = fma(t, wy, D[v][1]); D[v][2] = fma(t, wz, D[v][2]);
                const double gx = g * wx, gy = g * wy, gz = g * wz;
                S[v][0] = fma(gx, dx, S[v][0]); S[v][1] = fma(gx, dy, S[v][1]); S[v][2] = fma(gx, dz, S[v][2]);
                S[v][3] = fma(gy, dx, S[v][3]); S[v][4] = fma(gy, dy, S[v][4]); S[v][5] = fma(gy, dz, S[v][5]);
                S[v][6] = fma(gz, dx, S[v][6]); S[v][7] = fma(gz, dy, S[v][7]); S[v][8] = fma(gz, dz, S[v][8]);
            }
        }
#pragma unroll
        for (int v = 0; v < kV; ++v) {
            // F = (x - y) + f Pi d, A = I + f Pi R (fd_transport.h's A; f = 0: A = I, and F(y) = 0 exactly)
            double R[9], d[3] = {D[v][0], D[v][1], D[v][2]};
#pragma unroll
            for (int q = 0; q < 9; ++q) R[q] = fma(gs, S[v][q], af[4 * (q / 3) + 1 + q % 3]);
            if (proj) {
                op::project(a1[v], a2[v], d);
                transport::project(R, a1[v], a2[v]);
            }
            double F[3], A[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) F[c] = f[v] != 0.0 ? fma(f[v], d[c], x[v][c] - (double)yf[v][c]) : x[v][c] - (double)yf[v][c];
#pragma unroll
            for (int q = 0; q < 9; ++q) A[q] = ((q % 4 == 0) ? 1.0 : 0.0) + (f[v] != 0.0 ? f[v] * R[q] : 0.0);
            const double rn = sqrt(fma(F[2], F[2], fma(F[1], F[1], F[0] * F[0])));
            // cofactors of A (adj = cof^T) and one division
            const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
            const double c10 = A[2] * A[7] - A[1] * A[8], c11 = A[0] * A[8] - A[2] * A[6], c12 = A[1] * A[6] - A[0] * A[7];
            const double c20 = A[1] * A[5] - A[2] * A[4], c21 = A[2] * A[3] - A[0] * A[5], c22 = A[0] * A[4] - A[1] * A[3];
            const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
            const double inv = 1.0 / det;
            const double xn[3] = {x[v][0] - inv * (c00 * F[0] + c10 * F[1] + c20 * F[2]),
                                  x[v][1] - inv * (c01 * F[0] + c11 * F[1] + c21 * F[2]),
                                  x[v][2] - inv * (c02 * F[0] + c12 * F[1] + c22 * F[2])};

            const bool act = active[v];
            const bool fin = isfinite(rn);
            const bool better = act && fin && rn < bestres[v];
            const bool conv = act && fin && rn <= tol[v];
            const bool spent = act && fin && !conv && k == p.max_iter;      // no step is left to take: det A is not asked
            const bool broke = act && !conv && !spent && (!fin || det == 0.0 || !finite3(xn));
            const bool step = act && !conv && !broke && !spent;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                best[v][c] = better ? x[v][c] : best[v][c];
                x[v][c] = step ? xn[c] : x[v][c];
            }
            bestres[v] = better ? rn : bestres[v];
            res[v] = (conv || (report && solve[v] && status[v] < 0)) ? rn : res[v];
            status[v] = conv ? k : (broke ? -2 : (spent ? -1 : status[v]));
            active[v] = step;
        }
        if (report) break;
    }

#pragma unroll
    for (int v = 0; v < kV; ++v) {
        const int64_t i = base + v * kBlock + tid;
        if (i < p.N) {
            // (a lane left at -1 or -2 holds its best iterate, rounded, in x since the report pass, and that value's residual)
            float o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = !solve[v] ? yf[v][c] : (float)x[v][c];
            p.X[3 * i] = o[0]; p.X[3 * i + 1] = o[1]; p.X[3 * i + 2] = o[2];
            if (p.residual) p.residual[i] = !solve[v] ? 0.f : (float)res[v];
            if (p.iters) p.iters[i] = solve[v] ? status[v] : 0;
        }
    }
}

// k_invert64_<kind> and k_invert64_launch
FD_OP_KERNELS(k_invert64_, , (kBlock), InvParams, invert64_body<KIND>(p))

}  // namespace

hipError_t launch_invert(const DeformArgs &a, const InvertArgs &v, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    InvParams p = op::params_of<InvParams>(a);
    p.X = a.P_out;
    p.residual = v.residual_out; p.iters = v.iters_out;
    p.Mpad = a.Mpad;
    p.max_iter = v.max_iter <= 0 ? kInvertDefaultIter : (v.max_iter > kInvertMaxIter ? kInvertMaxIter : v.max_iter);
    p.tol = v.tol > 0.0 ? v.tol : 0.0;
    p.rec64 = a.rec64; p.model = a.model;
    const int64_t per = (int64_t)kBlock * kV;
    const dim3 grid((unsigned)((a.N + per - 1) / per));
    return k_invert64_launch(a.kind, grid, stream, p);
}

}  // namespace fd
