// fd_adjoint_points.hip -- the adjoint of the deformation in the vertex positions (fd_deform_adjoint_points*): per vertex
// grad_P = A^T g = g + J(x)^T r, r = f Pi g, and on request grad_f = g . Pi d(x), for a cotangent g at the deformed vertices
// (include/facedeform_hip.h states the contract).
//
// Mapping to the hardware: k_invert64_<kind>'s single pass (fd_invert.hip), not the adjoint's -- the sum runs over the
// records, so it is a VERTEX per lane.  256-thread workgroups, two vertices per lane; the 64 B records are wave-uniform and come
// through the scalar unit over Mpad (padded records carry zero weights); x - c is formed directly in raw coordinates;
// everything is fp64.  Per vertex, once: x, f, the axes, r = f (a1 (a1 . g) + a2 (a2 . g)).  Per (vertex, record): phi and g of
// grad phi from the kind's ONE transcendental, s = w . r, q = g s, three fma into the vertex's three sums -- three accumulators
// where the inverse carries nine -- and, for grad_f, three more with phi into the field.  The epilogue adds g and L^T r; a
// vertex where A = I (gated, model not built, f = 0) gets g widened by a select.  A wave none of whose lanes needs the sums
// skips the records (wave-uniform; a lane's own result is the same either way).  No LDS, no atomics, no cross-vertex sums.
// Built with -ffp-contract=off like fd_invert.hip: every fused multiply-add is written out.
#include "fd_operator.h"

namespace fd {

namespace {

constexpr int kBlock = 256;
constexpr int kV = 2;        // vertices per lane

using packing::grad_scale64;
using packing::phi_grad64;       // phi and g of grad phi = grad_scale64 g (x - c) from the kind's one transcendental (fd_pack.h)

typedef const __attribute__((address_space(4))) Rec64 *ConstRec64;

struct AdjPointsParams {
    int64_t N;
    const float *P, *G, *dist2;
    const float *tu, *tv, *nrm;          // projection frames (all or none)
    float radius2, falloffrate;
    int Mpad;
    const Rec64 *rec64;
    const DevModel *model;
    double *grad_P;                      // N x 3
    double *grad_f;                      // N (WANT_F)
};

template <int KIND, bool WANT_F>
__device__ __forceinline__ void adjoint_points64_body(const AdjPointsParams &p)
{
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * kV);
    const bool built = p.model->terminationtype == 1;
    const bool proj = p.tu != nullptr;

    double x[kV][3], g[kV][3], r[kV][3], pg[kV][3];
    bool moved[kV], live[kV];    // the forward map moves the vertex with f (in range, not gated, model built); ... and f != 0
#pragma unroll
    for (int v = 0; v < kV; ++v) {
        const int64_t i = base + v * kBlock + tid;
        const int64_t ic = i < p.N ? i : p.N - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[v][c] = (double)p.P[3 * ic + c];
            g[v][c] = (double)p.G[3 * ic + c];
            pg[v][c] = g[v][c];
        }
        const float d2f = p.dist2 ? p.dist2[ic] : 0.f;
        const double f = (double)transport::falloff(p.dist2 != nullptr, p.radius2, p.falloffrate, d2f);
        moved[v] = (i < p.N) && !(d2f > p.radius2) && built;
        live[v] = moved[v] && f != 0.0;
        if (proj) {
            // Pi = a1 a1^T + a2 a2^T is symmetric: Pi g, formed as the forward path forms Pi d
            double a1[3], a2[3];
            transport::axes<double>(p.tu, p.tv, p.nrm, ic, a1, a2);
            const double p1 = a1[0] * g[v][0] + a1[1] * g[v][1] + a1[2] * g[v][2];
            const double p2 = a2[0] * g[v][0] + a2[1] * g[v][1] + a2[2] * g[v][2];
#pragma unroll
            for (int c = 0; c < 3; ++c) pg[v][c] = a1[c] * p1 + a2[c] * p2;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) r[v][c] = f * pg[v][c];
    }

    const double *af = p.model->affine64;   // {const, x, y, z} per output
    double acc[kV][3], D[kV][3];
#pragma unroll
    for (int v = 0; v < kV; ++v) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[v][c] = 0.0;
            D[v][c] = fma(af[4 * c + 3], x[v][2], fma(af[4 * c + 2], x[v][1], fma(af[4 * c + 1], x[v][0], af[4 * c])));
        }
    }
    // grad_f is asked of an f = 0 vertex too: the map still depends on f there
    const bool need = WANT_F ? (moved[0] || moved[1]) : (live[0] || live[1]);
    const int records = __any(need) ? p.Mpad : 0;
#pragma unroll 2
    for (int j = 0; j < records; ++j) {
        ConstRec64 rec = (ConstRec64)(uintptr_t)(p.rec64 + j);
        const double cx = rec->cx, cy = rec->cy, cz = rec->cz, s = rec->s;
        const double wx = rec->wx, wy = rec->wy, wz = rec->wz;
#pragma unroll
        for (int v = 0; v < kV; ++v) {
            const double dx = x[v][0] - cx, dy = x[v][1] - cy, dz = x[v][2] - cz;
            const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
            double t, gg;
            phi_grad64<KIND>(d2, s, t, gg);
            const double wr = fma(wz, r[v][2], fma(wy, r[v][1], wx * r[v][0]));
            const double q = gg * wr;
            acc[v][0] = fma(q, dx, acc[v][0]); acc[v][1] = fma(q, dy, acc[v][1]); acc[v][2] = fma(q, dz, acc[v][2]);
            if constexpr (WANT_F) {
                D[v][0] = fma(t, wx, D[v][0]); D[v][1] = fma(t, wy, D[v][1]); D[v][2] = fma(t, wz, D[v][2]);
            }
        }
    }

    const double gs = grad_scale64(KIND);
#pragma unroll
    for (int v = 0; v < kV; ++v) {
        const int64_t i = base + v * kBlock + tid;
        if (i < p.N) {
            // grad_P = g + grad_scale64 acc + L^T r, (L^T r)[k] = sum_c L[c][k] r[c]; A = I: g, a select and not a product
            double o[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double lt = fma(af[9 + k], r[v][2], fma(af[5 + k], r[v][1], af[1 + k] * r[v][0]));
                const double s = g[v][k] + fma(gs, acc[v][k], lt);
                o[k] = live[v] ? s : g[v][k];
            }
            p.grad_P[3 * i] = o[0]; p.grad_P[3 * i + 1] = o[1]; p.grad_P[3 * i + 2] = o[2];
            if constexpr (WANT_F) {
                const double gf = fma(pg[v][2], D[v][2], fma(pg[v][1], D[v][1], pg[v][0] * D[v][0]));
                p.grad_f[i] = moved[v] ? gf : 0.0;
            }
        }
    }
}

// k_adjoint_points64_<kind>, _f with grad_f, and their k_adjoint_points64_launch, _f
FD_OP_KERNELS(k_adjoint_points64_, , (kBlock), AdjPointsParams, adjoint_points64_body<KIND, false>(p))
FD_OP_KERNELS(k_adjoint_points64_, _f, (kBlock), AdjPointsParams, adjoint_points64_body<KIND, true>(p))

}  // namespace

hipError_t launch_adjoint_points(const DeformArgs &a, const AdjointPointsArgs &g, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    AdjPointsParams p;
    op::fill_mesh(p, a);
    p.P = a.P_in; p.G = g.G;
    p.Mpad = a.Mpad;
    p.rec64 = a.rec64; p.model = a.model;
    p.grad_P = g.grad_P; p.grad_f = g.grad_f;
    const int64_t per = (int64_t)kBlock * kV;
    const dim3 grid((unsigned)((a.N + per - 1) / per));
    return g.grad_f ? k_adjoint_points64_launch_f(a.kind, grid, stream, p) : k_adjoint_points64_launch(a.kind, grid, stream, p);
}

}  // namespace fd
