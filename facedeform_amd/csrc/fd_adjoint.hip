// fd_adjoint.hip -- the adjoint of the deformation (fd_deform_adjoint*): grad_W = sum over the vertices of phi_j(x_v) r_v,
// r_v = f_v Pi_v g_v, for a cotangent g at the deformed vertices (include/facedeform_hip.h states the contract).
//
// The pair work of an evaluation with the reduction turned round: over the vertices, not the centres.  Mapping to the hardware:
// a CENTRE per lane.  A 256-thread workgroup takes tiles of 256 vertices; each thread forms x_v and r_v of one vertex once -- the
// gate, fall-off and axes of the forward path (fd_operator.h), r = 0 by a select where the vertex is out -- and writes them
// to LDS as fp64 (48 B per vertex, 12 KB per tile).  After the barrier every lane walks the tile: all lanes of a wave read the
// same LDS address (a broadcast), x - c in raw coordinates against the lane's own Rec64 centre, phi of the kind (fd_pack.h
// phi_grad64, the inverse's), three fma into the lane's three sums; the next vertex's values are requested from LDS before the
// current vertex's arithmetic.  No cross-lane reduction per pair.  A lane owns the centres
// j, j + 256, .. (kSlots of them, one walk each; a wave whose slot lies past C skips it, wave-uniformly); grid.y takes the
// centres beyond 256 kSlots.  The four polynomial rows are four more lanes' sums with 1, x, y, z in phi's place (wave 0 of
// grid.y == 0).  Every workgroup writes its (C + 4) x 3 partial block to the context's scratch; k_adjoint64_reduce adds the
// blocks in a fixed order, applies the factor the records' weights carry (fd_pack.h: 0.5 thin-plate, -1 biharmonic), undoes the
// multilayer records' centre-major order and writes exactly 0.0 for the rows the term lacks.  No atomics: the workgroups and
// their tile ranges are a function of N alone, so the same inputs give the same bits.  Everything is fp64; built with
// -ffp-contract=off like fd_invert.hip: every fused multiply-add is written out.
#include "fd_operator.h"

namespace fd {

namespace {

constexpr int kBlock = 256;
constexpr int kSlots = 2;                    // centres per lane
constexpr int kSpan = kBlock * kSlots;       // centres per grid.y
constexpr int kMaxGroups = 1024;             // workgroups along the vertices at most (four per CU)

using packing::phi_grad64;

struct AdjParams : op::Mesh {
    const float *G;
    int C;                               // records (fd_model_centres)
    int tiles_per;                       // 256-vertex tiles per workgroup
    const Rec64 *rec64;
    const DevModel *model;
    double *partial;                     // gridDim.x blocks of (C + 4) x 3
};

template <int KIND>
__device__ __forceinline__ void adjoint64_body(const AdjParams &p)
{
    __shared__ __attribute__((aligned(16))) double s_v[kBlock + 1][6];  // {x, r} of the tile's vertices; one row more for the walk's look-ahead
    const int tid = threadIdx.x;
    const int wave_lo = tid & ~63;
    const int cbase = (int)blockIdx.y * kSpan;
    const bool built = p.model->terminationtype == 1;
    const bool proj = p.tu != nullptr;
    const bool poly = blockIdx.y == 0 && tid < 4;                      // this lane sums polynomial row tid
    const int64_t ntiles = (p.N + kBlock - 1) / kBlock;
    const int64_t t0 = (int64_t)blockIdx.x * p.tiles_per;
    const int64_t t1 = t0 + p.tiles_per < ntiles ? t0 + p.tiles_per : ntiles;

    double cx[kSlots], cy[kSlots], cz[kSlots], cs[kSlots], acc[kSlots][3];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const int j = cbase + k * kBlock + tid;
        const Rec64 &r = p.rec64[j < p.C ? j : p.C - 1];               // (a lane past C sums into a row nobody writes)
        cx[k] = r.cx; cy[k] = r.cy; cz[k] = r.cz; cs[k] = r.s;
        acc[k][0] = 0.0; acc[k][1] = 0.0; acc[k][2] = 0.0;
    }
    double pacc[3] = {0.0, 0.0, 0.0};

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t i = t * kBlock + tid;
        const int64_t ic = i < p.N ? i : p.N - 1;
        double x[3], f;
        double r[3] = {(double)p.G[3 * ic], (double)p.G[3 * ic + 1], (double)p.G[3 * ic + 2]};
        // what the forward map moves, and f != 0 (f = 0: the displacement is 0 whatever d is)
        const bool live = op::vertex(p, i, ic, p.N, built, x, f) && f != 0.0;
        if (proj) {
            double a1[3], a2[3];
            transport::axes<double>(p.tu, p.tv, p.nrm, ic, a1, a2);
            op::project(a1, a2, r);
        }
        // a select, not a product: a vertex that is out contributes exactly nothing whatever G (or P) holds there
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            r[c] = live ? f * r[c] : 0.0;
            x[c] = live ? x[c] : 0.0;
        }
        __syncthreads();                                               // the walks over the previous tile are done
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_v[tid][c] = x[c]; s_v[tid][3 + c] = r[c]; }
        __syncthreads();
        const int64_t left = p.N - t * kBlock;
        const int nv = left < kBlock ? (int)left : kBlock;            // the last tile's vertices
#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
            if (cbase + k * kBlock + wave_lo >= p.C) continue;         // wave-uniform
            // the next vertex's six values are on their way from LDS under the current vertex's arithmetic (row kBlock is only loaded)
            double nx[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) nx[q] = s_v[0][q];
#pragma unroll 1
            for (int v = 0; v < nv; ++v) {
                double cur[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) { cur[q] = nx[q]; nx[q] = s_v[v + 1][q]; }
                const double dx = cur[0] - cx[k], dy = cur[1] - cy[k], dz = cur[2] - cz[k];
                const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                double ph, g;
                phi_grad64<KIND>(d2, cs[k], ph, g);
                (void)g;
                acc[k][0] = fma(ph, cur[3], acc[k][0]);
                acc[k][1] = fma(ph, cur[4], acc[k][1]);
                acc[k][2] = fma(ph, cur[5], acc[k][2]);
            }
        }
        if (blockIdx.y == 0 && wave_lo == 0) {
            for (int v = 0; v < nv; ++v) {
                const double ph = tid == 0 ? 1.0 : (tid == 1 ? s_v[v][0] : (tid == 2 ? s_v[v][1] : s_v[v][2]));
                pacc[0] = fma(ph, s_v[v][3], pacc[0]);
                pacc[1] = fma(ph, s_v[v][4], pacc[1]);
                pacc[2] = fma(ph, s_v[v][5], pacc[2]);
            }
        }
    }

    double *out = p.partial + (size_t)blockIdx.x * (size_t)(p.C + 4) * 3;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const int j = cbase + k * kBlock + tid;
        if (j < p.C) { out[3 * j] = acc[k][0]; out[3 * j + 1] = acc[k][1]; out[3 * j + 2] = acc[k][2]; }
    }
    if (poly) {
        const int j = p.C + tid;
        out[3 * j] = pacc[0]; out[3 * j + 1] = pacc[1]; out[3 * j + 2] = pacc[2];
    }
}

// k_adjoint64_<kind> and k_adjoint64_launch
FD_OP_KERNELS(k_adjoint64_, , (kBlock), AdjParams, adjoint64_body<KIND>(p))

// The blocks' sums in a fixed order, the same for every call with this N.  A workgroup takes kEnt entries of the (C + 4) x 3
// result; kParts threads per entry each add a contiguous range of the blocks in the blocks' order (the loads of eight blocks in
// flight at a time: one thread per entry over all the blocks would be a chain of a thousand dependent round trips to memory),
// then the parts are added in their order and stored by fd_operator.h's row rule.
constexpr int kParts = 16, kEnt = kBlock / kParts;
__global__ __launch_bounds__(kBlock) void k_adjoint64_reduce(const double *partial, int nblocks, int C, int layers, int T,
                                                             double wscale, double *grad_W)
{
    __shared__ double s_p[kParts][kEnt];
    const int le = (int)threadIdx.x % kEnt, part = (int)threadIdx.x / kEnt;
    const int e = (int)blockIdx.x * kEnt + le;
    const int n = (C + 4) * 3;
    const int per = (nblocks + kParts - 1) / kParts;
    const int b0 = part * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    double sum = 0.0;
    if (e < n) {
#pragma unroll 8
        for (int b = b0; b < b1; ++b) sum += partial[(size_t)b * n + e];
    }
    s_p[part][le] = sum;
    __syncthreads();
    if (part != 0 || e >= n) return;
    sum = s_p[0][le];
#pragma unroll
    for (int q = 1; q < kParts; ++q) sum += s_p[q][le];
    const int row = e / 3, a = e % 3;
    op::store_row(grad_W, row, a, C, layers, T, wscale, sum);
}

}  // namespace

int adjoint_groups(int64_t N)
{
    if (N <= 0) return 0;
    const int64_t ntiles = (N + kBlock - 1) / kBlock;
    const int64_t per = (ntiles + kMaxGroups - 1) / kMaxGroups;
    return (int)((ntiles + per - 1) / per);
}

hipError_t launch_adjoint(const DeformArgs &a, const AdjointArgs &g, hipStream_t stream)
{
    const int groups = adjoint_groups(a.N);
    if (groups > 0) {
        AdjParams p = op::params_of<AdjParams>(a);
        p.G = g.G;
        p.C = a.M;
        const int64_t ntiles = (a.N + kBlock - 1) / kBlock;
        p.tiles_per = (int)((ntiles + groups - 1) / groups);
        p.rec64 = a.rec64; p.model = a.model;
        p.partial = g.partial;
        const dim3 grid((unsigned)groups, (unsigned)((a.M + kSpan - 1) / kSpan));
        const hipError_t e = k_adjoint64_launch(a.kind, grid, stream, p);
        if (e != hipSuccess) return e;
    }
    const int n = (a.M + 4) * 3;
    hipLaunchKernelGGL(k_adjoint64_reduce, dim3((unsigned)((n + kEnt - 1) / kEnt)), dim3(kBlock), 0, stream,
                       (const double *)g.partial, groups, a.M, a.layers, g.T, packing::weight_scale64(a.kind), g.grad_W);
    return hipGetLastError();
}

}  // namespace fd
