// fd_adjoint_points_shot.hip -- the adjoint of the deformation in the vertex positions for ALL frames of a shot, one launch
// (fd_batch_deform_adjoint_points_shared_dev; include/facedeform_hip.h states the contract):
//     grad_P[v] = sum_f g_{f,v} + sum_{f built} J_f(x_v)^T r_{f,v},      r_{f,v} = f_v Pi_v g_{f,v}.
// The frames share the mesh, the gate and the rest rig, so the sum over the frames is taken INSIDE the sum over the centres:
//     sum_f J_f^T r_f = gs sum_j g_j(x) (x - c_j) s_j + sum_f L_f^T r_f,      s_j = sum_{f,b} w_{f,j,b} r_{f,b}.
// s is a (16 centres) x (16 vertices) product of depth 3 F on v_mfma_f64_16x16x4_f64, the same for every kind; the basis
// g_j(x) (x - c_j) is formed ONCE per (vertex, centre) whatever F is, where F one-frame launches form it F times.
//
// Definition: k_adjoint_points64_<kind>'s (fd_adjoint_points.hip) per frame -- the same gate, transport::falloff and
// transport::axes, the same Pi g and r, x - c in raw coordinates, phi_grad64<KIND>, q = g s, three fma -- with the sum over the
// frames moved inside.  Only the order and association of the fp64 sums differ.
//
// Two kernels and one for the fallback:
//   k_pack_adjoint_points_shot   the only reader of the contexts' models.  Writes, into scratch of the batch that nothing else
//                    uses (fd_adjoint_points_shot.h: the layout and the dealing): the frames' status, the affine tile, the rest
//                    rig's centre records and every frame's weights in A-operand order, rows = centres, depth = (frame,
//                    component).  A frame whose model is not built gets zero weights; one whose centres differ from frame
//                    0's is marked unbuilt and reported.
//   k_adjoint_points64_shot<KIND, NQ>   8 waves per workgroup, persistent; a wave owns one vertex tile of 16 per group of 128.
//                    Lane (k, j) = (lane >> 4, lane & 15) holds vertex j.  Once per vertex tile it reads G of frames k, 4 + k,
//                    ..., forms r = f Pi g for them (3 NQ doubles: the B operand of every step, exactly 0.0 by a select
//                    where the vertex is out or the frame unbuilt) and hands its widened g round the four lane groups, which
//                    all add sum_f g_f in frame order.  One pass of 3 NQ matrix instructions against the affine tile gives
//                    sum_f L_f^T r_f (direction d in lane group d).  Per tile of 16 centres: 3 NQ matrix instructions, then the
//                    lane holds s of its vertex for centres k, k + 4, k + 8, k + 12, forms their bases and adds q (x - c) into
//                    three sums.  At the end the four lane groups' sums are added in the order 0, 1, 2, 3; lane group d
//                    stores component d.  A vertex where every A_f = I gets sum_f g_f by a select.
//   LDS: the head and the affine tile stay; centre tiles (records and weights, 12.5 KB each at 32 frames) that do not all
//   fit are staged in evened chunks per group with the three sums live across them, as k_vectors64_shared stages its K steps.
//   k_adjoint_points_add   grad_P += the one-frame launch's result of the next frame: the per-context route, where the launch
//                    above does not apply.  Frame 0 writes grad_P itself, so the result is the frame-ordered sum of the F
//                    one-frame results, bit for bit, with N x 3 doubles of scratch and not F times that.
// No atomics; a vertex's bits depend on its own column of its wave's matrix instructions, on F and on the models only, not on
// N or its place in the launch.  Everything is fp64; built with -ffp-contract=off like fd_adjoint_points.hip.
#include "fd_adjoint_points_shot.h"
#include "fd_operator.h"
#include "fd_shared64.h"
#include "fd_shot_launch.h"

namespace fd {

namespace {

constexpr int kApsGroup = 16 * kShotWaves;      // vertices per workgroup and group
constexpr int kApsPackThreads = 256;
constexpr int kAddBlock = 256;
static_assert(kApsLdsBudget == kS64LdsBudget, "one LDS budget for the fp64 shot launches");

using packing::grad_scale64;
using packing::phi_grad64;

struct ApsPackArgs {
    const Rec64 *rec[kMaxBatch];
    const DevModel *model[kMaxBatch];
    const double *centres[kMaxBatch];     // fp64 M x 3 per context; entry f == entry 0: not compared
};

// threads [0, 64 kMaxBatch): one wave per frame -- status and the centre comparison; then one thread per double
__global__ __launch_bounds__(kApsPackThreads) void k_pack_adjoint_points_shot(const ApsPackArgs a, double *scratch, int nF, int M,
                                                                              int Mpad, int nq, int *mismatch)
{
    const size_t idx = (size_t)blockIdx.x * kApsPackThreads + threadIdx.x;
    const size_t nhead = (size_t)64 * kMaxBatch;
    if (idx < nhead) {
        const int f = (int)(idx >> 6), lane = (int)(idx & 63);
        int *built = reinterpret_cast<int *>(scratch);
        if (f >= nF) {
            if (lane == 0) built[f] = 0;
            return;
        }
        bool differs = false;
        if (a.centres[f] != a.centres[0])
            for (int q = lane; q < 3 * M; q += 64) differs |= a.centres[f][q] != a.centres[0][q];
        differs = __any(differs);
        if (lane == 0) {
            built[f] = (a.model[f]->terminationtype == 1 && !differs) ? 1 : 0;
            if (differs && mismatch) *mismatch = 1 + f;
        }
        return;
    }
    size_t q = idx - nhead;
    const size_t naff = (size_t)aps_steps(nq) * 64, ncen = (size_t)Mpad * 4, nw = (size_t)(Mpad / 16) * aps_steps(nq) * 64;
    if (q < naff) {
        int dir, f, b;
        aps_affine_source(q, dir, f, b);
        scratch[aps_aff_at() + q] = (dir < 3 && f < nF && a.model[f]->terminationtype == 1) ? a.model[f]->affine64[4 * b + 1 + dir] : 0.0;
        return;
    }
    q -= naff;
    if (q < ncen) {
        const Rec64 &r = a.rec[0][q >> 2];
        const int e = (int)(q & 3);
        scratch[aps_cen_at(nq) + q] = e == 0 ? r.cx : e == 1 ? r.cy : e == 2 ? r.cz : r.s;
        return;
    }
    q -= ncen;
    if (q < nw) {
        int centre, f, b;
        aps_weight_source(nq, q, centre, f, b);
        double w = 0.0;
        if (f < nF && a.model[f]->terminationtype == 1) {
            const Rec64 &r = a.rec[f][centre];
            w = b == 0 ? r.wx : b == 1 ? r.wy : r.wz;
        }
        scratch[aps_w_at(nq, Mpad) + q] = w;
    }
}

struct ApsParams : ShotEvalMesh {
    int nF, ntiles, tchunk, Mpad;
    const double *scratch;
    const float *G;                      // nF x N x 3
    double *grad_P;                      // N x 3
};

template <int KIND, int NQ>
__global__ __launch_bounds__(kShotThreads) void k_adjoint_points64_shot(const ApsParams p, int ngroups)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int S = 3 * NQ;
    // LDS: [head][affine tile S x 64][centre records tchunk x 64][weight tiles tchunk x S x 64]
    const int *s_built = reinterpret_cast<const int *>(smem);
    const double *s_aff = reinterpret_cast<const double *>(smem) + aps_aff_at();
    double *s_cen = reinterpret_cast<double *>(smem) + aps_cen_at(NQ);
    double *s_w = s_cen + 64 * p.tchunk;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;

    {
        const f64x2 *src = reinterpret_cast<const f64x2 *>(p.scratch);
        f64x2 *dst = reinterpret_cast<f64x2 *>(smem);
        for (int q = tid; q < (int)(aps_cen_at(NQ) / 2); q += kShotThreads) dst[q] = src[q];
    }
    // centre tiles t0 .. t0 + nt - 1 of the model into LDS
    auto stage = [&](int t0, int nt) {
        __syncthreads();
        const f64x2 *csrc = reinterpret_cast<const f64x2 *>(p.scratch + aps_cen_at(NQ) + (size_t)64 * t0);
        f64x2 *cdst = reinterpret_cast<f64x2 *>(s_cen);
        for (int q = tid; q < nt * 32; q += kShotThreads) cdst[q] = csrc[q];
        const f64x2 *wsrc = reinterpret_cast<const f64x2 *>(p.scratch + aps_w_at(NQ, p.Mpad) + (size_t)t0 * S * 64);
        f64x2 *wdst = reinterpret_cast<f64x2 *>(s_w);
        for (int q = tid; q < nt * S * 32; q += kShotThreads) wdst[q] = wsrc[q];
        __syncthreads();
    };
    const bool resident = p.ntiles <= p.tchunk;
    if (resident) stage(0, p.ntiles);
    else __syncthreads();
    bool any_built = false;
    for (int f = 0; f < p.nF; ++f) any_built |= s_built[f] != 0;

    const bool proj = p.tu != nullptr;
    const f64x4 zero4 = {0.0, 0.0, 0.0, 0.0};
    constexpr double gs = grad_scale64(KIND);
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t vi = ((int64_t)grp * kShotWaves + wave) * 16 + j;
        const bool inb = vi < p.N;
        const int64_t vc = inb ? vi : p.N - 1;
        const double px = (double)p.P_in[3 * vc], py = (double)p.P_in[3 * vc + 1], pz = (double)p.P_in[3 * vc + 2];
        const float d2f = p.dist2 ? p.dist2[vc] : 0.f;
        const double fv = (double)transport::falloff(p.dist2 != nullptr, p.radius2, p.falloffrate, d2f);
        // what the forward map moves in some frame: in range, not gated, f != 0, a model built
        const bool live = inb && !(d2f > p.radius2) && fv != 0.0 && any_built;
        const bool work = __any(live);
        double a1[3], a2[3];
        if (proj) transport::axes<double>(p.tu, p.tv, p.nrm, vc, a1, a2);

        // r of this lane's frames 4 q + g, and sum_f g_f in frame order in every lane group
        double r[NQ][3], sumg[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int f = 4 * q + g;
            const int fc = f < p.nF ? f : 0;
            const float *src = p.G + ((size_t)fc * (size_t)p.N + (size_t)vc) * 3;
            const double gq[3] = {(double)src[0], (double)src[1], (double)src[2]};
            double pg[3] = {gq[0], gq[1], gq[2]};
            if (proj) {
                // Pi = a1 a1^T + a2 a2^T is symmetric: Pi g, formed as the forward path forms Pi d
                const double p1 = a1[0] * gq[0] + a1[1] * gq[1] + a1[2] * gq[2];
                const double p2 = a2[0] * gq[0] + a2[1] * gq[1] + a2[2] * gq[2];
#pragma unroll
                for (int c = 0; c < 3; ++c) pg[c] = a1[c] * p1 + a2[c] * p2;
            }
            // a select, not a product: a vertex that is out, a frame the shot lacks and an unbuilt frame give exactly 0.0
            const bool keep = live && f < p.nF && s_built[fc] != 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) r[q][c] = keep ? fv * pg[c] : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (4 * q + k >= p.nF) continue;                       // uniform over the launch
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double o = __shfl(gq[c], 16 * k + j);
                    sumg[c] = (q == 0 && k == 0) ? o : sumg[c] + o;    // frame 0 starts the sum: F = 1 is g widened, bit for bit
                }
            }
        }

        // sum_f L_f^T r_f: the affine tile against R; row d of the product, direction d, is register 0 of lane group d
        f64x4 aff = zero4;
        if (work) {
#pragma unroll
            for (int s = 0; s < S; ++s) aff = __builtin_amdgcn_mfma_f64_16x16x4f64(s_aff[s * 64 + lane], r[s / 3][s % 3], aff, 0, 0, 0);
        }

        double acc[3] = {0.0, 0.0, 0.0};
        for (int t0 = 0; t0 < p.ntiles; t0 += p.tchunk) {
            const int nt = p.ntiles - t0 < p.tchunk ? p.ntiles - t0 : p.tchunk;
            if (!resident) stage(t0, nt);
            if (!work) continue;
            for (int t = 0; t < nt; ++t) {
                const double *wk = s_w + (size_t)t * S * 64 + lane;
                f64x4 sv = zero4;
#pragma unroll
                for (int s = 0; s < S; ++s) sv = __builtin_amdgcn_mfma_f64_16x16x4f64(wk[s * 64], r[s / 3][s % 3], sv, 0, 0, 0);
                // register i of the product is centre g + 4 i of the tile, for this lane's vertex
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f64x2 *cr = reinterpret_cast<const f64x2 *>(s_cen + 64 * t + 4 * (g + 4 * i));
                    const f64x2 c01 = cr[0], c23 = cr[1];
                    const double dx = px - c01[0], dy = py - c01[1], dz = pz - c23[0];
                    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                    double ph, gg;
                    phi_grad64<KIND>(d2, c23[1], ph, gg);
                    (void)ph;
                    const double qv = gg * sv[i];
                    acc[0] = fma(qv, dx, acc[0]); acc[1] = fma(qv, dy, acc[1]); acc[2] = fma(qv, dz, acc[2]);
                }
            }
        }

        // the lane groups' sums in the order 0, 1, 2, 3; then as the one-frame kernel: g + (gs acc + L^T r)
        double o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double tot = __shfl(acc[c], j);
#pragma unroll
            for (int k = 1; k < 4; ++k) tot += __shfl(acc[c], 16 * k + j);
            const double lt = __shfl(aff[0], 16 * c + j);
            const double s = sumg[c] + fma(gs, tot, lt);
            o[c] = live ? s : sumg[c];                                 // every A_f = I: sum_f g_f, a select and not a product
        }
        if (inb && g < 3) p.grad_P[3 * vi + g] = g == 0 ? o[0] : (g == 1 ? o[1] : o[2]);
    }
}

__global__ __launch_bounds__(kAddBlock) void k_adjoint_points_add(double *sum, const double *term, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kAddBlock + threadIdx.x;
    if (i < n) sum[i] = sum[i] + term[i];
}

template <int KIND>
hipError_t launch_kind(const ApsParams &p, int nq, const ShotGrid &gr, hipStream_t stream)
{
    switch (nq) {
    case 1: return launch_shot<k_adjoint_points64_shot<KIND, 1>>(gr, stream, p);
    case 2: return launch_shot<k_adjoint_points64_shot<KIND, 2>>(gr, stream, p);
    case 3: return launch_shot<k_adjoint_points64_shot<KIND, 3>>(gr, stream, p);
    case 4: return launch_shot<k_adjoint_points64_shot<KIND, 4>>(gr, stream, p);
    case 5: return launch_shot<k_adjoint_points64_shot<KIND, 5>>(gr, stream, p);
    case 6: return launch_shot<k_adjoint_points64_shot<KIND, 6>>(gr, stream, p);
    case 7: return launch_shot<k_adjoint_points64_shot<KIND, 7>>(gr, stream, p);
    case 8: return launch_shot<k_adjoint_points64_shot<KIND, 8>>(gr, stream, p);
    default: return hipErrorInvalidValue;
    }
}

// centre tiles staged at a time: all of them where they fit
int aps_tchunk(int Mpad, int nq)
{
    return even_chunks(Mpad / 16, aps_lds_tiles(nq));
}

}  // namespace

size_t shared_adjoint_points_scratch_bytes(int Mpad, int nF) { return 8 * aps_doubles(aps_quads(nF), Mpad); }

hipError_t launch_adjoint_points_shared(const SharedAdjointPointsArgs &a, hipStream_t stream)
{
    if (a.N <= 0 || a.nF <= 0) return hipSuccess;
    if (a.nF > kMaxBatch || a.Mpad <= 0 || a.Mpad % 16 != 0 || !a.scratch) return hipErrorInvalidValue;
    const int nq = aps_quads(a.nF);

    ApsPackArgs pa{};
    for (int f = 0; f < a.nF; ++f) { pa.rec[f] = a.rec64[f]; pa.model[f] = a.model[f]; pa.centres[f] = a.centres[f]; }
    const size_t nthreads = (size_t)64 * kMaxBatch + aps_doubles(nq, a.Mpad) - kApsHead;
    const unsigned pgrid = (unsigned)((nthreads + kApsPackThreads - 1) / kApsPackThreads);
    hipLaunchKernelGGL(k_pack_adjoint_points_shot, dim3(pgrid), dim3(kApsPackThreads), 0, stream, pa, (double *)a.scratch, a.nF, a.M,
                       a.Mpad, nq, a.mismatch);
    if (hipError_t e = shot_packed(a, stream); e != hipSuccess) return e;

    ApsParams p{};
    fill_eval_mesh(p, a);
    p.nF = a.nF; p.ntiles = a.Mpad / 16; p.Mpad = a.Mpad;
    p.tchunk = aps_tchunk(a.Mpad, nq);
    p.scratch = (const double *)a.scratch;
    p.G = a.G; p.grad_P = a.grad_P;
    ShotGrid gr;          // two workgroups per CU at most
    if (hipError_t e = shot_grid(a.N, kApsGroup, a.max_wgs, aps_lds_fixed(nq) + aps_lds_per_tile(nq) * (size_t)p.tchunk, 2, gr); e != hipSuccess)
        return e;
    switch (a.kind) {
    case FD_KERNEL_GAUSSIAN:
    case FD_KERNEL_GAUSSIAN_QNN: return launch_kind<FD_KERNEL_GAUSSIAN>(p, nq, gr, stream);
    case FD_KERNEL_THIN_PLATE: return launch_kind<FD_KERNEL_THIN_PLATE>(p, nq, gr, stream);
    case FD_KERNEL_BIHARMONIC: return launch_kind<FD_KERNEL_BIHARMONIC>(p, nq, gr, stream);
    case FD_KERNEL_CUBIC: return launch_kind<FD_KERNEL_CUBIC>(p, nq, gr, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_adjoint_points_add(double *sum, const double *term, int64_t n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_adjoint_points_add, dim3((unsigned)((n + kAddBlock - 1) / kAddBlock)), dim3(kAddBlock), 0, stream, sum, term, n);
    return hipGetLastError();
}

// The fewest frames at which the one launch beats F one-frame launches plus the ordered additions by more than the spread, by
// device events at 1M vertices and 256 centres (profiles/adjoint_points_shot_timing.txt): a launch of one quad
// costs the same for 1..4 frames -- 1.01 ms thin-plate, 0.51 ms QNN, 0.62 ms biharmonic, 0.48 ms cubic -- while the one-frame
// launches cost 0.82, 0.34, 0.44 and 0.30 ms per frame: 0.63x - 0.81x at one frame, 1.27x - 1.59x at two.
int shared_adjoint_points_min_frames(int kind)
{
#ifdef FD_APS_MIN_FRAMES
    // the rows of the timing table below the thresholds (tests/tools/adjoint_points_shot_timing.py): a library built with
    // FD_EXTRA_HIPCC_FLAGS=-DFD_APS_MIN_FRAMES=1 takes the launch from that many frames on, whatever the kind
    if (kind != FD_KERNEL_GAUSSIAN_ML) return FD_APS_MIN_FRAMES;
#endif
    switch (kind) {
    case FD_KERNEL_THIN_PLATE:
    case FD_KERNEL_BIHARMONIC:
    case FD_KERNEL_GAUSSIAN:
    case FD_KERNEL_GAUSSIAN_QNN:
    case FD_KERNEL_CUBIC: return 2;
    default: return 1;
    }
}

const char *shared_adjoint_points_kernel_name(int Mpad, int nF, int kind)
{
    return shared64_kernel_name(Mpad, nF, kind)[0] && nF >= shared_adjoint_points_min_frames(kind) ? "k_adjoint_points64_shot" : "";
}

}  // namespace fd
