// fd_vectors_shared64.hip -- the Jacobian and the vectors it carries for ALL frames of a shot in fp64, one matrix-pipe
// launch (fd_batch_deform_vectors_shared_fp64_dev).  The frames share the mesh and the rest rig, so the
// gradient basis g_j(x) (x - c_j) is formed ONCE per (vertex, centre), in fp64 from direct differences of the raw
// coordinates, and contracted with every frame's fp64 weights on v_mfma_f64_16x16x4_f64:
//     J_f(x) = gs sum_j w_f[j] (x) g_j(x) (x - c_j) + L_f,
// three (N x M) x (M x 3F) products, one per direction of the gradient, against the weights k_pack_shared64 left in the
// batch's fp64 scratch in A-operand order (fd_shared64.h: the position launch's layout, the one copy of it).
//
// Definition: k_vectors64_<kind>'s (fd_vectors.hip), per frame -- the same grad64<KIND>, the same d2 expression, fp64
// accumulation, then fd_transport.h's transport<double>.  Only the order and association of the fp64 sum differ: four
// centres per matrix instruction, w ((gs g) d) for gs ((g w) d), and L_f goes in first (one more K = 4 step against unit
// vectors, exact) where the one-frame kernel adds it last.
//
// Inputs: the scratch only (weights, centre records, affine tiles, frame status), the mesh and the vectors -- nothing of
// the contexts, so fd_batch_wait_consumed covers this launch as it does the position launch.
//
// Mapping: k_deform64_shared's.  8 waves per workgroup, persistent; a wave owns ONE vertex tile of 16 per group (three
// directions x NT row tiles x 4 doubles are 144 registers at 32 frames: a second vertex tile does not fit beside
// 8-wave workgroups).  Lane (g, j) = (lane >> 4, lane & 15) holds vertex j and, per K step of 4 centres, forms the basis
// of centre 4 ks + g: the B-operand layout, no exchange between lanes.  The A operand is one double per lane from LDS,
// shared by the three directions.  Rows are dealt by s64_row, so lane group g holds whole frames and finishes them alone:
// projection axes once per vertex, A_f = I + f Pi J_f for all its frames in place of J_f, then the vectors per frame
// (fd_transport.h's two halves), non-temporal stores.  A model that does not fit LDS is staged in chunks of K steps with the
// accumulators live across them.
// No floating-point atomics; a vertex's bits depend on its column of its own matrix instructions only, not on its place
// in the launch.  Built with -ffp-contract=off like the rest.
#include <algorithm>

#include "fd_eval_common.h"
#include "fd_pack.h"
#include "fd_shared64.h"
#include "fd_vectors_shot.h"

namespace fd {

namespace {

struct V64Params : ShotMesh {
    int nF, nks, kchunk, Mpad;
    const double *scratch;
};

template <int KIND, int NT, bool DENSE>
__global__ __launch_bounds__(kS64Threads) void k_vectors64_shared(const ShotOut out, const V64Params p, int ngroups)
{
    (void)out;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [head][affine tiles NT x 64][output pointers 32 x 4][centre records kchunk x 4 x 4][weight tiles kchunk x NT x 64]
    const S64Head *s_head = reinterpret_cast<const S64Head *>(smem);
    const double *s_aff = reinterpret_cast<const double *>(smem) + s64_aff_at();
    float **s_ptr = reinterpret_cast<float **>(reinterpret_cast<double *>(smem) + s64_cen_at(NT));
    double *s_cen = reinterpret_cast<double *>(s_ptr + 4 * kMaxBatch);
    double *s_w = s_cen + 16 * p.kchunk;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;

    {
        const f64x2 *src = reinterpret_cast<const f64x2 *>(p.scratch);
        f64x2 *dst = reinterpret_cast<f64x2 *>(smem);
        for (int q = tid; q < (int)(s64_cen_at(NT) / 2); q += kS64Threads) dst[q] = src[q];
    }
    deal_out_pointers(s_ptr, p.nF);
    // K steps ks0 .. ks0 + nk - 1 of the model into LDS
    auto stage = [&](int ks0, int nk) {
        __syncthreads();
        const f64x2 *csrc = reinterpret_cast<const f64x2 *>(p.scratch + s64_cen_at(NT) + (size_t)16 * ks0);
        f64x2 *cdst = reinterpret_cast<f64x2 *>(s_cen);
        for (int q = tid; q < nk * 8; q += kS64Threads) cdst[q] = csrc[q];
        const f64x2 *wsrc = reinterpret_cast<const f64x2 *>(p.scratch + s64_w_at(NT, p.Mpad) + (size_t)ks0 * NT * 64);
        f64x2 *wdst = reinterpret_cast<f64x2 *>(s_w);
        for (int q = tid; q < nk * NT * 32; q += kS64Threads) wdst[q] = wsrc[q];
        __syncthreads();
    };
    const bool resident = p.nks <= p.kchunk;
    if (resident) stage(0, p.nks);
    else __syncthreads();

    const f64x4 zero4 = {0.0, 0.0, 0.0, 0.0};
    constexpr double gs = packing::grad_scale64(KIND);
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t vi = ((int64_t)grp * kS64Waves + wave) * 16 + j;
        const bool inb = vi < p.N;
        const int64_t vc = inb ? vi : p.N - 1;
        const double px = p.P_in[3 * vc], py = p.P_in[3 * vc + 1], pz = p.P_in[3 * vc + 2];
        const float d2v = p.dist2 ? p.dist2[vc] : 0.f;
        const bool live = inb && !(d2v > p.radius2);
        const bool work = __any(live);
        // (ahead of the K loop: one register across it, where behind it powf would sit on top of all the accumulators)
        const float fall = transport::falloff(p.dist2 != nullptr, p.radius2, p.falloffrate, d2v);
        // L_f as the first K = 4 step: A = the frames' affine coefficients {const, x, y, z}, B = the unit vector of slot 1 + d
        // (exact: one coefficient times 1, the others times 0)
        f64x4 acc[3][NT];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double unit = g == 1 + d ? 1.0 : 0.0;
#pragma unroll
            for (int T = 0; T < NT; ++T) acc[d][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_aff[T * 64 + lane], unit, zero4, 0, 0, 0);
        }

        for (int ks0 = 0; ks0 < p.nks; ks0 += p.kchunk) {
            const int nk = p.nks - ks0 < p.kchunk ? p.nks - ks0 : p.kchunk;
            if (!resident) stage(ks0, nk);
            if (!work) continue;
            for (int ks = 0; ks < nk; ++ks) {
                // this lane's centre of the step: 4 ks + g
                const f64x2 *cr = reinterpret_cast<const f64x2 *>(s_cen + 16 * ks + 4 * g);
                const f64x2 c01 = cr[0], c23 = cr[1];
                const double dx = px - c01[0], dy = py - c01[1], dz = pz - c23[0];
                const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                const double gv = gs * packing::grad64<KIND>(d2, c23[1]);
                const double b[3] = {gv * dx, gv * dy, gv * dz};
                const double *wk = s_w + (size_t)ks * NT * 64 + lane;
#pragma unroll
                for (int T = 0; T < NT; ++T) {
                    const double a = wk[T * 64];
#pragma unroll
                    for (int d = 0; d < 3; ++d) acc[d][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[d], acc[d][T], 0, 0, 0);
                }
            }
        }

        // ---- epilogue: lane (g, j) finishes its vertex for the frames whose rows its lane group holds
        if (!inb) continue;
        FrameIO<double> io;
        io.tu = p.tu; io.tv = p.tv; io.nrm = p.nrm;
        io.vN = p.vN; io.vtu = p.vtu; io.vtv = p.vtv;
        if (live && p.tu && fall != 0.f) transport::axes<double>(p.tu, p.tv, p.nrm, vi, io.a1, io.a2);
        // the q-th frame this lane group holds, and the accumulator slot (tile, register) of its component c:
        //   dense:  lane group g's 12 registers s = 3 q' + c (register s % 4 of tile 3 B + s / 4) are frame 16 B + 4 g + q'
        //   padded: register c of tile T is frame 4 T + g
        constexpr int kHeld = DENSE ? 4 * (NT / 3) : NT;
        auto frame_of = [&](int q) { return DENSE ? 16 * (q / 4) + 4 * g + q % 4 : 4 * q + g; };
        auto tile_of = [](int q, int c) { return DENSE ? 3 * (q / 4) + (3 * (q % 4) + c) / 4 : q; };
        auto reg_of = [](int q, int c) { return DENSE ? (3 * (q % 4) + c) % 4 : c; };
        // first half, every frame: J_f in the accumulators becomes A_f in place (the axes die here, ahead of the cofactors)
        if (live) {
#pragma unroll
            for (int q = 0; q < kHeld; ++q) {
                const int f = frame_of(q);
                if (f >= p.nF || !s_head->built[f]) continue;
                double R[9], A[9];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < 3; ++k) R[3 * c + k] = acc[k][tile_of(q, c)][reg_of(q, c)];
                transport::jacobian<double>(io, vi, R, fall, A);
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < 3; ++k) acc[k][tile_of(q, c)][reg_of(q, c)] = A[3 * c + k];
            }
        }
        // second half: the vectors and A of every frame
#pragma unroll
        for (int q = 0; q < kHeld; ++q) {
            const int f = frame_of(q);
            if (f >= p.nF) continue;
            io.oN = s_ptr[4 * f]; io.otu = s_ptr[4 * f + 1]; io.otv = s_ptr[4 * f + 2]; io.jac = s_ptr[4 * f + 3];
            if (!live || !s_head->built[f]) {
                pass_through(io, vi);
                continue;
            }
            double A[9];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 3; ++k) A[3 * c + k] = acc[k][tile_of(q, c)][reg_of(q, c)];
            transport::carry<double>(io, vi, A);
        }
    }
}

template <int KIND>
hipError_t launch_kind(const ShotOut &out, const V64Params &p, int NT, bool dense, const ShotGrid &gr, hipStream_t stream)
{
    return for_tiles(NT, dense, [&](auto nt, auto dns) { return launch_shot<k_vectors64_shared<KIND, nt.value, dns.value>>(gr, stream, out, p); });
}

}  // namespace

hipError_t launch_vectors_shared64(const SharedVector64Args &a, hipStream_t stream)
{
    if (a.N <= 0 || a.nF <= 0) return hipSuccess;
    if (a.nF > kMaxBatch || a.Mpad <= 0 || a.Mpad % 16 != 0 || !a.scratch) return hipErrorInvalidValue;
    const int NT = s64_tiles(a.nF);
    const int nks = a.Mpad / 4;
    V64Params p{};
    ShotOut out{};
    fill_shot(p, out, a);
    p.nF = a.nF; p.nks = nks; p.Mpad = a.Mpad;
    p.scratch = (const double *)a.scratch;
    const size_t fixed = 8 * s64_cen_at(NT) + sizeof(float *) * 4 * kMaxBatch;
    const size_t per_ks = 8 * (16 + (size_t)NT * 64);
    p.kchunk = even_chunks(nks, (int)((kS64LdsBudget - fixed) / per_ks));
    ShotGrid gr;
    if (hipError_t e = shot_grid(a, fixed + per_ks * (size_t)p.kchunk, gr); e != hipSuccess) return e;
    const bool dense = a.nF > 12;
    switch (a.kind) {
    case FD_KERNEL_GAUSSIAN:
    case FD_KERNEL_GAUSSIAN_QNN: return launch_kind<FD_KERNEL_GAUSSIAN>(out, p, NT, dense, gr, stream);
    case FD_KERNEL_THIN_PLATE: return launch_kind<FD_KERNEL_THIN_PLATE>(out, p, NT, dense, gr, stream);
    case FD_KERNEL_BIHARMONIC: return launch_kind<FD_KERNEL_BIHARMONIC>(out, p, NT, dense, gr, stream);
    case FD_KERNEL_CUBIC: return launch_kind<FD_KERNEL_CUBIC>(out, p, NT, dense, gr, stream);
    default: return hipErrorInvalidValue;
    }
}

// The fewest frames at which the one launch beats the per-context k_vectors64_<kind> launches, measured at 1M vertices and
// 256 centres (profiles/vectors_shared_fp64_1M_256_kernel_stats.csv): a launch of one row tile costs the same
// for 1..4 frames -- the basis and one matrix instruction per direction per K step, 1.25 ms thin-plate, 0.83 ms Gaussian --
// while the per-context launches cost one basis per frame, 0.80 ms and 0.34 ms.  Biharmonic and cubic by device events at
// 1..4 frames: 0.84 ms against 0.46 ms per frame (1.06x at two frames) and 0.72 ms against 0.32 ms (0.89x at two, 1.30x at three).
int shared_vectors64_min_frames(int kind)
{
    switch (kind) {
    case FD_KERNEL_THIN_PLATE:
    case FD_KERNEL_BIHARMONIC: return 2;
    case FD_KERNEL_GAUSSIAN:
    case FD_KERNEL_GAUSSIAN_QNN:
    case FD_KERNEL_CUBIC: return 3;
    default: return 1;
    }
}

const char *shared_vectors64_kernel_name(int Mpad, int nF, int kind)
{
    return shared64_kernel_name(Mpad, nF, kind)[0] && nF >= shared_vectors64_min_frames(kind) ? "k_vectors64_shared" : "";
}

}  // namespace fd
