// fd_vectors_shared_ml64.hip -- the Jacobian and the vectors it carries for ALL frames of a shot of MULTILAYER models in
// fp64, one matrix-pipe launch (fd_batch_deform_vectors_shared_ml_fp64_dev).  The model is M x L Gaussian
// records with radii R / 2^l; the frames share the mesh and the rest rig, so the gradient basis g_l(x) (x - c) is formed
// ONCE per (vertex, record), in fp64 from direct differences of the raw coordinates, and contracted with every frame's
// fp64 weights on v_mfma_f64_16x16x4_f64:
//     J_f(x) = sum_c sum_l w_f[c][l] (x) 2 s_l E_l(x) (x - c) + L_f,
// three (N x M L) x (M L x 3F) products, one per direction of the gradient, against the weights k_pack_shared_ml64 left in
// the batch's multilayer-fp64 scratch in A-operand order [kc][l][T] (fd_shared_ml64.h: the position launch's layout, the
// one copy of it).
//
// Definition: k_vectors64_gaussian's (fd_vectors.hip) on the M L records, per frame -- the same d2 expression, fp64
// accumulation, then fd_transport.h's transport<double> -- but for
//   * the order and association of the fp64 sum: four centres of one layer per matrix instruction, w ((2 (E s)) d) for
//     2 (((E s) w) d), and L_f goes in first (one more K = 4 step against unit vectors, exact), and
//   * ONE exponential per centre and chain, k_deform64_shared_ml's chain exactly: E_0 = exp(d2 s_0) is the call
//     grad64<GAUSSIAN> makes, E <- (E E) (E E) gives the next layer, s_l = 4^(l - l0) s_chain exactly (the build forms R_l
//     with ldexp), and AT l = 4 THE CHAIN RESTARTS with a fresh exp(d2 s_4): never more than three quadruplings.  At
//     l = 0 and l = 4, E_l s_l is grad64<GAUSSIAN>(d2, s_l) bit for bit.
//
// Inputs: the scratch only (weights, centre records {cx, cy, cz, s_0, s_4}, affine tiles, frame status), the mesh and the
// vectors -- nothing of the contexts, so fd_batch_wait_consumed covers this launch as it does the position launch.
//
// Mapping: k_vectors64_shared's with k_deform64_shared_ml's centre ownership.  8 waves per workgroup, persistent; a wave owns
// ONE vertex tile of 16 per group.  Lane (g, j) = (lane >> 4, lane & 15) holds vertex j and OWNS centre 4 kc + g of centre
// step kc for all of its layers: d and d2 once, then per layer the basis b_k = g_l d_k and 3 x NT matrix instructions, the
// three directions against the one A value read from LDS.  Rows are dealt by s64_row, so lane group g holds whole frames
// and finishes them alone: projection axes once per vertex, A_f = I + f Pi J_f for all its frames in place of J_f, then
// the vectors per frame (fd_transport.h's two halves), non-temporal stores.  The model is staged in chunks of whole centre
// steps -- a chunk boundary never separates a centre's layers -- evened out, with the accumulators live across them.
// No floating-point atomics; a vertex's bits depend on its column of its own matrix instructions only, not on its place
// in the launch.  Built with -ffp-contract=off like the rest.
#include <algorithm>

#include "fd_eval_common.h"
#include "fd_pack.h"
#include "fd_shared64.h"
#include "fd_shared_ml64.h"
#include "fd_vectors_shot.h"
#include "fd_tuning.h"

namespace fd {

namespace {

struct VMl64Params : ShotMesh {
    int nF, nkc, kchunk, L, Mc4;
    const double *scratch;
};

// (the head of the scratch, the affine step and the epilogue are k_vectors64_shared's, fd_vectors_shared64.hip; the epilogue is
// each file's own text because a shared function compiles to a slower schedule: DESIGN.md 4.7f)
template <int NT, bool DENSE>
__global__ __launch_bounds__(kS64Threads) void k_vectors64_shared_ml(const ShotOut out, const VMl64Params p, int ngroups)
{
    (void)out;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [head][affine tiles NT x 64][output pointers 32 x 4][centre records kchunk x 4 x 6][weight tiles kchunk x L x NT x 64]
    const S64Head *s_head = reinterpret_cast<const S64Head *>(smem);
    const double *s_aff = reinterpret_cast<const double *>(smem) + s64_aff_at();
    float **s_ptr = reinterpret_cast<float **>(reinterpret_cast<double *>(smem) + ml64_cen_at(NT));
    double *s_cen = reinterpret_cast<double *>(s_ptr + 4 * kMaxBatch);
    double *s_w = s_cen + 4 * kMl64Cen * p.kchunk;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    const int L = p.L;
    const int stepw = L * NT * 64;                 // doubles of weights per centre step

    {
        const f64x2 *src = reinterpret_cast<const f64x2 *>(p.scratch);
        f64x2 *dst = reinterpret_cast<f64x2 *>(smem);
        for (int q = tid; q < (int)(ml64_cen_at(NT) / 2); q += kS64Threads) dst[q] = src[q];
    }
    deal_out_pointers(s_ptr, p.nF);
    // centre steps kc0 .. kc0 + nk - 1 of the model into LDS
    auto stage = [&](int kc0, int nk) {
        __syncthreads();
        const f64x2 *csrc = reinterpret_cast<const f64x2 *>(p.scratch + ml64_cen_at(NT) + (size_t)4 * kMl64Cen * kc0);
        f64x2 *cdst = reinterpret_cast<f64x2 *>(s_cen);
        for (int q = tid; q < nk * 2 * kMl64Cen; q += kS64Threads) cdst[q] = csrc[q];
        const f64x2 *wsrc = reinterpret_cast<const f64x2 *>(p.scratch + ml64_w_at(NT, p.Mc4) + (size_t)kc0 * stepw);
        f64x2 *wdst = reinterpret_cast<f64x2 *>(s_w);
        for (int q = tid; q < nk * (stepw / 2); q += kS64Threads) wdst[q] = wsrc[q];
        __syncthreads();
    };
    const bool resident = p.nkc <= p.kchunk;
    if (resident) stage(0, p.nkc);
    else __syncthreads();

    const f64x4 zero4 = {0.0, 0.0, 0.0, 0.0};
    constexpr double gs = packing::grad_scale64(FD_KERNEL_GAUSSIAN);
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t vi = ((int64_t)grp * kS64Waves + wave) * 16 + j;
        const bool inb = vi < p.N;
        const int64_t vc = inb ? vi : p.N - 1;
        // (fp32 across the K loop, widened per centre: three registers for six)
        const float pxf = p.P_in[3 * vc], pyf = p.P_in[3 * vc + 1], pzf = p.P_in[3 * vc + 2];
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

        for (int kc0 = 0; kc0 < p.nkc; kc0 += p.kchunk) {
            const int nk = p.nkc - kc0 < p.kchunk ? p.nkc - kc0 : p.kchunk;
            if (!resident) stage(kc0, nk);
            if (!work) continue;
            for (int kc = 0; kc < nk; ++kc) {
                // this lane's centre of the step, for all of its layers: 4 kc + g
                const f64x2 *cr = reinterpret_cast<const f64x2 *>(s_cen + 4 * kMl64Cen * kc + kMl64Cen * g);
                const f64x2 c01 = cr[0], c2s = cr[1];
                const double dx = (double)pxf - c01[0], dy = (double)pyf - c01[1], dz = (double)pzf - c2s[0];
                const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                const double *wk = s_w + (size_t)kc * stepw + lane;
                for (int l0 = 0; l0 < L; l0 += kMl64Restart) {
                    // a chain starts with the exponential grad64<GAUSSIAN> takes for this record ...
                    double sl = l0 == 0 ? c2s[1] : cr[2][0];
                    double E = exp(d2 * sl);
                    const int lend = L - l0 < kMl64Restart ? L : l0 + kMl64Restart;
                    for (int l = l0; l < lend; ++l) {
                        const double gv = gs * (E * sl);
                        const double b[3] = {gv * dx, gv * dy, gv * dz};
#pragma unroll
                        for (int T = 0; T < NT; ++T) {
                            const double a = wk[(l * NT + T) * 64];
#pragma unroll
                            for (int d = 0; d < 3; ++d) acc[d][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[d], acc[d][T], 0, 0, 0);
                        }
                        // ... and the next layer's radius is half this one's: E^4, 4 s
                        const double e2 = E * E;
                        E = e2 * e2;
                        sl = 4.0 * sl;
                    }
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

}  // namespace

hipError_t launch_vectors_shared_ml64(const SharedVectorMl64Args &a, hipStream_t stream)
{
    if (a.N <= 0 || a.nF <= 0) return hipSuccess;
    if (!shared_ml64_applies(a.M, a.layers, a.nF) || !a.scratch) return hipErrorInvalidValue;
    const int NT = s64_tiles(a.nF);
    const int Mc4 = round_up(a.M, 4), nkc = Mc4 / 4, L = a.layers;
    VMl64Params p{};
    ShotOut out{};
    fill_shot(p, out, a);
    p.nF = a.nF; p.nkc = nkc; p.L = L; p.Mc4 = Mc4;
    p.scratch = (const double *)a.scratch;
    const size_t fixed = 8 * ml64_cen_at(NT) + sizeof(float *) * 4 * kMaxBatch;
    const size_t per_kc = 8 * ((size_t)4 * kMl64Cen + ml64_step_w(NT, L));
    p.kchunk = even_chunks(nkc, (int)((kS64LdsBudget - fixed) / per_kc));         // kmax >= 6: 8 layers x 6 tiles are 24.2 KiB a step
    ShotGrid gr;
    if (hipError_t e = shot_grid(a, fixed + per_kc * (size_t)p.kchunk, gr); e != hipSuccess) return e;
    return for_tiles(NT, a.nF > 12, [&](auto nt, auto dns) { return launch_shot<k_vectors64_shared_ml<nt.value, dns.value>>(gr, stream, out, p); });
}

// The fewest frames at which the one launch is ahead of the per-context k_vectors64_gaussian launches over the M L records,
// measured at 1M vertices and 256 centres with the launch taken at every frame count (DESIGN.md 4.7d,
// profiles/vectors_shared_ml_fp64_1M_256_events.csv and ..._small_frames.csv).  A launch of one row tile (1..4 frames) takes
// 0.89 / 1.30 / 1.91 / 2.33 / 3.20 / 3.62 / 4.10 / 4.52 ms with 1..8 layers at one frame, the per-context launches 0.34 / 0.67 / 0.98 /
// 1.31 / 1.64 / 1.97 / 2.29 / 2.61 ms per frame: behind at one frame with every layer count; at two frames 0.76x with one layer,
// 1.02x .. 1.15x with 2..8 (the chain saves exponentials only from the second layer on); at three 1.13x with one.
int shared_vectors_ml64_min_frames(int layers)
{
    // tuning builds only (fd_tuning.h): FD_VML64_MIN_FRAMES=1 lets tools/vectors_shared_ml_fp64_profile.py time the launch
    // below the threshold; the product library reads no environment variable
    static const char *force = tuning_env("FD_VML64_MIN_FRAMES");
    if (force && atoi(force) >= 1) return atoi(force);
    return layers <= 1 ? 3 : 2;
}

const char *shared_vectors_ml64_kernel_name(int M, int layers, int nF)
{
    return shared_ml64_applies(M, layers, nF) && nF >= shared_vectors_ml64_min_frames(layers) ? "k_vectors64_shared_ml" : "";
}

}  // namespace fd
