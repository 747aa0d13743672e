// fd_eval_shared64.hip -- ALL frames of a shot evaluated in fp64 by one matrix-pipe launch
// (fd_batch_deform_shared_fp64_dev).  The frames share the mesh and the rest rig, so phi(|x - c_j|^2) is
// formed ONCE per (vertex, centre), in fp64 from direct differences of the raw coordinates, and contracted with every
// frame's fp64 weights on v_mfma_f64_16x16x4_f64: Phi is N x M, W is M x 3F.
//
// Definition: k_deform64's (fd_eval.hip), per frame -- the same phi64<KIND>, the same d2 expression, fp64 accumulation on
// top of the fp64 affine part, ONE rounding of the three sums to fp32, then epilogue_store.  Only the order of the fp64
// summation differs (four centres per matrix instruction, the affine part as one more K = 4 step).
//
// Those pieces -- phi64 / fast_log_pos, EvalParams and epilogue_store -- are fd_eval_point.h's: the very code the one-frame
// launch runs, with no second copy to keep in step.  The host side of the launch is fd_shot_launch.h's.
//
// Two kernels:
//   k_pack_shared64  the only reader of the contexts' models.  Writes, into scratch of the batch that nothing else uses:
//                    {built[32], P_out[32], falloff_out[32]}, the affine tiles, the rest rig's centre records
//                    {cx, cy, cz, s} (frame 0's: one rig) and the weights in A-operand tile order.  A frame whose model
//                    is not built, or whose centres differ from frame 0's, gets built = 0 and zero weights.
//   k_deform64_shared<KIND, NT, DENSE>
//                    8 waves per workgroup, persistent; a wave owns 32 vertices (two vertex tiles of 16) per group.
//                    Lane (g, j) = (lane >> 4, lane & 15) holds vertex j and, per K step of 4 centres, forms phi of
//                    centre 4 ks + g: exactly the B-operand layout, no exchange between lanes.  The A operand is one
//                    double per lane from LDS (row lane & 15, centre lane >> 4), shared by the two vertex tiles.
//                    The accumulator of row tile T holds, in lane group g, rows g, g + 4, g + 8, g + 12 for the lane's
//                    vertex.  Rows are dealt so that these are whole frames:
//                      F <= 12 (padded): row g + 4 c of tile T is component c of frame 4 T + g (rows 12..15 unused);
//                      F >= 13 (dense):  three tiles carry 16 frames; lane group g's 12 values s = 3 q + c
//                                        (register s % 4 of tile 3 B + s / 4) are component c of frame 16 B + 4 g + q.
//                    Either way every lane finishes its frames alone: round to fp32, epilogue_store.
//   LDS: the fp64 weights of M = 256 x 96 rows are 196 KB, more than a CU has, so the model is staged in chunks of
//   K steps with the accumulators kept live across them (two passes over half the frames would form phi twice, and phi is
//   the expensive part); a model that fits is staged once per workgroup.
// No floating-point atomics; a vertex's bits depend on its column of its own matrix instructions only, not on its
// place in the launch.  Built with -ffp-contract=off like the rest.
#include <cstdio>
#include <cstdlib>

#include "fd_eval_point.h"
#include "fd_shared64.h"
#include "fd_shot_launch.h"

namespace fd {

namespace {

constexpr int kS64VT = 2;                                 // vertex tiles per wave
constexpr int kS64Group = 16 * kS64VT * kS64Waves;        // vertices per workgroup and group
constexpr int kS64PackThreads = 256;
static_assert(kS64Threads == kShotThreads, "launch_shot's workgroup");

// (the scratch layout, S64Head, s64_tiles and s64_row: fd_shared64.h, shared with the vector launch)

struct S64PackArgs {
    const Rec64 *rec[kMaxBatch];
    const DevModel *model[kMaxBatch];
    const double *centres[kMaxBatch];     // fp64 M x 3 per context; entry f == entry 0: not compared
    float *P_out[kMaxBatch];
    float *fall[kMaxBatch];
};

// threads [0, 64 nF): one wave per frame -- status, outputs, the centre comparison; then one thread per double
__global__ __launch_bounds__(kS64PackThreads) void k_pack_shared64(const S64PackArgs a, double *scratch, int nF, int M, int Mpad,
                                                                   int NT, int dense, int *mismatch)
{
    const size_t idx = (size_t)blockIdx.x * kS64PackThreads + threadIdx.x;
    const size_t nhead = (size_t)64 * kMaxBatch;
    if (idx < nhead) {
        const int f = (int)(idx >> 6), lane = (int)(idx & 63);
        S64Head *h = reinterpret_cast<S64Head *>(scratch);
        if (f >= nF) {
            if (lane == 0) { h->built[f] = 0; h->P_out[f] = nullptr; h->fall[f] = nullptr; }
            return;
        }
        bool differs = false;
        if (a.centres[f] != a.centres[0])
            for (int q = lane; q < 3 * M; q += 64) differs |= a.centres[f][q] != a.centres[0][q];
        differs = __any(differs);
        if (lane == 0) {
            h->built[f] = (a.model[f]->terminationtype == 1 && !differs) ? 1 : 0;
            h->P_out[f] = a.P_out[f];
            h->fall[f] = a.fall[f];
            if (differs && mismatch) *mismatch = 1 + f;
        }
        return;
    }
    size_t q = idx - nhead;
    const size_t naff = (size_t)NT * 64, ncen = (size_t)Mpad * 4, nw = (size_t)(Mpad / 4) * NT * 64;
    if (q < naff) {
        // A operand of the affine step: lane l = row (l & 15), k = l >> 4 of [1, x, y, z]
        const int T = (int)(q >> 6), l = (int)(q & 63);
        int f, c;
        s64_row(dense != 0, T, l & 15, f, c);
        scratch[s64_aff_at() + q] = (f < nF && c < 3) ? a.model[f]->affine64[4 * c + (l >> 4)] : 0.0;
        return;
    }
    q -= naff;
    if (q < ncen) {
        const Rec64 &r = a.rec[0][q >> 2];
        const int e = (int)(q & 3);
        scratch[s64_cen_at(NT) + q] = e == 0 ? r.cx : e == 1 ? r.cy : e == 2 ? r.cz : r.s;
        return;
    }
    q -= ncen;
    if (q < nw) {
        const int l = (int)(q & 63), T = (int)((q >> 6) % NT), ks = (int)((q >> 6) / NT);
        int f, c;
        s64_row(dense != 0, T, l & 15, f, c);
        double w = 0.0;
        if (f < nF && c < 3 && a.model[f]->terminationtype == 1) {
            const Rec64 &r = a.rec[f][4 * ks + (l >> 4)];
            w = c == 0 ? r.wx : c == 1 ? r.wy : r.wz;
        }
        scratch[s64_w_at(NT, Mpad) + q] = w;
    }
}

struct S64Params : ShotEvalMesh {
    int nF, nks, kchunk, delta, Mpad;
    const double *scratch;
};

template <int KIND, int NT, bool DENSE>
__global__ __launch_bounds__(kS64Threads) void k_deform64_shared(const S64Params p, int ngroups)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [head][affine tiles NT x 64][centre records kchunk x 4 x 4][weight tiles kchunk x NT x 64]
    const S64Head *s_head = reinterpret_cast<const S64Head *>(smem);
    double *s_aff = reinterpret_cast<double *>(smem) + s64_aff_at();
    double *s_cen = s_aff + NT * 64;
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
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        float pf[kS64VT][3], d2v[kS64VT];
        int64_t vi[kS64VT];
        bool live[kS64VT], inb[kS64VT];
        bool any_live = false;
#pragma unroll
        for (int t = 0; t < kS64VT; ++t) {
            vi[t] = (((int64_t)grp * kS64Waves + wave) * kS64VT + t) * 16 + j;
            inb[t] = vi[t] < p.N;
            const int64_t vc = inb[t] ? vi[t] : p.N - 1;
            pf[t][0] = p.P_in[3 * vc]; pf[t][1] = p.P_in[3 * vc + 1]; pf[t][2] = p.P_in[3 * vc + 2];
            d2v[t] = p.dist2 ? p.dist2[vc] : 0.f;
            live[t] = inb[t] && !(d2v[t] > p.radius2);
            any_live |= live[t];
        }
        const bool work = __any(any_live);

        // the affine part as the first K = 4 step: A = the frames' coefficients, B = [1, x, y, z]
        f64x4 acc[kS64VT][NT];
#pragma unroll
        for (int t = 0; t < kS64VT; ++t) {
            const double b = g == 0 ? 1.0 : (double)(g == 1 ? pf[t][0] : g == 2 ? pf[t][1] : pf[t][2]);
#pragma unroll
            for (int T = 0; T < NT; ++T) acc[t][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_aff[T * 64 + lane], b, zero4, 0, 0, 0);
        }

        for (int ks0 = 0; ks0 < p.nks; ks0 += p.kchunk) {
            const int nk = p.nks - ks0 < p.kchunk ? p.nks - ks0 : p.kchunk;
            if (!resident) stage(ks0, nk);
            if (!work) continue;
            for (int ks = 0; ks < nk; ++ks) {
                // this lane's centre of the step: 4 ks + g
                const f64x2 *cr = reinterpret_cast<const f64x2 *>(s_cen + 16 * ks + 4 * g);
                const f64x2 c01 = cr[0], c23 = cr[1];
                double ph[kS64VT];
#pragma unroll
                for (int t = 0; t < kS64VT; ++t) {
                    const double dx = (double)pf[t][0] - c01[0];
                    const double dy = (double)pf[t][1] - c01[1];
                    const double dz = (double)pf[t][2] - c23[0];
                    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                    ph[t] = phi64<KIND>(d2, c23[1]);
                }
                const double *wk = s_w + (size_t)ks * NT * 64 + lane;
#pragma unroll
                for (int T = 0; T < NT; ++T) {
                    const double a = wk[T * 64];
#pragma unroll
                    for (int t = 0; t < kS64VT; ++t) acc[t][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ph[t], acc[t][T], 0, 0, 0);
                }
            }
        }

        // ---- epilogue: lane (g, j) finishes its vertices for the frames whose rows its lane group holds
#pragma unroll
        for (int t = 0; t < kS64VT; ++t) {
            if (!inb[t]) continue;
            const int64_t i = vi[t];
            const float pos[3] = {pf[t][0], pf[t][1], pf[t][2]};
            auto finish = [&](int f, double a0, double a1, double a2) {
                if (f >= p.nF) return;
                float *out = s_head->P_out[f];
                if (!live[t] || !s_head->built[f]) {
                    if (p.delta) {
                        out[3 * i] = 0.f; out[3 * i + 1] = 0.f; out[3 * i + 2] = 0.f;       // a gated or unbuilt vertex does not move
                    } else if (out != p.P_in) {
                        out[3 * i] = pos[0]; out[3 * i + 1] = pos[1]; out[3 * i + 2] = pos[2];
                    }
                    return;
                }
                const EvalParams ep = shot_eval_params(p, out, s_head->fall[f], p.Mpad, p.delta);
                float disp[3] = {(float)a0, (float)a1, (float)a2};           // the ONE rounding
                epilogue_store(ep, i, pos, disp, d2v[t]);
            };
            if constexpr (DENSE) {
#pragma unroll
                for (int B = 0; B < NT / 3; ++B)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        finish(16 * B + 4 * g + q, acc[t][3 * B + (3 * q) / 4][(3 * q) % 4], acc[t][3 * B + (3 * q + 1) / 4][(3 * q + 1) % 4],
                               acc[t][3 * B + (3 * q + 2) / 4][(3 * q + 2) % 4]);
            } else {
#pragma unroll
                for (int T = 0; T < NT; ++T) finish(4 * T + g, acc[t][T][0], acc[t][T][1], acc[t][T][2]);
            }
        }
    }
}

template <int KIND>
hipError_t launch_kind64(const S64Params &p, int NT, bool dense, const ShotGrid &gr, hipStream_t stream)
{
    return for_tiles(NT, dense, [&](auto nt, auto dns) { return launch_shot<k_deform64_shared<KIND, nt.value, dns.value>>(gr, stream, p); });
}

}  // namespace

size_t shared64_scratch_bytes(int Mpad, int nF)
{
    const int NT = s64_tiles(nF);
    return 8 * (s64_w_at(NT, Mpad) + (size_t)(Mpad / 4) * NT * 64);
}

hipError_t launch_deform_shared64(const Shared64Args &a, hipStream_t stream)
{
    if (a.N <= 0 || a.nF <= 0) return hipSuccess;
    if (a.nF > kMaxBatch || a.Mpad <= 0 || a.Mpad % 16 != 0 || !a.scratch) return hipErrorInvalidValue;
    const int NT = s64_tiles(a.nF);
    const bool dense = a.nF > 12;
    const int nks = a.Mpad / 4;

    S64PackArgs pa{};
    fill_pack(pa, a, a.rec64);
    for (int f = 0; f < a.nF; ++f) pa.centres[f] = a.centres[f];
    const size_t nthreads = (size_t)64 * kMaxBatch + (size_t)NT * 64 + (size_t)a.Mpad * 4 + (size_t)nks * NT * 64;
    const unsigned pgrid = (unsigned)((nthreads + kS64PackThreads - 1) / kS64PackThreads);
    hipLaunchKernelGGL(k_pack_shared64, dim3(pgrid), dim3(kS64PackThreads), 0, stream, pa, (double *)a.scratch, a.nF, a.M, a.Mpad, NT,
                       dense ? 1 : 0, a.mismatch);
    if (hipError_t e = shot_packed(a, stream); e != hipSuccess) return e;

    S64Params p{};
    fill_eval_mesh(p, a);
    p.nF = a.nF; p.nks = nks; p.delta = a.delta_out; p.Mpad = a.Mpad;
    p.scratch = (const double *)a.scratch;
    const size_t fixed = 8 * s64_cen_at(NT);
    const size_t per_ks = 8 * (16 + (size_t)NT * 64);
    p.kchunk = even_chunks(nks, (int)((kS64LdsBudget - fixed) / per_ks));
    ShotGrid gr;          // two workgroups per CU at most
    if (hipError_t e = shot_grid(a.N, kS64Group, a.max_wgs, fixed + per_ks * (size_t)p.kchunk, 2, gr); e != hipSuccess) return e;
    switch (a.kind) {
    case FD_KERNEL_GAUSSIAN:
    case FD_KERNEL_GAUSSIAN_QNN: return launch_kind64<FD_KERNEL_GAUSSIAN>(p, NT, dense, gr, stream);
    case FD_KERNEL_THIN_PLATE: return launch_kind64<FD_KERNEL_THIN_PLATE>(p, NT, dense, gr, stream);
    case FD_KERNEL_BIHARMONIC: return launch_kind64<FD_KERNEL_BIHARMONIC>(p, NT, dense, gr, stream);
    case FD_KERNEL_CUBIC: return launch_kind64<FD_KERNEL_CUBIC>(p, NT, dense, gr, stream);
    default: return hipErrorInvalidValue;
    }
}

const char *shared64_kernel_name(int Mpad, int nF, int kind)
{
    if (Mpad <= 0 || Mpad % 16 != 0 || nF < 1 || nF > kMaxBatch) return "";
    switch (kind) {
    case FD_KERNEL_THIN_PLATE:
    case FD_KERNEL_GAUSSIAN:
    case FD_KERNEL_GAUSSIAN_QNN:
    case FD_KERNEL_BIHARMONIC:
    case FD_KERNEL_CUBIC: return "k_deform64_shared";
    default: return "";
    }
}

}  // namespace fd
