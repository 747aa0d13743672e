// fd_eval_shared_ml64.hip -- ALL frames of a shot of MULTILAYER models evaluated in fp64 by one matrix-pipe launch
// (fd_batch_deform_shared_ml_fp64_dev).  The solved multilayer model is M x L Gaussian records with radii
// R / 2^l, laid centre-major by k_pack (record c L + l); the rest rig, hence every centre and every radius, is the same for
// all frames of the shot, so Phi (N x M L) is formed ONCE and contracted with every frame's fp64 weights (M L x 3 F) on
// v_mfma_f64_16x16x4_f64 -- fd_eval_shared64.hip's structure, whose row dealing, head and tile count (fd_shared64.h) are
// reused as they are.
//
// Definition: k_deform64's (fd_eval.hip) on the multilayer records, per frame -- the same d2 expression on raw coordinates,
// fp64 accumulation on top of the fp64 affine part, ONE rounding of the three sums to fp32, then epilogue_store (both
// fd_eval_point.h's, the one-frame launch's own code) -- but for
//   * the order of the fp64 summation (four centres of one layer per matrix instruction, the affine part as one more
//     K = 4 step), and
//   * ONE exponential per centre and chain, not per record: the layers of a centre share d2, and R_l = R / 2^l makes
//     s_l = 4^l s_0 exactly (the build forms R_l with ldexp), so E_{l+1} = E_l^4.  E_0 = exp(d2 s_0) is the very call
//     phi64<GAUSSIAN> makes; E <- (E E) (E E) gives the next layer; AT l = 4 THE CHAIN RESTARTS with a fresh exp(d2 s_4).
//     A chain never runs longer than three quadruplings: 4^3 times the exponential's ulp plus the squarings' own
//     roundings, below 96 x 2^-53 relative.  The restart is part of the definition (the error statement of
//     include/facedeform_hip.h rests on it), not a tuning knob.
//
// Two kernels:
//   k_pack_shared_ml64   the only reader of the contexts' models.  Writes, into scratch of the batch that nothing else
//                        uses: the head {built[32], P_out[32], falloff_out[32]}, the affine tiles, per centre a record
//                        {cx, cy, cz, s_0, s_4, 0} from frame 0's fp64 records (s_4 only where L > 4), and the weights in
//                        A-operand order, layer-minor within a centre step: tile [kc][l][T], K step (kc, l) carrying
//                        centres 4 kc .. 4 kc + 3 at layer l.  The centre count is padded to a multiple of 4 with centres
//                        at the first centre's position, s = 0 and zero weights: E = 1, finite.  A frame whose model is
//                        not built, or whose records {c, s} differ from frame 0's, gets built = 0 and zero weights.
//   k_deform64_shared_ml<NT, DENSE>
//                        8 waves per workgroup, persistent; a wave owns 32 vertices (two vertex tiles of 16) per group.
//                        Lane (g, j) = (lane >> 4, lane & 15) holds vertex j and OWNS centre 4 kc + g for all of its
//                        layers: d2 once, then per layer NT x 2 matrix instructions with E as the B operand.
//   LDS: 256 centres x 4 layers x 32 frames are 768 KiB of weights, so the model is staged in chunks with the accumulators
//   kept live across them: the normal case.  Chunks are whole centre steps -- a chunk boundary never separates a centre's
//   layers -- and evened out.
// No floating-point atomics; a vertex's bits depend on its column of its own matrix instructions only, not on its place in
// the launch nor on the number of workgroups.  Built with -ffp-contract=off like the rest.
#include <cstdio>
#include <cstdlib>

#include "fd_eval_point.h"
#include "fd_shared64.h"
#include "fd_shared_ml64.h"
#include "fd_shot_launch.h"

namespace fd {

namespace {

constexpr int kMl64VT = 2;                                // vertex tiles per wave
constexpr int kMl64Group = 16 * kMl64VT * kS64Waves;      // vertices per workgroup and group
constexpr int kMl64PackThreads = 256;
constexpr int kMl64MinFrames = 1;                         // fewer frames: fd_batch_deform_shared_fp64_dev
// (the scratch layout -- kMl64Cen, kMl64Restart, ml64_cen_at, ml64_w_at, ml64_step_w -- is fd_shared_ml64.h's: the vector launch reads it too)

struct Ml64PackArgs {
    const Rec64 *rec[kMaxBatch];          // per frame: M x L records, centre-major (k_pack)
    const DevModel *model[kMaxBatch];
    float *P_out[kMaxBatch];
    float *fall[kMaxBatch];
};

// threads [0, 64 kMaxBatch): one wave per frame -- status, outputs, the record comparison; then one thread per double
__global__ __launch_bounds__(kMl64PackThreads) void k_pack_shared_ml64(const Ml64PackArgs a, double *scratch, int nF, int M, int L, int Mc4,
                                                                       int NT, int dense, int check_rig, int *mismatch)
{
    const size_t idx = (size_t)blockIdx.x * kMl64PackThreads + threadIdx.x;
    const size_t nhead = (size_t)64 * kMaxBatch;
    if (idx < nhead) {
        const int f = (int)(idx >> 6), lane = (int)(idx & 63);
        S64Head *h = reinterpret_cast<S64Head *>(scratch);
        if (f >= nF) {
            if (lane == 0) { h->built[f] = 0; h->P_out[f] = nullptr; h->fall[f] = nullptr; }
            return;
        }
        bool differs = false;
        if (check_rig && a.rec[f] != a.rec[0])
            for (int r = lane; r < M * L; r += 64) {
                const Rec64 &x = a.rec[f][r], &y = a.rec[0][r];
                differs |= x.cx != y.cx || x.cy != y.cy || x.cz != y.cz || x.s != y.s;
            }
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
    const size_t naff = (size_t)NT * 64, ncen = (size_t)Mc4 * kMl64Cen, nw = (size_t)(Mc4 / 4) * ml64_step_w(NT, L);
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
        const int c = (int)(q / kMl64Cen), e = (int)(q % kMl64Cen);
        // a padding centre sits on the first centre with s = 0: E = 1, and its weights are zero
        const Rec64 &r0 = a.rec[0][(size_t)(c < M ? c : 0) * L];
        double v = 0.0;
        if (e == 0) v = r0.cx;
        else if (e == 1) v = r0.cy;
        else if (e == 2) v = r0.cz;
        else if (e == 3) v = c < M ? r0.s : 0.0;
        else if (e == 4) v = (c < M && L > kMl64Restart) ? a.rec[0][(size_t)c * L + kMl64Restart].s : 0.0;
        scratch[ml64_cen_at(NT) + q] = v;
        return;
    }
    q -= ncen;
    if (q < nw) {
        const int lane = (int)(q & 63);
        const size_t tile = q >> 6;
        const int T = (int)(tile % NT), l = (int)((tile / NT) % L), kc = (int)(tile / NT / L);
        const int c = 4 * kc + (lane >> 4);
        int f, comp;
        s64_row(dense != 0, T, lane & 15, f, comp);
        double w = 0.0;
        if (c < M && f < nF && comp < 3 && a.model[f]->terminationtype == 1) {
            const Rec64 &r = a.rec[f][(size_t)c * L + l];
            w = comp == 0 ? r.wx : comp == 1 ? r.wy : r.wz;
        }
        scratch[ml64_w_at(NT, Mc4) + q] = w;
    }
}

struct Ml64Params : ShotEvalMesh {
    int nF, nkc, kchunk, L, delta, Mpad, Mc4;
    const double *scratch;
};

template <int NT, bool DENSE>
__global__ __launch_bounds__(kS64Threads) void k_deform64_shared_ml(const Ml64Params p, int ngroups)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [head][affine tiles NT x 64][centre records kchunk x 4 x 6][weight tiles kchunk x L x NT x 64]
    const S64Head *s_head = reinterpret_cast<const S64Head *>(smem);
    double *s_aff = reinterpret_cast<double *>(smem) + s64_aff_at();
    double *s_cen = s_aff + NT * 64;
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
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        float pf[kMl64VT][3], d2v[kMl64VT];
        int64_t vi[kMl64VT];
        bool live[kMl64VT], inb[kMl64VT];
        bool any_live = false;
#pragma unroll
        for (int t = 0; t < kMl64VT; ++t) {
            vi[t] = (((int64_t)grp * kS64Waves + wave) * kMl64VT + t) * 16 + j;
            inb[t] = vi[t] < p.N;
            const int64_t vc = inb[t] ? vi[t] : p.N - 1;
            pf[t][0] = p.P_in[3 * vc]; pf[t][1] = p.P_in[3 * vc + 1]; pf[t][2] = p.P_in[3 * vc + 2];
            d2v[t] = p.dist2 ? p.dist2[vc] : 0.f;
            live[t] = inb[t] && !(d2v[t] > p.radius2);
            any_live |= live[t];
        }
        const bool work = __any(any_live);

        // the affine part as the first K = 4 step: A = the frames' coefficients, B = [1, x, y, z]
        f64x4 acc[kMl64VT][NT];
#pragma unroll
        for (int t = 0; t < kMl64VT; ++t) {
            const double b = g == 0 ? 1.0 : (double)(g == 1 ? pf[t][0] : g == 2 ? pf[t][1] : pf[t][2]);
#pragma unroll
            for (int T = 0; T < NT; ++T) acc[t][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_aff[T * 64 + lane], b, zero4, 0, 0, 0);
        }

        for (int kc0 = 0; kc0 < p.nkc; kc0 += p.kchunk) {
            const int nk = p.nkc - kc0 < p.kchunk ? p.nkc - kc0 : p.kchunk;
            if (!resident) stage(kc0, nk);
            if (!work) continue;
            for (int kc = 0; kc < nk; ++kc) {
                // this lane's centre of the step, for all of its layers: 4 kc + g
                const f64x2 *cr = reinterpret_cast<const f64x2 *>(s_cen + 4 * kMl64Cen * kc + kMl64Cen * g);
                const f64x2 c01 = cr[0], c2s = cr[1], s4p = cr[2];
                double d2[kMl64VT];
#pragma unroll
                for (int t = 0; t < kMl64VT; ++t) {
                    const double dx = (double)pf[t][0] - c01[0];
                    const double dy = (double)pf[t][1] - c01[1];
                    const double dz = (double)pf[t][2] - c2s[0];
                    d2[t] = fma(dz, dz, fma(dy, dy, dx * dx));
                }
                const double *wk = s_w + (size_t)kc * stepw + lane;
                for (int l0 = 0; l0 < L; l0 += kMl64Restart) {
                    // a chain starts with the exponential phi64<GAUSSIAN> takes for this record ...
                    const double sc = l0 == 0 ? c2s[1] : s4p[0];
                    double E[kMl64VT];
#pragma unroll
                    for (int t = 0; t < kMl64VT; ++t) E[t] = phi64<FD_KERNEL_GAUSSIAN>(d2[t], sc);
                    const int lend = L - l0 < kMl64Restart ? L : l0 + kMl64Restart;
                    for (int l = l0; l < lend; ++l) {
#pragma unroll
                        for (int T = 0; T < NT; ++T) {
                            const double a = wk[(l * NT + T) * 64];
#pragma unroll
                            for (int t = 0; t < kMl64VT; ++t) acc[t][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, E[t], acc[t][T], 0, 0, 0);
                        }
                        // ... and the next layer's radius is half this one's: E^4
#pragma unroll
                        for (int t = 0; t < kMl64VT; ++t) {
                            const double e2 = E[t] * E[t];
                            E[t] = e2 * e2;
                        }
                    }
                }
            }
        }

        // ---- epilogue: lane (g, j) finishes its vertices for the frames whose rows its lane group holds
#pragma unroll
        for (int t = 0; t < kMl64VT; ++t) {
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

}  // namespace

bool shared_ml64_applies(int M, int layers, int nF)
{
    return M > 0 && layers >= 1 && layers <= kMaxLayers && nF >= kMl64MinFrames && nF <= kMaxBatch;
}

int shared_ml64_min_frames() { return kMl64MinFrames; }

size_t shared_ml64_scratch_bytes(int M, int layers, int nF)
{
    const int NT = s64_tiles(nF), Mc4 = round_up(M, 4);
    return 8 * (ml64_w_at(NT, Mc4) + (size_t)(Mc4 / 4) * ml64_step_w(NT, layers));
}

const char *shared_ml64_kernel_name(int M, int layers, int nF)
{
    return shared_ml64_applies(M, layers, nF) ? "k_deform64_shared_ml" : "";
}

hipError_t launch_deform_shared_ml64(const SharedMl64Args &a, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!shared_ml64_applies(a.M, a.layers, a.nF) || !a.scratch) return hipErrorInvalidValue;
    const int NT = s64_tiles(a.nF);
    const bool dense = a.nF > 12;
    const int Mc4 = round_up(a.M, 4), nkc = Mc4 / 4, L = a.layers;

    Ml64PackArgs pa{};
    fill_pack(pa, a, a.rec64);
    const size_t nthreads = (size_t)64 * kMaxBatch + (size_t)NT * 64 + (size_t)Mc4 * kMl64Cen + (size_t)nkc * ml64_step_w(NT, L);
    const unsigned pgrid = (unsigned)((nthreads + kMl64PackThreads - 1) / kMl64PackThreads);
    hipLaunchKernelGGL(k_pack_shared_ml64, dim3(pgrid), dim3(kMl64PackThreads), 0, stream, pa, (double *)a.scratch, a.nF, a.M, L, Mc4, NT,
                       dense ? 1 : 0, a.check_rig, a.mismatch);
    if (hipError_t e = shot_packed(a, stream); e != hipSuccess) return e;

    Ml64Params p{};
    fill_eval_mesh(p, a);
    p.nF = a.nF; p.nkc = nkc; p.L = L; p.delta = a.delta_out; p.Mpad = round_up(a.M * L, kRecPad); p.Mc4 = Mc4;
    p.scratch = (const double *)a.scratch;
    const size_t fixed = 8 * ml64_cen_at(NT);
    const size_t per_kc = 8 * ((size_t)4 * kMl64Cen + ml64_step_w(NT, L));
    // even chunks of whole centre steps; kmax >= 6: 8 layers x 6 tiles are 24.2 KiB a step
    p.kchunk = even_chunks(nkc, (int)((kS64LdsBudget - fixed) / per_kc));
    ShotGrid gr;          // two workgroups per CU at most
    if (hipError_t e = shot_grid(a.N, kMl64Group, a.max_wgs, fixed + per_kc * (size_t)p.kchunk, 2, gr); e != hipSuccess) return e;
    return for_tiles(NT, dense, [&](auto nt, auto dns) { return launch_shot<k_deform64_shared_ml<nt.value, dns.value>>(gr, stream, p); });
}

}  // namespace fd
