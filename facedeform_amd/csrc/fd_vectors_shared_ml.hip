// fd_vectors_shared_ml.hip -- the Jacobian and the vectors it carries for ALL frames of a shot of MULTILAYER models in
// fp32, one matrix-pipe launch (fd_batch_deform_vectors_shared_ml_dev).  The model is M x L Gaussian
// records with radii R / 2^l, centre-major (record c L + l); the frames share the mesh and the rest rig, so the gradient
// basis g_r(x) (x - c_r) is formed ONCE per (vertex, record) and contracted with every frame's weights on the matrix pipe:
//     J_f(x) = sum_r w_f[r] (x) grad phi_r(x) + L_f(x),
// three (N x M L) x (M L x 3F) products, one per direction of the gradient, against the split fp16 weight tiles
// k_pack_shared_ml (fd_eval_shared_ml.hip) left in the batch's multilayer scratch (fd_shared_ml.h: the position launch's
// layout, the one copy of it).  The transport itself (Pi, fall-off, A, cofactors, rescale) is fd_transport.h, the
// one-frame launch's own code.
//
// Inputs: the scratch only (weight tiles, records {c'x, c'y, c'z, s_l}, polynomial tiles, frame records, normalisation),
// the mesh and the vectors -- nothing of the contexts, so fd_batch_wait_consumed covers this launch as it does the
// position launch.
//
// Mapping: k_vectors32_shared_gaussian's (fd_vectors_shared.hip) with k_deform32_shared_ml's record ownership.  8 waves per
// workgroup, persistent; a wave owns ONE vertex tile of 16 per group.  A K block is 32 consecutive records.  Lane
// (g, j) = (lane >> 4, lane & 15) holds vertex j and, as the eight K values of its B operand, the two aligned runs of four
// records 16 (g >> 1) + 4 (g & 1) + 8 a .. + 3, a = 0, 1: with L in {4, 8} layers of ONE centre, with L in {2, 6} two pairs
// of layers of one centre each, so x' - c' and d2 are formed once per SHARE = ml_share(L) records.  Every layer has its own
// multiply by its s_l and its own v_exp_f32 (never E_{l+1} = E_l^4: DESIGN.md 6d), its three basis values
// 2^8 s_l E_l (x' - c') and their fp16 hi / lo split; 3 directions x 3 split products per row tile on
// v_mfma_f32_16x16x32_f16, fp32 accumulation.
//   That run order is the pack kernel's own: K step s = g >> 1, lane half h = g & 1 of its 32 x 32 x 16 A operand hold
// exactly these eight records in this order, so staging deals whole 16-byte words -- row 3 f + c of the 32-row stack to the
// row the 16-row tiles want it in (padded up to 12 frames, dense from 13: k_vectors32_shared's order), rows of no frame
// zero -- and the weights are packed once, by the position launch.
//   The accumulator of tile T, direction d holds in lane group g rows 4 g .. 4 g + 3 for the lane's vertex: all three
// components of whole frames, so every lane finishes its frames with no exchange between lanes.  The model is staged in
// chunks of K blocks, evened out, with the accumulators live across them; zero records (the padding of the last block)
// give a zero basis.
// No floating-point atomics; a vertex's bits depend on its column of its own matrix instructions only, not on its place in
// the launch.  Built with -ffp-contract=off like the rest: every fused multiply-add is written out.
#include <algorithm>
#include <cstdlib>

#include "fd_eval_common.h"
#include "fd_pack.h"
#include "fd_shared_ml.h"
#include "fd_vectors_shot.h"
#include "fd_tuning.h"

namespace fd {

namespace {

// The basis enters the matrix pipe as 2^8 g (x' - c'), the one-layer launch's prescale (fd_vectors_shared.hip):
// |g (x' - c')| <= 0.52 sqrt(|s_l|), s_l = -log2(e) / R_l'^2, so its hi piece stays below the fp16 maximum for R_l' above
// ~0.0024 rig radii -- the FINEST layer's radius, R' / 2^(L - 1) (include/facedeform_hip.h states it); lo pieces are exact
// down to 2^-11.
constexpr int kVmlGradShift = 8;

struct VmlParams : ShotMesh {
    int nF, nkb, kchunk, srcNT;             // srcNT: ml_tiles(nF), the 32-row tiles the pack kernel wrote
    const uint4 *scratch;
};

// NT row tiles of 16: padded (tile T = frames 4 T .. 4 T + 3, row 4 (f % 4) + c) or DENSE (tile 3 B + c = component c of
// frames 16 B + row); SHARE consecutive records are layers of one centre
template <int NT, bool DENSE, int SHARE>
__global__ __launch_bounds__(kShotThreads) void k_vectors32_shared_ml(const ShotOut out, const VmlParams p, int ngroups)
{
    (void)out;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [frame constants 32 x 16 words][output pointers 32 x 4][records kchunk x 32 x 16 B][weight tiles kchunk x NT x 2 KiB]
    float *s_fc = reinterpret_cast<float *>(smem);
    float **s_ptr = reinterpret_cast<float **>(smem + sizeof(float) * kFrameWords * kMaxBatch);
    float4 *s_c = reinterpret_cast<float4 *>(smem + sizeof(float) * kFrameWords * kMaxBatch + sizeof(float *) * 4 * kMaxBatch);
    uint4 *s_w = reinterpret_cast<uint4 *>(s_c + 32 * p.kchunk);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    const float4 nrm4 = *reinterpret_cast<const float4 *>(p.scratch + kMlNormAt);
    const float n0 = nrm4.x, n1 = nrm4.y, n2 = nrm4.z, inv_s = nrm4.w;

    // frame constants: the basis scale 2^-k 2^-8 and the frame's linear part {L', q} (hi + lo of the polynomial tile: exact
    // in fp32, the 22 bits the position launch uses), 2^-k undone
    if (tid < p.nF) {
        const int f = tid;
        const unsigned *frames = reinterpret_cast<const unsigned *>(p.scratch);      // SharedFrame: {inv_scale, built, ...}, 8 words
        const float inv = __uint_as_float(frames[8 * f]);
        const float unscale = inv * (float)(1 << kGaussShift);                        // 2^-k
        float *fc = s_fc + kFrameWords * f;
        fc[0] = unscale * (1.f / (float)(1 << kVmlGradShift));
        fc[1] = frames[8 * f + 1] != 0u ? 1.f : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // lane 32 h + rho of polynomial tile T (k_pack_shared_ml): half 0 holds the hi pieces of {C0, Lx, Ly, Lz, q} in
            // elements 0..4, half 1 their lo pieces in elements 1..5
            const int row = 3 * f + c, T = row / 32, r = row % 32;
            const size_t w = kMlPolyAt + (size_t)T * 64;
            float coef[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) coef[e] = (half_at(p.scratch, w + r, e) + half_at(p.scratch, w + 32 + r, e + 1)) * unscale;
#pragma unroll
            for (int k = 0; k < 3; ++k) fc[2 + 3 * c + k] = coef[1 + k];
            fc[11 + c] = coef[4];
        }
    }
    deal_out_pointers(s_ptr, p.nF);
    // K blocks kb0 .. kb0 + nk - 1 of the model into LDS: the records as they are, the weight tiles dealt by whole words
    // from row 3 f + c of the 32-row stack into the 16-row order (above)
    auto stage = [&](int kb0, int nk) {
        __syncthreads();
        const uint4 *rsrc = p.scratch + ml_rec_at(p.srcNT) + (size_t)kb0 * 32;
        for (int q = tid; q < nk * 32; q += kShotThreads) reinterpret_cast<uint4 *>(s_c)[q] = rsrc[q];
        const uint4 *wsrc = p.scratch + ml_w_at(p.srcNT, p.nkb);
        for (int q = tid; q < nk * NT * 128; q += kShotThreads) {
            const int kb = kb0 + q / (NT * 128), rem = q % (NT * 128);
            const int T = rem / 128, hl = (rem >> 6) & 1, ln = rem & 63;
            const int gg = ln >> 4, rho = ln & 15;
            const int f = DENSE ? 16 * (T / 3) + rho : 4 * T + (rho >> 2), c = DENSE ? T % 3 : rho & 3;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (f < p.nF && c < 3) {
                const int row = 3 * f + c, Ts = row / 32, r = row % 32;
                v = wsrc[(size_t)kb * ml_w16(p.srcNT) + (size_t)((Ts * 2 + (gg >> 1)) * 2 + hl) * 64 + 32 * (gg & 1) + r];
            }
            s_w[q] = v;
        }
        __syncthreads();
    };
    const bool resident = p.nkb <= p.kchunk;
    if (resident) stage(0, p.nkb);
    else __syncthreads();

    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float gs = packing::grad_scale32(FD_KERNEL_GAUSSIAN);
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t vi = ((int64_t)grp * kShotWaves + wave) * 16 + j;
        const bool inb = vi < p.N;
        const int64_t vc = inb ? vi : p.N - 1;
        const float x = (p.P_in[3 * vc] - n0) * inv_s, y = (p.P_in[3 * vc + 1] - n1) * inv_s, z = (p.P_in[3 * vc + 2] - n2) * inv_s;
        const float d2v = p.dist2 ? p.dist2[vc] : 0.f;
        const bool live = inb && !(d2v > p.radius2);
        const bool work = __any(live);
        f32x4 acc[NT][3];
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int d = 0; d < 3; ++d) acc[T][d] = zero4;

        for (int kb0 = 0; kb0 < p.nkb; kb0 += p.kchunk) {
            const int nk = p.nkb - kb0 < p.kchunk ? p.nkb - kb0 : p.kchunk;
            if (!resident) stage(kb0, nk);
            if (!work) continue;
            for (int kb = 0; kb < nk; ++kb) {
                // the basis of this lane's two runs of four records: element 4 a + e of the operand is record
                // 16 (g >> 1) + 4 (g & 1) + 8 a + e of the block
                u32x4 bh[3], bl[3];
                const float4 *cr = s_c + 32 * kb + 16 * (g >> 1) + 4 * (g & 1);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const float4 *run = cr + 8 * a;
                    float b[3][4];
                    float dx = 0.f, dy = 0.f, dz = 0.f, d2 = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float s;
                        if (e % SHARE == 0) {
                            // record e - e % SHARE carries the centre of the SHARE layers that sit side by side
                            const float4 c = run[e];
                            dx = x - c.x; dy = y - c.y; dz = z - c.z;
                            d2 = dx * dx;
                            d2 = __builtin_fmaf(dy, dy, d2);
                            d2 = __builtin_fmaf(dz, dz, d2);
                            s = c.w;
                        } else {
                            s = run[e].w;
                        }
                        // its own multiply, its own exponential
                        float gv = __builtin_amdgcn_exp2f(d2 * s) * s;
                        gv *= (float)(1 << kVmlGradShift);
                        b[0][e] = gv * dx; b[1][e] = gv * dy; b[2][e] = gv * dz;
                        // The fp32 products are made opaque before the split.  Left visible, the compiler narrows the product in
                        // two ways: v_cvt_pk_f16_f32 of the rounded fp32 product for the hi piece it packs, v_fma_mixlo_f16 of the
                        // factors (ONE rounding) for the hi piece it subtracts.  Where the two roundings differ, lo is off by an
                        // ulp of hi, 2^-10 of the term: a few vertices in a thousand 10 to 20 times over the bar.
                        asm("" : "+v"(b[0][e]), "+v"(b[1][e]), "+v"(b[2][e]));
                    }
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        unsigned hh, ll;
                        split_pair_f16<true>(b[d][0], b[d][1], hh, ll); bh[d][2 * a] = hh; bl[d][2 * a] = ll;
                        split_pair_f16<true>(b[d][2], b[d][3], hh, ll); bh[d][2 * a + 1] = hh; bl[d][2 * a + 1] = ll;
                    }
                }
                const uint4 *wk = s_w + (size_t)kb * NT * 128 + lane;
#pragma unroll
                for (int T = 0; T < NT; ++T) {
                    const f16x8 ah = __builtin_bit_cast(f16x8, wk[T * 128]), al = __builtin_bit_cast(f16x8, wk[T * 128 + 64]);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const f16x8 vh = __builtin_bit_cast(f16x8, bh[d]), vl = __builtin_bit_cast(f16x8, bl[d]);
                        acc[T][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, vh, acc[T][d], 0, 0, 0);
                        acc[T][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, vh, acc[T][d], 0, 0, 0);
                        acc[T][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, vl, acc[T][d], 0, 0, 0);
                    }
                }
            }
        }

        // ---- epilogue: lane (g, j) finishes its vertex for the frames whose rows its lane group holds
        if (!inb) continue;
        float fall = 1.f;
        if (p.dist2 != nullptr || !(p.radius2 != 0.f)) {       // fd_eval.hip's fall-off, the same operations
            fall = fminf(d2v / p.radius2, 1.f);
            fall = powf(1.f - fall, p.falloffrate);
        }
        FrameIO<float> io;
        io.tu = p.tu; io.tv = p.tv; io.nrm = p.nrm;
        io.vN = p.vN; io.vtu = p.vtu; io.vtv = p.vtv;
        if (live && p.tu && fall != 0.f) transport::axes(p.tu, p.tv, p.nrm, vi, io.a1, io.a2);
        const float xp[3] = {x, y, z};
        auto frame = [&](int f, float j00, float j01, float j02, float j10, float j11, float j12, float j20, float j21, float j22) {
            if (f >= p.nF) return;
            const float *fc = s_fc + kFrameWords * f;
            io.oN = s_ptr[4 * f]; io.otu = s_ptr[4 * f + 1]; io.otv = s_ptr[4 * f + 2]; io.jac = s_ptr[4 * f + 3];
            if (!live || fc[1] == 0.f) {
                pass_through(io, vi);
                return;
            }
            const float S[9] = {j00, j01, j02, j10, j11, j12, j20, j21, j22};
            float R[9];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float poly = __builtin_fmaf(2.f * fc[11 + c], xp[k], fc[2 + 3 * c + k]);
                    R[3 * c + k] = inv_s * __builtin_fmaf(gs, S[3 * c + k] * fc[0], poly);       // 2^-k 2^-8: exact
                }
            transport::transport<float>(io, vi, R, fall);
        };
        if constexpr (DENSE) {
            // tile 3 B + c: component c of frames 16 B + row; lane group g holds rows 4 g + r
#pragma unroll
            for (int B = 0; B < NT / 3; ++B)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    frame(16 * B + 4 * g + r, acc[3 * B][0][r], acc[3 * B][1][r], acc[3 * B][2][r], acc[3 * B + 1][0][r], acc[3 * B + 1][1][r],
                          acc[3 * B + 1][2][r], acc[3 * B + 2][0][r], acc[3 * B + 2][1][r], acc[3 * B + 2][2][r]);
        } else {
            // tile T: frames 4 T .. 4 T + 3, row 4 (frame - 4 T) + component; lane group g holds frame 4 T + g
#pragma unroll
            for (int T = 0; T < NT; ++T)
                frame(4 * T + g, acc[T][0][0], acc[T][1][0], acc[T][2][0], acc[T][0][1], acc[T][1][1], acc[T][2][1], acc[T][0][2], acc[T][1][2],
                      acc[T][2][2]);
        }
    }
}

}  // namespace

hipError_t launch_vectors_shared_ml(const SharedVectorMlArgs &a, hipStream_t stream)
{
    if (a.N <= 0 || a.nF <= 0) return hipSuccess;
    if (!shared_ml_applies(a.M, a.layers, a.nF) || !a.scratch) return hipErrorInvalidValue;
    const int nrec = a.M * a.layers, nkb = (nrec + 31) / 32;
    const int NT = shot_tiles(a.nF);
    VmlParams p{};
    ShotOut out{};
    fill_shot(p, out, a);
    p.nF = a.nF; p.nkb = nkb; p.srcNT = ml_tiles(a.nF);
    p.scratch = (const uint4 *)a.scratch;
    const size_t fixed = sizeof(float) * kFrameWords * kMaxBatch + sizeof(float *) * 4 * kMaxBatch;
    const size_t per_kb = 32 * 16 + (size_t)NT * 128 * 16;
    p.kchunk = even_chunks(nkb, (int)((kSharedLdsBudget - fixed) / per_kb));       // kmax >= 12: six tiles are 12.5 KiB a block
    ShotGrid gr;
    if (hipError_t e = shot_grid(a, fixed + per_kb * (size_t)p.kchunk, gr); e != hipSuccess) return e;
    return for_tiles(NT, a.nF > 12, [&](auto nt, auto dns) {
        constexpr int kNT = nt.value;
        constexpr bool kDense = dns.value;
        switch (ml_share(a.layers)) {
        case 4: return launch_shot<k_vectors32_shared_ml<kNT, kDense, 4>>(gr, stream, out, p);
        case 2: return launch_shot<k_vectors32_shared_ml<kNT, kDense, 2>>(gr, stream, out, p);
        default: return launch_shot<k_vectors32_shared_ml<kNT, kDense, 1>>(gr, stream, out, p);
        }
    });
}

// The fewest frames at which the one launch is ahead of the per-context k_vectors32_gaussian launches over the M L records,
// measured at 1M vertices and 256 centres with the launch taken at every frame count from two on (DESIGN.md 4.7e,
// profiles/vectors_shared_ml_1M_256_events.csv and ..._small_frames.csv).  At two frames the launch takes 0.295 / 0.444 / 0.650 /
// 0.816 / 1.114 / 1.200 / 1.505 / 1.615 ms with 1..8 layers, the per-context launches 0.295 / 0.486 / 0.725 / 0.901 / 1.209 /
// 1.360 / 1.645 / 1.700 ms: a tie with one layer (1.33x at three frames), 1.05x .. 1.13x with 2..8.
int shared_vectors_ml_min_frames(int layers)
{
    // tuning builds only (fd_tuning.h): FD_VML_MIN_FRAMES=1 lets tools/vectors_shared_ml_profile.py time the launch below the
    // threshold; the product library reads no environment variable
    static const char *force = tuning_env("FD_VML_MIN_FRAMES");
    if (force && atoi(force) >= 1) return atoi(force);
    return layers <= 1 ? 3 : 2;
}

const char *shared_vectors_ml_kernel_name(int M, int layers, int nF)
{
    return shared_ml_applies(M, layers, nF) && nF >= shared_vectors_ml_min_frames(layers) ? "k_vectors32_shared_ml" : "";
}

}  // namespace fd
