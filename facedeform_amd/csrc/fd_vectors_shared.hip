// fd_vectors_shared.hip -- the Jacobian and the vectors it carries for ALL frames of a shot in one launch
// (fd_batch_deform_vectors_shared_dev).  The frames share the mesh and the rest rig, so the gradient
// basis g_j(x) (x - c_j) is formed once per (vertex, centre) and contracted with every frame's weights on the matrix pipe:
//     J_f(x) = sum_j w_f[j] (x) grad phi_j(x) + L_f(x),
// three (N x M) x (M x 3F) products, one per direction of the gradient, against the weight tiles launch_deform_shared's
// pack kernel left in the batch's scratch.  The transport itself (Pi, fall-off, A, cofactors, rescale) is fd_transport.h,
// the one-frame launch's own code.
//
// Inputs: the scratch set only (weight tiles in whichever of the four layouts the position launch packed, their frame
// records, the polynomial tiles, the rest rig's centre copy and normalisation), the mesh and the vectors -- nothing of
// the contexts, so fd_batch_wait_consumed covers this launch as it does the position launch.
//
// Layout: a workgroup of 8 waves keeps the model (or a chunk of K blocks) in LDS, re-dealt into the 16-row tile order of
// k_deform32_tps_shared (padded up to 12 frames, dense from 13: fd_eval_shared.hip) whatever order the pack kernel wrote;
// a wave owns 16 vertices (one vertex tile) at a time.  Per K block of 32 centres a lane forms the basis of its 8 centres
// for its vertex -- direct coordinate differences, one transcendental, three products -- splits the three directions into
// fp16 pieces (hi + lo) and issues 3 directions x 3 split products per output tile on v_mfma_f32_16x16x32_f16.  The
// accumulator of tile T, direction d holds in lane group g rows 4 g .. 4 g + 3 for the lane's vertex: in either row
// layout that is all three components of whole frames, so every lane finishes its frames with no exchange between lanes.
// Built with -ffp-contract=off like the rest: every fused multiply-add is written out.
#include <algorithm>

#include "fd_eval_common.h"
#include "fd_pack.h"
#include "fd_shared_plan.h"
#include "fd_vectors_shot.h"

namespace fd {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr size_t kVsLdsBudget = 158 * 1024;
// The basis enters the matrix pipe pre-scaled by a power of two per kind, so that its fp16 pieces stay clear of the subnormals
// where it matters and the hi piece below the fp16 maximum (65504) over the range the kind can reach:
//   thin-plate 2^4: |2^4 (log2 d2' + log2 e) (x' - c')| < 65504 up to |x' - c'| ~ 235 rig radii (normalised units) -- past the
//     ~70 at which the position launch's own fp16 phi (d2' log2 d2', unscaled) overflows, so every vertex it deforms finitely gets finite
//     vectors; lo pieces are exact down to |g (x - c)| ~ 2^-7, below that their error is 2^-29 absolute;
//   Gaussian kinds 2^8: |g (x - c)| <= 0.52 sqrt(|s_j|) (s_j = -log2(e) / R_j'^2), finite for R_j' above ~0.0024 rig radii
//     (include/facedeform_hip.h states it); lo pieces exact down to 2^-11.
constexpr int grad_shift(bool gauss) { return gauss ? 8 : 4; }

struct VsParams : ShotMesh {
    int nF, nkb, kchunk;
    int layout, srcNT;                   // SharedPlan::variant, ntiles
    unsigned poly_at, copy_at, norm_at;
    const uint4 *wtiles;
    const unsigned *frames;              // the pack kernel's frame records, 8 words each: {inv_scale, built, ...}
};

// lane row (r of 32) and row tile of component c of frame f in the 32-row layouts (k_pack_shared_wide)
__device__ __forceinline__ void wide_row(int layout, int f, int c, int &T, int &r)
{
    if (layout == 2) {
        const int row = 3 * f + c;
        T = row / 32; r = row % 32;
    } else {
        const int k = 3 * (f >> 1) + c, kk = k % 16;
        T = k / 16; r = 8 * (kk >> 2) + 4 * (f & 1) + (kk & 3);
    }
}

// row tile and lane row (of 16) of component c of frame f in the 16-row layouts (k_pack_shared)
template <bool DENSE>
__device__ __forceinline__ void narrow_row(int f, int c, int &T, int &rho)
{
    if (DENSE) { T = 3 * (f / 16) + c; rho = f % 16; }
    else { T = f / 4; rho = 4 * (f % 4) + c; }
}

template <bool GAUSS, int NT, bool DENSE>
__device__ __forceinline__ void vectors_shared_body(const VsParams &p, int ngroups)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [frame constants 32 x 16 words][output pointers 32 x 4][centre records kchunk x 32 x 16 B][weight tiles kchunk x NT x 2 KiB]
    float *s_fc = reinterpret_cast<float *>(smem);
    float **s_ptr = reinterpret_cast<float **>(smem + sizeof(float) * kFrameWords * kMaxBatch);
    float4 *s_c = reinterpret_cast<float4 *>(smem + sizeof(float) * kFrameWords * kMaxBatch + sizeof(float *) * 4 * kMaxBatch);
    uint4 *s_w = reinterpret_cast<uint4 *>(s_c + 32 * p.kchunk);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    const float *nrm4 = reinterpret_cast<const float *>(p.wtiles + p.norm_at);
    const float n0 = nrm4[0], n1 = nrm4[1], n2 = nrm4[2], inv_s = nrm4[3];
    const bool wide = p.layout >= 2;

    // frame constants: the basis scale 2^-k 2^-grad_shift and the frame's linear part {L', q} (hi + lo of the polynomial
    // tile: exact in fp32, the 22 bits the position launch uses), 2^-k undone
    if (tid < p.nF) {
        const int f = tid;
        const float inv = __uint_as_float(p.frames[8 * f]);
        const float unscale = GAUSS ? inv * (float)(1 << kGaussShift) : inv;         // 2^-k
        float *fc = s_fc + kFrameWords * f;
        fc[0] = unscale * (1.f / (float)(1 << grad_shift(GAUSS)));
        fc[1] = p.frames[8 * f + 1] != 0u ? 1.f : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float coef[5];
            if (!wide) {
                int T, rho;
                narrow_row<DENSE>(f, c, T, rho);
                const size_t w = p.poly_at + (size_t)T * 64;
#pragma unroll
                for (int e = 0; e < 5; ++e) coef[e] = (half_at(p.wtiles, w + rho, e) + half_at(p.wtiles, w + 32 + rho, e)) * unscale;
            } else {
                int T, r;
                wide_row(p.layout, f, c, T, r);
                const size_t w = p.poly_at + (size_t)T * 64;
#pragma unroll
                for (int e = 0; e < 5; ++e) coef[e] = (half_at(p.wtiles, w + r, e) + half_at(p.wtiles, w + 32 + r, e + 1)) * unscale;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) fc[2 + 3 * c + k] = coef[1 + k];
            fc[11 + c] = coef[4];
        }
    }
    deal_out_pointers(s_ptr, p.nF);
    // the model's K blocks kb0 .. kb0 + nk - 1 into LDS, in the 16-row order (above)
    auto stage = [&](int kb0, int nk) {
        __syncthreads();
        for (int q = tid; q < nk * 32; q += kShotThreads) {
            const int kb = kb0 + q / 32, m = q % 32;
            float4 c;
            if (GAUSS) {
                // {c'x, c'y, c'z, s}: the first half of Rec32, as the pack kernel copied it
                const size_t w = wide ? p.copy_at + (size_t)kb * 64 + m : p.copy_at + (size_t)2 * kb * (sizeof(MfmaTileH) / 16) + m;
                c = *reinterpret_cast<const float4 *>(p.wtiles + w);
            } else {
                // thin-plate: the centre tiles' fp16 pieces (hi + lo, exact in fp32: what the position launch's d2 uses)
                float cc[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const unsigned *u;
                    if (p.layout <= 1) {
                        u = reinterpret_cast<const unsigned *>(p.wtiles + p.copy_at + (size_t)(2 * kb + (m >> 4)) * (sizeof(MfmaTileH) / 16)) + 2 * (16 * d + (m & 15));
                    } else if (p.layout == 2) {
                        u = reinterpret_cast<const unsigned *>(p.wtiles + p.copy_at) + 2 * ((size_t)kb * 128 + (d >> 1) * 64 + 32 * (d & 1) + m);
                    } else {
                        u = reinterpret_cast<const unsigned *>(p.wtiles + p.copy_at + (size_t)kb * 64 + 32 * (d >> 1) + m) + 2 * (d & 1);
                    }
                    cc[d] = (float)__builtin_bit_cast(_Float16, (unsigned short)(u[0] & 0xffffu)) +
                            (float)__builtin_bit_cast(_Float16, (unsigned short)(u[1] & 0xffffu));
                }
                c = make_float4(cc[0], cc[1], cc[2], 0.f);
            }
            s_c[q] = c;
        }
        for (int q = tid; q < nk * NT * 128; q += kShotThreads) {
            const int kb = kb0 + q / (NT * 128), rem = q % (NT * 128);
            const int T = rem / 128, hl = (rem >> 6) & 1, ln = rem & 63;
            if (!wide) {
                s_w[q] = p.wtiles[((size_t)kb * NT + T) * 128 + rem % 128];      // the same layout (NT, DENSE from nF alike)
                continue;
            }
            const int gg = ln >> 4, rho = ln & 15;
            const int f = DENSE ? 16 * (T / 3) + rho : 4 * T + (rho >> 2), c = DENSE ? T % 3 : rho & 3;
            unsigned short e16[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                unsigned short v = 0;
                if (f < p.nF && c < 3) {
                    const int m = 16 * (s >> 2) + 4 * gg + (s & 3);           // centre of k-slot 8 gg + s
                    const int ks = m >> 4, e = 4 * ((m >> 3) & 1) + (m & 3), h = (m >> 2) & 1;
                    int Ts, r;
                    wide_row(p.layout, f, c, Ts, r);
                    const size_t w = (size_t)kb * p.srcNT * 256 + (size_t)((Ts * 2 + ks) * 2 + hl) * 64 + 32 * h + r;
                    v = reinterpret_cast<const unsigned short *>(p.wtiles + w)[e];
                }
                e16[s] = v;
            }
            s_w[q] = make_uint4(e16[0] | ((unsigned)e16[1] << 16), e16[2] | ((unsigned)e16[3] << 16), e16[4] | ((unsigned)e16[5] << 16),
                                e16[6] | ((unsigned)e16[7] << 16));
        }
        __syncthreads();
    };
    const bool resident = p.nkb <= p.kchunk;
    if (resident) stage(0, p.nkb);
    else __syncthreads();

    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float gs = packing::grad_scale32(GAUSS ? FD_KERNEL_GAUSSIAN : FD_KERNEL_THIN_PLATE);
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
                // the basis of this lane's 8 centres (k-slot 8 g + s = centre 16 (s >> 2) + 4 g + (s & 3) of the block)
                u32x4 bh[3], bl[3];
                const float4 *cr = s_c + 32 * kb;
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) {
                    float b[3][2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int s = 2 * s2 + u;
                        const float4 c = cr[16 * (s >> 2) + 4 * g + (s & 3)];
                        const float dx = x - c.x, dy = y - c.y, dz = z - c.z;
                        float gv;
                        if (GAUSS) {
                            float d2 = dx * dx;
                            d2 = __builtin_fmaf(dy, dy, d2);
                            d2 = __builtin_fmaf(dz, dz, d2);
                            gv = __builtin_amdgcn_exp2f(d2 * c.w) * c.w;
                        } else {
                            // + 1e-37 as in the one-frame kernels: the log stays finite, x - c = 0 gives 0
                            float d2 = __builtin_fmaf(dx, dx, 1e-37f);
                            d2 = __builtin_fmaf(dy, dy, d2);
                            d2 = __builtin_fmaf(dz, dz, d2);
                            gv = __builtin_amdgcn_logf(d2) + packing::kTpsGradLog2e;
                        }
                        gv *= (float)(1 << grad_shift(GAUSS));
                        b[0][u] = gv * dx; b[1][u] = gv * dy; b[2][u] = gv * dz;
                    }
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const _Float16 h0 = (_Float16)b[d][0], h1 = (_Float16)b[d][1];
                        const _Float16 l0 = (_Float16)(b[d][0] - (float)h0), l1 = (_Float16)(b[d][1] - (float)h1);
                        bh[d][s2] = __builtin_bit_cast(unsigned, (f16x2){h0, h1});
                        bl[d][s2] = __builtin_bit_cast(unsigned, (f16x2){l0, l1});
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
                    R[3 * c + k] = inv_s * __builtin_fmaf(gs, S[3 * c + k] * fc[0], poly);
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

// stable names for profiles: k_vectors32_shared_<kind> (the Gaussian kinds share one)
template <int NT, bool DENSE>
__global__ __launch_bounds__(kShotThreads) void k_vectors32_shared_thin_plate(const ShotOut out, const VsParams p, int ngroups)
{
    (void)out;
    vectors_shared_body<false, NT, DENSE>(p, ngroups);
}
template <int NT, bool DENSE>
__global__ __launch_bounds__(kShotThreads) void k_vectors32_shared_gaussian(const ShotOut out, const VsParams p, int ngroups)
{
    (void)out;
    vectors_shared_body<true, NT, DENSE>(p, ngroups);
}

}  // namespace

hipError_t launch_vectors_shared(const SharedVectorArgs &a, hipStream_t stream)
{
    if (a.N <= 0 || a.nF <= 0) return hipSuccess;
    if (a.nF > kMaxBatch || a.Mpad % 16 != 0) return hipErrorInvalidValue;
    const SharedPlan pk = shared_plan(a.Mpad, a.nF, a.kind);      // of the position launch that packed the scratch
    const int nkb = pk.nkb;
    const int NT = shot_tiles(a.nF);
    VsParams p{};
    ShotOut out{};
    fill_shot(p, out, a);
    p.nF = a.nF; p.nkb = nkb;
    p.layout = pk.variant; p.srcNT = pk.ntiles;
    p.poly_at = (unsigned)pk.poly_at; p.copy_at = (unsigned)pk.copy_at; p.norm_at = (unsigned)pk.norm_at;
    p.wtiles = (const uint4 *)a.wtiles; p.frames = (const unsigned *)a.frames;
    const size_t fixed = sizeof(float) * kFrameWords * kMaxBatch + sizeof(float *) * 4 * kMaxBatch;
    const size_t per_kb = 32 * 16 + (size_t)NT * 128 * 16;
    int kchunk = (int)((kVsLdsBudget - fixed) / per_kb);
    if (kchunk < 1) return hipErrorInvalidValue;
    if (kchunk > nkb) kchunk = nkb;
    p.kchunk = kchunk;
    ShotGrid gr;
    if (hipError_t e = shot_grid(a, fixed + per_kb * (size_t)kchunk, gr); e != hipSuccess) return e;
    const bool gauss = a.kind != FD_KERNEL_THIN_PLATE;
    return for_tiles(NT, a.nF > 12, [&](auto nt, auto dns) {
        return gauss ? launch_shot<k_vectors32_shared_gaussian<nt.value, dns.value>>(gr, stream, out, p)
                     : launch_shot<k_vectors32_shared_thin_plate<nt.value, dns.value>>(gr, stream, out, p);
    });
}

const char *shared_vectors_kernel_name(int Mpad, int nF, int kind)
{
    (void)Mpad; (void)nF;
    return kind == FD_KERNEL_THIN_PLATE ? "k_vectors32_shared_thin_plate" : "k_vectors32_shared_gaussian";
}

}  // namespace fd
