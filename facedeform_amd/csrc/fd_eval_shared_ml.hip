// fd_eval_shared_ml.hip -- ALL frames of a shot of MULTILAYER models in one launch (fd_batch_deform_shared_ml_dev;
// DESIGN.md 4.1f).  The solved multilayer model is M x L Gaussian records with radii R / 2^l, laid centre-major by k_pack
// (record c L + l); the rest rig, hence every centre and every radius, is the same for all frames of the shot, so
//     Delta_f(x_v) = poly_f(x_v) + sum_r exp(-|x_v - c_r|^2 / R_r^2) w_f[r]
// is Phi (N x M L) times W (M L x 3 F): phi is formed ONCE per (vertex, record) for all frames and contracted with every
// frame's weights on the fp16 matrix pipe, as k_deform32_tps_shared_wide<GAUSS = true> (fd_eval_shared.hip) does for the
// one-layer kinds: normalised coordinates and direct differences, v_exp_f32 with the 2^10 shift clear of the fp16
// subnormals, both operands as two fp16 pieces (split_pair_f16), three v_mfma_f32_32x32x16_f16 per weight tile (hi x hi,
// lo x hi, hi x lo), fp32 accumulation on top of the polynomial tiles.
//
// What is this file's own:
//   * K runs over RECORDS.  A K block is 32 consecutive centre-major records; in the B operand of the 32 x 32 x 16
//     instruction a lane holds aligned runs of four consecutive records (8 (2 s + a) + 4 h .. + 3 of K step s), which with
//     L in {4, 8} are layers of ONE centre and with L in {2, 6} two pairs of layers of one centre each: d2 is formed once per
//     centre inside a run (SHARE = 4, 2; other L: the largest of {4, 2, 1} that divides L -- the one-frame kernel's rule;
//     SHARE = 1 is the flat Gaussian form).  Every layer has its own multiply and its own v_exp_f32: E_{l+1} = E_l^4
//     would quadruple the relative error per layer.
//   * The model never fits LDS at the sizes that matter (M = 256 x 4 layers x 32 frames: 400 KiB), so it is staged in
//     chunks of K blocks with the accumulators kept live across them: the normal case here.
//   * The epilogue is the one-frame launch's own epilogue_store (fd_eval_point.h): gate, tangent projection, fall-off and
//     the stores are the very code fd_deform_dev runs.
//   * One pack kernel, the only reader of the contexts' models, into scratch of the batch that nothing else uses.
// No floating-point atomics; a vertex's bits depend on its own column of its own matrix instructions only -- not on its
// place in the launch, nor on the number of workgroups.  Built with -ffp-contract=off and -fno-slp-vectorize like
// fd_eval_shared.hip (no packed fp32 arithmetic under in-flight matrix instructions: DESIGN.md 4.1c).
#include <cstdio>
#include <cstdlib>

#include "fd_eval_point.h"
#include "fd_shared_common.h"
#include "fd_shared_ml.h"
#include "fd_shot_launch.h"

namespace fd {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMlWaves = 8;                       // two per SIMD, 64 vertices (two vertex tiles of 32) each per group
constexpr int kMlThreads = 64 * kMlWaves;
static_assert(kMlThreads == kShotThreads, "launch_shot's workgroup");
constexpr int kMlGroup = 64 * kMlWaves;           // vertices per workgroup and group

// (the scratch layout -- kMlNormAt, kMlPolyAt, ml_rec_at, ml_w_at, ml_w16, ml_tiles, ml_share -- and kMlMinFrames are
// fd_shared_ml.h's: the vector launch reads the scratch too)
constexpr int ml_tile_frames(int nt) { return 32 * nt / 3; }           // frames whose three rows fit nt tiles

struct MlPackArgs {
    const Rec32 *rec[kMaxBatch];
    const DevModel *model[kMaxBatch];
    float *P_out[kMaxBatch];
    float *fall[kMaxBatch];
    int nF, nrec;                 // frames; records of a model (M x L)
    int check_rig;                // compare every frame's records {c', scale} with frame 0's (contexts of more than one build)
    int *mismatch;                // page-locked word (device address) or null
};

// grid (nkb, NT), 256 threads.  Workgroup (0, 0) also writes the frame records and the normalisation; every workgroup of
// row tile 0 its K block's records.
__global__ __launch_bounds__(256) void k_pack_shared_ml(const MlPackArgs a, uint4 *scratch)
{
    const int kb = blockIdx.x, T = blockIdx.y, nkb = gridDim.x, NT = gridDim.y;
    const int tid = threadIdx.x;
    if (T == 0 && tid < 32) {
        // {c'x, c'y, c'z, -log2(e) s^2 / R_l^2}: the first half of Rec32.  Padding: zeros -- exp2(0 d2 + 10) is finite and
        // its weights are zero.
        const int r = 32 * kb + tid;
        scratch[ml_rec_at(NT) + (size_t)kb * 32 + tid] =
            r < a.nrec ? *reinterpret_cast<const uint4 *>(&a.rec[0][r]) : make_uint4(0u, 0u, 0u, 0u);
    }
    // per-frame scale: the largest |weight| or |polynomial coefficient| (left in the model by the build's packing code) to
    // [2^13, 2^14); 8 lanes per frame
    __shared__ float s_scale[kMaxBatch];
    {
        const int f = tid >> 3, l = tid & 7;
        bool same = true;
        if (kb == 0 && T == 0 && a.check_rig && f > 0 && f < a.nF && a.rec[f] != a.rec[0]) {
            bool diff = false;
            for (int r = l; r < a.nrec; r += 8) {
                const uint4 x = *reinterpret_cast<const uint4 *>(&a.rec[f][r]), y = *reinterpret_cast<const uint4 *>(&a.rec[0][r]);
                diff |= x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
            }
            same = !diff;
        }
        for (int off = 4; off >= 1; off >>= 1) same = (__shfl_xor((int)same, off) != 0) && same;
        if (l == 0) {
            const float m = f < a.nF ? a.model[f]->wmax32 : 0.f;
            int k = 0;
            if (m > 0.f && m < INFINITY) k = 13 - (__builtin_amdgcn_frexp_expf(m) - 1);
            k = k < -100 ? -100 : (k > 100 ? 100 : k);
            s_scale[f] = ldexpf(1.f, k);
            if (kb == 0 && T == 0) {
                SharedFrame fr;
                fr.inv_scale = ldexpf(1.f, -k - kGaussShift);
                fr.built = (f < a.nF && same && a.model[f]->terminationtype == 1) ? 1 : 0;
                fr.pad[0] = fr.pad[1] = 0;
                fr.P_out = f < a.nF ? a.P_out[f] : nullptr;
                fr.falloff_out = f < a.nF ? a.fall[f] : nullptr;
                reinterpret_cast<SharedFrame *>(scratch)[f] = fr;
                if (!same && a.mismatch) *a.mismatch = f + 1;
            }
        }
        if (kb == 0 && T == 0 && tid == 255) {
            const float *nn = a.model[0]->norm32;
            scratch[kMlNormAt] = make_uint4(__float_as_uint(nn[0]), __float_as_uint(nn[1]), __float_as_uint(nn[2]), __float_as_uint(nn[3]));
        }
    }
    __syncthreads();
    if (tid >= 128) return;
    // A operand of K step s: lane (h, rho) holds row 32 T + rho = component c of frame f, element m = record
    // 32 kb + 8 (2 s + m / 4) + 4 h + m % 4 -- the order the evaluation forms phi in
    const int s = tid >> 6, lane = tid & 63, h = lane >> 5;
    const int row = 32 * T + (lane & 31);
    const int f = row / 3, c = row % 3;
    const bool live = f < a.nF;
    const float sc = live ? s_scale[f] : 0.f;
    f16x8 hi, lo;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int r = 32 * kb + 8 * (2 * s + (m >> 2)) + 4 * h + (m & 3);
        float w = 0.f;
        if (live && r < a.nrec) {
            const Rec32 &q = a.rec[f][r];
            w = (c == 0 ? q.wx : (c == 1 ? q.wy : q.wz)) * sc;
        }
        const _Float16 hh = (_Float16)w;
        hi[m] = hh;
        lo[m] = (_Float16)(w - (float)hh);
    }
    uint4 *dst = scratch + ml_w_at(NT, nkb) + (size_t)kb * ml_w16(NT) + (size_t)((T * 2 + s) * 2) * 64;
    dst[lane] = __builtin_bit_cast(uint4, hi);
    dst[64 + lane] = __builtin_bit_cast(uint4, lo);
    if (kb == 0 && s == 0) {
        // polynomial tile of row tile T, K = 16: coefficients {C0, Lx, Ly, Lz, q} as (hi, lo) against the vertex operand's
        // {1, x, y, z, |x|^2} as (hi, lo) -- lane half 0: hi[0..4] x hi, then hi[1..3] x lo(x, y, z); lane half 1:
        // hi[4] x lo(|x|^2), lo[0..4] x hi, two unused
        f16x8 pt;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int coef = h == 0 ? (m < 5 ? m : m - 4) : (m == 0 ? 4 : (m < 6 ? m - 1 : -1));
            const bool want_lo = h == 1 && m >= 1;
            float w = 0.f;
            if (live && coef >= 0) w = a.model[f]->poly32[5 * c + coef] * sc;
            const _Float16 hh = (_Float16)w;
            pt[m] = want_lo ? (_Float16)(w - (float)hh) : hh;
        }
        scratch[kMlPolyAt + (size_t)T * 64 + lane] = __builtin_bit_cast(uint4, pt);
    }
}

struct MlParams : ShotEvalMesh {
    int nF, nkb, kchunk, delta, Mpad;
    const uint4 *scratch;
};

// NT row tiles of 32 (up to 10, 21, 32 frames); SHARE consecutive records are layers of one centre
template <int NT, int SHARE>
__global__ __launch_bounds__(kMlThreads) __attribute__((amdgpu_waves_per_eu(kMlWaves / 4, kMlWaves / 4)))
void k_deform32_shared_ml(const MlParams p, int ngroups)
{
    constexpr int TV = 2;                         // vertex tiles (of 32) per wave
    constexpr int kW16 = (int)ml_w16(NT);
    constexpr int kFrames = ml_tile_frames(NT) < kMaxBatch ? ml_tile_frames(NT) : kMaxBatch;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [frame records 32][polynomial tiles NT x 64 x 16 B][records kchunk x 32 x 16 B][weight tiles kchunk x NT x 4 KiB]
    const SharedFrame *s_frames = reinterpret_cast<const SharedFrame *>(smem);
    uint4 *s_poly = reinterpret_cast<uint4 *>(smem + sizeof(SharedFrame) * (size_t)kMaxBatch);
    float4 *s_rec = reinterpret_cast<float4 *>(s_poly + NT * 64);
    uint4 *s_w = reinterpret_cast<uint4 *>(s_rec + (size_t)32 * p.kchunk);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, j = lane & 31;
    const float4 nrm4 = *reinterpret_cast<const float4 *>(p.scratch + kMlNormAt);
    const float n0 = nrm4.x, n1 = nrm4.y, n2 = nrm4.z, inv_s = nrm4.w;
    const bool resident = p.nkb <= p.kchunk;
    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;

    // K blocks kb0 .. kb0 + nk - 1 of the model into LDS (four loads in flight per thread)
    auto copy16 = [&](u32x4 *dst, const u32x4 *src, int n16) {
        int q = tid;
        for (; q + 3 * kMlThreads < n16; q += 4 * kMlThreads) {
            const u32x4 v0 = src[q], v1 = src[q + kMlThreads], v2 = src[q + 2 * kMlThreads], v3 = src[q + 3 * kMlThreads];
            dst[q] = v0; dst[q + kMlThreads] = v1; dst[q + 2 * kMlThreads] = v2; dst[q + 3 * kMlThreads] = v3;
        }
        for (; q < n16; q += kMlThreads) dst[q] = src[q];
    };
    auto stage = [&](int kb0, int nk) {
        __syncthreads();
        copy16(reinterpret_cast<u32x4 *>(s_rec), reinterpret_cast<const u32x4 *>(p.scratch + ml_rec_at(NT)) + (size_t)kb0 * 32, nk * 32);
        copy16(reinterpret_cast<u32x4 *>(s_w), reinterpret_cast<const u32x4 *>(p.scratch + ml_w_at(NT, p.nkb)) + (size_t)kb0 * kW16, nk * kW16);
        __syncthreads();
    };
    // frame records and polynomial tiles: contiguous at the head of the scratch but for the normalisation word
    copy16(reinterpret_cast<u32x4 *>(smem), reinterpret_cast<const u32x4 *>(p.scratch), (int)kMlNormAt);
    copy16(reinterpret_cast<u32x4 *>(s_poly), reinterpret_cast<const u32x4 *>(p.scratch + kMlPolyAt), NT * 64);
    if (resident) stage(0, p.nkb);
    else __syncthreads();

    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        // lane (h, j) holds the two vertices (t, j) -- both lane halves the same two
        const int64_t vbase = ((int64_t)grp * kMlWaves + wave) * 64;
        float pin[TV][3], d2in[TV], xn[TV], yn[TV], zn[TV];
        f32x16 acc[NT][TV];
        bool lane_live = false;
#pragma unroll
        for (int t = 0; t < TV; ++t) {
            const int64_t vi = vbase + 32 * t + j;
            const int64_t vc = vi < p.N ? vi : p.N - 1;
            pin[t][0] = p.P_in[3 * vc]; pin[t][1] = p.P_in[3 * vc + 1]; pin[t][2] = p.P_in[3 * vc + 2];
            d2in[t] = p.dist2 ? p.dist2[vc] : 0.f;
            lane_live |= (vi < p.N) && !(d2in[t] > p.radius2);
            const float x = (pin[t][0] - n0) * inv_s, y = (pin[t][1] - n1) * inv_s, z = (pin[t][2] - n2) * inv_s;
            xn[t] = x; yn[t] = y; zn[t] = z;
            const float xx = __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x));
            // polynomial operand, K = 16 (k_pack_shared_ml): half 0 {1, xh, yh, zh, xxh, xl, yl, zl}, half 1
            // {xxl, 1, xh, yh, zh, xxh, 0, 0}; everything times 2^10, the factor phi carries (undone with the frame's scale)
            constexpr float ps = (float)(1 << kGaussShift);
            constexpr unsigned one16 = 0x6400u;          // fp16 1024
            unsigned xyh, xyl, zxh, zxl;
            split_pair_f16(x * ps, y * ps, xyh, xyl);
            split_pair_f16(z * ps, xx * ps, zxh, zxl);
            u32x4 pb;
            if (h == 0) pb = (u32x4){one16 | (xyh << 16), (xyh >> 16) | (zxh << 16), (zxh >> 16) | (xyl << 16), (xyl >> 16) | (zxl << 16)};
            else pb = (u32x4){(zxl >> 16) | (one16 << 16), xyh, zxh, 0u};
            const f16x8 pbv = __builtin_bit_cast(f16x8, pb);
#pragma unroll
            for (int c = 0; c < NT; ++c)
                acc[c][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, s_poly[c * 64 + lane]), pbv, zero16, 0, 0, 0);
        }
        const bool wave_work = __any(lane_live);

        // phi of K step s of block kb for the wave's two vertex tiles, split into fp16 pieces: the B operands.  This lane's
        // records of the step are the two runs 8 (2 s + a) + 4 h .. + 3, a = 0, 1.
        auto phi_half = [&](int kb, int s, u32x4 (&xh)[TV], u32x4 (&xl)[TV]) {
            const float4 *cr = s_rec + (size_t)kb * 32 + 4 * h;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float4 *run = cr + 8 * (2 * s + a);
                // centre of record e of the run: record e - e % SHARE carries it (the layers of a centre sit side by side)
                float4 cen[4];
                float sc[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e % SHARE == 0) cen[e] = run[e];
                    sc[e] = e % SHARE == 0 ? cen[e].w : run[e].w;
                }
#pragma unroll
                for (int t = 0; t < TV; ++t) {
                    float ph[4], d2 = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (e % SHARE == 0) {
                            // ONE value per instruction (no packed arithmetic under in-flight matrix instructions)
                            const float dx = xn[t] - cen[e].x, dy = yn[t] - cen[e].y, dz = zn[t] - cen[e].z;
                            d2 = dx * dx;
                            d2 = __builtin_fmaf(dy, dy, d2);
                            d2 = __builtin_fmaf(dz, dz, d2);
                        }
                        ph[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(d2, sc[e], (float)kGaussShift));
                    }
                    unsigned hh, ll;
                    split_pair_f16<true>(ph[0], ph[1], hh, ll); xh[t][2 * a] = hh; xl[t][2 * a] = ll;
                    split_pair_f16<true>(ph[2], ph[3], hh, ll); xh[t][2 * a + 1] = hh; xl[t][2 * a + 1] = ll;
                }
            }
        };
        auto contract_half = [&](int kb, int s, const u32x4 (&xh)[TV], const u32x4 (&xl)[TV]) {
            const uint4 *wk = s_w + (size_t)kb * kW16 + lane;
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const f16x8 ah = __builtin_bit_cast(f16x8, wk[((c * 2 + s) * 2) * 64]), al = __builtin_bit_cast(f16x8, wk[((c * 2 + s) * 2 + 1) * 64]);
#pragma unroll
                for (int t = 0; t < TV; ++t) acc[c][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, xh[t]), acc[c][t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < TV; ++t) acc[c][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, __builtin_bit_cast(f16x8, xh[t]), acc[c][t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < TV; ++t) acc[c][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(f16x8, xl[t]), acc[c][t], 0, 0, 0);
            }
        };
        for (int kb0 = 0; kb0 < p.nkb; kb0 += p.kchunk) {
            const int nk = p.nkb - kb0 < p.kchunk ? p.nkb - kb0 : p.kchunk;
            if (!resident) stage(kb0, nk);
            if (!wave_work) continue;
            // skewed by one K step: the vector unit forms the operands of the next step while the matrix pipe contracts this one
            u32x4 b0h[TV], b0l[TV], b1h[TV], b1l[TV];
            phi_half(0, 0, b0h, b0l);
            for (int kb = 0; kb + 1 < nk; ++kb) {
                phi_half(kb, 1, b1h, b1l);
                contract_half(kb, 0, b0h, b0l);
                phi_half(kb + 1, 0, b0h, b0l);
                contract_half(kb, 1, b1h, b1l);
            }
            phi_half(nk - 1, 1, b1h, b1l);
            contract_half(nk - 1, 0, b0h, b0l);
            contract_half(nk - 1, 1, b1h, b1l);
        }

        // ---- epilogue.  Register r of acc[T][vt] holds row 8 (r / 4) + 4 h + r % 4 of row tile T for vertex (vt, j); swapping
        // the upper half of vertex tile 0's register with the lower half of vertex tile 1's leaves every lane with its OWN
        // vertex (vbase + lane): acc[T][0][r] = row 8 (r / 4) + r % 4, acc[T][1][r] = row 8 (r / 4) + 4 + r % 4.
#pragma unroll
        for (int c = 0; c < NT; ++c) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const u32x2 sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[c][0][r]), __float_as_uint(acc[c][1][r]), false, false);
                acc[c][0][r] = __uint_as_float(sw[0]); acc[c][1][r] = __uint_as_float(sw[1]);
            }
        }
        const int64_t i = vbase + lane;
        if (i >= p.N) continue;                  // (no barrier below: a resident model's loop has none, a staged one's are above)
        const float pos[3] = {h ? pin[1][0] : pin[0][0], h ? pin[1][1] : pin[0][1], h ? pin[1][2] : pin[0][2]};
        const float own_d2 = h ? d2in[1] : d2in[0];
        const bool gated = own_d2 > p.radius2;
        auto row_of = [&](int f, int c) -> float {
            const int row = 3 * f + c, T = row / 32, rho = row % 32;
            return acc[T][(rho % 8) / 4][4 * (rho / 8) + rho % 4];
        };
#pragma unroll
        for (int f = 0; f < kFrames; ++f) {
            if (f >= p.nF) continue;          // (not break: the loop stays fully unrolled, the accumulator indices compile-time)
            const SharedFrame fr = s_frames[f];
            if (gated || !fr.built) {
                // a gated vertex, a frame whose model is not built: the position passes through (as a displacement: zero)
                // and no fd_falloff entry is written
                Pos3 FD_GLOBAL *dstP = (Pos3 FD_GLOBAL *)as_global(fr.P_out) + i;
                if (p.delta) store_pos3(dstP, 0.f, 0.f, 0.f);
                else if (fr.P_out != p.P_in) store_pos3(dstP, pos[0], pos[1], pos[2]);
                continue;
            }
            const EvalParams ep = shot_eval_params(p, fr.P_out, fr.falloff_out, p.Mpad, p.delta);
            float disp[3] = {row_of(f, 0) * fr.inv_scale, row_of(f, 1) * fr.inv_scale, row_of(f, 2) * fr.inv_scale};    // 2^-k is exact
            epilogue_store(ep, i, pos, disp, own_d2);
        }
    }
}

template <int NT>
hipError_t launch_ml_share(const MlParams &p, int share, const ShotGrid &gr, hipStream_t stream)
{
    if (share == 4) return launch_shot<k_deform32_shared_ml<NT, 4>>(gr, stream, p);
    if (share == 2) return launch_shot<k_deform32_shared_ml<NT, 2>>(gr, stream, p);
    return launch_shot<k_deform32_shared_ml<NT, 1>>(gr, stream, p);
}

}  // namespace

bool shared_ml_applies(int M, int layers, int nF)
{
    return M > 0 && layers >= 1 && layers <= kMaxLayers && nF >= kMlMinFrames && nF <= kMaxBatch;
}

int shared_ml_min_frames() { return kMlMinFrames; }

size_t shared_ml_scratch_bytes(int M, int layers, int nF)
{
    const int nkb = (M * layers + 31) / 32, NT = ml_tiles(nF);
    return 16 * (ml_w_at(NT, nkb) + (size_t)nkb * ml_w16(NT));
}

const char *shared_ml_kernel_name(int M, int layers, int nF)
{
    return shared_ml_applies(M, layers, nF) ? "k_deform32_shared_ml" : "";
}

hipError_t launch_deform_shared_ml(const SharedMlArgs &a, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    if (!shared_ml_applies(a.M, a.layers, a.nF) || !a.scratch) return hipErrorInvalidValue;
    const int nrec = a.M * a.layers, nkb = (nrec + 31) / 32, NT = ml_tiles(a.nF);

    MlPackArgs pa{};
    fill_pack(pa, a, a.rec32);
    pa.nF = a.nF; pa.nrec = nrec; pa.check_rig = a.check_rig; pa.mismatch = a.mismatch;
    hipLaunchKernelGGL(k_pack_shared_ml, dim3(nkb, NT), dim3(256), 0, stream, pa, (uint4 *)a.scratch);
    if (hipError_t e = shot_packed(a, stream); e != hipSuccess) return e;

    MlParams p{};
    fill_eval_mesh(p, a);
    p.nF = a.nF; p.nkb = nkb; p.delta = a.delta_out; p.Mpad = round_up(nrec, kRecPad);
    p.scratch = (const uint4 *)a.scratch;
    const size_t fixed = sizeof(SharedFrame) * (size_t)kMaxBatch + (size_t)NT * 64 * 16;
    const size_t per_kb = 32 * 16 + ml_w16(NT) * 16;
    p.kchunk = even_chunks(nkb, (int)((kSharedLdsBudget - fixed) / per_kb));
    ShotGrid gr;          // one persistent workgroup per CU (two 256-register waves per SIMD)
    if (hipError_t e = shot_grid(a.N, kMlGroup, a.max_wgs, fixed + per_kb * (size_t)p.kchunk, 1, gr); e != hipSuccess) return e;
    const int share = ml_share(a.layers);
    if (NT == 1) return launch_ml_share<1>(p, share, gr, stream);
    if (NT == 2) return launch_ml_share<2>(p, share, gr, stream);
    return launch_ml_share<3>(p, share, gr, stream);
}

}  // namespace fd
