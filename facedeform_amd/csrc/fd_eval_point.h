// fd_eval_point.h -- the one-frame evaluation's device helpers for ONE (vertex, centre) pair and ONE vertex's epilogue: the
// kernels phi, the fp64 logarithm, the tangent projection, and gate-to-store (epilogue_store) with the parameters it reads.
// fd_eval.hip's kernels run them, and the three staged shot launches (fd_eval_shared64.hip, fd_eval_shared_ml64.hip,
// fd_eval_shared_ml.hip) finish every frame of a vertex with the same epilogue_store and form phi with the same phi64:
// ONE copy, so "per frame, what the one-frame launch computes" holds by construction.
#pragma once
#include "fd_eval_common.h"

namespace fd {
namespace {

typedef const __attribute__((address_space(4))) Rec32 *ConstRec32;
typedef const __attribute__((address_space(4))) Rec64 *ConstRec64;

struct EvalParams {
    int64_t N;
    const float *P_in;
    float *P_out;
    const float *dist2;
    float *falloff_out;
    const float *tu, *tv, *nrm;
    float radius2, falloffrate;
    int Mpad;
    int delta;             // write the displacement, not P + displacement (fd_set_output); shares Mpad's 8 bytes
    const Rec32 *rec32;
    const Rec64 *rec64;
    const MfmaTile *tiles;
    const MfmaTileH *tiles16;
    const DevModel *model;
};

// ---- kernels phi'(d2) (constant factors live in the packed weights) ----------
template <int KIND>
__device__ __forceinline__ float phi32(float d2, float s)
{
    if constexpr (KIND == FD_KERNEL_THIN_PLATE) {
        return d2 * __builtin_amdgcn_logf(d2);        // d2*log2(d2); d2 carries +1e-37
    } else if constexpr (KIND == FD_KERNEL_GAUSSIAN || KIND == FD_KERNEL_GAUSSIAN_QNN) {
        return __builtin_amdgcn_exp2f(d2 * s);        // s = -log2(e)/R_j^2
    } else if constexpr (KIND == FD_KERNEL_BIHARMONIC) {
        return __builtin_amdgcn_sqrtf(d2);
    } else {
        return d2 * __builtin_amdgcn_sqrtf(d2);
    }
}

// Natural logarithm of a positive, normal double to ~1 ulp-and-a-half without the library's
// table walk: x = m * 2^e with m in [1/sqrt2, sqrt2), ln m = 2 atanh(s), s = (m - 1) / (m + 1),
// |s| <= 0.1716, eleven odd terms (the next one is below 1e-17).  About half the instructions of
// ocml's log; the fp64 evaluation spends most of its time here.
__device__ __forceinline__ double fast_log_pos(double x)
{
    double m = __builtin_amdgcn_frexp_mant(x);               // [0.5, 1)
    int e = __builtin_amdgcn_frexp_exp(x);
    if (m < 0.70710678118654752) { m *= 2.0; e -= 1; }
    const double num = m - 1.0, den = m + 1.0;
    // division by Newton on the hardware reciprocal (den in [1.7, 2.42))
    double r = __builtin_amdgcn_rcp(den);
    r = fma(fma(-den, r, 1.0), r, r);
    r = fma(fma(-den, r, 1.0), r, r);
    double s0 = num * r;
    s0 = fma(fma(-den, s0, num), r, s0);                     // one correction of the quotient
    const double z = s0 * s0;
    double p = 1.0 / 21.0;
    p = fma(p, z, 1.0 / 19.0);
    p = fma(p, z, 1.0 / 17.0);
    p = fma(p, z, 1.0 / 15.0);
    p = fma(p, z, 1.0 / 13.0);
    p = fma(p, z, 1.0 / 11.0);
    p = fma(p, z, 1.0 / 9.0);
    p = fma(p, z, 1.0 / 7.0);
    p = fma(p, z, 1.0 / 5.0);
    p = fma(p, z, 1.0 / 3.0);
    const double lnm = fma(s0 * z, 2.0 * p, 2.0 * s0);       // 2 s (1 + z p)
    return fma((double)e, 0.69314718055994530942, lnm);
}

template <int KIND>
__device__ __forceinline__ double phi64(double d2, double s)
{
    if constexpr (KIND == FD_KERNEL_THIN_PLATE) {
        // d2 is a sum of squares of fp32 differences: zero or >= 2^-298, never subnormal
        return d2 > 0.0 ? d2 * fast_log_pos(d2) : 0.0;       // weights carry the 0.5
    } else if constexpr (KIND == FD_KERNEL_GAUSSIAN || KIND == FD_KERNEL_GAUSSIAN_QNN) {
        return exp(d2 * s);                           // s = -1/R_j^2
    } else if constexpr (KIND == FD_KERNEL_BIHARMONIC) {
        return sqrt(d2);
    } else {
        return d2 * sqrt(d2);
    }
}

// thin-plate only: keeps log2 finite at d2 == 0 (phi -> -1.2e-35, i.e. 0) at no cost,
// because it rides in the first fma of the distance.
template <int KIND>
__device__ __forceinline__ constexpr float d2_bias()
{
    return KIND == FD_KERNEL_THIN_PLATE ? 1e-37f : 0.f;
}

// ---- fp32 epilogue, same operation order as the reference (normalize3: fd_eval_common.h) ----

// reference src/SOP_FaceDeform.hpp:28-41
__device__ __forceinline__ void project_to_tangents(const float u[3], const float v[3],
                                                    const float n[3], float d[3])
{
    float g[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) g[i][j] = u[i] * u[j] + v[i] * v[j] + n[i] * n[j];
    float a1[3], a2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        a1[j] = u[0] * g[0][j] + u[1] * g[1][j] + u[2] * g[2][j];
        a2[j] = v[0] * g[0][j] + v[1] * g[1][j] + v[2] * g[2][j];
    }
    normalize3(a1[0], a1[1], a1[2]);
    normalize3(a2[0], a2[1], a2[2]);
    const float da1 = d[0] * a1[0] + d[1] * a1[1] + d[2] * a1[2];
    const float da2 = d[0] * a2[0] + d[1] * a2[1] + d[2] * a2[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = a1[c] * da1 + a2[c] * da2;
}

// gate (:405-410) is decided by the caller; this is :415-438 for one vertex
__device__ __forceinline__ void epilogue_store(const EvalParams &p, int64_t i, const float pos[3],
                                               float disp[3], float dist2)
{
    if (p.tu) {
        float u[3] = {p.tu[3 * i], p.tu[3 * i + 1], p.tu[3 * i + 2]};
        float v[3] = {p.tv[3 * i], p.tv[3 * i + 1], p.tv[3 * i + 2]};
        float n[3] = {p.nrm[3 * i], p.nrm[3 * i + 1], p.nrm[3 * i + 2]};
        normalize3(u[0], u[1], u[2]);
        normalize3(v[0], v[1], v[2]);
        normalize3(n[0], n[1], n[2]);
        project_to_tangents(u, v, n, disp);
    }
    // :423-424.  Without a dist2 attribute the value is 0: min(0 / r2, 1) = +-0 and pow(1, rate) = 1
    // for every rate (C99), so the library powf -- a few dozen instructions per vertex -- is
    // skipped; r2 == 0 (0/0) keeps the general path.
    float falloff = 1.f;
    if (p.dist2 != nullptr || !(p.radius2 != 0.f)) {
        falloff = fminf(dist2 / p.radius2, 1.f);
        falloff = powf(1.f - falloff, p.falloffrate);
    }
    // non-temporal: a frame's 16 MB of output need not displace what a build running beside the evaluation keeps in L2
    // (measured on the shared-rig launch: +6 % on the whole pipeline)
#ifdef FD_EVAL_TEMPORAL_STORES
    if (p.falloff_out) p.falloff_out[i] = falloff;
    const float b0 = p.delta ? 0.f : pos[0], b1 = p.delta ? 0.f : pos[1], b2 = p.delta ? 0.f : pos[2];
    p.P_out[3 * i] = b0 + disp[0] * falloff;
    p.P_out[3 * i + 1] = b1 + disp[1] * falloff;
    p.P_out[3 * i + 2] = b2 + disp[2] * falloff;
#else
    if (p.falloff_out) __builtin_nontemporal_store(falloff, &p.falloff_out[i]);
    // (FD_OUTPUT_DISPLACEMENT: the addend of :438 alone -- 0 + d f is d f exactly)
    const float b0 = p.delta ? 0.f : pos[0], b1 = p.delta ? 0.f : pos[1], b2 = p.delta ? 0.f : pos[2];
    __builtin_nontemporal_store(b0 + disp[0] * falloff, &p.P_out[3 * i]);
    __builtin_nontemporal_store(b1 + disp[1] * falloff, &p.P_out[3 * i + 1]);
    __builtin_nontemporal_store(b2 + disp[2] * falloff, &p.P_out[3 * i + 2]);
#endif
}

}  // namespace
}  // namespace fd
