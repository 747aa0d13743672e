// fd_vectors.hip -- the Jacobian of the deformation and the normals / tangents it carries (fd_deform_vectors*).
//
// A = I + f Pi J(x) per vertex (include/facedeform_hip.h states the definition); t' = A t, n' = cof(A) n rescaled to |n|.
// A launch of its own beside the deformation kernel: P_out and falloff_out stay exactly fd_deform's, whichever variant
// that picks.
//
// Mapping to the hardware: fd_eval.hip's VALU structure.  The 32 B records are wave-uniform and come through the scalar
// unit; x - c is formed directly (not |x|^2 - 2 x.c + |c|^2); the fp32 kernel holds two vertices per lane
// in one register pair (v_pk_* arithmetic) and folds its nine fp32 partial sums per vertex into fp64 every 64 centres.
// Per (vertex, centre) pair: 3 sub, 3 fma (d2), one transcendental, 1-2 for g, 3 mul (w g), 9 fma.
// Built with -ffp-contract=off like fd_eval.hip: every fused multiply-add is written out.
#include "fd_eval_common.h"
#include "fd_operator.h"

namespace fd {

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 64;   // centres per fp32 partial sum

using packing::grad_scale32;
using packing::grad_scale64;
using packing::grad64;
using packing::kTpsGradLog2e;

typedef const __attribute__((address_space(4))) Rec32 *ConstRec32;
typedef const __attribute__((address_space(4))) Rec64 *ConstRec64;

struct VecParams {
    int64_t N;
    const float *P_in, *dist2;
    const float *tu, *tv, *nrm;          // projection frames (all or none)
    const float *vN, *vtu, *vtv;         // vectors to transport
    float *oN, *otu, *otv, *jac;
    float radius2, falloffrate;
    int Mpad;
    const Rec32 *rec32;
    const Rec64 *rec64;
    const DevModel *model;
    static constexpr bool kGivenAxes = false;      // (fd_transport.h: the axes are formed per vertex there)
    static __device__ __forceinline__ void store(float *dst, float v) { *dst = v; }
};

// g of fd_pack.h's derivative table: grad phi'_j = g_j (x - c_j), the kind's scale applied once per vertex
template <int KIND>
__device__ __forceinline__ f32x2 grad32(f32x2 d2, float s)
{
    if constexpr (KIND == FD_KERNEL_THIN_PLATE) {
        // d2 carries +1e-37 (as in fd_eval.hip): the log stays finite and x - c = 0 gives 0
        const f32x2 l = {__builtin_amdgcn_logf(d2.x), __builtin_amdgcn_logf(d2.y)};
        return l + kTpsGradLog2e;
    } else if constexpr (KIND == FD_KERNEL_GAUSSIAN || KIND == FD_KERNEL_GAUSSIAN_QNN) {
        const f32x2 e = d2 * s;
        return (f32x2){__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)} * s;
    } else if constexpr (KIND == FD_KERNEL_BIHARMONIC) {
        return (f32x2){d2.x > 0.f ? __builtin_amdgcn_rsqf(d2.x) : 0.f, d2.y > 0.f ? __builtin_amdgcn_rsqf(d2.y) : 0.f};
    } else {
        return (f32x2){__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)};
    }
}

__device__ __forceinline__ f32x2 pfma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// the transport epilogue: fd_transport.h
using transport::transport;

// gated vertex / unbuilt model: the vectors bit for bit, A = I
__device__ __forceinline__ void pass_through(const VecParams &p, int64_t i)
{
    if (p.vN && p.oN != p.vN)
        for (int c = 0; c < 3; ++c) p.oN[3 * i + c] = p.vN[3 * i + c];
    if (p.vtu && p.otu != p.vtu)
        for (int c = 0; c < 3; ++c) p.otu[3 * i + c] = p.vtu[3 * i + c];
    if (p.vtv && p.otv != p.vtv)
        for (int c = 0; c < 3; ++c) p.otv[3 * i + c] = p.vtv[3 * i + c];
    if (p.jac)
#pragma unroll
        for (int q = 0; q < 9; ++q) p.jac[9 * i + q] = (q % 4 == 0) ? 1.f : 0.f;
}

// transport::falloff's operations (fd_transport.h), kept here as text: called through that function k_vectors64_thin_plate
// measured above the range of the form with this text
__device__ __forceinline__ float falloff_of(const VecParams &p, float dist2)
{
    float falloff = 1.f;
    if (p.dist2 != nullptr || !(p.radius2 != 0.f)) {
        falloff = fminf(dist2 / p.radius2, 1.f);
        falloff = powf(1.f - falloff, p.falloffrate);
    }
    return falloff;
}

// ---- fp32: two vertices per lane (one f32x2 register per quantity), normalised coordinates ------------------------
template <int KIND>
__device__ __forceinline__ void vectors32_body(const VecParams &p)
{
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * 2);
    const float nx = p.model->norm32[0], ny = p.model->norm32[1], nz = p.model->norm32[2];
    const float inv_s = p.model->norm32[3];
    f32x2 px, py, pz;
    float d2v[2];
    bool live[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int64_t i = base + v * kBlock + tid;
        const int64_t ic = i < p.N ? i : p.N - 1;
        px[v] = (p.P_in[3 * ic] - nx) * inv_s;
        py[v] = (p.P_in[3 * ic + 1] - ny) * inv_s;
        pz[v] = (p.P_in[3 * ic + 2] - nz) * inv_s;
        d2v[v] = p.dist2 ? p.dist2[ic] : 0.f;
        live[v] = (i < p.N) && !(d2v[v] > p.radius2);
    }
    const bool built = p.model->terminationtype == 1;
    double S[2][9];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int q = 0; q < 9; ++q) S[v][q] = 0.0;

    if (__any(live[0] || live[1]) && built) {
        const f32x2 bias = {KIND == FD_KERNEL_THIN_PLATE ? 1e-37f : 0.f, KIND == FD_KERNEL_THIN_PLATE ? 1e-37f : 0.f};
        for (int j0 = 0; j0 < p.Mpad; j0 += kChunk) {
            const int j1 = j0 + kChunk < p.Mpad ? j0 + kChunk : p.Mpad;
            f32x2 a[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) a[q] = (f32x2){0.f, 0.f};
#pragma unroll 2
            for (int j = j0; j < j1; ++j) {
                ConstRec32 r = (ConstRec32)(uintptr_t)(p.rec32 + j);
                const float cx = r->cx, cy = r->cy, cz = r->cz, s = r->s;
                const float wx = r->wx, wy = r->wy, wz = r->wz;
                const f32x2 dx = px - cx, dy = py - cy, dz = pz - cz;
                f32x2 d2 = pfma(dx, dx, bias);
                d2 = pfma(dy, dy, d2);
                d2 = pfma(dz, dz, d2);
                const f32x2 g = grad32<KIND>(d2, s);
                const f32x2 gx = g * wx, gy = g * wy, gz = g * wz;
                a[0] = pfma(gx, dx, a[0]); a[1] = pfma(gx, dy, a[1]); a[2] = pfma(gx, dz, a[2]);
                a[3] = pfma(gy, dx, a[3]); a[4] = pfma(gy, dy, a[4]); a[5] = pfma(gy, dz, a[5]);
                a[6] = pfma(gz, dx, a[6]); a[7] = pfma(gz, dy, a[7]); a[8] = pfma(gz, dz, a[8]);
            }
#pragma unroll
            for (int q = 0; q < 9; ++q) { S[0][q] += (double)a[q].x; S[1][q] += (double)a[q].y; }
        }
    }

    const float gs = grad_scale32(KIND);
    const float *pc = p.model->poly32;   // {C0, L'x, L'y, L'z, q} per output
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int64_t i = base + v * kBlock + tid;
        if (i >= p.N) continue;
        if (!live[v] || !built) { pass_through(p, i); continue; }
        const float xp[3] = {px[v], py[v], pz[v]};
        float R[9];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float poly = __builtin_fmaf(2.f * pc[5 * c + 4], xp[k], pc[5 * c + 1 + k]);
                R[3 * c + k] = inv_s * __builtin_fmaf(gs, (float)S[v][3 * c + k], poly);
            }
        transport<float>(p, i, R, falloff_of(p, d2v[v]));
    }
}

// ---- fp64: raw coordinates, everything in fp64 ------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ void vectors64_body(const VecParams &p)
{
    constexpr int V = 2;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * V);
    double px[V], py[V], pz[V];
    float d2v[V];
    bool live[V];
    bool any_live = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int64_t i = base + v * kBlock + tid;
        const int64_t ic = i < p.N ? i : p.N - 1;
        px[v] = p.P_in[3 * ic]; py[v] = p.P_in[3 * ic + 1]; pz[v] = p.P_in[3 * ic + 2];
        d2v[v] = p.dist2 ? p.dist2[ic] : 0.f;
        live[v] = (i < p.N) && !(d2v[v] > p.radius2);
        any_live |= live[v];
    }
    const bool built = p.model->terminationtype == 1;
    double S[V][9];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int q = 0; q < 9; ++q) S[v][q] = 0.0;
    if (__any(any_live) && built) {
#pragma unroll 2
        for (int j = 0; j < p.Mpad; ++j) {
            ConstRec64 r = (ConstRec64)(uintptr_t)(p.rec64 + j);
            const double cx = r->cx, cy = r->cy, cz = r->cz, s = r->s;
            const double wx = r->wx, wy = r->wy, wz = r->wz;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double dx = px[v] - cx, dy = py[v] - cy, dz = pz[v] - cz;
                const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                const double g = grad64<KIND>(d2, s);
                const double gx = g * wx, gy = g * wy, gz = g * wz;
                S[v][0] = fma(gx, dx, S[v][0]); S[v][1] = fma(gx, dy, S[v][1]); S[v][2] = fma(gx, dz, S[v][2]);
                S[v][3] = fma(gy, dx, S[v][3]); S[v][4] = fma(gy, dy, S[v][4]); S[v][5] = fma(gy, dz, S[v][5]);
                S[v][6] = fma(gz, dx, S[v][6]); S[v][7] = fma(gz, dy, S[v][7]); S[v][8] = fma(gz, dz, S[v][8]);
            }
        }
    }
    const double gs = grad_scale64(KIND);
    const double *af = p.model->affine64;   // {const, x, y, z} per output
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int64_t i = base + v * kBlock + tid;
        if (i >= p.N) continue;
        if (!live[v] || !built) { pass_through(p, i); continue; }
        double R[9];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) R[3 * c + k] = fma(gs, S[v][3 * c + k], af[4 * c + 1 + k]);
        transport<double>(p, i, R, falloff_of(p, d2v[v]));
    }
}

// k_vectors32_<kind> / k_vectors64_<kind> and their k_vectors32_launch / k_vectors64_launch
FD_OP_KERNELS(k_vectors32_, , (kBlock), VecParams, vectors32_body<KIND>(p))
FD_OP_KERNELS(k_vectors64_, , (kBlock), VecParams, vectors64_body<KIND>(p))

}  // namespace

hipError_t launch_vectors(const DeformArgs &a, const VectorArgs &v, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    VecParams p;
    op::fill_mesh(p, a);
    p.P_in = a.P_in;
    p.vN = v.N; p.vtu = v.tu; p.vtv = v.tv;
    p.oN = v.N_out; p.otu = v.tu_out; p.otv = v.tv_out; p.jac = v.jacobian;
    p.Mpad = a.Mpad;
    p.rec32 = a.rec32; p.rec64 = a.rec64; p.model = a.model;
    const int64_t per = (int64_t)kBlock * 2;
    const dim3 grid((unsigned)((a.N + per - 1) / per));
    return a.precision == FD_EVAL_FP64 ? k_vectors64_launch(a.kind, grid, stream, p) : k_vectors32_launch(a.kind, grid, stream, p);
}

}  // namespace fd
