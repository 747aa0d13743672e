// fd_transport.h -- the transport epilogue of fd_deform_vectors* (DESIGN.md 4.7): ONE copy for the one-frame launch
// (fd_vectors.hip, k_vectors{32,64}_<kind>) and the four shot launches (fd_vectors_shared.hip and fd_vectors_shared_ml.hip call
// transport(), fd_vectors_shared64.hip and fd_vectors_shared_ml64.hip jacobian() and carry(); their FrameIO is fd_vectors_shot.h's).
//
// A = I + f Pi R per vertex, R = J before the projection; t' = A t, n' = cof(A) n rescaled to |n|
// (include/facedeform_hip.h states the definition).  `p` names the arrays of ONE frame: the projection frames tu, tv, nrm
// and the vectors vN, vtu, vtv (inputs, indexed by the vertex), oN, otu, otv, jac (outputs, indexed by the vertex).
// IO::kGivenAxes: the caller has formed the projection axes of the vertex once for all its frames (p.a1, p.a2; a launch
// that serves many frames per vertex); otherwise they are formed here from p.tu, p.tv, p.nrm.  IO::store writes one
// output value (the shared-rig launch: with the non-temporal hint).
#pragma once
#include <hip/hip_runtime.h>

namespace fd {
namespace transport {

template <typename T> __device__ __forceinline__ T vsqrt(T x);
template <> __device__ __forceinline__ float vsqrt(float x) { return sqrtf(x); }
template <> __device__ __forceinline__ double vsqrt(double x) { return sqrt(x); }

template <typename T>
__device__ __forceinline__ void normalize(T v[3])
{
    const T l2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (l2 > T(0)) {
        const T inv = T(1) / vsqrt(l2);
        v[0] *= inv; v[1] *= inv; v[2] *= inv;
    }
}

// The two axes of the projection at vertex i, for a launch that forms them once for all the frames of a vertex (IO::kGivenAxes).
// The same operations as the inline form in transport() below, which the one-frame kernels keep: routed through this
// function their fp64 instantiations come out with other register assignments (same results, other code objects).
template <typename T>
__device__ __forceinline__ void axes(const float *tu, const float *tv, const float *nrm, int64_t i, T a1[3], T a2[3])
{
    T u[3] = {(T)tu[3 * i], (T)tu[3 * i + 1], (T)tu[3 * i + 2]};
    T v[3] = {(T)tv[3 * i], (T)tv[3 * i + 1], (T)tv[3 * i + 2]};
    T n[3] = {(T)nrm[3 * i], (T)nrm[3 * i + 1], (T)nrm[3 * i + 2]};
    normalize(u); normalize(v); normalize(n);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        T g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = u[k] * u[j] + v[k] * v[j] + n[k] * n[j];
        a1[j] = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
        a2[j] = v[0] * g[0] + v[1] * g[1] + v[2] * g[2];
    }
    normalize(a1); normalize(a2);
}

// R <- Pi R
template <typename T>
__device__ __forceinline__ void project(T R[9], const T a1[3], const T a2[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T p1 = a1[0] * R[k] + a1[1] * R[3 + k] + a1[2] * R[6 + k];
        const T p2 = a2[0] * R[k] + a2[1] * R[3 + k] + a2[2] * R[6 + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * c + k] = a1[c] * p1 + a2[c] * p2;
    }
}

// The transport epilogue for one live vertex: R = (J before the projection, row c = output c, column k = d/dx_k), f the
// fall-off; T = float or double, the precision of the evaluation.  Reads the vectors, then writes (outputs may alias).
template <typename T, class IO>
__device__ __forceinline__ void transport(const IO &p, int64_t i, T R[9], float falloff)
{
    const T f = (T)falloff;
    T A[9];
    if (falloff == 0.f) {
#pragma unroll
        for (int q = 0; q < 9; ++q) A[q] = (q % 4 == 0) ? T(1) : T(0);
    } else {
        if (p.tu) {
            // Pi = a1 a1^T + a2 a2^T, a1, a2 as project_to_tangents (reference src/SOP_FaceDeform.hpp:28-41) builds them
            if constexpr (IO::kGivenAxes) {
                project(R, p.a1, p.a2);
            } else {
                T u[3] = {(T)p.tu[3 * i], (T)p.tu[3 * i + 1], (T)p.tu[3 * i + 2]};
                T v[3] = {(T)p.tv[3 * i], (T)p.tv[3 * i + 1], (T)p.tv[3 * i + 2]};
                T n[3] = {(T)p.nrm[3 * i], (T)p.nrm[3 * i + 1], (T)p.nrm[3 * i + 2]};
                normalize(u); normalize(v); normalize(n);
                T a1[3], a2[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    T g[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) g[k] = u[k] * u[j] + v[k] * v[j] + n[k] * n[j];
                    a1[j] = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
                    a2[j] = v[0] * g[0] + v[1] * g[1] + v[2] * g[2];
                }
                normalize(a1); normalize(a2);
                project(R, a1, a2);
            }
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) A[q] = ((q % 4 == 0) ? T(1) : T(0)) + f * R[q];
    }
    if (p.vtu) {
        const T t[3] = {(T)p.vtu[3 * i], (T)p.vtu[3 * i + 1], (T)p.vtu[3 * i + 2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = (float)(A[3 * c] * t[0] + A[3 * c + 1] * t[1] + A[3 * c + 2] * t[2]);
            IO::store(&p.otu[3 * i + c], r);
        }
    }
    if (p.vtv) {
        const T t[3] = {(T)p.vtv[3 * i], (T)p.vtv[3 * i + 1], (T)p.vtv[3 * i + 2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = (float)(A[3 * c] * t[0] + A[3 * c + 1] * t[1] + A[3 * c + 2] * t[2]);
            IO::store(&p.otv[3 * i + c], r);
        }
    }
    if (p.vN) {
        const float nf[3] = {p.vN[3 * i], p.vN[3 * i + 1], p.vN[3 * i + 2]};
        const T n[3] = {(T)nf[0], (T)nf[1], (T)nf[2]};
        // cof(A) n = n0 (c1 x c2) + n1 (c2 x c0) + n2 (c0 x c1), c_k = column k of A
        T m[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
            const T x12 = A[3 * r1 + 1] * A[3 * r2 + 2] - A[3 * r2 + 1] * A[3 * r1 + 2];
            const T x20 = A[3 * r1 + 2] * A[3 * r2 + 0] - A[3 * r2 + 2] * A[3 * r1 + 0];
            const T x01 = A[3 * r1 + 0] * A[3 * r2 + 1] - A[3 * r2 + 0] * A[3 * r1 + 1];
            m[r] = n[0] * x12 + n[1] * x20 + n[2] * x01;
        }
        const T nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        const T mm = m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
        float o[3] = {nf[0], nf[1], nf[2]};
        if (nn > T(0) && mm > T(0)) {
            const T sc = vsqrt(nn) / vsqrt(mm);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (float)(m[c] * sc);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) IO::store(&p.oN[3 * i + c], o[c]);
    }
    if (p.jac) {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const float r = (float)A[q];
            IO::store(&p.jac[9 * i + q], r);
        }
    }
}

// fd_eval.hip's fall-off, the same operations: the f the deformation multiplied by (d2: the vertex's dist2 entry, 0 without
// a dist2 array)
__device__ __forceinline__ float falloff(bool has_dist2, float radius2, float falloffrate, float d2)
{
    float f = 1.f;
    if (has_dist2 || !(radius2 != 0.f)) {
        f = fminf(d2 / radius2, 1.f);
        f = powf(1.f - f, falloffrate);
    }
    return f;
}

// transport() in its two halves, the same operations in the same order, for a launch that holds many frames of a vertex in
// registers (fd_vectors_shared64.hip, fd_vectors_shared_ml64.hip): it runs the first half for all of them before the second, so that the projection axes are
// not live under the cofactors.  The launches above keep transport() as it is: composed of these two, their code objects come
// out with other register assignments and schedules.
//   jacobian(): R = (J before the projection, row c = output c, column k = d/dx_k), f the fall-off -> A = I + f Pi R;
//   carry():    reads the vectors, then writes t' = A t, n' = cof(A) n rescaled to |n| and A (outputs may alias).
// T = float or double, the precision of the evaluation.
template <typename T, class IO>
__device__ __forceinline__ void jacobian(const IO &p, int64_t i, T R[9], float falloff, T A[9])
{
    const T f = (T)falloff;
    if (falloff == 0.f) {
#pragma unroll
        for (int q = 0; q < 9; ++q) A[q] = (q % 4 == 0) ? T(1) : T(0);
    } else {
        if (p.tu) {
            // Pi = a1 a1^T + a2 a2^T, a1, a2 as project_to_tangents (reference src/SOP_FaceDeform.hpp:28-41) builds them
            if constexpr (IO::kGivenAxes) {
                project(R, p.a1, p.a2);
            } else {
                T u[3] = {(T)p.tu[3 * i], (T)p.tu[3 * i + 1], (T)p.tu[3 * i + 2]};
                T v[3] = {(T)p.tv[3 * i], (T)p.tv[3 * i + 1], (T)p.tv[3 * i + 2]};
                T n[3] = {(T)p.nrm[3 * i], (T)p.nrm[3 * i + 1], (T)p.nrm[3 * i + 2]};
                normalize(u); normalize(v); normalize(n);
                T a1[3], a2[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    T g[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) g[k] = u[k] * u[j] + v[k] * v[j] + n[k] * n[j];
                    a1[j] = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
                    a2[j] = v[0] * g[0] + v[1] * g[1] + v[2] * g[2];
                }
                normalize(a1); normalize(a2);
                project(R, a1, a2);
            }
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) A[q] = ((q % 4 == 0) ? T(1) : T(0)) + f * R[q];
    }
}

template <typename T, class IO>
__device__ __forceinline__ void carry(const IO &p, int64_t i, const T A[9])
{
    if (p.vtu) {
        const T t[3] = {(T)p.vtu[3 * i], (T)p.vtu[3 * i + 1], (T)p.vtu[3 * i + 2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = (float)(A[3 * c] * t[0] + A[3 * c + 1] * t[1] + A[3 * c + 2] * t[2]);
            IO::store(&p.otu[3 * i + c], r);
        }
    }
    if (p.vtv) {
        const T t[3] = {(T)p.vtv[3 * i], (T)p.vtv[3 * i + 1], (T)p.vtv[3 * i + 2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = (float)(A[3 * c] * t[0] + A[3 * c + 1] * t[1] + A[3 * c + 2] * t[2]);
            IO::store(&p.otv[3 * i + c], r);
        }
    }
    if (p.vN) {
        const float nf[3] = {p.vN[3 * i], p.vN[3 * i + 1], p.vN[3 * i + 2]};
        const T n[3] = {(T)nf[0], (T)nf[1], (T)nf[2]};
        // cof(A) n = n0 (c1 x c2) + n1 (c2 x c0) + n2 (c0 x c1), c_k = column k of A
        T m[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
            const T x12 = A[3 * r1 + 1] * A[3 * r2 + 2] - A[3 * r2 + 1] * A[3 * r1 + 2];
            const T x20 = A[3 * r1 + 2] * A[3 * r2 + 0] - A[3 * r2 + 2] * A[3 * r1 + 0];
            const T x01 = A[3 * r1 + 0] * A[3 * r2 + 1] - A[3 * r2 + 0] * A[3 * r1 + 1];
            m[r] = n[0] * x12 + n[1] * x20 + n[2] * x01;
        }
        const T nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        const T mm = m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
        float o[3] = {nf[0], nf[1], nf[2]};
        if (nn > T(0) && mm > T(0)) {
            const T sc = vsqrt(nn) / vsqrt(mm);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (float)(m[c] * sc);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) IO::store(&p.oN[3 * i + c], o[c]);
    }
    if (p.jac) {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const float r = (float)A[q];
            IO::store(&p.jac[9 * i + q], r);
        }
    }
}

}  // namespace transport
}  // namespace fd
