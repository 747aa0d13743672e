// fd_operator.h -- what the one-context operators beside the evaluation share: fd_vectors.hip, fd_invert.hip,
// fd_adjoint.hip, fd_adjoint_points.hip, fd_adjoint_shot.hip, fd_gram.hip and fd_bake.hip.
//
// All of them rest on one contract: the forward map's gate, fall-off and projection, the same operations.  For all: the fill
// of the mesh fields from DeformArgs, the kind dispatch, and -- for the files that reduce partial blocks -- the partition of the
// vertices into ranges and the row rule of the reduce kernels.  For fd_adjoint.hip, fd_invert.hip and fd_bake.hip also the mesh head
// their parameters begin with and the vertex prologue, for the first two Pi r; the other four keep those expressions written out with the argument
// layout they had, because with the head their kernels measured slower.  The walks, the LDS layouts, the MFMA
// contractions and every constant stay in the files.  These files are built with -ffp-contract=off: every operation and its
// order here is the result's, written out.
#pragma once
#include "fd_pack.h"
#include "fd_transport.h"

namespace fd {
namespace op {

// ---- the mesh fields (host and device) --------------------------------------------------------------------------------------
// The head the parameters of fd_adjoint.hip and fd_invert.hip begin with (they derive from it); the kernels read it.  56 bytes
// ending on an 8-byte boundary: nothing behind it is pushed by padding (DESIGN.md 4.7g asked the same of ShotEvalMesh).
struct Mesh {
    int64_t N;
    const float *P, *dist2;              // P: the points the operator is taken at (the inverse: the deformed points y)
    const float *tu, *tv, *nrm;          // projection frames (all or none)
    float radius2, falloffrate;
};
static_assert(sizeof(Mesh) == 56 && alignof(Mesh) == 8, "the mesh head is 56 bytes and ends on an 8-byte boundary");

// the one fill of a kernel's mesh fields from `a`, wherever the fields stand in Params; the points are the caller's (P, P_in)
template <class Params>
void fill_mesh(Params &p, const DeformArgs &a)
{
    p.N = a.N;
    p.dist2 = a.dist2;
    p.tu = a.tu; p.tv = a.tv; p.nrm = a.nrm;
    p.radius2 = a.radius2; p.falloffrate = a.falloffrate;
}

// parameters that derive from Mesh, the head filled from `a`; the caller fills what is its own
template <class Params>
Params params_of(const DeformArgs &a)
{
    Params p;
    fill_mesh(p, a);
    p.P = a.P_in;
    return p;
}

// ---- host: the kind dispatch -----------------------------------------------------------------------------------------------
// The four __global__ entry points STEM<kind>SUFFIX of a body -- stable names for profiles -- and STEM##launch##SUFFIX, which
// launches the one for `kind` (FD_KERNEL_GAUSSIAN_QNN evaluates as a Gaussian; any other kind is hipErrorInvalidValue).
// BOUNDS: the launch bounds in parentheses; the last argument: the body's call, KIND its kind.  The including file defines
// kBlock, the threads of a workgroup, before it uses the macro: the launch takes it from there.
#define FD_OP_ENTRY(NAME, K, STEM, SUFFIX, BOUNDS, PARAMS, ...) \
    __global__ __launch_bounds__ BOUNDS void STEM##NAME##SUFFIX(const PARAMS p) { constexpr int KIND = K; __VA_ARGS__; }
#define FD_OP_KERNELS(STEM, SUFFIX, BOUNDS, PARAMS, ...)                                                                    \
    FD_OP_ENTRY(gaussian, FD_KERNEL_GAUSSIAN, STEM, SUFFIX, BOUNDS, PARAMS, __VA_ARGS__)                                    \
    FD_OP_ENTRY(thin_plate, FD_KERNEL_THIN_PLATE, STEM, SUFFIX, BOUNDS, PARAMS, __VA_ARGS__)                                \
    FD_OP_ENTRY(biharmonic, FD_KERNEL_BIHARMONIC, STEM, SUFFIX, BOUNDS, PARAMS, __VA_ARGS__)                                \
    FD_OP_ENTRY(cubic, FD_KERNEL_CUBIC, STEM, SUFFIX, BOUNDS, PARAMS, __VA_ARGS__)                                          \
    hipError_t STEM##launch##SUFFIX(int kind, dim3 grid, hipStream_t stream, const PARAMS &p)                               \
    {                                                                                                                       \
        switch (kind) {                                                                                                     \
        case FD_KERNEL_GAUSSIAN:                                                                                            \
        case FD_KERNEL_GAUSSIAN_QNN: hipLaunchKernelGGL(STEM##gaussian##SUFFIX, grid, dim3(kBlock), 0, stream, p); break;   \
        case FD_KERNEL_THIN_PLATE: hipLaunchKernelGGL(STEM##thin_plate##SUFFIX, grid, dim3(kBlock), 0, stream, p); break;   \
        case FD_KERNEL_BIHARMONIC: hipLaunchKernelGGL(STEM##biharmonic##SUFFIX, grid, dim3(kBlock), 0, stream, p); break;   \
        case FD_KERNEL_CUBIC: hipLaunchKernelGGL(STEM##cubic##SUFFIX, grid, dim3(kBlock), 0, stream, p); break;             \
        default: return hipErrorInvalidValue;                                                                               \
        }                                                                                                                   \
        return hipGetLastError();                                                                                           \
    }

// ---- host: the partition of the vertices into ranges -----------------------------------------------------------------------
// Vertices per range, a multiple of `super`: as many ranges as kMaxRanges and kScratchBound bytes of partial blocks allow, each
// block `block_bytes`.  A function of N and the block alone, so the same N and C give the same ranges and the same bits.
constexpr int kMaxRanges = 256;
constexpr size_t kScratchBound = (size_t)256 << 20;      // bytes of partial blocks at most

inline int64_t range_per(int64_t N, size_t block_bytes, int super)
{
    int64_t maxr = (int64_t)(kScratchBound / block_bytes);
    maxr = maxr < 1 ? 1 : (maxr > kMaxRanges ? kMaxRanges : maxr);
    const int64_t supers = (N + super - 1) / super;
    return (supers + maxr - 1) / maxr * super;
}

inline int range_count(int64_t N, int64_t per) { return N <= 0 ? 0 : (int)((N + per - 1) / per); }

// the side of a padded partial block: C + 4 rounded up to whole 16-row tiles
inline size_t padded_rows(int C) { return (size_t)(C + 4 + 15) / 16 * 16; }

// ---- device: fd_adjoint.hip and fd_invert.hip, and the reduce kernels -------------------------------------------------------
// The vertex prologue: x and f of vertex i (ic: i clamped into the mesh, `end`: where the caller's vertices end, N); true where
// the forward map moves the vertex with f: in range, not gated, model built.  A kernel puts its own last condition (f != 0)
// on top.  The gate and the fall-off are the evaluation's.
__device__ __forceinline__ bool vertex(const Mesh &m, int64_t i, int64_t ic, int64_t end, bool built, double x[3], double &f)
{
    x[0] = (double)m.P[3 * ic]; x[1] = (double)m.P[3 * ic + 1]; x[2] = (double)m.P[3 * ic + 2];
    const float d2f = m.dist2 ? m.dist2[ic] : 0.f;
    f = (double)transport::falloff(m.dist2 != nullptr, m.radius2, m.falloffrate, d2f);
    return (i < end) && !(d2f > m.radius2) && built;
}

// r <- Pi r, Pi = a1 a1^T + a2 a2^T (symmetric: Pi g is formed as the forward path forms Pi d)
__device__ __forceinline__ void project(const double a1[3], const double a2[3], double r[3])
{
    const double p1 = a1[0] * r[0] + a1[1] * r[1] + a1[2] * r[2];
    const double p2 = a2[0] * r[0] + a2[1] * r[1] + a2[2] * r[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = a1[c] * p1 + a2[c] * p2;
}

// The reduce kernels' row rule: `sum` is entry (row, a) of a (C + 4) x 3 block.  Record position `row` of a multilayer model
// (centre-major, fd_pack.h) goes back to its row of W (layer-major) and takes `wscale`, the factor between W and the records'
// weights (+ 0.0 keeps an empty sum at +0 under a negative factor); a polynomial row is the sum, or exactly 0.0 for a term the
// model lacks (T terms).  k_gram64_reduce keeps its own text: both of its indices are rows.
__device__ __forceinline__ void store_row(double *out, int row, int a, int C, int layers, int T, double wscale, double sum)
{
    if (row < C) {
        int j = row;
        if (layers > 1) { const int Mc = C / layers; j = (row % layers) * Mc + row / layers; }
        out[3 * j + a] = wscale * sum + 0.0;
    } else {
        out[3 * row + a] = row - C < T ? sum : 0.0;
    }
}

}  // namespace op
}  // namespace fd
