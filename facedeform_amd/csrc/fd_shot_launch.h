// fd_shot_launch.h -- the host side of a shot launch, ONE copy for the four vector launches (fd_vectors_shot.h) and the three
// staged position launches (fd_eval_shared64.hip, fd_eval_shared_ml64.hip, fd_eval_shared_ml.hip):
// evened K chunks, the grid of persistent workgroups, the launch with its LDS attribute, the (NT, DENSE) dispatch -- and,
// for the position launches, the head of the kernels' Params, what epilogue_store is handed per frame, the fill of the pack
// kernels' tables and the tail of a pack launch.  All of these launches run 8 waves per workgroup.
#pragma once
#include <algorithm>
#include <type_traits>

#include "fd_eval_common.h"
#include "fd_eval_point.h"

namespace fd {
namespace {

constexpr int kShotWaves = 8;
constexpr int kShotThreads = 64 * kShotWaves;

// n K steps in the fewest chunks of at most kmax, evened out (256 centres x 32 frames in fp64 are two chunks of 32 K steps)
inline int even_chunks(int n, int kmax)
{
    const int nchunks = (n + kmax - 1) / kmax;
    return (n + nchunks - 1) / nchunks;
}

struct ShotGrid {
    size_t lds;
    unsigned grid;
    int ngroups;
};

// persistent workgroups over groups of `group` vertices: as many per CU as the LDS admits, `per_cu_cap` at most; max_wgs > 0
// (fd_batch_set_eval_cus) names their number instead
inline hipError_t shot_grid(int64_t N, int group, int max_wgs, size_t lds, int per_cu_cap, ShotGrid &gr)
{
    const int64_t ngroups = (N + group - 1) / group;
    if (ngroups > 0x7fffffff) return hipErrorInvalidValue;
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(per_cu_cap, (int64_t)(160 * 1024 / lds)));
    const int64_t wgs = max_wgs > 0 ? (max_wgs < 4096 ? max_wgs : 4096) : (int64_t)device_cus() * per_cu;
    gr.lds = lds;
    gr.grid = (unsigned)(ngroups < wgs ? ngroups : wgs);
    gr.ngroups = (int)ngroups;
    return hipSuccess;
}

// Kernel(args..., ngroups)
template <auto Kernel, class... Args>
hipError_t launch_shot(const ShotGrid &gr, hipStream_t stream, const Args &...args)
{
    static LdsAttrOnce once;          // one per kernel instantiation
    hipError_t e = once.ensure((const void *)Kernel, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, dim3(gr.grid), dim3(kShotThreads), gr.lds, stream, args..., gr.ngroups);
    return hipGetLastError();
}

// f(NT, DENSE) as compile-time constants for the tile counts a shot can have (s64_tiles, dense from 13 frames):
//   for_tiles(NT, dense, [&](auto nt, auto dns) { return launch_shot<k<nt.value, dns.value>>(...); })
template <class F>
hipError_t for_tiles(int NT, bool dense, F &&f)
{
    using std::integral_constant;
    if (dense) {
        if (NT == 3) return f(integral_constant<int, 3>{}, std::true_type{});
        if (NT == 6) return f(integral_constant<int, 6>{}, std::true_type{});
    } else {
        if (NT == 1) return f(integral_constant<int, 1>{}, std::false_type{});
        if (NT == 2) return f(integral_constant<int, 2>{}, std::false_type{});
        if (NT == 3) return f(integral_constant<int, 3>{}, std::false_type{});
    }
    return hipErrorInvalidValue;
}

// ---- the position launches ----
// the head of their kernels' Params: 56 bytes, ending on an 8-byte boundary (nF follows in the Params themselves, as behind
// fd_vectors_shot.h's ShotMesh)
struct ShotEvalMesh {
    int64_t N;
    const float *P_in, *dist2;
    const float *tu, *tv, *nrm;
    float radius2, falloffrate;
};

inline void fill_eval_mesh(ShotEvalMesh &p, const SharedEvalCommon &a)
{
    p.N = a.N; p.P_in = a.P_in; p.dist2 = a.dist2; p.tu = a.tu; p.tv = a.tv; p.nrm = a.nrm;
    p.radius2 = a.radius2; p.falloffrate = a.falloffrate;
}

// what epilogue_store reads for one frame of a shot: the mesh, the frame's outputs, no model
__device__ __forceinline__ EvalParams shot_eval_params(const ShotEvalMesh &p, float *P_out, float *falloff_out, int Mpad, int delta)
{
    EvalParams ep;
    ep.N = p.N;
    ep.P_in = p.P_in; ep.P_out = P_out;
    ep.dist2 = p.dist2; ep.falloff_out = falloff_out;
    ep.tu = p.tu; ep.tv = p.tv; ep.nrm = p.nrm;
    ep.radius2 = p.radius2; ep.falloffrate = p.falloffrate;
    ep.Mpad = Mpad; ep.delta = delta;
    ep.rec32 = nullptr; ep.rec64 = nullptr; ep.tiles = nullptr; ep.tiles16 = nullptr; ep.model = nullptr;
    return ep;
}

// a pack kernel's per-frame tables {rec, model, P_out, fall}
template <class Pack, class Rec>
void fill_pack(Pack &pa, const SharedEvalCommon &a, const Rec *const *rec)
{
    for (int f = 0; f < a.nF; ++f) {
        pa.rec[f] = rec[f]; pa.model[f] = a.model[f];
        pa.P_out[f] = a.P_out[f]; pa.fall[f] = a.falloff_out ? a.falloff_out[f] : nullptr;
    }
}

// behind a pack kernel's launch: from here on nothing of the contexts is read
inline hipError_t shot_packed(const SharedEvalCommon &a, hipStream_t stream)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return a.packed_ev ? hipEventRecord(a.packed_ev, stream) : hipSuccess;
}

}  // namespace
}  // namespace fd
