// fd_vectors_shot.h -- what the four one-launch vector kernels of a shot share (fd_vectors_shared.hip, fd_vectors_shared64.hip,
// fd_vectors_shared_ml.hip, fd_vectors_shared_ml64.hip): the kernel arguments every one of them takes, the
// deal of the output pointers into LDS, the pass-through of a gated vertex, and the fill of the arguments; chunking, grid and
// the (NT, DENSE) dispatch are fd_shot_launch.h's, shared with the position launches.  ONE copy.  The files keep their frame
// constants, staging, K loops and their epilogues: in functions here the epilogues compile to other schedules, measurably
// slower in fp64; as the header stands, every kernel's instruction stream is what it was with the copies in
// the files.
//
// All four launches run 8 waves per workgroup, a wave owning one vertex tile of 16 per group, and deal the frames onto NT row
// tiles of 16: padded up to 12 frames (tile T = frames 4 T .. 4 T + 3), dense from 13.
#pragma once
#include "fd_shared64.h"
#include "fd_shot_launch.h"
#include "fd_transport.h"

namespace fd {
namespace {

constexpr int kShotGroup = 16 * kShotWaves;        // vertices per workgroup and group
static_assert(kShotThreads == kS64Threads, "the fp64 launches stage with the position launch's thread count");
constexpr int kFrameWords = 16;                    // fp32 launches, per frame in LDS: {basis scale, built, L'[3][3], q[3], 2 unused}

// ---- kernel arguments ----
struct ShotOut {                  // per-frame outputs (the kernel's FIRST argument; dealt into LDS by deal_out_pointers)
    float *N[kMaxBatch], *tu[kMaxBatch], *tv[kMaxBatch], *jac[kMaxBatch];
};

// the head of every launch's Params: the mesh and the vectors (nF follows in the Params themselves: in here it would end the
// struct with four bytes of padding and move every field behind it in the argument segment)
struct ShotMesh {
    int64_t N;
    const float *P_in, *dist2;
    const float *tu, *tv, *nrm;          // projection frames (all or none)
    const float *vN, *vtu, *vtv;         // vectors to transport (shared by the frames)
    float radius2, falloffrate;
};

// ---- device side ----
// one frame of one vertex, as fd_transport.h's transport(), jacobian() and carry() read it; T: the precision of the axes
template <typename T>
struct FrameIO {
    const float *tu, *tv, *nrm;
    T a1[3], a2[3];
    const float *vN, *vtu, *vtv;
    float *oN, *otu, *otv, *jac;
    static constexpr bool kGivenAxes = true;
    // (written once, read by nobody in this launch: past L2, like the position launch's stores)
    static __device__ __forceinline__ void store(float *dst, float v) { __builtin_nontemporal_store(v, dst); }
};

__device__ __forceinline__ float half_at(const uint4 *base, size_t word, int e)
{
    const unsigned short u = reinterpret_cast<const unsigned short *>(base + word)[e];
    return (float)__builtin_bit_cast(_Float16, u);
}

// ShotOut is the kernel's FIRST argument: its tables are read straight from the argument segment (indexed by the thread, the
// argument itself would be copied to scratch memory first; unrolled over constant indices, it is held in SGPRs and spilled)
__device__ __forceinline__ void deal_out_pointers(float **s_ptr, int nF)
{
    const int tid = threadIdx.x;
    if (tid < 4 * kMaxBatch) {
        const int f = tid >> 2, w = tid & 3;
        float *const *tab = (float *const *)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
        s_ptr[tid] = f < nF ? tab[kMaxBatch * w + f] : nullptr;
    }
}

// gated vertex / unbuilt frame: the vectors bit for bit, A = I
template <class IO>
__device__ __forceinline__ void pass_through(const IO &io, int64_t vi)
{
    for (int c = 0; c < 3; ++c) {
        if (io.vN) IO::store(&io.oN[3 * vi + c], io.vN[3 * vi + c]);
        if (io.vtu) IO::store(&io.otu[3 * vi + c], io.vtu[3 * vi + c]);
        if (io.vtv) IO::store(&io.otv[3 * vi + c], io.vtv[3 * vi + c]);
    }
    if (io.jac)
#pragma unroll
        for (int q = 0; q < 9; ++q) IO::store(&io.jac[9 * vi + q], (q % 4 == 0) ? 1.f : 0.f);
}

// ---- host side ----
inline int shot_tiles(int nF) { return nF > 12 ? 3 * ((nF + 15) / 16) : (nF + 3) / 4; }      // as s64_tiles

inline void fill_shot(ShotMesh &p, ShotOut &out, const SharedVectorCommon &a)
{
    p.N = a.N; p.P_in = a.P_in; p.dist2 = a.dist2; p.tu = a.tu; p.tv = a.tv; p.nrm = a.nrm;
    p.vN = a.vN; p.vtu = a.vtu; p.vtv = a.vtv;
    p.radius2 = a.radius2; p.falloffrate = a.falloffrate;
    for (int f = 0; f < a.nF; ++f) { out.N[f] = a.N_out[f]; out.tu[f] = a.tu_out[f]; out.tv[f] = a.tv_out[f]; out.jac[f] = a.jacobian[f]; }
}

// groups of kShotGroup vertices; two workgroups per CU at most (two waves per SIMD each)
inline hipError_t shot_grid(const SharedVectorCommon &a, size_t lds, ShotGrid &gr) { return shot_grid(a.N, kShotGroup, a.max_wgs, lds, 2, gr); }

}  // namespace
}  // namespace fd

