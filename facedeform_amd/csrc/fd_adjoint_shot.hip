// fd_adjoint_shot.hip -- the adjoint of the deformation for the F cotangents of a shot (fd_deform_adjoint_shot*):
// grad_W[f] = Psi^T R_f, r_{f,v} = f_v Pi_v g_{f,v}, over one mesh, one rig and one gate (include/facedeform_hip.h states the
// contract).  A product with C + 4 rows, 3 F columns and depth N, in fp64 on v_mfma_f64_16x16x4_f64: phi is formed once per
// (vertex, record) for a group of up to 32 frames, not once per frame as k_adjoint64_<kind> forms it.
//
// Mapping to the hardware.  Frames go in groups of at most kFrames = 32: 96 columns, six 16 x 16 tiles; one main launch and one
// reduce launch per group, one after the other on the stream, so the partial blocks of one group are all the scratch there is.
// The C + 4 rows are cut into panels of 128 (eight row tiles); grid = (vertex ranges, row panels).  A 256-thread workgroup
// keeps its 8 x 6 tiles in registers over its whole range: wave w holds row tiles 2 w, 2 w + 1 by six column tiles (96
// accumulator registers).  It walks its range in super-tiles of 128 vertices:
//   prepare   threads 0..127 form x_v and f_v of one vertex each, threads 128..255 the projection axes of the same vertices
//             -- the gate, transport::falloff and transport::axes of the forward path, f = 0 and x = 0 by a select where the
//             vertex is out (the expressions of fd_operator.h's prologue, written out here: DESIGN.md 4.14) -- into LDS, 11
//             doubles per vertex.
//             (128, not 256, vertices: the 10 KB this saves is what lets two workgroups share a CU's LDS.)
// and each super-tile in chunks of 32 vertices:
//   form      thread t owns panel column t & 127 and the chunk's vertices 16 (t >> 7) .. + 16 (a broadcast read of x),
//             x - c in raw coordinates against its Rec64 centre, phi of the kind (fd_pack.h phi_grad64), or 1, x, y, z for the
//             polynomial rows, 0 past C + 4: ONE phi per (vertex, column), written to LDS as fp64.  Each panel forms only its
//             own columns: nothing is formed twice.
//   stage R   thread t owns vertex t & 31 and frames t >> 5, + 8, + 16, + 24: the reads of G are contiguous per frame (their
//             loads are issued before the form phase and used after it), Pi g and the product by f in fp64, exactly 0.0 by a
//             select where the vertex is out -- an MFMA turns 0 x NaN into NaN -- and 0.0 for the frames the group lacks.
//             R is staged column-major (rows of 34 doubles): the writes of a wave's half are contiguous and the reads of the
//             contraction fall on 64 distinct banks.  R for a whole super-tile would not fit LDS; that is why it goes per chunk.
//   contract  lane l reads column l & 15 of vertex l >> 4 of the chunk's depth-4 slice for its two row tiles and the live
//             column tiles: 8 LDS reads feed 12 MFMAs with all six column tiles live.
// A wave whose row tiles both lie past C + 4 skips form and contract (wave-uniform; the columns such a wave would have formed
// are read by dead waves only); column tiles past 3 F are neither contracted nor stored.  At the end every wave writes its live
// tiles to the workgroup's partial block; k_adjoint64_shot_reduce adds the ranges' blocks in their order, applies the factor
// the records' weights carry (fd_pack.h weight_scale64), undoes the multilayer records' centre-major order and writes exactly
// 0.0 for the polynomial rows the term lacks.  No atomics: the ranges are a function of N and C alone (shot_per), never of F,
// and a column's sums do not depend on what the other columns hold, so frame f's block has the same bits whatever the other
// frames are and however many there are.  Everything is fp64; built with -ffp-contract=off like fd_adjoint.hip: every fused
// multiply-add is written out.
#include "fd_operator.h"

namespace fd {

namespace {

constexpr int kBlock = 256;
constexpr int kFrames = 32;                  // frames of a group (FD_MAX_BATCH)
constexpr int kCols = 3 * kFrames;           // 96 columns: six tiles
constexpr int kPanel = 128;                  // rows of a panel: eight tiles, two per wave
constexpr int kSuper = 128;                  // vertices prepared at a time
constexpr int kChunk = 32;                   // vertices staged through LDS per contraction (8 MFMA depths)
constexpr int kPsiRow = kPanel + 16;         // doubles per staged vertex row of Psi: the two vertex rows of a 32-lane read on disjoint banks
constexpr int kRRow = kChunk + 2;            // doubles per staged column of R
constexpr int kVRow = 11;                    // doubles per prepared vertex: x, f, a1, a2 and one of padding (an odd stride)
static_assert(kFrames == FD_MAX_BATCH, "a group is FD_MAX_BATCH frames");

using packing::phi_grad64;
typedef double double4_t __attribute__((ext_vector_type(4)));

struct ShotParams {
    int64_t N;
    const float *P, *G, *dist2;          // G: the group's frames, nF x N x 3
    const float *tu, *tv, *nrm;          // projection frames (all or none)
    float radius2, falloffrate;
    int C;                               // records (fd_model_centres)
    int nt;                              // 16-row tiles, ceil((C + 4) / 16)
    int nF;                              // frames of this group, 1..kFrames
    int64_t per;                         // vertices per range, a multiple of kSuper
    const Rec64 *rec64;
    const DevModel *model;
    double *partial;                     // [range][16 nt][kCols]
};

template <int KIND>
__device__ __forceinline__ void adjoint64_shot_body(const ShotParams &p)
{
    __shared__ __attribute__((aligned(16))) double s_psi[kChunk][kPsiRow];
    __shared__ __attribute__((aligned(16))) double s_r[kCols][kRRow];
    __shared__ __attribute__((aligned(16))) double s_v[kSuper][kVRow];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g = lane >> 4;
    const bool built = p.model->terminationtype == 1;
    const bool proj = p.tu != nullptr;
    const int n = p.C + 4;
    const int panel = (int)blockIdx.y;
    const int ntc = (3 * p.nF + 15) / 16;                              // live column tiles, 1..6

    // form: the column of this thread and its half of the chunk's vertices
    const int gcol = panel * kPanel + (tid & (kPanel - 1));
    const int vhalf = (tid >> 7) * (kChunk / 2);
    const bool form = (gcol & ~63) < n;                                // wave-uniform: 64 columns per wave
    const int type = gcol < p.C ? 0 : (gcol < n ? 1 + gcol - p.C : 5);  // 0 a centre; 1..4 the rows 1, x, y, z; 5 nothing
    const Rec64 &rec = p.rec64[gcol < p.C ? gcol : p.C - 1];
    const double cx = rec.cx, cy = rec.cy, cz = rec.cz, cs = rec.s;

    // stage R: the vertex of this thread within a chunk and its first frame
    const int rv = tid & (kChunk - 1), rf = tid >> 5;

    // contract: the two row tiles of this wave
    const int tr0 = panel * 8 + wave * 2;
    const bool work = tr0 < p.nt;                                      // wave-uniform
    const int acol = wave * 32 + c16;
    double4_t acc[2][6];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};

    const int64_t v0 = (int64_t)blockIdx.x * p.per;
    const int64_t v1 = v0 + p.per < p.N ? v0 + p.per : p.N;
    for (int64_t base = v0; base < v1; base += kSuper) {
        __syncthreads();                                               // the previous super-tile's chunks are done
        {
            const int sv = tid & (kSuper - 1);
            const int64_t i = base + sv;
            const int64_t ic = i < p.N ? i : p.N - 1;
            if (tid < kSuper) {
                double x[3] = {(double)p.P[3 * ic], (double)p.P[3 * ic + 1], (double)p.P[3 * ic + 2]};
                const float d2f = p.dist2 ? p.dist2[ic] : 0.f;
                const double f = (double)transport::falloff(p.dist2 != nullptr, p.radius2, p.falloffrate, d2f);
                // what the forward map moves: in range, not gated, model built, f != 0 (f = 0: the displacement is 0 whatever d is)
                const bool live = (i < v1) && !(d2f > p.radius2) && built && f != 0.0;
                // a select, not a product: a vertex that is out has f = 0.0 here, which stage R turns into r = 0.0 by a select
#pragma unroll
                for (int c = 0; c < 3; ++c) s_v[sv][c] = live ? x[c] : 0.0;
                s_v[sv][3] = live ? f : 0.0;
            } else if (proj) {
                // Pi = a1 a1^T + a2 a2^T with the forward path's axes
                double a1[3], a2[3];
                transport::axes<double>(p.tu, p.tv, p.nrm, ic, a1, a2);
#pragma unroll
                for (int c = 0; c < 3; ++c) { s_v[sv][4 + c] = a1[c]; s_v[sv][7 + c] = a2[c]; }
            }
        }
        __syncthreads();
        const int64_t left = v1 - base;
        const int nv = left < kSuper ? (int)left : kSuper;
        for (int cv = 0; cv < nv; cv += kChunk) {
            // the cotangents of this thread's vertex: requested now, used after the form phase
            float gin[4][3];
            {
                const int64_t i = base + cv + rv;
                const int64_t ic = i < p.N ? i : p.N - 1;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int f = rf + 8 * k;
                    const float *src = p.G + ((size_t)(f < p.nF ? f : 0) * (size_t)p.N + (size_t)ic) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) gin[k][c] = src[c];
                }
            }
            if (form) {
#pragma unroll 4
                for (int v = vhalf; v < vhalf + kChunk / 2; ++v) {
                    const double px = s_v[cv + v][0], py = s_v[cv + v][1], pz = s_v[cv + v][2];
                    double val;
                    if (type == 0) {
                        const double dx = px - cx, dy = py - cy, dz = pz - cz;
                        const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                        double gr;
                        phi_grad64<KIND>(d2, cs, val, gr);
                        (void)gr;
                    } else {
                        val = type == 1 ? 1.0 : (type == 2 ? px : (type == 3 ? py : (type == 4 ? pz : 0.0)));
                    }
                    s_psi[v][tid & (kPanel - 1)] = val;
                }
            }
            {
                const double fs = s_v[cv + rv][3];
                const bool in = fs != 0.0;
                double a1[3], a2[3];
                if (proj) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) { a1[c] = s_v[cv + rv][4 + c]; a2[c] = s_v[cv + rv][7 + c]; }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int f = rf + 8 * k;
                    if (3 * f >= 16 * ntc) continue;                   // a column tile nobody reads (uniform over 32 lanes)
                    double r[3] = {(double)gin[k][0], (double)gin[k][1], (double)gin[k][2]};
                    if (proj) {
                        // Pi is symmetric: Pi g, formed as the forward path forms Pi d
                        const double p1 = a1[0] * r[0] + a1[1] * r[1] + a1[2] * r[2];
                        const double p2 = a2[0] * r[0] + a2[1] * r[1] + a2[2] * r[2];
#pragma unroll
                        for (int c = 0; c < 3; ++c) r[c] = a1[c] * p1 + a2[c] * p2;
                    }
                    // a select, not a product: a vertex that is out (and a frame the group lacks) stages exactly 0.0 whatever G holds
                    const bool keep = in && f < p.nF;
#pragma unroll
                    for (int c = 0; c < 3; ++c) s_r[3 * f + c][rv] = keep ? fs * r[c] : 0.0;
                }
            }
            __syncthreads();
            if (work) {
#pragma unroll 2
                for (int ks = 0; ks < kChunk / 4; ++ks) {
                    const int v = ks * 4 + g;
                    double A[2], B[6];
#pragma unroll
                    for (int a = 0; a < 2; ++a) A[a] = s_psi[v][acol + 16 * a];
#pragma unroll
                    for (int b = 0; b < 6; ++b) B[b] = b < ntc ? s_r[16 * b + c16][v] : 0.0;
#pragma unroll
                    for (int b = 0; b < 6; ++b) {
                        if (b >= ntc) continue;                        // uniform over the workgroup
#pragma unroll
                        for (int a = 0; a < 2; ++a) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[a], B[b], acc[a][b], 0, 0, 0);
                    }
                }
            }
            __syncthreads();                                           // s_psi and s_r may be overwritten
        }
    }

    if (!work) return;
    // accumulator register r of lane (c16, g) is entry (g + 4 r, c16) of its tile: row = the first operand's index
    double *out = p.partial + (size_t)blockIdx.x * (size_t)(16 * p.nt) * kCols;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (tr0 + a >= p.nt) continue;                                 // wave-uniform
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            if (b >= ntc) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(16 * (tr0 + a) + g + 4 * r) * kCols + 16 * b + c16] = acc[a][b][r];
        }
    }
}

// k_adjoint64_shot_<kind> and k_adjoint64_shot_launch
FD_OP_KERNELS(k_adjoint64_shot_, , (kBlock, 2), ShotParams, adjoint64_shot_body<KIND>(p))

// The ranges' blocks added in their order, the same for every call with this N and C: one thread per entry (row, column) of the
// group, consecutive threads on consecutive columns, stored by fd_operator.h's row rule.  grad_W is the group's first frame:
// nF blocks of (C + 4) x 3.
__global__ __launch_bounds__(kBlock) void k_adjoint64_shot_reduce(const double *partial, int nranges, int nt, int nF, int C,
                                                                  int layers, int T, double wscale, double *grad_W)
{
    const int n = C + 4, ncols = 3 * nF;
    const int e = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (e >= n * ncols) return;
    const int row = e / ncols, col = e % ncols;
    const double *src = partial + (size_t)row * kCols + col;
    const size_t stride = (size_t)(16 * nt) * kCols;
    double sum = 0.0;
#pragma unroll 8
    for (int r = 0; r < nranges; ++r) sum += src[(size_t)r * stride];
    const int f = col / 3, a = col % 3;
    double *out = grad_W + (size_t)f * n * 3;
    op::store_row(out, row, a, C, layers, T, wscale, sum);
}

int64_t shot_per(int64_t N, int C) { return op::range_per(N, op::padded_rows(C) * kCols * sizeof(double), kSuper); }

}  // namespace

int adjoint_shot_ranges(int64_t N, int C) { return op::range_count(N, shot_per(N, C)); }

size_t adjoint_shot_partial_doubles(int64_t N, int C)
{
    return (size_t)adjoint_shot_ranges(N, C) * op::padded_rows(C) * kCols;
}

hipError_t launch_adjoint_shot(const DeformArgs &a, const AdjointShotArgs &g, hipStream_t stream)
{
    const int ranges = adjoint_shot_ranges(a.N, a.M);
    const int nt = (a.M + 4 + 15) / 16;
    const int n = a.M + 4;
    for (int f0 = 0; f0 < g.F; f0 += kFrames) {
        const int nF = g.F - f0 < kFrames ? g.F - f0 : kFrames;
        if (ranges > 0) {
            ShotParams p;
            op::fill_mesh(p, a);
            p.P = a.P_in; p.G = g.G + (size_t)f0 * (size_t)a.N * 3;
            p.C = a.M; p.nt = nt; p.nF = nF;
            p.per = shot_per(a.N, a.M);
            p.rec64 = a.rec64; p.model = a.model;
            p.partial = g.partial;
            const dim3 grid((unsigned)ranges, (unsigned)((nt + 7) / 8));
            const hipError_t e = k_adjoint64_shot_launch(a.kind, grid, stream, p);
            if (e != hipSuccess) return e;
        }
        const int entries = n * 3 * nF;
        hipLaunchKernelGGL(k_adjoint64_shot_reduce, dim3((unsigned)((entries + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                           (const double *)g.partial, ranges, nt, nF, a.M, a.layers, g.T, packing::weight_scale64(a.kind),
                           g.grad_W + (size_t)f0 * (size_t)n * 3);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace fd
