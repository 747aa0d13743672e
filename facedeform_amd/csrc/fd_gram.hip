// fd_gram.hip -- the Gram operator of the deformation (fd_deform_gram*): H[q][j][k] = sum over the vertices of
// q_v Psi_vj Psi_vk, q_v = omega_v f_v^2 (Pi_v^2)[b][c], Psi_v the row of length C + 4 that multiplies W in the forward map
// (include/facedeform_hip.h states the contract).  A symmetric rank-N update in fp64 on v_mfma_f64_16x16x4_f64.
//
// Mapping to the hardware.  The C + 4 columns are cut into panels of 128 (eight 16 x 16 tiles); grid.y is a panel pair
// (pi <= pj), grid.x a range of vertices, grid.z one of the nq projection components.  A 256-thread workgroup walks its range
// in super-tiles of 256 vertices: each thread forms x_v and q_v of one vertex once -- the gate, transport::falloff and
// transport::axes of the forward path, Pi squared in fp64, q = 0 and x = 0 by a select where the vertex is out -- into LDS.
// The super-tile goes through the matrix pipe in chunks of 32 vertices:
//   form      thread t owns staged column t (0..127 panel pi, 128..255 panel pj) and walks the chunk's vertices (a broadcast
//             read of x), x - c in raw coordinates against its Rec64 centre, phi of the kind (fd_pack.h phi_grad64), or
//             1, x, y, z for the polynomial columns, 0 past C + 4: ONE phi per (vertex, staged column), written to LDS as fp64
//             (rows of 272 doubles: the 16 doubles of padding put the two vertex rows of a 32-lane read group on disjoint banks);
//   contract  wave w holds the 4 x 4 tile block (w >> 1, w & 1) of the panel pair in registers (128 accumulator VGPRs) for
//             the whole range.  Lane l reads column l & 15 of vertex l >> 4 for its four row tiles and four column tiles --
//             eight 8-byte LDS reads and one of q_v feed sixteen MFMAs -- scales the row operands by q_v and issues the block.
// A wave whose block lies wholly past the last tile, or below the diagonal of a diagonal pair, skips both phases for that block
// (wave-uniform).  At the end every wave writes the tiles of its block that lie on or above the diagonal to the workgroup's
// partial block; k_gram64_reduce adds the ranges' blocks in their order, applies the factor the records' weights carry to rows
// and columns (fd_pack.h weight_scale64), undoes the multilayer records' centre-major order, writes exactly 0.0 for rows and
// columns of polynomial terms the model lacks and mirrors the upper triangle into the lower.  No atomics: the ranges are a
// function of N and C alone (gram_ranges), so the same inputs give the same bits.  Everything is fp64; built with
// -ffp-contract=off like fd_adjoint.hip: every fused multiply-add is written out.
#include "fd_operator.h"

namespace fd {

namespace {

constexpr int kBlock = 256;
constexpr int kPanel = 128;                  // columns of a panel: 8 tiles, two 4-tile blocks
constexpr int kSuper = 256;                  // vertices whose x and q are formed at a time
constexpr int kChunk = 32;                   // vertices staged through LDS per contraction (8 MFMA depths)
constexpr int kRow = 2 * kPanel + 16;        // doubles per staged vertex row

using packing::phi_grad64;
typedef double double4_t __attribute__((ext_vector_type(4)));

struct GramParams {
    int64_t N;
    const float *P, *omega, *dist2;
    const float *tu, *tv, *nrm;          // projection frames (all or none)
    float radius2, falloffrate;
    int C;                               // records (fd_model_centres)
    int nt;                              // 16 x 16 tiles per side, ceil((C + 4) / 16)
    int nq;                              // 1, or 6 with projection frames
    int64_t per;                         // vertices per range, a multiple of kSuper
    const Rec64 *rec64;
    const DevModel *model;
    double *partial;                     // [range][q][16 nt][16 nt]
};

// the component (b, c) of q = 0..5: xx, xy, xz, yy, yz, zz
__device__ __forceinline__ void component(int q, int &b, int &c)
{
    b = q < 3 ? 0 : (q < 5 ? 1 : 2);
    c = q < 3 ? q : (q < 5 ? q - 2 : 2);
}

template <int KIND>
__device__ __forceinline__ void gram64_body(const GramParams &p)
{
    __shared__ __attribute__((aligned(16))) double s_psi[kChunk][kRow];
    __shared__ __attribute__((aligned(16))) double s_v[kSuper][4];     // {x, q} of the super-tile's vertices
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g = lane >> 4;
    const bool built = p.model->terminationtype == 1;
    const bool proj = p.tu != nullptr;
    const int n = p.C + 4;

    // the panel pair of this workgroup: pairs in the order (0,0), (0,1), .., (0,np-1), (1,1), ..
    const int np = (p.nt + 7) / 8;
    int pi = 0, pj = (int)blockIdx.y;
    while (pj >= np - pi) { pj -= np - pi; ++pi; }
    pj += pi;
    const bool diag = pi == pj;
    int qb = 0, qc = 0;
    component((int)blockIdx.z, qb, qc);

    // form: the staged column of this thread
    const int half = tid >> 7;
    const int gcol = (half ? pj : pi) * kPanel + (tid & (kPanel - 1));
    const bool form = !(diag && half) && (gcol & ~63) < n;             // wave-uniform: 64 columns per wave, one block
    const int type = gcol < p.C ? 0 : (gcol < n ? 1 + gcol - p.C : 5);  // 0 a centre; 1..4 the columns 1, x, y, z; 5 nothing
    const Rec64 &rec = p.rec64[gcol < p.C ? gcol : p.C - 1];
    const double cx = rec.cx, cy = rec.cy, cz = rec.cz, cs = rec.s;

    // contract: the 4 x 4 tile block of this wave
    const int bi = wave >> 1, bj = wave & 1;
    const int tr0 = pi * 8 + bi * 4, tc0 = pj * 8 + bj * 4;
    const bool work = tr0 < p.nt && tc0 < p.nt && !(diag && bi > bj);  // wave-uniform
    const int acol = bi * 64 + c16, bcol = (diag ? 0 : kPanel) + bj * 64 + c16;
    double4_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};

    const int64_t v0 = (int64_t)blockIdx.x * p.per;
    const int64_t v1 = v0 + p.per < p.N ? v0 + p.per : p.N;
    for (int64_t base = v0; base < v1; base += kSuper) {
        const int64_t i = base + tid;
        const int64_t ic = i < p.N ? i : p.N - 1;
        double x[3] = {(double)p.P[3 * ic], (double)p.P[3 * ic + 1], (double)p.P[3 * ic + 2]};
        const float d2f = p.dist2 ? p.dist2[ic] : 0.f;
        const float wf = p.omega ? p.omega[ic] : 1.f;
        const double f = (double)transport::falloff(p.dist2 != nullptr, p.radius2, p.falloffrate, d2f);
        // what the forward map moves and the sum weighs: in range, not gated, model built, f != 0, omega != 0
        const bool live = (i < v1) && !(d2f > p.radius2) && built && f != 0.0 && wf != 0.f;
        double q = (double)wf * (f * f);
        if (proj) {
            // Pi = a1 a1^T + a2 a2^T with the forward path's axes; a1, a2 are not orthogonal, so Pi^2 != Pi
            double a1[3], a2[3];
            transport::axes<double>(p.tu, p.tv, p.nrm, ic, a1, a2);
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double pbk = fma(a1[qb], a1[k], a2[qb] * a2[k]);
                const double pkc = fma(a1[k], a1[qc], a2[k] * a2[qc]);
                s = fma(pbk, pkc, s);
            }
            q = q * s;
        }
        // a select, not a product: a vertex that is out contributes exactly nothing whatever P or omega hold there
        q = live ? q : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = live ? x[c] : 0.0;
        __syncthreads();                                               // the previous super-tile's chunks are done
        s_v[tid][0] = x[0]; s_v[tid][1] = x[1]; s_v[tid][2] = x[2]; s_v[tid][3] = q;
        __syncthreads();
        const int64_t left = v1 - base;
        const int nv = left < kSuper ? (int)left : kSuper;
        for (int cv = 0; cv < nv; cv += kChunk) {
            if (form) {
#pragma unroll 4
                for (int v = 0; v < kChunk; ++v) {
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
                    s_psi[v][tid] = val;
                }
            }
            __syncthreads();
            if (work) {
#pragma unroll 2
                for (int ks = 0; ks < kChunk / 4; ++ks) {
                    const int v = ks * 4 + g;
                    const double qv = s_v[cv + v][3];
                    double A[4], B[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) { A[a] = s_psi[v][acol + 16 * a] * qv; B[a] = s_psi[v][bcol + 16 * a]; }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[a], B[b], acc[a][b], 0, 0, 0);
                }
            }
            __syncthreads();                                           // s_psi may be overwritten
        }
    }

    if (!work) return;
    // accumulator register r of lane (c16, g) is entry (g + 4 r, c16) of its tile: row = the first operand's index
    const int ld = 16 * p.nt;
    double *out = p.partial + ((size_t)blockIdx.x * p.nq + blockIdx.z) * (size_t)ld * ld;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int tr = tr0 + a, tc = tc0 + b;
            if (tr >= p.nt || tc >= p.nt || tr > tc) continue;         // wave-uniform
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(16 * tr + g + 4 * r) * ld + 16 * tc + c16] = acc[a][b][r];
        }
    }
}

// k_gram64_<kind> and k_gram64_launch
FD_OP_KERNELS(k_gram64_, , (kBlock), GramParams, gram64_body<KIND>(p))

// The ranges' blocks added in their order, the same for every call with this N and C: one thread per entry j <= k of one
// component.  Record position `j` of a multilayer model (centre-major, fd_pack.h) goes back to its row of W (layer-major);
// `wscale` is the factor between W and the records' weights, applied once per record index; + 0.0 keeps an empty sum at +0
// under a negative factor.  The entry and its mirror are written from the same register.
__global__ __launch_bounds__(kBlock) void k_gram64_reduce(const double *partial, int nranges, int nq, int nt, int C, int layers,
                                                          int T, double wscale, double *H)
{
    const int n = C + 4;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (int64_t)nq * n * n) return;
    const int q = (int)(e / ((int64_t)n * n));
    const int j = (int)((e / n) % n), k = (int)(e % n);
    if (j > k) return;
    const size_t ld = (size_t)16 * nt;
    const double *src = partial + (size_t)q * ld * ld + (size_t)j * ld + k;
    const size_t stride = (size_t)nq * ld * ld;
    double sum = 0.0;
#pragma unroll 8
    for (int r = 0; r < nranges; ++r) sum += src[(size_t)r * stride];
    const bool lacking = (j >= C && j - C >= T) || (k >= C && k - C >= T);
    const double sc = (j < C ? wscale : 1.0) * (k < C ? wscale : 1.0);
    const double val = lacking ? 0.0 : sc * sum + 0.0;
    int jo = j, ko = k;
    if (layers > 1) {
        const int Mc = C / layers;
        if (j < C) jo = (j % layers) * Mc + j / layers;
        if (k < C) ko = (k % layers) * Mc + k / layers;
    }
    double *Hq = H + (size_t)q * n * n;
    Hq[(size_t)jo * n + ko] = val;
    Hq[(size_t)ko * n + jo] = val;
}

// (a range's block: all six components)
int64_t gram_per(int64_t N, int C)
{
    const size_t ld = op::padded_rows(C);
    return op::range_per(N, 6 * ld * ld * sizeof(double), kSuper);
}

}  // namespace

int gram_ranges(int64_t N, int C) { return op::range_count(N, gram_per(N, C)); }

size_t gram_partial_doubles(int64_t N, int C, int nq)
{
    const size_t ld = op::padded_rows(C);
    return (size_t)gram_ranges(N, C) * (size_t)nq * ld * ld;
}

hipError_t launch_gram(const DeformArgs &a, const GramArgs &g, hipStream_t stream)
{
    const int ranges = gram_ranges(a.N, a.M);
    const int nq = a.tu ? 6 : 1;
    const int nt = (a.M + 4 + 15) / 16;
    if (ranges > 0) {
        GramParams p;
        op::fill_mesh(p, a);
        p.P = a.P_in; p.omega = g.omega;
        p.C = a.M; p.nt = nt; p.nq = nq;
        p.per = gram_per(a.N, a.M);
        p.rec64 = a.rec64; p.model = a.model;
        p.partial = g.partial;
        const int np = (nt + 7) / 8;
        const dim3 grid((unsigned)ranges, (unsigned)(np * (np + 1) / 2), (unsigned)nq);
        const hipError_t e = k_gram64_launch(a.kind, grid, stream, p);
        if (e != hipSuccess) return e;
    }
    const int64_t entries = (int64_t)nq * (a.M + 4) * (a.M + 4);
    hipLaunchKernelGGL(k_gram64_reduce, dim3((unsigned)((entries + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                       (const double *)g.partial, ranges, nq, nt, a.M, a.layers, g.T, packing::weight_scale64(a.kind), g.H);
    return hipGetLastError();
}

}  // namespace fd
