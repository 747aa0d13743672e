// fd_bake.hip -- the deformer baked per vertex (fd_deform_bake*): B[v][i] = f_v sum_j Psi_vj S_ji, the influence of control
// point i on vertex v (include/facedeform_hip.h states the contract).  One N x (C + 4) x M product in fp64 on
// v_mfma_f64_16x16x4_f64 with phi formed on the fly: k_deform64_shared's shape (fd_eval_shared64.hip) with S in the place of
// the frames' weights.  The layout both kernels agree on is fd_bake_plan.h's.
//
// Two kernels:
//   k_bake_pack      the only reader of S.  Writes, into scratch of the context: the centre records {cx, cy, cz, s}, four per
//                    depth step, and S in operand-tile order -- rows permuted into the records' order (the multilayer model:
//                    centre-major <- layer-major) and scaled by weight_scale64(kind), which is exact (0.5, -1 or 1); the four
//                    polynomial rows as one more K = 4 step, exactly 0.0 for rows the term lacks; columns padded to 16 and rows
//                    to 4 with 0.0.
//   k_bake64_<kind>  (and k_bake64_<kind>_narrow: 4 accumulator tiles for rigs of up to 64 points, else the same text.)
//                    Eight waves per workgroup; a wave owns a tile of 16 vertices.  Lane (g, j) = (lane >> 4, lane & 15) holds
//                    vertex j and, per depth step, forms phi of record 4 ks + g -- or 1, x, y, z in the last step -- which IS
//                    the first operand's layout: no exchange between lanes.  The second operand is one double per lane and
//                    tile from LDS (row 4 ks + g, column lane & 15), read without bank conflicts, shared by the eight waves:
//                    the workgroup stages S in chunks of depth steps, accumulators live across them.  A panel of up to 256
//                    columns is 16 accumulator tiles (128 registers); M > 256 loops over panels and forms phi again per panel.
//                    Epilogue: accumulator register r of lane (g, j) is vertex g + 4 r, column j of its tile; f and the gate of
//                    that vertex come by a lane shuffle; one fp64 multiply by f or the zero select, then B and / or
//                    B32 = (float)B: sixteen lanes write sixteen consecutive columns, a whole 128-byte run of a row of B.
//   k_bake_grad64_<kind>  the same product differentiated once in x (fd_deform_bake_grad*): three first operands
//                    per depth step, three accumulators per tile, panels of 4 tiles; stated where it stands, below.
// The pack kernel serves both: it takes the panel cap of the launch that will read its scratch.
// No atomics, no partial blocks: the sum over C + 4 lives in one accumulator, in an order that depends on nothing but the
// model.  A vertex's bits depend on its own inputs, the model and S alone.  Built with -ffp-contract=off like the rest.
#include "fd_bake_plan.h"
#include "fd_operator.h"

namespace fd {

namespace {

constexpr int kBlock = bake::kBlock;

using packing::phi_grad64;
typedef double double4_t __attribute__((ext_vector_type(4)));

// one thread per double of the scratch
__global__ __launch_bounds__(bake::kPackThreads) void k_bake_pack(const Rec64 *rec64, const double *S, double *scratch, int C, int M,
                                                                  int layers, int T, double wscale, int cap)
{
    const bake::Plan pl = bake::plan(C, M, cap);
    const size_t idx = (size_t)blockIdx.x * bake::kPackThreads + threadIdx.x;
    if (idx >= pl.doubles()) return;
    if (idx < pl.cen_doubles()) {
        const int rec = (int)(idx >> 2), e = (int)(idx & 3);
        double v = 0.0;
        if (rec < C) {
            const Rec64 &r = rec64[rec];
            v = e == 0 ? r.cx : e == 1 ? r.cy : e == 2 ? r.cz : r.s;
        }
        scratch[idx] = v;
        return;
    }
    const size_t q = idx - pl.cen_doubles();
    const int lane = (int)(q & 63);
    const size_t t = q >> 6;
    const int tile = (int)(t % pl.ntp);
    const int step = (int)((t / pl.ntp) % pl.steps);
    const int panel = (int)(t / pl.ntp / pl.steps);
    const int g = lane >> 4;
    const int col = (panel * pl.ntp + tile) * 16 + (lane & 15);
    double v = 0.0;
    if (col < M) {
        if (step < pl.steps - 1) {
            const int rec = 4 * step + g;
            if (rec < C) {
                int row = rec;                                          // record position -> row of W (fd_operator.h store_row)
                if (layers > 1) { const int Mc = C / layers; row = (rec % layers) * Mc + rec / layers; }
                v = wscale * S[(size_t)row * M + col];
            }
        } else if (g < T) {
            v = S[(size_t)(C + g) * M + col];
        }
    }
    scratch[idx] = v;
}

struct BakeParams : op::Mesh {
    int C, M;
    const double *scratch;               // fd_bake_plan.h
    const DevModel *model;
    double *B;                           // N x M (the gradient launch: N x 3 x M), or null
    float *B32;                          // the same in fp32, or null
};

template <int KIND, int NT>
__device__ __forceinline__ void bake64_body(const BakeParams &p)
{
    __shared__ __attribute__((aligned(16))) double s_buf[bake::lds_doubles<NT>()];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    const bake::Plan pl = bake::plan(p.C, p.M);
    const int ntp = pl.ntp;                                              // <= NT (the host picks NT)
    const int sd = pl.step_doubles();
    const int kchunk = bake::lds_doubles<NT>() / sd;                     // depth steps staged at a time
    double *s_cen = s_buf, *s_w = s_buf + 16 * kchunk;

    // this lane's vertex: x and f by the forward path's gate and fall-off; out by a select, whatever P holds there
    const bool built = p.model->terminationtype == 1;
    const int64_t base = ((int64_t)blockIdx.x * bake::kWaves + wave) * bake::kTile;
    const int64_t i = base + j;
    const int64_t ic = i < p.N ? i : p.N - 1;
    double x[3], f;
    const bool live = op::vertex(p, i, ic, p.N, built, x, f) && f != 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = live ? x[c] : 0.0;
    const bool work = __any(live);                                       // wave-uniform
    // the vertices this lane's accumulator registers belong to: g + 4 r
    double fr[4];
    bool lr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        fr[r] = __shfl(f, g + 4 * r);
        lr[r] = __shfl((int)live, g + 4 * r) != 0;
    }

    for (int panel = 0; panel < pl.panels; ++panel) {
        double4_t acc[NT];
#pragma unroll
        for (int T = 0; T < NT; ++T) acc[T] = double4_t{0.0, 0.0, 0.0, 0.0};

        for (int ks0 = 0; ks0 < pl.steps; ks0 += kchunk) {
            const int nk = pl.steps - ks0 < kchunk ? pl.steps - ks0 : kchunk;
            __syncthreads();                                             // the previous chunk has been read
            {
                const double *csrc = p.scratch + (size_t)16 * ks0;
                for (int q = tid; q < 16 * nk; q += kBlock) s_cen[q] = csrc[q];
                const double *wsrc = p.scratch + pl.tile_at(panel, ks0, 0);
                const int nw = nk * ntp * 64;
                for (int q = tid; q < nw; q += kBlock) s_w[q] = wsrc[q];
            }
            __syncthreads();
            if (!work) continue;
            for (int ks = 0; ks < nk; ++ks) {
                double a;
                if (ks0 + ks < pl.steps - 1) {                           // wave-uniform: a step of records
                    const double *cr = s_cen + 16 * ks + 4 * g;
                    const double dx = x[0] - cr[0], dy = x[1] - cr[1], dz = x[2] - cr[2];
                    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                    double gr;
                    phi_grad64<KIND>(d2, cr[3], a, gr);
                    (void)gr;
                } else {                                                 // the polynomial step: 1, x, y, z
                    a = g == 0 ? 1.0 : (g == 1 ? x[0] : (g == 2 ? x[1] : x[2]));
                }
                const double *wk = s_w + (size_t)ks * ntp * 64 + lane;
#pragma unroll
                for (int T = 0; T < NT; ++T)
                    if (T < ntp) acc[T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wk[T * 64], acc[T], 0, 0, 0);
            }
        }

        // ---- epilogue: register r of tile T is (vertex g + 4 r, column j of the tile)
#pragma unroll
        for (int T = 0; T < NT; ++T) {
            if (T >= ntp) continue;                                      // wave-uniform
            const int col = (panel * ntp + T) * 16 + j;
            if (col >= p.M) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = base + g + 4 * r;
                if (row >= p.N) continue;
                const double val = lr[r] ? acc[T][r] * fr[r] : 0.0;      // a select, not a product
                const size_t at = (size_t)row * (size_t)p.M + col;
                if (p.B) p.B[at] = val;
                if (p.B32) p.B32[at] = (float)val;
            }
        }
    }
}

// k_bake64_<kind> / k_bake64_launch, and k_bake64_<kind>_narrow / k_bake64_launch_narrow
FD_OP_KERNELS(k_bake64_, , (kBlock), BakeParams, bake64_body<KIND, bake::kPanelTiles>(p))
FD_OP_KERNELS(k_bake64_, _narrow, (kBlock), BakeParams, bake64_body<KIND, 4>(p))

// ---- the gradient: G[v][a][i] = f_v sum_j dPsi_vj/dx_a S_ji (fd_deform_bake_grad*) ----------------------------
// bake64_body with three first operands per depth step -- a_c = grad_scale64 g (x - c)_c, g of phi_grad64 (the phi is dropped);
// the polynomial step's are the unit vectors: d/dx_c of 1, x, y, z -- and three accumulators per tile: one LDS read of S' feeds
// three MFMAs.  Panels of kGradPanelTiles tiles (96 accumulator registers).  The epilogue is the bake's, three times, into rows
// 3 v + a of G.
constexpr int kGradTiles = bake::kGradPanelTiles;

template <int KIND>
__device__ __forceinline__ void bake_grad64_body(const BakeParams &p)
{
    constexpr int NT = kGradTiles;
    __shared__ __attribute__((aligned(16))) double s_buf[bake::lds_doubles<NT>()];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    const bake::Plan pl = bake::plan(p.C, p.M, NT);
    const int ntp = pl.ntp;                                              // <= NT
    const int sd = pl.step_doubles();
    const int kchunk = bake::lds_doubles<NT>() / sd;                     // depth steps staged at a time
    double *s_cen = s_buf, *s_w = s_buf + 16 * kchunk;
    constexpr double gs = packing::grad_scale64(KIND);

    // this lane's vertex: x and f by the forward path's gate and fall-off; out by a select, whatever P holds there
    const bool built = p.model->terminationtype == 1;
    const int64_t base = ((int64_t)blockIdx.x * bake::kWaves + wave) * bake::kTile;
    const int64_t i = base + j;
    const int64_t ic = i < p.N ? i : p.N - 1;
    double x[3], f;
    const bool live = op::vertex(p, i, ic, p.N, built, x, f) && f != 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = live ? x[c] : 0.0;
    const bool work = __any(live);                                       // wave-uniform
    // the vertices this lane's accumulator registers belong to: g + 4 r
    double fr[4];
    bool lr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        fr[r] = __shfl(f, g + 4 * r);
        lr[r] = __shfl((int)live, g + 4 * r) != 0;
    }

    for (int panel = 0; panel < pl.panels; ++panel) {
        double4_t acc[3][NT];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int T = 0; T < NT; ++T) acc[c][T] = double4_t{0.0, 0.0, 0.0, 0.0};

        for (int ks0 = 0; ks0 < pl.steps; ks0 += kchunk) {
            const int nk = pl.steps - ks0 < kchunk ? pl.steps - ks0 : kchunk;
            __syncthreads();                                             // the previous chunk has been read
            {
                const double *csrc = p.scratch + (size_t)16 * ks0;
                for (int q = tid; q < 16 * nk; q += kBlock) s_cen[q] = csrc[q];
                const double *wsrc = p.scratch + pl.tile_at(panel, ks0, 0);
                const int nw = nk * ntp * 64;
                for (int q = tid; q < nw; q += kBlock) s_w[q] = wsrc[q];
            }
            __syncthreads();
            if (!work) continue;
            for (int ks = 0; ks < nk; ++ks) {
                double a[3];
                if (ks0 + ks < pl.steps - 1) {                           // wave-uniform: a step of records
                    const double *cr = s_cen + 16 * ks + 4 * g;
                    const double dx = x[0] - cr[0], dy = x[1] - cr[1], dz = x[2] - cr[2];
                    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                    double ph, gr;
                    phi_grad64<KIND>(d2, cr[3], ph, gr);
                    (void)ph;
                    const double q = gs * gr;                            // grad phi = (grad_scale64 g) (x - c)
                    a[0] = q * dx; a[1] = q * dy; a[2] = q * dz;
                } else {                                                 // the polynomial step: d/dx_c of 1, x, y, z
#pragma unroll
                    for (int c = 0; c < 3; ++c) a[c] = g == c + 1 ? 1.0 : 0.0;
                }
                const double *wk = s_w + (size_t)ks * ntp * 64 + lane;
#pragma unroll
                for (int T = 0; T < NT; ++T) {
                    if (T >= ntp) continue;                              // wave-uniform
                    const double w = wk[T * 64];
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[c], w, acc[c][T], 0, 0, 0);
                }
            }
        }

        // ---- epilogue: register r of tile T, component c is (vertex g + 4 r, component c, column j of the tile)
#pragma unroll
        for (int T = 0; T < NT; ++T) {
            if (T >= ntp) continue;                                      // wave-uniform
            const int col = (panel * ntp + T) * 16 + j;
            if (col >= p.M) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = base + g + 4 * r;
                if (row >= p.N) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double val = lr[r] ? acc[c][T][r] * fr[r] : 0.0;   // a select, not a product
                    const size_t at = ((size_t)row * 3 + c) * (size_t)p.M + col;
                    if (p.B) p.B[at] = val;
                    if (p.B32) p.B32[at] = (float)val;
                }
            }
        }
    }
}

// k_bake_grad64_<kind> / k_bake_grad64_launch
FD_OP_KERNELS(k_bake_grad64_, , (kBlock), BakeParams, bake_grad64_body<KIND>(p))

// tiles of a panel at most, by the components per vertex and column (1: B; 3: G)
int panel_cap(int comps) { return comps == 1 ? bake::kPanelTiles : bake::kGradPanelTiles; }

}  // namespace

size_t bake_scratch_doubles(int C, int M, int comps) { return bake::plan(C, M, panel_cap(comps)).doubles(); }

int64_t bake_chunk_vertices(int M, int comps, bool b64, bool b32)
{
    const size_t row = (size_t)comps * (size_t)M * ((b64 ? sizeof(double) : 0) + (b32 ? sizeof(float) : 0));
    const int64_t groups = (int64_t)(op::kScratchBound / (row ? row : 1)) / bake::kGroup;
    return (groups < 1 ? 1 : groups) * bake::kGroup;
}

hipError_t launch_bake_pack(const DeformArgs &a, const BakeArgs &g, hipStream_t stream)
{
    const size_t n = bake_scratch_doubles(a.M, g.M, g.comps);
    hipLaunchKernelGGL(k_bake_pack, dim3((unsigned)((n + bake::kPackThreads - 1) / bake::kPackThreads)), dim3(bake::kPackThreads), 0,
                       stream, a.rec64, g.S, g.scratch, a.M, g.M, a.layers, g.T, packing::weight_scale64(a.kind), panel_cap(g.comps));
    return hipGetLastError();
}

hipError_t launch_bake(const DeformArgs &a, const BakeArgs &g, hipStream_t stream)
{
    if (a.N <= 0) return hipSuccess;
    BakeParams p = op::params_of<BakeParams>(a);
    p.C = a.M; p.M = g.M;
    p.scratch = g.scratch; p.model = a.model;
    p.B = g.B; p.B32 = g.B32;
    const dim3 grid((unsigned)((a.N + bake::kGroup - 1) / bake::kGroup));
    if (g.comps == bake::kGradComps) return k_bake_grad64_launch(a.kind, grid, stream, p);
    return bake::plan(a.M, g.M).ntp <= 4 ? k_bake64_launch_narrow(a.kind, grid, stream, p) : k_bake64_launch(a.kind, grid, stream, p);
}

}  // namespace fd
