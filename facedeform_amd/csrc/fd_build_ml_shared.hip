// fd_build_ml_shared.hip -- a shot of multilayer models built from ONE factorisation per layer
// (fd_batch_set_shared_factor on a batch of FD_KERNEL_GAUSSIAN_ML contexts).
//
// Phi_l + lambda I depends on the rest rig, R, lambda and l alone: the frames of a shot differ in
// their right-hand sides only.  launch_build_ml_shared (fd_nullspace.hip) factorises the L layer
// matrices once, side by side, into scratch slots of the batch (the ordinary kernels, blockIdx.z =
// layer); this file holds what is new:
//
//   k_ml_shared_init    fills the scratch slot table (slot l: its own A, solver state and DevModel,
//                       context 0's centres, radii offset to layer l) and resets its status words
//   k_ml_solve_shared   every frame's three right-hand sides through those factors in one launch.
//                       The 3 F columns are cut into tiles of 16; one workgroup per tile keeps its
//                       npc x 16 fp64 block in LDS for the whole chain: deltas in, least-squares
//                       polynomial removed (k_ml_affine's arithmetic, per column), then per layer
//                       L y = r and L^T w = y in 32-row blocks -- the diagonal step a product with
//                       the stored inverse block, the update of the other rows rank-32 products on
//                       v_mfma_f64_16x16x4_f64, right-looking, the row tiles dealt to the four
//                       waves (no sum crosses a wave) with the next tile's piece of L in flight
//                       under the current one -- w into the owning context's W, lambda w on.
//   k_ml_shared_flags   what the factorisations reported, into every frame's DevModel
//
// No atomics, fixed summation orders: the same inputs give the same bits on every call.
#include "fd_internal.h"
#include "fd_eval_common.h"

namespace fd {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

// one 128-VGPR slot: this runs beside evaluation launches (see fd_nullspace.hip)
#define FD_FIT_BESIDE_EVAL __attribute__((amdgpu_waves_per_eu(4, 8)))

constexpr int kTile = 16;               // right-hand-side columns per workgroup: one MFMA tile
constexpr int kNB = 32;                 // the Cholesky block width of fd_nullspace.hip
constexpr int kMaxM = 1024;             // 128 M bytes of LDS per workgroup
constexpr int kMinFrames = 2;           // fewer frames: the per-context chain

struct SolveArgs {
    const BatchSlot *frames;            // the contexts' table
    const BatchSlot *layers;            // the scratch table: slot l holds the factor of layer l
    int M, T, L, nF, npc, lda;
    double lambda;
    MlSharedLayout at;
};

__global__ void k_ml_shared_init(const BatchSlot *frames, BatchSlot *layers, DevModel *models, double *ns, size_t ns_stride,
                                 double *A, size_t a_stride, int M, int npad, int lda)
{
    const int l = blockIdx.z;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double *Al = A + (size_t)l * a_stride;
    if (i == 0) {
        BatchSlot s = frames[0];
        s.radii = s.radii + (size_t)l * M;
        s.A = Al;
        s.ns = ns + (size_t)l * ns_stride;
        s.model = models + l;
        s.host_status = nullptr;
        layers[l] = s;
        DevModel *m = models + l;
        m->terminationtype = 0;
        m->dup_flag = 0;
        m->sing_flag = 0;
        m->iterations = 0;
        m->amax_bits = 0ull;
        m->pivmin_bits = 0x7FF0000000000000ull;  // +inf
        m->pivmax_bits = 0ull;
    }
    // the factorisation carries the right-hand-side columns along: zeros here, and in the 16 columns past them
    if (i < lda)
        for (int c = 0; c < kRhsCols + 16; ++c) Al[(size_t)(npad + c) * lda + i] = 0.0;
}

__global__ void k_ml_shared_flags(const BatchSlot *frames, const BatchSlot *layers, int nF, int L)
{
    const int f = threadIdx.x;
    if (f >= nF) return;
    DevModel *m = frames[f].model;
    int dup = m->dup_flag, sing = m->sing_flag;
    unsigned long long amax = m->amax_bits, pmin = m->pivmin_bits, pmax = m->pivmax_bits;    // non-negative doubles: ordered as their bits
    for (int l = 0; l < L; ++l) {
        const DevModel *s = layers[l].model;
        dup |= s->dup_flag;
        sing |= s->sing_flag;
        amax = s->amax_bits > amax ? s->amax_bits : amax;
        pmin = s->pivmin_bits < pmin ? s->pivmin_bits : pmin;
        pmax = s->pivmax_bits > pmax ? s->pivmax_bits : pmax;
    }
    m->dup_flag = dup; m->sing_flag = sing;
    m->amax_bits = amax; m->pivmin_bits = pmin; m->pivmax_bits = pmax;
    m->iterations = layers[L - 1].model->iterations;       // as the per-context chain leaves it: the last layer's
}

// the eight A operands of one 16-row tile against a 32-column block: -op[c][g + 4 s], element (row, col) at base[col * lda + row].
// `base` is wave-uniform (column kb, row 0), the lane's part a 32-bit offset: scalar base + one address register per load
__device__ __forceinline__ void load_ops(double (&a)[8], gcdouble *base, int lda, unsigned lane_off)
{
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = -(base + (size_t)(4 * s) * lda)[lane_off];
}

// rows r0 .. r0+15 of the block take the contribution of the 32 solved rows whose values wait in yb (B operands)
__device__ __forceinline__ void update_tile(double *Bs, int r0, int c, int g, const double (&a)[8], const double (&yb)[8])
{
    double *p = Bs + (size_t)(r0 + g) * kTile + c;
    double4_t acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = p[4 * r * kTile];
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], yb[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) p[4 * r * kTile] = acc[r];
}

// wave 0: rows kb .. kb+31 of the block <- inverse(L11) (forward) or inverse(L11)^T (backward) times themselves.
// inv: row-major [k][j] = inverse(L11)[k][j], lower triangular -- the half that is zero is skipped.
__device__ __forceinline__ void diag_step(double *Bs, int kb, int c, int g, gcdouble *inv, bool transposed)
{
    double yb[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) yb[s] = Bs[(size_t)(kb + g + 4 * s) * kTile + c];
    double4_t acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            // forward: rows 0..15 see columns 0..15 only; backward: rows 16..31 see rows 16..31 of the inverse only
            if ((!transposed && t == 0 && s >= 4) || (transposed && t == 1 && s < 4)) continue;
            const unsigned at = transposed ? (unsigned)((g + 4 * s) * kNB + 16 * t + c) : (unsigned)((16 * t + c) * kNB + g + 4 * s);
            const double a = inv[at];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[s], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) Bs[(size_t)(kb + 16 * t + g + 4 * r) * kTile + c] = acc[t][r];
}

__global__ __launch_bounds__(256) FD_FIT_BESIDE_EVAL void k_ml_solve_shared(const SolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double Bs[];        // [npc][16]
    __shared__ double s_red[16 * kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int M = a.M, T = a.T, npc = a.npc, lda = a.lda;

    // fit and hand-off: thread (j, rg) owns column j of the tile in the rows rg, rg + 16, ...
    const int j = tid & 15, rg = tid >> 4;
    const int gc = (int)blockIdx.x * kTile + j;
    const bool live = gc < 3 * a.nF;
    const int f = live ? gc / 3 : 0, comp = live ? gc % 3 : 0;
    const BatchSlot &fs = a.frames[f];
    const float FD_GLOBAL *delta = as_global(fs.delta);
    gdouble *W = as_global(fs.W);
    const BatchSlot &s0 = a.layers[0];
    gcdouble *V = as_global(s0.ns), *small = V + (size_t)12 * M, *centres = as_global(s0.centres);

    for (int i = rg; i < npc; i += 16) Bs[(size_t)i * kTile + j] = (live && i < M) ? (double)delta[3 * (size_t)i + comp] : 0.0;
    if (T > 0) {
        // Q^T f through the shared reflectors, in place; the polynomial from its pivot rows; then f - P a from the deltas anew
        for (int k = 0; k < T; ++k) {
            const int piv = M - 1 - k;
            const double tau = small[a.at.tau + k];
            double d = 0.0;
            for (int i = rg; i <= piv; i += 16) d = fma(V[4 * (size_t)i + k], Bs[(size_t)i * kTile + j], d);
            s_red[rg * kTile + j] = d;
            __syncthreads();
            d = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) d += s_red[q * kTile + j];
            for (int i = rg; i <= piv; i += 16) Bs[(size_t)i * kTile + j] = fma(-tau * d, V[4 * (size_t)i + k], Bs[(size_t)i * kTile + j]);
            __syncthreads();
        }
        double pa[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = T - 1; k >= 0; --k) {
            if (M - 1 - k < 0) continue;
            double v = Bs[(size_t)(M - 1 - k) * kTile + j];
            for (int cc = k + 1; cc < T; ++cc) v = fma(-small[a.at.R + 4 * k + cc], pa[cc], v);
            pa[k] = v / small[a.at.R + 4 * k + k];
        }
        __syncthreads();                  // everyone has read the pivot rows
        for (int i = rg; i < M; i += 16) {
            const double px = centres[3 * (size_t)i], py = centres[3 * (size_t)i + 1], pz = centres[3 * (size_t)i + 2];
            double v = live ? (double)delta[3 * (size_t)i + comp] : 0.0;
            v -= fma(pa[3], pz, fma(pa[2], py, fma(pa[1], px, pa[0])));
            Bs[(size_t)i * kTile + j] = live ? v : 0.0;
        }
        if (live && rg == 0) {
            gdouble *mine = as_global(fs.ns) + (size_t)12 * M;      // where k_ml_finish looks for the polynomial
#pragma unroll
            for (int k = 0; k < 4; ++k) mine[a.at.aff + 3 * k + comp] = pa[k];
        }
    }
    __syncthreads();

    const unsigned goff = (unsigned)(g * lda + c);        // the lane's place in a 16-row, 4-column piece of L
    for (int l = 0; l < a.L; ++l) {
        const BatchSlot &sl = a.layers[l];
        gcdouble *A = as_global(sl.A);
        gcdouble *ld = as_global(sl.ns) + (size_t)12 * M + a.at.ld;

        // ---- L y = r, top down: block kb solved, the rows below it updated
#pragma unroll 1
        for (int kb = 0; kb < npc; kb += kNB) {
            const int nt = (npc - kb - kNB) / 16;             // row tiles below the block
            int t = wave;
            double an[8];
            if (t < nt) load_ops(an, A + (size_t)kb * lda, lda, goff + (unsigned)(kb + kNB + 16 * t));     // in flight under the diagonal step
            if (wave == 0) diag_step(Bs, kb, c, g, ld + (size_t)(kb / kNB) * a.at.ld_stride + a.at.ld_inv, false);
            __syncthreads();
            if (nt > 0) {
                double yb[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) yb[s] = Bs[(size_t)(kb + g + 4 * s) * kTile + c];
                while (t < nt) {
                    double ac[8];
#pragma unroll
                    for (int s = 0; s < 8; ++s) ac[s] = an[s];
                    const int tn = t + 4;
                    if (tn < nt) load_ops(an, A + (size_t)kb * lda, lda, goff + (unsigned)(kb + kNB + 16 * tn));
                    update_tile(Bs, kb + kNB + 16 * t, c, g, ac, yb);
                    t = tn;
                }
                __syncthreads();
            }
        }
        // ---- L^T w = y, bottom up: the rows above block kb read L^T from the mirrored upper triangle
#pragma unroll 1
        for (int kb = npc - kNB; kb >= 0; kb -= kNB) {
            const int nt = kb / 16;
            int t = wave;
            double an[8];
            if (t < nt) load_ops(an, A + (size_t)kb * lda, lda, goff + (unsigned)(16 * t));
            if (wave == 0) diag_step(Bs, kb, c, g, ld + (size_t)(kb / kNB) * a.at.ld_stride + a.at.ld_inv, true);
            __syncthreads();
            if (nt > 0) {
                double yb[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) yb[s] = Bs[(size_t)(kb + g + 4 * s) * kTile + c];
                while (t < nt) {
                    double ac[8];
#pragma unroll
                    for (int s = 0; s < 8; ++s) ac[s] = an[s];
                    const int tn = t + 4;
                    if (tn < nt) load_ops(an, A + (size_t)kb * lda, lda, goff + (unsigned)(16 * tn));
                    update_tile(Bs, 16 * t, c, g, ac, yb);
                    t = tn;
                }
                __syncthreads();
            }
        }
        // ---- layer l solved: its weights into the owning model (layer-major, as k_ml_layer writes them), lambda w_l on
        const bool last = l + 1 == a.L;
        for (int i = rg; i < M; i += 16) {
            const double w = Bs[(size_t)i * kTile + j];
            if (live) W[3 * ((size_t)l * M + i) + comp] = w;
            if (!last) Bs[(size_t)i * kTile + j] = a.lambda * w;
        }
        __syncthreads();
    }
}

LdsAttrOnce g_lds_once;

}  // namespace

int ml_shared_min_frames() { return kMinFrames; }

bool ml_shared_applies(int M, int layers, int frames)
{
    return M > 0 && M <= kMaxM && layers >= 1 && layers <= kMaxLayers && frames >= kMinFrames && frames <= kMaxBatch;
}

const char *ml_shared_kernel_name(int M, int layers, int frames) { return ml_shared_applies(M, layers, frames) ? "k_ml_solve_shared" : ""; }

hipError_t ml_shared_init()
{
    return g_lds_once.ensure((const void *)k_ml_solve_shared, (int)(sizeof(double) * kTile * kMaxM));
}

// scratch: the slot table, the slots' DevModels, then per layer the solver state and the matrix
static size_t table_bytes() { return (sizeof(BatchSlot) * kMaxLayers + 255) & ~(size_t)255; }
static size_t models_bytes() { return (sizeof(DevModel) * kMaxLayers + 255) & ~(size_t)255; }
static size_t ns_stride(int M) { return (ns_doubles(M) + 31) & ~(size_t)31; }
static size_t a_stride(const BuildBuffers &b) { return (size_t)b.lda * (size_t)(b.ncols + 16); }

size_t ml_shared_scratch_bytes(const BuildBuffers &b)
{
    return table_bytes() + models_bytes() + sizeof(double) * (size_t)b.ml_layers * (ns_stride(b.M) + a_stride(b));
}

const BatchSlot *ml_shared_slots(void *scratch) { return (const BatchSlot *)scratch; }

hipError_t launch_ml_shared_init(const BuildBuffers &b, hipStream_t stream, void *scratch)
{
    char *p = (char *)scratch;
    BatchSlot *layers = (BatchSlot *)p;
    DevModel *models = (DevModel *)(p + table_bytes());
    double *ns = (double *)(p + table_bytes() + models_bytes());
    double *A = ns + (size_t)b.ml_layers * ns_stride(b.M);
    hipLaunchKernelGGL(k_ml_shared_init, dim3((unsigned)(b.lda + 255) / 256, 1, (unsigned)b.ml_layers), dim3(256), 0, stream, b.d_slots,
                       layers, models, ns, ns_stride(b.M), A, a_stride(b), b.M, b.npad, b.lda);
    return hipGetLastError();
}

hipError_t launch_ml_solve_shared(const BuildBuffers &b, hipStream_t stream, void *scratch, const MlSharedLayout &at)
{
    SolveArgs a;
    a.frames = b.d_slots;
    a.layers = ml_shared_slots(scratch);
    a.M = b.M; a.T = b.T; a.L = b.ml_layers; a.nF = b.nbatch;
    a.npc = round_up(b.M, kNB);
    a.lda = b.lda;
    a.lambda = b.lambda;
    a.at = at;
    const unsigned tiles = (unsigned)(3 * b.nbatch + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_ml_solve_shared, dim3(tiles), dim3(256), sizeof(double) * kTile * (size_t)a.npc, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ml_shared_flags, dim3(1), dim3(kMaxBatch), 0, stream, b.d_slots, a.layers, b.nbatch, b.ml_layers);
    return hipGetLastError();
}

}  // namespace fd
