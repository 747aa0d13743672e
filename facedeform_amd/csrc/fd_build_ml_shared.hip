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
//                       (Prologue, sweeps and tile products: fd_shared_solve.h, shared with the
//                       QNN model's k_qnn_solve_shared.)
//   k_ml_shared_flags   what the factorisations reported, into every frame's DevModel
//
// No atomics, fixed summation orders: the same inputs give the same bits on every call.
#include "fd_internal.h"
#include "fd_eval_common.h"
#include "fd_shared_solve.h"

namespace fd {

namespace {

using namespace shared_solve;          // what this kernel shares with k_qnn_solve_shared (fd_shared_solve.h)

constexpr int kMaxM = kMaxRows;         // 128 M bytes of LDS per workgroup
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
    hand_flags(frames[f].model, layers, L);       // (fd_shared_solve.h: the QNN model's shared build hands its one slot's on inside its solve kernel)
}

__global__ __launch_bounds__(256) FD_FIT_BESIDE_EVAL void k_ml_solve_shared(const SolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double Bs[];        // [npc][16]
    __shared__ double s_red[16 * kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int M = a.M, T = a.T, npc = a.npc, lda = a.lda;

    // fit and hand-off: thread (j, rg) owns column j of the tile in the rows rg, rg + 16, ...
    const Column o = own_column(tid, a.nF);
    const int j = o.j, rg = o.rg, comp = o.comp;
    const bool live = o.live;
    const BatchSlot &fs = a.frames[o.f];
    gdouble *W = as_global(fs.W);
    const BatchSlot &s0 = a.layers[0];
    gcdouble *V = as_global(s0.ns);

    // Q^T f through the shared reflectors, in place; the polynomial from its pivot rows; then f - P a from the deltas anew
    fit_polynomial(Bs, s_red, o, as_global(fs.delta), V, V + (size_t)12 * M, as_global(s0.centres), as_global(fs.ns) + (size_t)12 * M,
                   M, T, npc, a.at);

    for (int l = 0; l < a.L; ++l) {
        const BatchSlot &sl = a.layers[l];
        gcdouble *A = as_global(sl.A);
        gcdouble *inv = as_global(sl.ns) + (size_t)12 * M + a.at.ld + a.at.ld_inv;      // inverse(L11) of block 0

        // ---- L y = r, top down; L^T w = y, bottom up: the rows above a block read L^T from the mirrored upper triangle
        sweep_down(Bs, A, lda, npc, inv, (size_t)a.at.ld_stride, wave, c, g);
        sweep_up(Bs, A, lda, npc, inv, (size_t)a.at.ld_stride, wave, c, g);
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
