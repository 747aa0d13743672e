// fd_build_qnn_shared.hip -- a shot of QNN models built from ONE LU factorisation of the rest rig
// (fd_batch_set_shared_lu on a batch of FD_KERNEL_GAUSSIAN_QNN contexts).
//
// Phi + lambda I of the QNN model depends on the rest rig, q, z and lambda alone: the frames of a shot differ in their
// right-hand sides only.  launch_build_qnn_shared (fd_nullspace.hip) forms the reflectors of the polynomial block, assembles
// the kernel block and factorises it without pivot search ONCE, with the ordinary kernels, in a scratch slot of the batch;
// this file holds what is new:
//
//   k_qnn_shared_init     fills the scratch slot (its own A, solver state, DevModel, move lists and pivots on context 0's
//                         centres and radii) and resets its status words and move counts.  Launched when the slot has to
//                         be filled -- the first build, new scratch, contexts whose buffers moved, a build whose launches
//                         did not all go out -- and not otherwise: the solve kernel leaves the status words reset
//   k_qnn_shared_invert   the 32 x 32 diagonal blocks of the factor inverted, one 64-thread workgroup per block: lanes 0..31
//                         a column each of inverse(L11) (unit lower), lanes 32..63 a column each of inverse(U11), by
//                         substitution on e_j -- so that the solve's diagonal step is a matrix-pipe product, as it is
//                         for the Cholesky factors of the multilayer model
//   k_qnn_solve_shared    every frame's three right-hand sides through that factor in one launch.  The 3 F columns are cut
//                         into tiles of 16; one workgroup per tile keeps its rows x 16 fp64 block in LDS: deltas in,
//                         least-squares polynomial removed (k_ml_affine's arithmetic, per column), L y = r top down, U w = y
//                         bottom up in 32-row blocks (fd_shared_solve.h: the code k_ml_solve_shared runs), w into the owning
//                         context's X in the layout k_pack reads.  Its first workgroup also hands what the factorisation
//                         reported to every frame's DevModel (hand_flags, the body of k_ml_shared_flags with one slot)
//                         and resets the slot's own: the build of a lone system is a chain of short dependent
//                         launches, and every one counts.
//
// No atomics, fixed summation orders: the same inputs give the same bits on every call.
#include "fd_internal.h"
#include "fd_eval_common.h"
#include "fd_shared_solve.h"

namespace fd {

namespace {

using namespace shared_solve;

constexpr int kMaxOrderNp = 1024;       // the LU without pivot search: one row per thread of k_lu_panel_np
constexpr int kMinFrames = 2;           // fewer frames: the per-context chain
constexpr int kInvStride = 2 * kNB * kNB;   // per diagonal block: inverse(L11), then inverse(U11) transposed, both row-major lower triangles

struct QnnSolveArgs {
    const BatchSlot *frames;            // the contexts' table
    const BatchSlot *slot;              // the scratch slot: the factor
    const double *inv;                  // the inverted diagonal blocks
    int M, T, nF, rows, npad, lda;
    MlSharedLayout at;
};

// where the pieces of the scratch are, in bytes from its start
struct Layout {
    size_t model, ns, inv, ipiv, moves, A, total;
};
__host__ Layout layout_of(const BuildBuffers &b)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    Layout l;
    l.model = up(sizeof(BatchSlot));
    l.ns = l.model + up(sizeof(DevModel));
    l.inv = l.ns + up(sizeof(double) * ns_doubles(b.M));
    l.ipiv = l.inv + up(sizeof(double) * (size_t)(b.npad / kNB) * kInvStride);
    l.moves = l.ipiv + up(sizeof(int) * (size_t)b.npad);
    l.A = l.moves + up(sizeof(int) * (size_t)lu_step_capacity(b.npad) * kMovesStride);
    l.total = l.A + up(sizeof(double) * (size_t)b.lda * (size_t)(b.ncols + 16));
    return l;
}

// the slot's status words as a factorisation expects to find them
__device__ __forceinline__ void arm_flags(DevModel *model)
{
    model->terminationtype = 0;
    model->dup_flag = 0;
    model->sing_flag = 0;
    model->iterations = 0;
    model->amax_bits = 0ull;
    model->pivmin_bits = 0x7FF0000000000000ull;  // +inf
    model->pivmax_bits = 0ull;
}

__global__ void k_qnn_shared_init(const BatchSlot *frames, BatchSlot *slot, DevModel *model, double *ns, int *ipiv, int *moves,
                                  int nsteps, double *A)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        BatchSlot s = frames[0];          // context 0's centres and radii
        s.A = A;
        s.ns = ns;
        s.model = model;
        s.ipiv = ipiv;
        s.moves = moves;
        s.host_status = nullptr;
        slot[0] = s;
        arm_flags(model);
    }
    if (i < nsteps) moves[(size_t)i * kMovesStride] = 0;      // no interchanges, whatever step the update reads
    // (the factorisation of the slot carries no right-hand-side columns along -- launch_build_qnn_shared ends its matrix at
    //  column npad -- so the columns past it are never read and need no zeros)
}

__global__ __launch_bounds__(64) void k_qnn_shared_invert(const BatchSlot *slot, double *inv, int lda)
{
    const int kb = (int)blockIdx.x * kNB;
    gcdouble *A = as_global(slot[0].A);
    __shared__ double sA[kNB][kNB + 1];
    const int tid = threadIdx.x, j = tid & 31;
    for (int e = tid; e < kNB * kNB; e += 64) {
        const int r = e & 31, cc = e >> 5;
        sA[r][cc] = A[(size_t)(kb + cc) * lda + kb + r];
    }
    __syncthreads();
    gdouble *out = as_global(inv) + (size_t)blockIdx.x * kInvStride;
    double x[kNB];
    if (tid < 32) {
        // column j of inverse(L11): L11 x = e_j, unit diagonal; row-major [i][j]
#pragma unroll
        for (int i = 0; i < kNB; ++i) {
            double v = i == j ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) v = fma(-sA[i][k], x[k], v);
            x[i] = v;
        }
#pragma unroll
        for (int i = 0; i < kNB; ++i) out[i * kNB + j] = x[i];
    } else {
        // column j of inverse(U11): U11 x = e_j; stored transposed, [j][i], a lower triangle again
#pragma unroll
        for (int i = kNB - 1; i >= 0; --i) {
            double v = i == j ? 1.0 : 0.0;
#pragma unroll
            for (int k = i + 1; k < kNB; ++k) v = fma(-sA[i][k], x[k], v);
            x[i] = v / sA[i][i];
        }
#pragma unroll
        for (int i = 0; i < kNB; ++i) out[kNB * kNB + j * kNB + i] = x[i];
    }
}

__global__ __launch_bounds__(256) FD_FIT_BESIDE_EVAL void k_qnn_solve_shared(const QnnSolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double Bs[];        // [rows][16]
    __shared__ double s_red[16 * kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int M = a.M, rows = a.rows, npad = a.npad;

    const Column o = own_column(tid, a.nF);
    const BatchSlot &fs = a.frames[o.f];
    const BatchSlot &s0 = a.slot[0];
    gcdouble *V = as_global(s0.ns);
    gcdouble *A = as_global(s0.A);
    gcdouble *inv = as_global(a.inv);

    // Q^T f through the shared reflectors, in place; the polynomial from its pivot rows (into the owning frame's solver state,
    // where k_qnn_finish looks for it); then f - P a from the deltas anew
    fit_polynomial(Bs, s_red, o, as_global(fs.delta), V, V + (size_t)12 * M, as_global(s0.centres), as_global(fs.ns) + (size_t)12 * M,
                   M, a.T, rows, a.at);

    // L y = r with the unit-lower L below the diagonal of A, then U w = y with the U on and above it
    sweep_down(Bs, A, a.lda, rows, inv, (size_t)kInvStride, wave, c, g);
    sweep_up(Bs, A, a.lda, rows, inv + kNB * kNB, (size_t)kInvStride, wave, c, g);

    // the weights where the back-substitution of a per-context build leaves them: X[c * npad + j], zeros below row M
    // (k_qnn_finish puts the polynomial there)
    if (o.live) {
        gdouble *X = as_global(fs.X) + (size_t)o.comp * npad;
        for (int i = o.rg; i < npad; i += 16) X[i] = i < M ? Bs[(size_t)i * kTile + o.j] : 0.0;
    }
    if (blockIdx.x == 0) {
        if (tid < a.nF) hand_flags(a.frames[tid].model, a.slot, 1);
        __syncthreads();
        if (tid == 0) arm_flags(s0.model);        // ... and the slot is ready for the next build without k_qnn_shared_init
    }
}

LdsAttrOnce g_lds_once;

}  // namespace

int qnn_shared_min_frames() { return kMinFrames; }

bool qnn_shared_applies(int M, int frames)
{
    // (the order of the padded system is M + 4 rounded up to 32 with the linear term: every term fits below 1021 points)
    return M > 0 && round_up(M + 4, kNB) <= kMaxOrderNp && frames >= kMinFrames && frames <= kMaxBatch;
}

const char *qnn_shared_kernel_name(int M, int frames) { return qnn_shared_applies(M, frames) ? "k_qnn_solve_shared" : ""; }

hipError_t qnn_shared_init()
{
    return g_lds_once.ensure((const void *)k_qnn_solve_shared, (int)(sizeof(double) * kTile * kMaxRows));
}

size_t qnn_shared_scratch_bytes(const BuildBuffers &b) { return layout_of(b).total; }

const BatchSlot *qnn_shared_slot(void *scratch) { return (const BatchSlot *)scratch; }

hipError_t launch_qnn_shared_init(const BuildBuffers &b, hipStream_t stream, void *scratch)
{
    char *p = (char *)scratch;
    const Layout l = layout_of(b);
    const int nsteps = lu_step_capacity(b.npad);
    hipLaunchKernelGGL(k_qnn_shared_init, dim3((unsigned)(nsteps + 255) / 256), dim3(256), 0, stream, b.d_slots, (BatchSlot *)p,
                       (DevModel *)(p + l.model), (double *)(p + l.ns), (int *)(p + l.ipiv), (int *)(p + l.moves), nsteps,
                       (double *)(p + l.A));
    return hipGetLastError();
}

// behind the factorisation: the diagonal blocks inverted, all columns through the factor, its flags into every frame
hipError_t launch_qnn_solve_shared(const BuildBuffers &b, hipStream_t stream, void *scratch, const MlSharedLayout &at)
{
    char *p = (char *)scratch;
    const Layout l = layout_of(b);
    QnnSolveArgs a;
    a.frames = b.d_slots;
    a.slot = qnn_shared_slot(scratch);
    a.inv = (const double *)(p + l.inv);
    a.M = b.M; a.T = b.T; a.nF = b.nbatch;
    a.rows = round_up(b.M, kNB);
    a.npad = b.npad;
    a.lda = b.lda;
    a.at = at;
    if (a.rows > kMaxRows || a.rows > b.npad) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_qnn_shared_invert, dim3((unsigned)(a.rows / kNB)), dim3(64), 0, stream, a.slot, (double *)(p + l.inv), b.lda);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned tiles = (unsigned)(3 * b.nbatch + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_qnn_solve_shared, dim3(tiles), dim3(256), sizeof(double) * kTile * (size_t)a.rows, stream, a);
    return hipGetLastError();
}

}  // namespace fd
