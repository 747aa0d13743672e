// fd_capi.hip -- the C ABI of include/facedeform_hip.h over the HIP kernels.
// No CPU fallback anywhere: without a gfx950 device fd_create fails loudly.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <vector>

#include "fd_fit_host.h"
#include "fd_internal.h"
#include "fd_owned.h"
#include "fd_shared_plan.h"

using namespace fd;
using namespace fd_fit;

// what a captured build graph was made for (ensure_graph): another key captures again
struct GraphKey {
    int M, kind, term, nparams;       // term | the solver path's flags << 8
    double params[4];
    const void *A, *rest, *rec32;     // a single context's buffers (null for a batch: its graph reads the slot table)
};

struct fd_batch;
struct fd_ctx {
    int device = 0;
    Stream own_stream;                  // created on first use when the caller sets no stream; the first member: it outlives
                                        // everything that was enqueued on it
    hipStream_t stream_ = nullptr;          // fd_set_stream (borrowed); nullptr: own_stream
    int eval_precision = FD_EVAL_FP32;
    int eval_variant = 0;
    int output = FD_OUTPUT_POSITION;    // fd_set_output
    int solver = FD_SOLVER_AUTO;
    int imported_layers = 0;         // a multilayer model that came in through fd_import_model
    uint64_t rig_build_id = 0;       // nonzero: the id of the ONE batched build that read this context's rest rig, in place, from the same array as
                                     // its batch mates (their centres are equal by construction); 0: built on its own / from its own copy
    const float *rest_src = nullptr; // (borrowed) caller's device array the rest points were last read from in place (fd_batch_set_points_dev), else null
    bool prefer_lu = false;          // the Cholesky path lost definiteness on this rig: LU until kernel, term or M change
    unsigned long long model_gen = 0; // counts the models this context has held (every enqueued build, every import): what a
                                     // batch's packed copy of the weights is checked against before it is reused
    bool last_spd = false;           // the build in flight / last finished took the Cholesky path
    bool last_small = false;         // ... as k_build_small's one workgroup (otherwise, unless last_reg, the launch chain)
    bool last_nopivot = false;       // ... the LU without pivot search (QNN): a -4 from it is answered with the pivoted LU, like the Cholesky's
    bool last_reg = false;           // ... in its register-resident form (no factorisation is kept: fd_set_deltas builds again)

    // model configuration
    int M = 0, kind = FD_KERNEL_GAUSSIAN_QNN, term = FD_TERM_LINEAR, nparams = 0;
    double params[4] = {1.0, 5.0, 0.0, 0.0};
    bool points_set = false;
    bool build_pending = false;   // enqueued, status not read back yet
    bool built = false;           // status read back and == 1
    bool have_report = false;
    fd_report report{};
    // fd_set_deltas: a full build with the current rest points / kernel / term has been enqueued
    // (its factorisation sits in d_A), and the next build only has new right-hand sides
    bool have_factor = false;
    bool factor_grouped = false;   // the factorisation in d_A was built with grouped panels (a batched build)
    bool deltas_only = false;
    GraphExec resolve_exec;

    // device buffers (grow-only)
    int cap_M = 0;                // capacity in centres
    int cap_npad = 0;
    int cap_records = 0;             // centres / radii / weights / records: M, or M * layers for the multilayer model
    DevBuf<float> d_rest, d_delta;
    DevBuf<double> d_centres, d_radii, d_W;
    DevBuf<double> d_A, d_X;
    DevBuf<int> d_ipiv, d_moves;
    DevBuf<Rec32> d_rec32;
    DevBuf<Rec64> d_rec64;
    DevBuf<MfmaTile> d_tiles;
    DevBuf<MfmaTileH> d_tiles16;
    DevBuf<double> d_ns;             // null-space solver state (fd_nullspace.hip)
    DevBuf<DevModel> d_model;
    Pinned<DevModel> h_model;     // pinned mirror
    // where the build kernels find the buffers above: a one-entry device table (a single build
    // is a batch of one); re-uploaded whenever a buffer is reallocated
    DevBuf<BatchSlot> d_slot;
    BatchSlot h_slot{};
    uint64_t alloc_gen = 0;
    // set while the model comes from a batched build on another stream (fd_batch_build_async)
    // (borrowed: the batch's event, the stream the batch built on)
    hipEvent_t wait_event = nullptr;
    hipStream_t wait_stream = nullptr;
    struct fd_batch *wait_batch = nullptr;
    hipEvent_t tev0 = nullptr, tev_mid = nullptr, tev1 = nullptr;   // events the report's timings come from (borrowed: ev0 / ev_mid / ev1, or the batch's)
    Pinned<ModelHeader> h_header;     // pinned, for device-side export
    // Asynchronous status: after every enqueued build a one-thread kernel drops the model's
    // terminationtype into this page-locked word and status_ev is recorded behind it.  Every later
    // call on the context polls the event (no wait): a Cholesky that lost definiteness is then
    // rebuilt with the LU right away, on the stream, before whatever the call enqueues; a failure
    // the LU confirms becomes a sticky error that fd_deform* returns until the next set-up call.
    Pinned<int> h_status;
    int *d_status_alias = nullptr;      // (borrowed) the same word as the device sees it (looked up once: hipHostGetDevicePointer costs a runtime call per build)
    Event status_ev;
    hipEvent_t status_poll = nullptr;   // (borrowed) the event that says h_status is in: status_ev, or the one of the batch that built the model
    bool status_inflight = false;
    int sticky_rc = FD_OK;

    // staging for the host-pointer deform
    int64_t cap_N = 0;
    DevBuf<float> d_P, d_dist2, d_fall;
    DevBuf<float> d_tu, d_tv, d_nrm;
    // fd_deform_vectors: staging of the transported vectors + Jacobian (N x 18), and P_in set aside when it is overwritten.
    // This and the scratch buffers below grow by need (DevBuf::grow).
    DevBuf<float> d_vec, d_vecP;
    // fd_invert: staging of iters_out (residual_out goes through d_fall)
    DevBuf<int> d_iters;
    // fd_deform_adjoint*: the workgroups' partial blocks and, behind them, the host call's staging of grad_W (adjoint_scratch);
    // the host call's G goes through d_vecP
    DevBuf<double> d_adj;
    // fd_deform_adjoint_points: the host call's staging of grad_P (N x 3) and, behind it, grad_f (N); its G goes through d_vecP
    DevBuf<double> d_adjp;
    // fd_deform_gram*: the workgroups' partial blocks and, behind them, the host call's staging of H (gram_scratch); the host
    // call's omega goes through d_fall
    DevBuf<double> d_gram;
    // fd_deform_bake* and fd_deform_bake_grad*: the pack kernel's scratch (bake_scratch_doubles) and, behind it, the host call's
    // copy of S; the host call's vertex chunk of B (G) and, behind it, of B32 (G32) comes back through d_bakeout
    DevBuf<double> d_bake, d_bakeout;
    // fd_deform_adjoint_shot*: the ranges' partial blocks of one group of frames and, behind them, the host call's staging of
    // grad_W (adjoint_shot_scratch); the host call's G goes group by group through d_gshot
    DevBuf<double> d_adjs;
    DevBuf<float> d_gshot;
    // fd_fit_deltas_shot: a group's cotangents g_f = omega (T_f - P) on the host (malloc)
    size_t cap_hgshot = 0;
    float *h_gshot = nullptr;
    // fd_mesh_set: the mesh arrays that stay the same from cook to cook live in their own
    // device buffers (the staging above is evaluated in place, so it cannot serve as a cache)
    int64_t mesh_N = 0, mesh_cap = 0;
    bool mesh_has_dist2 = false, mesh_has_frames = false;
    DevBuf<float> m_P, m_dist2, m_tu, m_tv, m_nrm;
    DevBuf<float> m_out, m_fall;                    // result staging for pageable outputs

    Event ev0, ev_mid, ev1;

    // The build is ~25 dependent launches whose arguments depend only on the configuration
    // and on buffer addresses: captured once into a hipGraph, replayed on every later build.
    GraphExec build_exec;
    bool use_graph = true;
    GraphKey graph_key{}, resolve_key{};
    char err[512] = {0};
};

// Scratch of a one-launch shot call that keeps its own (fd_batch_deform_shared_fp64_dev, _ml_dev, _ml_fp64_dev; the vector call
// that goes with each reads it too), and the two events that order the contexts' models and the scratch around its launches.
struct ShotScratch {
    DevBuf<void> d;                      // what the call's pack kernel writes and its evaluation reads
    Event consumed_ev;                   // behind the last read of the contexts' models by that call (its pack kernel, or its per-context launches)
    bool consumed = false;               // ... and recorded: fd_batch_wait_consumed waits for it too
    Event eval_ev;                       // behind its last evaluation: the next pack kernel rewrites the scratch that one reads
    bool eval_pending = false;
};

struct fd_batch {
    int n = 0;
    int device = 0;
    fd_ctx *ctxs[kMaxBatch] = {};
    uint64_t gens[kMaxBatch] = {};
    DevBuf<BatchSlot> d_slots;
    PointSrc src{};
    bool have_src = false;
    Event ev0, ev_mid, ev1;
    GraphExec exec;
    bool use_graph = true;
    GraphKey key{};
    // a stream that already waits for the current build (set by the first evaluation that
    // needed it): the other contexts' evaluations on that stream need no wait of their own
    hipStream_t waited_stream = nullptr;    // (borrowed)
    Event status_ev;                    // behind the kernel that posts every context's status after a batched build
    // scratch of the shared-rig evaluation (fd_batch_deform_shared_dev): weight tiles + frame records
    // Two sets: the set a launch reads must not be rewritten by the pack kernel of the NEXT models before that launch
    // has finished -- with fd_batch_prepare_shared the next pack runs on the build stream, under the previous evaluation.
    struct SharedSet {
        DevBuf<void> d_wtiles, d_frames;
        Event packed_ev;                 // behind the pack kernel that filled the set
        Event eval_ev;                   // behind the last evaluation that read it
        hipEvent_t eval_done = nullptr;  // (borrowed) the event that says so: eval_ev, or -- a lean group call -- the batch's ev1, recorded right behind
        bool eval_pending = false;
    } sets[2];
    // "One rest rig" is decided on the host by the address the rest points were read from; an address does not identify
    // its contents (the array may have been rewritten, or freed and allocated again, between the set-ups of two contexts:
    // ADVICE r2), so the pack kernel compares every context's centres with context 0's ON THE DEVICE, passes a frame that
    // differs through like a failed build and posts 1 + its index here (page-locked); the next call on the batch reports it.
    Pinned<int> h_mismatch;
    int eval_cus = 0;                    // fd_batch_set_eval_cus: CUs a shared-rig evaluation may occupy (0: all)
    int shared_factor = 0;               // fd_batch_set_shared_factor: one factorisation per build where the contexts share the rest rig
    DevBuf<double> d_fac;                // ... and its scratch (reg_factor_doubles())
    int last_shared_factor = 0;          // the last build took that path
    DevBuf<void> d_mlfac;                // multilayer batches: the L layer factors' scratch (ml_shared_scratch_bytes), allocated at the first such build
    int shared_lu = 0;                   // fd_batch_set_shared_lu: QNN batches, one LU of the rest rig's kernel block per build
    DevBuf<void> d_qnnfac;               // ... and its scratch (qnn_shared_scratch_bytes), allocated at the first such build, grown by need
    bool qnn_slot_ready = false;         // the last shared build went out whole: its solve kernel left the scratch slot filled and reset
    int qnn_slot_M = 0, qnn_slot_npad = 0;   // ... for a system of these sizes (they decide where the slot's pieces lie in the scratch)
    int cur_set = 0;                     // the set packed last
    bool packed_valid = false;           // sets[cur_set].packed_ev is recorded (fd_batch_wait_consumed)
    bool prepared = false;               // sets[cur_set] holds the contexts' CURRENT models and prep_* outputs
    unsigned long long prep_gen[kMaxBatch] = {0};   // the contexts' model_gen when the set was packed
    float *prep_P_out[kMaxBatch] = {nullptr};
    float *prep_fall[kMaxBatch] = {nullptr};
    bool prep_has_fall = false;
    Event fallback_ev;                   // behind the per-frame launches when the shared launch does not apply
    // the other one-launch shot calls: a scratch of their own each (the two fp32 sets, packed_valid, cur_set and prepared are not
    // their business)
    ShotScratch s64;                     // fd_batch_deform_shared_fp64_dev
    ShotScratch sml;                     // fd_batch_deform_shared_ml_dev, for the multilayer shot launch
    ShotScratch sml64;                   // fd_batch_deform_shared_ml_fp64_dev, for the fp64 multilayer shot launch
    ShotScratch sadjp;                   // fd_batch_deform_adjoint_points_shared_dev: its pack kernel's copy, or the per-context route's one-frame result
    Event group_ev;                      // fd_batch_cook_group: behind the group's builds, for the evaluation stream
    // fd_batch_cook_group with the evaluation on the build stream itself (one unpipelined group): stream order does what the
    // events between build, packing and evaluation do across streams, and every event record is a barrier packet that keeps the
    // queue idle for ~4 us.  `lean`: the build's end (ev1) and the packing's are not recorded where they happen; ev1 goes behind
    // the evaluation (later than needed, never earlier), and "the models are consumed" is the evaluation's own event.
    bool lean = false;
    hipEvent_t consumed_override = nullptr;     // (borrowed: ev1)
    char err[512] = {0};
};


static thread_local char g_err[512] = {0};

static void set_err(fd_ctx *ctx, const char *fmt, ...)
{
    char *dst = ctx ? ctx->err : g_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
}

// The stream work is enqueued on: the caller's (fd_set_stream) or the context's own, which is
// created on first use -- a process with many contexts on caller streams should not spend a
// hardware queue per context (HIP maps streams onto GPU_MAX_HW_QUEUES queues round-robin, and
// two streams on one queue serialise).
static hipStream_t cur_stream(fd_ctx *ctx)
{
    if (ctx->stream_) return ctx->stream_;
    if (!ctx->own_stream && ctx->own_stream.create() != hipSuccess) (void)hipGetLastError();      // falls back to the null stream
    return ctx->own_stream;
}

#define FD_HIP(ctx, call)                                                               \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            set_err(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return FD_E_DEVICE;                                                         \
        }                                                                               \
    } while (0)

static int use_device(fd_ctx *ctx)
{
    int cur = -1;
    FD_HIP(ctx, hipGetDevice(&cur));
    if (cur != ctx->device) FD_HIP(ctx, hipSetDevice(ctx->device));
    return FD_OK;
}

// DevBuf's alloc -- with kGrow its grow: a scratch that grows on demand and never shrinks -- and the context's error text
constexpr bool kGrow = true;
template <typename T>
static int dev_alloc(fd_ctx *ctx, DevBuf<T> &b, size_t count, bool grow = false)
{
    const hipError_t e = grow ? b.grow(count) : b.alloc(count);
    if (e == hipSuccess) return FD_OK;
    set_err(ctx, "hipMalloc(%zu bytes) failed: %s", (count ? count : 1) * sizeof(T), hipGetErrorString(e));
    return FD_E_NOMEM;
}

static int order_of(const fd_ctx *ctx) { return ctx->M + term_cols(ctx->term); }
static int ml_layers(const fd_ctx *ctx) { return ctx->kind == FD_KERNEL_GAUSSIAN_ML ? (int)ctx->params[1] : 0; }
// Gaussian records of the solved model, and the kernel the evaluation sees
static int model_centres(const fd_ctx *ctx) { return ctx->kind == FD_KERNEL_GAUSSIAN_ML ? ctx->M * ml_layers(ctx) : ctx->M; }
static int eval_kind(const fd_ctx *ctx) { return ctx->kind == FD_KERNEL_GAUSSIAN_ML ? FD_KERNEL_GAUSSIAN_QNN : ctx->kind; }
// layers per centre in the evaluation records (built here or imported); 0 = a flat model
static int record_layers(const fd_ctx *ctx) { return ctx->kind == FD_KERNEL_GAUSSIAN_ML ? ml_layers(ctx) : ctx->imported_layers; }

// the solved model's arrays: one entry per Gaussian record (= per centre, times the layers of the
// multilayer model).  Everything in them is produced by a build or an import, so growing them loses nothing.
static int ensure_records_capacity(fd_ctx *ctx, int n)
{
    int rc;
    if (n > ctx->cap_records) {
        const int npad = round_up(n, kRecPad);
        if ((rc = dev_alloc(ctx, ctx->d_centres, (size_t)n * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_radii, (size_t)n))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_W, (size_t)(n + 4) * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_rec32, (size_t)npad))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_rec64, (size_t)npad))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_tiles, (size_t)npad / 16))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_tiles16, (size_t)npad / 16))) return rc;
        ctx->cap_records = n;
    }
    return FD_OK;
}

static int ensure_model_capacity(fd_ctx *ctx, int M)
{
    int rc;
    if (M > ctx->cap_M) {
        if ((rc = dev_alloc(ctx, ctx->d_rest, (size_t)M * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_delta, (size_t)M * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_ns, ns_doubles(M)))) return rc;
        ctx->cap_M = M;
    }
    return ensure_records_capacity(ctx, M);
}

static int ensure_solver_capacity(fd_ctx *ctx, int npad)
{
    int rc;
    if (npad > ctx->cap_npad) {
        const size_t cols = (size_t)npad + kRhsCols + 16;  // + 16 zero columns (block overrun)
        if ((rc = dev_alloc(ctx, ctx->d_A, (size_t)npad * cols))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_X, (size_t)npad * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_ipiv, (size_t)npad))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_moves, (size_t)kMovesStride * (size_t)lu_step_capacity(npad)))) return rc;
        ctx->cap_npad = npad;
    }
    return FD_OK;
}

static int sync_slot(fd_ctx *ctx)
{
    BatchSlot t{};
    t.rest = ctx->d_rest; t.delta = ctx->d_delta;
    t.centres = ctx->d_centres; t.radii = ctx->d_radii;
    t.A = ctx->d_A; t.X = ctx->d_X; t.W = ctx->d_W;
    t.ipiv = ctx->d_ipiv; t.moves = ctx->d_moves;
    t.rec32 = ctx->d_rec32; t.rec64 = ctx->d_rec64; t.tiles = ctx->d_tiles; t.tiles16 = ctx->d_tiles16;
    t.model = ctx->d_model;
    t.ns = ctx->d_ns;
    t.host_status = ctx->d_status_alias;
    if (ctx->alloc_gen != 0 && memcmp(&t, &ctx->h_slot, sizeof(t)) == 0) return FD_OK;
    // a buffer moved: hipFree in DevBuf::alloc has drained the device, nothing reads the old table
    FD_HIP(ctx, hipMemcpy(ctx->d_slot, &t, sizeof(t), hipMemcpyHostToDevice));
    ctx->h_slot = t;
    ++ctx->alloc_gen;
    return FD_OK;
}

// a model that a batched build is producing on another stream: make `s` wait for it
static bool host_is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

static int order_after_batch(fd_ctx *ctx, hipStream_t s)
{
    if (!ctx->wait_event || s == ctx->wait_stream) return FD_OK;
    if (ctx->wait_batch && ctx->wait_batch->waited_stream == s) return FD_OK;
    FD_HIP(ctx, hipStreamWaitEvent(s, ctx->wait_event, 0));
    if (ctx->wait_batch) ctx->wait_batch->waited_stream = s;
    return FD_OK;
}

// the models' statuses into page-locked host memory (one thread each; the build's last kernel wrote them)
struct StatusTable { const DevModel *model[kMaxBatch]; int *host_word[kMaxBatch]; };
__global__ void k_post_status_batch(const StatusTable t, int n)
{
    const int i = threadIdx.x;
    if (i < n) *t.host_word[i] = t.model[i]->terminationtype;
}

// Arms the asynchronous status (fd_ctx::h_status) of a build of ctxs[0..n) just enqueued on `s`.  The register-resident build
// (`reg`) posts every status word itself when each has a device address: `done`, the event behind the build, says they are in.
// Otherwise one kernel posts them all and `status_ev` is recorded behind it (one event for all: a record on every context's own
// event object would cost a stream operation each).  A context without the device address arms nothing.
static void arm_status(fd_ctx *const *ctxs, int n, hipStream_t s, bool reg, hipEvent_t done, hipEvent_t status_ev)
{
    bool posted_in_kernel = reg;
    for (int i = 0; i < n; ++i) posted_in_kernel = posted_in_kernel && ctxs[i]->h_slot.host_status != nullptr;
    hipEvent_t poll = done;
    if (!posted_in_kernel) {
        StatusTable t{};
        for (int i = 0; i < n; ++i) {
            if (!ctxs[i]->d_status_alias) return;
            t.model[i] = ctxs[i]->d_model;
            t.host_word[i] = ctxs[i]->d_status_alias;
        }
        hipLaunchKernelGGL(k_post_status_batch, dim3(1), dim3(kMaxBatch), 0, s, t, n);
        if (hipGetLastError() != hipSuccess || hipEventRecord(status_ev, s) != hipSuccess) { (void)hipGetLastError(); return; }
        poll = status_ev;
    }
    for (int i = 0; i < n; ++i) { ctxs[i]->status_poll = poll; ctxs[i]->status_inflight = true; }
}

// A build of c's model has been enqueued on `s`: later calls on other streams wait for `done` (recorded on `s`, by `batch` for a
// batched build), the report times the build by t0 / t_mid / t1, and its status is not read back yet.  `path`: the solver path of
// a full build, which leaves a factorisation fd_set_deltas can reuse (not the multilayer model's); null for a re-solve through the
// factorisation left before, whose path stays.  `rig_build_id` (fd_ctx) is a batch's alone.
static void note_build_enqueued(fd_ctx *c, hipEvent_t done, hipStream_t s, fd_batch *batch, hipEvent_t t0, hipEvent_t t_mid,
                                hipEvent_t t1, const BuildBuffers *path, uint64_t rig_build_id)
{
    c->wait_event = done; c->wait_stream = s; c->wait_batch = batch;
    c->tev0 = t0; c->tev_mid = t_mid; c->tev1 = t1;
    if (path) {
        c->have_factor = path->ml_layers == 0;
        c->factor_grouped = path->group_panels != 0;
        c->last_spd = path->spd != 0;
        c->last_small = path->spd != 0 && path->small != 0;
        c->last_reg = path->spd != 0 && path->reg != 0;
        c->last_nopivot = path->nopivot != 0;
        c->deltas_only = false;
    }
    if (batch) c->rig_build_id = rig_build_id;
    c->build_pending = true;
    ++c->model_gen;
    c->built = false;
    c->have_report = false;
    c->sticky_rc = FD_OK;
}

// The graph for `key` in *exec, captured from what `launch()` enqueues on `s` unless *exec was made for this key already.  On
// failure *exec is null: the caller launches directly.
template <typename Launch>
static hipError_t ensure_graph(hipStream_t s, GraphExec *owner, GraphKey *exec_key, const GraphKey &key, Launch launch)
{
    hipGraphExec_t *exec = &owner->exec;
    if (*exec && memcmp(&key, exec_key, sizeof(key)) == 0) return hipSuccess;
    owner->reset();
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        const hipError_t e1 = launch();
        e = hipStreamEndCapture(s, &graph);
        if (e == hipSuccess && e1 != hipSuccess) e = e1;
    }
    if (e == hipSuccess && graph) e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { (void)hipGetLastError(); *exec = nullptr; }
    else *exec_key = key;
    return e;
}

// the key of a graph that builds c's model along the solver path `flags`; a single context's graph reads its own buffers
static GraphKey graph_key(const fd_ctx *c, int flags, bool single)
{
    GraphKey k{};
    k.M = c->M; k.kind = c->kind; k.term = c->term | flags; k.nparams = c->nparams;
    memcpy(k.params, c->params, sizeof(k.params));
    if (single) { k.A = c->d_A; k.rest = c->d_rest; k.rec32 = c->d_rec32; }
    return k;
}

// same M, kernel, parameters and term: one launch chain builds their models, one shared-rig evaluation reads them
static bool same_model(const fd_ctx *a, const fd_ctx *b)
{
    return a->M == b->M && a->kind == b->kind && a->term == b->term && a->nparams == b->nparams &&
           memcmp(a->params, b->params, sizeof(a->params)) == 0;
}

// tangent frames: all three arrays or none
static bool frames_ok(const void *tu, const void *tv, const void *nrm)
{
    const int n = (tu != nullptr) + (tv != nullptr) + (nrm != nullptr);
    return n == 0 || n == 3;
}

static int poll_status(fd_ctx *ctx);

extern "C" {

int fd_abi_version(void) { return FD_ABI_VERSION; }

const char *fd_last_error(const fd_ctx *ctx) { return ctx ? ctx->err : g_err; }

fd_ctx *fd_create(const fd_config *cfg)
{
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_err(nullptr, "fd_create: no HIP device visible (%s); this engine has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "0 devices");
        return nullptr;
    }
    fd_ctx *ctx = new (std::nothrow) fd_ctx();
    if (!ctx) { set_err(nullptr, "fd_create: out of host memory"); return nullptr; }
    int dev = cfg ? cfg->device : -1;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) {
        set_err(nullptr, "fd_create: device %d out of range (%d visible)", dev, ndev);
        delete ctx;
        return nullptr;
    }
    ctx->device = dev;
    if (cfg) {
        ctx->eval_precision = cfg->eval_precision == FD_EVAL_FP64 ? FD_EVAL_FP64 : FD_EVAL_FP32;
        ctx->eval_variant = cfg->eval_variant;
        ctx->solver = (cfg->solver == FD_SOLVER_LU || cfg->solver == FD_SOLVER_ONE_WORKGROUP || cfg->solver == FD_SOLVER_REGISTER ||
                       cfg->solver == FD_SOLVER_CHAIN) ? cfg->solver : FD_SOLVER_AUTO;
    }
    hipDeviceProp_t prop;
    if (hipSetDevice(dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        set_err(nullptr, "fd_create: cannot query device %d", dev);
        delete ctx;
        return nullptr;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(nullptr, "fd_create: device %d is %s; kernels are built for gfx950 (MI355X) only",
                dev, prop.gcnArchName);
        delete ctx;
        return nullptr;
    }
    bool ok = true;
    ok = ok && ctx->ev0.create(hipEventDefault) == hipSuccess && ctx->ev_mid.create(hipEventDefault) == hipSuccess &&
         ctx->ev1.create(hipEventDefault) == hipSuccess;
    ok = ok && ctx->d_model.alloc(1) == hipSuccess;
    ok = ok && ctx->d_slot.alloc(1) == hipSuccess;
    ok = ok && ctx->h_model.alloc(1, hipHostMallocDefault) == hipSuccess;
    ok = ok && ctx->h_header.alloc(1, hipHostMallocDefault) == hipSuccess;
    ok = ok && ctx->h_status.alloc(1, hipHostMallocDefault) == hipSuccess;
    if (ok && hipHostGetDevicePointer((void **)&ctx->d_status_alias, ctx->h_status.p, 0) != hipSuccess) { (void)hipGetLastError(); ctx->d_status_alias = nullptr; }
    ok = ok && ctx->status_ev.create(hipEventDisableTiming) == hipSuccess;
    if (ok) ok = hipMemset(ctx->d_model, 0, sizeof(DevModel)) == hipSuccess;
    if (!ok) {
        set_err(nullptr, "fd_create: device resource allocation failed: %s",
                hipGetErrorString(hipGetLastError()));
        fd_destroy(ctx);        // releases what has been created
        return nullptr;
    }
    ctx->tev0 = ctx->ev0; ctx->tev_mid = ctx->ev_mid; ctx->tev1 = ctx->ev1;
    return ctx;
}

void fd_destroy(fd_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream_ || ctx->own_stream) (void)hipStreamSynchronize(cur_stream(ctx));
    free(ctx->h_gshot);
    delete ctx;                 // the members release what they own, own_stream last
}

int fd_set_stream(fd_ctx *ctx, void *hip_stream)
{
    if (!ctx) return FD_E_INVALID;
    int rc = use_device(ctx);
    if (rc) return rc;
    if (ctx->stream_ || ctx->own_stream) FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    ctx->stream_ = (hipStream_t)hip_stream;
    return FD_OK;
}

int fd_synchronize(fd_ctx *ctx)
{
    if (!ctx) return FD_E_INVALID;
    int rc = use_device(ctx);
    if (rc) return rc;
    FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    return FD_OK;
}

static int set_points_common(fd_ctx *ctx, const float *rest, const float *delta, int M, bool on_device)
{
    if (!ctx) return FD_E_INVALID;
    if (!rest || !delta || M <= 0) { set_err(ctx, "fd_set_points: need M > 0 and both arrays"); return FD_E_INVALID; }
    if (M + 4 > kMaxOrder) { set_err(ctx, "fd_set_points: M = %d exceeds the supported %d", M, kMaxOrder - 4); return FD_E_INVALID; }
    int rc = use_device(ctx);
    if (rc) return rc;
    if ((rc = ensure_model_capacity(ctx, M))) return rc;
    const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    FD_HIP(ctx, hipMemcpyAsync(ctx->d_rest, rest, sizeof(float) * 3 * (size_t)M, k, cur_stream(ctx)));
    FD_HIP(ctx, hipMemcpyAsync(ctx->d_delta, delta, sizeof(float) * 3 * (size_t)M, k, cur_stream(ctx)));
    if (!on_device) FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));  // caller may reuse its arrays
    if (M != ctx->M) ctx->prefer_lu = false;
    ctx->M = M;
    ctx->rest_src = nullptr;
    ctx->rig_build_id = 0;
    ctx->sticky_rc = FD_OK; ctx->status_inflight = false;
    ctx->points_set = true;
    ctx->built = false;
    ctx->build_pending = false;
    ctx->have_factor = false;
    ctx->deltas_only = false;
    return FD_OK;
}

// New deltas for the rest points already factorised (the animated-rig case: the rest rig stands
// still, the deformed rig moves).  The next fd_build* only carries the new right-hand sides
// through the stored factorisation.
static int set_deltas_common(fd_ctx *ctx, const float *delta, int M, bool on_device)
{
    if (!ctx) return FD_E_INVALID;
    if (!delta || M <= 0) { set_err(ctx, "fd_set_deltas: need M > 0 and the array"); return FD_E_INVALID; }
    if (!ctx->have_factor || M != ctx->M) {
        set_err(ctx, "fd_set_deltas: no factorisation for %d control points (call fd_set_points + fd_build first; "
                     "fd_set_kernel / fd_set_term / fd_import_model discard it)", M);
        return FD_E_NOT_BUILT;
    }
    if (!ctx->last_spd && round_up(order_of(ctx), 32) > 2048) {
        set_err(ctx, "fd_set_deltas: supported up to order 2048 (M = %d here); use fd_set_points", M);
        return FD_E_INVALID;
    }
    int rc = use_device(ctx);
    if (rc) return rc;
    const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    FD_HIP(ctx, hipMemcpyAsync(ctx->d_delta, delta, sizeof(float) * 3 * (size_t)M, k, cur_stream(ctx)));
    if (!on_device) FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    ctx->deltas_only = true;
    ctx->built = false;
    ctx->build_pending = false;
    ctx->sticky_rc = FD_OK; ctx->status_inflight = false;
    return FD_OK;
}

int fd_set_deltas(fd_ctx *ctx, const float *delta_xyz, int M) { return set_deltas_common(ctx, delta_xyz, M, false); }
int fd_set_deltas_dev(fd_ctx *ctx, const float *d_delta_xyz, int M) { return set_deltas_common(ctx, d_delta_xyz, M, true); }

int fd_set_points(fd_ctx *ctx, const float *rest_xyz, const float *delta_xyz, int M)
{
    return set_points_common(ctx, rest_xyz, delta_xyz, M, false);
}

int fd_set_points_dev(fd_ctx *ctx, const float *d_rest_xyz, const float *d_delta_xyz, int M)
{
    return set_points_common(ctx, d_rest_xyz, d_delta_xyz, M, true);
}

int fd_set_kernel(fd_ctx *ctx, int kind, const double *params, int nparams)
{
    if (!ctx) return FD_E_INVALID;
    if (kind < FD_KERNEL_GAUSSIAN || kind > FD_KERNEL_GAUSSIAN_ML || nparams < 0 || nparams > 4 ||
        (nparams > 0 && !params)) {
        set_err(ctx, "fd_set_kernel: bad kind %d / nparams %d", kind, nparams);
        return FD_E_INVALID;
    }
    double p[4] = {0, 0, 0, 0};
    for (int i = 0; i < nparams; ++i) p[i] = params[i];
    if (kind == FD_KERNEL_GAUSSIAN) {
        if (nparams < 1) p[0] = 1.0;
        if (!(p[0] > 0.0)) { set_err(ctx, "fd_set_kernel: Gaussian radius must be > 0"); return FD_E_INVALID; }
    } else if (kind == FD_KERNEL_GAUSSIAN_QNN) {
        if (nparams < 1) p[0] = 1.0;
        if (nparams < 2) p[1] = 5.0;
        if (!(p[0] > 0.0) || !(p[1] > 0.0)) { set_err(ctx, "fd_set_kernel: q and z must be > 0"); return FD_E_INVALID; }
    } else if (kind == FD_KERNEL_GAUSSIAN_ML) {
        if (nparams < 1) p[0] = 1.0;
        if (nparams < 2) p[1] = 4.0;
        if (nparams < 3) p[2] = 0.1;     // the SOP's defaults for radius, layers, lambda (src/SOP_FaceDeform.cpp:125-131)
        p[1] = floor(p[1]);
        if (!(p[0] > 0.0) || !(p[1] >= 1.0 && p[1] <= (double)kMaxLayers) || !(p[2] >= 0.0)) {
            set_err(ctx, "fd_set_kernel: multilayer needs radius > 0, 1 <= layers <= %d, lambda >= 0", kMaxLayers);
            return FD_E_INVALID;
        }
    }
    if (kind == ctx->kind && nparams == ctx->nparams && memcmp(ctx->params, p, sizeof(p)) == 0)
        return FD_OK;                 // nothing changes: the model and its factorisation stay valid
    ctx->kind = kind;
    ctx->nparams = nparams;
    memcpy(ctx->params, p, sizeof(p));
    ctx->imported_layers = 0;
    ctx->prefer_lu = false;
    ctx->built = false;
    ctx->build_pending = false;
    ctx->have_factor = false;
    ctx->deltas_only = false;
    return FD_OK;
}

int fd_set_term(fd_ctx *ctx, int term)
{
    if (!ctx) return FD_E_INVALID;
    if (term < FD_TERM_LINEAR || term > FD_TERM_ZERO) { set_err(ctx, "fd_set_term: bad term %d", term); return FD_E_INVALID; }
    if (term == ctx->term) return FD_OK;
    ctx->term = term;
    ctx->prefer_lu = false;
    ctx->built = false;
    ctx->build_pending = false;
    ctx->have_factor = false;
    ctx->deltas_only = false;
    return FD_OK;
}

static double ctx_lambda(const fd_ctx *ctx)
{
    const int idx = ctx->kind == FD_KERNEL_GAUSSIAN ? 1 : (ctx->kind == FD_KERNEL_GAUSSIAN_QNN || ctx->kind == FD_KERNEL_GAUSSIAN_ML ? 2 : 0);
    return ctx->nparams > idx ? ctx->params[idx] : 0.0;
}

// FD_SOLVER_LU keeps every system on the pivoted LU
static bool use_spd(const fd_ctx *ctx)
{
    if (ctx->solver == FD_SOLVER_LU || ctx->prefer_lu) return false;
    if (ctx->kind == FD_KERNEL_GAUSSIAN_ML) return false;          // its own pipeline (launch_build_ml)
    return spd_applicable(ctx->kind, ctx->term, ctx_lambda(ctx), ctx->M);
}

// The QNN model's kernel block without pivot search (fd_build.hip k_lu_panel_np): one row per thread, order <= 1024; not once
// a build of this rig has asked for the pivoted LU (prefer_lu), nor under FD_SOLVER_LU.
static bool use_nopivot(const fd_ctx *ctx)
{
    if (ctx->solver == FD_SOLVER_LU || ctx->prefer_lu) return false;
    return ctx->kind == FD_KERNEL_GAUSSIAN_QNN && round_up(ctx->M, 32) <= 1024;
}

// The register-resident one-launch build (fd_build_reg.hip): what FD_SOLVER_AUTO takes on the definite path up to 256
// control points; FD_SOLVER_CHAIN keeps the launch chain, FD_SOLVER_ONE_WORKGROUP the round-2 one-workgroup build.
static bool use_reg(const fd_ctx *ctx)
{
    if (!(ctx->solver == FD_SOLVER_AUTO || ctx->solver == FD_SOLVER_REGISTER)) return false;
    return reg_applicable(ctx->kind, ctx->term, ctx_lambda(ctx), ctx->M);
}

static void fill_build_buffers(const fd_ctx *ctx, BuildBuffers &b)
{
    b.M = ctx->M;
    b.T = term_cols(ctx->term);
    b.n = order_of(ctx);
    b.npad = round_up(b.n, 32);
    b.lda = b.npad;
    b.ncols = b.npad + kRhsCols;
    b.ml_layers = ml_layers(ctx);
    b.kind = b.ml_layers ? FD_KERNEL_GAUSSIAN : ctx->kind;       // what the assembly evaluates
    b.term = ctx->term;
    b.lambda = ctx_lambda(ctx);
    b.gauss_R = (ctx->kind == FD_KERNEL_GAUSSIAN || b.ml_layers) ? ctx->params[0] : 1.0;
    b.qnn_q = ctx->params[0];
    b.qnn_z = ctx->params[1];
    b.Mpad = round_up(ctx->M, kRecPad);
    b.d_slots = ctx->d_slot;
    b.nbatch = 1;
    b.group_panels = 0;
    b.spd = b.small = b.reg = b.nopivot = 0;     // the solver path: choose_build
    b.reg_front = 1;
}

// The solver path of a build of ctxs[0..n) (n = 1: a single build), whose models are context 0's: every path is everybody's
// choice or nobody's -- one context that fell back to the LU takes the batch with it.
static void choose_build(fd_ctx *const *ctxs, int n, BuildBuffers &b)
{
    fill_build_buffers(ctxs[0], b);
    b.spd = b.small = b.reg = b.nopivot = 1;
    for (int i = 0; i < n; ++i) {
        if (!use_spd(ctxs[i])) b.spd = 0;
        if (ctxs[i]->solver != FD_SOLVER_ONE_WORKGROUP) b.small = 0;
        if (!use_reg(ctxs[i])) b.reg = 0;
        if (!use_nopivot(ctxs[i])) b.nopivot = 0;
    }
    if (!b.spd) b.reg = 0;      // the register-resident build is a form of the definite path
    // ... and so is the one-workgroup build, up to the size k_build_small takes: beyond it FD_SOLVER_ONE_WORKGROUP is the launch
    // chain, and fd_report.solver_used says so
    if (!b.spd || !small_applicable(b.M, b.T)) b.small = 0;
}

int fd_build_async(fd_ctx *ctx)
{
    if (!ctx) return FD_E_INVALID;
    if (!ctx->points_set) { set_err(ctx, "fd_build: fd_set_points has not been called"); return FD_E_INVALID; }
    ctx->imported_layers = 0;        // whatever was imported is about to be replaced
    int rc = use_device(ctx);
    if (rc) return rc;
    const int npad = round_up(order_of(ctx), 32);
    const bool grew = npad > ctx->cap_npad;
    if ((rc = ensure_solver_capacity(ctx, npad))) return rc;
    if ((rc = ensure_records_capacity(ctx, model_centres(ctx)))) return rc;
    if ((rc = sync_slot(ctx))) return rc;
    BuildBuffers b;
    choose_build(&ctx, 1, b);
    if (b.reg) FD_HIP(ctx, reg_build_init());
    if (ctx->deltas_only && ctx->have_factor && ctx->last_reg) {
        // the register-resident build keeps no factorisation (it is faster than the stored-factor path was): new deltas
        // are a new build from the context's own copy of the points -- bit-identical to fd_set_points + fd_build by construction
        ctx->deltas_only = false;
    }
    hipStream_t st = cur_stream(ctx);
    const bool resolve = ctx->deltas_only && ctx->have_factor;
    if (resolve) {
        // fd_set_deltas: right-hand sides only, through the factorisation of the last full build
        b.group_panels = ctx->factor_grouped ? 1 : 0;
        b.spd = ctx->last_spd ? 1 : 0;                // the path that left the factorisation (a batch may have overruled this context's own choice)
        const GraphKey key = graph_key(ctx, (b.group_panels << 8) | (b.spd << 9), true);
        if (ctx->use_graph) (void)ensure_graph(st, &ctx->resolve_exec, &ctx->resolve_key, key, [&] { return launch_resolve(b, st, nullptr); });
        FD_HIP(ctx, hipEventRecord(ctx->ev0, st));
        FD_HIP(ctx, hipEventRecord(ctx->ev_mid, st));
        if (ctx->use_graph && ctx->resolve_exec) FD_HIP(ctx, hipGraphLaunch(ctx->resolve_exec, st));
        else FD_HIP(ctx, launch_resolve(b, st, nullptr));
    } else if (b.reg) {
        // the register-resident build is ONE launch, control table included: nothing to capture, nothing to prepare
        // (it keeps no factorisation, yet fd_set_deltas is allowed: it builds again, see above)
        FD_HIP(ctx, hipEventRecord(ctx->ev0, st));
        FD_HIP(ctx, launch_build_reg(b, st, nullptr, ctx->ev_mid));
    } else {
        if (grew) {
            // the 16 overrun columns past the RHS block must read as zero forever
            const size_t cols = (size_t)ctx->cap_npad + kRhsCols + 16;
            FD_HIP(ctx, hipMemsetAsync(ctx->d_A, 0, sizeof(double) * (size_t)ctx->cap_npad * cols, st));
        }
        const GraphKey key = graph_key(ctx, (b.spd << 9) | (b.reg << 11) | (b.nopivot << 12), true);
        if (ctx->use_graph && ensure_graph(st, &ctx->build_exec, &ctx->graph_key, key, [&] {
                const hipError_t e1 = launch_prepare(b, st, nullptr);
                const hipError_t e2 = launch_build(b, st, nullptr);
                return e1 != hipSuccess ? e1 : e2;
            }) != hipSuccess)
            ctx->use_graph = false;      // this runtime cannot capture the sequence: launch directly
        FD_HIP(ctx, hipEventRecord(ctx->ev0, st));
        if (ctx->use_graph && ctx->build_exec) {
            FD_HIP(ctx, hipEventRecord(ctx->ev_mid, st));   // phases are not split inside a graph
            FD_HIP(ctx, hipGraphLaunch(ctx->build_exec, st));
        } else {
            FD_HIP(ctx, launch_prepare(b, st, nullptr));
            FD_HIP(ctx, launch_build(b, st, ctx->ev_mid));
        }
    }
    FD_HIP(ctx, hipEventRecord(ctx->ev1, st));
    // A later evaluation on ANOTHER stream is ordered behind this build (order_after_batch): a single build as much as
    // a batched one, and in particular the LU rebuild that poll_status enqueues here when the Cholesky lost definiteness --
    // the evaluation that triggered the repair may launch on a stream that knows nothing of this one.
    note_build_enqueued(ctx, ctx->ev1, st, nullptr, ctx->ev0, ctx->ev_mid, ctx->ev1, resolve ? nullptr : &b, 0);
    arm_status(&ctx, 1, st, !resolve && b.reg, ctx->ev1, ctx->status_ev);
    return FD_OK;
}

int fd_build_result(fd_ctx *ctx, fd_report *report)
{
    if (!ctx) return FD_E_INVALID;
    int rc = use_device(ctx);
    if (rc) return rc;
    if (ctx->build_pending) {
        if ((rc = order_after_batch(ctx, cur_stream(ctx)))) return rc;
        FD_HIP(ctx, hipMemcpyAsync(ctx->h_model, ctx->d_model, sizeof(DevModel), hipMemcpyDeviceToHost, cur_stream(ctx)));
        FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
        ctx->status_inflight = false;
        ctx->wait_event = nullptr; ctx->wait_stream = nullptr; ctx->wait_batch = nullptr;   // the batched build it named is complete
        fd_report r{};
        r.terminationtype = ctx->h_model->terminationtype;
        r.iterationscount = ctx->h_model->iterations;
        r.n = order_of(ctx);
        r.solver_used = ctx->last_reg ? FD_SOLVER_REGISTER
                        : ctx->last_spd ? (ctx->last_small ? FD_SOLVER_ONE_WORKGROUP : FD_SOLVER_CHAIN)
                        : ctx->last_nopivot ? FD_SOLVER_LU_NOPIVOT : FD_SOLVER_LU;
        double pmin, pmax;
        memcpy(&pmin, &ctx->h_model->pivmin_bits, 8);
        memcpy(&pmax, &ctx->h_model->pivmax_bits, 8);
        r.pivot_ratio = (pmax > 0.0 && pmin <= pmax) ? pmin / pmax : 0.0;
        float ms = 0.f;
        r.fp32_error = ctx->h_model->fp32_error; r.cancellation = ctx->h_model->cancellation;
        r.delta_min = ctx->h_model->delta_min; r.delta_max = ctx->h_model->delta_max; r.extent = ctx->h_model->extent;
        if (ctx->tev0 && ctx->tev_mid && hipEventElapsedTime(&ms, ctx->tev0, ctx->tev_mid) == hipSuccess) r.t_assemble_ms = ms;
        if (ctx->tev_mid && ctx->tev1 && hipEventElapsedTime(&ms, ctx->tev_mid, ctx->tev1) == hipSuccess) r.t_solve_ms = ms;
        ctx->report = r;
        ctx->have_report = true;
        ctx->build_pending = false;
        ctx->built = r.terminationtype == 1;
        // The Cholesky pivot of two nearly coincident centres is the SQUARE of what partial
        // pivoting sees (1e-12 vs 2e-7 of the largest at 1e-7 apart), and a wide fixed-radius
        // Gaussian loses definiteness to rounding before the LU gives up.  Nothing that the LU
        // accepts may fail here: build again with it, and keep it for this rig.
        if (r.terminationtype == -4 && (ctx->last_spd || ctx->last_nopivot) && ctx->points_set) {
            ctx->prefer_lu = true;
            ctx->have_factor = false;
            ctx->deltas_only = false;
            if ((rc = fd_build_async(ctx))) return rc;
            return fd_build_result(ctx, report);
        }
    }
    if (!ctx->have_report) { set_err(ctx, "fd_build_result: no build has been enqueued"); return FD_E_NOT_BUILT; }
    if (report) *report = ctx->report;
    if (ctx->report.terminationtype == 1) return FD_OK;
    if (ctx->report.terminationtype == -5) { set_err(ctx, "fd_build: coincident control points"); return FD_E_DUPLICATE; }
    set_err(ctx, "fd_build: singular system (terminationtype %d)", ctx->report.terminationtype);
    return FD_E_SINGULAR;
}

int fd_fp32_holds(const fd_report *report, double tol)
{
    if (!report || report->terminationtype != 1) return 0;
    if (!(report->delta_max > 0.0)) return 1;             // nothing to measure against (imported model, or no displacement at all)
    const double ulp = 5.9604644775390625e-08 * (report->extent + report->delta_max);
    return report->fp32_error <= tol * 0.5 * report->delta_min + ulp ? 1 : 0;     // (vertices between control points move less than the least of those)
}

int fd_set_eval_precision(fd_ctx *ctx, int eval_precision)
{
    if (!ctx) return FD_E_INVALID;
    if (eval_precision != FD_EVAL_FP32 && eval_precision != FD_EVAL_FP64) { set_err(ctx, "fd_set_eval_precision: unknown precision %d", eval_precision); return FD_E_INVALID; }
    ctx->eval_precision = eval_precision;
    return FD_OK;
}

int fd_set_output(fd_ctx *ctx, int what)
{
    if (!ctx) return FD_E_INVALID;
    if (what != FD_OUTPUT_POSITION && what != FD_OUTPUT_DISPLACEMENT) { set_err(ctx, "fd_set_output: unknown output %d", what); return FD_E_INVALID; }
    ctx->output = what;
    return FD_OK;
}

int fd_build(fd_ctx *ctx, fd_report *report)
{
    int rc = fd_build_async(ctx);
    if (rc) {
        if (report) { memset(report, 0, sizeof(*report)); report->terminationtype = -4; }
        return rc;
    }
    return fd_build_result(ctx, report);
}

}  // extern "C"

// Non-blocking look at the status the last enqueued build posted (see fd_ctx::h_status).
static int poll_status(fd_ctx *ctx)
{
    if (ctx->sticky_rc != FD_OK) {
        set_err(ctx, ctx->sticky_rc == FD_E_DUPLICATE ? "the model's build failed: coincident control points"
                                                      : "the model's build failed: singular system");
        return ctx->sticky_rc;
    }
    if (!ctx->status_inflight) return FD_OK;
    const hipError_t q = hipEventQuery(ctx->status_poll);
    if (q == hipErrorNotReady) { (void)hipGetLastError(); return FD_OK; }     // not known yet: nothing to act on
    ctx->status_inflight = false;
    if (q != hipSuccess) { (void)hipGetLastError(); return FD_OK; }
    const int tt = *ctx->h_status;
    if (tt == 1 || tt == 0) return FD_OK;
    if (tt == -4 && (ctx->last_spd || ctx->last_nopivot) && ctx->points_set) {
        // the Cholesky lost definiteness on this rig (header: FD_SOLVER_AUTO): the LU now, enqueued on
        // the context's stream ahead of whatever the caller is about to enqueue
        ctx->prefer_lu = true;
        ctx->have_factor = false;
        ctx->deltas_only = false;
        // rare path: evaluations of the failed model enqueued earlier (pass-throughs) may still be reading
        // its buffers on streams this context knows nothing about
        if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
        ctx->wait_event = nullptr; ctx->wait_stream = nullptr; ctx->wait_batch = nullptr;
        return fd_build_async(ctx);       // leaves wait_event = the rebuild's end on cur_stream(ctx): callers order their stream behind it
    }
    ctx->sticky_rc = tt == -5 ? FD_E_DUPLICATE : FD_E_SINGULAR;
    set_err(ctx, tt == -5 ? "the model's build failed: coincident control points" : "the model's build failed: singular system");
    return ctx->sticky_rc;
}

// The mesh a one-context call works on: N vertices, their optional gate distances and projection frames, and the gate's two
// parameters.  Host arrays in the host calls, device arrays everywhere else; stage_mesh makes the second of the first.
struct Mesh {
    int64_t N;
    const float *P, *dist2, *tu, *tv, *nrm;
    float radius2, falloffrate;
};

// the evaluation of c's model over the mesh m
static DeformArgs deform_args(const fd_ctx *c, const Mesh &m, float *P_out, float *falloff_out)
{
    DeformArgs a;
    a.N = m.N;
    a.P_in = m.P; a.P_out = P_out;
    a.dist2 = m.dist2; a.falloff_out = falloff_out;
    a.tu = m.tu; a.tv = m.tv; a.nrm = m.nrm;
    a.radius2 = m.radius2; a.falloffrate = m.falloffrate;
    a.M = model_centres(c); a.Mpad = round_up(a.M, kRecPad); a.kind = eval_kind(c); a.layers = record_layers(c);
    a.rec32 = c->d_rec32; a.rec64 = c->d_rec64; a.tiles = c->d_tiles; a.tiles16 = c->d_tiles16;
    a.model = c->d_model;
    a.precision = c->eval_precision;
    a.variant = c->eval_variant;
    a.delta_out = c->output == FD_OUTPUT_DISPLACEMENT;
    return a;
}

// fd_deform_vectors*: a struct of at least this ABI's size, each transported vector with its output
static bool vectors_ok(fd_ctx *ctx, const fd_vectors *vec)
{
    if (!vec) return true;
    if (vec->struct_size < (int)sizeof(fd_vectors)) {
        set_err(ctx, "fd_deform_vectors: vec->struct_size is %d, must be sizeof(fd_vectors) = %d", vec->struct_size,
                (int)sizeof(fd_vectors));
        return false;
    }
    if ((!vec->N != !vec->N_out) || (!vec->tu != !vec->tu_out) || (!vec->tv != !vec->tv_out)) {
        set_err(ctx, "fd_deform_vectors: every vector needs its input and its output (both or neither)");
        return false;
    }
    return true;
}
static bool vectors_wanted(const fd_vectors *vec) { return vec && (vec->N || vec->tu || vec->tv || vec->jacobian); }

// fd_invert*: a struct of at least this ABI's size
static bool invert_opts_ok(fd_ctx *ctx, const fd_invert_opts *opts)
{
    if (!opts) { set_err(ctx, "fd_invert: opts is NULL"); return false; }
    if (opts->struct_size < (int)sizeof(fd_invert_opts)) {
        set_err(ctx, "fd_invert: opts->struct_size is %d, must be sizeof(fd_invert_opts) = %d", opts->struct_size,
                (int)sizeof(fd_invert_opts));
        return false;
    }
    return true;
}

// fd_deform_adjoint_points*: NULL opts (no grad_f), or a struct of at least this ABI's size
static bool adjoint_points_opts_ok(fd_ctx *ctx, const fd_adjoint_points_opts *opts)
{
    if (opts && opts->struct_size < (int)sizeof(fd_adjoint_points_opts)) {
        set_err(ctx, "fd_deform_adjoint_points: opts->struct_size is %d, must be sizeof(fd_adjoint_points_opts) = %d",
                opts->struct_size, (int)sizeof(fd_adjoint_points_opts));
        return false;
    }
    return true;
}

// fd_deform_bake* and fd_deform_bake_grad*: which of the two a call is (comps: fd_internal.h BakeArgs), with the names its
// messages use
struct BakeCall {
    const char *who, *opts_name, *out, *out32;
    int comps;
};
static const BakeCall kBake{"fd_deform_bake", "fd_bake_opts", "B", "B32", 1};
static const BakeCall kBakeGrad{"fd_deform_bake_grad", "fd_bake_grad_opts", "G", "G32", 3};
// The two opts structs are one layout under two names: the host layer reads both as fd_bake_opts (G32 as B32), and
// sizeof(fd_bake_opts) in a message is the size of either.
static_assert(sizeof(fd_bake_grad_opts) == sizeof(fd_bake_opts) && offsetof(fd_bake_grad_opts, struct_size) == offsetof(fd_bake_opts, struct_size) &&
              offsetof(fd_bake_grad_opts, G32) == offsetof(fd_bake_opts, B32), "fd_bake_grad_opts is fd_bake_opts' layout");
static const fd_bake_opts *bake_opts_view(const fd_bake_grad_opts *opts) { return reinterpret_cast<const fd_bake_opts *>(opts); }

// NULL opts (B alone), or a struct of at least this ABI's size; B or B32, one at least
static bool bake_outputs_ok(fd_ctx *ctx, const BakeCall &k, const double *B, const fd_bake_opts *opts)
{
    if (opts && opts->struct_size < (int)sizeof(fd_bake_opts)) {
        set_err(ctx, "%s: opts->struct_size is %d, must be sizeof(%s) = %d", k.who, opts->struct_size, k.opts_name,
                (int)sizeof(fd_bake_opts));
        return false;
    }
    if (!B && !(opts && opts->B32)) { set_err(ctx, "%s: %s and opts->%s are both NULL", k.who, k.out, k.out32); return false; }
    return true;
}

// The scratch of the adjoint, the Gram operator and the shot adjoint for N vertices and C records: the workgroups' partial blocks
// and, behind them, room for the result, where the host call stages it (*_staging).  Grown on demand (DevBuf::grow).
// fd_deform_adjoint*: adjoint_groups(N) partial blocks of (C + 4) x 3 doubles and one more for grad_W
static size_t adjoint_block(int C) { return (size_t)(C + 4) * 3; }
static size_t adjoint_scratch(int64_t N, int C) { return ((size_t)adjoint_groups(N) + 1) * adjoint_block(C); }
static double *adjoint_staging(const fd_ctx *ctx, int64_t N, int C) { return ctx->d_adj + (size_t)adjoint_groups(N) * adjoint_block(C); }
// fd_deform_gram*: gram_partial_doubles partial blocks and H, nq components of (C + 4) x (C + 4)
static size_t gram_block(int C, int nq) { return (size_t)nq * (size_t)(C + 4) * (size_t)(C + 4); }
static size_t gram_scratch(int64_t N, int C, int nq) { return gram_partial_doubles(N, C, nq) + gram_block(C, nq); }
static double *gram_staging(const fd_ctx *ctx, int64_t N, int C, int nq) { return ctx->d_gram + gram_partial_doubles(N, C, nq); }
// fd_deform_adjoint_shot*: adjoint_shot_partial_doubles partial blocks, which the groups of frames use one after the other, and
// `staged` frames' grad_W.  The launch's own request (staged = 0) keeps what the host call asked for: the buffer never shrinks.
static size_t adjoint_shot_scratch(int64_t N, int C, int staged) { return adjoint_shot_partial_doubles(N, C) + (size_t)staged * adjoint_block(C); }
static double *adjoint_shot_staging(const fd_ctx *ctx, int64_t N, int C) { return ctx->d_adjs + adjoint_shot_partial_doubles(N, C); }

// What every one-context call on a mesh checks first, for the entry point `who`; out_ok: the call has the output array it needs
static int mesh_checks(fd_ctx *ctx, const char *who, const Mesh &m, bool out_ok)
{
    if (m.N < 0 || (m.N > 0 && (!m.P || !out_ok))) { set_err(ctx, "%s: bad N / P pointers", who); return FD_E_INVALID; }
    if (!frames_ok(m.tu, m.tv, m.nrm)) { set_err(ctx, "%s: tu, tv, nrm must be all set or all NULL", who); return FD_E_INVALID; }
    if (!ctx->built && !ctx->build_pending) { set_err(ctx, "%s: no successfully built model", who); return FD_E_NOT_BUILT; }
    return FD_OK;
}

// What every one-context device call does before its launches: the checks; for an empty mesh nothing more (the caller returns
// on m.N == 0 as it does on an error); else the device, the model's status, the evaluation's arguments and the order behind a
// batched build.  *s is the stream to launch on: hip_stream, or the context's when that is null.
static int deform_begin(fd_ctx *ctx, const char *who, void *hip_stream, const Mesh &m, float *d_P_out, float *d_falloff_out,
                        bool out_ok, DeformArgs *a, hipStream_t *s)
{
    *s = hip_stream ? (hipStream_t)hip_stream : cur_stream(ctx);
    int rc = mesh_checks(ctx, who, m, out_ok);
    if (rc || m.N == 0) return rc;
    if ((rc = use_device(ctx))) return rc;
    if ((rc = poll_status(ctx))) return rc;           // a failed asynchronous build: repaired here, or reported
    *a = deform_args(ctx, m, d_P_out, d_falloff_out);
    return order_after_batch(ctx, *s);
}

// fd_deform_dev_stream / fd_deform_vectors_dev / the staged host calls: the deformation's launch, with vec the vectors' as well
static int deform_dev(fd_ctx *ctx, const char *who, void *hip_stream, const Mesh &m, float *d_P_out, float *d_falloff_out,
                      const fd_vectors *vec)
{
    DeformArgs a;
    hipStream_t launch_stream;
    int rc = deform_begin(ctx, who, hip_stream, m, d_P_out, d_falloff_out, d_P_out != nullptr, &a, &launch_stream);
    if (rc || m.N == 0) return rc;
    if (!vec) {
        FD_HIP(ctx, launch_deform(a, launch_stream));
        return FD_OK;
    }
    // The vectors' launch reads P_in and the frames, the deformation's writes P_out: the vectors go first, so that
    // P_out may alias P_in.  A transported vector written over a projection frame (N_out == nrm: the SOP's in-place N)
    // must wait for the deformation instead, which then may not overwrite P_in: P_in is copied aside for that case.
    const VectorArgs v{vec->N, vec->tu, vec->tv, vec->N_out, vec->tu_out, vec->tv_out, vec->jacobian};
    const float *const outs[3] = {v.N_out, v.tu_out, v.tv_out};
    bool clash = false;
    for (const float *o : outs) clash |= o && (o == m.tu || o == m.tv || o == m.nrm || o == m.dist2);
    if (!clash) {
        FD_HIP(ctx, launch_vectors(a, v, launch_stream));
        FD_HIP(ctx, launch_deform(a, launch_stream));
        return FD_OK;
    }
    DeformArgs av = a;
    if (d_P_out == m.P) {
        if ((rc = dev_alloc(ctx, ctx->d_vecP, (size_t)m.N * 3, kGrow))) return rc;
        FD_HIP(ctx, hipMemcpyAsync(ctx->d_vecP, m.P, sizeof(float) * 3 * (size_t)m.N, hipMemcpyDeviceToDevice, launch_stream));
        av.P_in = ctx->d_vecP;
    }
    FD_HIP(ctx, launch_deform(a, launch_stream));
    FD_HIP(ctx, launch_vectors(av, v, launch_stream));
    return FD_OK;
}

// fd_invert_dev: the inverse's one launch (m.P = the deformed points, d_X_out = the rest-space points)
static int invert_dev(fd_ctx *ctx, const Mesh &m, float *d_X_out, const InvertArgs &inv)
{
    DeformArgs a;
    hipStream_t s;
    const int rc = deform_begin(ctx, "fd_invert", nullptr, m, d_X_out, nullptr, d_X_out != nullptr, &a, &s);
    if (rc || m.N == 0) return rc;
    FD_HIP(ctx, launch_invert(a, inv, s));
    return FD_OK;
}

// fd_deform_adjoint_dev: the adjoint's two launches.  Like the two below it writes nothing for an empty mesh: the caller zeroes.
static int adjoint_dev(fd_ctx *ctx, const char *who, const Mesh &m, const float *d_G, double *d_grad_W)
{
    DeformArgs a;
    hipStream_t s;
    int rc = deform_begin(ctx, who, nullptr, m, nullptr, nullptr, true, &a, &s);
    if (rc || m.N == 0) return rc;
    if ((rc = dev_alloc(ctx, ctx->d_adj, adjoint_scratch(m.N, a.M), kGrow))) return rc;
    const AdjointArgs g{d_G, d_grad_W, ctx->d_adj, term_cols(ctx->term)};
    FD_HIP(ctx, launch_adjoint(a, g, s));
    return FD_OK;
}

// fd_deform_adjoint_points_dev: the one launch (d_grad_f: null for none); nothing is written for an empty mesh
static int adjoint_points_dev(fd_ctx *ctx, const char *who, const Mesh &m, const float *d_G, double *d_grad_P, double *d_grad_f)
{
    DeformArgs a;
    hipStream_t s;
    const int rc = deform_begin(ctx, who, nullptr, m, nullptr, nullptr, true, &a, &s);
    if (rc || m.N == 0) return rc;
    FD_HIP(ctx, launch_adjoint_points(a, AdjointPointsArgs{d_G, d_grad_P, d_grad_f}, s));
    return FD_OK;
}

// fd_deform_gram_dev: the Gram operator's two launches
static int gram_dev(fd_ctx *ctx, const char *who, const Mesh &m, const float *d_omega, double *d_H)
{
    DeformArgs a;
    hipStream_t s;
    int rc = deform_begin(ctx, who, nullptr, m, nullptr, nullptr, true, &a, &s);
    if (rc || m.N == 0) return rc;
    if ((rc = dev_alloc(ctx, ctx->d_gram, gram_scratch(m.N, a.M, m.tu ? 6 : 1), kGrow))) return rc;
    const GramArgs g{d_omega, d_H, ctx->d_gram, term_cols(ctx->term)};
    FD_HIP(ctx, launch_gram(a, g, s));
    return FD_OK;
}

// fd_deform_bake_dev and fd_deform_bake_grad_dev: the pack kernel and the one launch; nothing is written for an empty mesh
static int bake_dev(fd_ctx *ctx, const BakeCall &k, const Mesh &m, const double *d_S, double *d_B, float *d_B32)
{
    DeformArgs a;
    hipStream_t s;
    int rc = deform_begin(ctx, k.who, nullptr, m, nullptr, nullptr, true, &a, &s);
    if (rc || m.N == 0) return rc;
    if ((rc = dev_alloc(ctx, ctx->d_bake, bake_scratch_doubles(a.M, ctx->M, k.comps), kGrow))) return rc;
    const BakeArgs g{d_S, ctx->M, term_cols(ctx->term), ctx->d_bake, d_B, d_B32, k.comps};
    FD_HIP(ctx, launch_bake_pack(a, g, s));
    FD_HIP(ctx, launch_bake(a, g, s));
    return FD_OK;
}

// fd_deform_adjoint_shot_dev: the shot adjoint's two launches per group of frames
static int adjoint_shot_dev(fd_ctx *ctx, const char *who, const Mesh &m, int F, const float *d_G, double *d_grad_W)
{
    DeformArgs a;
    hipStream_t s;
    int rc = deform_begin(ctx, who, nullptr, m, nullptr, nullptr, true, &a, &s);
    if (rc || m.N == 0) return rc;
    if ((rc = dev_alloc(ctx, ctx->d_adjs, adjoint_shot_scratch(m.N, a.M, 0), kGrow))) return rc;
    const AdjointShotArgs g{d_G, d_grad_W, ctx->d_adjs, F, term_cols(ctx->term)};
    FD_HIP(ctx, launch_adjoint_shot(a, g, s));
    return FD_OK;
}

// the staging arrays of the host calls for N vertices: d_P, d_dist2, d_fall; the frames' on first use.  cap_N is 0 while the
// first three are being replaced, and d_nrm, which comes last, is set only when all three frames are.
static int ensure_staging(fd_ctx *ctx, int64_t N, bool frames)
{
    int rc;
    if (N > ctx->cap_N) {
        ctx->cap_N = 0;                 // one capacity for three buffers: DevBuf::grow's rule for them together
        if ((rc = dev_alloc(ctx, ctx->d_P, (size_t)N * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_dist2, (size_t)N))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_fall, (size_t)N))) return rc;
        // tangent frames are optional and 3x as large: allocate on first use
        for (DevBuf<float> *b : {&ctx->d_tu, &ctx->d_tv, &ctx->d_nrm}) b->reset();
        ctx->cap_N = N;
    }
    if (frames && !ctx->d_nrm) {
        if ((rc = dev_alloc(ctx, ctx->d_tu, (size_t)ctx->cap_N * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_tv, (size_t)ctx->cap_N * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->d_nrm, (size_t)ctx->cap_N * 3))) return rc;
    }
    return FD_OK;
}

// one more host array of `floats` per vertex that goes up among the mesh's, into the staging buffer *dst (read once
// ensure_staging has run, which may replace it); src == nullptr: none
struct Upload { float *const *dst; const float *src; int floats; };

// The host mesh h on the device, for the host calls: the staging buffers grown for it, the uploads enqueued on s -- P, after_P's,
// dist2, after_dist2's, the three frames -- and *d the same mesh in the staging buffers, null where h has null.  An empty
// mesh touches no device and is handed back as it came: whether it has frames still says how large a result is.
static int stage_mesh(fd_ctx *ctx, const Mesh &h, hipStream_t s, Mesh *d, Upload after_P = {}, Upload after_dist2 = {})
{
    *d = h;
    if (h.N == 0) return FD_OK;
    int rc = use_device(ctx);
    if (rc) return rc;
    if ((rc = ensure_staging(ctx, h.N, h.tu != nullptr))) return rc;
    const size_t b1 = sizeof(float) * (size_t)h.N, b3 = 3 * b1;
    FD_HIP(ctx, hipMemcpyAsync(ctx->d_P, h.P, b3, hipMemcpyHostToDevice, s));
    if (after_P.src) FD_HIP(ctx, hipMemcpyAsync(*after_P.dst, after_P.src, b1 * (size_t)after_P.floats, hipMemcpyHostToDevice, s));
    if (h.dist2) FD_HIP(ctx, hipMemcpyAsync(ctx->d_dist2, h.dist2, b1, hipMemcpyHostToDevice, s));
    if (after_dist2.src) FD_HIP(ctx, hipMemcpyAsync(*after_dist2.dst, after_dist2.src, b1 * (size_t)after_dist2.floats, hipMemcpyHostToDevice, s));
    d->P = ctx->d_P;
    d->dist2 = h.dist2 ? ctx->d_dist2 : nullptr;
    if (h.tu) {
        FD_HIP(ctx, hipMemcpyAsync(ctx->d_tu, h.tu, b3, hipMemcpyHostToDevice, s));
        FD_HIP(ctx, hipMemcpyAsync(ctx->d_tv, h.tv, b3, hipMemcpyHostToDevice, s));
        FD_HIP(ctx, hipMemcpyAsync(ctx->d_nrm, h.nrm, b3, hipMemcpyHostToDevice, s));
        d->tu = ctx->d_tu; d->tv = ctx->d_tv; d->nrm = ctx->d_nrm;
    }
    return FD_OK;
}

// fd_deform / fd_deform_vectors on host arrays: staged through the context's device buffers, or -- page-locked arrays and
// no vectors -- read and written in place
static int deform_host(fd_ctx *ctx, const char *who, const Mesh &m, float *P_out, float *falloff_out, const fd_vectors *vec)
{
    const int64_t N = m.N;
    const float *const P_in = m.P, *const dist2 = m.dist2, *const tu = m.tu, *const tv = m.tv, *const nrm = m.nrm;
    int rc = mesh_checks(ctx, who, m, P_out != nullptr);
    if (rc || N == 0) return rc;
    if ((rc = use_device(ctx))) return rc;
    // Page-locked caller arrays (fd_host_alloc, hipHostMalloc, hipHostRegister): the kernel reads
    // and writes them in place over the host link -- reads and writes travel in both directions
    // at once and nothing is staged.  Measured at C2: 0.44 ms against 0.62 ms for upload +
    // evaluate + download (chunking those copies over two streams did not overlap them at all).
    const bool all_pinned = !vec && host_is_pinned(P_in) && host_is_pinned(P_out) && (!dist2 || host_is_pinned(dist2)) &&
                            (!falloff_out || host_is_pinned(falloff_out)) &&
                            (!tu || (host_is_pinned(tu) && host_is_pinned(tv) && host_is_pinned(nrm)));
    if (all_pinned) {
        bool ok = true;
        auto dp = [&ok](const void *h) -> void * {
            void *d = nullptr;
            if (!h) return nullptr;
            if (hipHostGetDevicePointer(&d, const_cast<void *>(h), 0) != hipSuccess) { (void)hipGetLastError(); ok = false; }
            return d;
        };
        const float *zP = (const float *)dp(P_in), *zD = (const float *)dp(dist2), *zU = (const float *)dp(tu),
                    *zV = (const float *)dp(tv), *zN = (const float *)dp(nrm);
        float *zO = (float *)dp(P_out), *zF = (float *)dp(falloff_out);
        if (ok) {
            hipStream_t s = cur_stream(ctx);
            rc = fd_deform_dev_stream(ctx, s, N, zP, zO, zD, zF, zU, zV, zN, m.radius2, m.falloffrate);
            if (rc) return rc;
            FD_HIP(ctx, hipStreamSynchronize(s));
            return FD_OK;
        }
    }
    // A vertex whose gate fails keeps the caller's fd_falloff entry, so that array goes up as
    // well -- unless no vertex can be gated (no dist2 and a non-negative radius^2).
    const bool fall_up = falloff_out && (dist2 || m.radius2 < 0.f);
    hipStream_t s = cur_stream(ctx);
    Mesh d;
    if ((rc = stage_mesh(ctx, m, s, &d, {}, Upload{&ctx->d_fall.p, fall_up ? falloff_out : nullptr, 1}))) return rc;
    const size_t b3 = sizeof(float) * 3 * (size_t)N, b1 = sizeof(float) * (size_t)N;
    // the vectors: each staged in its own device array and transported in place there
    fd_vectors dv{};
    if (vec) {
        if ((rc = dev_alloc(ctx, ctx->d_vec, (size_t)N * 18, kGrow))) return rc;
        float *const slot[4] = {ctx->d_vec, ctx->d_vec + 3 * N, ctx->d_vec + 6 * N, ctx->d_vec + 9 * N};
        const float *const in[3] = {vec->N, vec->tu, vec->tv};
        for (int k = 0; k < 3; ++k)
            if (in[k]) FD_HIP(ctx, hipMemcpyAsync(slot[k], in[k], b3, hipMemcpyHostToDevice, s));
        dv.struct_size = (int)sizeof(fd_vectors);
        if (vec->N) { dv.N = slot[0]; dv.N_out = slot[0]; }
        if (vec->tu) { dv.tu = slot[1]; dv.tu_out = slot[1]; }
        if (vec->tv) { dv.tv = slot[2]; dv.tv_out = slot[2]; }
        if (vec->jacobian) dv.jacobian = slot[3];
    }
    if ((rc = deform_dev(ctx, who, nullptr, d, ctx->d_P, falloff_out ? ctx->d_fall : nullptr, vec ? &dv : nullptr))) return rc;
    FD_HIP(ctx, hipMemcpyAsync(P_out, ctx->d_P, b3, hipMemcpyDeviceToHost, s));
    if (falloff_out) FD_HIP(ctx, hipMemcpyAsync(falloff_out, ctx->d_fall, b1, hipMemcpyDeviceToHost, s));
    if (vec) {
        if (vec->N) FD_HIP(ctx, hipMemcpyAsync(vec->N_out, dv.N_out, b3, hipMemcpyDeviceToHost, s));
        if (vec->tu) FD_HIP(ctx, hipMemcpyAsync(vec->tu_out, dv.tu_out, b3, hipMemcpyDeviceToHost, s));
        if (vec->tv) FD_HIP(ctx, hipMemcpyAsync(vec->tv_out, dv.tv_out, b3, hipMemcpyDeviceToHost, s));
        if (vec->jacobian) FD_HIP(ctx, hipMemcpyAsync(vec->jacobian, dv.jacobian, 3 * b3, hipMemcpyDeviceToHost, s));
    }
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

// fd_invert on host arrays: staged like deform_host with vectors (no zero-copy form); solved in place in d_P, residual_out
// through d_fall, iters_out through d_iters
static int invert_host(fd_ctx *ctx, const Mesh &m, float *X_out, const fd_invert_opts *opts)
{
    int rc = mesh_checks(ctx, "fd_invert", m, X_out != nullptr);
    if (rc || m.N == 0) return rc;
    if ((rc = use_device(ctx))) return rc;
    if (opts->iters_out && (rc = dev_alloc(ctx, ctx->d_iters, (size_t)m.N, kGrow))) return rc;
    hipStream_t s = cur_stream(ctx);
    Mesh d;
    if ((rc = stage_mesh(ctx, m, s, &d))) return rc;
    const InvertArgs inv{opts->max_iter, opts->tol, opts->residual_out ? ctx->d_fall : nullptr, opts->iters_out ? ctx->d_iters : nullptr};
    if ((rc = invert_dev(ctx, d, ctx->d_P, inv))) return rc;
    const size_t b1 = sizeof(float) * (size_t)m.N;
    FD_HIP(ctx, hipMemcpyAsync(X_out, ctx->d_P, 3 * b1, hipMemcpyDeviceToHost, s));
    if (opts->residual_out) FD_HIP(ctx, hipMemcpyAsync(opts->residual_out, ctx->d_fall, b1, hipMemcpyDeviceToHost, s));
    if (opts->iters_out) FD_HIP(ctx, hipMemcpyAsync(opts->iters_out, ctx->d_iters, sizeof(int) * (size_t)m.N, hipMemcpyDeviceToHost, s));
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

// fd_deform_adjoint on host arrays: staged like invert_host; G through d_vecP, grad_W through the block behind the partial sums
static int adjoint_host(fd_ctx *ctx, const char *who, const Mesh &m, const float *G, double *grad_W)
{
    int rc = mesh_checks(ctx, who, m, true);
    if (rc) return rc;
    const int C = model_centres(ctx);
    if (m.N == 0) { memset(grad_W, 0, sizeof(double) * adjoint_block(C)); return FD_OK; }
    if ((rc = use_device(ctx))) return rc;
    if ((rc = dev_alloc(ctx, ctx->d_vecP, (size_t)m.N * 3, kGrow))) return rc;
    if ((rc = dev_alloc(ctx, ctx->d_adj, adjoint_scratch(m.N, C), kGrow))) return rc;
    hipStream_t s = cur_stream(ctx);
    Mesh d;
    if ((rc = stage_mesh(ctx, m, s, &d, Upload{&ctx->d_vecP.p, G, 3}))) return rc;
    double *d_out = adjoint_staging(ctx, m.N, C);
    if ((rc = adjoint_dev(ctx, who, d, ctx->d_vecP, d_out))) return rc;
    FD_HIP(ctx, hipMemcpyAsync(grad_W, d_out, sizeof(double) * adjoint_block(C), hipMemcpyDeviceToHost, s));
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

// fd_deform_adjoint_points on host arrays: staged like adjoint_host, G through d_vecP behind P; grad_P and, behind it, grad_f
// come back from d_adjp
static int adjoint_points_host(fd_ctx *ctx, const char *who, const Mesh &m, const float *G, double *grad_P, double *grad_f)
{
    int rc = mesh_checks(ctx, who, m, true);
    if (rc || m.N == 0) return rc;
    if ((rc = use_device(ctx))) return rc;
    const size_t n = (size_t)m.N;
    if ((rc = dev_alloc(ctx, ctx->d_vecP, n * 3, kGrow))) return rc;
    if ((rc = dev_alloc(ctx, ctx->d_adjp, n * 4, kGrow))) return rc;
    hipStream_t s = cur_stream(ctx);
    Mesh d;
    if ((rc = stage_mesh(ctx, m, s, &d, Upload{&ctx->d_vecP.p, G, 3}))) return rc;
    double *d_f = grad_f ? ctx->d_adjp + n * 3 : nullptr;
    if ((rc = adjoint_points_dev(ctx, who, d, ctx->d_vecP, ctx->d_adjp, d_f))) return rc;
    FD_HIP(ctx, hipMemcpyAsync(grad_P, ctx->d_adjp, sizeof(double) * n * 3, hipMemcpyDeviceToHost, s));
    if (grad_f) FD_HIP(ctx, hipMemcpyAsync(grad_f, d_f, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

// The Gram operator of a mesh that stage_mesh has put on the device (d_omega: where its omega went, or null), H to the host: H
// is staged in the block behind the partial blocks.  An empty mesh gives zeros and touches no device.
static int gram_staged(fd_ctx *ctx, const char *who, const Mesh &d, const float *d_omega, double *H)
{
    const int C = model_centres(ctx), nq = d.tu ? 6 : 1;
    if (d.N == 0) { memset(H, 0, sizeof(double) * gram_block(C, nq)); return FD_OK; }
    int rc = dev_alloc(ctx, ctx->d_gram, gram_scratch(d.N, C, nq), kGrow);
    if (rc) return rc;
    hipStream_t s = cur_stream(ctx);
    double *d_out = gram_staging(ctx, d.N, C, nq);
    if ((rc = gram_dev(ctx, who, d, d_omega, d_out))) return rc;
    FD_HIP(ctx, hipMemcpyAsync(H, d_out, sizeof(double) * gram_block(C, nq), hipMemcpyDeviceToHost, s));
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

// fd_deform_gram on host arrays: omega goes up through d_fall
static int gram_host(fd_ctx *ctx, const char *who, const Mesh &m, const float *omega, double *H)
{
    int rc = mesh_checks(ctx, who, m, true);
    if (rc) return rc;
    Mesh d;
    if ((rc = stage_mesh(ctx, m, cur_stream(ctx), &d, Upload{&ctx->d_fall.p, omega, 1}))) return rc;
    return gram_staged(ctx, who, d, omega ? ctx->d_fall : nullptr, H);
}

// fd_deform_bake and fd_deform_bake_grad on host arrays: S (computed here where the caller has none) goes up behind the pack
// kernel's scratch, is packed once, and B and B32 (G and G32: k.comps rows of M per vertex) come back in chunks of vertices
// through d_bakeout (bake_chunk_vertices: the block stays within the operators' scratch bound).  A vertex's rows depend on
// nothing else in the launch, so the chunks are the bits of one launch.
static int bake_host(fd_ctx *ctx, const BakeCall &k, const Mesh &m, const double *S, double *B, float *B32)
{
    const char *who = k.who;
    int rc = mesh_checks(ctx, who, m, true);
    if (rc || m.N == 0) return rc;
    const int C = model_centres(ctx), M = ctx->M;
    const size_t s_doubles = (size_t)(C + 4) * (size_t)M;
    std::vector<double> S_own;
    if (!S) {
        S_own.resize(s_doubles);
        if ((rc = fd_solve_operator(ctx, S_own.data()))) return rc;
        S = S_own.data();
    }
    if ((rc = use_device(ctx))) return rc;
    hipStream_t s = cur_stream(ctx);
    Mesh d;
    if ((rc = stage_mesh(ctx, m, s, &d))) return rc;
    DeformArgs a;
    hipStream_t launch_stream;
    if ((rc = deform_begin(ctx, who, nullptr, d, nullptr, nullptr, true, &a, &launch_stream))) return rc;
    const size_t scratch = bake_scratch_doubles(C, M, k.comps);
    if ((rc = dev_alloc(ctx, ctx->d_bake, scratch + s_doubles, kGrow))) return rc;
    const int64_t per = bake_chunk_vertices(M, k.comps, B != nullptr, B32 != nullptr);
    const size_t vrow = (size_t)k.comps * (size_t)M;                    // entries per vertex
    const size_t chunk = (size_t)(m.N < per ? m.N : per) * vrow;
    if ((rc = dev_alloc(ctx, ctx->d_bakeout, (B ? chunk : 0) + (B32 ? (chunk + 1) / 2 : 0), kGrow))) return rc;
    double *d_S = ctx->d_bake + scratch;
    double *d_B = B ? ctx->d_bakeout.p : nullptr;
    float *d_B32 = B32 ? reinterpret_cast<float *>(ctx->d_bakeout + (B ? chunk : 0)) : nullptr;
    FD_HIP(ctx, hipMemcpyAsync(d_S, S, sizeof(double) * s_doubles, hipMemcpyHostToDevice, s));
    BakeArgs g{d_S, M, term_cols(ctx->term), ctx->d_bake, d_B, d_B32, k.comps};
    FD_HIP(ctx, launch_bake_pack(a, g, s));
    for (int64_t v0 = 0; v0 < m.N; v0 += per) {
        const int64_t n = m.N - v0 < per ? m.N - v0 : per;
        DeformArgs ac = a;
        ac.N = n;
        ac.P_in = d.P + 3 * v0;
        ac.dist2 = d.dist2 ? d.dist2 + v0 : nullptr;
        if (d.tu) { ac.tu = d.tu + 3 * v0; ac.tv = d.tv + 3 * v0; ac.nrm = d.nrm + 3 * v0; }
        FD_HIP(ctx, launch_bake(ac, g, s));
        const size_t at = (size_t)v0 * vrow, cnt = (size_t)n * vrow;
        if (B) FD_HIP(ctx, hipMemcpyAsync(B + at, d_B, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
        if (B32) FD_HIP(ctx, hipMemcpyAsync(B32 + at, d_B32, sizeof(float) * cnt, hipMemcpyDeviceToHost, s));
    }
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

// The shot adjoint of a mesh that stage_mesh has put on the device, for F cotangents G on the host: G goes through d_gshot
// one group of FD_MAX_BATCH frames at a time, each group's launches behind its copy on the stream; grad_W of all frames is staged
// behind the partial blocks and comes back in one copy.  An empty mesh gives zeros and touches no device.
static int adjoint_shot_staged(fd_ctx *ctx, const char *who, const Mesh &d, int F, const float *G, double *grad_W)
{
    const int C = model_centres(ctx);
    if (d.N == 0) { memset(grad_W, 0, sizeof(double) * (size_t)F * adjoint_block(C)); return FD_OK; }
    const int group = F < FD_MAX_BATCH ? F : FD_MAX_BATCH;
    const size_t frame = (size_t)d.N * 3;
    int rc;
    if ((rc = dev_alloc(ctx, ctx->d_gshot, (size_t)group * frame, kGrow))) return rc;
    if ((rc = dev_alloc(ctx, ctx->d_adjs, adjoint_shot_scratch(d.N, C, F), kGrow))) return rc;
    hipStream_t s = cur_stream(ctx);
    double *d_out = adjoint_shot_staging(ctx, d.N, C);
    for (int f0 = 0; f0 < F; f0 += FD_MAX_BATCH) {
        const int nF = F - f0 < FD_MAX_BATCH ? F - f0 : FD_MAX_BATCH;
        FD_HIP(ctx, hipMemcpyAsync(ctx->d_gshot, G + (size_t)f0 * frame, sizeof(float) * frame * (size_t)nF, hipMemcpyHostToDevice, s));
        if ((rc = adjoint_shot_dev(ctx, who, d, nF, ctx->d_gshot, d_out + (size_t)f0 * adjoint_block(C)))) return rc;
    }
    FD_HIP(ctx, hipMemcpyAsync(grad_W, d_out, sizeof(double) * (size_t)F * adjoint_block(C), hipMemcpyDeviceToHost, s));
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

// fd_deform_adjoint_shot on host arrays
static int adjoint_shot_host(fd_ctx *ctx, const char *who, const Mesh &m, int F, const float *G, double *grad_W)
{
    int rc = mesh_checks(ctx, who, m, true);
    if (rc) return rc;
    Mesh d;
    if ((rc = stage_mesh(ctx, m, cur_stream(ctx), &d))) return rc;
    return adjoint_shot_staged(ctx, who, d, F, G, grad_W);
}

extern "C" {

int fd_deform_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, float *d_P_out, const float *d_dist2,
                  float *d_falloff_out, const float *d_tu, const float *d_tv, const float *d_nrm,
                  float radius2, float falloffrate)
{
    if (!ctx) return FD_E_INVALID;
    return fd_deform_dev_stream(ctx, cur_stream(ctx), N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv,
                                d_nrm, radius2, falloffrate);
}

int fd_deform_dev_stream(fd_ctx *ctx, void *hip_stream, int64_t N, const float *d_P_in, float *d_P_out,
                         const float *d_dist2, float *d_falloff_out, const float *d_tu,
                         const float *d_tv, const float *d_nrm, float radius2, float falloffrate)
{
    if (!ctx) return FD_E_INVALID;
    return deform_dev(ctx, "fd_deform", hip_stream, Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_P_out,
                      d_falloff_out, nullptr);
}

int fd_deform_vectors_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, float *d_P_out, const float *d_dist2,
                          float *d_falloff_out, const float *d_tu, const float *d_tv, const float *d_nrm,
                          float radius2, float falloffrate, const fd_vectors *vec)
{
    if (!ctx) return FD_E_INVALID;
    if (!vectors_ok(ctx, vec)) return FD_E_INVALID;
    return deform_dev(ctx, "fd_deform_vectors", nullptr, Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_P_out,
                      d_falloff_out, vectors_wanted(vec) ? vec : nullptr);
}

int fd_deform(fd_ctx *ctx, int64_t N, const float *P_in, float *P_out, const float *dist2,
              float *falloff_out, const float *tu, const float *tv, const float *nrm, float radius2,
              float falloffrate)
{
    if (!ctx) return FD_E_INVALID;
    return deform_host(ctx, "fd_deform", Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, P_out, falloff_out, nullptr);
}

int fd_deform_vectors(fd_ctx *ctx, int64_t N, const float *P_in, float *P_out, const float *dist2,
                      float *falloff_out, const float *tu, const float *tv, const float *nrm,
                      float radius2, float falloffrate, const fd_vectors *vec)
{
    if (!ctx) return FD_E_INVALID;
    if (!vectors_ok(ctx, vec)) return FD_E_INVALID;
    return deform_host(ctx, "fd_deform_vectors", Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, P_out, falloff_out,
                       vectors_wanted(vec) ? vec : nullptr);
}

int fd_invert_dev(fd_ctx *ctx, int64_t N, const float *d_Y, float *d_X_out, const float *d_dist2, const float *d_tu,
                  const float *d_tv, const float *d_nrm, float radius2, float falloffrate, const fd_invert_opts *opts)
{
    if (!ctx) return FD_E_INVALID;
    if (!invert_opts_ok(ctx, opts)) return FD_E_INVALID;
    const InvertArgs inv{opts->max_iter, opts->tol, opts->residual_out, opts->iters_out};
    return invert_dev(ctx, Mesh{N, d_Y, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_X_out, inv);
}

int fd_invert(fd_ctx *ctx, int64_t N, const float *Y, float *X_out, const float *dist2, const float *tu, const float *tv,
              const float *nrm, float radius2, float falloffrate, const fd_invert_opts *opts)
{
    if (!ctx) return FD_E_INVALID;
    if (!invert_opts_ok(ctx, opts)) return FD_E_INVALID;
    if (N < 0 || (N > 0 && (!Y || !X_out))) { set_err(ctx, "fd_invert: bad N / Y / X_out pointers"); return FD_E_INVALID; }
    return invert_host(ctx, Mesh{N, Y, dist2, tu, tv, nrm, radius2, falloffrate}, X_out, opts);
}

int fd_deform_adjoint_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_G, const float *d_dist2, const float *d_tu,
                          const float *d_tv, const float *d_nrm, float radius2, float falloffrate, double *d_grad_W)
{
    if (!ctx) return FD_E_INVALID;
    if (!d_G || !d_grad_W || N < 0) { set_err(ctx, "fd_deform_adjoint: bad N / G / grad_W pointers"); return FD_E_INVALID; }
    int rc = adjoint_dev(ctx, "fd_deform_adjoint", Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_G, d_grad_W);
    if (rc || N > 0) return rc;
    // no vertex: no launch, zeros
    if ((rc = use_device(ctx))) return rc;
    FD_HIP(ctx, hipMemsetAsync(d_grad_W, 0, sizeof(double) * adjoint_block(model_centres(ctx)), cur_stream(ctx)));
    return FD_OK;
}

int fd_deform_adjoint(fd_ctx *ctx, int64_t N, const float *P_in, const float *G, const float *dist2, const float *tu, const float *tv,
                      const float *nrm, float radius2, float falloffrate, double *grad_W)
{
    if (!ctx) return FD_E_INVALID;
    if (!G || !grad_W || N < 0) { set_err(ctx, "fd_deform_adjoint: bad N / G / grad_W pointers"); return FD_E_INVALID; }
    return adjoint_host(ctx, "fd_deform_adjoint", Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, G, grad_W);
}

int fd_deform_adjoint_points_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_G, const float *d_dist2,
                                 const float *d_tu, const float *d_tv, const float *d_nrm, float radius2, float falloffrate,
                                 double *d_grad_P, const fd_adjoint_points_opts *opts)
{
    if (!ctx) return FD_E_INVALID;
    if (!d_G || !d_grad_P || N < 0) { set_err(ctx, "fd_deform_adjoint_points: bad N / G / grad_P pointers"); return FD_E_INVALID; }
    if (!adjoint_points_opts_ok(ctx, opts)) return FD_E_INVALID;
    return adjoint_points_dev(ctx, "fd_deform_adjoint_points", Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_G,
                              d_grad_P, opts ? opts->grad_f : nullptr);
}

int fd_deform_adjoint_points(fd_ctx *ctx, int64_t N, const float *P_in, const float *G, const float *dist2, const float *tu,
                             const float *tv, const float *nrm, float radius2, float falloffrate, double *grad_P,
                             const fd_adjoint_points_opts *opts)
{
    if (!ctx) return FD_E_INVALID;
    if (!G || !grad_P || N < 0) { set_err(ctx, "fd_deform_adjoint_points: bad N / G / grad_P pointers"); return FD_E_INVALID; }
    if (!adjoint_points_opts_ok(ctx, opts)) return FD_E_INVALID;
    return adjoint_points_host(ctx, "fd_deform_adjoint_points", Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, G, grad_P,
                               opts ? opts->grad_f : nullptr);
}

int fd_deform_gram_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_omega, const float *d_dist2, const float *d_tu,
                       const float *d_tv, const float *d_nrm, float radius2, float falloffrate, double *d_H)
{
    if (!ctx) return FD_E_INVALID;
    if (!d_H || N < 0) { set_err(ctx, "fd_deform_gram: bad N / H pointers"); return FD_E_INVALID; }
    int rc = gram_dev(ctx, "fd_deform_gram", Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_omega, d_H);
    if (rc || N > 0) return rc;
    // no vertex: no launch, zeros
    if ((rc = use_device(ctx))) return rc;
    FD_HIP(ctx, hipMemsetAsync(d_H, 0, sizeof(double) * gram_block(model_centres(ctx), d_tu ? 6 : 1), cur_stream(ctx)));
    return FD_OK;
}

int fd_deform_gram(fd_ctx *ctx, int64_t N, const float *P_in, const float *omega, const float *dist2, const float *tu, const float *tv,
                   const float *nrm, float radius2, float falloffrate, double *H)
{
    if (!ctx) return FD_E_INVALID;
    if (!H || N < 0) { set_err(ctx, "fd_deform_gram: bad N / H pointers"); return FD_E_INVALID; }
    return gram_host(ctx, "fd_deform_gram", Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, omega, H);
}

// fd_deform_bake* and fd_deform_bake_grad*: what both forms check before any device work
static int bake_checks(fd_ctx *ctx, const BakeCall &k, int64_t N, int M, const void *tu, const void *tv, const void *nrm,
                       const double *B, const fd_bake_opts *opts)
{
    if (N < 0) { set_err(ctx, "%s: N < 0", k.who); return FD_E_INVALID; }
    if (M != ctx->M) { set_err(ctx, "%s: M is %d, the context has %d control points", k.who, M, ctx->M); return FD_E_INVALID; }
    if (!bake_outputs_ok(ctx, k, B, opts)) return FD_E_INVALID;
    if (!frames_ok(tu, tv, nrm)) { set_err(ctx, "%s: tu, tv, nrm must be all set or all NULL", k.who); return FD_E_INVALID; }
    return FD_OK;
}

int fd_deform_bake_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_dist2, const float *d_tu, const float *d_tv,
                       const float *d_nrm, float radius2, float falloffrate, const double *d_S, int M, double *d_B,
                       const fd_bake_opts *opts)
{
    if (!ctx) return FD_E_INVALID;
    if (!d_S) { set_err(ctx, "fd_deform_bake: S is NULL"); return FD_E_INVALID; }
    if (int rc = bake_checks(ctx, kBake, N, M, d_tu, d_tv, d_nrm, d_B, opts)) return rc;
    return bake_dev(ctx, kBake, Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_S, d_B, opts ? opts->B32 : nullptr);
}

int fd_deform_bake(fd_ctx *ctx, int64_t N, const float *P_in, const float *dist2, const float *tu, const float *tv, const float *nrm,
                   float radius2, float falloffrate, const double *S, int M, double *B, const fd_bake_opts *opts)
{
    if (!ctx) return FD_E_INVALID;
    if (int rc = bake_checks(ctx, kBake, N, M, tu, tv, nrm, B, opts)) return rc;
    return bake_host(ctx, kBake, Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, S, B, opts ? opts->B32 : nullptr);
}

int fd_deform_bake_grad_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_dist2, const float *d_tu, const float *d_tv,
                            const float *d_nrm, float radius2, float falloffrate, const double *d_S, int M, double *d_G,
                            const fd_bake_grad_opts *opts)
{
    if (!ctx) return FD_E_INVALID;
    if (!d_S) { set_err(ctx, "fd_deform_bake_grad: S is NULL"); return FD_E_INVALID; }
    if (int rc = bake_checks(ctx, kBakeGrad, N, M, d_tu, d_tv, d_nrm, d_G, bake_opts_view(opts))) return rc;
    return bake_dev(ctx, kBakeGrad, Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_S, d_G,
                    opts ? opts->G32 : nullptr);
}

int fd_deform_bake_grad(fd_ctx *ctx, int64_t N, const float *P_in, const float *dist2, const float *tu, const float *tv,
                        const float *nrm, float radius2, float falloffrate, const double *S, int M, double *G,
                        const fd_bake_grad_opts *opts)
{
    if (!ctx) return FD_E_INVALID;
    if (int rc = bake_checks(ctx, kBakeGrad, N, M, tu, tv, nrm, G, bake_opts_view(opts))) return rc;
    return bake_host(ctx, kBakeGrad, Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, S, G, opts ? opts->G32 : nullptr);
}

int fd_deform_adjoint_shot_dev(fd_ctx *ctx, int64_t N, int F, const float *d_P_in, const float *d_G, const float *d_dist2,
                               const float *d_tu, const float *d_tv, const float *d_nrm, float radius2, float falloffrate,
                               double *d_grad_W)
{
    if (!ctx) return FD_E_INVALID;
    if (!d_G || !d_grad_W || N < 0 || F < 1) { set_err(ctx, "fd_deform_adjoint_shot: bad N / F / G / grad_W pointers"); return FD_E_INVALID; }
    int rc = adjoint_shot_dev(ctx, "fd_deform_adjoint_shot", Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, F, d_G,
                              d_grad_W);
    if (rc || N > 0) return rc;
    // no vertex: no launch, zeros
    if ((rc = use_device(ctx))) return rc;
    FD_HIP(ctx, hipMemsetAsync(d_grad_W, 0, sizeof(double) * (size_t)F * adjoint_block(model_centres(ctx)), cur_stream(ctx)));
    return FD_OK;
}

int fd_deform_adjoint_shot(fd_ctx *ctx, int64_t N, int F, const float *P_in, const float *G, const float *dist2, const float *tu,
                           const float *tv, const float *nrm, float radius2, float falloffrate, double *grad_W)
{
    if (!ctx) return FD_E_INVALID;
    if (!G || !grad_W || N < 0 || F < 1) { set_err(ctx, "fd_deform_adjoint_shot: bad N / F / G / grad_W pointers"); return FD_E_INVALID; }
    return adjoint_shot_host(ctx, "fd_deform_adjoint_shot", Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, F, G, grad_W);
}

}  // extern "C"

// ---- fillers of the shot launches' argument structs (fd_batch_deform_*shared*_dev below; templates, so outside the C linkage block) ----
// the mesh part of a launch's arguments (SharedDeformArgs, SharedEvalCommon and SharedVectorCommon name these fields alike)
template <typename Args>
static void fill_mesh(Args &a, int64_t N, const float *d_P_in, const float *d_dist2, const float *d_tu, const float *d_tv,
                      const float *d_nrm, float radius2, float falloffrate)
{
    a.N = N; a.P_in = d_P_in; a.dist2 = d_dist2; a.tu = d_tu; a.tv = d_tv; a.nrm = d_nrm;
    a.radius2 = radius2; a.falloffrate = falloffrate;
}

// what the three staged position launches' arguments have in common (SharedEvalCommon), on the scratch shot_reserve gave
static void fill_eval_common(SharedEvalCommon &a, const fd_batch *b, const ShotScratch &sc, int64_t N, const float *d_P_in,
                             float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out, const float *d_tu,
                             const float *d_tv, const float *d_nrm, float radius2, float falloffrate)
{
    fill_mesh(a, N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate);
    a.nF = b->n;
    for (int i = 0; i < b->n; ++i) { a.model[i] = b->ctxs[i]->d_model; a.P_out[i] = d_P_out ? d_P_out[i] : nullptr; }      // (no table: a call without position outputs)
    a.falloff_out = d_falloff_out;
    a.delta_out = b->ctxs[0]->output == FD_OUTPUT_DISPLACEMENT;
    a.max_wgs = b->eval_cus;
    a.scratch = sc.d;
    a.packed_ev = sc.consumed_ev;
    if (b->h_mismatch && hipHostGetDevicePointer((void **)&a.mismatch, b->h_mismatch, 0) != hipSuccess) { (void)hipGetLastError(); a.mismatch = nullptr; }
}

// the vector tables of a SharedVector*Args
template <typename Args>
static void fill_vector_tables(Args &a, int n, const fd_batch_vectors *vec)
{
    a.vN = vec->N; a.vtu = vec->tu; a.vtv = vec->tv;
    for (int i = 0; i < n; ++i) {
        a.N_out[i] = vec->N ? vec->N_out[i] : nullptr;
        a.tu_out[i] = vec->tu ? vec->tu_out[i] : nullptr;
        a.tv_out[i] = vec->tv ? vec->tv_out[i] : nullptr;
        a.jacobian[i] = vec->jacobian ? vec->jacobian[i] : nullptr;
    }
}

extern "C" {

// ---- dist2 producer (next row N2; kernel in fd_capture.hip) -----------------------------------
int fd_capture_dist2_dev(fd_ctx *ctx, int64_t N, const float *d_P, const unsigned char *d_mask, int T,
                         const float *d_tri_xyz, float radius2, int dofalloff, float *d_dist2)
{
    if (!ctx) return FD_E_INVALID;
    if (N < 0 || T < 0 || (N > 0 && (!d_P || !d_dist2)) || (T > 0 && !d_tri_xyz)) {
        set_err(ctx, "fd_capture_dist2: bad sizes or NULL arrays");
        return FD_E_INVALID;
    }
    int rc = use_device(ctx);
    if (rc) return rc;
    FD_HIP(ctx, launch_capture_dist2(d_P, N, d_mask, d_tri_xyz, T, radius2, dofalloff, d_dist2, cur_stream(ctx)));
    return FD_OK;
}

int fd_capture_dist2(fd_ctx *ctx, int64_t N, const float *P, const unsigned char *mask, int T, const float *tri_xyz,
                     float radius2, int dofalloff, float *dist2)
{
    if (!ctx) return FD_E_INVALID;
    if (N < 0 || T < 0 || (N > 0 && (!P || !dist2)) || (T > 0 && !tri_xyz)) {
        set_err(ctx, "fd_capture_dist2: bad sizes or NULL arrays");
        return FD_E_INVALID;
    }
    if (N == 0) return FD_OK;
    int rc = use_device(ctx);
    if (rc) return rc;
    hipStream_t s = cur_stream(ctx);
    DevBuf<float> d_P, d_tri, d_out;         // released on the way out
    DevBuf<unsigned char> d_mask;
    hipError_t e = d_P.alloc(3 * (size_t)N);
    if (e == hipSuccess) e = d_out.alloc((size_t)N);
    if (e == hipSuccess && T > 0) e = d_tri.alloc(9 * (size_t)T);
    if (e == hipSuccess && mask) e = d_mask.alloc((size_t)N);
    if (e == hipSuccess) e = hipMemcpyAsync(d_P, P, sizeof(float) * 3 * (size_t)N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && T > 0) e = hipMemcpyAsync(d_tri, tri_xyz, sizeof(float) * 9 * (size_t)T, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && mask) e = hipMemcpyAsync(d_mask, mask, (size_t)N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_capture_dist2(d_P, N, d_mask, d_tri, T, radius2, dofalloff, d_out, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dist2, d_out, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_err(ctx, "fd_capture_dist2 failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    return FD_OK;
}

int fd_capture_islands_dev(fd_ctx *ctx, int64_t N, const float *d_P, const int64_t *d_offsets, const int *d_neighbours,
                           int M, const float *d_rig_xyz, int max_edges, unsigned char *d_mask)
{
    if (!ctx) return FD_E_INVALID;
    if (N < 0 || M < 0 || max_edges < 0 || (N > 0 && (!d_P || !d_offsets || !d_mask)) || (M > 0 && !d_rig_xyz)) {
        set_err(ctx, "fd_capture_islands: bad sizes or NULL arrays");
        return FD_E_INVALID;
    }
    int rc = use_device(ctx);
    if (rc) return rc;
    FD_HIP(ctx, launch_capture_islands(d_P, N, d_offsets, d_neighbours, d_rig_xyz, M, max_edges, d_mask, cur_stream(ctx)));
    return FD_OK;
}

int fd_capture_islands(fd_ctx *ctx, int64_t N, const float *P, const int64_t *offsets, const int *neighbours, int M,
                       const float *rig_xyz, int max_edges, unsigned char *mask)
{
    if (!ctx) return FD_E_INVALID;
    if (N < 0 || M < 0 || max_edges < 0 || (N > 0 && (!P || !offsets || !mask)) || (M > 0 && !rig_xyz)) {
        set_err(ctx, "fd_capture_islands: bad sizes or NULL arrays");
        return FD_E_INVALID;
    }
    if (N == 0) return FD_OK;
    const int64_t E = offsets[N];
    if (E < 0 || (E > 0 && !neighbours)) { set_err(ctx, "fd_capture_islands: bad adjacency"); return FD_E_INVALID; }
    int rc = use_device(ctx);
    if (rc) return rc;
    hipStream_t s = cur_stream(ctx);
    DevBuf<float> d_P, d_rig;                // released on the way out
    DevBuf<int64_t> d_off;
    DevBuf<int> d_nb;
    DevBuf<unsigned char> d_mask;
    hipError_t e = d_P.alloc(3 * (size_t)N);
    if (e == hipSuccess) e = d_off.alloc((size_t)(N + 1));
    if (e == hipSuccess) e = d_nb.alloc((size_t)(E > 0 ? E : 1));
    if (e == hipSuccess) e = d_mask.alloc((size_t)N);
    if (e == hipSuccess && M > 0) e = d_rig.alloc(3 * (size_t)M);
    if (e == hipSuccess) e = hipMemcpyAsync(d_P, P, sizeof(float) * 3 * (size_t)N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, offsets, sizeof(int64_t) * (size_t)(N + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && E > 0) e = hipMemcpyAsync(d_nb, neighbours, sizeof(int) * (size_t)E, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && M > 0) e = hipMemcpyAsync(d_rig, rig_xyz, sizeof(float) * 3 * (size_t)M, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_capture_islands(d_P, N, d_off, d_nb, d_rig, M, max_edges, d_mask, s);
    if (e == hipSuccess) e = hipMemcpyAsync(mask, d_mask, (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_err(ctx, "fd_capture_islands failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    return FD_OK;
}

void *fd_host_alloc(size_t bytes)
{
    Pinned<void> h;
    if (h.alloc(bytes, hipHostMallocDefault) != hipSuccess) {
        set_err(nullptr, "fd_host_alloc(%zu) failed: %s", bytes, hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    return h.release();         // the caller's, until fd_host_free
}

void fd_host_free(void *p)
{
    Pinned<void> h;
    h.adopt(p);                 // released on the way out
}

// ---- device-resident mesh (next row N3, engine side) ----------------------------------------
int fd_mesh_set(fd_ctx *ctx, int64_t N, const float *P, const float *dist2, const float *tu, const float *tv,
                const float *nrm)
{
    if (!ctx) return FD_E_INVALID;
    if (N <= 0 || !P) { set_err(ctx, "fd_mesh_set: need N > 0 and P"); return FD_E_INVALID; }
    if (!frames_ok(tu, tv, nrm)) { set_err(ctx, "fd_mesh_set: tu, tv, nrm must be all set or all NULL"); return FD_E_INVALID; }
    int rc = use_device(ctx);
    if (rc) return rc;
    ctx->mesh_N = 0;
    if (N > ctx->mesh_cap) {
        if ((rc = dev_alloc(ctx, ctx->m_P, (size_t)N * 3))) return rc;
        for (DevBuf<float> *b : {&ctx->m_dist2, &ctx->m_tu, &ctx->m_tv, &ctx->m_nrm, &ctx->m_out, &ctx->m_fall}) b->reset();
        ctx->mesh_cap = N;
    }
    if (dist2 && !ctx->m_dist2 && (rc = dev_alloc(ctx, ctx->m_dist2, (size_t)ctx->mesh_cap))) return rc;
    if (tu && !ctx->m_tu) {
        if ((rc = dev_alloc(ctx, ctx->m_tu, (size_t)ctx->mesh_cap * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->m_tv, (size_t)ctx->mesh_cap * 3))) return rc;
        if ((rc = dev_alloc(ctx, ctx->m_nrm, (size_t)ctx->mesh_cap * 3))) return rc;
    }
    hipStream_t s = cur_stream(ctx);
    const size_t b3 = sizeof(float) * 3 * (size_t)N, b1 = sizeof(float) * (size_t)N;
    FD_HIP(ctx, hipMemcpyAsync(ctx->m_P, P, b3, hipMemcpyHostToDevice, s));
    if (dist2) FD_HIP(ctx, hipMemcpyAsync(ctx->m_dist2, dist2, b1, hipMemcpyHostToDevice, s));
    if (tu) {
        FD_HIP(ctx, hipMemcpyAsync(ctx->m_tu, tu, b3, hipMemcpyHostToDevice, s));
        FD_HIP(ctx, hipMemcpyAsync(ctx->m_tv, tv, b3, hipMemcpyHostToDevice, s));
        FD_HIP(ctx, hipMemcpyAsync(ctx->m_nrm, nrm, b3, hipMemcpyHostToDevice, s));
    }
    FD_HIP(ctx, hipStreamSynchronize(s));      // the caller's arrays may change after this returns
    ctx->mesh_N = N;
    ctx->mesh_has_dist2 = dist2 != nullptr;
    ctx->mesh_has_frames = tu != nullptr;
    return FD_OK;
}

int64_t fd_mesh_size(const fd_ctx *ctx) { return ctx ? ctx->mesh_N : 0; }

int fd_deform_mesh(fd_ctx *ctx, float *P_out, float *falloff_out, float radius2, float falloffrate)
{
    if (!ctx) return FD_E_INVALID;
    if (ctx->mesh_N <= 0) { set_err(ctx, "fd_deform_mesh: fd_mesh_set has not been called"); return FD_E_INVALID; }
    if (!P_out) { set_err(ctx, "fd_deform_mesh: P_out is NULL"); return FD_E_INVALID; }
    if (!ctx->built && !ctx->build_pending) { set_err(ctx, "fd_deform_mesh: no successfully built model"); return FD_E_NOT_BUILT; }
    int rc = use_device(ctx);
    if (rc) return rc;
    const int64_t N = ctx->mesh_N;
    hipStream_t s = cur_stream(ctx);
    const float *d2 = ctx->mesh_has_dist2 ? ctx->m_dist2 : nullptr;
    const float *tu = ctx->mesh_has_frames ? ctx->m_tu : nullptr, *tv = ctx->mesh_has_frames ? ctx->m_tv : nullptr,
                *nr = ctx->mesh_has_frames ? ctx->m_nrm : nullptr;
    // page-locked outputs: the kernel reads the mesh from HBM and writes the results straight
    // into the caller's arrays -- the only traffic on the host link is the result itself
    if (host_is_pinned(P_out) && (!falloff_out || host_is_pinned(falloff_out))) {
        void *zo = nullptr, *zf = nullptr;
        bool ok = hipHostGetDevicePointer(&zo, P_out, 0) == hipSuccess;
        if (ok && falloff_out) ok = hipHostGetDevicePointer(&zf, falloff_out, 0) == hipSuccess;
        if (ok) {
            rc = fd_deform_dev_stream(ctx, s, N, ctx->m_P, (float *)zo, d2, (float *)zf, tu, tv, nr, radius2, falloffrate);
            if (rc) return rc;
            FD_HIP(ctx, hipStreamSynchronize(s));
            return FD_OK;
        }
        (void)hipGetLastError();
    }
    if (!ctx->m_out && (rc = dev_alloc(ctx, ctx->m_out, (size_t)ctx->mesh_cap * 3))) return rc;
    if (falloff_out && !ctx->m_fall && (rc = dev_alloc(ctx, ctx->m_fall, (size_t)ctx->mesh_cap))) return rc;
    const size_t b3 = sizeof(float) * 3 * (size_t)N, b1 = sizeof(float) * (size_t)N;
    // a gated vertex keeps the caller's fd_falloff entry (see fd_deform)
    if (falloff_out && (d2 || radius2 < 0.f)) FD_HIP(ctx, hipMemcpyAsync(ctx->m_fall, falloff_out, b1, hipMemcpyHostToDevice, s));
    rc = fd_deform_dev_stream(ctx, s, N, ctx->m_P, ctx->m_out, d2, falloff_out ? ctx->m_fall : nullptr, tu, tv, nr, radius2,
                              falloffrate);
    if (rc) return rc;
    FD_HIP(ctx, hipMemcpyAsync(P_out, ctx->m_out, b3, hipMemcpyDeviceToHost, s));
    if (falloff_out) FD_HIP(ctx, hipMemcpyAsync(falloff_out, ctx->m_fall, b1, hipMemcpyDeviceToHost, s));
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

// ProximityCapture on the device-resident mesh: islands, then squared distances, into m_dist2
int fd_mesh_capture(fd_ctx *ctx, const int64_t *offsets, const int *neighbours, int M, const float *rig_xyz,
                    int max_edges, int T, const float *tri_xyz, float radius2, int dofalloff, float *dist2_out)
{
    if (!ctx) return FD_E_INVALID;
    const int64_t N = ctx->mesh_N;
    if (N <= 0) { set_err(ctx, "fd_mesh_capture: fd_mesh_set has not been called"); return FD_E_INVALID; }
    if (!offsets || M < 0 || T < 0 || max_edges < 0 || (M > 0 && !rig_xyz) || (T > 0 && !tri_xyz)) {
        set_err(ctx, "fd_mesh_capture: bad sizes or NULL arrays");
        return FD_E_INVALID;
    }
    const int64_t E = offsets[N];
    if (offsets[0] != 0 || E < 0 || (E > 0 && !neighbours)) { set_err(ctx, "fd_mesh_capture: bad adjacency"); return FD_E_INVALID; }
    int rc = use_device(ctx);
    if (rc) return rc;
    if (!ctx->m_dist2 && (rc = dev_alloc(ctx, ctx->m_dist2, (size_t)ctx->mesh_cap))) return rc;
    hipStream_t s = cur_stream(ctx);
    DevBuf<float> d_rig, d_tri;              // released on the way out
    DevBuf<int64_t> d_off;
    DevBuf<int> d_nb;
    DevBuf<unsigned char> d_mask;
    hipError_t e = d_off.alloc((size_t)(N + 1));
    if (e == hipSuccess) e = d_nb.alloc((size_t)(E > 0 ? E : 1));
    if (e == hipSuccess) e = d_mask.alloc((size_t)N);
    if (e == hipSuccess) e = d_rig.alloc(3 * (size_t)(M > 0 ? M : 1));
    if (e == hipSuccess) e = d_tri.alloc(9 * (size_t)(T > 0 ? T : 1));
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, offsets, sizeof(int64_t) * (size_t)(N + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && E > 0) e = hipMemcpyAsync(d_nb, neighbours, sizeof(int) * (size_t)E, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && M > 0) e = hipMemcpyAsync(d_rig, rig_xyz, sizeof(float) * 3 * (size_t)M, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && T > 0) e = hipMemcpyAsync(d_tri, tri_xyz, sizeof(float) * 9 * (size_t)T, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_capture_islands(ctx->m_P, N, d_off, d_nb, d_rig, M, max_edges, d_mask, s);
    if (e == hipSuccess) e = launch_capture_dist2(ctx->m_P, N, d_mask, d_tri, T, radius2, dofalloff, ctx->m_dist2, s);
    if (e == hipSuccess && dist2_out) e = hipMemcpyAsync(dist2_out, ctx->m_dist2, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipGetLastError(); set_err(ctx, "fd_mesh_capture failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    ctx->mesh_has_dist2 = true;
    return FD_OK;
}

int fd_mesh_get_dist2(fd_ctx *ctx, float *dist2_out)
{
    if (!ctx || !dist2_out) return FD_E_INVALID;
    if (ctx->mesh_N <= 0 || !ctx->mesh_has_dist2 || !ctx->m_dist2) { set_err(ctx, "fd_mesh_get_dist2: the mesh has no dist2 array"); return FD_E_INVALID; }
    int rc = use_device(ctx);
    if (rc) return rc;
    hipStream_t s = cur_stream(ctx);
    FD_HIP(ctx, hipMemcpyAsync(dist2_out, ctx->m_dist2, sizeof(float) * (size_t)ctx->mesh_N, hipMemcpyDeviceToHost, s));
    FD_HIP(ctx, hipStreamSynchronize(s));
    return FD_OK;
}

static int require_built(fd_ctx *ctx, const char *who)
{
    if (ctx->build_pending) {
        int rc = fd_build_result(ctx, nullptr);
        if (rc) return rc;
    }
    if (!ctx->built) { set_err(ctx, "%s: no successfully built model", who); return FD_E_NOT_BUILT; }
    return FD_OK;
}

int fd_model_centres(const fd_ctx *ctx) { return ctx ? model_centres(ctx) : 0; }

int fd_get_weights(fd_ctx *ctx, double *W, double *radii)
{
    if (!ctx || !W) return FD_E_INVALID;
    int rc = use_device(ctx);
    if (rc) return rc;
    if ((rc = require_built(ctx, "fd_get_weights"))) return rc;
    const int n = model_centres(ctx);
    FD_HIP(ctx, hipMemcpyAsync(W, ctx->d_W, sizeof(double) * 3 * (size_t)(n + 4), hipMemcpyDeviceToHost, cur_stream(ctx)));
    if (radii) FD_HIP(ctx, hipMemcpyAsync(radii, ctx->d_radii, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, cur_stream(ctx)));
    FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    return FD_OK;
}

static size_t model_bytes_for(int M)
{
    return sizeof(ModelHeader) + sizeof(double) * ((size_t)M * 3 + (size_t)M + (size_t)(M + 4) * 3);
}

size_t fd_model_bytes(const fd_ctx *ctx) { return ctx ? model_bytes_for(model_centres(ctx)) : 0; }

int fd_export_model(fd_ctx *ctx, void *buf, size_t capacity, int on_device)
{
    if (!ctx || !buf) return FD_E_INVALID;
    int rc = use_device(ctx);
    if (rc) return rc;
    if ((rc = require_built(ctx, "fd_export_model"))) return rc;
    // a multilayer model travels as what it is once solved: M * layers Gaussians with their own radii
    const int M = model_centres(ctx);
    if (capacity < model_bytes_for(M)) { set_err(ctx, "fd_export_model: buffer too small"); return FD_E_INVALID; }
    // the pinned header may still be the source of an earlier in-flight copy
    FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    ModelHeader *h = ctx->h_header;
    memset(h, 0, sizeof(*h));
    h->magic = kModelMagic;
    h->M = M; h->kind = eval_kind(ctx); h->term = ctx->term; h->nparams = ctx->nparams;
    h->terminationtype = 1;
    h->layers = record_layers(ctx);
    memcpy(h->params, ctx->params, sizeof(h->params));
    h->rig_token = (uint64_t)(uintptr_t)ctx->rest_src;
    char *p = (char *)buf;
    const hipMemcpyKind kh = on_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
    const hipMemcpyKind kd = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    FD_HIP(ctx, hipMemcpyAsync(p, h, sizeof(*h), kh, cur_stream(ctx)));
    p += sizeof(*h);
    FD_HIP(ctx, hipMemcpyAsync(p, ctx->d_centres, sizeof(double) * 3 * (size_t)M, kd, cur_stream(ctx)));
    p += sizeof(double) * 3 * (size_t)M;
    FD_HIP(ctx, hipMemcpyAsync(p, ctx->d_radii, sizeof(double) * (size_t)M, kd, cur_stream(ctx)));
    p += sizeof(double) * (size_t)M;
    FD_HIP(ctx, hipMemcpyAsync(p, ctx->d_W, sizeof(double) * 3 * (size_t)(M + 4), kd, cur_stream(ctx)));
    if (!on_device) FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    return FD_OK;
}

int fd_import_model(fd_ctx *ctx, const void *buf, size_t bytes, int on_device)
{
    if (!ctx || !buf || bytes < sizeof(ModelHeader)) return FD_E_INVALID;
    int rc = use_device(ctx);
    if (rc) return rc;
    ModelHeader h;
    if (on_device) {
        FD_HIP(ctx, hipMemcpyAsync(ctx->h_header, buf, sizeof(h), hipMemcpyDeviceToHost, cur_stream(ctx)));
        FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
        h = *ctx->h_header;
    } else {
        memcpy(&h, buf, sizeof(h));
    }
    if (h.magic != kModelMagic || h.M <= 0 || h.M > kMaxOrder * kMaxLayers || h.kind < 0 || h.kind > FD_KERNEL_CUBIC ||
        h.term < 0 || h.term > 2 || h.terminationtype != 1 || bytes < model_bytes_for(h.M) ||
        h.layers < 0 || h.layers > kMaxLayers || (h.layers > 1 && h.M % h.layers != 0)) {
        set_err(ctx, "fd_import_model: not a valid model blob");
        return FD_E_INVALID;
    }
    const int M = h.M;
    if ((rc = ensure_model_capacity(ctx, M))) return rc;
    ctx->M = M; ctx->kind = h.kind; ctx->term = h.term; ctx->nparams = h.nparams;
    ctx->imported_layers = h.layers > 1 ? h.layers : 0;
    memcpy(ctx->params, h.params, sizeof(h.params));
    const char *p = (const char *)buf + sizeof(ModelHeader);
    const hipMemcpyKind kd = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    FD_HIP(ctx, hipMemcpyAsync(ctx->d_centres, p, sizeof(double) * 3 * (size_t)M, kd, cur_stream(ctx)));
    p += sizeof(double) * 3 * (size_t)M;
    FD_HIP(ctx, hipMemcpyAsync(ctx->d_radii, p, sizeof(double) * (size_t)M, kd, cur_stream(ctx)));
    p += sizeof(double) * (size_t)M;
    FD_HIP(ctx, hipMemcpyAsync(ctx->d_W, p, sizeof(double) * 3 * (size_t)(M + 4), kd, cur_stream(ctx)));
    if ((rc = sync_slot(ctx))) return rc;
    BuildBuffers b;
    fill_build_buffers(ctx, b);
    FD_HIP(ctx, launch_pack_from_weights(b, cur_stream(ctx), ctx->imported_layers));
    FD_HIP(ctx, hipEventRecord(ctx->ev1, cur_stream(ctx)));
    ctx->wait_event = ctx->ev1; ctx->wait_stream = cur_stream(ctx); ctx->wait_batch = nullptr;      // evaluations on other streams wait for the pack
    if (!on_device) FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));
    ctx->have_factor = false;
    ctx->deltas_only = false;
    ++ctx->model_gen;
    ctx->points_set = false;   // no rest/delta on this context: it can deform, not rebuild
    // never dereferenced, only compared: bit 0 marks an imported identity (arrays are at least 4-byte aligned), so that it
    // can only ever equal another imported model's
    ctx->rig_build_id = 0;
    ctx->rest_src = h.rig_token ? (const float *)(uintptr_t)(h.rig_token | 1u) : nullptr;
    ctx->build_pending = false;
    ctx->built = true;
    fd_report r{};
    r.terminationtype = 1;
    r.n = order_of(ctx);
    ctx->report = r;
    ctx->have_report = true;
    return FD_OK;
}

// ---- batched build ----------------------------------------------------------------
// Several contexts with the same M, kernel, parameters and term -- frames of one rig, or the
// nodes of one cook graph -- are assembled and factorised by ONE launch chain: grid z selects
// the context.  A lone build of this size keeps one CU busy through ~25 dependent launches and
// the device overlaps only two or three such chains, so throughput-oriented callers batch.
static void batch_err(fd_batch *b, const char *fmt, ...)
{
    char *dst = b ? b->err : g_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
}

fd_batch *fd_batch_create(fd_ctx *const *ctxs, int n)
{
    if (!ctxs || n <= 0 || n > kMaxBatch) { set_err(nullptr, "fd_batch_create: need 1..%d contexts", kMaxBatch); return nullptr; }
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i] || ctxs[i]->device != ctxs[0]->device) { set_err(nullptr, "fd_batch_create: contexts must exist and share one device"); return nullptr; }
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) { set_err(nullptr, "fd_batch_create: context listed twice"); return nullptr; }
    }
    fd_batch *b = new (std::nothrow) fd_batch();
    if (!b) { set_err(nullptr, "fd_batch_create: out of host memory"); return nullptr; }
    b->n = n;
    b->device = ctxs[0]->device;
    for (int i = 0; i < n; ++i) b->ctxs[i] = ctxs[i];
    bool ok = hipSetDevice(b->device) == hipSuccess;
    ok = ok && b->d_slots.alloc((size_t)n) == hipSuccess;
    ok = ok && b->ev0.create(hipEventDefault) == hipSuccess && b->ev_mid.create(hipEventDefault) == hipSuccess &&
         b->ev1.create(hipEventDefault) == hipSuccess;
    ok = ok && b->status_ev.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && b->h_mismatch.alloc(1, hipHostMallocMapped) == hipSuccess;
    if (ok) *b->h_mismatch = 0;
    if (!ok) {
        set_err(nullptr, "fd_batch_create: device resource allocation failed: %s", hipGetErrorString(hipGetLastError()));
        fd_batch_destroy(b);
        return nullptr;
    }
    return b;
}

void fd_batch_destroy(fd_batch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        if (c && c->wait_event == b->ev1) {
            if (c->wait_stream) (void)hipStreamSynchronize(c->wait_stream);
            c->wait_event = nullptr; c->wait_stream = nullptr; c->wait_batch = nullptr;
        }
        if (c && c->tev0 == b->ev0) { c->tev0 = c->ev0; c->tev_mid = c->ev_mid; c->tev1 = c->ev1; }
        if (c && (c->status_poll == b->status_ev || c->status_poll == b->ev1)) { c->status_poll = c->status_ev; c->status_inflight = false; }
    }
    delete b;                   // the members release what they own
}

const char *fd_batch_last_error(const fd_batch *b) { return b ? b->err : g_err; }

int fd_batch_set_points_dev(fd_batch *b, const float *const *d_rest_xyz, const float *const *d_delta_xyz, int M)
{
    if (!b || !d_rest_xyz || !d_delta_xyz) return FD_E_INVALID;
    if (M <= 0 || M + 4 > kMaxOrder) { batch_err(b, "fd_batch_set_points_dev: M = %d outside 1..%d", M, kMaxOrder - 4); return FD_E_INVALID; }
    b->prepared = false;
    if (b->h_mismatch && *b->h_mismatch != 0) {
        // The pack kernel of the batch's PREVIOUS evaluation found a context built on other rest points than context 0 (same
        // address, other contents) and passed its frame through.  It posts the word asynchronously; a pipeline comes through
        // here before it ever polls (the word was cleared unseen): report it now, once, then start clean.
        const int who = *b->h_mismatch - 1;
        *b->h_mismatch = 0;
        batch_err(b, "shared-rig evaluation of the previous group: context %d was built on other rest points than context 0 (same "
                     "address, other contents); its frame was passed through", who);
        return FD_E_INVALID;
    }
    for (int i = 0; i < b->n; ++i)
        if (!d_rest_xyz[i] || !d_delta_xyz[i]) { batch_err(b, "fd_batch_set_points_dev: null array for context %d", i); return FD_E_INVALID; }
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        int rc = use_device(c);
        if (!rc) rc = ensure_model_capacity(c, M);
        if (rc) { batch_err(b, "context %d: %s", i, c->err); return rc; }
        c->M = M;
        c->points_set = true;
        c->built = false;
        c->build_pending = false;
        c->have_factor = false;
        c->deltas_only = false;
        c->rest_src = d_rest_xyz[i];
        c->rig_build_id = 0;
        b->src.rest[i] = d_rest_xyz[i];
        b->src.delta[i] = d_delta_xyz[i];
    }
    b->have_src = true;
    return FD_OK;
}

int fd_batch_build_async(fd_batch *b, void *hip_stream)
{
    if (!b) return FD_E_INVALID;
    b->prepared = false;
    fd_ctx *c0 = b->ctxs[0];
    int rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        if (!c->points_set) { batch_err(b, "fd_batch_build: context %d has no control points", i); return FD_E_INVALID; }
        c->imported_layers = 0;
        if (!same_model(c, c0)) {
            batch_err(b, "fd_batch_build: context %d differs from context 0 in M, kernel, parameters or term", i);
            return FD_E_INVALID;
        }
    }
    const int npad = round_up(order_of(c0), 32);
    bool table_stale = false;
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        const bool grew = npad > c->cap_npad;
        if ((rc = ensure_solver_capacity(c, npad)) || (rc = ensure_records_capacity(c, model_centres(c))) || (rc = sync_slot(c))) {
            batch_err(b, "context %d: %s", i, c->err);
            return rc;
        }
        if (grew) {
            const size_t cols = (size_t)c->cap_npad + kRhsCols + 16;
            hipError_t e = hipMemsetAsync(c->d_A, 0, sizeof(double) * (size_t)c->cap_npad * cols, stream);
            if (e != hipSuccess) { batch_err(b, "hipMemsetAsync failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
        }
        if (b->gens[i] != c->alloc_gen) table_stale = true;
    }
    if (table_stale) {
        b->qnn_slot_ready = false;       // the scratch slot of the shared QNN build borrows context 0's buffers
        BatchSlot tab[kMaxBatch];
        for (int i = 0; i < b->n; ++i) { tab[i] = b->ctxs[i]->h_slot; b->gens[i] = b->ctxs[i]->alloc_gen; }
        // buffers only move through hipFree, which has drained the device: nobody reads the old table
        hipError_t e = hipMemcpy(b->d_slots, tab, sizeof(BatchSlot) * (size_t)b->n, hipMemcpyHostToDevice);
        if (e != hipSuccess) { batch_err(b, "slot table upload failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    }
    BuildBuffers bb;
    choose_build(b->ctxs, b->n, bb);
    bb.d_slots = b->d_slots;
    bb.nbatch = b->n;
    if (bb.reg && reg_build_init() != hipSuccess) { (void)hipGetLastError(); bb.reg = 0; }
    // a caller that leaves CUs to the builds (fd_batch_set_eval_cus below the device's count) runs them BESIDE evaluation launches:
    // one workgroup per model then stays on those CUs; the front end's short wide launches would queue for CUs the evaluation holds
    bb.reg_front = (b->eval_cus <= 0 || b->eval_cus >= (int)device_cus()) ? 1 : 0;
    bb.group_panels = b->n >= 4 ? 1 : 0;

    // every context reads its rest rig in place from ONE array, in this one launch sequence: their centres are equal by construction
    bool same_rest_launch = b->have_src;
    for (int i = 1; i < b->n && same_rest_launch; ++i) same_rest_launch = b->src.rest[i] == b->src.rest[0];
    // A shot of multilayer models (fd_batch_set_shared_factor): one factorisation per LAYER for the group, every frame's
    // right-hand sides through them in one launch (launch_build_ml_shared).  Anything it does not take -- other rest arrays,
    // one context, more than 1024 points, no scratch -- builds every model on its own as ever.
    bool shared_ml = b->shared_factor != 0 && bb.ml_layers > 0 && same_rest_launch && ml_shared_applies(bb.M, bb.ml_layers, b->n);
    if (shared_ml && ml_shared_init() != hipSuccess) { (void)hipGetLastError(); shared_ml = false; }
    // (a scratch that grows: hipFree drains the device, nobody reads the old one)
    if (shared_ml && b->d_mlfac.grow(ml_shared_scratch_bytes(bb)) != hipSuccess) { (void)hipGetLastError(); shared_ml = false; }
    // A shot of QNN models (fd_batch_set_shared_lu): radii per frame, then reflectors, kernel block and its LU without pivot
    // search once for the group, every frame's right-hand sides through that factor in one launch (launch_build_qnn_shared).
    // Anything it does not take -- other rest arrays, too few contexts, a context that fell back to the pivoted LU, fewer points
    // than polynomial columns, no scratch -- builds every model on its own as ever.
    bool shared_qnn = b->shared_lu != 0 && c0->kind == FD_KERNEL_GAUSSIAN_QNN && bb.ml_layers == 0 && bb.nopivot && !bb.spd &&
                      bb.npad <= 1024 && bb.M >= bb.T && same_rest_launch && qnn_shared_applies(bb.M, b->n);
    for (int i = 0; i < b->n && shared_qnn; ++i) shared_qnn = b->ctxs[i]->solver == FD_SOLVER_AUTO;
    if (shared_qnn && qnn_shared_init() != hipSuccess) { (void)hipGetLastError(); shared_qnn = false; }
    if (shared_qnn && qnn_shared_scratch_bytes(bb) > b->d_qnnfac.cap) {
        b->qnn_slot_ready = false;                          // (the slot goes with the old scratch; hipFree drains the device)
        if (b->d_qnnfac.grow(qnn_shared_scratch_bytes(bb)) != hipSuccess) { (void)hipGetLastError(); shared_qnn = false; }
    }

    const GraphKey key = graph_key(c0, (bb.spd << 9) | (bb.small << 10) | (bb.reg << 11) | (bb.nopivot << 12), false);
    if (!bb.reg && !shared_ml && !shared_qnn && b->use_graph &&
        ensure_graph(stream, &b->exec, &b->key, key, [&] { return launch_build(bb, stream, nullptr); }) != hipSuccess)
        b->use_graph = false;
#define FD_BHIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) { batch_err(b, "%s failed: %s", #call, hipGetErrorString(e_)); return FD_E_DEVICE; } \
    } while (0)
    // One factorisation for the group (fd_batch_set_shared_factor): the register-resident build applies and every context reads
    // its rest rig, in place, from the SAME device array (fd_batch_set_points_dev with one rest pointer); anything else builds
    // every model on its own as ever.
    const bool shared_fac_ok = same_rest_launch;
    bool shared_fac = b->shared_factor != 0 && bb.reg && shared_fac_ok && b->n > 1;
    if (shared_fac && !b->d_fac && b->d_fac.alloc(reg_factor_doubles()) != hipSuccess) {
        (void)hipGetLastError(); shared_fac = false;
    }
    b->last_shared_factor = (shared_fac || shared_ml || shared_qnn) ? 1 : 0;
    if (!b->lean) FD_BHIP(hipEventRecord(b->ev0, stream));      // (lean: the group's first packet is its first kernel; the reports carry no phase times)
    if (shared_fac) {
        FD_BHIP(launch_build_reg_shared(bb, stream, &b->src, nullptr, b->d_fac));
        b->have_src = false;
    } else if (bb.reg) {
        // one launch, one workgroup per model, control table included
        FD_BHIP(launch_build_reg(bb, stream, b->have_src ? &b->src : nullptr, nullptr));      // (no phases to split: the report's assembly time is 0)
        b->have_src = false;
    } else {
    // the control points are kernel arguments (they change every call), so k_prepare stays
    // outside the captured graph
    FD_BHIP(launch_prepare(bb, stream, b->have_src ? &b->src : nullptr));
    b->have_src = false;
    if (shared_ml) {
        // plain launches, outside the captured graph (which is the per-context chain's)
        FD_BHIP(hipEventRecord(b->ev_mid, stream));
        FD_BHIP(launch_build_ml_shared(bb, stream, b->d_mlfac));
    } else if (shared_qnn) {
        FD_BHIP(hipEventRecord(b->ev_mid, stream));
        // plain launches, outside the captured graph (measured: replaying them from a graph of their own changes nothing)
        const bool fill = !(b->qnn_slot_ready && b->qnn_slot_M == bb.M && b->qnn_slot_npad == bb.npad);
        b->qnn_slot_ready = false;
        FD_BHIP(launch_build_qnn_shared(bb, stream, b->d_qnnfac, fill));
        b->qnn_slot_ready = true; b->qnn_slot_M = bb.M; b->qnn_slot_npad = bb.npad;
    } else if (b->use_graph && b->exec) {
        FD_BHIP(hipEventRecord(b->ev_mid, stream));
        FD_BHIP(hipGraphLaunch(b->exec, stream));
    } else {
        FD_BHIP(launch_build(bb, stream, b->ev_mid));
    }
    }
    if (!b->lean) FD_BHIP(hipEventRecord(b->ev1, stream));      // (lean: fd_batch_cook_group records it behind the evaluation)
    b->waited_stream = nullptr;
#undef FD_BHIP
    static std::atomic<uint64_t> build_ids{0};
    const uint64_t this_build = same_rest_launch ? ++build_ids : 0;
    // (lean: the reports carry no phase times; the register-resident build has no phases to split)
    hipEvent_t t0 = b->lean ? nullptr : b->ev0, t_mid = b->lean ? nullptr : (bb.reg ? b->ev0 : b->ev_mid), t1 = b->lean ? nullptr : b->ev1;
    for (int i = 0; i < b->n; ++i) note_build_enqueued(b->ctxs[i], b->ev1, stream, b, t0, t_mid, t1, &bb, this_build);
    if (shared_qnn)      // the factor stays in the batch's scratch: nothing of it in the contexts for fd_set_deltas
        for (int i = 0; i < b->n; ++i) b->ctxs[i]->have_factor = false;
    arm_status(b->ctxs, b->n, stream, bb.reg != 0, b->ev1, b->status_ev);
    return FD_OK;
}

// the statuses a batched build posted: one event query while they are in flight, then every context on its own
static int batch_poll(fd_batch *b)
{
    if (b->h_mismatch && *b->h_mismatch != 0) {
        batch_err(b, "shared-rig evaluation: context %d was built on other rest points than context 0 (same address, other "
                     "contents); its frame was passed through", *b->h_mismatch - 1);
        return FD_E_INVALID;
    }
    bool any = false;
    for (int i = 0; i < b->n; ++i) any = any || b->ctxs[i]->status_inflight || b->ctxs[i]->sticky_rc != FD_OK;
    if (!any) return FD_OK;
    bool shared_pending = false;
    hipEvent_t shared_ev = nullptr;
    for (int i = 0; i < b->n; ++i)
        if (b->ctxs[i]->status_inflight && (b->ctxs[i]->status_poll == b->status_ev || b->ctxs[i]->status_poll == b->ev1)) {
            shared_pending = true; shared_ev = b->ctxs[i]->status_poll;
        }
    if (shared_pending) {
        const hipError_t q = hipEventQuery(shared_ev);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return FD_OK; }
    }
    for (int i = 0; i < b->n; ++i) {
        const bool lu_before = b->ctxs[i]->prefer_lu;
        const int rc = poll_status(b->ctxs[i]);
        if (b->ctxs[i]->prefer_lu != lu_before) b->prepared = false;     // a model was rebuilt: a set packed from the old one is stale
        if (rc) { batch_err(b, "context %d: %s", i, b->ctxs[i]->err); return rc; }
    }
    return FD_OK;
}

int fd_batch_build_result(fd_batch *b, fd_report *reports)
{
    if (!b) return FD_E_INVALID;
    int first = FD_OK;
    for (int i = 0; i < b->n; ++i) {
        const int rc = fd_build_result(b->ctxs[i], reports ? &reports[i] : nullptr);
        if (rc && !first) { first = rc; batch_err(b, "context %d: %s", i, b->ctxs[i]->err); }
    }
    return first;
}

// The map deltas -> weights of ctx's rest rig, column by column: helper contexts with ctx's kernel, parameters, term and solver
// read ctx's own copy of the rest points in place and are built in batches on unit deltas -- build k has 1 in x of point 3k, in
// y of point 3k + 1 and in z of point 3k + 2, so its weight columns are columns 3k, 3k + 1, 3k + 2 of S.  Nothing of ctx changes.
int fd_solve_operator(fd_ctx *ctx, double *S)
{
    if (!ctx || !S) return FD_E_INVALID;
    if (!ctx->points_set) { set_err(ctx, "fd_solve_operator: no control points (call fd_set_points first)"); return FD_E_NOT_BUILT; }
    int rc = use_device(ctx);
    if (rc) return rc;
    FD_HIP(ctx, hipStreamSynchronize(cur_stream(ctx)));             // d_rest may still be on its way (fd_set_points_dev)
    const int M = ctx->M, rows = model_centres(ctx) + 4;
    const int builds = (M + 2) / 3;
    const int nh = builds < kMaxBatch ? builds : kMaxBatch;
    fd_ctx *helpers[kMaxBatch] = {};
    DevBuf<float> d_unit;
    fd_batch *batch = nullptr;
    auto done = [&](int code) {
        if (batch) fd_batch_destroy(batch);
        for (fd_ctx *h : helpers) if (h) fd_destroy(h);
        d_unit.reset();
        return code;
    };
    fd_config cfg{};
    cfg.struct_size = (int)sizeof(cfg);
    cfg.device = ctx->device; cfg.eval_precision = ctx->eval_precision; cfg.solver = ctx->solver;
    for (int i = 0; i < nh; ++i) {
        fd_ctx *h = helpers[i] = fd_create(&cfg);
        if (!h) { set_err(ctx, "fd_solve_operator: %s", g_err); return done(FD_E_NOMEM); }
        if ((rc = fd_set_kernel(h, ctx->kind, ctx->params, ctx->nparams)) || (rc = fd_set_term(h, ctx->term))) {
            set_err(ctx, "fd_solve_operator: %s", h->err);
            return done(rc);
        }
        h->prefer_lu = ctx->prefer_lu;      // a rig that has asked for the pivoted LU asks for it under any deltas
        h->stream_ = cur_stream(ctx);       // one stream for all: no hardware queue per helper
    }
    const size_t per = (size_t)M * 3;
    if (d_unit.alloc(per * (size_t)nh) != hipSuccess) {
        (void)hipGetLastError();
        set_err(ctx, "fd_solve_operator: hipMalloc(%zu bytes) failed", sizeof(float) * per * (size_t)nh);
        return done(FD_E_NOMEM);
    }
    std::vector<float> unit(per * (size_t)nh);
    std::vector<double> W((size_t)rows * 3);
    for (int k0 = 0; k0 < builds; k0 += nh) {
        const int n = builds - k0 < nh ? builds - k0 : nh;
        std::fill(unit.begin(), unit.end(), 0.f);
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) {
                const int col = 3 * (k0 + i) + a;
                if (col < M) unit[per * (size_t)i + 3 * (size_t)col + a] = 1.f;
            }
        if (hipMemcpy(d_unit, unit.data(), sizeof(float) * per * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
            set_err(ctx, "fd_solve_operator: upload of the unit deltas failed: %s", hipGetErrorString(hipGetLastError()));
            return done(FD_E_DEVICE);
        }
        if (!(batch = fd_batch_create(helpers, n))) { set_err(ctx, "fd_solve_operator: %s", g_err); return done(FD_E_NOMEM); }
        const float *rest[kMaxBatch], *delta[kMaxBatch];
        for (int i = 0; i < n; ++i) { rest[i] = ctx->d_rest; delta[i] = d_unit + per * (size_t)i; }
        if ((rc = fd_batch_set_points_dev(batch, rest, delta, M)) || (rc = fd_batch_build_async(batch, nullptr)) ||
            (rc = fd_batch_build_result(batch, nullptr))) {
            set_err(ctx, "fd_solve_operator: %s", batch->err);
            return done(rc);
        }
        for (int i = 0; i < n; ++i) {
            if ((rc = fd_get_weights(helpers[i], W.data(), nullptr))) { set_err(ctx, "fd_solve_operator: %s", helpers[i]->err); return done(rc); }
            for (int a = 0; a < 3; ++a) {
                const int col = 3 * (k0 + i) + a;
                if (col >= M) continue;
                for (int r = 0; r < rows; ++r) S[(size_t)r * M + col] = W[3 * (size_t)r + a];
            }
        }
        fd_batch_destroy(batch);
        batch = nullptr;
    }
    return done(FD_OK);
}

// ---- fd_fit_deltas, fd_fit_deltas_shot: the host composition on top of the Gram operator, the adjoint and the solve operator;
// its dense algebra is fd_fit_host.h's ----
static double fit_ms_since(const std::chrono::steady_clock::time_point &t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int fit_checks(fd_ctx *ctx, const char *who, int64_t N, const float *P_in, const float *T, double mu, const float *tu,
                      const float *tv, const float *nrm, const double *delta_out, const fd_fit_report *reports, int F)
{
    if (!T || !delta_out || N < 0 || (N > 0 && !P_in)) { set_err(ctx, "%s: bad N / P / T / delta_out pointers", who); return FD_E_INVALID; }
    if (!(mu >= 0.0) || !(mu < INFINITY)) { set_err(ctx, "%s: mu must be finite and >= 0", who); return FD_E_INVALID; }
    for (int f = 0; reports && f < F; ++f) {
        if (reports[f].struct_size < (int)sizeof(fd_fit_report)) {
            set_err(ctx, "%s: report->struct_size is %d, must be sizeof(fd_fit_report) = %d", who, reports[f].struct_size,
                    (int)sizeof(fd_fit_report));
            return FD_E_INVALID;
        }
    }
    if (!frames_ok(tu, tv, nrm)) { set_err(ctx, "%s: tu, tv, nrm must be all set or all NULL", who); return FD_E_INVALID; }
    const int M = ctx->M, n = model_centres(ctx) + 4, order = tu ? 3 * M : M;
    if (n > FD_FIT_MAX_ROWS || order > FD_FIT_MAX_ORDER) {
        set_err(ctx, "%s: C + 4 = %d (at most %d) or the order of the normal system %d (at most %d) is beyond the host composition",
                who, n, FD_FIT_MAX_ROWS, order, FD_FIT_MAX_ORDER);
        return FD_E_INVALID;
    }
    if (!ctx->built && !ctx->build_pending) { set_err(ctx, "%s: no successfully built model", who); return FD_E_NOT_BUILT; }
    return FD_OK;
}

static int fit_singular(fd_ctx *ctx, const char *who, double pmin)
{
    set_err(ctx, "%s: the normal matrix is not positive definite (pivot %.3e): control points that no live vertex "
                 "constrains need mu > 0", who, pmin);
    return FD_E_SINGULAR;
}

// fd_fit_deltas (shot = false, F = 1) and fd_fit_deltas_shot: the fit of F targets T (F x N x 3) over one mesh, omega and mu;
// delta0 and delta_out are F x M x 3, reports F structs.  One Gram launch, one normal matrix and one factor serve all frames.  The
// two calls differ in the first-order stage alone: the adjoint's launch there, the shot adjoint's here, even for one frame.
static int fit_frames(fd_ctx *ctx, const char *who, bool shot, const Mesh &m, int F, const float *T, const float *omega, double mu,
                      const float *delta0, const double *S, double *delta_out, fd_fit_report *reports)
{
    int rc;
    if ((rc = fit_checks(ctx, who, m.N, m.P, T, mu, m.tu, m.tv, m.nrm, delta_out, reports, F))) return rc;
    FitSystem sys;
    sys.M = ctx->M; sys.n = model_centres(ctx) + 4; sys.proj = m.tu != nullptr;
    sys.nq = sys.proj ? 6 : 1; sys.order = sys.proj ? 3 * sys.M : sys.M; sys.mu = mu;
    const int M = sys.M, n = sys.n;
    std::vector<double> S_own;
    if (!S) {
        S_own.resize((size_t)n * M);
        if ((rc = fd_solve_operator(ctx, S_own.data()))) return rc;
        S = S_own.data();
    }
    sys.S = S;
    // ---- the second-order term, once; the mesh stays staged for the shot adjoint
    auto t0 = std::chrono::steady_clock::now();
    std::vector<double> H((size_t)sys.nq * n * n);
    Mesh d;
    if ((rc = stage_mesh(ctx, m, cur_stream(ctx), &d, Upload{&ctx->d_fall.p, omega, 1}))) return rc;
    if ((rc = gram_staged(ctx, who, d, omega ? ctx->d_fall : nullptr, H.data()))) return rc;
    const double ms_gram = fit_ms_since(t0);
    // ---- the first-order terms: the adjoint of g_f = omega (T_f - P)
    t0 = std::chrono::steady_clock::now();
    const size_t frame = (size_t)m.N * 3, cblock = (size_t)n * 3, dblock = (size_t)M * 3;
    std::vector<double> tt((size_t)F), c((size_t)F * cblock);
    if (!shot) {
        std::vector<float> g(frame);
        tt[0] = fit_cotangent(m.N, m.P, T, omega, g.data());
        if ((rc = adjoint_host(ctx, who, m, g.data(), c.data()))) return rc;
    } else {
        // one group of frames at a time, its cotangents on the host in a buffer the context keeps: fresh pages for 32 frames of
        // a large mesh cost more than everything else in this stage
        const size_t gneed = (size_t)(F < FD_MAX_BATCH ? F : FD_MAX_BATCH) * frame + 1;
        if (gneed > ctx->cap_hgshot) {
            free(ctx->h_gshot);
            ctx->cap_hgshot = 0;
            ctx->h_gshot = (float *)malloc(gneed * sizeof(float));
            if (!ctx->h_gshot) { set_err(ctx, "%s: malloc(%zu bytes) failed", who, gneed * sizeof(float)); return FD_E_NOMEM; }
            ctx->cap_hgshot = gneed;
        }
        float *const g = ctx->h_gshot;
        for (int f0 = 0; f0 < F; f0 += FD_MAX_BATCH) {
            const int nF = F - f0 < FD_MAX_BATCH ? F - f0 : FD_MAX_BATCH;
            for (int f = 0; f < nF; ++f) tt[f0 + f] = fit_cotangent(m.N, m.P, T + (size_t)(f0 + f) * frame, omega, g + (size_t)f * frame);
            if ((rc = adjoint_shot_staged(ctx, who, d, nF, g, c.data() + (size_t)f0 * cblock))) return rc;
        }
    }
    const double ms_adjoint = fit_ms_since(t0);
    // ---- the normal system, once, and every frame's right-hand side
    t0 = std::chrono::steady_clock::now();
    fit_compose_G(sys, H.data());
    std::vector<std::vector<double>> b((size_t)F), Stc((size_t)F);
    std::vector<double> E0((size_t)F);
    for (int f = 0; f < F; ++f) {
        const float *d0 = delta0 ? delta0 + (size_t)f * dblock : nullptr;
        fit_rhs(sys, c.data() + (size_t)f * cblock, d0, b[f], Stc[f]);
        E0[f] = fit_energy_at_delta0(sys, Stc[f], tt[f], d0);
    }
    fit_compose_A(sys);
    const double ms_compose = fit_ms_since(t0);
    // ---- one factorisation, F solves
    t0 = std::chrono::steady_clock::now();
    const bool ok = fit_factor(sys);
    if (ok) for (int f = 0; f < F; ++f) fit_solve(sys, b[f].data());
    const double ms_solve = fit_ms_since(t0);
    for (int f = 0; reports && f < F; ++f) {
        fd_fit_report *report = reports + f;
        const float *d0 = delta0 ? delta0 + (size_t)f * dblock : nullptr;
        report->order = sys.order;
        report->E0 = E0[f];
        report->E_fit = ok ? fit_energy(sys, Stc[f], tt[f], d0, b[f].data()) : E0[f];
        report->pivot_min = sys.order > 0 ? sys.pmin : 0.0;
        report->pivot_max = sys.pmax;
        report->ms_gram = ms_gram; report->ms_adjoint = ms_adjoint; report->ms_compose = ms_compose; report->ms_solve = ms_solve;
    }
    if (!ok) return fit_singular(ctx, who, sys.pmin);
    for (int f = 0; f < F; ++f)
        for (size_t i = 0; i < dblock; ++i) delta_out[(size_t)f * dblock + i] = b[f][i];
    return FD_OK;
}

int fd_fit_deltas(fd_ctx *ctx, int64_t N, const float *P_in, const float *T, const float *omega, const float *dist2, const float *tu,
                  const float *tv, const float *nrm, float radius2, float falloffrate, double mu, const float *delta0,
                  const double *S, double *delta_out, fd_fit_report *report)
{
    if (!ctx) return FD_E_INVALID;
    return fit_frames(ctx, "fd_fit_deltas", false, Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, 1, T, omega, mu, delta0, S,
                      delta_out, report);
}

int fd_fit_deltas_shot(fd_ctx *ctx, int64_t N, int F, const float *P_in, const float *T, const float *omega, const float *dist2,
                       const float *tu, const float *tv, const float *nrm, float radius2, float falloffrate, double mu,
                       const float *delta0, const double *S, double *delta_out, fd_fit_report *reports)
{
    if (!ctx) return FD_E_INVALID;
    if (F < 1) { set_err(ctx, "fd_fit_deltas_shot: F < 1"); return FD_E_INVALID; }
    return fit_frames(ctx, "fd_fit_deltas_shot", true, Mesh{N, P_in, dist2, tu, tv, nrm, radius2, falloffrate}, F, T, omega, mu, delta0, S,
                      delta_out, reports);
}

// One launch evaluates every context of the batch on its own vertex arrays (grid y = context)
// when they all take the default thin-plate kernel on equally sized inputs; otherwise the
// single launches are enqueued one after the other.  Results are those of fd_deform_dev_stream
// per context, bit for bit.
int fd_batch_deform_dev(fd_batch *b, void *hip_stream, int64_t N, const float *const *d_P_in, float *const *d_P_out,
                        const float *const *d_dist2, float *const *d_falloff_out, const float *const *d_tu,
                        const float *const *d_tv, const float *const *d_nrm, float radius2, float falloffrate)
{
    if (!b || !d_P_in || !d_P_out) return FD_E_INVALID;
    if (N < 0) { batch_err(b, "fd_batch_deform_dev: N < 0"); return FD_E_INVALID; }
    if (!frames_ok(d_tu, d_tv, d_nrm)) { batch_err(b, "fd_batch_deform_dev: tu, tv, nrm tables must be all set or all NULL"); return FD_E_INVALID; }
    if (N == 0) return FD_OK;
    fd_ctx *c0 = b->ctxs[0];
    int rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    DeformArgs args[kMaxBatch];
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        if (!d_P_in[i] || !d_P_out[i]) { batch_err(b, "fd_batch_deform_dev: NULL vertex array for context %d", i); return FD_E_INVALID; }
        if (!c->built && !c->build_pending) { batch_err(b, "fd_batch_deform_dev: context %d has no built model", i); return FD_E_NOT_BUILT; }
        const float *tu = d_tu ? d_tu[i] : nullptr, *tv = d_tv ? d_tv[i] : nullptr, *nr = d_nrm ? d_nrm[i] : nullptr;
        if (!frames_ok(tu, tv, nr)) { batch_err(b, "fd_batch_deform_dev: context %d: tu, tv, nrm must be all set or all NULL", i); return FD_E_INVALID; }
        args[i] = deform_args(c, Mesh{N, d_P_in[i], d_dist2 ? d_dist2[i] : nullptr, tu, tv, nr, radius2, falloffrate}, d_P_out[i],
                              d_falloff_out ? d_falloff_out[i] : nullptr);
        if (c->output != c0->output) { batch_err(b, "fd_batch_deform_dev: context %d has another fd_set_output setting than context 0", i); return FD_E_INVALID; }
    }
    // statuses first: a model the poll had to rebuild (on its context's stream) is then ordered like any other build
    if ((rc = batch_poll(b))) return rc;
    for (int i = 0; i < b->n; ++i)
        if ((rc = order_after_batch(b->ctxs[i], stream))) { batch_err(b, "context %d: %s", i, b->ctxs[i]->err); return rc; }
    hipError_t e = launch_deform_batch(args, b->n, stream);
    if (e != hipSuccess) { batch_err(b, "launch_deform_batch failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    return FD_OK;
}

// Frames of ONE mesh and ONE rest rig: phi(|x - c|^2) is formed once per (vertex, centre) for all of
// them and the weight contraction runs on the matrix pipe (fd_eval.hip, k_deform32_tps_shared).
// ---- frames of one mesh and one rest rig (fd_batch_deform_shared_dev, fd_batch_prepare_shared) ----
// 1: the shared-rig launch applies; 0: the per-frame launches do; < 0: error
static int shared_applies(fd_batch *b, const char *who, float *const *d_P_out, int *ek_out)
{
    fd_ctx *c0 = b->ctxs[0];
    const int ek = eval_kind(c0);
    *ek_out = ek;
    bool fast = (ek == FD_KERNEL_THIN_PLATE || ek == FD_KERNEL_GAUSSIAN || ek == FD_KERNEL_GAUSSIAN_QNN) && round_up(c0->M, kRecPad) >= 32;
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        if (!d_P_out[i]) { batch_err(b, "%s: NULL output array for context %d", who, i); return FD_E_INVALID; }
        if (!c->built && !c->build_pending) { batch_err(b, "%s: context %d has no built model", who, i); return FD_E_NOT_BUILT; }
        // one rest rig: every context read its rest points in place from the SAME device array
        if (!c->rest_src || c->rest_src != c0->rest_src || !same_model(c, c0)) {
            batch_err(b, "%s: the contexts must share one rest rig (fd_batch_set_points_dev with the "
                         "same rest array for all), kernel and term; context %d does not", who, i);
            return FD_E_INVALID;
        }
        if (c->output != c0->output) { batch_err(b, "%s: context %d has another fd_set_output setting than context 0", who, i); return FD_E_INVALID; }
        if (c->eval_precision != FD_EVAL_FP32 || c->eval_variant > 0 || record_layers(c) != 0) fast = false;
    }
    return fast ? 1 : 0;
}

// ---- what the eight shot calls share on the host: argument checks, the ShotScratch protocol, the per-context vector launches
// (fill_mesh and fill_vector_tables, being templates, are in front of this linkage block) ----
static int shot_check_mesh(fd_batch *b, const char *who, int64_t N, const float *d_P_in, const float *d_tu, const float *d_tv,
                           const float *d_nrm)
{
    if (N < 0 || (N > 0 && !d_P_in)) { batch_err(b, "%s: bad N / P_in", who); return FD_E_INVALID; }
    if (!frames_ok(d_tu, d_tv, d_nrm)) { batch_err(b, "%s: tu, tv, nrm must be all set or all NULL", who); return FD_E_INVALID; }
    return FD_OK;
}

// aliasing of a position call, before any device work: one input serves every frame, so no output may be a shared input --
// except the one frame of a batch of one written in place over the mesh, as in fd_deform_dev
static int shot_check_aliasing(fd_batch *b, const char *who, const float *d_P_in, float *const *d_P_out, const float *d_dist2,
                               float *const *d_falloff_out, const float *d_tu, const float *d_tv, const float *d_nrm)
{
    const void *ins[5] = {d_P_in, d_dist2, d_tu, d_tv, d_nrm};
    for (int i = 0; i < b->n; ++i) {
        if (!d_P_out[i]) { batch_err(b, "%s: NULL output array for context %d", who, i); return FD_E_INVALID; }
        const void *outs[2] = {d_P_out[i], d_falloff_out ? d_falloff_out[i] : nullptr};
        for (int o = 0; o < 2; ++o)
            for (int k = 0; k < 5; ++k) {
                if (!outs[o] || outs[o] != ins[k]) continue;
                if (b->n == 1 && o == 0 && k == 0) continue;
                batch_err(b, "%s: an output of context %d is a shared input array", who, i);
                return FD_E_INVALID;
            }
    }
    return FD_OK;
}

// The argument block of a vector call.  *want: vectors or a Jacobian are asked for; where they are not, nothing but the struct's
// size has been looked at and the call is its position call's.
static int shot_check_vectors(fd_batch *b, const char *who, int64_t N, const float *d_P_in, float *const *d_P_out, const float *d_dist2,
                              float *const *d_falloff_out, const float *d_tu, const float *d_tv, const float *d_nrm,
                              const fd_batch_vectors *vec, bool *want)
{
    *want = false;
    if (vec && vec->struct_size < (int)sizeof(fd_batch_vectors)) {
        batch_err(b, "%s: vec->struct_size is %d, must be sizeof(fd_batch_vectors) = %d", who, vec->struct_size, (int)sizeof(fd_batch_vectors));
        return FD_E_INVALID;
    }
    *want = vec && (vec->N || vec->N_out || vec->tu || vec->tu_out || vec->tv || vec->tv_out || vec->jacobian);
    if (!*want) return FD_OK;
    if ((!vec->N != !vec->N_out) || (!vec->tu != !vec->tu_out) || (!vec->tv != !vec->tv_out)) {
        batch_err(b, "%s: every vector needs its input and its output table (both or neither)", who);
        return FD_E_INVALID;
    }
    if (int rc = shot_check_mesh(b, who, N, d_P_in, d_tu, d_tv, d_nrm)) return rc;
    // tables of n non-NULL entries, none of which is a shared input -- a batch of one included: the vector launch reads d_P_in
    // after the position launch has written
    const void *ins[8] = {d_P_in, d_dist2, d_tu, d_tv, d_nrm, vec->N, vec->tu, vec->tv};
    float *const *tabs[6] = {d_P_out, d_falloff_out, vec->N_out, vec->tu_out, vec->tv_out, vec->jacobian};
    for (int t = 0; t < 6; ++t) {
        if (!tabs[t]) continue;
        for (int i = 0; i < b->n; ++i) {
            const void *o = tabs[t][i];
            if (!o) { batch_err(b, "%s: output table %d has a NULL entry for context %d", who, t, i); return FD_E_INVALID; }
            for (const void *in : ins)
                if (in && o == in) { batch_err(b, "%s: an output of context %d is a shared input array", who, i); return FD_E_INVALID; }
        }
    }
    return FD_OK;
}

// before a call with a scratch of its own reads the contexts' models: their statuses, `stream` behind their builds, and the
// event the call's reads will end at
static int shot_begin(fd_batch *b, const char *who, ShotScratch &sc, hipStream_t stream)
{
    int rc;
    if (!b->lean && (rc = batch_poll(b))) return rc;           // before the ordering: a repaired model's rebuild is ordered with the rest
    for (int i = 0; i < b->n; ++i)
        if ((rc = order_after_batch(b->ctxs[i], stream))) { batch_err(b, "context %d: %s", i, b->ctxs[i]->err); return rc; }
    if (!sc.consumed_ev.make()) { batch_err(b, "%s: hipEventCreate failed", who); return FD_E_DEVICE; }
    return FD_OK;
}

// Before the pack kernel about to be enqueued on `stream` rewrites a scratch: the evaluation that last read it (`done` is recorded
// behind it while *pending) must be through with it
static int wait_last_eval(fd_batch *b, const char *who, hipStream_t stream, bool *pending, hipEvent_t done)
{
    if (*pending && done && hipStreamWaitEvent(stream, done, 0) != hipSuccess) {
        batch_err(b, "%s: hipStreamWaitEvent failed: %s", who, hipGetErrorString(hipGetLastError()));
        return FD_E_DEVICE;
    }
    *pending = false;
    return FD_OK;
}

// Behind an evaluation on `stream` that read a scratch: `ev` recorded there, for wait_last_eval.  False: there is no event to order
// the next pack kernel by, and the stream has been waited for instead
static bool record_eval(Event &ev, hipStream_t stream)
{
    if (ev.make() && hipEventRecord(ev, stream) == hipSuccess) return true;
    (void)hipGetLastError();
    (void)hipStreamSynchronize(stream);
    return false;
}

// `bytes` of scratch for the pack kernel about to be enqueued on `stream`
static int shot_reserve(fd_batch *b, const char *who, ShotScratch &sc, size_t bytes, hipStream_t stream)
{
    if (bytes > sc.d.cap) {
        // (hipFree drains the device: no launch still reads the old scratch)
        sc.eval_pending = false;
        if (sc.d.grow(bytes) != hipSuccess) {
            (void)hipGetLastError();
            batch_err(b, "%s: scratch allocation (%zu bytes) failed", who, bytes);
            return FD_E_NOMEM;
        }
    }
    return wait_last_eval(b, who, stream, &sc.eval_pending, sc.eval_ev);
}

// behind the position launch (pack kernel and evaluation; the launch itself records sc.consumed_ev behind the pack kernel)
static void shot_evaluated(ShotScratch &sc, hipStream_t stream)
{
    sc.consumed = true;
    sc.eval_pending = record_eval(sc.eval_ev, stream);
}

// behind the vector launch on the same scratch
static void shot_vectors_evaluated(ShotScratch &sc, hipStream_t stream)
{
    // the next pack kernel rewrites the scratch this launch reads: its event moves behind the vector launch
    if (sc.eval_pending && hipEventRecord(sc.eval_ev, stream) == hipSuccess) return;
    (void)hipGetLastError();
    (void)hipStreamSynchronize(stream);
}

// ONE batched build read every context's rest rig from one array: their centres are equal by construction
static bool one_build(const fd_batch *b)
{
    const uint64_t id = b->ctxs[0]->rig_build_id;
    if (id == 0) return false;
    for (int i = 1; i < b->n; ++i)
        if (b->ctxs[i]->rig_build_id != id) return false;
    return true;
}

// per context, what fd_deform_vectors_dev launches for a context of `precision` on the shared arrays; these launches read the
// models to their end, and `consumed_ev` is recorded behind them
static int vectors_per_context(fd_batch *b, hipStream_t stream, int precision, hipEvent_t consumed_ev, int64_t N, const float *d_P_in,
                               float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out, const float *d_tu,
                               const float *d_tv, const float *d_nrm, float radius2, float falloffrate, const fd_batch_vectors *vec)
{
    for (int i = 0; i < b->n; ++i) {
        DeformArgs a = deform_args(b->ctxs[i], Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_P_out[i],
                                   d_falloff_out ? d_falloff_out[i] : nullptr);
        a.precision = precision;
        const VectorArgs v{vec->N, vec->tu, vec->tv, vec->N ? vec->N_out[i] : nullptr, vec->tu ? vec->tu_out[i] : nullptr,
                           vec->tv ? vec->tv_out[i] : nullptr, vec->jacobian ? vec->jacobian[i] : nullptr};
        hipError_t e = launch_vectors(a, v, stream);
        if (e != hipSuccess) { batch_err(b, "launch_vectors failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    }
    if (hipEventRecord(consumed_ev, stream) != hipSuccess) { (void)hipGetLastError(); return FD_E_DEVICE; }
    return FD_OK;
}

// the pack kernel of the contexts' current models into the set NOT read by the evaluation before; on `stream`
static int shared_pack(fd_batch *b, hipStream_t stream, int ek, float *const *d_P_out, float *const *d_falloff_out)
{
    fd_ctx *c0 = b->ctxs[0];
    const int si = b->packed_valid ? (b->cur_set ^ 1) : 0;
    fd_batch::SharedSet &st = b->sets[si];
    SharedDeformArgs a{};
    a.N = 1; a.Mpad = round_up(c0->M, kRecPad); a.nF = b->n; a.kind = ek; a.ctiles = c0->d_tiles16;
    a.falloff_out = d_falloff_out;
    int rc;
    // (lean: the build's event is recorded behind the evaluation -- a query now would see the PREVIOUS build's completion; the
    //  status arrives with the next call, and an evaluation of an unbuilt model passes its frame through: header)
    if (!b->lean && (rc = batch_poll(b))) return rc;           // before the ordering: a repaired model's rebuild is ordered with the rest
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        a.rec32[i] = c->d_rec32; a.model[i] = c->d_model; a.P_out[i] = d_P_out[i]; a.centres[i] = c->d_centres;
        if ((rc = order_after_batch(c, stream))) { batch_err(b, "context %d: %s", i, c->err); return rc; }
    }
    // "one rest rig" by content is what the pack kernel checks (an address does not identify contents); contexts that ONE batched
    // build read from one array are equal by construction, and the comparison -- the pack kernel's longest chain -- is skipped
    if (one_build(b)) for (int i = 1; i < b->n; ++i) a.centres[i] = a.centres[0];
    const SharedPlan pl = shared_plan(a.Mpad, a.nF, a.kind);
    const size_t wb = pl.wtile_bytes, fb = pl.frame_bytes;
    if (wb > st.d_wtiles.cap || fb > st.d_frames.cap) {
        // the two go together (hipFree drains the device: no launch still reads the old scratch)
        st.d_wtiles.reset(); st.d_frames.reset(); st.eval_pending = false;
        if (st.d_wtiles.grow(wb) != hipSuccess || st.d_frames.grow(fb) != hipSuccess) {
            (void)hipGetLastError();
            batch_err(b, "shared-rig evaluation: scratch allocation (%zu bytes) failed", wb + fb);
            return FD_E_NOMEM;
        }
    }
    if ((rc = wait_last_eval(b, "shared-rig evaluation", stream, &st.eval_pending, st.eval_done))) return rc;
    a.wtiles = st.d_wtiles; a.frames = st.d_frames;
    a.packed_ev = b->lean ? nullptr : (st.packed_ev.make() ? st.packed_ev : nullptr);
    b->consumed_override = nullptr;
    a.mode = 1;
    a.M = c0->M;
    if (b->h_mismatch && hipHostGetDevicePointer((void **)&a.mismatch, b->h_mismatch, 0) != hipSuccess) { (void)hipGetLastError(); a.mismatch = nullptr; }
    hipError_t e = launch_deform_shared(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_deform_shared (pack) failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    b->cur_set = si;
    b->packed_valid = b->lean || st.packed_ev != nullptr;
    b->prepared = true;
    for (int i = 0; i < b->n; ++i) {
        b->prep_P_out[i] = d_P_out[i]; b->prep_fall[i] = d_falloff_out ? d_falloff_out[i] : nullptr;
        b->prep_gen[i] = b->ctxs[i]->model_gen;
    }
    b->prep_has_fall = d_falloff_out != nullptr;
    return FD_OK;
}

int fd_batch_prepare_shared(fd_batch *b, void *hip_stream, float *const *d_P_out, float *const *d_falloff_out)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    fd_ctx *c0 = b->ctxs[0];
    int rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    int ek = 0;
    const int applies = shared_applies(b, "fd_batch_prepare_shared", d_P_out, &ek);
    if (applies < 0) return applies;
    if (applies == 0) return FD_OK;              // the per-frame launches read the models themselves: nothing to prepare
    return shared_pack(b, stream, ek, d_P_out, d_falloff_out);
}

int fd_batch_deform_shared_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, float *const *d_P_out,
                               const float *d_dist2, float *const *d_falloff_out, const float *d_tu,
                               const float *d_tv, const float *d_nrm, float radius2, float falloffrate)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    int rc = shot_check_mesh(b, "fd_batch_deform_shared_dev", N, d_P_in, d_tu, d_tv, d_nrm);
    if (rc) return rc;
    if (N == 0) return FD_OK;
    fd_ctx *c0 = b->ctxs[0];
    rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    int ek = 0;
    const int applies = shared_applies(b, "fd_batch_deform_shared_dev", d_P_out, &ek);
    if (applies < 0) return applies;
    if (applies == 0) {
        // any other kernel / precision: the per-frame launches on the shared arrays (same results as fd_deform_dev)
        const float *pin[kMaxBatch], *pd2[kMaxBatch], *ptu[kMaxBatch], *ptv[kMaxBatch], *pnr[kMaxBatch];
        for (int i = 0; i < b->n; ++i) { pin[i] = d_P_in; pd2[i] = d_dist2; ptu[i] = d_tu; ptv[i] = d_tv; pnr[i] = d_nrm; }
        rc = fd_batch_deform_dev(b, hip_stream, N, pin, d_P_out, d_dist2 ? pd2 : nullptr, d_falloff_out, d_tu ? ptu : nullptr,
                                 d_tu ? ptv : nullptr, d_tu ? pnr : nullptr, radius2, falloffrate);
        // these launches read the models to their end: fd_batch_wait_consumed waits for all of them
        if (rc == FD_OK && b->fallback_ev.make()) {
            if (hipEventRecord(b->fallback_ev, stream) != hipSuccess) { (void)hipGetLastError(); rc = FD_E_DEVICE; }
            b->packed_valid = false;
            b->consumed_override = nullptr;
        }
        return rc;
    }
    // the prepared set, if it was packed from these models for these outputs; else pack now, on this stream
    bool reuse = b->prepared && b->prep_has_fall == (d_falloff_out != nullptr);
    for (int i = 0; reuse && i < b->n; ++i)
        reuse = b->prep_P_out[i] == d_P_out[i] && (!d_falloff_out || b->prep_fall[i] == d_falloff_out[i]) &&
                b->prep_gen[i] == b->ctxs[i]->model_gen;          // a context rebuilt or re-imported on its own since: pack again
    if (reuse) {
        if (!b->lean && (rc = batch_poll(b))) return rc;
        if (!b->prepared) reuse = false;         // the poll repaired a model: pack again (shared_pack orders the stream)
        for (int i = 0; reuse && i < b->n; ++i)
            if ((rc = order_after_batch(b->ctxs[i], stream))) { batch_err(b, "context %d: %s", i, b->ctxs[i]->err); return rc; }
    }
    if (reuse) {
        fd_batch::SharedSet &ps = b->sets[b->cur_set];
        if (!b->lean && ps.packed_ev && hipStreamWaitEvent(stream, ps.packed_ev, 0) != hipSuccess) {
            batch_err(b, "fd_batch_deform_shared_dev: hipStreamWaitEvent failed: %s", hipGetErrorString(hipGetLastError()));
            return FD_E_DEVICE;
        }
    } else if ((rc = shared_pack(b, stream, ek, d_P_out, d_falloff_out))) {
        return rc;
    }
    fd_batch::SharedSet &st = b->sets[b->cur_set];
    SharedDeformArgs a{};
    a.N = N; a.P_in = d_P_in; a.dist2 = d_dist2; a.tu = d_tu; a.tv = d_tv; a.nrm = d_nrm;
    a.radius2 = radius2; a.falloffrate = falloffrate;
    a.Mpad = round_up(c0->M, kRecPad); a.nF = b->n;
    a.ctiles = c0->d_tiles16;
    a.kind = ek;
    a.falloff_out = d_falloff_out;
    for (int i = 0; i < b->n; ++i) { a.rec32[i] = b->ctxs[i]->d_rec32; a.model[i] = b->ctxs[i]->d_model; a.P_out[i] = d_P_out[i]; }
    a.wtiles = st.d_wtiles; a.frames = st.d_frames;
    a.packed_ev = nullptr;
    a.mode = 2;
    a.delta_out = c0->output == FD_OUTPUT_DISPLACEMENT;
    a.max_wgs = b->eval_cus;
    hipError_t e = launch_deform_shared(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_deform_shared failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    if (b->lean) {
        // (one stream for the whole group: fd_batch_cook_group records the batch's ev1 right behind this launch -- that record says
        //  "evaluated" as well as "built"; one trailing packet fewer in front of the caller's wait.  A later re-record of ev1 belongs to
        //  a build that was itself ordered behind this evaluation by fd_batch_wait_consumed: waiting for it still implies this.)
        st.eval_done = b->ev1;
        st.eval_pending = true;
    } else {
        st.eval_pending = record_eval(st.eval_ev, stream);
        st.eval_done = st.eval_ev;
    }
    return FD_OK;
}

// fd_batch_deform_vectors_shared_dev: the position launch as fd_batch_deform_shared_dev runs it, then the vector launch
// (fd_vectors_shared.hip) on the same scratch set; where the shared launch does not apply, fd_deform_vectors_dev's work per context
int fd_batch_deform_vectors_shared_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, float *const *d_P_out,
                                       const float *d_dist2, float *const *d_falloff_out, const float *d_tu, const float *d_tv,
                                       const float *d_nrm, float radius2, float falloffrate, const fd_batch_vectors *vec)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    const char *who = "fd_batch_deform_vectors_shared_dev";
    bool want;
    int rc = shot_check_vectors(b, who, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, vec, &want);
    if (rc) return rc;
    if (!want)
        return fd_batch_deform_shared_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    if (N == 0) return FD_OK;
    fd_ctx *c0 = b->ctxs[0];
    rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    int ek = 0;
    const int applies = shared_applies(b, who, d_P_out, &ek);
    if (applies < 0) return applies;
    if (applies == 0) {
        // any other kernel / precision / size: what fd_deform_vectors_dev runs, per context, on the shared arrays
        for (int i = 0; i < b->n; ++i) {
            fd_ctx *c = b->ctxs[i];
            const fd_vectors v{(int)sizeof(fd_vectors), vec->N, vec->N ? vec->N_out[i] : nullptr, vec->tu, vec->tu ? vec->tu_out[i] : nullptr,
                               vec->tv, vec->tv ? vec->tv_out[i] : nullptr, vec->jacobian ? vec->jacobian[i] : nullptr};
            rc = deform_dev(c, "fd_deform", stream, Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_P_out[i],
                            d_falloff_out ? d_falloff_out[i] : nullptr, &v);
            if (rc) { batch_err(b, "context %d: %s", i, c->err); return rc; }
        }
        // these launches read the models to their end: fd_batch_wait_consumed waits for all of them
        if (b->fallback_ev.make()) {
            if (hipEventRecord(b->fallback_ev, stream) != hipSuccess) { (void)hipGetLastError(); return FD_E_DEVICE; }
            b->packed_valid = false;
            b->consumed_override = nullptr;
        }
        return FD_OK;
    }
    if ((rc = fd_batch_deform_shared_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate)))
        return rc;
    fd_batch::SharedSet &st = b->sets[b->cur_set];
    SharedVectorArgs a{};
    fill_mesh(a, N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate);
    a.Mpad = round_up(c0->M, kRecPad); a.nF = b->n; a.kind = ek;
    fill_vector_tables(a, b->n, vec);
    a.wtiles = st.d_wtiles; a.frames = st.d_frames;
    a.max_wgs = b->eval_cus;
    hipError_t e = launch_vectors_shared(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_vectors_shared failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    // the next pack into this set waits for the vector launch too (the position launch's event is behind it in stream order)
    if (st.eval_pending && st.eval_done == st.eval_ev && st.eval_ev && hipEventRecord(st.eval_ev, stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream);
    }
    return FD_OK;
}

const char *fd_shared_vectors_kernel_name(int M, int frames, int kind)
{
    const char *pos = fd_shared_kernel_name(M, frames, kind);
    return pos[0] ? shared_vectors_kernel_name(round_up(M, kRecPad), frames, kind) : "";
}

// ---- every frame in fp64 by one matrix-pipe launch (fd_eval_shared64.hip) ----
static bool shared64_kind(int kind)
{
    return kind == FD_KERNEL_THIN_PLATE || kind == FD_KERNEL_GAUSSIAN || kind == FD_KERNEL_GAUSSIAN_QNN || kind == FD_KERNEL_BIHARMONIC ||
           kind == FD_KERNEL_CUBIC;
}

// the one launch, or (the multilayer model, an eval_variant override) the per-context launches
static bool shared64_fast(const fd_batch *b)
{
    const fd_ctx *c0 = b->ctxs[0];
    bool fast = shared64_kind(eval_kind(c0)) && c0->kind != FD_KERNEL_GAUSSIAN_ML;
    for (int i = 0; i < b->n; ++i)
        if (b->ctxs[i]->eval_variant > 0 || record_layers(b->ctxs[i]) != 0) fast = false;
    return fast;
}

// every context holds a model (built or being built) of ONE rest rig: each read its rest points in place from the SAME device
// array (as fd_batch_deform_shared_dev), with one kernel and term; `outputs`: and one fd_set_output setting
static int shot_check_rig(fd_batch *b, const char *who, bool outputs)
{
    const fd_ctx *c0 = b->ctxs[0];
    for (int i = 0; i < b->n; ++i) {
        const fd_ctx *c = b->ctxs[i];
        if (!c->built && !c->build_pending) { batch_err(b, "%s: context %d has no built model", who, i); return FD_E_NOT_BUILT; }
        if (!c->rest_src || c->rest_src != c0->rest_src || !same_model(c, c0)) {
            batch_err(b, "%s: the contexts must share one rest rig (fd_batch_set_points_dev with the "
                         "same rest array for all), kernel and term; context %d does not", who, i);
            return FD_E_INVALID;
        }
        if (outputs && c->output != c0->output) { batch_err(b, "%s: context %d has another fd_set_output setting than context 0", who, i); return FD_E_INVALID; }
    }
    return FD_OK;
}

int fd_batch_deform_shared_fp64_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, float *const *d_P_out,
                                    const float *d_dist2, float *const *d_falloff_out, const float *d_tu, const float *d_tv,
                                    const float *d_nrm, float radius2, float falloffrate)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    const char *who = "fd_batch_deform_shared_fp64_dev";
    int rc = shot_check_mesh(b, who, N, d_P_in, d_tu, d_tv, d_nrm);
    if (!rc) rc = shot_check_aliasing(b, who, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm);
    if (rc) return rc;
    if (N == 0) return FD_OK;
    fd_ctx *c0 = b->ctxs[0];
    rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    const bool fast = shared64_fast(b);
    if ((rc = shot_check_rig(b, who, true))) return rc;
    ShotScratch &sc = b->s64;
    if ((rc = shot_begin(b, who, sc, stream))) return rc;
    if (!fast) {
        // the multilayer model, an eval_variant override: per context, the launch of an FD_EVAL_FP64 context on the shared arrays
        for (int i = 0; i < b->n; ++i) {
            DeformArgs a = deform_args(b->ctxs[i], Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, d_P_out[i],
                                       d_falloff_out ? d_falloff_out[i] : nullptr);
            a.precision = FD_EVAL_FP64;
            hipError_t e = launch_deform(a, stream);
            if (e != hipSuccess) { batch_err(b, "launch_deform failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
        }
        // these launches read the models to their end
        if (hipEventRecord(sc.consumed_ev, stream) != hipSuccess) { (void)hipGetLastError(); return FD_E_DEVICE; }
        sc.consumed = true;
        return FD_OK;
    }
    Shared64Args a{};
    a.M = c0->M; a.Mpad = round_up(c0->M, kRecPad); a.kind = eval_kind(c0);
    const bool same_rig = one_build(b);
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        a.rec64[i] = c->d_rec64;
        a.centres[i] = same_rig ? c0->d_centres : c->d_centres;       // (one batched build read one array: equal by construction)
    }
    const size_t bytes = shared64_scratch_bytes(a.Mpad, b->n);
    if ((rc = shot_reserve(b, who, sc, bytes, stream))) return rc;
    fill_eval_common(a, b, sc, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    hipError_t e = launch_deform_shared64(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_deform_shared64 failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    shot_evaluated(sc, stream);
    return FD_OK;
}

const char *fd_shared_fp64_kernel_name(int M, int frames, int kind)
{
    if (M <= 0 || !shared64_kind(kind)) return "";
    return shared64_kernel_name(round_up(M, kRecPad), frames, kind);
}

// fd_batch_deform_vectors_shared_fp64_dev: the position call above, unchanged, then the vector launch (fd_vectors_shared64.hip)
// on the scratch its pack kernel wrote; where the one launch does not apply, launch_vectors per context in fp64
int fd_batch_deform_vectors_shared_fp64_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, float *const *d_P_out,
                                            const float *d_dist2, float *const *d_falloff_out, const float *d_tu, const float *d_tv,
                                            const float *d_nrm, float radius2, float falloffrate, const fd_batch_vectors *vec)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    const char *who = "fd_batch_deform_vectors_shared_fp64_dev";
    bool want;
    int rc = shot_check_vectors(b, who, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, vec, &want);
    if (rc) return rc;
    if (!want)
        return fd_batch_deform_shared_fp64_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    if (N == 0) return FD_OK;
    rc = fd_batch_deform_shared_fp64_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    if (rc) return rc;
    fd_ctx *c0 = b->ctxs[0];
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    if (!shared64_fast(b) || b->n < shared_vectors64_min_frames(eval_kind(c0))) {
        // per context, what fd_deform_vectors_dev launches for an FD_EVAL_FP64 context on the shared arrays (the multilayer model,
        // an eval_variant override -- and so few frames that these launches are the faster way: the positions above are
        // fd_batch_deform_shared_fp64_dev's either way)
        return vectors_per_context(b, stream, FD_EVAL_FP64, b->s64.consumed_ev, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm,
                                   radius2, falloffrate, vec);
    }
    SharedVector64Args a{};
    fill_mesh(a, N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate);
    a.Mpad = round_up(c0->M, kRecPad); a.nF = b->n; a.kind = eval_kind(c0);
    fill_vector_tables(a, b->n, vec);
    a.scratch = b->s64.d;
    a.max_wgs = b->eval_cus;
    hipError_t e = launch_vectors_shared64(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_vectors_shared64 failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    shot_vectors_evaluated(b->s64, stream);
    return FD_OK;
}

const char *fd_shared_vectors_fp64_kernel_name(int M, int frames, int kind)
{
    if (M <= 0 || !shared64_kind(kind)) return "";
    return shared_vectors64_kernel_name(round_up(M, kRecPad), frames, kind);
}

// ---- the adjoint in the vertex positions summed over the frames of a shot (fd_adjoint_points_shot.hip) ----
// grad_P = sum_f A_f^T g_f by one matrix-pipe launch on a scratch of its own; where that launch does not apply (the multilayer
// model, an eval_variant override, fewer frames than shared_adjoint_points_min_frames), launch_adjoint_points per context and
// the additions in frame order
int fd_batch_deform_adjoint_points_shared_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, const float *d_G,
                                              const float *d_dist2, const float *d_tu, const float *d_tv, const float *d_nrm,
                                              float radius2, float falloffrate, double *d_grad_P)
{
    if (!b) return FD_E_INVALID;
    const char *who = "fd_batch_deform_adjoint_points_shared_dev";
    if (!d_G || !d_grad_P) { batch_err(b, "%s: bad G / grad_P pointers", who); return FD_E_INVALID; }
    int rc = shot_check_mesh(b, who, N, d_P_in, d_tu, d_tv, d_nrm);
    if (rc) return rc;
    for (const void *in : {(const void *)d_P_in, (const void *)d_G, (const void *)d_dist2, (const void *)d_tu, (const void *)d_tv, (const void *)d_nrm})
        if (in && in == (const void *)d_grad_P) { batch_err(b, "%s: grad_P is an input array", who); return FD_E_INVALID; }
    if ((rc = shot_check_rig(b, who, false))) return rc;
    if (N == 0) return FD_OK;
    fd_ctx *c0 = b->ctxs[0];
    rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    ShotScratch &sc = b->sadjp;
    if ((rc = shot_begin(b, who, sc, stream))) return rc;
    if (!shared64_fast(b) || b->n < shared_adjoint_points_min_frames(eval_kind(c0))) {
        // frame 0 into grad_P, every later frame into the scratch and added: the frame-ordered sum of the one-frame results
        if (b->n > 1 && (rc = shot_reserve(b, who, sc, sizeof(double) * 3 * (size_t)N, stream))) return rc;
        for (int i = 0; i < b->n; ++i) {
            const DeformArgs a = deform_args(b->ctxs[i], Mesh{N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate}, nullptr, nullptr);
            double *dst = i == 0 ? d_grad_P : (double *)(void *)sc.d;
            hipError_t e = launch_adjoint_points(a, AdjointPointsArgs{d_G + (size_t)i * (size_t)N * 3, dst, nullptr}, stream);
            if (e == hipSuccess && i > 0) e = launch_adjoint_points_add(d_grad_P, dst, 3 * N, stream);
            if (e != hipSuccess) { batch_err(b, "launch_adjoint_points failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
        }
        // these launches read the models to their end
        if (hipEventRecord(sc.consumed_ev, stream) != hipSuccess) { (void)hipGetLastError(); return FD_E_DEVICE; }
        sc.consumed = true;
        if (b->n > 1) sc.eval_pending = record_eval(sc.eval_ev, stream);
        return FD_OK;
    }
    SharedAdjointPointsArgs a{};
    a.M = c0->M; a.Mpad = round_up(c0->M, kRecPad); a.kind = eval_kind(c0);
    const bool same_rig = one_build(b);
    for (int i = 0; i < b->n; ++i) {
        fd_ctx *c = b->ctxs[i];
        a.rec64[i] = c->d_rec64;
        a.centres[i] = same_rig ? c0->d_centres : c->d_centres;       // (one batched build read one array: equal by construction)
    }
    if ((rc = shot_reserve(b, who, sc, shared_adjoint_points_scratch_bytes(a.Mpad, b->n), stream))) return rc;
    fill_eval_common(a, b, sc, N, d_P_in, nullptr, d_dist2, nullptr, d_tu, d_tv, d_nrm, radius2, falloffrate);
    a.G = d_G; a.grad_P = d_grad_P;
    hipError_t e = launch_adjoint_points_shared(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_adjoint_points_shared failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    shot_evaluated(sc, stream);
    return FD_OK;
}

const char *fd_shared_adjoint_points_kernel_name(int M, int frames, int kind)
{
    if (M <= 0 || !shared64_kind(kind)) return "";
    return shared_adjoint_points_kernel_name(round_up(M, kRecPad), frames, kind);
}

// ---- every frame of a shot of multilayer models by one matrix-pipe launch (fd_eval_shared_ml.hip) ----
// where the launch applies: multilayer contexts of one model on one rest array, fp32, no eval_variant, enough frames.  Anything
// else -- an unbuilt context, another rest array, mixed outputs included -- is fd_batch_deform_shared_dev's to answer.
static bool shared_ml_fast(const fd_batch *b)
{
    const fd_ctx *c0 = b->ctxs[0];
    if (c0->kind != FD_KERNEL_GAUSSIAN_ML || !shared_ml_applies(c0->M, ml_layers(c0), b->n)) return false;
    for (int i = 0; i < b->n; ++i) {
        const fd_ctx *c = b->ctxs[i];
        if (!c->built && !c->build_pending) return false;
        if (!c->rest_src || c->rest_src != c0->rest_src || !same_model(c, c0) || c->output != c0->output) return false;
        if (c->eval_precision != FD_EVAL_FP32 || c->eval_variant > 0) return false;
    }
    return true;
}

int fd_batch_deform_shared_ml_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, float *const *d_P_out,
                                  const float *d_dist2, float *const *d_falloff_out, const float *d_tu, const float *d_tv,
                                  const float *d_nrm, float radius2, float falloffrate)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    const char *who = "fd_batch_deform_shared_ml_dev";
    int rc = shot_check_mesh(b, who, N, d_P_in, d_tu, d_tv, d_nrm);
    if (!rc) rc = shot_check_aliasing(b, who, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm);
    if (rc) return rc;
    if (N == 0) return FD_OK;
    if (!shared_ml_fast(b))
        return fd_batch_deform_shared_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    fd_ctx *c0 = b->ctxs[0];
    rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    ShotScratch &sc = b->sml;
    if ((rc = shot_begin(b, who, sc, stream))) return rc;
    SharedMlArgs a{};
    a.M = c0->M; a.layers = ml_layers(c0);
    a.check_rig = one_build(b) ? 0 : 1;                        // (one batched build read one array: equal by construction)
    for (int i = 0; i < b->n; ++i) a.rec32[i] = b->ctxs[i]->d_rec32;
    const size_t bytes = shared_ml_scratch_bytes(a.M, a.layers, b->n);
    if ((rc = shot_reserve(b, who, sc, bytes, stream))) return rc;
    fill_eval_common(a, b, sc, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    hipError_t e = launch_deform_shared_ml(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_deform_shared_ml failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    shot_evaluated(sc, stream);
    return FD_OK;
}

const char *fd_shared_ml_kernel_name(int M, int layers, int frames)
{
    return shared_ml_kernel_name(M, layers, frames);
}

// fd_batch_deform_vectors_shared_ml_dev: the position call above, unchanged, then the vector launch
// (fd_vectors_shared_ml.hip) on the scratch its pack kernel wrote; a multilayer batch of too few frames gets launch_vectors
// per context in fp32; anything else is fd_batch_deform_vectors_shared_dev's
int fd_batch_deform_vectors_shared_ml_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, float *const *d_P_out,
                                          const float *d_dist2, float *const *d_falloff_out, const float *d_tu, const float *d_tv,
                                          const float *d_nrm, float radius2, float falloffrate, const fd_batch_vectors *vec)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    const char *who = "fd_batch_deform_vectors_shared_ml_dev";
    bool want;
    int rc = shot_check_vectors(b, who, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, vec, &want);
    if (rc) return rc;
    if (!want)
        return fd_batch_deform_shared_ml_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    if (N == 0) return FD_OK;
    // other kinds, fp64 contexts, an eval_variant override, an imported model, layer counts outside 1..8, fewer frames than the
    // position launch takes: the one-layer call's, before anything of this one's is touched
    if (!shared_ml_fast(b))
        return fd_batch_deform_vectors_shared_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2,
                                                  falloffrate, vec);
    rc = fd_batch_deform_shared_ml_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    if (rc) return rc;
    fd_ctx *c0 = b->ctxs[0];
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    if (b->n < shared_vectors_ml_min_frames(ml_layers(c0))) {
        // so few frames that the per-context launches are the faster way: what fd_deform_vectors_dev launches for an
        // FD_EVAL_FP32 context -- which shared_ml_fast demands every context to be -- on the shared arrays (the positions above
        // are fd_batch_deform_shared_ml_dev's either way)
        return vectors_per_context(b, stream, FD_EVAL_FP32, b->sml.consumed_ev, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm,
                                   radius2, falloffrate, vec);
    }
    SharedVectorMlArgs a{};
    fill_mesh(a, N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate);
    a.M = c0->M; a.layers = ml_layers(c0); a.nF = b->n;
    fill_vector_tables(a, b->n, vec);
    a.scratch = b->sml.d;
    a.max_wgs = b->eval_cus;
    hipError_t e = launch_vectors_shared_ml(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_vectors_shared_ml failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    shot_vectors_evaluated(b->sml, stream);
    return FD_OK;
}

const char *fd_shared_vectors_ml_kernel_name(int M, int layers, int frames)
{
    return shared_vectors_ml_kernel_name(M, layers, frames);
}

// ---- every frame of a shot of multilayer models in fp64 by one matrix-pipe launch (fd_eval_shared_ml64.hip) ----
// where the launch applies: multilayer contexts of one model on one rest array, built here, no eval_variant, enough frames.
// Anything else -- an unbuilt context, another rest array, mixed outputs included -- is fd_batch_deform_shared_fp64_dev's to
// answer.
static bool shared_ml64_fast(const fd_batch *b)
{
    const fd_ctx *c0 = b->ctxs[0];
    if (c0->kind != FD_KERNEL_GAUSSIAN_ML || !shared_ml64_applies(c0->M, ml_layers(c0), b->n)) return false;
    for (int i = 0; i < b->n; ++i) {
        const fd_ctx *c = b->ctxs[i];
        if (!c->built && !c->build_pending) return false;
        if (!c->rest_src || c->rest_src != c0->rest_src || !same_model(c, c0) || c->output != c0->output) return false;
        if (c->eval_variant > 0) return false;
    }
    return true;
}

int fd_batch_deform_shared_ml_fp64_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, float *const *d_P_out,
                                       const float *d_dist2, float *const *d_falloff_out, const float *d_tu, const float *d_tv,
                                       const float *d_nrm, float radius2, float falloffrate)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    const char *who = "fd_batch_deform_shared_ml_fp64_dev";
    int rc = shot_check_mesh(b, who, N, d_P_in, d_tu, d_tv, d_nrm);
    if (!rc) rc = shot_check_aliasing(b, who, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm);
    if (rc) return rc;
    if (N == 0) return FD_OK;
    if (!shared_ml64_fast(b))
        return fd_batch_deform_shared_fp64_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    fd_ctx *c0 = b->ctxs[0];
    rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    ShotScratch &sc = b->sml64;
    if ((rc = shot_begin(b, who, sc, stream))) return rc;
    SharedMl64Args a{};
    a.M = c0->M; a.layers = ml_layers(c0);
    a.check_rig = one_build(b) ? 0 : 1;                        // (one batched build read one array: equal by construction)
    for (int i = 0; i < b->n; ++i) a.rec64[i] = b->ctxs[i]->d_rec64;
    const size_t bytes = shared_ml64_scratch_bytes(a.M, a.layers, b->n);
    if ((rc = shot_reserve(b, who, sc, bytes, stream))) return rc;
    fill_eval_common(a, b, sc, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    hipError_t e = launch_deform_shared_ml64(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_deform_shared_ml64 failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    shot_evaluated(sc, stream);
    return FD_OK;
}

const char *fd_shared_ml_fp64_kernel_name(int M, int layers, int frames)
{
    return shared_ml64_kernel_name(M, layers, frames);
}

// fd_batch_deform_vectors_shared_ml_fp64_dev: the position call above, unchanged, then the vector launch
// (fd_vectors_shared_ml64.hip) on the scratch its pack kernel wrote; a multilayer batch of too few frames gets launch_vectors
// per context in fp64; anything else is fd_batch_deform_vectors_shared_fp64_dev's
int fd_batch_deform_vectors_shared_ml_fp64_dev(fd_batch *b, void *hip_stream, int64_t N, const float *d_P_in, float *const *d_P_out,
                                               const float *d_dist2, float *const *d_falloff_out, const float *d_tu, const float *d_tv,
                                               const float *d_nrm, float radius2, float falloffrate, const fd_batch_vectors *vec)
{
    if (!b || !d_P_out) return FD_E_INVALID;
    const char *who = "fd_batch_deform_vectors_shared_ml_fp64_dev";
    bool want;
    int rc = shot_check_vectors(b, who, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, vec, &want);
    if (rc) return rc;
    if (!want)
        return fd_batch_deform_shared_ml_fp64_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    if (N == 0) return FD_OK;
    // other kinds, an eval_variant override, an imported model, layer counts outside 1..8: the one-layer call's, before
    // anything of this one's is touched
    if (!shared_ml64_fast(b))
        return fd_batch_deform_vectors_shared_fp64_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2,
                                                       falloffrate, vec);
    rc = fd_batch_deform_shared_ml_fp64_dev(b, hip_stream, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm, radius2, falloffrate);
    if (rc) return rc;
    fd_ctx *c0 = b->ctxs[0];
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    if (b->n < shared_vectors_ml64_min_frames(ml_layers(c0))) {
        // so few frames that the per-context launches are the faster way: what fd_deform_vectors_dev launches for an
        // FD_EVAL_FP64 context on the shared arrays (the positions above are fd_batch_deform_shared_ml_fp64_dev's either way)
        return vectors_per_context(b, stream, FD_EVAL_FP64, b->sml64.consumed_ev, N, d_P_in, d_P_out, d_dist2, d_falloff_out, d_tu, d_tv, d_nrm,
                                   radius2, falloffrate, vec);
    }
    SharedVectorMl64Args a{};
    fill_mesh(a, N, d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate);
    a.M = c0->M; a.layers = ml_layers(c0); a.nF = b->n;
    fill_vector_tables(a, b->n, vec);
    a.scratch = b->sml64.d;
    a.max_wgs = b->eval_cus;
    hipError_t e = launch_vectors_shared_ml64(a, stream);
    if (e != hipSuccess) { batch_err(b, "launch_vectors_shared_ml64 failed: %s", hipGetErrorString(e)); return FD_E_DEVICE; }
    shot_vectors_evaluated(b->sml64, stream);
    return FD_OK;
}

const char *fd_shared_vectors_ml_fp64_kernel_name(int M, int layers, int frames)
{
    return shared_vectors_ml64_kernel_name(M, layers, frames);
}

int fd_batch_wait_consumed(fd_batch *b, void *hip_stream)
{
    if (!b) return FD_E_INVALID;
    hipEvent_t ev = b->consumed_override ? b->consumed_override : (b->packed_valid ? b->sets[b->cur_set].packed_ev : b->fallback_ev);
    // ... and the reads of the calls that keep a scratch of their own as well
    hipEvent_t evs[5] = {ev, nullptr, nullptr, nullptr, nullptr};
    int n_ev = ev ? 1 : 0;
    for (const ShotScratch *sc : {&b->s64, &b->sml, &b->sml64, &b->sadjp})
        if (sc->consumed) evs[n_ev++] = sc->consumed_ev;
    if (n_ev == 0) return FD_OK;                 // no shared-rig evaluation enqueued: nothing reads the models beyond stream order
    fd_ctx *c0 = b->ctxs[0];
    int rc = use_device(c0);
    if (rc) { batch_err(b, "%s", c0->err); return rc; }
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : cur_stream(c0);
    for (int i = 0; i < n_ev; ++i)
        if (hipStreamWaitEvent(stream, evs[i], 0) != hipSuccess) {
            batch_err(b, "fd_batch_wait_consumed: hipStreamWaitEvent failed: %s", hipGetErrorString(hipGetLastError()));
            return FD_E_DEVICE;
        }
    return FD_OK;
}

int fd_batch_cook_group(fd_batch *b, void *build_stream, void *eval_stream, const float *d_rest_xyz,
                        const float *const *d_delta_xyz, int M, int64_t N, const float *d_P_in, float *const *d_P_out,
                        float *const *d_falloff_out, const fd_group_events *events)
{
    if (!b || !d_rest_xyz || !d_delta_xyz || !d_P_out) return FD_E_INVALID;
    fd_ctx *c0 = b->ctxs[0];
    hipStream_t bs = build_stream ? (hipStream_t)build_stream : cur_stream(c0);
    hipStream_t es = eval_stream ? (hipStream_t)eval_stream : bs;
    auto mark = [&](void *ev, hipStream_t st) { if (ev && hipEventRecord((hipEvent_t)ev, st) != hipSuccess) (void)hipGetLastError(); };
#ifdef FD_TUNING
    // FD_COOK_TIMING=1: host time of the call's pieces on stderr (us): wait_consumed | set_points | build (launches) | packing | evaluation
    static const bool cook_timing = tuning_env("FD_COOK_TIMING") != nullptr;
    struct CookClock {
        bool on; double t[6]; int n = 0;
        static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
        void tick() { if (on && n < 6) t[n++] = now(); }
        ~CookClock() { if (on && n == 6) fprintf(stderr, "[cook_group host us] wait_consumed %.1f | set_points %.1f | build %.1f | packing %.1f | evaluation %.1f\n", t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4]); }
    } clk{cook_timing};
#define FD_COOK_TICK() clk.tick()
#else
#define FD_COOK_TICK()
#endif
    FD_COOK_TICK();
    int rc = fd_batch_wait_consumed(b, build_stream);
    if (rc) return rc;
    FD_COOK_TICK();
    const float *rest[kMaxBatch];
    for (int i = 0; i < b->n; ++i) rest[i] = d_rest_xyz;
    if ((rc = fd_batch_set_points_dev(b, rest, d_delta_xyz, M))) return rc;
    // one stream for everything: no event between the build, the packing and the evaluation (see fd_batch::lean)
    const bool lean = es == bs;
    struct LeanScope {
        fd_batch *b; hipStream_t s; bool on, built = false;
        ~LeanScope() {
            if (!on) return;
            // the build's end, as every waiter and the status poll know it: behind whatever of the group was enqueued
            if (built && hipEventRecord(b->ev1, s) != hipSuccess) (void)hipGetLastError();
            b->prepared = false;          // the set was packed without its event: a later call on another stream packs again
            b->lean = false;
        }
    } scope{b, bs, lean};
    b->lean = lean;
    FD_COOK_TICK();
    if (events) mark(events->before_build, bs);
    if ((rc = fd_batch_build_async(b, build_stream))) return rc;
    scope.built = true;
    if (events) mark(events->after_build, bs);
    FD_COOK_TICK();
    if ((rc = fd_batch_prepare_shared(b, build_stream, d_P_out, d_falloff_out))) return rc;
    FD_COOK_TICK();
    if (es != bs) {
        // (the evaluation waits for the pack kernel's event inside fd_batch_deform_shared_dev when the set was prepared; the
        // per-frame fallback -- other kernels -- needs the builds themselves)
        if (!b->group_ev.make() || hipEventRecord(b->group_ev, bs) != hipSuccess || hipStreamWaitEvent(es, b->group_ev, 0) != hipSuccess) {
            batch_err(b, "fd_batch_cook_group: ordering the evaluation stream failed: %s", hipGetErrorString(hipGetLastError()));
            return FD_E_DEVICE;
        }
    }
    if (events) mark(events->before_eval, es);
    rc = fd_batch_deform_shared_dev(b, es, N, d_P_in, d_P_out, nullptr, d_falloff_out, nullptr, nullptr, nullptr, 1.0f, 1.0f);
    if (events) mark(events->after_eval, es);
    FD_COOK_TICK();
    if (lean && rc == FD_OK && b->packed_valid && b->sets[b->cur_set].eval_pending) b->consumed_override = b->ev1;      // (recorded by `scope` on the way out)
    return rc;
}

int fd_batch_set_eval_cus(fd_batch *b, int n_cus)
{
    if (!b) return FD_E_INVALID;
    b->eval_cus = n_cus > 0 ? n_cus : 0;
    return FD_OK;
}

int fd_batch_set_shared_factor(fd_batch *b, int on)
{
    if (!b) return FD_E_INVALID;
    b->shared_factor = on ? 1 : 0;
    return FD_OK;
}

int fd_batch_last_build_shared_factor(const fd_batch *b) { return b ? b->last_shared_factor : 0; }

const char *fd_shared_ml_build_kernel_name(int M, int layers, int frames) { return ml_shared_kernel_name(M, layers, frames); }

int fd_batch_set_shared_lu(fd_batch *b, int on)
{
    if (!b) return FD_E_INVALID;
    b->shared_lu = on ? 1 : 0;
    return FD_OK;
}

const char *fd_shared_qnn_build_kernel_name(int M, int frames) { return qnn_shared_kernel_name(M, frames); }

int fd_batch_size(const fd_batch *b) { return b ? b->n : 0; }

const char *fd_shared_kernel_name(int M, int frames, int kind)
{
    const bool takes = (kind == FD_KERNEL_THIN_PLATE || kind == FD_KERNEL_GAUSSIAN || kind == FD_KERNEL_GAUSSIAN_QNN) && M > 0 && round_up(M, kRecPad) >= 32 &&
                       frames >= 1 && frames <= kMaxBatch;
    return takes ? shared_plan(round_up(M, kRecPad), frames, kind).kernel : "";
}

}  // extern "C"

// ---- the device side of fdsop_cook_shot (fd_shot_dev.h) ----------------------------------------------------------------
#include "fd_shot_dev.h"

struct fd_shot_dev {
    fd_ctx *engine = nullptr;
    Stream work, copy;                  // in front of what is enqueued on them: they outlive it
    DevBuf<float> d_rig;                // rest (M x 3), then F x M x 3 deltas
    int M = 0, F = 0;
    DevBuf<float> d_vecs;               // the mesh's N, tu, tv as uploaded by fd_shot_dev_set_vectors (a slice each), cap / 9 vertices each
    const float *v_in[3] = {nullptr, nullptr, nullptr};   // N, tu, tv inputs, or null
    struct Set {
        DevBuf<float> d;
        Event eval_ev, delivered_ev;
        bool delivering = false;
    } sets[2];
    int set_frames = 0;                 // what the two sets were laid out for
    int64_t set_Np = 0;
    bool set_fall = false;
    int set_nvec = 0;
    char err[512] = {0};
};

static void shot_err(fd_shot_dev *sd, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(sd->err, sizeof(sd->err), fmt, ap);
    va_end(ap);
}

// a runtime call that failed, as the shot calls report it
static int shot_failed(fd_shot_dev *sd, const char *call, hipError_t e)
{
    (void)hipGetLastError();
    shot_err(sd, "%s failed: %s", call, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? FD_E_NOMEM : FD_E_DEVICE;
}

#define FD_SHIP(sd, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return shot_failed(sd, #call, e_);                                   \
    } while (0)

// slices of a staging set: positions of every frame, then the fall-off of every frame, then the vectors
static int64_t shot_pad(int64_t N) { return (N + 63) / 64 * 64; }
static float *shot_slice_P(const fd_shot_dev *sd, int set, int slot) { return sd->sets[set].d + (size_t)slot * 3 * (size_t)sd->set_Np; }
static float *shot_slice_fall(const fd_shot_dev *sd, int set, int slot)
{
    return sd->set_fall ? sd->sets[set].d + ((size_t)sd->set_frames * 3 + (size_t)slot) * (size_t)sd->set_Np : nullptr;
}
static float *shot_slice_vec(const fd_shot_dev *sd, int set, int which, int slot)
{
    const size_t base = (size_t)sd->set_frames * (sd->set_fall ? 4 : 3);
    return sd->sets[set].d + (base + ((size_t)which * sd->set_frames + (size_t)slot) * 3) * (size_t)sd->set_Np;
}
static int shot_nvec(const fd_shot_dev *sd) { return (sd->v_in[0] != nullptr) + (sd->v_in[1] != nullptr) + (sd->v_in[2] != nullptr); }

fd_shot_dev *fd_shot_dev_create(fd_ctx *engine)
{
    if (!engine || use_device(engine) != FD_OK) return nullptr;
    fd_shot_dev *sd = new (std::nothrow) fd_shot_dev();
    if (!sd) return nullptr;
    sd->engine = engine;
    bool ok = sd->work.create() == hipSuccess && sd->copy.create() == hipSuccess;
    for (auto &st : sd->sets)
        ok = ok && st.eval_ev.create(hipEventDisableTiming) == hipSuccess && st.delivered_ev.create(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        set_err(nullptr, "fd_shot_dev_create: device resource allocation failed: %s", hipGetErrorString(hipGetLastError()));
        fd_shot_dev_destroy(sd);
        return nullptr;
    }
    return sd;
}

void fd_shot_dev_destroy(fd_shot_dev *sd)
{
    if (!sd) return;
    (void)hipSetDevice(sd->engine->device);
    if (sd->work) { (void)hipStreamSynchronize(sd->work); }
    if (sd->copy) { (void)hipStreamSynchronize(sd->copy); }
    delete sd;                  // the members release what they own, the two streams last
}

const char *fd_shot_dev_error(const fd_shot_dev *sd) { return sd ? sd->err : g_err; }
void *fd_shot_dev_work_stream(fd_shot_dev *sd) { return sd ? (void *)sd->work : nullptr; }

int fd_shot_dev_set_rig(fd_shot_dev *sd, const float *rest, const float *deltas, int M, int F)
{
    if (!sd || !rest || !deltas || M <= 0 || F <= 0) return FD_E_INVALID;
    int rc = use_device(sd->engine);
    if (rc) { shot_err(sd, "%s", sd->engine->err); return rc; }
    const size_t floats = (size_t)(F + 1) * (size_t)M * 3;
    if (floats > sd->d_rig.cap) {
        // (the batches read the old block in place: nothing of them may still be in flight)
        FD_SHIP(sd, hipStreamSynchronize(sd->work));
        const hipError_t e = sd->d_rig.grow(floats);
        if (e != hipSuccess) return shot_failed(sd, "hipMalloc((void **)&sd->d_rig, sizeof(float) * floats)", e);
    }
    sd->M = M; sd->F = F;
    const size_t rb = sizeof(float) * 3 * (size_t)M;
    FD_SHIP(sd, hipMemcpyAsync(sd->d_rig, rest, rb, hipMemcpyHostToDevice, sd->work));
    FD_SHIP(sd, hipMemcpyAsync(sd->d_rig + 3 * (size_t)M, deltas, rb * (size_t)F, hipMemcpyHostToDevice, sd->work));
    FD_SHIP(sd, hipStreamSynchronize(sd->work));          // pageable sources: the caller's vectors may go away
    return FD_OK;
}

const float *fd_shot_dev_rest(const fd_shot_dev *sd) { return sd ? sd->d_rig : nullptr; }
const float *fd_shot_dev_delta(const fd_shot_dev *sd, int frame)
{
    return (sd && sd->d_rig && frame >= 0 && frame < sd->F) ? sd->d_rig + (size_t)(frame + 1) * 3 * (size_t)sd->M : nullptr;
}

int fd_shot_dev_set_vectors(fd_shot_dev *sd, const float *N, const float *tu, const float *tv)
{
    if (!sd) return FD_E_INVALID;
    sd->v_in[0] = sd->v_in[1] = sd->v_in[2] = nullptr;
    if (!N && !tu && !tv) return FD_OK;
    const int64_t n = sd->engine->mesh_N;
    if (n <= 0) { shot_err(sd, "fd_shot_dev_set_vectors: the engine has no mesh"); return FD_E_INVALID; }
    int rc = use_device(sd->engine);
    if (rc) { shot_err(sd, "%s", sd->engine->err); return rc; }
    const int64_t Np = shot_pad(n);
    if (9 * (size_t)Np > sd->d_vecs.cap) {
        FD_SHIP(sd, hipStreamSynchronize(sd->work));
        const hipError_t e = sd->d_vecs.grow(9 * (size_t)Np);
        if (e != hipSuccess) return shot_failed(sd, "hipMalloc((void **)&sd->d_vecs, sizeof(float) * 9 * (size_t)Np)", e);
    }
    const float *src[3] = {N, tu, tv};
    for (int i = 0; i < 3; ++i) {
        if (!src[i]) continue;
        float *dst = sd->d_vecs + (size_t)i * (sd->d_vecs.cap / 3);
        FD_SHIP(sd, hipMemcpyAsync(dst, src[i], sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, sd->work));
        sd->v_in[i] = dst;
    }
    FD_SHIP(sd, hipStreamSynchronize(sd->work));
    return FD_OK;
}

int fd_shot_dev_reserve(fd_shot_dev *sd, int frames, int want_falloff)
{
    if (!sd || frames <= 0 || frames > kMaxBatch) return 0;
    const int64_t n = sd->engine->mesh_N;
    if (n <= 0 || use_device(sd->engine) != FD_OK) return 0;
    const int64_t Np = shot_pad(n);
    const int nvec = shot_nvec(sd);
    const bool fall = want_falloff != 0;
    if (sd->sets[0].d && sd->sets[1].d && sd->set_frames >= frames && sd->set_Np == Np && sd->set_fall == fall && sd->set_nvec == nvec)
        return frames;
    // another layout: the old sets go (nothing reads them once both streams have drained)
    (void)hipStreamSynchronize(sd->work);
    (void)hipStreamSynchronize(sd->copy);
    for (auto &st : sd->sets) { st.d.reset(); st.delivering = false; }
    sd->set_frames = 0;
    for (int f = frames; f >= 1; f = f / 2) {
        const size_t floats = (size_t)f * (size_t)Np * (size_t)(3 + (fall ? 1 : 0) + 3 * nvec);
        bool ok = true;
        for (auto &st : sd->sets) ok = ok && st.d.grow(floats) == hipSuccess;
        if (ok) {
            sd->set_frames = f; sd->set_Np = Np; sd->set_fall = fall; sd->set_nvec = nvec;
            return f;
        }
        (void)hipGetLastError();
        for (auto &st : sd->sets) st.d.reset();
    }
    shot_err(sd, "hipMalloc of the shot's staging sets failed: %s", hipGetErrorString(hipErrorOutOfMemory));
    return 0;
}

int fd_shot_dev_wait(fd_shot_dev *sd, int set)
{
    if (!sd || set < 0 || set > 1) return FD_E_INVALID;
    if (!sd->sets[set].delivering) return FD_OK;
    sd->sets[set].delivering = false;
    FD_SHIP(sd, hipEventSynchronize(sd->sets[set].delivered_ev));
    return FD_OK;
}

// the engine's device-resident mesh as the evaluation calls take it
struct ShotMesh { int64_t N; const float *P, *d2, *tu, *tv, *nr; };
static ShotMesh shot_mesh(const fd_ctx *e)
{
    ShotMesh m{e->mesh_N, e->m_P, e->mesh_has_dist2 ? e->m_dist2 : nullptr, nullptr, nullptr, nullptr};
    if (e->mesh_has_frames) { m.tu = e->m_tu; m.tv = e->m_tv; m.nr = e->m_nrm; }
    return m;
}

int fd_shot_dev_eval(fd_shot_dev *sd, fd_batch *b, int set, int fp64, int multilayer, float radius2, float falloffrate)
{
    if (!sd || !b || set < 0 || set > 1) return FD_E_INVALID;
    const int n = b->n;
    if (!sd->sets[set].d || n > sd->set_frames) { shot_err(sd, "fd_shot_dev_eval: no staging set for %d frames", n); return FD_E_INVALID; }
    int rc = fd_shot_dev_wait(sd, set);
    if (rc) return rc;
    const ShotMesh m = shot_mesh(sd->engine);
    if (m.N <= 0 || shot_pad(m.N) != sd->set_Np) { shot_err(sd, "fd_shot_dev_eval: the staging sets were laid out for another mesh"); return FD_E_INVALID; }
    float *P_out[kMaxBatch], *fall[kMaxBatch], *vo[3][kMaxBatch];
    for (int i = 0; i < n; ++i) {
        P_out[i] = shot_slice_P(sd, set, i);
        fall[i] = shot_slice_fall(sd, set, i);
    }
    fd_batch_vectors vec{};
    vec.struct_size = (int)sizeof(vec);
    int which = 0;
    for (int k = 0; k < 3; ++k) {
        if (!sd->v_in[k]) continue;
        for (int i = 0; i < n; ++i) vo[k][i] = shot_slice_vec(sd, set, which, i);
        ++which;
    }
    if (sd->v_in[0]) { vec.N = sd->v_in[0]; vec.N_out = vo[0]; }
    if (sd->v_in[1]) { vec.tu = sd->v_in[1]; vec.tu_out = vo[1]; }
    if (sd->v_in[2]) { vec.tv = sd->v_in[2]; vec.tv_out = vo[2]; }
    const bool with_vec = which > 0;
    // a gated vertex's fd_falloff entry is not written by the launches: it reads 0, the attribute's default (:401)
    if (sd->set_fall && (m.d2 || radius2 < 0.f))
        FD_SHIP(sd, hipMemsetAsync(shot_slice_fall(sd, set, 0), 0, sizeof(float) * (size_t)n * (size_t)sd->set_Np, sd->work));
    float *const *fo = sd->set_fall ? fall : nullptr;
    if (with_vec) {
        auto call = fp64 ? (multilayer ? fd_batch_deform_vectors_shared_ml_fp64_dev : fd_batch_deform_vectors_shared_fp64_dev)
                         : (multilayer ? fd_batch_deform_vectors_shared_ml_dev : fd_batch_deform_vectors_shared_dev);
        rc = call(b, sd->work, m.N, m.P, P_out, m.d2, fo, m.tu, m.tv, m.nr, radius2, falloffrate, &vec);
    } else {
        auto call = fp64 ? (multilayer ? fd_batch_deform_shared_ml_fp64_dev : fd_batch_deform_shared_fp64_dev)
                         : (multilayer ? fd_batch_deform_shared_ml_dev : fd_batch_deform_shared_dev);
        rc = call(b, sd->work, m.N, m.P, P_out, m.d2, fo, m.tu, m.tv, m.nr, radius2, falloffrate);
    }
    if (rc) { shot_err(sd, "%s", b->err); return rc; }
    FD_SHIP(sd, hipEventRecord(sd->sets[set].eval_ev, sd->work));
    return FD_OK;
}

int fd_shot_dev_eval_fp64_over(fd_shot_dev *sd, fd_ctx *ctx, int set, int slot, float radius2, float falloffrate)
{
    if (!sd || !ctx || set < 0 || set > 1 || slot < 0 || slot >= sd->set_frames || !sd->sets[set].d) return FD_E_INVALID;
    const ShotMesh m = shot_mesh(sd->engine);
    fd_vectors vec{};
    vec.struct_size = (int)sizeof(vec);
    int which = 0;
    float *vo[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k)
        if (sd->v_in[k]) vo[k] = shot_slice_vec(sd, set, which++, slot);
    if (sd->v_in[0]) { vec.N = sd->v_in[0]; vec.N_out = vo[0]; }
    if (sd->v_in[1]) { vec.tu = sd->v_in[1]; vec.tu_out = vo[1]; }
    if (sd->v_in[2]) { vec.tv = sd->v_in[2]; vec.tv_out = vo[2]; }
    const int before = ctx->eval_precision;
    ctx->eval_precision = FD_EVAL_FP64;
    const int rc = deform_dev(ctx, "fd_deform", sd->work, Mesh{m.N, m.P, m.d2, m.tu, m.tv, m.nr, radius2, falloffrate},
                              shot_slice_P(sd, set, slot), shot_slice_fall(sd, set, slot), which > 0 ? &vec : nullptr);
    ctx->eval_precision = before;
    if (rc) { shot_err(sd, "%s", ctx->err); return rc; }
    FD_SHIP(sd, hipEventRecord(sd->sets[set].eval_ev, sd->work));
    return FD_OK;
}

int fd_shot_dev_deliver(fd_shot_dev *sd, int set, int n, const unsigned char *skip, float *const *P_out, float *const *falloff,
                        float *const *N_out, float *const *tu_out, float *const *tv_out)
{
    if (!sd || set < 0 || set > 1 || n <= 0 || n > sd->set_frames || !P_out || !sd->sets[set].d) return FD_E_INVALID;
    const int64_t N = sd->engine->mesh_N;
    const size_t b3 = sizeof(float) * 3 * (size_t)N, b1 = sizeof(float) * (size_t)N;
    FD_SHIP(sd, hipStreamWaitEvent(sd->copy, sd->sets[set].eval_ev, 0));
    float *const *vt[3] = {N_out, tu_out, tv_out};
    for (int i = 0; i < n; ++i) {
        if (skip && skip[i]) continue;
        // page-locked arrays are written asynchronously; pageable ones go through the runtime's staging, as in fd_deform_mesh
        if (P_out[i]) FD_SHIP(sd, hipMemcpyAsync(P_out[i], shot_slice_P(sd, set, i), b3, hipMemcpyDeviceToHost, sd->copy));
        if (falloff && falloff[i] && sd->set_fall)
            FD_SHIP(sd, hipMemcpyAsync(falloff[i], shot_slice_fall(sd, set, i), b1, hipMemcpyDeviceToHost, sd->copy));
        int which = 0;
        for (int k = 0; k < 3; ++k) {
            if (!sd->v_in[k]) continue;
            if (vt[k] && vt[k][i]) FD_SHIP(sd, hipMemcpyAsync(vt[k][i], shot_slice_vec(sd, set, which, i), b3, hipMemcpyDeviceToHost, sd->copy));
            ++which;
        }
    }
    FD_SHIP(sd, hipEventRecord(sd->sets[set].delivered_ev, sd->copy));
    sd->sets[set].delivering = true;
    return FD_OK;
}

int fd_shot_dev_vectors_engine(fd_shot_dev *sd, float radius2, float falloffrate, float *N_out, float *tu_out, float *tv_out)
{
    if (!sd || !sd->sets[0].d || sd->set_frames < 1) return FD_E_INVALID;
    int rc = fd_shot_dev_wait(sd, 0);
    if (rc) return rc;
    fd_ctx *e = sd->engine;
    const ShotMesh m = shot_mesh(e);
    fd_vectors vec{};
    vec.struct_size = (int)sizeof(vec);
    int which = 0;
    float *vo[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k)
        if (sd->v_in[k]) vo[k] = shot_slice_vec(sd, 0, which++, 0);
    if (which == 0) { shot_err(sd, "fd_shot_dev_vectors_engine: no vectors were set"); return FD_E_INVALID; }
    if (sd->v_in[0]) { vec.N = sd->v_in[0]; vec.N_out = vo[0]; }
    if (sd->v_in[1]) { vec.tu = sd->v_in[1]; vec.tu_out = vo[1]; }
    if (sd->v_in[2]) { vec.tv = sd->v_in[2]; vec.tv_out = vo[2]; }
    hipStream_t s = cur_stream(e);
    if (sd->set_fall && (m.d2 || radius2 < 0.f)) FD_SHIP(sd, hipMemsetAsync(shot_slice_fall(sd, 0, 0), 0, sizeof(float) * (size_t)sd->set_Np, s));
    rc = deform_dev(e, "fd_deform", s, Mesh{m.N, m.P, m.d2, m.tu, m.tv, m.nr, radius2, falloffrate}, shot_slice_P(sd, 0, 0),
                    shot_slice_fall(sd, 0, 0), &vec);
    if (rc) { shot_err(sd, "%s", e->err); return rc; }
    float *const host[3] = {N_out, tu_out, tv_out};
    const size_t b3 = sizeof(float) * 3 * (size_t)m.N;
    for (int k = 0; k < 3; ++k)
        if (vo[k] && host[k]) FD_SHIP(sd, hipMemcpyAsync(host[k], vo[k], b3, hipMemcpyDeviceToHost, s));
    FD_SHIP(sd, hipStreamSynchronize(s));
    return FD_OK;
}
