// fd_internal.h -- shared declarations of the gfx950 RBF deformation engine.
// Not part of the ABI (that is include/facedeform_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/facedeform_hip.h"

#include "fd_tuning.h"

namespace fd {

// A pointer fetched from a table in memory is a generic pointer to the compiler: every access
// through it becomes a flat_load / flat_store, which counts on BOTH wait counters and so
// serialises against LDS traffic.  The build kernels take their buffers from the batch table, so
// they say explicitly that these live in global memory.
#define FD_GLOBAL __attribute__((address_space(1)))
typedef double FD_GLOBAL gdouble;
typedef const double FD_GLOBAL gcdouble;
template <typename T> __host__ __device__ __forceinline__ T FD_GLOBAL *as_global(T *p) { return (T FD_GLOBAL *)p; }

// ---- solved model as the evaluation kernels read it --------------------------
// One record per centre, 32 B: the unit a scalar s_load_dwordx8 fetches.
//   s  = per-centre kernel scale (Gaussian: -log2(e)/R_j^2, otherwise 0)
//   w* = RBF weight pre-multiplied by the kernel's constant factor
//        (thin-plate: 0.5*ln2, so phi' = d2*log2(d2); biharmonic: -1, phi' = sqrt(d2))
struct Rec32 {
    float cx, cy, cz, s;
    float wx, wy, wz, pad;
};
struct Rec64 {
    double cx, cy, cz, s;
    double wx, wy, wz, pad;
};

// Centres are padded with zero-weight records to a multiple of this.
constexpr int kRecPad = 16;   // also the centre-tile height of the matrix-pipe evaluation

// Centre tile of the thin-plate matrix-pipe evaluation (16 centres): the A operand of one
// v_mfma_f32_16x16x32_bf16 as every lane reads it, and the weights of the tile arranged per
// 16-lane group the way the accumulate consumes them.  1280 B, 16-byte aligned.
struct MfmaTile {
    unsigned int a[64][4];   // lane l: 8 bf16 = k-slots 8*(l>>4) .. +7 of centre (l&15)
    float w[4][12];          // group g: {c0:(r0,r1) c1:(r0,r1) c2:(r0,r1) c0:(r2,r3) c1:(r2,r3) c2:(r2,r3)}, centre = 4g + r
    float pad[16];
};
static_assert(sizeof(MfmaTile) == 1280, "tile image must stay 1280 bytes");

// The same tile for v_mfma_f32_16x16x16_f16: every fp32 value as TWO fp16 pieces (hi + lo, 22
// bits; fp16 subnormals are honoured by the matrix pipe, tools/mfma_f16_subnormal_test.hip), all
// four cross products per coordinate in K = 16.  Half the operand bytes and half the MFMA time
// of the bf16 tile, at ~2x its d2 rounding error.  768 B.
struct MfmaTileH {
    unsigned int a[64][2];   // lane l: 4 fp16 = k-slots 4*(l>>4) .. +3 of centre (l&15)
    float w[4][12];          // as MfmaTile::w
    float pad[16];
};
static_assert(sizeof(MfmaTileH) == 768, "fp16 tile image must stay 768 bytes");

// Device-resident build status + affine part; read by the deform kernel so that
// an asynchronous build needs no host round trip before the deform launch.
struct DevModel {
    int terminationtype;   // 1 ok, -4, -5; 0 = not built
    int dup_flag;          // set by the assembly kernel: coincident centres
    int sing_flag;         // set by the panel kernel: pivot below threshold
    int iterations;        // elimination steps done
    unsigned long long amax_bits;  // max |A_ij| as raw double bits (atomicMax)
    unsigned long long pivmin_bits;
    unsigned long long pivmax_bits;
    // fp64 evaluation, raw coordinates: affine64[c*4 + 0] = constant of output c,
    // affine64[c*4 + 1..3] = x,y,z coefficients
    double affine64[12];
    // fp32 evaluation works in normalised coordinates x' = (x - x0) * inv_s, inv_s a power of
    // two (exact): norm32 = {x0.x, x0.y, x0.z, inv_s}.  poly32[c*5 + 0..4] = {C0, Lx, Ly, Lz, q}
    // of output c: affine part re-expressed in x' plus, for thin-plate, the exact correction
    // kappa * sum_j w_j |x' - c'_j|^2 that the change of length unit brings (kappa = s^2 ln s).
    float norm32[4];
    float poly32[15];
    float wmax32;          // largest |weight| or |polynomial coefficient| as the fp32 records carry them: the shared-rig launch scales by it
    // what the packing code estimates about the fp32 evaluation of this model (fd_pack.h; fd_report carries them)
    double fp32_error, cancellation, delta_min, delta_max, extent;
};

// Blob header for fd_export_model / fd_import_model.
struct ModelHeader {
    uint32_t magic;        // 'FDM2'
    int32_t M, kind, term, nparams;
    int32_t terminationtype;
    int32_t layers;        // multilayer Gaussian model: records per centre (the blob's arrays are layer-major); 0 otherwise
    int32_t reserved;
    double params[4];
    // Identity of the rest rig the model was built on: the exporter's in-place rest array (fd_batch_set_points_dev), 0 when
    // it had none.  Models imported with the same non-zero token came from ONE rest rig -- frames of a shot that one rank
    // solved and the others received -- which is what fd_batch_deform_shared_dev needs to know about them.
    uint64_t rig_token;
};
constexpr uint32_t kModelMagic = 0x324D4446u;

static inline int term_cols(int term) { return term == FD_TERM_LINEAR ? 4 : (term == FD_TERM_CONST ? 1 : 0); }
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- build pipeline (fd_build.hip) -------------------------------------------
constexpr int kPanelThreads = 1024;   // one workgroup factors a panel
constexpr int kMaxOrder = 5632;       // back-substitution keeps Y (3 x order fp64) in LDS
constexpr int kRhsCols = 16;          // 3 right-hand sides padded to one MFMA tile
constexpr int kMovesStride = 132;     // ints per elimination step's move list: count + 2 * (2 * 32) pairs
static inline int lu_step_capacity(int npad) { return npad / 4 + 2; }   // steps a system of this order can take

constexpr int kMaxBatch = 32;         // models one launch chain may build together

// Device-side table entry: the buffers of one model.  Every build kernel indexes the table
// with blockIdx.z, so a batch of contexts is assembled and factorised by one launch chain.
struct BatchSlot {
    float *rest, *delta;              // M x 3, the context's own copy of the control points
    double *centres;                  // M x 3
    double *radii;                    // M
    double *A;                        // lda x (ncols + 16): 16 zero columns absorb block overrun
    double *X;                        // 3 x npad solution, column per right-hand side
    double *W;                        // (M+4) x 3
    int *ipiv;                        // npad
    int *moves;                       // [0] = count, then (dst, src) pairs, per panel
    Rec32 *rec32;
    Rec64 *rec64;
    MfmaTile *tiles;                  // Mpad / 16 tiles (thin-plate only)
    MfmaTileH *tiles16;               // the fp16 form of the same tiles
    DevModel *model;
    double *ns;                       // null-space solver state (fd_nullspace.hip): ns_doubles(M) doubles
    int *host_status;                 // the context's page-locked status word as the device sees it (or null): the packing code
                                      // posts terminationtype there itself, so a one-launch build needs no status kernel behind it
};

// compute units of the current device (hipDeviceProp_t::multiProcessorCount: 256 on MI355X), looked up once per device
inline unsigned device_cus()
{
    static unsigned cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256u; }
    if (dev >= 0 && dev < 64 && cached[dev]) return cached[dev];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
    if (dev >= 0 && dev < 64) cached[dev] = (unsigned)n;
    return (unsigned)n;
}

// Caller-owned device arrays of control points, one pair per model of a batch (kernel argument).
struct PointSrc {
    const float *rest[kMaxBatch];
    const float *delta[kMaxBatch];
};

// Dimensions and parameters shared by all models of a launch chain + where their slots are.
struct BuildBuffers {
    int M, T, n, npad, lda, ncols;    // A is lda x ncols column-major; cols npad.. hold the RHS
    int kind, term;
    double lambda;
    double gauss_R, qnn_q, qnn_z;
    int Mpad;
    const BatchSlot *d_slots;         // device table, nbatch entries
    int nbatch;
    // Panels grouped under one deep trailing update (fd_build.hip group_at): pays when the
    // trailing updates are HBM-bound, i.e. for batches; a lone system is launch-bound and stays
    // ungrouped.  The factorisation's layout depends on it, so fd_set_deltas must replay it.
    int group_panels;
    // Symmetric definite path (fd_nullspace.hip): the polynomial constraints are eliminated with
    // Householder reflectors and the projected kernel block, order M - T, is Cholesky-factorised
    // -- no pivot search, so the panel is no longer one workgroup's serial chain.
    int small;                        // FD_SOLVER_ONE_WORKGROUP where k_build_small applies (small_applicable): it runs
    int reg;                          // the register-resident one-launch build (fd_build_reg.hip) where it applies: M <= 256 on the definite path
    // ... with its parallel front end (k_reg_front1 / k_reg_front2 over all CUs, then the factorisation in one workgroup per model):
    // shorter alone; 0 keeps the whole build in its one workgroup -- what a pipeline wants whose evaluation launches hold most CUs
    // (fd_batch_set_eval_cus below the device's count: the builds then stay on the CUs left to them)
    int reg_front;
    int spd;
    // QNN model, order <= 1024: the LU of its kernel block WITHOUT pivot search (fd_build.hip k_lu_panel_np); a multiplier
    // above kMaxMultiplier or a pivot below the threshold ends the build with -4 and the host repeats it with the pivoted LU.
    int nopivot;
    // Multilayer Gaussian model (FD_KERNEL_GAUSSIAN_ML, fd_nullspace.hip launch_build_ml): number of
    // layers, 0 for every other kind.  `kind` is then FD_KERNEL_GAUSSIAN (what the assembly evaluates).
    int ml_layers;
};

hipError_t launch_prepare(const BuildBuffers &b, hipStream_t stream, const PointSrc *src);
hipError_t launch_build(const BuildBuffers &b, hipStream_t stream, hipEvent_t ev_mid);
hipError_t launch_resolve(const BuildBuffers &b, hipStream_t stream, const PointSrc *src);
hipError_t launch_pack(const BuildBuffers &b, hipStream_t stream);
hipError_t launch_pack_from_weights(const BuildBuffers &b, hipStream_t stream, int layers = 0);
// pieces of the LU pipeline the null-space path reuses: the kernel block alone (order M, identity
// padding to npad_a) and back-substitution with the upper triangle over rows [0, rows)
hipError_t launch_assemble_block(const BuildBuffers &b, hipStream_t stream, int npad_a, int radii_off = 0);
// k_pack over `records` centres whose weights are already in W (mode 1: imported model, status from
// the values alone; mode 2: built here, the factorisation's flags count too)
hipError_t launch_pack_records(const BuildBuffers &b, hipStream_t stream, int records, int kind, int mode, int layers);
hipError_t launch_backsub_rows(const BuildBuffers &b, hipStream_t stream, int rows);
hipError_t launch_prepare_rhs(const BuildBuffers &b, hipStream_t stream, const PointSrc *src);
hipError_t launch_backsub_update(const BuildBuffers &b, hipStream_t stream, int row_lo, int w);
// the QNN model (fd_nullspace.hip launch_build_qnn) takes the LU apart: radii, then the pivoted
// factorisation + back-substitution of whatever has been assembled, full build or right-hand sides only
hipError_t launch_qnn_radii(const BuildBuffers &b, hipStream_t stream);
hipError_t launch_lu_factor_solve(const BuildBuffers &b, hipStream_t stream);
hipError_t launch_lu_factor(const BuildBuffers &b, hipStream_t stream);      // ... the factorisation alone: no back-substitution
hipError_t launch_lu_resolve_core(const BuildBuffers &b, hipStream_t stream);

// ---- null-space Cholesky build (fd_nullspace.hip) -----------------------------------
// Which (kernel, term, lambda) make the projected block positive definite; M large enough to project.
bool spd_applicable(int kind, int term, double lambda, int M);
// ... and small enough for FD_SOLVER_ONE_WORKGROUP's k_build_small (T polynomial columns); beyond it that choice is the launch chain
bool small_applicable(int M, int T);
static inline size_t ns_doubles(int M) { return (size_t)12 * (size_t)M + 64 + (size_t)(M / 32 + 2) * 66 * 32; }
hipError_t launch_build_spd(const BuildBuffers &b, hipStream_t stream, hipEvent_t ev_mid);
hipError_t launch_resolve_spd(const BuildBuffers &b, hipStream_t stream, const PointSrc *src);
// ---- register-resident one-launch build (fd_build_reg.hip): the definite path for rigs of up to 256 control points
bool reg_applicable(int kind, int term, double lambda, int M);
// the WHOLE build in one launch, control table included (src == nullptr: the contexts' own copies of the control points)
hipError_t launch_build_reg(const BuildBuffers &b, hipStream_t stream, const PointSrc *src, hipEvent_t ev_mid);
hipError_t launch_build_reg_shared(const BuildBuffers &b, hipStream_t stream, const PointSrc *src, hipEvent_t ev_mid, double *fac);
size_t reg_factor_doubles();
hipError_t reg_build_init();          // once per device, outside stream capture
constexpr int kMaxLayers = 8;
hipError_t launch_build_ml(const BuildBuffers &b, hipStream_t stream, hipEvent_t ev_mid);
// ---- a shot of multilayer models from one factorisation per layer (fd_batch_set_shared_factor; fd_build_ml_shared.hip)
// The L layer matrices are factorised once, side by side, in scratch slots of the batch (ml_shared_scratch_bytes; slot l is
// layer l's A, solver state and DevModel on context 0's centres), and k_ml_solve_shared takes every frame's right-hand sides
// through them in one launch.  launch_build_ml_shared is everything after k_prepare, as launch_build_ml is.
bool ml_shared_applies(int M, int layers, int frames);      // sizes the path takes; fewer frames than ml_shared_min_frames: no
int ml_shared_min_frames();
const char *ml_shared_kernel_name(int M, int layers, int frames);
hipError_t ml_shared_init();                                // once per device, outside stream capture
size_t ml_shared_scratch_bytes(const BuildBuffers &b);
const BatchSlot *ml_shared_slots(void *scratch);            // the scratch slot table, b.ml_layers entries
hipError_t launch_build_ml_shared(const BuildBuffers &b, hipStream_t stream, void *scratch);
// where fd_nullspace.hip keeps what the solve reads of the solver state (BatchSlot::ns), in doubles: tau, R and the
// multilayer polynomial inside the small block at 12 M; the diagonal blocks from `ld` past 12 M on, `ld_stride` apart,
// inverse(L11) at `ld_inv` inside each
struct MlSharedLayout { int tau, R, aff, ld, ld_stride, ld_inv; };
hipError_t launch_ml_shared_init(const BuildBuffers &b, hipStream_t stream, void *scratch);
hipError_t launch_ml_solve_shared(const BuildBuffers &b, hipStream_t stream, void *scratch, const MlSharedLayout &at);
// ---- a shot of QNN models from one LU of the rest rig's kernel block (fd_batch_set_shared_lu; fd_build_qnn_shared.hip)
// Radii per frame as ever; reflectors, kernel block and its LU without pivot search once, in a scratch slot of the batch
// (qnn_shared_scratch_bytes: its own A, solver state, DevModel, move lists, inverted diagonal blocks, on context 0's centres and
// radii); k_qnn_solve_shared takes every frame's right-hand sides through it in one launch.  launch_build_qnn_shared
// (fd_nullspace.hip) is everything after k_prepare, as launch_build_qnn is; b.nopivot must be set.
bool qnn_shared_applies(int M, int frames);                 // sizes the path takes; fewer frames than qnn_shared_min_frames: no
int qnn_shared_min_frames();
const char *qnn_shared_kernel_name(int M, int frames);
hipError_t qnn_shared_init();                               // once per device, outside stream capture
size_t qnn_shared_scratch_bytes(const BuildBuffers &b);
const BatchSlot *qnn_shared_slot(void *scratch);            // the scratch slot table, one entry
// fill_slot: the slot's table entry and status words have to be written first (k_qnn_shared_init); false when the batch's last
// shared build went out whole on this scratch and these contexts' buffers -- its solve kernel left the slot ready
hipError_t launch_build_qnn_shared(const BuildBuffers &b, hipStream_t stream, void *scratch, bool fill_slot);
hipError_t launch_qnn_shared_init(const BuildBuffers &b, hipStream_t stream, void *scratch);
hipError_t launch_qnn_solve_shared(const BuildBuffers &b, hipStream_t stream, void *scratch, const MlSharedLayout &at);
// FD_KERNEL_GAUSSIAN_QNN, the SOP's model = 0: least-squares polynomial first, then the pivoted LU
// of the (non-symmetric) kernel block on what is left
hipError_t launch_build_qnn(const BuildBuffers &b, hipStream_t stream, hipEvent_t ev_mid);
hipError_t launch_resolve_qnn(const BuildBuffers &b, hipStream_t stream, const PointSrc *src);

// ---- evaluation (fd_eval.hip) --------------------------------------------------
struct DeformArgs {
    int64_t N;
    const float *P_in; float *P_out;
    const float *dist2; float *falloff_out;
    const float *tu, *tv, *nrm;
    float radius2, falloffrate;
    int M, Mpad, kind;
    const Rec32 *rec32; const Rec64 *rec64;
    const MfmaTile *tiles;
    const MfmaTileH *tiles16;
    const DevModel *model;
    int precision, variant;
    int layers;            // multilayer Gaussian model: records are centre-major, `layers` per centre; 0 otherwise
    int delta_out;         // FD_OUTPUT_DISPLACEMENT: P_out receives the displacement (the addend of :438), not P + displacement
};
hipError_t launch_deform(const DeformArgs &a, hipStream_t stream);
// the deformation's Jacobian and the vectors it carries (fd_vectors.hip, fd_deform_vectors*): reads P_in, dist2, the
// projection frames and the model of `a`; writes neither P_out nor falloff_out.  Each output may alias its own input.
struct VectorArgs {
    const float *N, *tu, *tv;
    float *N_out, *tu_out, *tv_out;
    float *jacobian;      // N x 9, row-major A
};
hipError_t launch_vectors(const DeformArgs &a, const VectorArgs &v, hipStream_t stream);
// the inverse of the deformation (fd_invert.hip, fd_invert*): `a` names the mesh attributes and the model as for the
// deformation, P_in = the deformed points y, P_out = the rest-space points x (may alias P_in); falloff_out, precision, variant
// and delta_out are not read: the iteration is fp64 and takes positions to positions.
constexpr int kInvertDefaultIter = 20, kInvertMaxIter = 64;
struct InvertArgs {
    int max_iter;          // <= 0: kInvertDefaultIter; capped at kInvertMaxIter
    double tol;            // <= 0: per vertex 2^-25 max(|y|_inf, 1 / norm32[3])
    float *residual_out;   // N or null
    int *iters_out;        // N or null
};
hipError_t launch_invert(const DeformArgs &a, const InvertArgs &v, hipStream_t stream);
// the adjoint of the deformation (fd_adjoint.hip, fd_deform_adjoint*): `a` names the mesh attributes and the model as for the
// deformation (P_out, falloff_out, precision, variant and delta_out are not read: everything is fp64); G is the cotangent at the
// deformed vertices (N x 3), grad_W the (M + 4) x 3 result in W's layout, T the polynomial rows the term has (the others
// are written as 0.0), partial a scratch of adjoint_groups(N) * (M + 4) * 3 doubles.  Two launches; N = 0 writes zeros.
struct AdjointArgs {
    const float *G;
    double *grad_W;
    double *partial;
    int T;
};
int adjoint_groups(int64_t N);        // workgroups along the vertices: a function of N alone
hipError_t launch_adjoint(const DeformArgs &a, const AdjointArgs &g, hipStream_t stream);
// the adjoint in the vertex positions (fd_adjoint_points.hip, fd_deform_adjoint_points*): `a` as for the adjoint; G is the
// cotangent at the deformed vertices (N x 3), grad_P the N x 3 result A^T g, grad_f the N values g . Pi d(x) or null.  One
// launch, no scratch; N = 0 launches nothing.
struct AdjointPointsArgs {
    const float *G;
    double *grad_P;
    double *grad_f;
};
hipError_t launch_adjoint_points(const DeformArgs &a, const AdjointPointsArgs &g, hipStream_t stream);
// the adjoint for the F cotangents of a shot (fd_adjoint_shot.hip, fd_deform_adjoint_shot*): `a` as for the adjoint; G is
// F x N x 3 frame-major, grad_W F x (M + 4) x 3, T as above, partial a scratch of adjoint_shot_partial_doubles(N, M) doubles
// that the groups of 32 frames use one after the other.  Two launches per group; N = 0 writes zeros.
struct AdjointShotArgs {
    const float *G;
    double *grad_W;
    double *partial;
    int F, T;
};
int adjoint_shot_ranges(int64_t N, int C);    // workgroups along the vertices: a function of N and C alone, not of F
size_t adjoint_shot_partial_doubles(int64_t N, int C);
hipError_t launch_adjoint_shot(const DeformArgs &a, const AdjointShotArgs &g, hipStream_t stream);
// the Gram operator of the deformation (fd_gram.hip, fd_deform_gram*): `a` as for the adjoint; omega the per-vertex weights
// (N, or null for 1), H the nq x (M + 4) x (M + 4) result (nq = 6 with projection frames, else 1), T as above, partial a
// scratch of gram_partial_doubles(N, M, nq) doubles.  Two launches; N = 0 writes zeros.
struct GramArgs {
    const float *omega;
    double *H;
    double *partial;
    int T;
};
int gram_ranges(int64_t N, int C);    // workgroups along the vertices: a function of N and C alone
size_t gram_partial_doubles(int64_t N, int C, int nq);
hipError_t launch_gram(const DeformArgs &a, const GramArgs &g, hipStream_t stream);
// the deformer baked per vertex (fd_bake.hip, fd_deform_bake* and fd_deform_bake_grad*): `a` as for the adjoint (a.M the records C); S the (C + 4) x M
// solve operator on the device, M its columns (the control points), T as above, scratch bake_scratch_doubles(C, M) doubles; B
// and B32 the N x M results, either may be null.  launch_bake_pack is the only reader of S and fills the scratch; launch_bake
// reads the scratch and the mesh of `a` (one launch; N = 0 launches nothing), so one pack serves any number of vertex ranges.
// comps = 3 is the gradient (fd_deform_bake_grad*): B and B32 are then G and G32, N x 3 x M, the scratch is laid out for the
// gradient launch's narrower panels, and launch_bake launches that kernel.  comps is 1 or 3.
struct BakeArgs {
    const double *S;
    int M, T;
    double *scratch;
    double *B;
    float *B32;
    int comps;
};
size_t bake_scratch_doubles(int C, int M, int comps);
// vertices of a chunk of the host call: a multiple of the launch's vertex group whose block of comps x M doubles (b64) and
// floats (b32) per vertex stays within the operators' scratch bound (one group at least)
int64_t bake_chunk_vertices(int M, int comps, bool b64, bool b32);
hipError_t launch_bake_pack(const DeformArgs &a, const BakeArgs &g, hipStream_t stream);
hipError_t launch_bake(const DeformArgs &a, const BakeArgs &g, hipStream_t stream);
hipError_t launch_deform_batch(const DeformArgs *a, int n, hipStream_t stream);
// frames that share the mesh and the rest rig (fd_eval.hip, k_deform32_tps_shared): phi once per
// (vertex, centre), the 3 F-wide weight contraction on the matrix pipe
struct SharedDeformArgs {
    int64_t N;
    const float *P_in;                    // the one mesh
    const float *dist2;
    const float *tu, *tv, *nrm;
    float radius2, falloffrate;
    int Mpad, nF;
    int kind;                             // FD_KERNEL_THIN_PLATE, or a Gaussian kind (FD_KERNEL_GAUSSIAN / _QNN records)
    const MfmaTileH *ctiles;              // centre tiles of the shared rest rig (thin-plate; the Gaussian kinds read rec32[0])
    const Rec32 *rec32[kMaxBatch];        // per frame: the solved model's records (weights)
    const DevModel *model[kMaxBatch];
    float *P_out[kMaxBatch];
    float *const *falloff_out;            // nF entries or nullptr
    void *wtiles, *frames;                // scratch of SharedPlan::wtile_bytes / frame_bytes
    hipEvent_t packed_ev;                 // recorded once the pack kernel has read the models (may be null): from then on the
                                          // launch reads nothing of the contexts -- their next build may start
    int mode;                             // 0: pack kernel + evaluation; 1: pack kernel only (fd_batch_prepare_shared);
                                          // 2: evaluation only, on a scratch set packed earlier
    int delta_out;                        // FD_OUTPUT_DISPLACEMENT (see DeformArgs)
    int max_wgs;                          // CUs the launch may occupy (one persistent workgroup each); 0 or >= 256: all of them
    // pack kernel only: every model's centres (fp64, M x 3) are compared with model 0's -- "one rest rig" checked by content --
    // and 1 + the index of a model that differs is posted to *mismatch (device address of a page-locked word; may be null)
    const double *centres[kMaxBatch];
    int M;
    int *mismatch;
};
// (scratch sizes, the kernel's name and where its pack kernel leaves what in the scratch: shared_plan, fd_shared_plan.h)
hipError_t launch_deform_shared(const SharedDeformArgs &a, hipStream_t stream);
// What the arguments of the four shot vector launches have in common (fd_vectors_shot.h fills the kernels' arguments from it):
// the mesh, the vectors to carry and the per-frame outputs.
struct SharedVectorCommon {
    int64_t N;
    const float *P_in, *dist2, *tu, *tv, *nrm;
    float radius2, falloffrate;
    int nF;
    const float *vN, *vtu, *vtv;
    float *N_out[kMaxBatch], *tu_out[kMaxBatch], *tv_out[kMaxBatch], *jacobian[kMaxBatch];
    int max_wgs;
};
// The Jacobian and the vectors it carries for every frame of a shared-rig evaluation (fd_vectors_shared.hip): reads the
// scratch set launch_deform_shared packed (wtiles, frames), the mesh and the vectors; nothing of the contexts.
struct SharedVectorArgs : SharedVectorCommon {
    int Mpad, kind;
    const void *wtiles, *frames;
};
hipError_t launch_vectors_shared(const SharedVectorArgs &a, hipStream_t stream);
const char *shared_vectors_kernel_name(int Mpad, int nF, int kind);
// What the arguments of the three staged shot evaluations have in common (fd_eval_shared64.hip, fd_eval_shared_ml.hip,
// fd_eval_shared_ml64.hip; fd_shot_launch.h fills the kernels' arguments from it): the mesh, the frames' models and outputs, the
// scratch the pack kernel fills and what the launch reports.
struct SharedEvalCommon {
    int64_t N;
    const float *P_in, *dist2, *tu, *tv, *nrm;
    float radius2, falloffrate;
    int nF;
    const DevModel *model[kMaxBatch];
    float *P_out[kMaxBatch];
    float *const *falloff_out;            // nF entries or nullptr
    void *scratch;
    hipEvent_t packed_ev;                 // as SharedDeformArgs::packed_ev
    int delta_out, max_wgs;
    int *mismatch;                        // as SharedDeformArgs::mismatch
};
// Every frame of a shared-rig batch in fp64 by one matrix-pipe launch (fd_eval_shared64.hip, fd_batch_deform_shared_fp64_dev):
// a pack kernel copies what the launch needs of the models into `scratch` (shared64_scratch_bytes; packed_ev is recorded
// behind it, may be null), the evaluation reads only that copy.
struct Shared64Args : SharedEvalCommon {
    int M, Mpad, kind;                    // kind: any but the multilayer model's
    const Rec64 *rec64[kMaxBatch];
    const double *centres[kMaxBatch];     // compared with entry 0 by content unless equal to it by address; a frame that differs is passed through
};
hipError_t launch_deform_shared64(const Shared64Args &a, hipStream_t stream);
size_t shared64_scratch_bytes(int Mpad, int nF);
const char *shared64_kernel_name(int Mpad, int nF, int kind);
// The Jacobian and the vectors it carries for every frame of that batch, in fp64 by one matrix-pipe launch
// (fd_vectors_shared64.hip, fd_batch_deform_vectors_shared_fp64_dev): reads the scratch launch_deform_shared64's pack kernel
// wrote for the same Mpad and nF, the mesh and the vectors; nothing of the contexts.
struct SharedVector64Args : SharedVectorCommon {
    int Mpad, kind;
    const void *scratch;
};
hipError_t launch_vectors_shared64(const SharedVector64Args &a, hipStream_t stream);
const char *shared_vectors64_kernel_name(int Mpad, int nF, int kind);      // "" below shared_vectors64_min_frames too
int shared_vectors64_min_frames(int kind);                                  // fewer frames: the per-context launches are faster
// The adjoint in the vertex positions summed over the frames of that batch, grad_P = sum_f A_f^T g_f, in fp64 by one
// matrix-pipe launch (fd_adjoint_points_shot.hip, fd_batch_deform_adjoint_points_shared_dev): a pack kernel copies what the
// launch needs of the models into `scratch` (shared_adjoint_points_scratch_bytes, a scratch of this call's own; packed_ev is
// recorded behind it), the main launch reads only that copy.  P_out, falloff_out and delta_out are not looked at.
struct SharedAdjointPointsArgs : SharedEvalCommon {
    int M, Mpad, kind;                    // kind: any but the multilayer model's
    const Rec64 *rec64[kMaxBatch];
    const double *centres[kMaxBatch];     // as Shared64Args::centres; a frame that differs contributes g_f alone
    const float *G;                       // nF x N x 3, frame-major
    double *grad_P;                       // N x 3
};
hipError_t launch_adjoint_points_shared(const SharedAdjointPointsArgs &a, hipStream_t stream);
size_t shared_adjoint_points_scratch_bytes(int Mpad, int nF);
const char *shared_adjoint_points_kernel_name(int Mpad, int nF, int kind);  // "" below shared_adjoint_points_min_frames too
int shared_adjoint_points_min_frames(int kind);                             // fewer frames: the per-context launches are faster
// sum[i] += term[i], i < n: the per-context route of that call adds the one-frame results in frame order with it
hipError_t launch_adjoint_points_add(double *sum, const double *term, int64_t n, hipStream_t stream);
// Every frame of a shared-rig batch of MULTILAYER models by one matrix-pipe launch (fd_eval_shared_ml.hip,
// fd_batch_deform_shared_ml_dev): a pack kernel copies what the launch needs of the models into `scratch`
// (shared_ml_scratch_bytes; packed_ev is recorded behind it, may be null), the evaluation reads only that copy.
struct SharedMlArgs : SharedEvalCommon {
    int M, layers;                        // centres, layers per centre (1..kMaxLayers); with nF: shared_ml_applies
    const Rec32 *rec32[kMaxBatch];        // per frame: M x layers records, centre-major (k_pack)
    int check_rig;                        // compare every frame's records {c', scale} with frame 0's; a frame that differs is passed through
};
hipError_t launch_deform_shared_ml(const SharedMlArgs &a, hipStream_t stream);
bool shared_ml_applies(int M, int layers, int nF);      // sizes the launch takes; fewer frames than shared_ml_min_frames: no
int shared_ml_min_frames();
size_t shared_ml_scratch_bytes(int M, int layers, int nF);
const char *shared_ml_kernel_name(int M, int layers, int nF);
// Every frame of a shared-rig batch of MULTILAYER models in fp64 by one matrix-pipe launch (fd_eval_shared_ml64.hip,
// fd_batch_deform_shared_ml_fp64_dev): a pack kernel copies what the launch needs of the models into `scratch`
// (shared_ml64_scratch_bytes; packed_ev is recorded behind it, may be null), the evaluation reads only that copy.
struct SharedMl64Args : SharedEvalCommon {
    int M, layers;                        // centres, layers per centre (1..kMaxLayers); with nF: shared_ml64_applies
    const Rec64 *rec64[kMaxBatch];        // per frame: M x layers records, centre-major (k_pack)
    int check_rig;                        // compare every frame's records {c, s} with frame 0's; a frame that differs is passed through
};
hipError_t launch_deform_shared_ml64(const SharedMl64Args &a, hipStream_t stream);
bool shared_ml64_applies(int M, int layers, int nF);    // sizes the launch takes; fewer frames than shared_ml64_min_frames: no
int shared_ml64_min_frames();
size_t shared_ml64_scratch_bytes(int M, int layers, int nF);
const char *shared_ml64_kernel_name(int M, int layers, int nF);
// The Jacobian and the vectors it carries for every frame of that batch, in fp64 by one matrix-pipe launch
// (fd_vectors_shared_ml64.hip, fd_batch_deform_vectors_shared_ml_fp64_dev): reads the scratch launch_deform_shared_ml64's
// pack kernel wrote for the same M, layers and nF, the mesh and the vectors; nothing of the contexts.
struct SharedVectorMl64Args : SharedVectorCommon {
    int M, layers;
    const void *scratch;
};
hipError_t launch_vectors_shared_ml64(const SharedVectorMl64Args &a, hipStream_t stream);
const char *shared_vectors_ml64_kernel_name(int M, int layers, int nF);    // "" below shared_vectors_ml64_min_frames too
int shared_vectors_ml64_min_frames(int layers);                             // fewer frames: the per-context launches are faster
// The Jacobian and the vectors it carries for every frame of a shared-rig batch of MULTILAYER models, in fp32 by one
// matrix-pipe launch (fd_vectors_shared_ml.hip, fd_batch_deform_vectors_shared_ml_dev): reads the scratch
// launch_deform_shared_ml's pack kernel wrote for the same M, layers and nF, the mesh and the vectors; nothing of the contexts.
struct SharedVectorMlArgs : SharedVectorCommon {
    int M, layers;
    const void *scratch;
};
hipError_t launch_vectors_shared_ml(const SharedVectorMlArgs &a, hipStream_t stream);
const char *shared_vectors_ml_kernel_name(int M, int layers, int nF);      // "" below shared_vectors_ml_min_frames too
int shared_vectors_ml_min_frames(int layers);                               // fewer frames: the per-context launches are faster
// island mask (fd_capture.hip): nearest mesh point per rig point + max_edges breadth-first rings
hipError_t launch_capture_islands(const float *d_P, int64_t N, const int64_t *d_offsets, const int *d_neighbours,
                                  const float *d_rig, int M, int max_edges, unsigned char *d_mask, hipStream_t stream);
// dist2 producer (fd_capture.hip): all pointers are device pointers, d_mask may be null
hipError_t launch_capture_dist2(const float *d_P, int64_t N, const unsigned char *d_mask, const float *d_tri, int T,
                                float radius2, int dofalloff, float *d_dist2, hipStream_t stream);
const char *deform_kernel_name(int kind, int precision, int variant);

}  // namespace fd
