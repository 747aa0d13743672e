/*
 * facedeform_hip.h -- C ABI of the MI355X (gfx950) RBF deformation engine.
 *
 * This is the drop-in boundary for the hot path of symek/facedeform's
 * SOP_FaceDeform::cookMySop.  Each entry point names the reference interface
 * it replaces (paths relative to the reference tree).  Plain C: no C++ types,
 * no torch types, no exceptions cross it.  All functions return 0 (FD_OK) on
 * success and a negative FD_E_* code on failure unless stated otherwise;
 * fd_last_error() gives the text.
 *
 * Threading: an fd_ctx is not thread-safe; distinct contexts are independent
 * and re-entrant (different SOP instances may cook concurrently).
 *
 * Memory: "host" entry points take caller-owned host pointers and copy.
 * "_dev" entry points take device pointers valid on the context's device and
 * enqueue on the context's stream without synchronising.
 */
#ifndef FACEDEFORM_HIP_H
#define FACEDEFORM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_ABI_VERSION 9   /* 3: fd_config.solver, FD_KERNEL_GAUSSIAN_ML, fd_model_centres; 4: fd_mesh_capture, capture inputs at the end of fdsop_geo; 5: fd_batch_wait_consumed, fd_batch_prepare_shared; 6: fd_batch_set_eval_cus; 7: fd_batch_cook_group, FD_SOLVER_REGISTER / FD_SOLVER_CHAIN; 8: fd_report grows by the fp32 estimate (callers built against 7 pass a shorter struct: rebuild), fd_set_eval_precision, fd_fp32_holds, fd_report.reserved becomes solver_used; 9: fd_shared_kernel_name, fd_set_output, fd_batch_set_shared_factor */

/* ---- error codes ---------------------------------------------------------- */
enum {
    FD_OK = 0,
    FD_E_INVALID = -1,    /* bad argument / call order                           */
    FD_E_NOMEM = -2,      /* host or device allocation failed                    */
    FD_E_DEVICE = -3,     /* HIP runtime error (text in fd_last_error)           */
    FD_E_SINGULAR = -4,   /* solver failure; report.terminationtype = -4         */
    FD_E_DUPLICATE = -5,  /* coincident control points; terminationtype = -5     */
    FD_E_NOT_BUILT = -6,  /* fd_deform before a successful fd_build              */
    FD_E_NO_DEVICE = -7   /* no usable gfx950 device / kernels cannot load       */
};

/* ---- radial kernels (d2 = squared distance to centre j) --------------------
 * The reference exposes ALGLIB's two Gaussian models through the `model` parm
 * (src/SOP_FaceDeform.cpp:48-53,342-349).  The engine solves the dense system
 * north_star describes; kinds 0/1 are the reference's family, 2..4 BASELINE's.
 *   FD_KERNEL_GAUSSIAN      exp(-d2/R^2)            params {R [, lambda]}
 *       (model=1 "Multilayer" collapsed to one layer: R = radius, lambda = lambda)
 *   FD_KERNEL_GAUSSIAN_QNN  exp(-d2/R_j^2), R_j = min(q*nn_j, z*median_k(q*nn_k))
 *       (model=0 "QNN": q = qcoef, z = zcoef)      params {q, z [, lambda]}
 *       Built in ALGLIB's order, like FD_KERNEL_GAUSSIAN_ML below: the term's polynomial is a
 *       least-squares fit to the deltas, removed first; then (Phi + lambda I) w = f - P a (Phi is
 *       not symmetric with per-centre radii: pivoted LU).  The median is element M/2 of the
 *       sorted radii.
 *   FD_KERNEL_THIN_PLATE    r^2 ln r                params {[lambda]}
 *   FD_KERNEL_BIHARMONIC    -r                      params {[lambda]}
 *   FD_KERNEL_CUBIC         r^3                     params {[lambda]}
 * lambda is added to the diagonal of the kernel block (smoothing); default 0.
 *   FD_KERNEL_GAUSSIAN_ML   model=1 "Multilayer" as rbfsetalgomultilayer(model, radius, layers, lambda)
 *       (src/SOP_FaceDeform.cpp:346-348) lays it out, in dense form   params {R [, layers [, lambda]]}
 *       -- the term's polynomial is fitted to the deltas first, by least squares, and removed
 *       (ALGLIB's order; the kinds above solve it together with the weights); then layer
 *       l = 0 .. layers-1 fits what is left with exp(-d2/R_l^2), R_l = R / 2^l, on every centre:
 *       (Phi_l + lambda I) w_l = r_l,  r_{l+1} = r_l - Phi_l w_l.  The solved model is M * layers
 *       Gaussian records (fd_model_centres).  1 <= layers <= 8; defaults 4 and 0.1 as the SOP's.
 *       Not bit-parity with ALGLIB's truncated-Gaussian LSQR fit (absent here): parity with this
 *       dense statement, pinned by tests/golden/ml_golden.npz. */
enum {
    FD_KERNEL_GAUSSIAN = 0,
    FD_KERNEL_GAUSSIAN_QNN = 1,
    FD_KERNEL_THIN_PLATE = 2,
    FD_KERNEL_BIHARMONIC = 3,
    FD_KERNEL_CUBIC = 4,
    FD_KERNEL_GAUSSIAN_ML = 5
};

/* Same integers as ALGLIB_TERM_LINEAR/CONST/ZERO, src/SOP_FaceDeform.hpp:16-18. */
enum { FD_TERM_LINEAR = 0, FD_TERM_CONST = 1, FD_TERM_ZERO = 2 };

/* Evaluation arithmetic.  The solve is always fp64.
 * FP32, thin-plate with 49 or more centres (the default kernel of BASELINE's configurations,
 *   k_deform32_tps_mfma): the squared distances come from the matrix pipe as
 *   |x|^2 - 2 x.c + |c|^2 on operands split into two fp16 pieces (22 significant bits, about
 *   1.4e-6 absolute in normalised coordinates); logarithm, weights and accumulation are fp32,
 *   partial sums folded into a second fp32 level every <= 96 terms.  No fp64 anywhere.
 * FP32, every other kernel and small rigs (k_deform32): fp32 coordinate differences and kernel,
 *   partial sums folded into fp64 accumulators every 64 centres.
 * FP64: everything in fp64 (ill-conditioned weights). */
enum { FD_EVAL_FP32 = 0, FD_EVAL_FP64 = 1 };

/* Direct solver of the dense system.  AUTO: where the kernel is conditionally positive definite
 * of the order its polynomial term covers (thin-plate and cubic with the linear term, biharmonic
 * with a constant or linear term, the fixed-radius Gaussian with any term; lambda >= 0, M >= 16)
 * the polynomial constraints are eliminated with Householder reflectors and the projected kernel
 * block is Cholesky-factorised -- no pivot search; up to 256 control points that whole build is ONE
 * launch of one workgroup per model with the matrix in registers (FD_SOLVER_REGISTER names it; FD_SOLVER_CHAIN
 * keeps the launch chain at any size: same mathematics, weights equal to rounding, 1e-12);
 * everything else (QNN radii make Phi non-symmetric) goes through LU (the QNN model without the pivot
 * search where that is exact, see below).  LU forces the partially pivoted LU everywhere.  A
 * system on which the Cholesky loses definiteness to rounding (centres one fp32 step apart, a
 * fixed-radius Gaussian wider than the rig) is rebuilt with the LU before anything is reported,
 * and the context keeps the LU until its kernel, term or M change: nothing the LU accepts fails.
 * The rebuild happens where the status is first seen: in fd_build / fd_build_result /
 * fd_batch_build_result, or -- in a pipeline that enqueues builds and evaluations without collecting
 * results -- in the first fd_deform* / fd_batch_deform* call made after the build has executed
 * (every enqueued build posts its status to page-locked memory; every later call polls it without
 * waiting).  Evaluations enqueued BEFORE the status could be known pass the mesh through; from then
 * on the rig is evaluated correctly, or, if the LU fails too, fd_deform* returns FD_E_SINGULAR /
 * FD_E_DUPLICATE (sticky until the next fd_set_points / fd_set_deltas).  Both
 * are fp64 direct solves of the same system: their weights agree to rounding (~1e-12 relative
 * on the benchmark rigs), far inside the parity tolerance. */
/* ONE_WORKGROUP (thin-plate / Gaussian family as for AUTO's Cholesky path, while M minus the term's polynomial columns,
 * rounded up to a multiple of 32, is at most 512: up to 516 control points under the linear term, 513 under the constant
 * term, 512 without a term; a larger definite system takes the launch chain and reports FD_SOLVER_CHAIN, anything else
 * behaves as AUTO): everything after the assembly of K -- projection, Cholesky, substitution, packing -- in ONE
 * launch of ONE workgroup per model.  A single build is slower that way (0.37 against 0.25 ms at 256 control
 * points), but a batch of 32 costs what one does, as 32 workgroups on 32 CUs and nothing else on the device: the
 * choice for a pipeline that keeps evaluating on the other CUs while the next frames' models are solved (bench.py).
 * Same arithmetic within this choice for single and batched builds (bit-identical weights); against AUTO the
 * weights agree to rounding (1e-12 relative). */
/* QNN model (FD_KERNEL_GAUSSIAN_QNN, the SOP's default: rbfsetalgoqnn, src/SOP_FaceDeform.cpp:342-345), up to 1024 control
 * points, under AUTO: the LU of its kernel block runs WITHOUT pivot search -- with q <= 1 partial pivoting never interchanges
 * (profiles/r02_qnn_pivot_stats.txt) and the factors are bit-identical to the pivoted ones.  A multiplier above 4 or a pivot
 * below the threshold ends that build with -4 and the pivoted LU repeats it, through the same path as above (q = 2 rigs).
 * FD_SOLVER_LU_NOPIVOT is a value of fd_report.solver_used only, not a choice. */
enum { FD_SOLVER_AUTO = 0, FD_SOLVER_LU = 1, FD_SOLVER_ONE_WORKGROUP = 2, FD_SOLVER_REGISTER = 3, FD_SOLVER_CHAIN = 4, FD_SOLVER_LU_NOPIVOT = 5 };

typedef struct fd_ctx fd_ctx;

typedef struct fd_config {
    int struct_size;     /* = sizeof(fd_config); 0 is accepted as "version 1"   */
    int device;          /* HIP device ordinal; -1 = the calling thread's current */
    int eval_precision;  /* FD_EVAL_*                                            */
    int eval_variant;    /* 0 = auto; otherwise a kernel variant id (tuning/tests) */
    int solver;          /* FD_SOLVER_*                                           */
    int reserved[3];
} fd_config;

/* Replaces alglib::rbfreport as read at src/SOP_FaceDeform.cpp:365-373. */
typedef struct fd_report {
    int terminationtype; /* 1 ok; -5 coincident centres; -4 solver failure       */
    int iterationscount; /* unknowns eliminated by the direct solver (n when done) */
    int n;               /* order of the solved system (M + term columns)        */
    int solver_used;     /* FD_SOLVER_* the build actually ran (FD_SOLVER_LU after a fallback; FD_SOLVER_LU_NOPIVOT: QNN) */
    double pivot_ratio;  /* min|pivot| / max|pivot| of the LU (cheap rcond proxy) */
    float t_assemble_ms; /* device time: prepare + kernel-matrix assembly        */
    float t_solve_ms;    /* device time: factorisation + substitution + pack     */
    /* What the fp32 evaluation (FD_EVAL_FP32) can be trusted with for THIS model.  It adds up M terms w_j phi(d_j) whose
     * magnitudes sum to S = sum_j |w_j| max phi over the rig's extent (+ the polynomial); each carries a relative 2^-24,
     * so a displacement comes out with an absolute error of up to 2^-24 S whatever its own size; the kernels measure at
     * 0.3 .. 0.4 of that and fp32_error = 2^-25 S is what is reported.  The
     * reference (fp64 inside ALGLIB, src/SOP_FaceDeform.cpp:404-439) has no such floor.  fd_fp32_holds() turns these into
     * the decision fdsop_cook takes; 0 in all four for imported models (no control table to measure against). */
    double fp32_error;   /* ~ absolute error of an fp32-evaluated displacement, in position units        */
    double cancellation; /* S / max_i |delta_i|: how much larger the summed terms are than what they add up to */
    double delta_min;    /* smallest |delta_i| among the control points that move (|delta_i| >= 0.1 delta_max): a
                          * stationary or barely moving control point -- most of a face rig in most frames, the fringe of a
                          * localised deformation -- does not count */
    double delta_max;    /* largest                                                                       */
    double extent;       /* largest |rest_i|: the size of the positions the displacement is added to     */
} fd_report;

/* 1 when the fp32 evaluation of the reported model is expected to hold `tol` (the reference's 1e-5) of every
 * vertex's own displacement: fp32_error <= tol * delta_min / 2 (vertices between the moving control points move less than the
 * least of those; around a stationary one the field is zero to within the next term in fp32 too) + one fp32 ulp of the positions (both sides round P + d to
 * fp32, :438, which shelters errors below that).  0: evaluate this model with FD_EVAL_FP64 (fd_set_eval_precision).
 * Conservative where the displacement field has zeros between control points -- no estimate from M points sees those. */
int fd_fp32_holds(const fd_report *report, double tol);

/* ---- lifetime ---------------------------------------------------------------
 * fd_create replaces `alglib::rbfmodel model; alglib::rbfcreate(3, 3, model)`
 * (src/SOP_FaceDeform.cpp:332,335).  NULL on failure (no device, out of
 * memory); fd_last_error(NULL) then holds the reason. */
fd_ctx *fd_create(const fd_config *cfg);
void fd_destroy(fd_ctx *ctx);
const char *fd_last_error(const fd_ctx *ctx);
int fd_abi_version(void);

/* Launch everything on `hip_stream` (a hipStream_t) instead of the context's
 * own stream.  NULL restores the context's stream. */
int fd_set_stream(fd_ctx *ctx, void *hip_stream);

/* FD_EVAL_FP32 / FD_EVAL_FP64 for the evaluations from here on (fd_config.eval_precision is the initial value).  A built
 * model carries the records of both: no rebuild.  fdsop_cook switches per cook on fd_fp32_holds(). */
int fd_set_eval_precision(fd_ctx *ctx, int eval_precision);
/* What the evaluation calls write into P_out.  FD_OUTPUT_POSITION (default): P + d f, the reference's write-back
 * (src/SOP_FaceDeform.cpp:438).  FD_OUTPUT_DISPLACEMENT: the addend alone, d f -- the fp32 displacement after the tangent projection
 * and the fall-off (:415-437), BEFORE it is added to the position; gated vertices and frames without a built model, which the
 * reference leaves where they are, get 0.  P_in is still the evaluation point.  For callers that keep a delta attribute, and for
 * parity tests that hold the displacement itself to 1e-5 without the rounding of P + d in the way.  Takes effect with the next
 * fd_deform* call; a batch takes the setting of its first context (all of them must agree). */
enum { FD_OUTPUT_POSITION = 0, FD_OUTPUT_DISPLACEMENT = 1 };
int fd_set_output(fd_ctx *ctx, int what);

/* ---- model set-up -----------------------------------------------------------
 * fd_set_points replaces alglib::rbfsetpoints(model, xy) with the M x 6 table
 * split into its two halves (src/SOP_FaceDeform.cpp:268-287,336): rest_xyz and
 * delta_xyz are AoS M x 3 fp32; delta = float(deformP - restP) computed by the
 * caller in fp32 as the reference does (:278). */
int fd_set_points(fd_ctx *ctx, const float *rest_xyz, const float *delta_xyz, int M);
int fd_set_points_dev(fd_ctx *ctx, const float *d_rest_xyz, const float *d_delta_xyz, int M);

/* Replaces rbfsetalgoqnn / rbfsetalgomultilayer (src/SOP_FaceDeform.cpp:342-349). */
/* New deltas for rest points that have already been factorised: the animated-rig case, where
 * the rest rig (input 1) stands still and only the deformed rig (input 2) moves.  The reference
 * rebuilds its model on every cook (src/SOP_FaceDeform.cpp:331-363); the system matrix depends on
 * the rest points, kernel and term only, so after fd_set_deltas the next fd_build* carries just
 * the new right-hand sides through the stored factorisation (same kernels and operand order as
 * a full build: the weights are bit-identical to fd_set_points + fd_build with the same data).
 * Exception: where FD_SOLVER_AUTO takes the register-resident one-launch build (thin-plate, cubic, biharmonic, fixed-radius
 * Gaussian with a term that makes them definite, up to 256 control points) no factorisation is stored -- the matrix never leaves
 * the registers -- and the next fd_build* simply builds again (0.18 ms at M = 256, less than the stored-factor
 * path's launch chain); the weights are the same bits either way.  FD_SOLVER_CHAIN keeps and reuses the factorisation.
 * FD_E_NOT_BUILT when there is no factorisation to reuse (no build yet, or fd_set_points /
 * fd_set_kernel / fd_set_term / fd_import_model since); M must match; order <= 2048. */
int fd_set_deltas(fd_ctx *ctx, const float *delta_xyz, int M);
int fd_set_deltas_dev(fd_ctx *ctx, const float *d_delta_xyz, int M);
int fd_set_kernel(fd_ctx *ctx, int kind, const double *params, int nparams);

/* Replaces rbfsetlinterm / rbfsetconstterm / rbfsetzeroterm (:351-361). */
int fd_set_term(fd_ctx *ctx, int term);

/* fd_build replaces alglib::rbfbuildmodel(model, report) (:363-368): kernel
 * matrix assembly + dense solve on the device; synchronises; fills *report.
 * Returns FD_OK iff report->terminationtype == 1.
 * fd_build_async enqueues the same work and returns; fd_build_result waits and
 * reports.  A deform enqueued after a failed build passes P through unchanged; once the failure is
 * known to the host (no wait: see FD_SOLVER_AUTO) fd_deform* repairs it or returns its error code. */
int fd_build(fd_ctx *ctx, fd_report *report);
int fd_build_async(fd_ctx *ctx);
int fd_build_result(fd_ctx *ctx, fd_report *report);

/* ---- evaluation -------------------------------------------------------------
 * fd_deform replaces the whole loop body src/SOP_FaceDeform.cpp:404-439
 * (gate :405-410, rbfcalc :411-415, project_to_tangents :416-422 with
 * src/SOP_FaceDeform.hpp:28-41, fall-off :423-425, write-back :437-438).
 *   P_in / P_out   N x 3 AoS fp32; P_out may alias P_in
 *   dist2          N fp32 squared capture distance, or NULL (= 0 everywhere)
 *   falloff_out    N fp32 (the fd_falloff attribute), or NULL; vertices skipped
 *                  by the gate are not written (the attribute keeps its default)
 *   tu, tv, nrm    N x 3 fp32 tangentu / tangentv / N, all three or all NULL
 *   radius2        radius*radius (:402);  falloffrate  the exponent (:424)
 * Synchronises before returning. */
int fd_deform(fd_ctx *ctx, int64_t N, const float *P_in, float *P_out, const float *dist2,
              float *falloff_out, const float *tu, const float *tv, const float *nrm,
              float radius2, float falloffrate);

/* Same, device pointers, asynchronous on the context's stream. */
int fd_deform_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, float *d_P_out,
                  const float *d_dist2, float *d_falloff_out, const float *d_tu,
                  const float *d_tv, const float *d_nrm, float radius2, float falloffrate);

/* Same again, but launched on `hip_stream` (a hipStream_t) instead of the context's stream, so
 * that one stream can evaluate frame after frame while other streams build the next models.
 * Ordering is the caller's: make `hip_stream` wait for this context's build (an event recorded
 * on the context's stream after fd_build_async), and make the next fd_set_points / fd_build on
 * this context wait for the evaluation, which reads the model. */
int fd_deform_dev_stream(fd_ctx *ctx, void *hip_stream, int64_t N, const float *d_P_in, float *d_P_out,
                         const float *d_dist2, float *d_falloff_out, const float *d_tu,
                         const float *d_tv, const float *d_nrm, float radius2, float falloffrate);

/* ---- normals, tangents and the Jacobian of the deformation -------------------
 * At a vertex x that the gate lets through (!(dist2 > radius2), :408), the evaluation writes
 * P' = x + f . Pi . d(x):
 *   d   is the RBF field, including its polynomial term;
 *   Pi  = a1 a1^T + a2 a2^T is the tangent projection of project_to_tangents, built from the same
 *       normalised u, v, n.  It is the identity when no frames are given;
 *   f   is the fall-off.
 * dist2 and the frames are per-point attributes, so f and Pi are constant under the derivative.
 * The local Jacobian is therefore
 *   A = I + f . Pi . J(x),   J = dd/dx = sum_j w_j grad phi_j(x - c_j) + L
 * (L: the 3x3 linear-term block; 0 for CONST/ZERO terms).  The outputs follow from A:
 *   jacobian            A, row-major, 9 floats per vertex;
 *   tangentu, tangentv  t' = A t, not renormalised, so stretch shows;
 *   N                   n' = cof(A) n, rescaled to |n|.  cof(A) = det(A) A^-T, written with cofactors
 *                       and no division: exactly the normal of the deformed tangent plane,
 *                       cof(A)(u x v) = (A u) x (A v), and defined when A is singular.  If n = 0 or
 *                       cof(A) n = 0, n is written unchanged.
 * Gated vertices and a model that is not built (terminationtype != 1, fd_deform's pass-through):
 * every output is the input bit for bit, and A = I exactly.  A vertex with f = 0 also gets A = I exactly.
 * grad phi per kind, in the raw form of the table above (r = |x - c|):
 *   thin-plate   (x - c)(2 ln r + 1), 0 at r = 0;
 *   Gaussian, QNN and multilayer   -2 (x - c) / R_j^2 . phi, one record per layer for the multilayer model;
 *   cubic        3 r (x - c);
 *   biharmonic   -(x - c) / r, taken as 0 at r = 0: the cone -r has no gradient at its tip.
 * A is evaluated in the context's precision (fd_set_eval_precision) and stored as fp32.
 *
 * fd_vectors: what to transport.  N, tu, tv are N x 3 fp32, each with its *_out (both or neither);
 * an output may alias its own input.  jacobian: N x 9, or NULL.  The projection frames (tu, tv, nrm
 * of the call) are separate arguments: a caller may transport N without projecting, and may pass
 * the same arrays to both. */
typedef struct fd_vectors {
    int struct_size;                 /* = sizeof(fd_vectors); smaller is FD_E_INVALID          */
    const float *N;  float *N_out;   /* transported as normals (n' = cof(A) n, |n'| = |n|)     */
    const float *tu; float *tu_out;  /* transported as tangents (t' = A t)                     */
    const float *tv; float *tv_out;
    float *jacobian;                 /* N x 9 row-major A, or NULL                             */
} fd_vectors;

/* fd_deform plus the outputs of `vec`.  P_out and falloff_out are bit-identical to fd_deform's for the
 * same arguments, precision and fd_set_output setting; vec == NULL, or every pointer in it NULL, is
 * fd_deform.  Same error codes, build-status poll and repair as fd_deform.  Host arrays, synchronous. */
int fd_deform_vectors(fd_ctx *ctx, int64_t N, const float *P_in, float *P_out, const float *dist2,
                      float *falloff_out, const float *tu, const float *tv, const float *nrm,
                      float radius2, float falloffrate, const fd_vectors *vec);
/* Same, device pointers (those in `vec` too), asynchronous on the context's stream, like fd_deform_dev. */
int fd_deform_vectors_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, float *d_P_out, const float *d_dist2,
                          float *d_falloff_out, const float *d_tu, const float *d_tv, const float *d_nrm,
                          float radius2, float falloffrate, const fd_vectors *vec);

/* ---- the inverse of the deformation -------------------------------------------
 * Given a point y of the deformed mesh, fd_invert finds the rest-space point x with
 *   x + f . Pi . d(x) = y
 * (d, Pi, f as above).  Uses: pulling a corrective sculpt made on the posed mesh back to the rest pose, re-binding
 * data captured in a pose, round-tripping a cache.
 *
 * Vertex attributes.  dist2[i] and tu/tv/nrm[i] belong to vertex i, exactly as in fd_deform, so f_i and Pi_i are
 *   constants of vertex i's equation: the call solves F_i(x) = x + f_i Pi_i d(x) - y_i = 0, d the built model's field
 *   including its polynomial term.
 * Iteration.  x0 = y_i; while |F(x)|_2 > tol_i:  x <- x - A(x)^-1 F(x),  A = I + f_i Pi_i J(x) (fd_vectors' definition).
 *   The 3x3 solve uses cofactors and one division by det A.  Everything is fp64 whatever fd_set_eval_precision says: the
 *   fp32 positions widened, direct differences x - c_j in raw coordinates, phi and grad phi of the kind in fp64 from one
 *   shared transcendental.  No line search and no damping: the algorithm is fixed, so step counts can be compared with
 *   a reference.
 * Result.  X_out[i] is the converged x rounded once to fp32.  Status -1 or -2: the iterate with the smallest residual
 *   seen is written, y_i at worst; it is always finite.  -2 means a non-finite iterate (or residual) or det A == 0.
 *   For such a vertex residual_out is taken at the fp32 value that is written (one more evaluation, only in waves that
 *   hold such a vertex), so that it describes what the caller holds; rounding that value to fp32 changes nothing.
 * Pass-through.  X_out[i] = Y[i] bit for bit, iters = 0, residual = 0 for a gated vertex (dist2 > radius2) and for a model
 *   with terminationtype != 1.  With f = 0, step 0 already converges: F(y) = 0 exactly.
 * Determinism.  The same inputs give the same bits on every call; a vertex's result does not depend on N or on its
 *   place in the launch.
 * Aliasing.  X_out may alias Y; nothing else may.
 * Non-injective maps.  Where the forward map is not injective (folds; the tangent projection with det A near 0) the
 *   call returns *a* preimage when Newton finds one.  This is not an error.
 * Checks and errors.  The build-status poll and repair, FD_E_NOT_BUILT, the all-or-none rule for tu/tv/nrm and the ordering
 *   behind a batched build are fd_deform's.  FD_E_INVALID for a NULL context, NULL opts or a bad struct_size comes before
 *   any device work.  fd_set_output has no effect: the call takes positions and returns positions. */
typedef struct fd_invert_opts {
    int struct_size;      /* = sizeof(fd_invert_opts); smaller is FD_E_INVALID */
    int max_iter;         /* Newton steps allowed per vertex; <= 0: 20; capped at 64 */
    double tol;           /* position units; <= 0: per vertex 2^-25 * max(|y|_inf, s), s the model's normalisation scale
                             (the rest rig's extent rounded to a power of two) */
    float *residual_out;  /* N, or NULL: |x + f Pi d(x) - y|_2 at the x that is written, before its rounding to fp32 */
    int *iters_out;       /* N, or NULL: steps taken (>= 0) when converged; -1 max_iter reached; -2 broke down */
} fd_invert_opts;

/* Host arrays (those in `opts` too), synchronous. */
int fd_invert(fd_ctx *ctx, int64_t N, const float *Y, float *X_out, const float *dist2,
              const float *tu, const float *tv, const float *nrm,
              float radius2, float falloffrate, const fd_invert_opts *opts);
/* Same, device pointers (those in `opts` too), asynchronous on the context's stream, like fd_deform_dev: one launch. */
int fd_invert_dev(fd_ctx *ctx, int64_t N, const float *d_Y, float *d_X_out, const float *d_dist2,
                  const float *d_tu, const float *d_tv, const float *d_nrm,
                  float radius2, float falloffrate, const fd_invert_opts *opts);

/* ---- the adjoint of the deformation ---------------------------------------------
 * Given a sensitivity g_v = dL/dP'_v at the deformed vertices, fd_deform_adjoint returns dL/dW for the built model's
 * weights.  The forward map P' = x + f . Pi . d(x) is linear in W, so this is its exact transpose, no linearisation:
 *   grad_W[j][a]     = sum_v phi_j(x_v) r_v[a],   r_v = f_v Pi_v g_v   (Pi is symmetric; d, Pi, f as above)
 *   grad_W[C][a]     = sum_v r_v[a]                                    (the constant row)
 *   grad_W[C+1+b][a] = sum_v x_v[b] r_v[a]                             (the linear rows)
 * grad_W is (C+4) x 3 fp64 row-major, C = fd_model_centres(ctx): the layout of fd_get_weights' W, and dual to it.
 *
 * The contract.  For the built model and any W' in fd_get_weights' layout and convention,
 *   sum_{j,a} grad_W[j][a] W'[j][a] = sum_v g_v . D_v(W'),
 *   D_v the displacement FD_OUTPUT_DISPLACEMENT defines, evaluated exactly with the weights W'.  This fixes every factor
 *   between the evaluation records and W (the 0.5 of the thin-plate weights, the biharmonic sign, the normalisation).
 * Arithmetic.  Everything is fp64 whatever fd_set_eval_precision says: the fp32 positions and g widened, x - c_j in raw
 *   coordinates, phi of the kind as the inverse forms it; the gate, f and Pi are the forward path's own code.
 * Vertices that contribute nothing.  A gated vertex (dist2 > radius2) and a vertex with f = 0 contribute exactly nothing
 *   whatever G holds there, NaN and infinity included (a select, not a product).  A model with terminationtype != 1 gives
 *   zeros and FD_OK: its forward map is the identity.  N = 0 gives zeros.  Rows of a polynomial term the model lacks are 0.0.
 * Determinism.  No atomics: workgroups write partial sums that a second launch adds in a fixed order, and the number of
 *   workgroups and their vertex ranges depend on N alone.  The same inputs give the same bits on every call.
 * Checks and errors.  The build-status poll and repair, FD_E_NOT_BUILT, the all-or-none rule for tu/tv/nrm and the ordering
 *   behind a batched build are fd_deform's.  FD_E_INVALID for a NULL context, a NULL G or grad_W or N < 0 comes before any
 *   device work.  fd_set_output has no effect.  Only the (C+4) x 3 entries are written.
 * The sensitivity with respect to P_in is not part of this: it is A^T g, which fd_deform_adjoint_points returns (below).
 *
 * Device pointers, asynchronous on the context's stream (two launches; the partial sums live in the context). */
int fd_deform_adjoint_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_G, const float *d_dist2,
                          const float *d_tu, const float *d_tv, const float *d_nrm,
                          float radius2, float falloffrate, double *d_grad_W);
/* Same, host arrays, staged through the context's buffers as fd_invert's; synchronous. */
int fd_deform_adjoint(fd_ctx *ctx, int64_t N, const float *P_in, const float *G, const float *dist2,
                      const float *tu, const float *tv, const float *nrm,
                      float radius2, float falloffrate, double *grad_W);
/* The map deltas -> weights of the context's rest points, kernel, parameters and term: S is (C+4) x M fp64 row-major, and for
 * each component a,  W[:, a] = S . delta[:, a].  Host array, synchronous.  Column i is the weight column a build of the rest rig
 * gives for the delta e_i: helper contexts that share the context's rest array are built in batches (ceil(M/3) builds in
 * groups of FD_MAX_BATCH), created and destroyed inside the call.  Valid for every kind, FD_KERNEL_GAUSSIAN_QNN and
 * FD_KERNEL_GAUSSIAN_ML included: radii and layers depend on the rest rig alone.  The context's own model, its deltas and the
 * factorisation fd_set_deltas reuses are left as they were; nothing is cached, the caller keeps S for as long as the rest rig
 * stands.  FD_E_NOT_BUILT before fd_set_points; a helper build's own error if one fails.
 * The gradient for the deltas is then one small product on the caller's side:  grad_delta = S^T . grad_W  (M x 3). */
int fd_solve_operator(fd_ctx *ctx, double *S);

/* ---- the adjoint of the deformation in the vertex positions ---------------------------
 * Given the same sensitivity g_v = dL/dP'_v, fd_deform_adjoint_points returns dL/dP_in: the reverse-mode derivative of
 * P' = x + f . Pi . d(x) in the positions, dual to the forward-mode transport t' = A t of fd_deform_vectors.  With d, Pi, f, J, L
 * and A = I + f Pi J as above and r_v = f_v Pi_v g_v:
 *   grad_P[v] = A_v^T g_v = g_v + J(x_v)^T r_v,   J(x)^T r = sum_j (w_j . r) grad phi_j(x - c_j) + L^T r
 *   grad_f[v] = g_v . Pi_v d(x_v)                 (d including its polynomial term; the sensitivity for the fall-off value f_v,
 *                                                  what a caller needs to tune radius, falloffrate or the capture distances)
 * grad_P is N x 3 fp64, grad_f N fp64.  dist2 and the frames are per-point attributes: they are not differentiated.
 *
 * The contract.  For any tangent field t (N x 3),
 *   sum_v grad_P[v] . t_v = sum_v g_v . (A_v t_v),
 *   A_v t_v what fd_deform_vectors writes as tu_out for tu = t, evaluated exactly.  This fixes every factor as the adjoint's
 *   identity fixes the weights' factors.
 * Arithmetic.  Everything is fp64 whatever fd_set_eval_precision says: the fp32 positions and g widened, x - c_j in raw
 *   coordinates, phi and g of grad phi of the kind from one shared transcendental as the inverse forms them; the gate, f and Pi
 *   are the forward path's own code.  r is formed as a1 (a1 . g) + a2 (a2 . g), then times f.
 * Vertices where A = I.  A gated vertex (dist2 > radius2), a model with terminationtype != 1 (FD_OK, as fd_deform passes such a
 *   model through) and a vertex with f = 0: grad_P[v] is g_v widened, bit for bit, NaN and infinity included (a select, not a
 *   product): fd_deform_vectors' "A = I exactly".  grad_f[v] is 0.0 for the gated vertex and for the model that is not built;
 *   for f = 0 it is the formula's value: the map still depends on f there.
 * Determinism.  A vertex's result depends on nothing but its own inputs and the model: the same bits for any N, at any place in
 *   the launch, on every call, in the host and the device-pointer form.  No atomics and no sums across vertices.
 * fd_set_output has no effect: the result is the cotangent of the POSITION output.  For FD_OUTPUT_DISPLACEMENT the caller
 *   subtracts g.
 * Aliasing.  None allowed.
 * Checks and errors.  FD_E_INVALID for a NULL context, a NULL G or grad_P (G even with N = 0, as the adjoint's), N < 0 or an opts
 *   whose struct_size is too small comes before any device work.  The build-status poll and repair, FD_E_NOT_BUILT, the
 *   all-or-none rule for tu/tv/nrm and the ordering behind a batched build are fd_deform's.  N = 0 writes nothing. */
typedef struct fd_adjoint_points_opts {
    int struct_size;     /* = sizeof(fd_adjoint_points_opts); smaller is FD_E_INVALID */
    int reserved;
    double *grad_f;      /* N, or NULL */
} fd_adjoint_points_opts;

/* Device pointers (grad_f in `opts` too), asynchronous on the context's stream: one launch.  opts == NULL: no grad_f. */
int fd_deform_adjoint_points_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_G, const float *d_dist2,
                                 const float *d_tu, const float *d_tv, const float *d_nrm,
                                 float radius2, float falloffrate, double *d_grad_P, const fd_adjoint_points_opts *opts);
/* Same, host arrays (grad_f in `opts` too), staged through the context's buffers as fd_deform_adjoint's; synchronous. */
int fd_deform_adjoint_points(fd_ctx *ctx, int64_t N, const float *P_in, const float *G, const float *dist2,
                             const float *tu, const float *tv, const float *nrm,
                             float radius2, float falloffrate, double *grad_P, const fd_adjoint_points_opts *opts);

/* ---- the Gram operator and the fit ------------------------------------------------
 * The deformation is linear in the weights and the weights are linear in the deltas (W = S delta, fd_solve_operator), so
 * fitting the deformed mesh to target positions by least squares is ONE linear problem.  Its second-order term is the Gram
 * matrix of the forward map over the vertices, which fd_deform_gram returns; fd_fit_deltas composes it with the adjoint and S
 * and solves for the deltas.
 *
 * Notation.  For vertex v, Psi_v is the row of length C+4 that multiplies W in fd_get_weights' layout and convention: its
 *   first C entries are phi_j(x_v) times the factor the records' weights carry, then 1, x, y, z.
 *   D_v(W) = f_v Pi_v (Psi_v W).
 * With optional per-vertex fp32 weights omega_v >= 0 (NULL means 1):
 *   H[q][j][k] = sum_v omega_v f_v^2 (Pi_v^2)[b][c] Psi_vj Psi_vk        q <-> (b,c)
 * The contract.  For the built model and any W', W'' in fd_get_weights' layout,
 *   sum_{b,c} sum_{j,k} W'[j][b] H[q(b,c)][j][k] W''[k][c] = sum_v omega_v D_v(W') . D_v(W''),
 *   D what FD_OUTPUT_DISPLACEMENT defines, evaluated exactly.
 * Pi is not idempotent: the projection axes a1, a2 are normalised but not orthogonalised, so the weight is Pi_v^2, not Pi_v.
 *   Pi_v is formed with the forward path's own code and squared in fp64.
 * Output.  nq x (C+4) x (C+4) fp64 row-major.  Without projection frames nq = 1 (Pi = I; H (x) I_3 is the full operator);
 *   with projection frames nq = 6, ordered xx, xy, xz, yy, yz, zz.  Both triangles are written, and the lower is the mirror of
 *   the upper bit for bit.  Multilayer records come out in fd_get_weights' layer-major order.  Rows and columns of polynomial
 *   terms the model lacks are 0.0.  Only the nq (C+4)^2 entries are written.
 * Arithmetic.  The adjoint's: everything is fp64 whatever fd_set_eval_precision says, x - c_j in raw coordinates, phi of the
 *   kind as the inverse forms it; the gate, f and Pi are the forward path's own code.  The products run on the fp64 matrix pipe.
 * Vertices that contribute nothing.  A gated vertex, a vertex with f = 0 and a vertex with omega = 0 contribute exactly
 *   nothing whatever P or omega hold there, NaN included (a select, not a product).  A model with terminationtype != 1, or
 *   N = 0, gives zeros and FD_OK.
 * Determinism.  No atomics: workgroups write partial blocks that a second launch adds in a fixed order.  The number of vertex
 *   ranges is a function of N and C alone; the same inputs give the same bits on every call, and the host and device-pointer
 *   forms agree bit for bit.  The scratch for partial blocks lives in the context and is bounded by lowering the number of
 *   ranges: at most 256 ranges, and at most 256 MiB with all six components (one range above that; C + 4 <= 2352 stays inside).
 * Checks and errors.  FD_E_INVALID for a NULL context, a NULL H or N < 0 comes before any device work.  The build-status poll
 *   and repair, FD_E_NOT_BUILT, the all-or-none rule for tu/tv/nrm and the ordering behind a batched build are fd_deform's.
 *   fd_set_output has no effect.
 *
 * Device pointers, asynchronous on the context's stream (two launches). */
int fd_deform_gram_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_omega, const float *d_dist2,
                       const float *d_tu, const float *d_tv, const float *d_nrm,
                       float radius2, float falloffrate, double *d_H);
/* Same, host arrays, staged through the context's buffers as fd_deform_adjoint's; synchronous. */
int fd_deform_gram(fd_ctx *ctx, int64_t N, const float *P_in, const float *omega, const float *dist2,
                   const float *tu, const float *tv, const float *nrm,
                   float radius2, float falloffrate, double *H);

/* fd_fit_deltas minimises over delta (M x 3)
 *   E(delta) = sum_v omega_v |D_v(S delta) - (T_v - P_v)|^2 + mu sum_i |delta_i - delta0_i|^2
 * for the context's rest rig, kernel and term: the mesh arguments of fd_deform (host arrays), targets T (N x 3 fp32), omega
 * (N fp32 or NULL for 1), mu >= 0, delta0 (M x 3 fp32, or NULL for 0) and S -- what fd_solve_operator returned, which the
 * caller keeps while the rest rig stands, or NULL to have it computed inside the call.  A host composition, no new kernel:
 *   right-hand side  S^T . fd_deform_adjoint(g) + mu delta0,  g_v = omega_v (T_v - P_v): the difference and the product by
 *                    omega_v are formed in fp32 (the cotangent fd_deform_adjoint takes is fp32); everything after is fp64.
 *   normal matrix    without projection S^T H S + mu I, of order M, solved with three right-hand sides; with projection the
 *                    3M x 3M block form of S^T H_q S (unknown 3 i + b).  Plain blocked loops and a Cholesky factorisation on
 *                    the host in fp64.  FD_E_SINGULAR when a pivot is not positive -- not above order . 2^-52 times its
 *                    diagonal entry, which is where a zero pivot lands in fp64: mu = 0 and control points that no live
 *                    vertex constrains.
 * Limits.  FD_E_INVALID, with a message, when C + 4 > FD_FIT_MAX_ROWS (1028) or the order of the system exceeds
 *   FD_FIT_MAX_ORDER (3072): the host composition is O(order^3) and is not meant for more.
 * Outputs.  delta_out, M x 3 fp64 (the caller rounds it for fd_set_deltas), and, unless report is NULL, an fd_fit_report.
 * State.  The context's model, deltas and stored factorisation are left as they were.
 * Checks and errors.  FD_E_INVALID for a NULL context, NULL T or delta_out, N < 0, mu < 0 or not finite, a report whose
 *   struct_size is too small, a bad frame triple, or a limit above comes before any device work; then FD_E_NOT_BUILT, and
 *   whatever fd_solve_operator, fd_deform_gram or fd_deform_adjoint return.  Synchronous. */
#define FD_FIT_MAX_ROWS 1028
#define FD_FIT_MAX_ORDER 3072
typedef struct fd_fit_report {
    int struct_size;      /* = sizeof(fd_fit_report); smaller is FD_E_INVALID */
    int order;            /* the order of the system solved: M, or 3 M with projection frames */
    double E0;            /* E(delta0) */
    double E_fit;         /* E at the solution, predicted from the quadratic form */
    double pivot_min;     /* the smallest and the largest Cholesky pivot (before the square root); on FD_E_SINGULAR */
    double pivot_max;     /*   pivot_min is the pivot that failed */
    double ms_gram;       /* milliseconds in fd_deform_gram, fd_deform_adjoint (with forming g), the composition of the */
    double ms_adjoint;    /*   normal system, and the factorisation and solve */
    double ms_compose;
    double ms_solve;
} fd_fit_report;
int fd_fit_deltas(fd_ctx *ctx, int64_t N, const float *P_in, const float *T, const float *omega, const float *dist2,
                  const float *tu, const float *tv, const float *nrm, float radius2, float falloffrate,
                  double mu, const float *delta0, const double *S, double *delta_out, fd_fit_report *report);

/* ---- the adjoint and the fit for the frames of a shot --------------------------------
 * F cotangents over one mesh, one built model, one gate and one set of projection frames -- a scan sequence, per-frame
 * corrective sculpts -- go through the adjoint in one launch per group of FD_MAX_BATCH frames:
 *   grad_W[f] = Psi^T R_f,   r_{f,v} = f_v Pi_v g_{f,v}
 * which is fd_deform_adjoint's result for the cotangent G_f.  It is a product with C+4 rows, 3F columns and depth N, and it
 * runs on the fp64 matrix pipe with phi formed once per (vertex, record) for all frames of a group.
 * Layout.  G is F x N x 3 fp32, frame-major: frame f's cotangent at vertex v is G[(f N + v) 3 ..].  grad_W is F x (C+4) x 3
 *   fp64: frame f's block, in fd_get_weights' layout, starts at grad_W[f (C+4) 3].
 * The contract.  For every frame f, the built model and any W' in fd_get_weights' layout and convention,
 *   sum_{j,a} grad_W[f][j][a] W'[j][a] = sum_v g_{f,v} . D_v(W'),
 *   D_v the displacement FD_OUTPUT_DISPLACEMENT defines, evaluated exactly with the weights W'.
 * Arithmetic.  The adjoint's: everything is fp64 whatever fd_set_eval_precision says, x - c_j in raw coordinates, phi of the
 *   kind as the inverse forms it; the gate, f and Pi are the forward path's own code; Pi g and the product by f are fp64.
 * The shot form and fd_deform_adjoint differ in the order of additions and are not bit-equal to each other.  Each stays
 *   inside the same bound against the exact sum.
 * Independence of F.  No atomics: workgroups write partial blocks that a second launch adds in a fixed order, and the number
 *   of vertex ranges is a function of N and C alone, not of F.  The block of frame f has the same bits whether it is computed
 *   alone (F = 1) or among any number of other frames, whatever those hold, on every call, and in the host and the
 *   device-pointer forms.
 * Vertices that contribute nothing.  A gated vertex (dist2 > radius2) and a vertex with f = 0 contribute exactly nothing in
 *   every frame whatever G holds there, NaN and infinity included (a select before the product).  A NaN or infinity in frame
 *   f's G at a live vertex reaches frame f's block only.  A model with terminationtype != 1 gives zeros and FD_OK; N = 0 gives
 *   zeros.  Rows of a polynomial term the model lacks are 0.0.
 * Scratch.  The partial blocks live in the context and grow on demand: at most 256 ranges, and at most 256 MiB for a group
 *   of 32 frames at any C + 4 <= 1028 (fewer ranges above that).  The groups use them one after the other.
 * Checks and errors.  FD_E_INVALID for a NULL context, a NULL G or grad_W, N < 0 or F < 1 comes before any device work; any
 *   F >= 1 is accepted.  The build-status poll and repair, FD_E_NOT_BUILT, the all-or-none rule for tu/tv/nrm and the
 *   ordering behind a batched build are fd_deform's.  fd_set_output has no effect.  Only the F (C+4) x 3 entries are written.
 *
 * Device pointers, asynchronous on the context's stream: two launches per group of FD_MAX_BATCH frames. */
int fd_deform_adjoint_shot_dev(fd_ctx *ctx, int64_t N, int F, const float *d_P_in, const float *d_G, const float *d_dist2,
                               const float *d_tu, const float *d_tv, const float *d_nrm,
                               float radius2, float falloffrate, double *d_grad_W);
/* Same, host arrays; synchronous.  G is staged group by group through a buffer the context owns (FD_MAX_BATCH frames of
 * N x 3 fp32 at most). */
int fd_deform_adjoint_shot(fd_ctx *ctx, int64_t N, int F, const float *P_in, const float *G, const float *dist2,
                           const float *tu, const float *tv, const float *nrm,
                           float radius2, float falloffrate, double *grad_W);
/* fd_fit_deltas for F targets over the same mesh, rest rig, omega, mu and gate: frame f minimises E with T_f (T is F x N x 3
 * fp32, frame-major) and delta0_f (delta0 is F x M x 3 fp32, or NULL for 0).  The Gram matrix, S^T H_q S + mu I and its
 * Cholesky factor hold nothing of the target, so the call runs fd_deform_gram once, composes and factorises once, takes
 * g_{f,v} = omega_v (T_{f,v} - P_v) (fp32, as fd_fit_deltas forms it) through fd_deform_adjoint_shot in groups of FD_MAX_BATCH
 * frames -- for every F, F = 1 included -- and solves every frame's right-hand side against the one factor.
 * Frame f's deltas have the same bits whatever the other frames are and however many there are.  They are not bit-equal to
 *   fd_fit_deltas' on the same target: the two adjoints add in different orders.
 * Outputs.  delta_out is F x M x 3 fp64.  reports is NULL or F entries, each with struct_size set: E0 and E_fit are the
 *   frame's; order, the pivots and the four ms_* are the call's own and the same in every entry (ms_adjoint covers forming
 *   every g_f and all groups).  On FD_E_SINGULAR nothing is written to delta_out.
 * Limits, FD_E_SINGULAR, the checks and the state guarantee are fd_fit_deltas'; in addition F < 1 is FD_E_INVALID and every
 *   entry's struct_size is checked before any device work.  Synchronous. */
int fd_fit_deltas_shot(fd_ctx *ctx, int64_t N, int F, const float *P_in, const float *T, const float *omega,
                       const float *dist2, const float *tu, const float *tv, const float *nrm,
                       float radius2, float falloffrate, double mu, const float *delta0, const double *S,
                       double *delta_out, fd_fit_report *reports);

/* ---- the baked deformer: every control point's influence on every vertex -----------------
 * The deformation is linear in the rig's deltas: W = S delta (fd_solve_operator) and D_v = f_v Pi_v Psi_v W.  fd_deform_bake
 * hands out that linear map itself, per vertex:
 *   B[v][i] = f_v sum_j Psi_vj S_ji          (N x M)
 * the cardinal function of control point i at vertex v with the vertex's fall-off folded in -- what a rigger paints and
 * inspects as the influence of a control, and what an exporter needs to turn the node into a delta-blend rig for an engine
 * that cannot run an RBF solve:  P'_v = P_v + Pi_v sum_i B[v][i] delta_i,  exact for every pose of the rig.
 *
 * Definition.  S is (C+4) x M fp64 row-major, in fd_get_weights' layout and convention, as fd_solve_operator returns it.  B is
 *   N x M fp64 row-major, B[v][i] = f_v sum_j Psi_vj S_ji.  Psi_v is the Gram section's row: phi in W's convention, then 1, x,
 *   y, z.  Columns for polynomial terms the model lacks count as 0.
 * The contract.  For the built model and any delta' (M x 3),
 *   Pi_v sum_i B[v][i] delta'_i = D_v(S delta'),
 *   D what FD_OUTPUT_DISPLACEMENT defines, evaluated exactly.  Pi is a 3 x 3 and is not folded in: the frames are accepted,
 *   checked by the all-or-none rule, and otherwise unused.
 * Arithmetic.  The adjoint's: everything is fp64 whatever fd_set_eval_precision says, x - c_j in raw coordinates, phi of the
 *   kind as the inverse forms it; the gate and f are the forward path's own code.  The product Psi S runs on the fp64 matrix
 *   pipe; the product by f is one fp64 multiply after the sum.
 * Kinds.  All of them; the multilayer model with its M L records and S in layer-major rows, as fd_deform_gram handles them.
 * Rows that are exactly zero.  A gated vertex (dist2 > radius2), a vertex with f = 0 and every vertex of a model with
 *   terminationtype != 1 (FD_OK) get a row of 0.0 by a select, not a product: P may hold NaN there.
 * Determinism.  A vertex's row depends on its own inputs, the model and S only: the same bits for any N, at any place in the
 *   launch, on every call, in the host and the device-pointer form.  No atomics and no partial blocks: the sum over C+4 lives
 *   in one accumulator.  A caller short of memory bakes vertex ranges and gets the same bits.
 * B or B32.  opts->B32, N x M fp32, is B rounded once: bit for bit (float)B, what an exporter stores.  Either output may be
 *   NULL, not both; with opts == NULL, B is required.
 * Aliasing.  None allowed.
 * Checks and errors.  FD_E_INVALID for a NULL context, a NULL S in the _dev form, N < 0, M not equal to the context's number of
 *   control points, both outputs NULL, an opts whose struct_size is too small or a bad frame triple comes before any device
 *   work.  The build-status poll and repair, FD_E_NOT_BUILT and the ordering behind a batched build are fd_deform's.  N = 0
 *   writes nothing.  fd_set_output has no effect. */
typedef struct fd_bake_opts {
    int struct_size;   /* = sizeof(fd_bake_opts); smaller is FD_E_INVALID */
    int reserved;
    float *B32;        /* N x M, or NULL: B rounded once to fp32 (what an exporter stores) */
} fd_bake_opts;

/* Device pointers (B32 in `opts` too), asynchronous on the context's stream: a pack kernel, the only reader of S, and one
 * launch.  The packed copy of S lives in the context. */
int fd_deform_bake_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_dist2,
                       const float *d_tu, const float *d_tv, const float *d_nrm,
                       float radius2, float falloffrate, const double *d_S, int M,
                       double *d_B, const fd_bake_opts *opts);
/* Same, host arrays (B32 in `opts` too); synchronous.  S == NULL computes it inside the call, as fd_fit_deltas does.  B comes
 * back in chunks of vertices whose device block stays within 256 MiB, so a million vertices by 256 points need no 2 GB of
 * scratch; a vertex's row depends on nothing else in the launch, so the chunks are bit-identical to one launch. */
int fd_deform_bake(fd_ctx *ctx, int64_t N, const float *P_in, const float *dist2,
                   const float *tu, const float *tv, const float *nrm,
                   float radius2, float falloffrate, const double *S, int M,
                   double *B, const fd_bake_opts *opts);

/* ---- the baked deformer's gradient: what a baked rig needs to carry normals and tangents -----------------
 * fd_deform_vectors transports vectors with the Jacobian A = I + f Pi J(x), and J is linear in the weights as the displacement
 * is.  fd_deform_bake_grad hands out B's linear map differentiated once in x:
 *   G[v][a][i] = f_v sum_j dPsi_vj/dx_a S_ji          (N x 3 x M)
 *   A_v = I + Pi_v sum_i delta_i (x) G[v][.][i],   i.e.  (A_v - I)[b][a] = sum_c Pi_v[b][c] sum_i delta_i[c] G[v][a][i]
 * exact for every pose of the rig.  With B and G an engine that cannot run an RBF solve reproduces all of fd_deform_vectors:
 * positions, t' = A t, n' = cof(A) n.
 *
 * Layout.  G is N x 3 x M fp64 row-major: vertex, component a of x, control point.  For each a, G[:, a, :] is an N x M matrix
 *   with row stride 3 M.  S is fd_deform_bake's.
 * dPsi.  For a record, d phi_j / d x_a in W's convention:
 *     thin-plate                 (x - c)(2 ln r + 1), 0 at r = 0
 *     Gaussian, QNN, multilayer  -2 (x - c) / R_j^2 . phi, one record per layer
 *     cubic                      3 r (x - c)
 *     biharmonic                 -(x - c) / r, 0 at r = 0
 *   for the polynomial columns 1, x, y, z: 0, delta_a0, delta_a1, delta_a2.  Columns the term lacks count as 0.
 * The contract.  For the built model and any delta' (M x 3),
 *   I + Pi_v sum_i delta'_i (x) G[v][.][i] = the A of fd_deform_vectors for the model built on delta',
 *   evaluated exactly.  Pi stays out, as in the bake: the frames are accepted, checked by the all-or-none rule, and otherwise
 *   unused.
 * Arithmetic.  Everything is fp64 whatever fd_set_eval_precision says, x - c_j in raw coordinates, the derivative of the kind
 *   as the inverse forms it; the gate and f are the forward path's own code.  The product runs on the fp64 matrix pipe; the
 *   product by f is one fp64 multiply after the sum.
 * Rows that are exactly zero (so A = I exactly, as fd_deform_vectors says).  A gated vertex (dist2 > radius2), a vertex with
 *   f = 0 and every vertex of a model with terminationtype != 1 (FD_OK) get a 3 x M block of 0.0 by a select, not a product: P
 *   may hold NaN there.
 * Determinism.  A vertex's 3 x M block depends on its own inputs, the model and S only: the same bits for any N, at any place
 *   in the launch, on every call, in the host and the device-pointer form.  No atomics and no partial blocks.
 * G or G32.  opts->G32, N x 3 x M fp32, is G rounded once: bit for bit (float)G.  Either output may be NULL, not both; with
 *   opts == NULL, G is required.
 * Aliasing.  None allowed.
 * Checks and errors.  FD_E_INVALID for a NULL context, a NULL S in the _dev form, N < 0, M not equal to the context's number of
 *   control points, both outputs NULL, an opts whose struct_size is too small or a bad frame triple comes before any device
 *   work.  The build-status poll and repair, FD_E_NOT_BUILT and the ordering behind a batched build are fd_deform's.  N = 0
 *   writes nothing.  fd_set_output has no effect. */
typedef struct fd_bake_grad_opts {
    int struct_size;   /* = sizeof(fd_bake_grad_opts); smaller is FD_E_INVALID */
    int reserved;
    float *G32;        /* N x 3 x M, or NULL: G rounded once to fp32 */
} fd_bake_grad_opts;

/* Device pointers (G32 in `opts` too), asynchronous on the context's stream: the bake's pack kernel, the only reader of S, and
 * one launch.  The packed copy of S lives in the context, in the place of the bake's. */
int fd_deform_bake_grad_dev(fd_ctx *ctx, int64_t N, const float *d_P_in, const float *d_dist2,
                            const float *d_tu, const float *d_tv, const float *d_nrm,
                            float radius2, float falloffrate, const double *d_S, int M,
                            double *d_G, const fd_bake_grad_opts *opts);
/* Same, host arrays (G32 in `opts` too); synchronous.  S == NULL computes it inside the call.  G comes back in chunks of
 * vertices whose device block (3 M doubles and / or floats per vertex) stays within 256 MiB; the chunks are bit-identical to
 * one launch. */
int fd_deform_bake_grad(fd_ctx *ctx, int64_t N, const float *P_in, const float *dist2,
                        const float *tu, const float *tv, const float *nrm,
                        float radius2, float falloffrate, const double *S, int M,
                        double *G, const fd_bake_grad_opts *opts);

/* ---- device-resident mesh (next row N3, engine side) --------------------------
 * In an animated shot the mesh on input 0 -- P, the capture's dist2, the tangent
 * frames -- is the same from cook to cook (Houdini tells by the attributes' data
 * IDs) while the rig moves.  fd_mesh_set uploads those arrays once (host
 * pointers; dist2 and the three frame arrays optional; synchronous);
 * fd_deform_mesh evaluates the current model on them and delivers P_out (and
 * falloff_out, may be NULL) into host arrays: written in place over the host link
 * when they are page-locked, through a device staging copy otherwise.  Same
 * results as fd_deform on the same arrays. */
int fd_mesh_set(fd_ctx *ctx, int64_t N, const float *P, const float *dist2, const float *tu, const float *tv,
                const float *nrm);
int64_t fd_mesh_size(const fd_ctx *ctx);
int fd_deform_mesh(fd_ctx *ctx, float *P_out, float *falloff_out, float radius2, float falloffrate);
/* ProximityCapture::init + capture (src/capture.cpp:10-99; called at src/SOP_FaceDeform.cpp:310-322)
 * on the device-resident mesh of fd_mesh_set: the island mask (fd_capture_islands: nearest mesh
 * point of each of the M rest-rig points, then max_edges edge rings over the CSR adjacency) and,
 * for the island points, the squared distance to the rig's surface (fd_capture_dist2: T triangles,
 * 9 floats each; -1 beyond radius2, 0 with dofalloff off and outside every island).  The result
 * becomes the mesh's dist2 array -- the detached attribute `dist_a` of capture.cpp:31 -- and stays
 * on the device until the next fd_mesh_set / fd_mesh_capture: fd_deform_mesh gates and falls off
 * with it.  Host pointers; synchronous.  dist2_out (may be NULL) receives a copy (npoints). */
int fd_mesh_capture(fd_ctx *ctx, const int64_t *offsets, const int *neighbours, int M, const float *rig_xyz,
                    int max_edges, int T, const float *tri_xyz, float radius2, int dofalloff, float *dist2_out);
/* The device-resident dist2 array (uploaded by fd_mesh_set or produced by fd_mesh_capture) into a
 * host array of fd_mesh_size() floats; FD_E_INVALID when the mesh has none. */
int fd_mesh_get_dist2(fd_ctx *ctx, float *dist2_out);

/* ---- model access -----------------------------------------------------------
 * W is (C+4) x 3 fp64 row-major: C RBF weights, the constant row, the x,y,z
 * linear rows (zero when the term lacks them).  radii (may be NULL) gets C
 * Gaussian radii.  C = fd_model_centres(ctx): the control points M, or M * layers
 * for FD_KERNEL_GAUSSIAN_ML (layer-major: record l*M + j is centre j in layer l).
 * For tests and for RCCL-free replication. */
int fd_model_centres(const fd_ctx *ctx);
int fd_get_weights(fd_ctx *ctx, double *W, double *radii);

/* Solved model as one relocatable blob (header + centres + radii + weights):
 * what a vertex-range split broadcasts from the solving GPU (RCCL over xGMI,
 * or any other transport).  on_device != 0: buf is a device pointer and the
 * copy is enqueued on the context's stream.  The header carries the identity of the rest rig the
 * model was built on (the array fd_batch_set_points_dev read it from): contexts that imported
 * models with the same identity form a batch fd_batch_deform_shared_dev accepts -- the frames of a
 * shot, solved on one GPU, evaluated on every GPU's vertex range with one launch per group. */
size_t fd_model_bytes(const fd_ctx *ctx);
int fd_export_model(fd_ctx *ctx, void *buf, size_t capacity, int on_device);
int fd_import_model(fd_ctx *ctx, const void *buf, size_t bytes, int on_device);

/* Block until everything enqueued on the context's stream has finished. */
int fd_synchronize(fd_ctx *ctx);

/* Page-locked host memory for the arrays handed to fd_deform (replaces nothing
 * in the reference: GA pages are ordinary memory; the wrapper gathers them
 * into a flat array anyway, hdk/SOP_FaceDeformHip.cpp).  When every array of a
 * fd_deform call is page-locked the kernel reads and writes them in place over
 * the host link (no staging copies, traffic in both directions at once);
 * pageable arrays are uploaded, evaluated and downloaded one after the other. */
void *fd_host_alloc(size_t bytes);
void fd_host_free(void *p);

/* ---- batched build ------------------------------------------------------------
 * The reference cooks one node at a time: one rbfbuildmodel per cookMySop
 * (src/SOP_FaceDeform.cpp:363).  A dense system of order 260 keeps one CU of a
 * 256-CU device busy, and the device overlaps only two or three such launch
 * chains.  Contexts that share M, kernel, parameters and term -- the frames of
 * one rig, or several facedeform nodes of one cook graph -- can therefore be
 * assembled and factorised together: one launch chain, one workgroup column per
 * context.  Each context ends up as after its own fd_build_async and is
 * evaluated with the usual fd_deform* calls; those wait for the batch where
 * they run on another stream.  Same kernels and pivots; up to order 512 the
 * results are bit-identical to single builds, above that a batch of four or
 * more groups its panels under deeper trailing updates (they are HBM-bound
 * there) and the weights agree to rounding.  Destroy the batch before its
 * contexts. */
typedef struct fd_batch fd_batch;
#define FD_MAX_BATCH 32
fd_batch *fd_batch_create(fd_ctx *const *ctxs, int n);          /* 1..FD_MAX_BATCH contexts of one device */
void fd_batch_destroy(fd_batch *batch);
int fd_batch_size(const fd_batch *batch);
const char *fd_batch_last_error(const fd_batch *batch);
/* Control points of all contexts from caller-owned DEVICE arrays, one pointer
 * pair per context (host arrays of n device pointers).  No copy is enqueued:
 * the next fd_batch_build_async reads them in place, so they must stay valid
 * and unchanged until that build has executed.  Optional -- contexts whose
 * points were set with fd_set_points(_dev) are built from their own copies. */
int fd_batch_set_points_dev(fd_batch *batch, const float *const *d_rest_xyz,
                            const float *const *d_delta_xyz, int M);
/* Enqueue the build of every context on hip_stream (NULL: the stream of
 * context 0).  FD_E_INVALID if the contexts differ in M, kernel or term. */
int fd_batch_build_async(fd_batch *batch, void *hip_stream);
/* Wait and report per context (reports may be NULL, else n entries).  Returns
 * the first non-zero per-context code. */
int fd_batch_build_result(fd_batch *batch, fd_report *reports);
/* Evaluate every context of the batch on its own vertex arrays with ONE launch
 * (tables of n device pointers, host arrays; the optional tables may be NULL,
 * and so may their entries except P).  A launch over 1M vertices spends ~12 %
 * of its time ramping up and draining; a launch over all frames of a group
 * does not.  Falls back to one launch per context when they do not all take
 * the default thin-plate kernel on equally sized inputs.  Per context the
 * result is exactly that of fd_deform_dev_stream. */
int fd_batch_deform_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *const *d_P_in,
                        float *const *d_P_out, const float *const *d_dist2, float *const *d_falloff_out,
                        const float *const *d_tu, const float *const *d_tv, const float *const *d_nrm,
                        float radius2, float falloffrate);

/* The same for frames that share the MESH and the REST RIG -- the frames of an animated shot, the
 * blendshapes of one head (BASELINE configs 2-4 as SURVEY.md 8d lays them out: "same mesh and rest
 * rig, deltas phase-shifted"): one input mesh (d_P_in, d_dist2, frames: single arrays), one output
 * pair per context.  phi(|x - c_j|^2) depends on the vertex and the centre only, so it is formed
 * once for all frames, and the contraction with the 3 F columns of weights is a dense
 * (N x M) x (M x 3F) product on the matrix pipe (fp16 x 2 split operands, 22 bits, fp32
 * accumulation).  Every frame still has its own model, built by its own assemble + solve.  The
 * contexts must have read their rest points from ONE device array (fd_batch_set_points_dev with
 * the same d_rest_xyz for all; FD_E_INVALID otherwise); thin-plate or Gaussian kernel
 * (FD_KERNEL_GAUSSIAN, FD_KERNEL_GAUSSIAN_QNN -- the SOP's default model: exp(-d2 / R_j^2) from direct
 * coordinate differences, formed once for all frames), fp32 evaluation, 32 or more centres -- anything else
 * (biharmonic, cubic, the multilayer model, fp64) takes fd_batch_deform_dev on the shared arrays.  Parity
 * with the oracle as for fd_deform (1e-5); NOT bit-identical to the one-frame kernels.
 * Fastest form: 17..32 frames (32-row output tiles, rows packed three per frame: 20 frames cost two tiles, not three), no d_dist2, no tangent frames, every d_falloff_out
 * given and 16-byte aligned (results are the same without, through a slower epilogue).  Outputs are written with
 * the non-temporal hint: they are not expected in L2 by whatever runs next. */
int fd_batch_deform_shared_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                               float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out,
                               const float *d_tu, const float *d_tv, const float *d_nrm, float radius2,
                               float falloffrate);
/* fd_batch_vectors: what fd_batch_deform_vectors_shared_dev transports for every frame of the batch.  N, tu, tv are
 * ONE N x 3 fp32 input array each (the shared mesh's), each with a table of n output pointers (one per context);
 * jacobian: a table of n pointers to N x 9 row-major A, or NULL.  A table is either NULL or has n non-NULL entries,
 * and each input comes with its output table: both or neither. */
typedef struct fd_batch_vectors {
    int struct_size;                              /* = sizeof(fd_batch_vectors); smaller is FD_E_INVALID  */
    const float *N;  float *const *N_out;         /* ONE input array (the shared mesh), n output pointers  */
    const float *tu; float *const *tu_out;
    const float *tv; float *const *tv_out;
    float *const *jacobian;                       /* n pointers to N x 9 row-major A, or NULL              */
} fd_batch_vectors;

/* fd_batch_deform_shared_dev plus, for every frame f, the Jacobian and the vectors it carries.
 *   Definition: exactly fd_deform_vectors' (above), per frame: A_f = I + f Pi J_f, t' = A_f t (not renormalised),
 *     n' = cof(A_f) n rescaled to |n|.  Gated vertices, unbuilt frames and f = 0 pass every vector through bit for bit,
 *     with A = I exactly.  Entries past N are not touched.
 *   Positions: P_out and falloff_out are bit-identical to fd_batch_deform_shared_dev called with the same arguments:
 *     that launch runs unchanged and a launch of its own writes the vector outputs.  vec == NULL, or every pointer in
 *     it NULL, is exactly fd_batch_deform_shared_dev.
 *   Aliasing: every output pointer (P_out, falloff_out and the tables of vec) must differ from every shared input
 *     (d_P_in, d_dist2, vec->N / tu / tv, the projection frames d_tu / d_tv / d_nrm); otherwise FD_E_INVALID, before
 *     any device work.  (One input serves F outputs: written in place, the first frame would clobber the others' input.)
 *   Where the matrix-pipe launch applies: where fd_batch_deform_shared_dev takes its own launch (thin-plate,
 *     FD_KERNEL_GAUSSIAN, FD_KERNEL_GAUSSIAN_QNN, fp32 evaluation, M >= 32, one rest array).  There J_f is a split-fp16
 *     contraction of the gradient basis with the weight tiles of the position launch (its error bar is
 *     ||dA||_F <= 2^-22 ||A||_F + 2^-21 f S').  Range: thin-plate stays finite to ~235 rig radii from every centre (the
 *     position launch itself to ~70); the Gaussian kinds need every radius R_j above ~0.0024 rig radii (0.24 % of the
 *     rig's extent, rounded to a power of two), below which the basis overflows fp16 and A is not finite.  Everywhere else (biharmonic, cubic, multilayer, fp64, fewer centres) the
 *     call runs, per context, exactly what fd_deform_vectors_dev runs on the shared arrays, bit for bit.
 *   Reads of the models: fd_batch_wait_consumed covers the vector launch as well -- it reads only the batch's scratch,
 *     the mesh and the vectors; after it the contexts may be rebuilt while the vector launch still runs.
 * Asynchronous on hip_stream (NULL: context 0's), like fd_batch_deform_shared_dev. */
int fd_batch_deform_vectors_shared_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                                       float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out,
                                       const float *d_tu, const float *d_tv, const float *d_nrm,
                                       float radius2, float falloffrate, const fd_batch_vectors *vec);
/* The kernel the vector launch of fd_batch_deform_vectors_shared_dev takes for M centres, `frames` contexts and a
 * kernel kind ("k_vectors32_shared_thin_plate" / "k_vectors32_shared_gaussian"), or "" where the call runs the
 * per-context launches instead.  Like fd_shared_kernel_name it sees no context: the name holds for a batch evaluated
 * in fp32 (fd_set_eval_precision) -- a batch set to FD_EVAL_FP64 always takes the per-context launches, whatever this
 * returns (the one-launch fp64 form is fd_batch_deform_vectors_shared_fp64_dev).  For tests and profiles. */
const char *fd_shared_vectors_kernel_name(int M, int frames, int kind);
/* The frames of a shot evaluated in fp64 by ONE matrix-pipe launch: fd_batch_deform_shared_dev's arguments, gate,
 * tangent projection, fall-off, fd_set_output handling, error codes, build-status poll, stream ordering behind the
 * batch's builds and one-rest-rig condition (FD_E_INVALID), with
 *   Precision: every frame is evaluated in fp64 whatever fd_set_eval_precision says on the contexts (a built model
 *     carries its fp64 records either way); the contexts' settings are not changed by the call.
 *   Definition: per frame, the FD_EVAL_FP64 evaluation of fd_deform_dev -- fp32 positions widened to fp64, direct
 *     differences in raw coordinates, the kind's fp64 phi, fp64 accumulation over the centres on top of the fp64 affine
 *     part, ONE rounding of the three sums to fp32, then the fp32 epilogue (projection, fall-off, write-back) of every
 *     other launch.  Only the order of the fp64 summation differs from the per-frame launch: every output component is
 *     within one fp32 ulp of fd_batch_deform_dev's on FD_EVAL_FP64 contexts, every fd_falloff value bit-identical.  phi is
 *     formed once per (vertex, centre) for all frames and contracted with the frames' fp64 weights on
 *     v_mfma_f64_16x16x4_f64.  No floating-point atomics: the same inputs give the same bits on every call, and a
 *     vertex's result does not depend on its place in the launch ([0, N) in one call or in two ranges: same bits).
 *   Pass-through: a gated vertex (d_dist2 > radius2), and every vertex of a frame whose model is not built
 *     (terminationtype != 1), is passed through -- the position bit for bit, or 0 in FD_OUTPUT_DISPLACEMENT mode -- and
 *     its fd_falloff entry is not written.  Entries past N are not touched.
 *   Where the launch applies: thin-plate, FD_KERNEL_GAUSSIAN, FD_KERNEL_GAUSSIAN_QNN, biharmonic and cubic; any term;
 *     1..FD_MAX_BATCH frames (no lower threshold); any M a model can be built for (a model that does not fit LDS is staged
 *     in chunks of centres).  Everywhere else -- the multilayer model, an eval_variant override -- the call runs, per
 *     context, exactly the launch fd_deform_dev_stream runs for an FD_EVAL_FP64 context on the shared arrays, bit for bit.
 *   Aliasing: with more than one frame no output (P_out, falloff_out) may be a shared input (d_P_in, d_dist2, d_tu,
 *     d_tv, d_nrm): FD_E_INVALID, before any device work.  With one frame P_out[0] == d_P_in is allowed, as in
 *     fd_deform_dev; nothing else is.
 *   Reads of the models: fd_batch_wait_consumed covers this launch as it covers fd_batch_deform_shared_dev -- a first
 *     small kernel copies the fp64 weights (in matrix-operand order), the centre records, the affine parts, the frames'
 *     status and the output addresses into scratch of the batch that only this call uses, and the evaluation reads that
 *     copy alone; after fd_batch_wait_consumed the contexts may be rebuilt while the evaluation still runs.  The fp32
 *     call's two scratch sets and fd_batch_prepare_shared are not involved.
 *   Not covered: fd_batch_cook_group, fdsop_cook and fd_batch_deform_vectors_shared_dev do not take this launch, and
 *     the multilayer model runs the per-context launches in THIS call: the one-launch fp64 form of a multilayer shot is
 *     a call of its own, fd_batch_deform_shared_ml_fp64_dev (below).  The Jacobian and the vectors of an fp64 shot have a
 *     call of their own on top of this one: fd_batch_deform_vectors_shared_fp64_dev (below).
 * Asynchronous on hip_stream (NULL: context 0's). */
int fd_batch_deform_shared_fp64_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                                    float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out,
                                    const float *d_tu, const float *d_tv, const float *d_nrm,
                                    float radius2, float falloffrate);
/* The kernel fd_batch_deform_shared_fp64_dev launches for M centres, `frames` contexts and a kernel kind
 * ("k_deform64_shared"), or "" where it runs the per-context launches (FD_KERNEL_GAUSSIAN_ML: see
 * fd_batch_deform_shared_ml_fp64_dev).  It sees no context: an
 * eval_variant override takes the per-context launches whatever this returns.  For tests and profiles. */
const char *fd_shared_fp64_kernel_name(int M, int frames, int kind);
/* The frames of a shot of MULTILAYER models (FD_KERNEL_GAUSSIAN_ML) evaluated by ONE matrix-pipe launch:
 * fd_batch_deform_shared_dev's arguments, gate, tangent projection, fall-off, fd_set_output handling, error codes,
 * build-status poll and repair, stream ordering behind the batch's builds and one-rest-rig condition (FD_E_INVALID), with
 *   Definition: per frame, the fp32 evaluation of the solved model's M x L Gaussian records (radii R / 2^l) on top of its
 *     polynomial, then the fp32 epilogue of fd_deform_dev.  exp(-d2 / R_l^2) is formed once per (vertex, record) for all
 *     frames -- d2 once per centre for the layers that sit side by side in a lane's operand, every layer with its own
 *     multiply and its own exponential -- and contracted with the frames' weights, as two fp16 pieces each, on
 *     v_mfma_f32_32x32x16_f16 with fp32 accumulation.  The result meets the 1e-5 parity bar against the reference like the
 *     per-context launches do; it is not bit-identical to them (22 significant bits in the contraction against 24); every
 *     fd_falloff value is.  No floating-point atomics: the same inputs give the same bits on every call, a vertex's
 *     result does not depend on its place in the launch ([0, N) in one call or in two ranges: same bits), nor on
 *     fd_batch_set_eval_cus.
 *   Where the launch applies: every context FD_KERNEL_GAUSSIAN_ML with the same M, radius, layers, lambda and term, built
 *     on one rest array; FD_EVAL_FP32; no eval_variant override; 1..8 layers; any M a multilayer model can be built for (the
 *     model is staged through LDS in chunks of records); 2..FD_MAX_BATCH frames.  Measured at 1M vertices and 256 centres
 *     (DESIGN.md 4.1f), launch against per-context launches: with 4 layers 0.31 / 0.35 ms at 2 frames (1.14x), 0.32 / 1.32 ms
 *     at 8, 0.57 / 5.26 ms at 32 (9.3x); with 8 layers 0.60 / 0.62 ms at 2 (1.04x), 0.99 / 10.1 ms at 32 (10.2x).
 *   Everywhere else -- other kinds, fp64 contexts, eval_variant overrides, imported models, one frame, layer counts
 *     outside 1..8 -- the call IS fd_batch_deform_shared_dev with the same arguments, bit for bit.
 *   Pass-through: a gated vertex (d_dist2 > radius2), and every vertex of a frame whose model is not built
 *     (terminationtype != 1), is passed through -- the position bit for bit, or 0 in FD_OUTPUT_DISPLACEMENT mode -- and
 *     its fd_falloff entry is not written.  Entries past N are not touched.
 *   Aliasing: no output (P_out, falloff_out) may be a shared input (d_P_in, d_dist2, d_tu, d_tv, d_nrm): FD_E_INVALID,
 *     before any device work.  With one frame P_out[0] == d_P_in is allowed, as in fd_batch_deform_shared_fp64_dev.
 *   Reads of the models: fd_batch_wait_consumed covers this launch -- a first small kernel copies the frames' weights
 *     (split fp16 tiles), the M x L records {c'x, c'y, c'z, -log2(e) s^2 / R_l^2}, the polynomial tiles, the frames' status
 *     and the output addresses into scratch of the batch that only this call uses, and the evaluation reads that copy
 *     alone; after fd_batch_wait_consumed the contexts may be rebuilt while the evaluation still runs.  The fp32 call's
 *     two scratch sets, fd_batch_prepare_shared and the fp64 scratch are not involved.
 *   Not covered: fd_batch_cook_group, fdsop_cook and the four other shared calls do not take this launch (a multilayer
 *     batch runs the per-context launches there, as before).  The Jacobian and the vectors of a multilayer shot are a
 *     call of their own on top of this one: fd_batch_deform_vectors_shared_ml_dev (below).  A multilayer shot that needs
 *     fp64 has fd_batch_deform_shared_ml_fp64_dev (below).
 * Asynchronous on hip_stream (NULL: context 0's). */
int fd_batch_deform_shared_ml_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                                  float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out,
                                  const float *d_tu, const float *d_tv, const float *d_nrm,
                                  float radius2, float falloffrate);
/* The kernel fd_batch_deform_shared_ml_dev launches for M centres, `layers` layers and `frames` contexts
 * ("k_deform32_shared_ml"), or "" where it is fd_batch_deform_shared_dev (layers outside 1..8, frames outside
 * 2..FD_MAX_BATCH, M <= 0).  It sees no context: another kind, fp64 contexts or an eval_variant override delegate whatever
 * this returns.  For tests and profiles. */
const char *fd_shared_ml_kernel_name(int M, int layers, int frames);
/* fd_batch_deform_shared_ml_dev plus, for every frame f, the Jacobian and the vectors it carries, in fp32 by ONE
 * matrix-pipe launch of its own: to fd_batch_deform_shared_ml_dev what fd_batch_deform_vectors_shared_ml_fp64_dev is to
 * fd_batch_deform_shared_ml_fp64_dev, and for a multilayer shot what fd_batch_deform_vectors_shared_dev is for the
 * one-layer kinds.
 *   Positions: P_out and falloff_out are bit-identical to fd_batch_deform_shared_ml_dev called with the same arguments:
 *     that call runs unchanged first (its pack kernel, its position launch, its mismatch report), then one launch of its
 *     own writes the vector outputs.  vec == NULL, or every pointer in it NULL, is exactly fd_batch_deform_shared_ml_dev.
 *     Inherited from it: error codes, build-status poll and repair, ordering behind the batch's builds, the one-rest-rig
 *     condition and fd_set_output handling.
 *   Vectors: fd_deform_vectors' definition, per frame, in fp32, on the model's M x L Gaussian records (radii R / 2^l):
 *     A_f = I + f Pi J_f with J_f = sum_c sum_l w_f[c][l] (x) grad phi_l(x - c) + L_f(x) in the normalised coordinates of
 *     the fp32 evaluation, direct differences; t' = A_f t (not renormalised), n' = cof(A_f) n rescaled to |n|;
 *     A is stored as fp32.  The gradient basis 2^8 s_l E_l (x' - c') is formed once per (vertex, record) for all frames -- x' - c'
 *     and d2 once per centre for the layers that sit side by side in a lane's operand, every layer with its own multiply
 *     by s_l = -log2(e) / R_l'^2 and its own v_exp_f32, never E_{l+1} = E_l^4 -- and contracted with the frames' weights, as
 *     two fp16 pieces each (hi x hi, lo x hi, hi x lo), on v_mfma_f32_16x16x32_f16 with fp32 accumulation; the weight and
 *     polynomial tiles are the ones the position call's pack kernel wrote, their per-frame power-of-two scales undone
 *     exactly.  Projection, fall-off, cofactors and the rescale are the one-frame launch's own code.
 *   Error statement.  With S'_f(x) = sum_r ||w_f[r]|| |grad phi_r(x)| + ||L_f|| over the M L records: against an
 *     independent fp64 restatement ||A - A_ref||_F <= 2^-22 ||A_ref||_F + 2^-21 f S'_f(x) -- the bar of
 *     fd_batch_deform_vectors_shared_dev's launch, twice the one-frame fp32 launch's second term (22 significant bits in
 *     the contraction, the dropped lo x lo product, fp32 accumulation).  It is not bit-identical to the per-context
 *     launches.
 *   Radius limit: the hi piece of the basis is finite in fp16 while |2^8 g (x' - c')| <= 2^8 0.52 sqrt(|s_l|) stays below
 *     65504, that is for a FINEST-layer radius R' / 2^(L - 1) of at least 0.00245 rig radii (R' >= 0.00245 2^(L - 1):
 *     0.0196 with 4 layers, 0.314 with 8; a rig radius is the normalisation scale of the rest rig, its extent rounded to
 *     a power of two; fd_batch_deform_vectors_shared_dev's 0.0024, to one more digit and rounded up).  Below that
 *     limit the basis of vertices near d = R_l' / sqrt(2) of a centre overflows to infinity and their A is not finite;
 *     nothing is clamped and nothing is reported.  The positions have no such limit.
 *   Pass-through: every vector output is the input bit for bit, and A = I exactly, for gated vertices
 *     (d_dist2 > radius2), where f = 0, and for frames whose model is not built or whose centres differ from frame 0's
 *     (built = 0 in the frame record, as the position call's pack kernel decided).  Entries past N are not touched.
 *   Aliasing: no output (P_out, falloff_out, the tables of vec) may equal any shared input (d_P_in, d_dist2, d_tu, d_tv,
 *     d_nrm, vec->N / tu / tv): FD_E_INVALID, before any device work.  This holds for a batch of one as well -- the
 *     position call's in-place exception does not apply, because the vector launch reads d_P_in after the position
 *     launch has written.
 *   Tables: as in fd_batch_deform_vectors_shared_ml_fp64_dev -- vec->struct_size at least sizeof(fd_batch_vectors), every
 *     input with its output table (both or neither), a table has n non-NULL entries; otherwise FD_E_INVALID, before any
 *     device work, the checks in that call's order.  N == 0 is FD_OK before any device work.
 *   Where the launch applies: where fd_batch_deform_shared_ml_dev's own launch does (multilayer contexts of one model
 *     built on one rest array, FD_EVAL_FP32, 1..8 layers, no eval_variant override, not an imported model, any M,
 *     2..FD_MAX_BATCH frames) and the frame count is at or above the measured threshold: 3 frames with one layer, 2 frames with
 *     2 to 8 layers.  Measured at 1M vertices and 256 centres (device events, the position-only call subtracted; DESIGN.md
 *     4.7e), vectors alone, launch against per-context launches: with 4 layers 0.82 / 0.90 ms at 2 frames (1.10x),
 *     0.82 / 1.36 ms at 3, 1.65 / 5.91 ms at 12, 3.73 / 15.6 ms at 32 (4.2x); with 8 layers 1.61 / 1.70 ms at 2 (1.05x),
 *     2.65 / 11.3 ms at 12, 4.60 / 30.7 ms at 32 (6.7x); at 2 frames 1.09x to 1.13x with 2, 3, 5, 6, 7 layers and a tie with
 *     one layer (0.295 / 0.295 ms; 0.340 / 0.452 ms at 3 frames, 1.33x).
 *     A multilayer batch below the threshold that the position launch takes keeps the positions of
 *     fd_batch_deform_shared_ml_dev and gets its vectors from the per-context launches: per context and bit for bit what
 *     fd_deform_vectors_dev writes for an FD_EVAL_FP32 context on the shared arrays (the batch's consumed event is
 *     re-recorded behind them: they read the models to their end).
 *   Everywhere else -- other kinds, fp64 contexts, eval_variant overrides, imported models, layer counts outside 1..8,
 *     one frame -- the call IS fd_batch_deform_vectors_shared_dev with the same arguments, bit for bit: it delegates
 *     before touching anything of its own.
 *   Reads of the models: the vector launch reads only the batch's multilayer scratch (as the position call packed it),
 *     the mesh, the vectors and its own arguments: fd_batch_wait_consumed covers it, and the contexts may be rebuilt
 *     while it runs; the next call's pack kernel waits for it before it rewrites that scratch.
 *   Bits: no floating-point atomics; the same inputs give the same bits on every call, a vertex's result does not
 *     depend on its place in the launch ([0, N) in one call or in two ranges: same bits), nor on fd_batch_set_eval_cus.
 * The seven other shared calls, fd_batch_cook_group and fdsop_cook are unchanged.
 * Asynchronous on hip_stream (NULL: context 0's). */
int fd_batch_deform_vectors_shared_ml_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                                          float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out,
                                          const float *d_tu, const float *d_tv, const float *d_nrm,
                                          float radius2, float falloffrate, const fd_batch_vectors *vec);
/* The kernel the vector launch of fd_batch_deform_vectors_shared_ml_dev takes for M centres, `layers` layers and
 * `frames` contexts ("k_vectors32_shared_ml"), or "" where the call runs the per-context launches or is
 * fd_batch_deform_vectors_shared_dev (M <= 0, layers outside 1..8, frames outside 2..FD_MAX_BATCH, frames below the
 * threshold above).  It sees no context: another kind, fp64 contexts, an imported model or an eval_variant override
 * delegate whatever this returns.  For tests and profiles. */
const char *fd_shared_vectors_ml_kernel_name(int M, int layers, int frames);
/* The frames of a shot of MULTILAYER models evaluated in FP64 by ONE matrix-pipe launch: what
 * fd_batch_deform_shared_fp64_dev is for the one-layer kinds.  Inherited from that call: the arguments, the argument
 * checks and their order, N == 0 answered FD_OK before any device work, gate, tangent projection, fall-off,
 * fd_set_output handling, error codes, build-status poll and repair, stream ordering behind the batch's builds and the
 * one-rest-rig condition (FD_E_INVALID), with
 *   Precision: every frame is evaluated in fp64 whatever fd_set_eval_precision says on the contexts (FD_EVAL_FP32 and
 *     FD_EVAL_FP64 contexts give the same bits); the contexts' settings are not changed by the call.
 *   Definition: per frame, the FD_EVAL_FP64 evaluation of fd_deform_dev on the model's M x L Gaussian records (radii
 *     R / 2^l) -- fp32 positions widened to fp64, direct differences in raw coordinates, fp64 accumulation on top of the
 *     fp64 affine part, ONE rounding of the three sums to fp32, then the fp32 epilogue of every other launch -- with two
 *     differences.  (1) The order of the fp64 summation: phi is formed once per (vertex, record) for all frames and
 *     contracted with the frames' fp64 weights on v_mfma_f64_16x16x4_f64.  (2) One exponential per centre and chain, not
 *     per record: the layers of a centre share d2 and R_l = R / 2^l, so E_0 = exp(-d2 / R_0^2) is taken with the library
 *     exp, E_{l+1} = (E_l E_l) (E_l E_l), and AT l = 4 THE CHAIN RESTARTS with a fresh exp(-d2 / R_4^2): a chain never runs
 *     longer than three quadruplings.
 *   Error statement, against the per-context fp64 launches on the same batch (what fd_batch_deform_shared_fp64_dev runs
 *     for a multilayer batch): the two fp64 sums ahead of the one rounding differ by at most (96 + M L) 2^-53 S_f, where
 *     S_f = max_a sum_r |w_f[r][a]| (phi <= 1) -- 96 = 4^3 x 1.5 ulp covers the chain, M L the summation order -- so every
 *     output component is within one fp32 ulp plus that bound of theirs; every fd_falloff value is bit-identical.  No
 *     floating-point atomics: the same inputs give the same bits on every call, a vertex's result does not depend on its
 *     place in the launch ([0, N) in one call or in two ranges: same bits), nor on fd_batch_set_eval_cus.
 *   Where the launch applies: every context FD_KERNEL_GAUSSIAN_ML with the same M, radius, layers, lambda and term, built
 *     on one rest array; 1..8 layers; no eval_variant override; not an imported model; any fd_set_eval_precision
 *     setting; any M a multilayer model can be built for (the model is staged through LDS in chunks of whole centres);
 *     1..FD_MAX_BATCH frames.  No lower threshold on the frame count: one frame already saves L - 1 or L - 2 of L
 *     exponentials, and measured at 1M vertices and 256 centres the launch is ahead of the per-context fp64 launches from
 *     one frame on with 4 and with 8 layers (1.1x at 1 frame, 8.8x at 32).
 *   Everywhere else -- other kinds, eval_variant overrides, imported models, layer counts outside 1..8 -- the call IS
 *     fd_batch_deform_shared_fp64_dev with the same arguments, bit for bit: it delegates before touching anything of
 *     its own.
 *   Pass-through: a gated vertex (d_dist2 > radius2), and every vertex of a frame whose model is not built
 *     (terminationtype != 1) or whose centres differ from frame 0's (contexts of more than one build are compared on the
 *     device; reported as by fd_batch_deform_shared_fp64_dev), is passed through -- the position bit for bit, or 0 in
 *     FD_OUTPUT_DISPLACEMENT mode -- and its fd_falloff entry is not written.  Entries past N are not touched.
 *   Aliasing: no output (P_out, falloff_out) may be a shared input (d_P_in, d_dist2, d_tu, d_tv, d_nrm): FD_E_INVALID,
 *     before any device work.  With one frame P_out[0] == d_P_in is allowed, as in fd_batch_deform_shared_fp64_dev;
 *     nothing else is.
 *   Reads of the models: fd_batch_wait_consumed covers this launch -- a first small kernel copies the frames' fp64
 *     weights (in matrix-operand order, layer-minor within a step of four centres), per centre {cx, cy, cz, s_0, s_4},
 *     the affine parts, the frames' status and the output addresses into scratch of the batch that only this call uses,
 *     and the evaluation reads that copy alone; after fd_batch_wait_consumed the contexts may be rebuilt while the
 *     evaluation still runs.  The fp32 call's two scratch sets, fd_batch_prepare_shared, the fp64 scratch and the fp32
 *     multilayer scratch are not involved.
 *   Not covered: fd_batch_cook_group and fdsop_cook do not take this launch; the Jacobian and the vectors of a
 *     multilayer shot in fp64 are a call of their own on top of this one: fd_batch_deform_vectors_shared_ml_fp64_dev
 *     (below).
 * Asynchronous on hip_stream (NULL: context 0's). */
int fd_batch_deform_shared_ml_fp64_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                                       float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out,
                                       const float *d_tu, const float *d_tv, const float *d_nrm,
                                       float radius2, float falloffrate);
/* The kernel fd_batch_deform_shared_ml_fp64_dev launches for M centres, `layers` layers and `frames` contexts
 * ("k_deform64_shared_ml"), or "" where it is fd_batch_deform_shared_fp64_dev (layers outside 1..8, frames outside
 * 1..FD_MAX_BATCH, M <= 0).  It sees no context: another kind, an imported model or an eval_variant override delegate
 * whatever this returns.  For tests and profiles. */
const char *fd_shared_ml_fp64_kernel_name(int M, int layers, int frames);
/* fd_batch_deform_shared_fp64_dev plus, for every frame f, the Jacobian and the vectors it carries, in fp64 by ONE
 * matrix-pipe launch of its own.
 *   Positions: P_out and falloff_out are bit-identical to fd_batch_deform_shared_fp64_dev called with the same arguments:
 *     that call runs unchanged first, then a launch of its own writes the vector outputs.  vec == NULL, or every pointer
 *     in it NULL, is exactly fd_batch_deform_shared_fp64_dev.  Inherited from it: precision (fp64 whatever the contexts
 *     say, their settings untouched), error codes, build-status poll, ordering behind the batch's builds, the
 *     one-rest-rig condition and fd_set_output handling.
 *   Vectors: fd_deform_vectors' definition, per frame, in fp64: A_f = I + f Pi J_f with
 *     J_f = gs sum_j w_f[j] (x) g_j(x) (x - c_j) + L_f from fp32 positions widened to fp64 and direct differences in raw
 *     coordinates (g and gs: the FD_EVAL_FP64 evaluation's of fd_deform_vectors_dev); t' = A_f t (not renormalised),
 *     n' = cof(A_f) n rescaled to |n|; A is stored as fp32.  Only the order and association of the fp64 sum differ from
 *     the per-frame fp64 launch (k_vectors64_<kind>): the basis g_j(x) (x - c_j) is formed once per (vertex, centre) for
 *     all frames and contracted with the frames' fp64 weights on v_mfma_f64_16x16x4_f64.
 *   Pass-through: every vector output is the input bit for bit, and A = I exactly, for gated vertices
 *     (d_dist2 > radius2), for frames whose model is not built, and where f = 0.  Entries past N are not touched.
 *   Aliasing: no output (P_out, falloff_out, the tables of vec) may equal any shared input (d_P_in, d_dist2, d_tu, d_tv,
 *     d_nrm, vec->N / tu / tv): FD_E_INVALID, before any device work.  This holds for a batch of one as well -- the
 *     position call's in-place exception does not apply, because the vector launch reads d_P_in after the position
 *     launch has written.
 *   Tables: as in fd_batch_deform_vectors_shared_dev -- vec->struct_size at least sizeof(fd_batch_vectors), every input
 *     with its output table (both or neither), a table has n non-NULL entries; otherwise FD_E_INVALID.
 *   Where the launch applies: where fd_batch_deform_shared_fp64_dev's does -- thin-plate, FD_KERNEL_GAUSSIAN,
 *     FD_KERNEL_GAUSSIAN_QNN, biharmonic and cubic; any term; 1..FD_MAX_BATCH frames; any M (a model that does not fit
 *     LDS is staged in chunks of centres).  The multilayer model and an eval_variant override do not take it: there the
 *     vector outputs are, per context and bit for bit, what fd_deform_vectors_dev writes for an FD_EVAL_FP64 context on
 *     the shared arrays.  Neither does a batch of
 *     fewer than 2 frames (thin-plate, biharmonic) or 3 (the Gaussian kinds, cubic): measured at
 *     1M vertices and 256 centres, one frame costs the launch 1.25 ms against 0.80 ms per context (thin-plate) and
 *     0.83 ms against 0.34 ms (Gaussian), the launch's time stays there up to 4 frames, and it is 4.4x / 2.3x faster at
 *     13 frames and 5.5x / 2.5x at 32.  Those batches get the per-context vector launches too, positions
 *     unchanged.  (Biharmonic 0.84 ms against 0.46 ms per frame, cubic 0.72 ms against 0.32 ms.)
 *   Reads of the models: the vector launch reads only the batch's fp64 scratch (as the position call packed it), the
 *     mesh, the vectors and its own arguments: fd_batch_wait_consumed covers it, and the contexts may be rebuilt while
 *     it runs.
 *   Bits: no floating-point atomics; the same inputs give the same bits on every call, and a vertex's result does not
 *     depend on its place in the launch ([0, N) in one call or in two ranges: same bits).
 * fd_batch_deform_vectors_shared_dev is unchanged (per-context launches on fp64 contexts), and so are
 * fd_batch_cook_group and fdsop_cook.  Asynchronous on hip_stream (NULL: context 0's). */
int fd_batch_deform_vectors_shared_fp64_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                                            float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out,
                                            const float *d_tu, const float *d_tv, const float *d_nrm,
                                            float radius2, float falloffrate, const fd_batch_vectors *vec);
/* The kernel the vector launch of fd_batch_deform_vectors_shared_fp64_dev takes for M centres, `frames` contexts and a
 * kernel kind ("k_vectors64_shared"), or "" where the call runs the per-context launches (FD_KERNEL_GAUSSIAN_ML, M <= 0,
 * frames outside 1..FD_MAX_BATCH, and frames below the kind's threshold above: 1 for thin-plate and biharmonic, 1..2 for the
 * Gaussian kinds and cubic).  It sees no context: an eval_variant override takes the per-context launches whatever this returns.  For
 * tests and profiles. */
const char *fd_shared_vectors_fp64_kernel_name(int M, int frames, int kind);
/* fd_batch_deform_shared_ml_fp64_dev plus, for every frame f, the Jacobian and the vectors it carries, in fp64 by ONE
 * matrix-pipe launch of its own: to fd_batch_deform_shared_ml_fp64_dev what fd_batch_deform_vectors_shared_fp64_dev is to
 * fd_batch_deform_shared_fp64_dev.
 *   Positions: P_out and falloff_out are bit-identical to fd_batch_deform_shared_ml_fp64_dev called with the same arguments:
 *     that call runs unchanged first (its pack kernel, its position launch, its mismatch report), then one launch of its
 *     own writes the vector outputs.  vec == NULL, or every pointer in it NULL,
 *     is exactly fd_batch_deform_shared_ml_fp64_dev.  Inherited from it: precision (fp64 whatever the contexts say, their
 *     settings untouched), error codes, build-status poll and repair, ordering behind the batch's builds, the
 *     one-rest-rig condition and fd_set_output handling.
 *   Vectors: fd_deform_vectors' definition, per frame, in fp64, on the model's M x L Gaussian records (radii R / 2^l):
 *     A_f = I + f Pi J_f with J_f = sum_c sum_l w_f[c][l] (x) 2 s_l E_l(x) (x - c) + L_f, s_l = -1 / R_l^2, from fp32
 *     positions widened to fp64 and direct differences in raw coordinates; t' = A_f t (not renormalised),
 *     n' = cof(A_f) n rescaled to |n|; A is stored as fp32.  Two differences from the per-context fp64 launch
 *     (k_vectors64_gaussian on the M L records).  (1) The order and association of the fp64 sum: the basis
 *     2 s_l E_l (x - c) is formed once per (vertex, record) for all frames and contracted with the frames' fp64 weights on
 *     v_mfma_f64_16x16x4_f64, L_f first.  (2) One exponential per centre and chain, exactly the position launch's chain:
 *     E_0 = exp(d2 s_0) with the library exp, E_{l+1} = (E_l E_l) (E_l E_l), s_{l+1} = 4 s_l (exact: the build forms R_l
 *     with ldexp), and AT l = 4 THE CHAIN RESTARTS with a fresh exp(d2 s_4): a chain never runs longer than three
 *     quadruplings, and the restart is part of the definition.  At l = 0 and l = 4 the factor E_l s_l is the per-context
 *     launch's, bit for bit.
 *   Error statement.  With S'_f(x) = sum_r ||w_f[r]|| |grad phi_r(x)| + ||L_f|| over the M L records: against the
 *     per-context fp64 launches on the same batch (fd_batch_deform_vectors_shared_fp64_dev) the two fp64 values of J_f
 *     ahead of the rounding differ in Frobenius norm by at most (104 + 2 M L) 2^-53 S'_f(x) -- 96 = 4^3 x 1.5 ulp covers
 *     the chain, as in the position call's statement, 8 the products' associations on both sides, M L per side the
 *     summation order -- so ||A - A_ctx||_F <= 2^-23 ||A_ctx||_F + (104 + 2 M L) 2^-53 f S'_f; for M L <= 2048 the
 *     second term is at most 4.7e-13 f S'_f, inside the 1e-12 f S'_f of the project's fp64 bar against an independent
 *     restatement, ||A - A_ref||_F <= 2^-22 ||A_ref||_F + 1e-12 f S'_f, which this launch is held to as well.  A chain value
 *     in the subnormal range loses the relative bound; its absolute contribution to J_f is below 2^-1000 |s| ||w||.
 *   Pass-through: every vector output is the input bit for bit, and A = I exactly, for gated vertices
 *     (d_dist2 > radius2), where f = 0, and for frames whose model is not built or whose centres differ from frame 0's
 *     (built = 0 in the scratch head, as the position call's pack kernel decided).  Entries past N are not touched.
 *   Aliasing: no output (P_out, falloff_out, the tables of vec) may equal any shared input (d_P_in, d_dist2, d_tu, d_tv,
 *     d_nrm, vec->N / tu / tv): FD_E_INVALID, before any device work.  This holds for a batch of one as well -- the
 *     position call's in-place exception does not apply, because the vector launch reads d_P_in after the position
 *     launch has written.
 *   Tables: as in fd_batch_deform_vectors_shared_fp64_dev -- vec->struct_size at least sizeof(fd_batch_vectors), every
 *     input with its output table (both or neither), a table has n non-NULL entries; otherwise FD_E_INVALID, before any
 *     device work, the checks in that call's order.  N == 0 is FD_OK before any device work.
 *   Where the launch applies: where fd_batch_deform_shared_ml_fp64_dev's own launch does (multilayer contexts of one
 *     model built on one rest array, 1..8 layers, no eval_variant override, not an imported model, any M) and the frame
 *     count is at or above the measured threshold: 3 frames with one layer, 2 frames with 2 to 8 layers.  Measured at 1M
 *     vertices and 256 centres with the launch taken at every frame count (device events, the position-only call
 *     subtracted), vectors alone, launch against per-context launches: with 4 layers 2.33 / 1.31 ms at
 *     1 frame (0.56x), 2.34 / 2.62 ms at 2 (1.12x), 2.35 / 3.94 ms at 3, 5.40 / 15.8 ms at 12, 10.4 / 41.8 ms
 *     at 32 (4.0x); with 8 layers 4.52 / 2.61 ms at 1 (0.58x), 4.54 / 5.21 ms at 2 (1.15x), 4.54 / 7.81 ms
 *     at 3, 10.2 / 31.3 ms at 12, 19.3 / 82.9 ms at 32 (4.3x).  At 2 frames the ratio is 0.76x with one layer and
 *     1.02x, 1.03x, 1.02x, 1.09x, 1.11x with 2, 3, 5, 6, 7; at 1 frame it is below one with every layer count.
 *     A multilayer batch below the threshold keeps the positions of fd_batch_deform_shared_ml_fp64_dev and gets its
 *     vectors from the per-context launches: per context and bit for bit what fd_deform_vectors_dev writes for an
 *     FD_EVAL_FP64 context on the shared arrays (the batch's consumed event is re-recorded behind them: they read the
 *     models to their end).
 *   Everywhere else -- other kinds, eval_variant overrides, imported models, layer counts outside 1..8 -- the call
 *     IS fd_batch_deform_vectors_shared_fp64_dev with the same arguments, bit for bit: it delegates before touching
 *     anything of its own.
 *   Reads of the models: the vector launch reads only the batch's multilayer-fp64 scratch (as the position call packed
 *     it), the mesh, the vectors and its own arguments: fd_batch_wait_consumed covers it, and the contexts may be
 *     rebuilt while it runs; the next call's pack kernel waits for it before it rewrites that scratch.
 *   Bits: no floating-point atomics; the same inputs give the same bits on every call, a vertex's result does not
 *     depend on its place in the launch ([0, N) in one call or in two ranges: same bits), nor on fd_batch_set_eval_cus.
 * fd_batch_deform_vectors_shared_fp64_dev, fd_batch_deform_vectors_shared_dev, fd_batch_cook_group and fdsop_cook are unchanged.
 * Asynchronous on hip_stream (NULL: context 0's). */
int fd_batch_deform_vectors_shared_ml_fp64_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                                               float *const *d_P_out, const float *d_dist2, float *const *d_falloff_out,
                                               const float *d_tu, const float *d_tv, const float *d_nrm,
                                               float radius2, float falloffrate, const fd_batch_vectors *vec);
/* The kernel the vector launch of fd_batch_deform_vectors_shared_ml_fp64_dev takes for M centres, `layers` layers and
 * `frames` contexts ("k_vectors64_shared_ml"), or "" where the call runs the per-context launches or is
 * fd_batch_deform_vectors_shared_fp64_dev (M <= 0, layers outside 1..8, frames outside 1..FD_MAX_BATCH, frames below
 * the threshold above).  It sees no context: another kind, an imported model or an eval_variant override delegate
 * whatever this returns.  For tests and profiles. */
const char *fd_shared_vectors_ml_fp64_kernel_name(int M, int layers, int frames);
/* The adjoint of the deformation in the vertex positions, summed over the frames of a shot:
 *     grad_P[v] = sum_f A_{f,v}^T g_{f,v},      A_f = I + f Pi J_f(x) the Jacobian of frame f's map (fd_deform_vectors),
 * for the batch's n contexts, which hold n models of ONE rest rig (the condition of fd_batch_deform_shared_fp64_dev: the same
 * in-place rest array, kernel and term; FD_E_INVALID otherwise), on one mesh with one dist2, one set of projection frames,
 * one radius2 and one falloffrate.  It is the gradient that moves the rest mesh or the evaluation points against n scans
 * at once, and what autograd returns for P when P feeds n frames.  With r_{f,v} = f_v Pi_v g_{f,v}:
 *     grad_P[v] = sum_f g_{f,v}  +  sum_{f built} J_f(x_v)^T r_{f,v}.
 *   d_G: n x N x 3 fp32, frame-major (frame f's cotangents at d_G + 3 N f, context f's), as fd_deform_adjoint_shot takes
 *     them.  d_grad_P: N x 3 fp64.  d_P_in, d_dist2, d_tu, d_tv, d_nrm, radius2, falloffrate: as for fd_deform_dev.
 *   Arithmetic: everything is fp64; positions and G are widened; x - c_j in raw coordinates on the fp64 records; phi' of
 *     the kind from its one transcendental, as fd_deform_adjoint_points forms it; gate, fall-off and projection axes are
 *     the forward path's own code.
 *   One launch: for thin-plate, Gaussian, QNN, biharmonic and cubic models (any term, any M, no eval_variant override)
 *     from 2 frames upwards (the threshold of every kind.  Measured at 1M vertices and 256 centres with dist2 and frames, device
 *     events, medians of 25, the launch against n one-frame launches plus the additions: thin-plate 1.01 / 0.82 ms at 1
 *     frame (0.81x), 1.01 / 1.60 ms at 2 (1.59x), 2.08 / 24.1 ms at 32 (11.6x); QNN 0.51 / 0.34 ms at 1 (0.66x),
 *     0.51 / 0.67 ms at 2 (1.33x), 1.55 / 9.88 ms at 32 (6.4x); biharmonic 0.71x at 1, 1.42x at 2; cubic 0.63x at 1,
 *     1.27x at 2), a pack kernel copies the
 *     frames' fp64 weights, the centre records, the affine parts and the frames' status into scratch of the batch that
 *     only this call uses, and one persistent launch reads that copy alone.  The sum over the frames is taken inside the
 *     sum over the centres:
 *         sum_f J_f^T r_f = gs sum_j g_j(x) (x - c_j) s_j + sum_f L_f^T r_f,     s_j = sum_{f,b} w_{f,j,b} r_{f,b},
 *     s and sum_f L_f^T r_f on v_mfma_f64_16x16x4_f64 (depth 3 n), the basis g_j(x) (x - c_j) once per (vertex, centre)
 *     whatever n is.  The result differs from the sum of n fd_deform_adjoint_points_dev results only by the order and
 *     association of the fp64 additions; it is not bit-equal to it.
 *   Everywhere else -- the multilayer model, an eval_variant override, fewer frames -- the call runs
 *     fd_deform_adjoint_points_dev's launch per context and adds the n results in frame order, ((p_0 + p_1) + p_2) + ...:
 *     bit for bit that sum.  (With one frame: bit for bit fd_deform_adjoint_points_dev.)
 *   Vertices where every A_f = I -- gated vertices, vertices with f = 0, all vertices when no frame is built: grad_P[v] is
 *     the fp64 sum of the widened g_{f,v} in frame order, (g_0 + g_1) + g_2 ..., and nothing else.  A select, not a
 *     product: NaN or infinity in the weights or the basis cannot reach it, nor can the G of such a vertex reach another.
 *     With one frame this is g widened, bit for bit.  A frame whose model is not built (terminationtype != 1, or centres
 *     that differ from context 0's) contributes g_{f,v} only, with FD_OK; the status arrives with the next call, as for
 *     fd_batch_deform_shared_fp64_dev.
 *   Bits: no atomics.  A vertex's result depends on its own inputs, n and the models only: the same bits for any N, in one
 *     range or in two, at any place in the launch, on every call, with any fd_batch_set_eval_cus.
 *   Checks, errors, the status poll and repair and the ordering of hip_stream behind the batch's builds are those of
 *     fd_batch_deform_shared_fp64_dev.  FD_E_INVALID before any device work: a NULL batch, a NULL d_G or d_grad_P, N < 0,
 *     a NULL d_P_in with N > 0, some but not all of d_tu / d_tv / d_nrm, d_grad_P equal to an input array (no aliasing is
 *     allowed), contexts of different rest arrays, kernels or terms.  N = 0 writes nothing.  fd_set_output has no effect.
 *   Reads of the models: the one launch reads only its scratch, the mesh and G; fd_batch_wait_consumed covers this call as
 *     it covers fd_batch_deform_shared_fp64_dev (on the per-context route its event lies behind the last launch), and
 *     the next call's pack kernel waits for this call's own event before it rewrites the scratch.
 *   Out of scope: per-frame outputs A_f^T g_f (n calls of fd_deform_adjoint_points_dev, or the Jacobian of
 *     fd_batch_deform_vectors_shared_fp64_dev); grad_f per frame; a one-launch multilayer form; fp32 accumulation;
 *     host-array forms; fdsop_* and the HDK wrapper.
 * Asynchronous on hip_stream (NULL: context 0's). */
int fd_batch_deform_adjoint_points_shared_dev(fd_batch *batch, void *hip_stream, int64_t N, const float *d_P_in,
                                              const float *d_G, const float *d_dist2,
                                              const float *d_tu, const float *d_tv, const float *d_nrm,
                                              float radius2, float falloffrate, double *d_grad_P);
/* The kernel the one launch of fd_batch_deform_adjoint_points_shared_dev takes for M centres, `frames` contexts and `kind`
 * ("k_adjoint_points64_shot"), or "" where the per-context launches run (M <= 0, frames outside 1..FD_MAX_BATCH or below the
 * threshold above, the multilayer kind).  It sees no context: an eval_variant override takes the per-context route
 * whatever this returns.  For tests and profiles. */
const char *fd_shared_adjoint_points_kernel_name(int M, int frames, int kind);
/* Makes hip_stream (NULL: context 0's) wait until the batch's last fd_batch_deform_shared_dev no longer reads the
 * contexts' models: that launch copies what it needs of them (weights as fp16 tiles, the rest rig's centre tiles)
 * into the batch's own scratch with a first small kernel, and the evaluation proper reads only that copy.  A pipeline
 * that cooks group after group on the same contexts puts this in front of the next fd_batch_set_points_dev /
 * fd_batch_build_async instead of waiting for the evaluation itself: the next models are assembled and solved while
 * the current ones are still being evaluated.  (The output arrays ARE still being written: they stay the caller's to
 * order.)  No-op when no shared-rig evaluation has been enqueued on the batch. */
int fd_batch_wait_consumed(fd_batch *batch, void *hip_stream);
/* The first, small part of fd_batch_deform_shared_dev on its own, on a stream of the caller's choice (NULL: context
 * 0's) -- typically the build stream, right behind fd_batch_build_async: the models' weights become fp16 tiles in
 * the batch's scratch (two sets, used in turn) together with the frames' output addresses.  A following
 * fd_batch_deform_shared_dev with the SAME output tables then launches the evaluation alone (its stream waits for
 * this kernel), so an evaluation stream runs evaluations back to back while packing happens beside the builds.
 * Invalidated by the next fd_batch_set_points_dev / fd_batch_build_async (and by a model the library had to
 * rebuild); without it, or with other outputs, fd_batch_deform_shared_dev packs by itself as before.  A no-op when
 * the shared-rig launch does not apply to the batch (other kernels). */
int fd_batch_prepare_shared(fd_batch *batch, void *hip_stream, float *const *d_P_out, float *const *d_falloff_out);
/* CU budget of this batch's shared-rig evaluation launches: fd_batch_deform_shared_dev runs one persistent workgroup per
 * CU (it needs a CU's whole LDS), and a pipeline that builds the next group's models beside the evaluation may want to
 * leave some CUs to those builds.  n_cus <= 0: one workgroup per CU (the default).  More than the device's CU count
 * oversubscribes: shares get shorter and the workgroups beyond the resident ones start as CUs come free (measured: no gain over
 * 224 of 256 beside three batches of builds).  Per batch, not
 * per process: two nodes cooking side by side choose independently (round 2 read an environment variable once).
 * The budget also tells the batch's BUILDS where they run (register-resident build, up to 256 control points): with CUs left
 * to them (n_cus below the device's count) each model is built by one workgroup from start to end and stays on those CUs; with
 * none left (the default: nothing evaluates beside the builds) the assembly of K, Y = K V and the projection run as two short
 * launches over all CUs before the factorisation's workgroup -- the same model to rounding, 0.04 ms sooner. */
int fd_batch_set_eval_cus(fd_batch *batch, int n_cus);
/* One factorisation per batched build where the contexts share the rest rig ("factor once and treat frames as extra
 * right-hand sides").  The reference rebuilds its model on every cook (src/SOP_FaceDeform.cpp:331-363); the system matrix depends
 * on the rest points, the kernel and the term only, so the frames of a shot -- one rest rig, other deltas -- can share it.
 * With `on`, fd_batch_build_async (and fd_batch_cook_group through it) takes one of two shared paths; off by default.
 *
 * Thin-plate family: the call assembles, projects and factorises ONCE, in the register-resident one-launch build of the batch's
 * first context, and carries every other context's right-hand sides through that factor, one workgroup per context (Q^T f, both
 * substitutions, the polynomial, packing).  Conditions: the register-resident build applies (a definite kernel + term pair, up
 * to 256 control points), every context was given the SAME rest array by fd_batch_set_points_dev, and the batch has at least
 * two contexts.
 *
 * Multilayer model (FD_KERNEL_GAUSSIAN_ML): "the factor" is L factors, one per layer -- Phi_l + lambda I depends on the rest
 * rig, R, lambda and l alone.  The call forms the reflectors of the polynomial block once, assembles and Cholesky-factorises
 * the L layer matrices once, side by side, and takes all 3 F right-hand-side columns through them in ONE launch
 * (k_ml_solve_shared: least-squares polynomial, then per layer both substitutions, the weights, lambda w on to the next
 * layer); setup, the records and every frame's terminationtype come from the same kernels as a per-context build, so all
 * that follows -- the shot calls, the per-context launches, fd_export_model -- sees ordinary built models.  Conditions: every
 * context is FD_KERNEL_GAUSSIAN_ML with the same (R, layers, lambda) and term (a batch's contexts always are), every context
 * was given the SAME rest array by fd_batch_set_points_dev, the batch has at least two contexts, and M <= 1024 (a workgroup
 * keeps M x 16 doubles in LDS).  fd_shared_ml_build_kernel_name tells whether a size is taken.  The factors live in scratch of
 * the batch for the one call: nothing is kept for fd_set_deltas, which stays FD_E_NOT_BUILT on a multilayer context.
 *
 * Delegation: a batch that misses a condition -- other rest arrays, other kernels (QNN, lambda > 0 on the thin-plate family),
 * one context, larger rigs, no memory for the scratch -- is built model by model exactly as without the switch, bit for bit.
 * On a shared path the weights equal the per-context builds' to rounding, not bit for bit (1e-12 of max |w| at the sizes
 * tested); the same inputs give the same bits on every call.
 * fd_batch_last_build_shared_factor: 1 if the batch's last build took a shared path. */
int fd_batch_set_shared_factor(fd_batch *batch, int on);
int fd_batch_last_build_shared_factor(const fd_batch *batch);
/* Which kernel takes a multilayer batch's right-hand sides through the shared layer factors when fd_batch_set_shared_factor is
 * on and the contexts share the rest array: "k_ml_solve_shared" for M in 1..1024, layers in 1..8 and 2..32 frames, "" where the
 * build is the per-context one. */
const char *fd_shared_ml_build_kernel_name(int M, int layers, int frames);
/* One LU factorisation per batched build for a shot of QNN models (FD_KERNEL_GAUSSIAN_QNN, the SOP's default model = 0,
 * src/SOP_FaceDeform.cpp:342-345).  A switch of its own, off by default: fd_batch_set_shared_factor keeps its meaning, and a QNN
 * batch under that switch alone is built per frame as ever.  The QNN kernel block Phi + lambda I depends on the rest rig, q, z
 * and the smoothing alone and carries no right-hand sides: in a shot only the deltas differ between frames.
 *
 * What is shared: with `on`, fd_batch_build_async (and fd_batch_cook_group through it) computes the radii, the reflectors of the
 * polynomial block, the assembled kernel block and its LU without pivot search ONCE (the kernels of a per-context build, on one
 * system), inverts the factor's 32 x 32 diagonal blocks, and takes all 3 F right-hand-side columns through that factor in ONE
 * launch (k_qnn_solve_shared: least-squares polynomial, forward and backward substitution, the weights); the records and every
 * frame's terminationtype come from the same kernels as a per-context build, so all that follows -- the shot calls, the
 * per-context launches, fd_export_model -- sees ordinary built models.
 *
 * Conditions: every context is FD_KERNEL_GAUSSIAN_QNN (a batch's contexts already agree on q, z, smoothing, term and M); the LU
 * without pivot search applies -- the padded order is at most 1024, every context has FD_SOLVER_AUTO and none has fallen back to
 * the pivoted LU on this rig; M >= the term's polynomial columns; every context was given the SAME rest array by
 * fd_batch_set_points_dev; the batch has at least the path's minimum frame count (fd_shared_qnn_build_kernel_name is its
 * statement: 2); and the scratch could be allocated.  Measured on MI355X against the per-context batched build:
 * 1.12x faster at 256 points x 32 frames and 1.44x at 1000 x 32, but SLOWER below 8 frames at 256 points (1.6 % at 2 frames) and
 * below 16 frames at 1000 points (13 % at 2 frames) -- the per-context chains already run side by side; leave the switch off for
 * such small groups.
 *
 * Delegation: a batch that misses a condition is built model by model exactly as without the switch, bit for bit; the switch
 * does not touch batches of other kernels.
 *
 * Results: the weights equal the per-context builds' to rounding, not bit for bit; the same inputs give the same bits on every
 * call; the radii are bit-identical to the per-context build's; each frame's fd_report says terminationtype, iterationscount, n
 * and solver_used (= FD_SOLVER_LU_NOPIVOT) as its own build would; coincident centres give -5 in every frame.
 *
 * Fallback: when the shared factorisation finds a multiplier above 4 or a pivot at or below the threshold, every frame reports
 * -4 and the existing host repair applies -- from fd_build_result and from the poll in front of an evaluation each context is
 * rebuilt with the pivoted LU and keeps it for this rig; from then on the batch misses the condition and builds per context.
 *
 * Nothing is kept: the factor lives in scratch of the batch for the one call; fd_set_deltas on a context built this way is
 * FD_E_NOT_BUILT, as after the multilayer shared build.
 * fd_batch_last_build_shared_factor answers 1 when the batch's last build took this path, too. */
int fd_batch_set_shared_lu(fd_batch *batch, int on);
/* Which kernel takes a QNN batch's right-hand sides through the shared LU when fd_batch_set_shared_lu is on and the conditions
 * hold: "k_qnn_solve_shared" for M in 1..1020 (the padded order of every term within 1024) and 2..32 frames, "" where the build
 * is the per-context one. */
const char *fd_shared_qnn_build_kernel_name(int M, int frames);
/* Which kernel fd_batch_deform_shared_dev launches for `frames` frames of an M-centre model of `kind` (a name for profiles and
 * benchmark lines -- the one rocprofv3 prints): "k_deform32_shared_w1" (17..32 frames, the model resident in LDS),
 * "k_deform32_tps_shared_wide" (17..32 frames, staged in chunks), "k_deform32_tps_shared" (up to 16 frames), or "" where the
 * shared-rig launch does not apply (other kernels, fewer than 32 centres: the per-frame launch runs).  No reference counterpart:
 * the reference has one loop (src/SOP_FaceDeform.cpp:404-439). */
const char *fd_shared_kernel_name(int M, int frames, int kind);
/* One GROUP of frames of a shot in one call -- what a frame pipeline enqueues per group, in the order it must be enqueued:
 *   fd_batch_wait_consumed(batch, build_stream)            the batch's previous evaluation has its own copy of the models
 *   fd_batch_set_points_dev(batch, d_rest, d_delta, M)      (the SAME rest array for every context: frames of one rig)
 *   fd_batch_build_async(batch, build_stream)               every frame's model: assembled, factorised, solved
 *   fd_batch_prepare_shared(batch, build_stream, ...)       weights -> fp16 tiles, beside the builds
 *   eval_stream waits for build_stream;  fd_batch_deform_shared_dev(batch, eval_stream, ...)
 * build_stream / eval_stream: the caller's HIP streams (eval_stream NULL: the evaluation goes on build_stream).  d_rest_xyz:
 * the one rest rig; d_delta_xyz: n pointers, one per context.  No d_dist2 / tangent frames: a group that needs them
 * makes the calls above itself.  Replaces, for n frames, n cooks of reference src/SOP_FaceDeform.cpp:268-287, 331-368, 404-439.
 * A host language pays for ONE foreign call per group instead of five with pointer tables (bench.py reports both).
 * events (may be NULL): four caller-owned hipEvent_t handles recorded around the builds (on build_stream) and around the
 * evaluation launch (on eval_stream), for callers that time the pieces; NULL members are skipped.
 * With the evaluation on build_stream itself (eval_stream NULL or equal: one group, nothing to overlap) the call records NO event
 * of its own in front of the builds, between them and the packing or before the evaluation (the build's reports then carry no
 * phase times) -- stream order does what they do across streams, and every
 * record is a barrier packet the queue idles ~4 us for.  The batch's "build done" event is then recorded BEHIND the evaluation:
 * fd_batch_build_result and any other stream ordered after the builds wait a little longer than needed, never too little, and a
 * failed build's status arrives with the NEXT call on the batch (the evaluation of an unbuilt model passes its frame through,
 * as documented for asynchronous builds above). */
typedef struct fd_group_events {
    void *before_build, *after_build;      /* hipEvent_t, recorded on build_stream */
    void *before_eval, *after_eval;        /* hipEvent_t, recorded on eval_stream, around the evaluation launch alone */
} fd_group_events;
int fd_batch_cook_group(fd_batch *batch, void *build_stream, void *eval_stream, const float *d_rest_xyz,
                        const float *const *d_delta_xyz, int M, int64_t N, const float *d_P_in, float *const *d_P_out,
                        float *const *d_falloff_out, const fd_group_events *events);

/* ---- dist2 producer (next row N2) ---------------------------------------------
 * The per-point body of ProximityCapture::capture (src/capture.cpp:58-97) on the
 * device: for every mesh point of an island (mask[i] != 0; mask NULL = all points)
 * the squared distance to the closest point of the rest rig's surface -- what
 * GU_RayIntersect::minimumPoint returns there -- when it is below radius2, else
 * -1 (:76-88); 0 when dofalloff is off (:71-75) and for points outside every
 * island (the detached attribute's default, :31).  The rig surface is T
 * triangles, 9 floats each (a, b, c); degenerate ones (a point, a segment, three
 * points on a line) count as the point sets they are.  Error bound, for every
 * triangle shape and independent of where the scene lies relative to the origin:
 * |dist2 - exact| <= 2e-6 * (exact + E^2), E the longest edge among the T
 * triangles, for points within 10 E of the surface (the range that is tested); a
 * point whose exact distance is within that margin of radius2 may fall on either
 * side of the -1 decision.  The result is fd_deform's dist2 input;
 * with the _dev form it never leaves the device.  Island finding (nearest mesh
 * point of every rig point + edge rings, :101-141) needs the mesh topology and
 * stays with the caller. */
int fd_capture_dist2_dev(fd_ctx *ctx, int64_t N, const float *d_P, const unsigned char *d_mask, int T,
                         const float *d_tri_xyz, float radius2, int dofalloff, float *d_dist2);
int fd_capture_dist2(fd_ctx *ctx, int64_t N, const float *P, const unsigned char *mask, int T,
                     const float *tri_xyz, float radius2, int dofalloff, float *dist2);
/* The island mask itself: ProximityCapture::findIslands (src/capture.cpp:101-141).
 * For every rig point the nearest mesh point (GEO_PointTree::findNearestIdx;
 * ties to the lower index), then every mesh point within max_edges edges of it
 * (GQ_Detail::groupEdgePoints, the start point included).  The handle classes
 * only partition the islands into groups capture() treats alike, so the product
 * is their union, mask[i] in {0, 1}.  The mesh's edges come as a CSR adjacency
 * (offsets[N + 1], neighbours[offsets[N]]), which a static mesh needs building
 * once.  max_edges is capped at 250. */
int fd_capture_islands_dev(fd_ctx *ctx, int64_t N, const float *d_P, const int64_t *d_offsets,
                           const int *d_neighbours, int M, const float *d_rig_xyz, int max_edges,
                           unsigned char *d_mask);
int fd_capture_islands(fd_ctx *ctx, int64_t N, const float *P, const int64_t *offsets, const int *neighbours,
                       int M, const float *rig_xyz, int max_edges, unsigned char *mask);

/* ---- morph-space reprojection (next row N1) ---------------------------------
 * Replaces DirectBSEdit (src/dbse.hpp:7-33, src/dbse.cpp:9-87) and the loop
 * that applies it after the RBF pass (src/SOP_FaceDeform.cpp:444-473).  The
 * 3N x S matrix of blendshape deltas lives on the device; the per-cook passes
 * stream over it once each (HBM-bound).
 *   fd_morph_init            DirectBSEdit::init (dbse.cpp:9-37): deltas
 *                            float(shape - rest) widened to fp64, Householder QR
 *                            in Eigen's packed form.  S <= 3N and
 *                            S <= FD_MORPH_MAX_SHAPES (the per-cook launches keep
 *                            32 bytes of workgroup memory per blendshape, 64 KB in
 *                            all); more is FD_E_INVALID before any device work and
 *                            leaves the object as it was.  Synchronous.
 *   fd_morph_compute_weights_dev  computeWeights (dbse.cpp:39-60):
 *                            w_s = sum_i float(P_i - rest_i) * QRpacked[i][s]
 *   fd_morph_displace_dev    displaceVector + the loop at SOP :458-473:
 *                            P = rest + sum_s delta_s * clamp(float(3 w_s))
 *                                [+ (P - rest) * falloffradius if add_delta]
 *                            clamp_lo_hi: host pointer to {lo, hi} or NULL.
 *   fd_morph_apply           both, on a host array in place; w_out (S) may be NULL.
 * hip_stream NULL = the object's own stream.  is_initialised / is_computed
 * mirror DirectBSEdit::isInitialized / isComputed, which the cook logic tests. */
#define FD_MORPH_MAX_SHAPES 2048
typedef struct fd_morph fd_morph;
fd_morph *fd_morph_create(const fd_config *cfg);
void fd_morph_destroy(fd_morph *m);
const char *fd_morph_last_error(const fd_morph *m);
int fd_morph_init(fd_morph *m, int64_t N, int S, const float *rest_xyz, const float *const *shapes_xyz);
int fd_morph_init_dev(fd_morph *m, int64_t N, int S, const float *d_rest_xyz, const float *const *d_shapes_xyz);
/* The `rest` point attribute the per-cook passes measure against
 * (SOP_FaceDeform.cpp:178-184, 445-447).  Default (or NULL): the rest pose
 * given to fd_morph_init -- what setupBlends stores when input 0 has no rest
 * attribute of its own.  Reset by fd_morph_init. */
int fd_morph_set_rest(fd_morph *m, const float *rest_xyz, int on_device);
int fd_morph_is_initialised(const fd_morph *m);
int fd_morph_is_computed(const fd_morph *m);
int fd_morph_shape_count(const fd_morph *m);
float fd_morph_last_init_ms(const fd_morph *m);
int fd_morph_compute_weights_dev(fd_morph *m, const float *d_P_xyz, void *hip_stream);
int fd_morph_displace_dev(fd_morph *m, float *d_P_xyz, const float *clamp_lo_hi, int add_delta,
                          float falloffradius, void *hip_stream);
int fd_morph_apply(fd_morph *m, float *P_xyz, const float *clamp_lo_hi, int add_delta, float falloffradius,
                   double *w_out);
int fd_morph_get_weights(fd_morph *m, double *w);
int fd_morph_get_qr(fd_morph *m, double *qr, double *tau);   /* 3N x S column-major packed QR (tests) */

/* The F = 1..FD_MAX_BATCH frames of one shot in one pass over each matrix: what
 * a cook per frame runs F times (computeWeights, dbse.cpp:39-60; displaceVector
 * and the loop at SOP_FaceDeform.cpp:458-473, dbse.cpp:62-77) with the packed QR
 * and the deltas read from memory once per call instead of once per frame.
 * d_P_xyz: a host array of F device pointers, each N x 3 fp32 -- the d_P_out
 * table of fd_batch_deform_shared_dev / fd_batch_cook_group as it stands.
 *   fd_morph_compute_weights_batch_dev  per frame fd_morph_compute_weights_dev's
 *       definition: P_f - rest in fp32 (the rest of fd_morph_set_rest), widened,
 *       multiplied with the fp64 packed QR and summed in fp64.  The summation
 *       order differs from the one-frame call's, so the two agree to rounding,
 *       not bit for bit; no floating-point atomics: the same inputs give the
 *       same bits on every call.  Entries of the table may repeat.
 *   fd_morph_displace_batch_dev  per frame fd_morph_displace_dev's arithmetic in
 *       place on d_P_xyz[f], with frame f's batched weights: columns in order
 *       s = 0..S-1, multiply and add rounded separately, float(3 w), the clamp,
 *       the add_delta term and rest + d as there.  Given equal weights frame f
 *       is bit-identical to the one-frame call.  clamp_lo_hi, add_delta and
 *       falloffradius are node parameters: one value for all frames.  Reads
 *       the weights in stream order.  Two equal entries (two frames writing
 *       one array) are FD_E_INVALID.
 *   fd_morph_get_weights_batch  F x S row-major, synchronous (the object's stream).
 * The batched weights are a state of their own: these calls neither read nor
 * write the one-frame weights or is_computed, the one-frame calls do not touch
 * the batched weights, fd_morph_init* clears them.  Displacement and
 * get_weights before a batched compute: FD_E_NOT_BUILT; with an F other than
 * the last batched compute's: FD_E_INVALID.  Argument errors (F outside
 * 1..FD_MAX_BATCH, a NULL table or entry, equal entries for the displacement)
 * return FD_E_INVALID before any device work, the text in fd_morph_last_error.
 * S = 0, any N: as the one-frame calls; entries past N are not touched.
 * Asynchronous on hip_stream (NULL: the object's own stream). */
int fd_morph_compute_weights_batch_dev(fd_morph *m, int F, const float *const *d_P_xyz, void *hip_stream);
int fd_morph_displace_batch_dev(fd_morph *m, int F, float *const *d_P_xyz, const float *clamp_lo_hi, int add_delta,
                                float falloffradius, void *hip_stream);
int fd_morph_get_weights_batch(fd_morph *m, int F, double *w);

/* ---- host-side cook: the HDK-free mirror of cookMySop ----------------------
 * fdsop_* mirrors the SOP's parm surface (src/SOP_FaceDeform.cpp:99-137) and
 * the cook sequence (:215-489) over plain arrays standing in for GU_Detail:
 * same parm tokens, defaults and clamps, same error / warning texts.  The HDK
 * wrapper (hdk/SOP_FaceDeformHip.cpp) and the tests drive this. */
typedef struct fdsop_node fdsop_node;

/* Severity of the worst message of the last cook, as OP_ERROR orders them. */
enum { FDSOP_OK = 0, FDSOP_MESSAGE = 1, FDSOP_WARNING = 2, FDSOP_ERROR = 3 };

typedef struct fdsop_geo {
    /* input 0: the mesh (cooked in place into the output, duplicatePointSource :226) */
    int64_t npoints;
    const float *P;        /* npoints x 3 */
    const float *tangentu; /* npoints x 3 or NULL */
    const float *tangentv;
    const float *N;
    const float *dist2;    /* ProximityCapture's detached attribute (capture.cpp:31) or NULL */
    /* inputs 1 and 2: rest and deformed rig */
    int64_t rest_npoints, deform_npoints;
    const float *rest_P;
    const float *deform_P;
    /* outputs */
    float *P_out;          /* npoints x 3 */
    float *fd_falloff;     /* npoints, or NULL */
    float *Cd;             /* npoints x 3, or NULL (always white, :386-388) */
    /* inputs 3..: blendshapes of the morph-space pass (:175-213, 444-482); all optional */
    int64_t nshapes;                 /* connected inputs beyond the deformed rig */
    const float *const *shapes_P;    /* nshapes arrays, shapes_npoints[s] x 3 each */
    const int64_t *shapes_npoints;   /* a count different from npoints drops the shape with a warning (:200-204) */
    const float *rest;               /* input 0's `rest` point attribute (npoints x 3) or NULL (:178) */
    int rest_changed;                /* what checkChangedSourceFlags(0) reports: the rest pose changed (:180-184) */
    int blends_changed;              /* ... and for any of inputs 3.. (:186-194) */
    double *weights;                 /* out: the detail array `weights` (:474-481), room for nshapes, or NULL */
    int64_t *weights_count;          /* out: entries written; 0 when the morph pass did not run; or NULL */
    /* The rest rig (input 1) is the one of the previous cook -- what checkChangedSourceFlags(1)
     * tells the wrapper.  Then only the deltas are new and the engine reuses its factorisation
     * (fd_set_deltas); 0 = rebuild, as the reference does every cook (B12). */
    int rig_rest_unchanged;
    /* The arrays of input 0 (P, dist2, tangent frames) are the ones of the previous cook -- their
     * data IDs did not change.  Then the engine's device-resident copy (fd_mesh_set) is used and
     * nothing of the mesh is uploaded; 0 = upload. */
    int mesh_unchanged;
    /* ---- ProximityCapture's inputs (src/capture.cpp:10-44, 101-141; cook :301-322) -- all optional.
     * When `dist2` above is NULL and these are present, the cook captures on the device exactly
     * where the reference does: on the first cook and whenever the rest pose (input 0) or the rest
     * rig (input 1) changed -- NOT when only radius / maxedges / dofalloff changed (the author's
     * FIXME at :309, kept) -- and gates / falls off with the result.
     *   edge_offsets / edge_neighbours   the mesh's edges as a CSR adjacency (what GQ_Detail::
     *                                    groupEdgePoints walks): offsets[npoints + 1], neighbours[offsets[npoints]]
     *   rig_tris                         the rest rig's surface as rig_ntris triangles, 9 floats each
     *                                    (what GU_RayIntersect::minimumPoint searches)
     *   dist2_out                        out: the captured attribute, npoints floats, or NULL */
    const int64_t *edge_offsets;
    const int *edge_neighbours;
    int64_t rig_ntris;
    const float *rig_tris;
    float *dist2_out;
} fdsop_geo;

fdsop_node *fdsop_create(const fd_config *cfg);
void fdsop_destroy(fdsop_node *node);
/* Parm access by token ("radius", "model", ...).  Unknown token: FD_E_INVALID. */
int fdsop_set_float(fdsop_node *node, const char *token, int index, double value);
int fdsop_set_int(fdsop_node *node, const char *token, int value);
int fdsop_set_string(fdsop_node *node, const char *token, const char *value);
int fdsop_get_float(const fdsop_node *node, const char *token, int index, double *value);
int fdsop_get_int(const fdsop_node *node, const char *token, int *value);
int fdsop_parm_count(void);
const char *fdsop_parm_token(int i);
/* Cook.  Returns the FDSOP_* severity.  Messages: "severity\ttext\n" lines. */
int fdsop_cook(fdsop_node *node, const fdsop_geo *geo);
const char *fdsop_messages(const fdsop_node *node);
/* The clamped values the last cook actually used (A1), and the engine underneath. */
int fdsop_effective_float(const fdsop_node *node, const char *token, double *value);
fd_ctx *fdsop_engine(fdsop_node *node);

/* ---- all frames of a shot through the node in one call ------------------------
 * One mesh, one rest rig, F deformed rigs (input 2 at F times).  `geo` supplies everything that does not change over the
 * shot -- the mesh and its attributes, the rest rig and the point counts, the capture inputs, the blendshapes, the change
 * flags; geo->deform_P, geo->P_out and geo->fd_falloff are not read and may be NULL; geo->Cd, dist2_out, weights and
 * weights_count are written once.  fdsop_shot (additive: the ABI version stays; fdsop_geo is unchanged) carries the frames.
 *
 * Contract: frame k is the k-th of F consecutive fdsop_cook calls on this node.  Call 0 uses geo's flags as given; calls
 * k >= 1 use rig_rest_unchanged = mesh_unchanged = 1 and rest_changed = blends_changed = 0; each call's deform_P and outputs
 * are the shot's k-th.  Hence:
 *   Capture runs where the first cook would run it, and never again.
 *   Morph space: the pass applies to the first frame that reaches it while fd_morph_is_computed is false -- frame 0 -- and
 *     every later frame gets the reference's warning (:448-452, the quirk fdsop_cook keeps).  `weights` is that frame's.
 *   Clamps and fdsop_effective_float values are the single cook's.
 *   Gating: a gated vertex is bit-identical to P in every frame, and its fd_falloff entry is 0.
 *   Precision, per frame: with `precision` = 0 frame k is evaluated in fp64 exactly when fd_fp32_holds(report_k, 1e-5) is 0,
 *     its neighbours stay fp32, and the warning comes once per rig; 1: every frame fp64; 2: every frame fp32.
 *   Errors: a shot-wide error (bad arrays, differing rig counts, no engine, a capture failure, a model the engine refuses)
 *     makes every P_out[k] the copy of input 0 and every frame_severity[k] an error, with fdsop_cook's text.  A failure that
 *     belongs to a frame passes that frame through and the others are cooked.
 *   Node state: afterwards a following fdsop_cook(..., rig_rest_unchanged = 1, mesh_unchanged = 1) is correct.
 *   F = 1 IS fdsop_cook, bit for bit (positions, fall-off, messages apart from the frame prefix).
 * Messages: lines a single cook emits for the mesh, the parms or the capture come once, as in fdsop_cook.  Lines that belong
 * to a frame read "<severity>\tframe <k>: <text>\n": `Termination type`, a solve failure, a failed evaluation, the fp64
 * warning (on the first frame that needs it) and the morph warning of frames >= 1.  The return value is the worst severity;
 * frame_severity[k] is what the k-th cook would have returned.
 *
 * How the frames are cooked.  Groups of up to FD_MAX_BATCH frames, on contexts and batch objects the node owns (created on
 * first use, re-created with the engine when `device` changes, freed in fdsop_destroy; a tail group has a batch object of its
 * size over the first contexts -- everything of a shot is enqueued on ONE stream and every group's build is collected before
 * the next batch object touches the contexts).  The rest rig and all frames' fp32 deltas (deform - rest, :278) go to the
 * device as one block; every context of a group gets the SAME rest pointer (fd_batch_set_points_dev).  One batched build per
 * group, then the group is evaluated on the engine's device-resident mesh (fd_mesh_set's arrays, the captured dist2) by ONE
 * launch: fd_batch_deform_shared_dev / _ml_dev (fp32), _fp64_dev / _ml_fp64_dev (fp64), and their *_vectors_* forms when
 * transport tables are given; those calls' own fall-backs cover what they do not take.  A group in which only some frames
 * need fp64 is evaluated in fp32 as a whole -- so an fp32 frame's bits do not depend on which neighbours needed fp64 -- and
 * the frames that need it are then evaluated again in fp64, per context, over their outputs.  Results are staged in HBM in
 * two sets: group g is downloaded on a stream of its own while group g + 1 is built and evaluated.  Page-locked output arrays
 * are copied asynchronously, pageable ones through the runtime's staging.  When the staging sets cannot be allocated the
 * groups get smaller (halved), and with no room for one frame the shot is cooked frame by frame.
 * The contexts, the batch objects and the staging sets (two sets of 16 B per vertex and frame of a group, 36 B more per
 * transported vector) stay with the node for the next shot and go in fdsop_destroy.
 * Shared builds (one factorisation of the rest rig per group): QNN (fd_batch_set_shared_lu) from 8 frames a group up to 256
 * control points and from 16 frames above, where DESIGN 4.2i measured it ahead; off for the thin-plate family (4.2f: slower
 * as latency) and for the multilayer model (4.2h: not measured yet).
 * Sequential route: F = 1 (by contract), an empty mesh, a group with a model that did not solve (its frames then report as
 * their own cooks do), and no memory for staging take consecutive fdsop_cook calls inside this call.  Nothing else does:
 * at 1M vertices and 256 control points every F >= 2 measured at or ahead of F cooks with rig and mesh unchanged, for the
 * node's defaults, kernel = 1 and model = 1, page-locked and pageable outputs (the least: 2 QNN frames, 1.01x .. 1.10x over
 * two runs; 1.8x .. 3.4x at 32 frames).
 * Transport: N_out / tangentu_out / tangentv_out, each NULL or F arrays of npoints x 3, receive geo->N / tangentu / tangentv
 * carried through each frame's deformation by fd_vectors' rules (geo's attribute must be there: "Invalid geometry arrays."
 * otherwise); a frame that is passed through gets them unchanged.  NULL tables: the attributes are left alone, as in the
 * reference. */
typedef struct fdsop_shot {
    int struct_size;                 /* = sizeof(fdsop_shot); smaller: error before anything else */
    int nframes;                     /* F >= 1, any count */
    const float *const *deform_P;    /* F arrays, geo->deform_npoints x 3: input 2 at each frame */
    float *const *P_out;             /* F arrays, npoints x 3 */
    float *const *fd_falloff;        /* F arrays of npoints, or NULL */
    int *frame_severity;             /* out, F entries, or NULL */
    float *const *N_out, *const *tangentu_out, *const *tangentv_out;
} fdsop_shot;
int fdsop_cook_shot(fdsop_node *node, const fdsop_geo *geo, const fdsop_shot *shot);
/* One line per group of the last shot: "first_frame\tnframes\tbuild\teval32\tn32\teval64\tn64\n".  build: the shared
 * build's kernel name, or "" for per-context builds.  eval32 / eval64: what fd_shared_kernel_name / fd_shared_ml_kernel_name
 * and fd_shared_fp64_kernel_name / fd_shared_ml_fp64_kernel_name answer for the group's launch of that precision, or ""
 * where the frames went per context (a sequential group; the fp64 frames of a mixed group).  n32 / n64: the frames
 * delivered in each precision. */
const char *fdsop_shot_paths(const fdsop_node *node);

#ifdef __cplusplus
}
#endif
#endif /* FACEDEFORM_HIP_H */
