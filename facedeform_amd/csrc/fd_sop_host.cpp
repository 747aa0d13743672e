// fd_sop_host.cpp -- HDK-free mirror of SOP_FaceDeform's cook over plain arrays.
//
// Same parm tokens, defaults and clamps as the reference's PRM_Template list
// (reference src/SOP_FaceDeform.cpp:99-137), same cook order and the same
// error / warning / message texts (:215-489), with the ALGLIB call sequence and
// the evaluation loop replaced by the fd_* C ABI.  The HDK wrapper
// (hdk/SOP_FaceDeformHip.cpp) gathers GU_Detail attributes into an fdsop_geo
// and calls fdsop_cook; the tests drive the same entry points through ctypes.
//
// The morph-space pass (setupBlends :175-213, the loop at :444-482, DirectBSEdit in
// src/dbse.cpp) runs on the device through fd_morph_*.  ProximityCapture (:301-322,
// src/capture.cpp) runs on the device too, through fd_mesh_capture, when the caller hands over
// what it needs (the mesh's edge adjacency and the rig's triangles) and no dist2 array of its
// own; cached across cooks exactly as the reference caches m_mesh_capture.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/facedeform_hip.h"
#include "fd_shot_dev.h"

namespace {

enum ParmType { P_STRING, P_ORD, P_FLOAT, P_INT, P_TOGGLE, P_FLOAT2 };

struct ParmDef {
    const char *token;
    ParmType type;
    double def0, def1;
    const char *label;
};

// reference src/SOP_FaceDeform.cpp:99-137; the last four are additions that the
// survey allows (new parms, nothing renamed or removed).
const ParmDef kParms[] = {
    {"group", P_STRING, 0, 0, "Group"},
    {"model", P_ORD, 0, 0, "Model"},                       // 0 QNN, 1 Multilayer   (:48-53)
    {"term", P_ORD, 0, 0, "RBF Term"},                     // 0 Linear, 1 Constant, 2 Zero (:55-61)
    {"qcoef", P_FLOAT, 1, 0, "Q (Smoothness)"},
    {"zcoef", P_FLOAT, 5, 0, "Z (Deviation)"},
    {"radius", P_FLOAT, 1, 0, "Radius"},
    {"maxedges", P_INT, 4, 0, "Max edges"},
    {"layers", P_INT, 4, 0, "Layers"},
    {"lambda", P_FLOAT, 0.1, 0, "Lambda"},
    {"tangent", P_TOGGLE, 0, 0, "Tangent space"},
    {"morphspace", P_TOGGLE, 0, 0, "Blendshapes subspace"},
    {"doclampweight", P_TOGGLE, 0, 0, "Clamp weights"},
    {"weightrange", P_FLOAT2, 0, 1, "Range"},
    {"dofalloff", P_TOGGLE, 0, 0, "Falloff"},
    {"falloffradius", P_FLOAT, 1, 0, "Falloff radius"},
    {"falloffrate", P_FLOAT, 1, 0, "Falloff rate (exponent)"},
    // -- additions
    {"kernel", P_ORD, 0, 0, "Kernel"},        // 0 = per `model` (Gaussian), 1 thin-plate, 2 biharmonic, 3 cubic
    {"smoothing", P_FLOAT, 0, 0, "Smoothing"},  // diagonal lambda for kernel != 0 and for QNN
    {"precision", P_ORD, 0, 0, "Evaluation precision"},  // 0 fp32 while its error estimate holds the tolerance (else fp64 for that cook), 1 fp64, 2 fp32 always
    {"device", P_INT, -1, 0, "GPU device"},
};
constexpr int kNumParms = (int)(sizeof(kParms) / sizeof(kParms[0]));

int find_parm(const char *token)
{
    if (!token) return -1;
    for (int i = 0; i < kNumParms; ++i)
        if (strcmp(kParms[i].token, token) == 0) return i;
    return -1;
}

template <typename T>
T sys_max(T a, T b) { return a > b ? a : b; }

}  // namespace

struct fdsop_node {
    fd_config cfg{};
    fd_ctx *engine = nullptr;
    // what the engine's device-resident mesh (fd_mesh_set) was uploaded with
    bool mesh_had_dist2 = false, mesh_had_frames = false;
    // m_mesh_capture.isInitialized() && isCaptured() (:310-311): the device-resident dist2 is the
    // product of a capture that is still valid
    bool captured = false;
    fd_morph *morph = nullptr;        // m_direct_blends (:SOP_FaceDeform.hpp), lives as long as the node
    int morph_device = -2;
    double fval[kNumParms][2];
    std::string sval[kNumParms];
    std::string messages;
    int severity = FDSOP_OK;
    // clamped values of the last cook (A1)
    float e_qcoef = 0, e_zcoef = 0, e_radius = 0, e_lambda = 0;
    int e_layers = 0, e_maxedges = 0;
    int engine_precision = -1, engine_device = -2;
    bool fp64_warned = false;         // the "evaluating in fp64" warning has been given for the current rest rig (once per rig, not per cook)
    bool last_cook_fp64 = false;      // the last fdsop_cook evaluated in fp64
    // fdsop_cook_shot: the frames' own contexts (up to FD_MAX_BATCH, created on first use), a batch object per group size over
    // the first n of them, and the device side (streams, control tables, staging sets).  All of one device with the engine;
    // freed before the engine goes.
    fd_ctx *shot_ctx[FD_MAX_BATCH] = {};
    int shot_nctx = 0;
    fd_batch *shot_batch[FD_MAX_BATCH + 1] = {};
    fd_shot_dev *shot_dev = nullptr;
    // a batched shot built its models on another rest rig than the one the engine factorised last: the engine's factorisation
    // must not be reused by fd_set_deltas until the engine has seen the rig itself
    bool engine_rig_stale = false;
    std::string shot_paths;

    void free_shot()
    {
        for (fd_batch *&b : shot_batch) { if (b) fd_batch_destroy(b); b = nullptr; }
        for (int i = 0; i < shot_nctx; ++i) { fd_destroy(shot_ctx[i]); shot_ctx[i] = nullptr; }
        shot_nctx = 0;
        if (shot_dev) { fd_shot_dev_destroy(shot_dev); shot_dev = nullptr; }
    }

    void add(int sev, const char *text)
    {
        const char *name = sev == FDSOP_ERROR ? "error" : (sev == FDSOP_WARNING ? "warning" : "message");
        messages += name;
        messages += '\t';
        messages += text;
        messages += '\n';
        if (sev > severity) severity = sev;
    }
    // ordinal parms are strings parsed with atoi, as reference :247-248
    int ord(int idx) const { return atoi(sval[idx].c_str()); }
};

extern "C" {

int fdsop_parm_count(void) { return kNumParms; }
const char *fdsop_parm_token(int i) { return (i >= 0 && i < kNumParms) ? kParms[i].token : nullptr; }

fdsop_node *fdsop_create(const fd_config *cfg)
{
    fdsop_node *n = new (std::nothrow) fdsop_node();
    if (!n) return nullptr;
    if (cfg) n->cfg = *cfg;
    else { memset(&n->cfg, 0, sizeof(n->cfg)); n->cfg.device = -1; }
    for (int i = 0; i < kNumParms; ++i) {
        n->fval[i][0] = kParms[i].def0;
        n->fval[i][1] = kParms[i].def1;
        if (kParms[i].type == P_ORD) n->sval[i] = std::to_string((int)kParms[i].def0);
    }
    n->fval[find_parm("device")][0] = n->cfg.device;
    n->sval[find_parm("precision")] = std::to_string(n->cfg.eval_precision == FD_EVAL_FP64 ? 1 : 0);
    return n;
}

void fdsop_destroy(fdsop_node *node)
{
    if (!node) return;
    node->free_shot();
    if (node->engine) fd_destroy(node->engine);
    if (node->morph) fd_morph_destroy(node->morph);
    delete node;
}

int fdsop_set_float(fdsop_node *node, const char *token, int index, double value)
{
    const int i = find_parm(token);
    if (!node || i < 0 || index < 0 || index > 1) return FD_E_INVALID;
    if (kParms[i].type == P_STRING) return FD_E_INVALID;
    if (index == 1 && kParms[i].type != P_FLOAT2) return FD_E_INVALID;
    node->fval[i][index] = value;
    if (kParms[i].type == P_ORD) node->sval[i] = std::to_string((int)value);
    return FD_OK;
}

int fdsop_set_int(fdsop_node *node, const char *token, int value)
{
    return fdsop_set_float(node, token, 0, (double)value);
}

int fdsop_set_string(fdsop_node *node, const char *token, const char *value)
{
    const int i = find_parm(token);
    if (!node || i < 0 || !value) return FD_E_INVALID;
    if (kParms[i].type != P_STRING && kParms[i].type != P_ORD) return FD_E_INVALID;
    node->sval[i] = value;
    if (kParms[i].type == P_ORD) node->fval[i][0] = atoi(value);
    return FD_OK;
}

int fdsop_get_float(const fdsop_node *node, const char *token, int index, double *value)
{
    const int i = find_parm(token);
    if (!node || i < 0 || !value || index < 0 || index > 1) return FD_E_INVALID;
    *value = node->fval[i][index];
    return FD_OK;
}

int fdsop_get_int(const fdsop_node *node, const char *token, int *value)
{
    const int i = find_parm(token);
    if (!node || i < 0 || !value) return FD_E_INVALID;
    *value = kParms[i].type == P_ORD ? node->ord(i) : (int)node->fval[i][0];
    return FD_OK;
}

const char *fdsop_messages(const fdsop_node *node) { return node ? node->messages.c_str() : ""; }

fd_ctx *fdsop_engine(fdsop_node *node) { return node ? node->engine : nullptr; }

int fdsop_effective_float(const fdsop_node *node, const char *token, double *value)
{
    if (!node || !token || !value) return FD_E_INVALID;
    if (!strcmp(token, "qcoef")) *value = node->e_qcoef;
    else if (!strcmp(token, "zcoef")) *value = node->e_zcoef;
    else if (!strcmp(token, "radius")) *value = node->e_radius;
    else if (!strcmp(token, "lambda")) *value = node->e_lambda;
    else if (!strcmp(token, "layers")) *value = node->e_layers;
    else if (!strcmp(token, "maxedges")) *value = node->e_maxedges;
    else return FD_E_INVALID;
    return FD_OK;
}

// What a cook settles before it turns to the deformed rig: the clamped parms, the morph engine, the GPU engine, input 0 on the
// device, the capture.  fdsop_cook and fdsop_cook_shot run this part once, from the same code.
struct CookSetup {
    int model_index, term_index, layers, tangent_disp, morph_space, max_edges, kernel_ext, precision_parm, precision, device, M;
    float qcoef, zcoef, radius, lambda, falloffrate;
    double smoothing;
    bool do_tangent_disp, have_blends, morph_inited_this_cook, use_capture, mesh_ready;
    const float *rest_attr;
    int dofalloff_parm;
};

// :228-322.  false: the cook stops here (the message has been added).
static bool cook_setup(fdsop_node *node, const fdsop_geo *geo, CookSetup &cs)
{
    // :228-234
    if (geo->rest_npoints != geo->deform_npoints) {
        node->add(FDSOP_ERROR, "Rest and deform geometry should match.");
        return false;
    }

    // :244-263 -- SYSmax(0.1, fpreal) is evaluated in double, then narrowed to float
    const int model_index = cs.model_index = node->ord(find_parm("model"));
    cs.term_index = node->ord(find_parm("term"));
    const float qcoef = cs.qcoef = (float)sys_max(0.1, node->fval[find_parm("qcoef")][0]);
    const float zcoef = cs.zcoef = (float)sys_max(0.1, node->fval[find_parm("zcoef")][0]);
    const float radius = cs.radius = (float)sys_max(0.01, node->fval[find_parm("radius")][0]);
    const int layers = cs.layers = sys_max(1, (int)node->fval[find_parm("layers")][0]);
    const float lambda = cs.lambda = (float)sys_max(0.01, node->fval[find_parm("lambda")][0]);
    const int tangent_disp = cs.tangent_disp = (int)node->fval[find_parm("tangent")][0];
    const int morph_space = cs.morph_space = (int)node->fval[find_parm("morphspace")][0];
    const int max_edges = cs.max_edges = sys_max(1, (int)node->fval[find_parm("maxedges")][0]);
    cs.falloffrate = (float)node->fval[find_parm("falloffrate")][0];
    node->e_qcoef = qcoef; node->e_zcoef = zcoef; node->e_radius = radius; node->e_lambda = lambda;
    node->e_layers = layers; node->e_maxedges = max_edges;
    cs.kernel_ext = node->ord(find_parm("kernel"));
    cs.smoothing = node->fval[find_parm("smoothing")][0];
    const int precision_parm = cs.precision_parm = node->ord(find_parm("precision"));
    const int precision = cs.precision = precision_parm == 1 ? FD_EVAL_FP64 : FD_EVAL_FP32;
    const int device = cs.device = (int)node->fval[find_parm("device")][0];
    (void)model_index;

    const int M = cs.M = (int)geo->rest_npoints;

    // :289-298
    const bool do_tangent_disp = cs.do_tangent_disp = tangent_disp && geo->tangentu && geo->tangentv && geo->N;
    if (tangent_disp && !do_tangent_disp)
        node->add(FDSOP_WARNING, "Append PolyFrameSOP and enable tangent[u/v] and N attribute to allow tangent displacement.");

    // :323-329 -- morph space needs blendshapes on inputs 3..; setupBlends (:175-213)
    const bool have_blends = cs.have_blends = geo->nshapes > 0 && geo->shapes_P && geo->shapes_npoints;
    if (geo->weights_count) *geo->weights_count = 0;
    // the `rest` attribute: input 0's own unless the rest pose changed or there is none, in
    // which case it is a copy of the incoming P (:178-184)
    cs.rest_attr = (geo->rest && !geo->rest_changed) ? geo->rest : geo->P;
    bool &morph_inited_this_cook = cs.morph_inited_this_cook = false;
    if (morph_space && have_blends) {
        if (!node->morph || node->morph_device != device) {
            if (node->morph) { fd_morph_destroy(node->morph); node->morph = nullptr; }
            fd_config mcfg = node->cfg;
            mcfg.struct_size = (int)sizeof(fd_config);
            mcfg.device = device;
            node->morph = fd_morph_create(&mcfg);
            node->morph_device = device;
        }
        if (node->morph && (geo->blends_changed || !fd_morph_is_initialised(node->morph))) {
            std::vector<const float *> shapes;
            bool mismatch = false;
            for (int64_t sidx = 0; sidx < geo->nshapes; ++sidx) {
                if (geo->shapes_npoints[sidx] != geo->npoints || !geo->shapes_P[sidx]) { mismatch = true; continue; }
                shapes.push_back(geo->shapes_P[sidx]);
            }
            if (mismatch)   // :201-203
                node->add(FDSOP_WARNING, "Some blendshapes don't match rest pose point count. Ignoring them.");
            // DirectBSEdit::init measures the shapes against the mesh's CURRENT P (dbse.cpp:22), not
            // against the rest attribute
            if (geo->npoints <= 0 ||
                fd_morph_init(node->morph, geo->npoints, (int)shapes.size(), geo->P, shapes.empty() ? nullptr : shapes.data()) != FD_OK)
                node->add(FDSOP_WARNING, "Can't proceed with morph space deformation. Ingoring it.");   // :209-211
            else
                morph_inited_this_cook = true;
        }
    } else if (morph_space) {
        node->add(FDSOP_WARNING, "No blendshapes found. Ignoring morphspace deformation.");
    }

    // engine (re)creation when the device changed (the precision is set per cook, below)
    if (!node->engine || node->engine_device != device) {
        node->free_shot();             // the shot's contexts and streams are of the engine's device
        if (node->engine) { fd_destroy(node->engine); node->engine = nullptr; }
        node->engine_rig_stale = false;
        fd_config cfg = node->cfg;
        cfg.struct_size = (int)sizeof(fd_config);
        cfg.device = device;
        cfg.eval_precision = precision;
        node->engine = fd_create(&cfg);
        node->engine_precision = precision;
        node->engine_device = device;
        if (!node->engine) {
            std::string t = std::string("Can't create the GPU deformation engine: ") + fd_last_error(nullptr);
            node->add(FDSOP_ERROR, t.c_str());
            return false;
        }
    }
    fd_ctx *ctx = node->engine;

    // :301-322 -- proximity capture, where the reference has it: before the model.  Input 0's arrays
    // go to the device first (fd_mesh_set; skipped when the caller vouches they are the previous
    // cook's), then -- with no dist2 array from the caller but the capture's own inputs at hand --
    // islands and squared distances are produced there.  Re-captured on the first cook and when the
    // rest pose or the rest rig changed; NOT when radius / maxedges / dofalloff alone changed (the
    // FIXME at :309: kept, B12).
    const int dofalloff_parm = cs.dofalloff_parm = (int)node->fval[find_parm("dofalloff")][0];
    const bool want_d2 = geo->dist2 != nullptr;
    const bool use_capture = cs.use_capture = !want_d2 && geo->edge_offsets && geo->rig_ntris >= 0 && (geo->rig_ntris == 0 || geo->rig_tris);
    cs.mesh_ready = false;
    if (geo->npoints > 0) {
        // (a mesh that still carries an earlier cook's CAPTURED dist2 is not reusable once the capture's inputs are gone:
        // the reference then applies neither radius nor fall-off, :396-399 -- fd_mesh_set drops the stale attribute)
        const bool reuse = geo->mesh_unchanged && fd_mesh_size(ctx) == geo->npoints &&
                           node->mesh_had_dist2 == want_d2 && node->mesh_had_frames == do_tangent_disp &&
                           !(node->captured && !use_capture);
        int mrc = FD_OK;
        if (!reuse) {
            mrc = fd_mesh_set(ctx, geo->npoints, geo->P, geo->dist2, do_tangent_disp ? geo->tangentu : nullptr,
                              do_tangent_disp ? geo->tangentv : nullptr, do_tangent_disp ? geo->N : nullptr);
            node->mesh_had_dist2 = want_d2;
            node->mesh_had_frames = do_tangent_disp;
            node->captured = false;
        }
        if (mrc != FD_OK) {
            std::string t = std::string("GPU deformation failed: ") + fd_last_error(ctx);
            node->add(FDSOP_ERROR, t.c_str());
            return false;
        }
        cs.mesh_ready = true;
        if (!use_capture) node->captured = false;
        if (use_capture && (!node->captured || !geo->rig_rest_unchanged)) {
            // capture(max_edges, radius, dofalloff, falloffrate) (:317): radius^2 is the search bound
            mrc = fd_mesh_capture(ctx, geo->edge_offsets, geo->edge_neighbours, M > 0 ? M : 0, geo->rest_P, max_edges,
                                  (int)geo->rig_ntris, geo->rig_tris, radius * radius, dofalloff_parm, nullptr);
            if (mrc != FD_OK) {
                node->add(FDSOP_ERROR, "Can't capture geometry with a rig!");     // :318
                return false;
            }
            node->captured = true;
        }
    }
    return true;
}

// :342-361 -- model select on one context; `kernel` (addition) overrides the Gaussian family.
static int cook_select_model(fd_ctx *ctx, const CookSetup &cs)
{
    const int kernel_ext = cs.kernel_ext, model_index = cs.model_index, term_index = cs.term_index, layers = cs.layers;
    const float radius = cs.radius, lambda = cs.lambda, qcoef = cs.qcoef, zcoef = cs.zcoef;
    const double smoothing = cs.smoothing;
    int rc = FD_OK;
    if (kernel_ext == 1 || kernel_ext == 2 || kernel_ext == 3) {
        const int kind = kernel_ext == 1 ? FD_KERNEL_THIN_PLATE : (kernel_ext == 2 ? FD_KERNEL_BIHARMONIC : FD_KERNEL_CUBIC);
        const double p[1] = {smoothing};
        rc = fd_set_kernel(ctx, kind, p, 1);
    } else if (model_index == 1) {   // ALGLIB_MODEL_ML: rbfsetalgomultilayer(model, radius, layers, lambda)
        // the engine's multilayer model takes up to 8 layers: beyond that the radius has shrunk
        // 256-fold and the remaining layers see only lambda^8 of the residual
        const double p[3] = {(double)radius, (double)(layers < 8 ? layers : 8), (double)lambda};
        rc = fd_set_kernel(ctx, FD_KERNEL_GAUSSIAN_ML, p, 3);
    } else {                         // ALGLIB_MODEL_QNN: rbfsetalgoqnn(model, qcoef, zcoef)
        const double p[3] = {(double)qcoef, (double)zcoef, smoothing};
        rc = fd_set_kernel(ctx, FD_KERNEL_GAUSSIAN_QNN, p, 3);
    }
    // :351-361 -- any other ordinal leaves ALGLIB's default (linear) in place
    const int term = (term_index == 1) ? FD_TERM_CONST : (term_index == 2 ? FD_TERM_ZERO : FD_TERM_LINEAR);
    if (rc == FD_OK) rc = fd_set_term(ctx, term);
    return rc;
}

// The cook: reference src/SOP_FaceDeform.cpp:215-489, step for step.
int fdsop_cook(fdsop_node *node, const fdsop_geo *geo)
{
    if (!node || !geo) return FDSOP_ERROR;
    node->messages.clear();
    node->severity = FDSOP_OK;
    if (geo->npoints < 0 || (geo->npoints > 0 && (!geo->P || !geo->P_out)) || !geo->rest_P || !geo->deform_P) {
        node->add(FDSOP_ERROR, "Invalid geometry arrays.");
        return node->severity;
    }
    // duplicatePointSource(0) (:226): the output starts as a copy of input 0.  On the success
    // path fd_deform writes every point of P_out from P (gated points are copied through), so
    // the 12 B/point host copy is only made where the cook stops early.
    struct PassThrough {
        const fdsop_geo *g; bool armed;
        ~PassThrough() {
            if (armed && g->P_out != g->P && g->npoints > 0)
                memcpy(g->P_out, g->P, sizeof(float) * 3 * (size_t)g->npoints);
        }
    } pass{geo, true};

    CookSetup cs;
    if (!cook_setup(node, geo, cs)) return node->severity;
    const int M = cs.M, precision = cs.precision, precision_parm = cs.precision_parm, morph_space = cs.morph_space,
              dofalloff_parm = cs.dofalloff_parm;
    const float radius = cs.radius, falloffrate = cs.falloffrate;
    const bool have_blends = cs.have_blends, morph_inited_this_cook = cs.morph_inited_this_cook, use_capture = cs.use_capture,
               mesh_ready = cs.mesh_ready;
    const float *rest_attr = cs.rest_attr;
    fd_ctx *ctx = node->engine;
    // :268-287 -- M x 6 table: rest position and fp32 delta
    std::vector<float> delta((size_t)(M > 0 ? M : 0) * 3);
    for (int i = 0; i < M; ++i)
        for (int c = 0; c < 3; ++c) delta[3 * (size_t)i + c] = geo->deform_P[3 * (size_t)i + c] - geo->rest_P[3 * (size_t)i + c];

    // :342-361 -- the model.  (Set before the points here: an unchanged kernel / term leaves the engine's factorisation in
    // place, and fd_set_deltas below depends on that; every failure ends in the same message as at :337-340.)
    int rc = cook_select_model(ctx, cs);
    // :331-340 -- rbfcreate + rbfsetpoints.  The reference rebuilds its model on every cook (B12);
    // when the caller vouches that the rest rig has not changed since the last cook
    // (checkChangedSourceFlags(1) in the wrapper) only the deltas are new and the engine reuses
    // its factorisation -- bit-identical weights, half the cook.  Anything that invalidates it
    // (first cook, another M, kernel or term) falls back to the full path.
    if (rc == FD_OK) {
        rc = FD_E_NOT_BUILT;
        if (M > 0 && geo->rig_rest_unchanged && !node->engine_rig_stale) rc = fd_set_deltas(ctx, delta.data(), M);
        if (rc != FD_OK) {
            rc = M > 0 ? fd_set_points(ctx, geo->rest_P, delta.data(), M) : FD_E_INVALID;
            if (rc == FD_OK) node->engine_rig_stale = false;
        }
    }
    if (rc != FD_OK) {
        node->add(FDSOP_ERROR, "Can't build RBF model.");
        return node->severity;
    }
    // :363-368
    fd_report report;
    memset(&report, 0, sizeof(report));
    rc = fd_build(ctx, &report);
    if (report.terminationtype != 1 || rc != FD_OK) {
        node->add(FDSOP_ERROR, "Can't solve the problem.");
        return node->severity;
    }
    // The reference evaluates in fp64 inside ALGLIB (:404-439); the fp32 evaluation has an absolute error floor that the
    // build reports (fd_report.fp32_error).  Where that floor exceeds the reference's 1e-5 of the smallest displacements of
    // the control table, this cook is evaluated in fp64 -- unless the artist asked for fp32 outright (precision = 2).
    int cook_precision = precision;
    if (!geo->rig_rest_unchanged) node->fp64_warned = false;       // another rest rig: say it again if it applies
    if (precision_parm == 0 && !fd_fp32_holds(&report, 1e-5)) {
        cook_precision = FD_EVAL_FP64;
        if (!node->fp64_warned) {                                  // once per rig: an animated shot cooks the same rig every frame
            char t[240];
            snprintf(t, sizeof(t), "fp32 evaluation would not hold 1e-5 of this rig's displacements (error ~%.2g, smallest delta %.2g): "
                                   "evaluating in fp64.", report.fp32_error, report.delta_min);
            node->add(FDSOP_WARNING, t);
            node->fp64_warned = true;
        }
    }
    fd_set_eval_precision(ctx, cook_precision);
    node->last_cook_fp64 = cook_precision == FD_EVAL_FP64;
    // :370-373
    char info[200];
    snprintf(info, sizeof(info), "Termination type: %d, Iterations: %d", report.terminationtype, report.iterationscount);
    node->add(FDSOP_MESSAGE, info);

    // :386-388 -- Cd is added white and never written again
    if (geo->Cd)
        for (int64_t i = 0; i < geo->npoints * 3; ++i) geo->Cd[i] = 1.f;
    // :396-399
    if (!geo->dist2 && !(use_capture && node->captured))
        node->add(FDSOP_WARNING, "Can't find distance capture attribute. Won't apply radius nor falloff.");
    // :401 -- a fresh float attribute reads 0 until written
    if (geo->fd_falloff && geo->npoints > 0) memset(geo->fd_falloff, 0, sizeof(float) * (size_t)geo->npoints);
    const float radius_sqrt = radius * radius;   // :402 (a square, despite the name)

    // :404-439.  The mesh arrays go to the device through fd_mesh_set; when the caller vouches
    // that input 0 is the one of the previous cook (same data IDs) the upload is skipped and the
    // cook moves only its results over the host link.
    pass.armed = false;
    rc = FD_OK;
    if (mesh_ready) rc = fd_deform_mesh(ctx, geo->P_out, geo->fd_falloff, radius_sqrt, falloffrate);
    if (rc == FD_OK && geo->dist2_out && use_capture && node->captured)
        rc = fd_mesh_get_dist2(ctx, geo->dist2_out);
    if (rc != FD_OK) {
        std::string t = std::string("GPU deformation failed: ") + fd_last_error(ctx);
        node->add(FDSOP_ERROR, t.c_str());
        pass.armed = true;
        return node->severity;
    }

    // :444-482 -- morph-space reprojection of the deformed mesh
    if (morph_space && have_blends && node->morph && fd_morph_is_initialised(node->morph)) {
        // :448-450: the weights are computed only while isComputed() is false, i.e. on the first
        // cook after DirectBSEdit::init; every later cook with unchanged blendshapes takes the
        // warning branch below.  Kept as the reference has it.
        bool weights_done = false;
        const int S = fd_morph_shape_count(node->morph);
        if (!fd_morph_is_computed(node->morph)) {
            const int dofalloff = dofalloff_parm;
            const int doclampweight = (int)node->fval[find_parm("doclampweight")][0];
            const float falloffradius = (float)node->fval[find_parm("falloffradius")][0];
            const float weightrange[2] = {(float)node->fval[find_parm("weightrange")][0],
                                          (float)node->fval[find_parm("weightrange")][1]};
            std::vector<double> w((size_t)(S > 0 ? S : 1));
            // the engine already holds this cook's P as its rest pose when it was initialised in
            // this cook and input 0 has no rest attribute of its own; otherwise send the attribute
            const bool same_rest = morph_inited_this_cook && rest_attr == geo->P;
            int mrc = fd_morph_set_rest(node->morph, same_rest ? nullptr : rest_attr, 0);
            // computeWeights (dbse.cpp:39-60) + the displacement loop (:458-473), P_out in place
            if (mrc == FD_OK)
                mrc = fd_morph_apply(node->morph, geo->P_out, doclampweight ? weightrange : nullptr,
                                     dofalloff && falloffradius != 0.f, falloffradius, w.data());
            weights_done = mrc == FD_OK;
            if (weights_done) {   // :474-481, the detail array attribute `weights`
                if (geo->weights) memcpy(geo->weights, w.data(), sizeof(double) * (size_t)S);
                if (geo->weights_count) *geo->weights_count = S;
            }
        }
        if (!weights_done)
            node->add(FDSOP_WARNING, "Can't compute weights for morphspace deformation. Ingoring it.");   // :452
    }
    return node->severity;
}

// ---- fdsop_cook_shot ----------------------------------------------------------------------------------------------------
namespace {

int severity_of(const std::string &name) { return name == "error" ? FDSOP_ERROR : (name == "warning" ? FDSOP_WARNING : FDSOP_MESSAGE); }

bool starts_with(const std::string &s, const char *p) { return s.compare(0, strlen(p), p) == 0; }

// a line of one frame's cook that belongs to that frame (the others are the mesh's, the parms' or the capture's: once per shot)
bool is_frame_line(const std::string &text, int frame)
{
    if (starts_with(text, "Termination type:") || starts_with(text, "Can't solve the problem.") ||
        starts_with(text, "fp32 evaluation would not hold") || starts_with(text, "GPU deformation failed:"))
        return true;
    return frame >= 1 && starts_with(text, "Can't compute weights for morphspace deformation.");
}

// the messages of a shot as they add up
struct ShotLog {
    std::string text;
    std::vector<std::string> seen;       // shot-wide lines already in `text`
    int severity = FDSOP_OK;
    int common = FDSOP_OK;               // worst severity among the shot-wide lines
    void frame(int k, int sev, const std::string &t)
    {
        text += sev == FDSOP_ERROR ? "error" : (sev == FDSOP_WARNING ? "warning" : "message");
        text += "\tframe " + std::to_string(k) + ": " + t + "\n";
        if (sev > severity) severity = sev;
    }
    void shot(int sev, const std::string &t)
    {
        if (sev > severity) severity = sev;
        if (sev > common) common = sev;
        for (const std::string &s : seen) if (s == t) return;
        seen.push_back(t);
        text += sev == FDSOP_ERROR ? "error" : (sev == FDSOP_WARNING ? "warning" : "message");
        text += "\t" + t + "\n";
    }
    // the lines fdsop_cook left in the node: frame lines prefixed, the others once.  true: an ERROR among the shot-wide ones
    bool take(const fdsop_node *node, int k)
    {
        bool shot_error = false;
        size_t pos = 0;
        const std::string &m = node->messages;
        while (pos < m.size()) {
            size_t end = m.find('\n', pos);
            if (end == std::string::npos) end = m.size();
            const std::string line = m.substr(pos, end - pos);
            pos = end + 1;
            const size_t tab = line.find('\t');
            if (tab == std::string::npos) continue;
            const int sev = severity_of(line.substr(0, tab));
            const std::string t = line.substr(tab + 1);
            if (is_frame_line(t, k)) frame(k, sev, t);
            else { shot(sev, t); shot_error = shot_error || sev == FDSOP_ERROR; }
        }
        return shot_error;
    }
};

// frame k's transported vectors are the mesh's own
void shot_pass_vectors(const fdsop_geo *geo, const fdsop_shot *shot, int k)
{
    const size_t b3 = sizeof(float) * 3 * (size_t)(geo->npoints > 0 ? geo->npoints : 0);
    if (b3 == 0) return;
    const float *const src[3] = {geo->N, geo->tangentu, geo->tangentv};
    float *const *const dst[3] = {shot->N_out, shot->tangentu_out, shot->tangentv_out};
    for (int v = 0; v < 3; ++v)
        if (dst[v] && dst[v][k] && src[v] && dst[v][k] != src[v]) memcpy(dst[v][k], src[v], b3);
}

// frame k is the copy of input 0 (duplicatePointSource, :226)
void shot_pass_through(const fdsop_geo *geo, const fdsop_shot *shot, int k)
{
    if (geo->npoints > 0 && geo->P && shot->P_out[k] && shot->P_out[k] != geo->P)
        memcpy(shot->P_out[k], geo->P, sizeof(float) * 3 * (size_t)geo->npoints);
    shot_pass_vectors(geo, shot, k);
}

bool shot_transport(const fdsop_shot *shot) { return shot->N_out || shot->tangentu_out || shot->tangentv_out; }

void add_path(fdsop_node *node, int first, int n, const char *build, const char *e32, int n32, const char *e64, int n64)
{
    char line[320];
    snprintf(line, sizeof(line), "%d\t%d\t%s\t%s\t%d\t%s\t%d\n", first, n, build ? build : "", e32 ? e32 : "", n32, e64 ? e64 : "", n64);
    node->shot_paths += line;
}

// Frames [first, first + count) as consecutive fdsop_cook calls.  `fresh`: no cook of this shot has set the node up yet, so
// the first call here takes geo's flags as given; every other call has the flags of a cook that follows one.  Frame 0 alone
// writes Cd, dist2_out and the weights.  true: a shot-wide error ended the sequence (the remaining frames are passed through).
bool cook_frames_sequential(fdsop_node *node, const fdsop_geo *geo, const fdsop_shot *shot, int first, int count, bool fresh,
                            ShotLog &log)
{
    int n32 = 0, n64 = 0;
    bool stopped = false;
    for (int k = first; k < first + count; ++k) {
        if (stopped) {
            shot_pass_through(geo, shot, k);
            if (shot->frame_severity) shot->frame_severity[k] = FDSOP_ERROR;
            continue;
        }
        fdsop_geo g = *geo;
        g.deform_P = shot->deform_P[k];
        g.P_out = shot->P_out[k];
        g.fd_falloff = shot->fd_falloff ? shot->fd_falloff[k] : nullptr;
        if (!(fresh && k == first)) {
            g.rig_rest_unchanged = g.mesh_unchanged = 1;
            g.rest_changed = g.blends_changed = 0;
        }
        if (k != 0) {
            g.Cd = nullptr; g.dist2_out = nullptr;
            // (a later frame reaches the morph pass only if frame 0 did not: then the weights are that frame's)
            if (node->morph && fd_morph_is_computed(node->morph)) { g.weights = nullptr; g.weights_count = nullptr; }
        }
        const int sev = fdsop_cook(node, &g);
        if (shot->frame_severity) shot->frame_severity[k] = sev;
        const bool shot_error = log.take(node, k);
        if (sev != FDSOP_ERROR) (node->last_cook_fp64 ? n64 : n32) += 1;
        // the mesh's own vectors through this frame's deformation, or unchanged where the frame was passed through
        if (shot_transport(shot) && geo->npoints > 0) {
            int vrc = FD_E_INVALID;
            if (sev != FDSOP_ERROR && node->shot_dev)
                vrc = fd_shot_dev_vectors_engine(node->shot_dev, node->e_radius * node->e_radius, (float)node->fval[find_parm("falloffrate")][0],
                                                 shot->N_out ? shot->N_out[k] : nullptr, shot->tangentu_out ? shot->tangentu_out[k] : nullptr,
                                                 shot->tangentv_out ? shot->tangentv_out[k] : nullptr);
            if (vrc != FD_OK) {
                shot_pass_vectors(geo, shot, k);
                if (sev != FDSOP_ERROR) {
                    log.frame(k, FDSOP_ERROR, std::string("GPU deformation failed: ") + (node->shot_dev ? fd_shot_dev_error(node->shot_dev) : "no device resources for the vectors"));
                    if (shot->frame_severity) shot->frame_severity[k] = FDSOP_ERROR;
                }
            }
        }
        if (shot_error) stopped = true;
    }
    add_path(node, first, count, "", "", n32, "", n64);
    return stopped;
}

// the transported vectors' inputs on the device
bool shot_prepare_vectors(fdsop_node *node, const fdsop_geo *geo, const fdsop_shot *shot)
{
    return node->shot_dev && geo->npoints > 0 &&
           fd_shot_dev_set_vectors(node->shot_dev, shot->N_out ? geo->N : nullptr, shot->tangentu_out ? geo->tangentu : nullptr,
                                   shot->tangentv_out ? geo->tangentv : nullptr) == FD_OK;
}

}  // namespace

const char *fdsop_shot_paths(const fdsop_node *node) { return node ? node->shot_paths.c_str() : ""; }

int fdsop_cook_shot(fdsop_node *node, const fdsop_geo *geo, const fdsop_shot *shot)
{
    if (!node) return FDSOP_ERROR;
    node->messages.clear();
    node->severity = FDSOP_OK;
    node->shot_paths.clear();
    // the struct first, then its tables: nothing else is read before they are known to be there
    if (!geo || !shot || shot->struct_size < (int)sizeof(fdsop_shot) || shot->nframes <= 0 || !shot->deform_P || !shot->P_out) {
        node->add(FDSOP_ERROR, "Invalid shot arguments.");
        if (shot && shot->struct_size >= (int)sizeof(fdsop_shot) && shot->frame_severity)
            for (int k = 0; k < shot->nframes; ++k) shot->frame_severity[k] = FDSOP_ERROR;
        return node->severity;
    }
    const int F = shot->nframes;
    auto all_frames_error = [&] { if (shot->frame_severity) for (int k = 0; k < F; ++k) shot->frame_severity[k] = FDSOP_ERROR; };
    for (int k = 0; k < F; ++k) {
        const bool bad = !shot->deform_P[k] || !shot->P_out[k] || (shot->fd_falloff && !shot->fd_falloff[k]) ||
                         (shot->N_out && !shot->N_out[k]) || (shot->tangentu_out && !shot->tangentu_out[k]) ||
                         (shot->tangentv_out && !shot->tangentv_out[k]);
        if (bad) {
            node->add(FDSOP_ERROR, "Invalid shot arguments.");
            all_frames_error();
            return node->severity;
        }
    }
    if (geo->npoints < 0 || (geo->npoints > 0 && !geo->P) || !geo->rest_P || (shot->N_out && !geo->N) ||
        (shot->tangentu_out && !geo->tangentu) || (shot->tangentv_out && !geo->tangentv)) {
        node->add(FDSOP_ERROR, "Invalid geometry arrays.");
        all_frames_error();
        return node->severity;
    }

    ShotLog log;
    auto finish = [&] {
        node->messages = log.text;
        node->severity = log.severity;
        return node->severity;
    };
    const bool transport = shot_transport(shot);

    // F = 1 is fdsop_cook; so is a shot over an empty mesh (nothing to batch)
    if ((F == 1 && !transport) || geo->npoints == 0) {
        cook_frames_sequential(node, geo, shot, 0, F, true, log);
        return finish();
    }

    // ---- what the first cook settles, once (:228-322)
    struct PassAll {
        const fdsop_geo *g; const fdsop_shot *s; bool armed;
        ~PassAll() { if (armed) for (int k = 0; k < s->nframes; ++k) shot_pass_through(g, s, k); }
    } pass{geo, shot, true};
    CookSetup cs;
    bool ok = cook_setup(node, geo, cs);
    int rc = FD_OK;
    if (ok) {
        rc = cook_select_model(node->engine, cs);
        if (rc == FD_OK && cs.M <= 0) rc = FD_E_INVALID;
        if (rc != FD_OK) { node->add(FDSOP_ERROR, "Can't build RBF model."); ok = false; }
    }
    log.take(node, 0);               // (no frame lines yet: everything so far is the shot's)
    if (!ok) {
        all_frames_error();
        return finish();
    }
    pass.armed = false;              // from here on every frame is written by its own path
    const int M = cs.M;
    const int64_t npoints = geo->npoints;
    if (!geo->rig_rest_unchanged) { node->fp64_warned = false; node->engine_rig_stale = true; }

    // ---- the node's device side, contexts and staging
    if (!node->shot_dev) node->shot_dev = fd_shot_dev_create(node->engine);
    bool batched = node->shot_dev != nullptr && F > 1;
    if (transport && !shot_prepare_vectors(node, geo, shot)) batched = false;
    int G = 0;
    if (node->shot_dev) {
        G = fd_shot_dev_reserve(node->shot_dev, F < FD_MAX_BATCH ? F : FD_MAX_BATCH, shot->fd_falloff != nullptr);
        if (G <= 0) batched = false;
    }
    if (batched) {
        for (int i = node->shot_nctx; i < G; ++i) {
            fd_config cfg = node->cfg;
            cfg.struct_size = (int)sizeof(fd_config);
            cfg.device = cs.device;
            cfg.eval_precision = FD_EVAL_FP32;
            node->shot_ctx[i] = fd_create(&cfg);
            if (!node->shot_ctx[i]) break;
            node->shot_nctx = i + 1;
        }
        if (node->shot_nctx < 1) batched = false;
        else if (node->shot_nctx < G) G = node->shot_nctx;
    }
    // all frames' deltas as fp32 deform - rest (:278), one block with the rest rig
    if (batched) {
        std::vector<float> deltas((size_t)F * (size_t)M * 3);
        for (int k = 0; k < F; ++k) {
            const float *dp = shot->deform_P[k];
            float *d = deltas.data() + (size_t)k * (size_t)M * 3;
            for (size_t i = 0; i < (size_t)M * 3; ++i) d[i] = dp[i] - geo->rest_P[i];
        }
        if (fd_shot_dev_set_rig(node->shot_dev, geo->rest_P, deltas.data(), M, F) != FD_OK) batched = false;
    }
    if (!batched) {
        // (the node is set up: every call of the sequence follows a cook)
        cook_frames_sequential(node, geo, shot, 0, F, false, log);
        return finish();
    }

    fd_shot_dev *sd = node->shot_dev;
    const int kind = cs.kernel_ext == 1 ? FD_KERNEL_THIN_PLATE : (cs.kernel_ext == 2 ? FD_KERNEL_BIHARMONIC : (cs.kernel_ext == 3 ? FD_KERNEL_CUBIC :
                     (cs.model_index == 1 ? FD_KERNEL_GAUSSIAN_ML : FD_KERNEL_GAUSSIAN_QNN)));
    const bool ml = kind == FD_KERNEL_GAUSSIAN_ML;
    const int ml_layers = cs.layers < 8 ? cs.layers : 8;
    const float radius2 = cs.radius * cs.radius;   // :402 (a square, despite the name)
    std::vector<unsigned char> frame_ok((size_t)F, 0);
    std::vector<int> frame_sev((size_t)F, FDSOP_OK);
    int set = 0;
    for (int first = 0; first < F; first += G) {
        const int n = F - first < G ? F - first : G;
        fd_batch *&b = node->shot_batch[n];
        bool group_ok = true;
        if (!b) b = fd_batch_create(node->shot_ctx, n);
        if (!b) group_ok = false;
        for (int i = 0; i < n && group_ok; ++i) group_ok = cook_select_model(node->shot_ctx[i], cs) == FD_OK;
        fd_report reports[FD_MAX_BATCH];
        memset(reports, 0, sizeof(reports));
        const char *build_name = "";
        if (group_ok) {
            // the shared builds where they were measured ahead (see the header)
            const bool qnn_shared = kind == FD_KERNEL_GAUSSIAN_QNN && (M <= 256 ? n >= 8 : n >= 16);
            fd_batch_set_shared_lu(b, qnn_shared ? 1 : 0);
            fd_batch_set_shared_factor(b, 0);
            const float *rest[FD_MAX_BATCH], *delta[FD_MAX_BATCH];
            for (int i = 0; i < n; ++i) { rest[i] = fd_shot_dev_rest(sd); delta[i] = fd_shot_dev_delta(sd, first + i); }
            rc = fd_batch_set_points_dev(b, rest, delta, M);
            if (rc == FD_OK) rc = fd_batch_build_async(b, fd_shot_dev_work_stream(sd));
            if (rc == FD_OK) rc = fd_batch_build_result(b, reports);
            for (int i = 0; i < n; ++i) group_ok = group_ok && reports[i].terminationtype == 1;
            group_ok = group_ok && rc == FD_OK;
            if (group_ok && fd_batch_last_build_shared_factor(b)) build_name = fd_shared_qnn_build_kernel_name(M, n);
        }
        if (!group_ok) {
            // a model that does not build (or no batch object): the group's frames report as their own cooks do
            const bool stopped = cook_frames_sequential(node, geo, shot, first, n, false, log);
            for (int k = first; k < first + n; ++k) frame_sev[(size_t)k] = -1;      // (written by the sequence)
            if (stopped) {
                for (int k = first + n; k < F; ++k) { shot_pass_through(geo, shot, k); frame_sev[(size_t)k] = FDSOP_ERROR; }
                break;
            }
            continue;
        }
        // the precision, per frame
        unsigned char need64[FD_MAX_BATCH];
        int n64 = 0;
        for (int i = 0; i < n; ++i) {
            const int k = first + i;
            need64[i] = cs.precision_parm == 1 || (cs.precision_parm == 0 && !fd_fp32_holds(&reports[i], 1e-5));
            if (need64[i] && cs.precision_parm == 0 && !node->fp64_warned) {       // once per rig
                char t[240];
                snprintf(t, sizeof(t), "fp32 evaluation would not hold 1e-5 of this rig's displacements (error ~%.2g, smallest delta %.2g): "
                                       "evaluating in fp64.", reports[i].fp32_error, reports[i].delta_min);
                log.frame(k, FDSOP_WARNING, t);
                if (frame_sev[(size_t)k] < FDSOP_WARNING) frame_sev[(size_t)k] = FDSOP_WARNING;
                node->fp64_warned = true;
            }
            n64 += need64[i] ? 1 : 0;
            char info[200];
            snprintf(info, sizeof(info), "Termination type: %d, Iterations: %d", reports[i].terminationtype, reports[i].iterationscount);
            log.frame(k, FDSOP_MESSAGE, info);
            if (frame_sev[(size_t)k] < FDSOP_MESSAGE) frame_sev[(size_t)k] = FDSOP_MESSAGE;
        }
        const bool all64 = n64 == n;
        rc = fd_shot_dev_eval(sd, b, set, all64 ? 1 : 0, ml ? 1 : 0, radius2, cs.falloffrate);
        if (rc == FD_OK && !all64)
            for (int i = 0; i < n && rc == FD_OK; ++i)
                if (need64[i]) rc = fd_shot_dev_eval_fp64_over(sd, node->shot_ctx[i], set, i, radius2, cs.falloffrate);
        if (rc == FD_OK)
            rc = fd_shot_dev_deliver(sd, set, n, nullptr, shot->P_out + first, shot->fd_falloff ? shot->fd_falloff + first : nullptr,
                                     shot->N_out ? shot->N_out + first : nullptr, shot->tangentu_out ? shot->tangentu_out + first : nullptr,
                                     shot->tangentv_out ? shot->tangentv_out + first : nullptr);
        if (rc != FD_OK) {
            const std::string t = std::string("GPU deformation failed: ") + fd_shot_dev_error(sd);
            for (int k = first; k < first + n; ++k) {
                log.frame(k, FDSOP_ERROR, t);
                frame_sev[(size_t)k] = FDSOP_ERROR;
                shot_pass_through(geo, shot, k);
            }
            continue;
        }
        for (int k = first; k < first + n; ++k) frame_ok[(size_t)k] = 1;
        const int nl = n;    // the fp32 launch of a mixed group covers the whole group
        const char *e32 = all64 ? "" : (ml ? fd_shared_ml_kernel_name(M, ml_layers, nl) : fd_shared_kernel_name(M, nl, kind));
        const char *e64 = all64 ? (ml ? fd_shared_ml_fp64_kernel_name(M, ml_layers, n) : fd_shared_fp64_kernel_name(M, n, kind)) : "";
        add_path(node, first, n, build_name, e32, n - n64, e64, n64);
        set ^= 1;
    }
    bool arrived = fd_shot_dev_wait(sd, 0) == FD_OK;
    arrived = (fd_shot_dev_wait(sd, 1) == FD_OK) && arrived;
    if (!arrived) {
        const std::string t = std::string("GPU deformation failed: ") + fd_shot_dev_error(sd);
        for (int k = 0; k < F; ++k)
            if (frame_ok[(size_t)k]) { log.frame(k, FDSOP_ERROR, t); frame_sev[(size_t)k] = FDSOP_ERROR; frame_ok[(size_t)k] = 0; shot_pass_through(geo, shot, k); }
    }
    bool any_ok = false;
    for (int k = 0; k < F; ++k) any_ok = any_ok || frame_ok[(size_t)k];

    // ---- what a cook does once around its evaluation, for the frames cooked here
    if (any_ok) {
        // :386-388 -- Cd is added white and never written again
        if (geo->Cd)
            for (int64_t i = 0; i < npoints * 3; ++i) geo->Cd[i] = 1.f;
        // :396-399
        if (!geo->dist2 && !(cs.use_capture && node->captured))
            log.shot(FDSOP_WARNING, "Can't find distance capture attribute. Won't apply radius nor falloff.");
        if (geo->dist2_out && cs.use_capture && node->captured && fd_mesh_get_dist2(node->engine, geo->dist2_out) != FD_OK)
            log.shot(FDSOP_ERROR, std::string("GPU deformation failed: ") + fd_last_error(node->engine));
    }
    // :444-482 -- the morph-space pass, in frame order: the first frame that reaches it with the weights not computed yet
    // gets the reprojection (frame 0); every later one the reference's warning
    if (cs.morph_space && cs.have_blends && node->morph && fd_morph_is_initialised(node->morph)) {
        for (int k = 0; k < F; ++k) {
            if (!frame_ok[(size_t)k]) continue;
            bool weights_done = false;
            const int S = fd_morph_shape_count(node->morph);
            if (!fd_morph_is_computed(node->morph)) {
                const int doclampweight = (int)node->fval[find_parm("doclampweight")][0];
                const float falloffradius = (float)node->fval[find_parm("falloffradius")][0];
                const float weightrange[2] = {(float)node->fval[find_parm("weightrange")][0],
                                              (float)node->fval[find_parm("weightrange")][1]};
                std::vector<double> w((size_t)(S > 0 ? S : 1));
                const bool same_rest = cs.morph_inited_this_cook && cs.rest_attr == geo->P;
                int mrc = fd_morph_set_rest(node->morph, same_rest ? nullptr : cs.rest_attr, 0);
                if (mrc == FD_OK)
                    mrc = fd_morph_apply(node->morph, shot->P_out[k], doclampweight ? weightrange : nullptr,
                                         cs.dofalloff_parm && falloffradius != 0.f, falloffradius, w.data());
                weights_done = mrc == FD_OK;
                if (weights_done) {
                    if (geo->weights) memcpy(geo->weights, w.data(), sizeof(double) * (size_t)S);
                    if (geo->weights_count) *geo->weights_count = S;
                }
            }
            if (!weights_done) {
                const char *t = "Can't compute weights for morphspace deformation. Ingoring it.";   // :452
                if (k == 0) log.shot(FDSOP_WARNING, t);
                else log.frame(k, FDSOP_WARNING, t);
                if (frame_sev[(size_t)k] < FDSOP_WARNING) frame_sev[(size_t)k] = FDSOP_WARNING;
            }
        }
    }
    if (shot->frame_severity)
        for (int k = 0; k < F; ++k)
            if (frame_sev[(size_t)k] >= 0)      // (-1: the sequence wrote it)
                shot->frame_severity[k] = frame_sev[(size_t)k] == FDSOP_ERROR ? FDSOP_ERROR
                                          : (frame_sev[(size_t)k] > log.common ? frame_sev[(size_t)k] : log.common);
    return finish();
}

}  // extern "C"
