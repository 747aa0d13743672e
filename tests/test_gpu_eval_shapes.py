"""GPU: the one-frame evaluation (csrc/fd_eval.hip: k_deform32, k_deform32_tps_mfma, k_deform64, their _batch forms and the
multilayer SHARE variants -- what fd_deform*, fd_deform_mesh, fdsop_cook, the autograd forward and bench.py's single launch
run) held to the fp64 oracle at every shape its launch code distinguishes: centre counts on both sides of the matrix-pipe
threshold, of a tile, of the resident / chunked model and of the fp32 -> fp64 flush; vertex counts around a tile, a wave
and each kernel's workgroup; gate patterns that empty a wave, a workgroup, or all but one lane; the batched forms.  The
shapes and why each is there: tests/eval_shape_cases.py; tests/test_eval_shape_table.py ties them to the constants.

Reference: oracle.deform (oracle/fd_oracle.c, fp64) on the oracle's control table with the weights the ENGINE solved
(Engine.get_weights()), so a failure names the evaluation and not the build; once per model the engine's weights are held
to the oracle's, |W - W_oracle|.max() <= 1e-7 |W_oracle|.max(), which proves the two layouts agree.  Multilayer: the table
of oracle.build_multilayer with per-record radii, as tests/test_gpu_multilayer.py.

Bars (the suite's own, none made here): conftest.parity_ratio(out, ref, P, tol) <= 1 with tol = 1e-5 in fp32, 3e-5 for cubic
in fp32 (test_gpu_parity.py explains it), 2e-7 in EVAL_FP64; with tangent frames the displacement's size is taken from the
oracle's unprojected result (scale_out=, as test_gpu_edges.py).  Fall-off: np.allclose(rtol=2e-6, atol=1e-7) and the same
zeros.  Every fp32 rig must pass fd_fp32_holds at its bar: that is a condition on the table (another pose index), never a
skip.  Each test prints every shape's ratio and its worst before it asserts.

Measured on MI355X: worst parity ratio (1 = the bar) without attributes | with dist2 + frames + fall-off, and the shape of
the latter.  Every weight check, fall-off check, sentinel and bit comparison held.
  centre counts (N = 1025):
    thin-plate, default dispatch   0.41 (M = 47)   | 0.70 (M = 80);  chunked sizes 385 .. 769: 0.40 | 0.61
    thin-plate, bf16 tiles         0.37 (M = 49)   | 0.61 (M = 49)
    QNN                            0.53 (M = 65)   | 0.85 (M = 17)
    Gaussian                       0.39 (M = 128)  | 0.84 (M = 64)
    biharmonic                     0.50 (M = 64)   | 0.85 (M = 65)
    cubic (bar 3e-5)               0.31 (M = 17)   | 0.86 (M = 63)
    multilayer                     0.54 (33 x 4)   | 0.95 (33 x 3)
    constant and zero terms        0.63 (thin-plate 49, zero) | 0.91 (thin-plate 49, constant)
    EVAL_FP64 (bar 2e-7)           below 0.0005    | 0.98 (cubic 127); 0.87 .. 0.98 at all eleven: with frames on, the fp32
                                   projection of both sides is what is left, about one fp32 rounding of the displacement
  vertex counts, worst over the 16 prefixes: matrix pipe resident 0.60 (N = 513), chunked 0.61 (N = 513), k_deform32 QNN
    0.28 (N = 513), k_deform64 0.82 (N = 1025)
  gate patterns: matrix pipe resident 0.66, chunked 0.23, k_deform32 QNN 0.45, k_deform64 0.60
  batches of three, context 0, worst of the three configurations: thin-plate 48 0.49, 49 0.69, 385 0.61, 400 0.47; QNN 65 0.53
The fp32 estimate (fd_report.fp32_error over fd_fp32_holds' budget) of the rigs is 0.09 .. 0.98 at the poses the table
takes; the rigs that exceed 1 at the default pose are listed with eval_shape_cases.POSE_OVERRIDE.

Arithmetic-only slips this file was run against (each caught, the rest of the file green): dropping the second-level sum
of the chunked matrix-pipe model (every thin-plate case from M = 385, none below); dropping k_deform32's end-of-loop flush
(Mpad 16, 32, 48, 80, 112, 144; not 64 or 128); forming the shared distances only at stage 0 (layers 2, 6 and 4); `>=` for
`>` in the gate of each kernel (test_gate_patterns of that launch, by the fall-off of the vertices on the radius)."""
import numpy as np
import pytest
import torch

import eval_shape_cases as cases
from conftest import parity_ratio
from facedeform_amd import capi
from oracle import fd_oracle as fo

pytestmark = pytest.mark.gpu

KINDS = {"thin_plate": (capi.KERNEL_THIN_PLATE, fo.KERNEL_THIN_PLATE), "qnn": (capi.KERNEL_GAUSSIAN_QNN, fo.KERNEL_GAUSSIAN_QNN),
         "gaussian": (capi.KERNEL_GAUSSIAN, fo.KERNEL_GAUSSIAN), "biharmonic": (capi.KERNEL_BIHARMONIC, fo.KERNEL_BIHARMONIC),
         "cubic": (capi.KERNEL_CUBIC, fo.KERNEL_CUBIC), "ml": (capi.KERNEL_GAUSSIAN_ML, fo.KERNEL_GAUSSIAN_QNN)}
TERM_NAMES = {capi.TERM_LINEAR: "linear", capi.TERM_CONST: "const", capi.TERM_ZERO: "zero"}
R2, RATE, SENT = float(cases.RADIUS2), cases.FALLOFFRATE, float(cases.SENTINEL)


def _tol(kind, fp64):
    return 2e-7 if fp64 else (3e-5 if kind == "cubic" else 1e-5)


# ---- models --------------------------------------------------------------------------------------
class Reference:
    """the oracle and its own builds, one per rig, shared by the tests of this module"""

    def __init__(self, oracle):
        self.oracle, self._models = oracle, {}

    def model(self, kind, M, term, L, pose):
        """(table, W_oracle, radii)"""
        key = (kind, M, term, L, pose)
        if key not in self._models:
            rest, deform = cases.rig(M, pose)
            table = self.oracle.control_table(rest, deform)
            if kind == "ml":
                tt, table, W, radii = self.oracle.build_multilayer(table, cases.ML_RADIUS, L, cases.ML_LAMBDA, term)
            else:
                rc, tt, W, radii = self.oracle.build(table, KINDS[kind][1], cases.kernel_params(kind, M), term)
                assert rc == 0
            assert tt == 1, key
            self._models[key] = (table, W, radii)
        return self._models[key]


@pytest.fixture(scope="module")
def ref(oracle):
    return Reference(oracle)


class Model:
    """a built engine and what the oracle needs to evaluate ITS weights"""

    def __init__(self, ref, kind, M, L=0, term=capi.TERM_LINEAR, fp64=False, variant=0, pose=None, engine=None, report=None):
        self.kind, self.M, self.L, self.term, self.fp64 = kind, M, L, term, fp64
        self.tol = _tol(kind, fp64)
        pose = cases.pose_of(kind, M, term) if pose is None else pose
        self.label = f"{kind} M={M}" + (f" L={L}" if L else "") + (f" pose {pose}" if pose != cases.POSE else "") + (f" {TERM_NAMES[term]}" if term else "") + \
                     (" fp64" if fp64 else "") + (f" variant={variant}" if variant else "")
        self.table, W_ref, self.radii = ref.model(kind, M, term, L, pose)
        self.ko = KINDS[kind][1]
        if engine is None:
            rest, deform = cases.rig(M, pose)
            engine = capi.Engine(precision=capi.EVAL_FP64 if fp64 else capi.EVAL_FP32, variant=variant)
            engine.set_kernel(KINDS[kind][0], cases.kernel_params(kind, M, L)); engine.set_term(term)
            engine.set_points(rest, (deform - rest).astype(np.float32))
            report = engine.build()
        self.e, self.rep = engine, report
        assert report.terminationtype == 1, self.label
        self.W, _ = engine.get_weights()
        werr = np.abs(self.W - W_ref).max() / np.abs(W_ref).max()
        assert self.W.shape == W_ref.shape and werr <= 1e-7, (self.label, werr)
        if kind == "ml":
            assert engine.L.fd_model_centres(engine.ctx) == M * L, self.label
        # the fp32 estimate: a rig that fails it is a wrong table entry (eval_shape_cases.POSE_OVERRIDE), not a finding
        self.holds = fp64 or engine.fp32_holds(report, self.tol)

    def reference(self, ref, P, dist2=None, tangents=None):
        """(positions, fall-off, plain): the oracle's positions and fall-off, and its positions before the tangent projection"""
        kw = dict(dist2=dist2, radius2=R2, falloffrate=RATE)
        out, out_fall = ref.oracle.deform(self.table, self.ko, self.radii, self.W, P, tangents=tangents, **kw)
        plain = out if tangents is None else ref.oracle.deform(self.table, self.ko, self.radii, self.W, P, **kw)[0]
        return out, out_fall, plain


def _fall_ok(fall, ref_fall):
    return bool(np.allclose(fall, ref_fall, rtol=2e-6, atol=1e-7) and np.array_equal(fall == 0, ref_fall == 0))


def _report(title, rows, failures):
    """rows: (ratio, label).  Prints every shape and the worst, then fails with everything that missed."""
    for ratio, label in rows:
        print(f"  {title}: {label}: ratio {ratio:.3f}")
    if rows:
        worst = max(rows)
        print(f"{title}: worst parity ratio {worst[0]:.3f} at {worst[1]} ({len(rows)} runs)")
    assert not failures, failures


# ---- 1. centre counts ------------------------------------------------------------------------------
def _centre_cases(group):
    if group == "thin_plate":
        return [dict(kind="thin_plate", M=m) for m in cases.THIN_PLATE_M]
    if group in ("qnn", "gaussian", "biharmonic"):
        return [dict(kind=group, M=m) for m in cases.VALU_M]
    if group == "cubic":
        return [dict(kind="cubic", M=m) for m in cases.CUBIC_M]
    if group == "multilayer":
        return [dict(kind="ml", M=m, L=L) for m, L in cases.ML_CASES]
    if group == "fp64":
        return [dict(kind=c[0], M=c[1], L=c[2] if len(c) > 2 else 0, fp64=True) for c in cases.FP64_CASES]
    if group == "bf16_tiles":
        return [dict(kind="thin_plate", M=m, variant=200) for m in cases.BF16_TILE_M]
    assert group == "terms"
    return [dict(kind=k, M=m, term=t) for k, m in cases.TERM_CASES for t in (capi.TERM_CONST, capi.TERM_ZERO)]


@pytest.mark.parametrize("group", ["thin_plate", "qnn", "gaussian", "biharmonic", "cubic", "multilayer", "fp64", "bf16_tiles", "terms"])
def test_centre_counts(hip_lib, ref, group):
    """N = 1025; every model once without attributes and once with dist2 (a third gated) + tangent frames + fall-off."""
    rows, failures = [], []
    for case in _centre_cases(group):
        m = Model(ref, **case)
        if not m.holds:
            failures.append(f"{m.label}: fd_fp32_holds({m.tol:g}) is false -- give the rig another pose index")
        P, tan = cases.mesh(m.M)
        for attrs in (False, True):
            d2, t = (cases.ragged_dist2(), tan) if attrs else (None, None)
            out, fall = m.e.deform(P, dist2=d2, tangents=t, radius2=R2, falloffrate=RATE)
            want, ref_fall, plain = m.reference(ref, P, d2, t)
            ratio = parity_ratio(out, want, P, m.tol, scale_out=plain)
            label = m.label + (", dist2 + frames + fall-off" if attrs else "")
            rows.append((ratio, label))
            if not ratio <= 1.0:
                failures.append(f"{label}: parity ratio {ratio:.3f}")
            if not _fall_ok(fall, ref_fall):
                failures.append(f"{label}: fall-off off by {np.abs(fall - ref_fall).max():.3g}")
        m.e.close()
    _report(f"centre counts, {group}", rows, failures)


# ---- the four launches of the vertex-count and gate tests --------------------------------------------
@pytest.fixture(scope="module")
def launches(hip_lib, ref):
    built = {}

    def get(name):
        if name not in built:
            _, kind, M, fp64 = next(l for l in cases.LAUNCHES if l[0] == name)
            m = Model(ref, kind, M, fp64=fp64)
            assert m.holds, f"{m.label}: fd_fp32_holds is false -- give the rig another pose index"
            built[name] = m
        return built[name]

    yield get
    for m in built.values():
        m.e.close()


LAUNCH_NAMES = [l[0] for l in cases.LAUNCHES]


def _to_dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(torch.device("cuda", 0))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class DevMesh:
    """the 1025-vertex mesh of a rig on the device, with one dist2 attribute and the tangent frames"""

    def __init__(self, M, dist2):
        self.P, self.tan = cases.mesh(M)
        self.dist2 = dist2
        self.d_P, self.d_d2 = _to_dev(self.P), _to_dev(dist2)
        self.d_tan = [_to_dev(t) for t in self.tan]

    def run(self, e, N, in_place=False):
        """fd_deform_dev on the first N vertices into buffers of N + 5 rows pre-filled with the sentinel; -> (out, fall)
        as numpy, all N + 5 rows.  in_place: P_out is P_in (a copy of the mesh with five sentinel rows appended)."""
        dev = self.d_P.device
        d_fall = torch.full((N + 5,), SENT, device=dev)
        d_out = torch.full((N + 5, 3), SENT, device=dev)
        if in_place:
            d_out[:N] = self.d_P[:N]
        d_in = d_out if in_place else self.d_P
        torch.cuda.synchronize()
        e.deform_dev(N, d_in.data_ptr(), d_out.data_ptr(), d_dist2=self.d_d2.data_ptr(), d_falloff=d_fall.data_ptr(),
                     d_tu=self.d_tan[0].data_ptr(), d_tv=self.d_tan[1].data_ptr(), d_nrm=self.d_tan[2].data_ptr(),
                     radius2=R2, falloffrate=RATE)
        e.synchronize()
        return d_out.cpu().numpy(), d_fall.cpu().numpy()


def _check_dev_result(label, out, fall, N, P, dist2, want, ref_fall, plain, tol, failures):
    """what every device-pointer run must satisfy on its first N rows and the five behind them; -> parity ratio"""
    live = cases.is_live(dist2[:N])
    ratio = parity_ratio(out[:N], want[:N], P[:N], tol, scale_out=plain[:N])
    if not ratio <= 1.0:
        failures.append(f"{label}: parity ratio {ratio:.3f}")
    if not _fall_ok(fall[:N][live], ref_fall[:N][live]):
        failures.append(f"{label}: fall-off of live vertices off by {np.abs(fall[:N][live] - ref_fall[:N][live]).max():.3g}")
    if not np.array_equal(_bits(fall[:N][~live]), _bits(np.full(int((~live).sum()), SENT, np.float32))):
        failures.append(f"{label}: a gated vertex's fall-off was written")
    if not np.array_equal(_bits(out[:N][~live]), _bits(P[:N][~live])):
        failures.append(f"{label}: a gated vertex moved")
    if not (np.all(out[N:] == np.float32(SENT)) and np.all(fall[N:] == np.float32(SENT))):
        failures.append(f"{label}: rows past N were written")
    return ratio


# ---- 2. vertex counts ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAUNCH_NAMES)
def test_vertex_counts(launches, ref, name):
    """Prefixes of the mesh with dist2 (a third gated), frames and fall-off on: parity on the prefix, nothing written past
    it, and every vertex's bits those of the 1025-vertex call (a result does not depend on its neighbours)."""
    m = launches(name)
    mesh = DevMesh(m.M, cases.ragged_dist2())
    want, ref_fall, plain = m.reference(ref, mesh.P, mesh.dist2, mesh.tan)
    full_out, full_fall = mesh.run(m.e, cases.N_MESH)
    rows, failures = [], []
    for N in cases.N_LIST:
        out, fall = (full_out, full_fall) if N == cases.N_MESH else mesh.run(m.e, N)
        label = f"{m.label} N={N}"
        rows.append((_check_dev_result(label, out, fall, N, mesh.P, mesh.dist2, want, ref_fall, plain, m.tol, failures), label))
        if not (np.array_equal(_bits(out[:N]), _bits(full_out[:N])) and np.array_equal(_bits(fall[:N]), _bits(full_fall[:N]))):
            failures.append(f"{label}: bits differ from the {cases.N_MESH}-vertex call")
    _report(f"vertex counts, {name}", rows, failures)


# ---- 3. gate patterns ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAUNCH_NAMES)
def test_gate_patterns(launches, ref, name):
    """A gated wave beside live ones, a gated workgroup, a wave with one live lane, vertices exactly on the radius (live)
    and at -1.0, frames and fall-off on: the position output, the displacement output and the in-place call."""
    m = launches(name)
    mesh = DevMesh(m.M, cases.gate_dist2())
    N, P = cases.N_MESH, mesh.P
    live = cases.is_live(mesh.dist2)
    want, ref_fall, plain = m.reference(ref, P, mesh.dist2, mesh.tan)
    assert ref_fall[mesh.dist2 == np.float32(-1.0)].min() > 1.0            # the capture's -1: fall-off above 1, as the oracle gives
    assert np.all(ref_fall[mesh.dist2 == cases.RADIUS2] == 0.0)            # on the radius: live, fall-off 0
    rows, failures = [], []
    out, fall = mesh.run(m.e, N)
    rows.append((_check_dev_result(f"{m.label} positions", out, fall, N, P, mesh.dist2, want, ref_fall, plain, m.tol, failures),
                 f"{m.label} positions"))
    try:
        m.e.set_output(capi.OUTPUT_DISPLACEMENT)
        disp, dfall = mesh.run(m.e, N)
    finally:
        m.e.set_output(capi.OUTPUT_POSITION)
    if not np.all(_bits(disp[:N][~live]) == 0):
        failures.append(f"{m.label}: a gated row of the displacement output is not +0.0")
    if not np.array_equal(_bits((P[live] + disp[:N][live]).astype(np.float32)), _bits(out[:N][live])):
        failures.append(f"{m.label}: fp32(P + displacement output) is not the position output on live rows")
    if not (np.array_equal(_bits(dfall), _bits(fall)) and np.all(disp[N:] == np.float32(SENT))):
        failures.append(f"{m.label}: displacement output: fall-off differs or rows past N were written")
    inp, ifall = mesh.run(m.e, N, in_place=True)
    if not (np.array_equal(_bits(inp), _bits(out)) and np.array_equal(_bits(ifall), _bits(fall))):
        failures.append(f"{m.label}: the in-place call differs from the out-of-place call")
    _report(f"gate patterns, {name}", rows, failures)


# ---- 4. batched forms ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", cases.BATCH_CASES)
def test_batched_forms(hip_lib, ref, kind, M):
    """fd_batch_deform_dev over three poses of one rig equals each context's fd_deform_dev bit for bit (k_deform32_batch below
    the matrix-pipe threshold and for QNN, k_deform32_tps_mfma_batch from it on, resident and chunked), and context 0 passes
    oracle parity -- without attributes, with dist2, with dist2 + frames."""
    dev = torch.device("cuda", 0)
    nb, N = len(cases.BATCH_POSES), cases.N_BATCH
    engines = []
    for pose in cases.BATCH_POSES:
        rest, deform = cases.rig(M, pose)
        e = capi.Engine()
        e.set_kernel(KINDS[kind][0], cases.kernel_params(kind, M)); e.set_term(capi.TERM_LINEAR)
        e.set_points(rest, (deform - rest).astype(np.float32))
        engines.append(e)
    b = capi.Batch(engines)
    b.build_async()
    reps = b.build_result()
    assert [r.terminationtype for r in reps] == [1] * nb
    m = Model(ref, kind, M, pose=cases.BATCH_POSES[0], engine=engines[0], report=reps[0])
    assert m.holds, f"{m.label}: fd_fp32_holds is false -- give the rig another pose index"
    P_all, tan_all = cases.mesh(M)
    P, tan, d2 = P_all[-N:].copy(), [t[-N:].copy() for t in tan_all], cases.ragged_dist2()[-N:].copy()     # the rest points are in
    d_P, d_d2, d_tan = _to_dev(P), _to_dev(d2), [_to_dev(t) for t in tan]
    stream = torch.cuda.Stream(device=dev)
    rows, failures = [], []
    for use_d2, use_tan in ((False, False), (True, False), (True, True)):
        label = f"{m.label} x{nb}, N={N}" + (", dist2" if use_d2 else "") + (" + frames" if use_tan else "")
        outs = [torch.full((N + 5, 3), SENT, device=dev) for _ in range(nb)]
        falls = [torch.full((N + 5,), SENT, device=dev) for _ in range(nb)]
        singles = [torch.full((N + 5, 3), SENT, device=dev) for _ in range(nb)]
        sfalls = [torch.full((N + 5,), SENT, device=dev) for _ in range(nb)]
        torch.cuda.synchronize()
        b.deform_dev(N, [d_P.data_ptr()] * nb, [o.data_ptr() for o in outs], [d_d2.data_ptr()] * nb if use_d2 else None,
                     [f.data_ptr() for f in falls], [[t.data_ptr()] * nb for t in d_tan] if use_tan else None,
                     radius2=R2, falloffrate=RATE, stream_ptr=stream.cuda_stream)
        stream.synchronize()
        for e, o, f in zip(engines, singles, sfalls):
            e.deform_dev(N, d_P.data_ptr(), o.data_ptr(), d_dist2=d_d2.data_ptr() if use_d2 else 0, d_falloff=f.data_ptr(),
                         d_tu=d_tan[0].data_ptr() if use_tan else 0, d_tv=d_tan[1].data_ptr() if use_tan else 0,
                         d_nrm=d_tan[2].data_ptr() if use_tan else 0, radius2=R2, falloffrate=RATE)
            e.synchronize()
        for k in range(nb):
            if not (torch.equal(outs[k].view(torch.int32), singles[k].view(torch.int32)) and
                    torch.equal(falls[k].view(torch.int32), sfalls[k].view(torch.int32))):
                failures.append(f"{label}: context {k} of the batched call differs from its single launch")
        if torch.equal(outs[0], outs[1]):
            failures.append(f"{label}: two poses gave the same result")
        dist2 = d2 if use_d2 else np.zeros(N, np.float32)
        want, ref_fall, plain = m.reference(ref, P, d2 if use_d2 else None, tan if use_tan else None)
        rows.append((_check_dev_result(label, outs[0].cpu().numpy(), falls[0].cpu().numpy(), N, P, dist2, want, ref_fall, plain,
                                       m.tol, failures), label))
    b.close()
    for e in engines:
        e.close()
    _report(f"batched forms, {kind} M={M}", rows, failures)
