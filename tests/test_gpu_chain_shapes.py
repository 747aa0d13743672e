"""GPU: the null-space Cholesky launch chain (FD_SOLVER_CHAIN: k_ns_reflectors / k_ns_kv / k_ns_rotate, the fused
k_chol_step, k_backsub_inv / k_ns_recover, and k_chol_solve / k_chol_trail for fd_set_deltas) and its one-workgroup sibling
k_build_small (FD_SOLVER_ONE_WORKGROUP) at every block shape, asked for by name.  FD_SOLVER_AUTO is the register-resident
build up to 256 control points (tests/test_gpu_register_build.py), so a test that asks for AUTO reaches neither below that.

Shapes are named by n1 = M - T, the order of the projected block (T polynomial columns: 4 linear, 1 constant, 0 none); the
chain pads it to npc = round_up(n1, 32).  SMALL walks one block, the 192-row slabs of k_chol_step (one exactly, one plus a
row, two, two plus a row), the 64-row waves inside them, the identity padding of a ragged last block, and npc == 512: the
last size without deferred trailing updates and the largest k_build_small takes.  DEEP (npc > 512: a bulk update every 4th
step, every 8th in a batch of four or more) gives block counts 17 .. 25 -- every residue modulo 4 and modulo 8, a ragged
last block in each group position -- and back-substitution ranges of 32 | 256 | 256 rows, exactly 3 x 256, and 32 over.

Reference: the fp64 oracle (oracle.build on oracle.control_table).  Bar: |W - W_oracle|.max() <= 2e-9 |W_oracle|.max(),
as in test_gpu_solver.py::test_cholesky_and_lu_agree_with_each_other_and_the_oracle; the oracle itself moves by at most
1.2e-10 of max|W| under a permutation of the control points (another elimination order of the same system) on all eight
pairs at these sizes, a sixteenth of the bar.  Every test prints its worst error as a fraction of the bar before it
asserts; the measured figures are in DESIGN.md 4.2b.

Measured on MI355X, worst error as a fraction of the bar (the size n1 it occurred at in brackets):
  every shape, chain (= AUTO above 256 points) | k_build_small:
    thin-plate + linear 0.0012 (640) | 0.00065 (511);  with lambda = 1e-3 0.0013 (769) | 0.00049 (480);
    cubic + linear 0.050 (640) | 0.044 (511);  biharmonic + linear 0.0001 (672) | 0.00008 (512);
    biharmonic + constant 0.0002 (641) | 0.0001 (416);  Gaussian + linear 0.042 (289) | 0.042 (289);
    Gaussian + constant 0.13 (289) | 0.13 (289);  Gaussian, lambda = 1e-2, no term 0.00044 (289) | 0.00044 (289)
  after fd_set_deltas, chain | k_build_small: T = 4 0.00097 (641) | 0.00042 (512); T = 1 0.00028 (769) | 0.00016 (512);
    T = 0 0.00026 (257) | 0.00026 (257)
  deep batches of 2 | of 5: T = 4 0.0014 (736) | 0.0023 (640); T = 1 0.00032 (768) | 0.00032 (768); T = 0 3e-6 | 4e-6 (768)"""
import numpy as np
import pytest
import torch

from facedeform_amd import capi, synth
from test_gpu_solver import SPD_CASES

pytestmark = pytest.mark.gpu

SMALL = [12, 16, 31, 32, 33, 63, 64, 65, 96, 97, 160, 191, 192, 193, 223, 224, 225,
         255, 256, 257, 288, 289, 383, 384, 385, 416, 417, 480, 511, 512]
DEEP = [513, 544, 545, 576, 577, 608, 609, 640, 641, 672, 704, 736, 768, 769]
BAR = 2e-9                      # of max|W_oracle|
SMALL_MAX_NPC = 512             # k_build_small's bound (fd_nullspace.hip kSmallMaxNpc)
REG_MAX_M = 256                 # FD_SOLVER_AUTO is the register-resident build up to here

# one pair per T: thin-plate + linear (4), biharmonic + constant (1), Gaussian + lambda without a term (0)
T_CASES = [SPD_CASES[0], SPD_CASES[4], SPD_CASES[7]]


def _ids(cases):
    names = {capi.KERNEL_THIN_PLATE: "thin_plate", capi.KERNEL_CUBIC: "cubic", capi.KERNEL_BIHARMONIC: "biharmonic",
             capi.KERNEL_GAUSSIAN: "gaussian"}
    terms = {capi.TERM_LINEAR: "linear", capi.TERM_CONST: "const", capi.TERM_ZERO: "zero"}
    return [f"{names[k]}{'_smoothed' if (k != capi.KERNEL_GAUSSIAN and p) else ''}-{terms[t]}" for k, p, t in cases]


def _params(kind, params, M):
    """test_gpu_solver.py's rule: a fixed Gaussian radius of 0.35 over more than 300 centres is numerically singular."""
    if kind == capi.KERNEL_GAUSSIAN and M > 300:
        return [0.12] + list(params[1:])
    return list(params)


def _npc(n1):
    return (n1 + 31) // 32 * 32


def _engine(kind, params, term, rest, delta, solver):
    e = capi.Engine(solver=solver)
    e.set_kernel(kind, params); e.set_term(term)
    e.set_points(rest, delta)
    return e


_oracle_cache = {}


def _table_for_deltas(oracle, rest, delta):
    """oracle.control_table's table (centres, then deltas, widened to fp64) for a rig given as rest points and fp32 deltas:
    the delta columns are the very deltas the engine is handed, which rest + delta - rest in fp32 would not return bit for
    bit."""
    table = oracle.control_table(rest, rest)
    table[:, 3:6] = delta.astype(np.float64)
    return table


def _oracle_weights(oracle, kind, params, term, table, tag):
    """The oracle's weights for `table`, computed once per (pair, M, tag) and shared read-only."""
    key = (kind, tuple(params), term, table.shape[0], tag)
    if key not in _oracle_cache:
        rc, tt, W, radii = oracle.build(table, kind, params, term)
        assert tt == 1, key
        W.setflags(write=False)
        _oracle_cache[key] = W
    return _oracle_cache[key]


def _ratio(W, Wo):
    return float(np.abs(W - Wo).max() / (BAR * np.abs(Wo).max()))


def _check_report(rep, M, T, used, where):
    assert rep.terminationtype == 1, where
    assert rep.n == M + T and rep.iterationscount == M + T, (where, rep.n, rep.iterationscount)
    assert 0.0 < rep.pivot_ratio <= 1.0, (where, rep.pivot_ratio)
    assert rep.solver_used == used, (where, rep.solver_used)


@pytest.mark.parametrize("kind,params,term", SPD_CASES, ids=_ids(SPD_CASES))
def test_every_shape_against_the_oracle(hip_lib, oracle, kind, params, term):
    """Every size of SMALL + DEEP with the chain, with k_build_small where it applies (and one row beyond: the chain, and
    reported as such), and with FD_SOLVER_AUTO above 256 control points, where it is the chain bit for bit."""
    T = (4, 1, 0)[term]
    worst = {}
    failures = []
    for n1 in SMALL + DEEP:
        M = n1 + T
        if M < 16:
            continue                      # spd_applicable: nothing under 16 points is projected
        p = _params(kind, params, M)
        rest = synth.control_points(M, "head")
        deform = synth.deformed_rig(rest, 2)
        delta = (deform - rest).astype(np.float32)
        Wo = _oracle_weights(oracle, kind, p, term, oracle.control_table(rest, deform), "rig2")
        builds = [("chain", capi.SOLVER_CHAIN, capi.SOLVER_CHAIN)]
        if _npc(n1) <= SMALL_MAX_NPC:
            builds.append(("one_workgroup", capi.SOLVER_ONE_WORKGROUP, capi.SOLVER_ONE_WORKGROUP))
        elif n1 == SMALL_MAX_NPC + 1:
            builds.append(("one_workgroup_beyond", capi.SOLVER_ONE_WORKGROUP, capi.SOLVER_CHAIN))
        if M > REG_MAX_M:
            builds.append(("auto", capi.SOLVER_AUTO, capi.SOLVER_CHAIN))
        got = {}
        for name, solver, used in builds:
            e = _engine(kind, p, term, rest, delta, solver)
            _check_report(e.build(), M, T, used, (name, n1))
            got[name] = e.get_weights()[0]
            e.close()
            r = _ratio(got[name], Wo)
            if r > worst.get(name, (0.0, 0))[0]:
                worst[name] = (r, n1)
            if not r <= 1.0:
                failures.append((name, n1, r))
        for name in ("auto", "one_workgroup_beyond"):
            if name in got:
                assert np.array_equal(got[name], got["chain"]), (name, n1)          # the same path
        if "one_workgroup" in got:
            a, b = got["chain"], got["one_workgroup"]
            assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max(), n1                 # same system, another elimination order
    print("worst |W - W_oracle| / bar: " + ", ".join(f"{k} {v[0]:.2g} (n1 = {v[1]})" for k, v in sorted(worst.items())))
    assert not failures, failures


@pytest.mark.parametrize("kind,params,term", T_CASES, ids=_ids(T_CASES))
def test_new_deltas_through_the_stored_factor(hip_lib, oracle, kind, params, term):
    """fd_set_deltas on the Cholesky path (launch_resolve_spd: k_chol_solve / k_chol_trail on the right-hand sides alone)
    with 4, 1 and 0 polynomial columns, behind the chain's factor and behind k_build_small's: bit-identical to a rebuild,
    and -- so that an error the two share cannot hide behind that -- within the bar of the oracle for the new deltas."""
    T = (4, 1, 0)[term]
    worst = {}
    failures = []
    for n1 in (16, 33, 192, 193, 257, 512, 513, 545, 641, 769):
        M = n1 + T
        p = _params(kind, params, M)
        rest = synth.control_points(M, "head")
        d0 = synth.smooth_deltas(rest, 0).astype(np.float32)
        d1 = synth.smooth_deltas(rest, 1).astype(np.float32)
        Wo = _oracle_weights(oracle, kind, p, term, _table_for_deltas(oracle, rest, d1), "smooth1")
        solvers = [("chain", capi.SOLVER_CHAIN)]
        if _npc(n1) <= SMALL_MAX_NPC:
            solvers.append(("one_workgroup", capi.SOLVER_ONE_WORKGROUP))
        for name, solver in solvers:
            e = _engine(kind, p, term, rest, d0, solver)
            _check_report(e.build(), M, T, solver, (name, n1))
            e.set_deltas(d1)
            assert e.build().terminationtype == 1, (name, n1)
            Wd = e.get_weights()[0]
            e.set_points(rest, d1)
            assert e.build().terminationtype == 1, (name, n1)
            assert np.array_equal(Wd, e.get_weights()[0]), (name, n1)               # through the stored factor == rebuilt
            e.close()
            r = _ratio(Wd, Wo)
            if r > worst.get(name, (0.0, 0))[0]:
                worst[name] = (r, n1)
            if not r <= 1.0:
                failures.append((name, n1, r))
    print("worst |W - W_oracle| / bar after fd_set_deltas: " + ", ".join(f"{k} {v[0]:.2g} (n1 = {v[1]})" for k, v in sorted(worst.items())))
    assert not failures, failures


def _batch_against_singles(kind, p, term, rest, F, solver, used):
    """F contexts on one rest array with deltas smooth_deltas(rest, f), built as one batch; every context's weights must
    equal the same model built alone with the same solver choice, bit for bit.  Returns the batch's weights per context."""
    M = rest.shape[0]
    T = (4, 1, 0)[term]
    dev = torch.device("cuda", 0)
    deltas = [synth.smooth_deltas(rest, f).astype(np.float32) for f in range(F)]
    d_rest = torch.from_numpy(rest).to(dev)
    d_del = [torch.from_numpy(d).to(dev) for d in deltas]
    es = []
    for _ in range(F):
        e = capi.Engine(solver=solver); e.set_kernel(kind, p); e.set_term(term); es.append(e)
    b = capi.Batch(es)
    b.set_points_dev([d_rest.data_ptr()] * F, [t.data_ptr() for t in d_del], M)
    b.build_async()
    for f, rep in enumerate(b.build_result()):
        _check_report(rep, M, T, used, (M, F, f))
    Wb = [e.get_weights()[0] for e in es]
    single = capi.Engine(solver=solver); single.set_kernel(kind, p); single.set_term(term)
    for f in range(F):
        single.set_points(rest, deltas[f])
        _check_report(single.build(), M, T, used, (M, "single", f))
        assert np.array_equal(single.get_weights()[0], Wb[f]), (M, F, f)
    single.close(); b.close()
    for e in es:
        e.close()
    return Wb, deltas


@pytest.mark.parametrize("F", [2, 5])
@pytest.mark.parametrize("kind,params,term", T_CASES, ids=_ids(T_CASES))
def test_batches_in_the_deep_regime(hip_lib, oracle, kind, params, term, F):
    """Batches of the chain above npc = 512: F = 2 defers the bulk update as a lone system does (every 4th step), F = 5 twice
    as long (every 8th), over every residue of the block count.  Every context equals its single build bit for bit
    ("at every order"); the first and the last are held to the oracle."""
    T = (4, 1, 0)[term]
    worst = (0.0, 0)
    failures = []
    for n1 in (512, 544, 545, 576, 608, 640, 672, 704, 736, 768):
        M = n1 + T
        p = _params(kind, params, M)
        rest = synth.control_points(M, "head")
        Wb, deltas = _batch_against_singles(kind, p, term, rest, F, capi.SOLVER_CHAIN, capi.SOLVER_CHAIN)
        for f in (0, F - 1):
            Wo = _oracle_weights(oracle, kind, p, term, _table_for_deltas(oracle, rest, deltas[f]), f"smooth{f}")
            r = _ratio(Wb[f], Wo)
            if r > worst[0]:
                worst = (r, n1)
            if not r <= 1.0:
                failures.append((n1, f, r))
    print(f"worst |W - W_oracle| / bar, batch of {F}: {worst[0]:.2g} (n1 = {worst[1]})")
    assert not failures, failures


@pytest.mark.parametrize("kind,params,term", T_CASES, ids=_ids(T_CASES))
def test_one_workgroup_batches_on_both_sides_of_its_edge(hip_lib, kind, params, term):
    """Five FD_SOLVER_ONE_WORKGROUP contexts at n1 = 512 (k_build_small's largest, a grid of five such workgroups) and at
    513 (the chain): each equals its single builds bit for bit, and the report names what ran."""
    T = (4, 1, 0)[term]
    for n1, used in ((512, capi.SOLVER_ONE_WORKGROUP), (513, capi.SOLVER_CHAIN)):
        M = n1 + T
        rest = synth.control_points(M, "head")
        _batch_against_singles(kind, _params(kind, params, M), term, rest, 5, capi.SOLVER_ONE_WORKGROUP, used)


def test_failures_report_the_same_way_in_the_deep_regime(hip_lib):
    """test_gpu_solver.py::test_failures_report_the_same_way at M = 600 (19 blocks, deferred updates, ranged
    back-substitution): -5 for coincident centres, -4 for a flat rig under the linear term and for a poisoned matrix, and
    the context recovers."""
    rest = synth.control_points(600, "head")
    delta = synth.smooth_deltas(rest, 0).astype(np.float32)
    for solver in (capi.SOLVER_CHAIN, capi.SOLVER_AUTO):
        dup = rest.copy(); dup[9] = dup[40]
        e = _engine(capi.KERNEL_THIN_PLATE, [], capi.TERM_LINEAR, dup, delta, solver)
        assert e.build(check=False).terminationtype == -5
        flat = rest.copy(); flat[:, 2] = 0.25
        e.set_points(flat, delta)
        assert e.build(check=False).terminationtype == -4
        nan = rest.copy(); nan[3, 1] = np.nan
        e.set_points(nan, delta)
        assert e.build(check=False).terminationtype in (-4, -5)
        e.set_points(rest, delta)
        assert e.build().terminationtype == 1                      # and the context recovers
        e.close()
