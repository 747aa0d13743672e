"""CPU: the case table of tests/test_gpu_eval_shapes.py (tests/eval_shape_cases.py) against the launch constants of the
one-frame evaluation, read out of the sources.  If a constant moves -- the record padding, the tiles staged per chunk,
the centres per fp32 partial sum, the workgroup size, the matrix-pipe threshold -- an edge moves with it and this test
says which entry of the table no longer sits on it."""
import os
import re

import numpy as np

import eval_shape_cases as cases

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "facedeform_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _constant(text, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, f"constexpr int {name} not found"
    return int(m.group(1))


def _constants():
    ev = _source("fd_eval.hip")
    m = re.search(r"KIND == FD_KERNEL_THIN_PLATE && a\.tiles != nullptr && a\.Mpad >= (\d+)\)", ev)
    assert m, "the matrix-pipe dispatch condition of launch_kind not found"
    return dict(kRecPad=_constant(_source("fd_internal.h"), "kRecPad"), kTileChunk=_constant(ev, "kTileChunk"),
                kChunk=_constant(ev, "kChunk"), kBlock=_constant(ev, "kBlock"), mfma_from=int(m.group(1)),
                default_variant=_constant(ev, "kDefaultVariant"))


def _mpad(M, pad):
    return (M + pad - 1) // pad * pad


def test_thin_plate_sizes_sit_on_the_matrix_pipe_and_chunk_edges():
    c = _constants()
    pad, chunk = c["kRecPad"], c["kTileChunk"]
    Ms = cases.THIN_PLATE_M
    last_valu = c["mfma_from"] - pad                       # the largest M whose Mpad is below the threshold
    assert last_valu in Ms and last_valu - 1 in Ms, "both of the last k_deform32 sizes"
    assert last_valu + 1 in Ms and _mpad(last_valu + 1, pad) == c["mfma_from"], "the first matrix-pipe size"
    mfma = [m for m in Ms if _mpad(m, pad) >= c["mfma_from"]]
    assert any(m % pad == 0 and m + 1 in mfma and m - 1 in mfma for m in mfma), "an exact tile multiple, one under, one over"
    resident = chunk * pad                                 # the largest model staged once
    assert resident in Ms, "the last resident tile count"
    assert resident + 1 in Ms and resident + pad in Ms, "the first chunked tile count, with one centre and full"
    assert resident + pad + 1 in Ms, "a second chunk of two tiles"
    assert 2 * resident in Ms and 2 * resident + 1 in Ms, "two full chunks, and three"
    assert min(Ms) <= pad, "one record group"
    assert set(cases.BF16_TILE_M) <= set(mfma) and any(m > resident for m in cases.BF16_TILE_M) and \
        any(m > 2 * resident for m in cases.BF16_TILE_M) and any(m <= resident for m in cases.BF16_TILE_M)
    for kind, M in cases.BATCH_CASES:
        assert kind != "thin_plate" or M in Ms
    batch_tp = [M for kind, M in cases.BATCH_CASES if kind == "thin_plate"]
    assert last_valu in batch_tp and last_valu + 1 in batch_tp and resident + 1 in batch_tp and resident + pad in batch_tp


def test_valu_sizes_sit_on_the_partial_sum_edges():
    c = _constants()
    pad, flush = c["kRecPad"], c["kChunk"]
    assert pad % 8 == 0 and flush % 8 == 0                 # eight records per pass of k_deform32's loop
    for Ms in (cases.VALU_M, cases.CUBIC_M):
        mpads = {_mpad(m, pad) for m in Ms}
        assert pad in mpads and 2 * pad in mpads, "Mpad below kChunk: the flush comes from j + 8 >= Mpad alone"
        assert flush in mpads, "Mpad == kChunk: both flush conditions in one pass"
        assert flush + pad in mpads, "one tile past kChunk: a tail after a flush"
        assert {flush - 1, flush, flush + 1} <= set(Ms), "63 .. 65 for one kind"
    mpads = {_mpad(m, pad) for m in cases.VALU_M}
    assert 2 * flush in mpads and 2 * flush + pad in mpads, "two flushes, and a tail after them"
    # (not a launch constant: where cubic's fp32 estimate stops holding, measured; the sizes above it run in fp64)
    assert set(cases.CUBIC_M) == {m for m in cases.VALU_M if m <= max(cases.CUBIC_M)}, "CUBIC_M: a prefix of VALU_M"
    cubic64 = {m for k, m, *_ in cases.FP64_CASES if k == "cubic"}
    assert cubic64 and cubic64 <= {m for m in cases.VALU_M if m > max(cases.CUBIC_M)}, "FP64_CASES: cubic at sizes CUBIC_M leaves out"


def test_multilayer_cases_take_every_share_and_the_general_kernel():
    pad = _constants()["kRecPad"]
    layers = [L for _, L in cases.ML_CASES]
    share = {L: (8 if L % 8 == 0 else 4 if L % 4 == 0 else 2 if L % 2 == 0 else 1) for L in layers}      # launch_kind
    assert sorted(set(share.values())) == [1, 2, 4, 8]
    assert sum(1 for L in layers if share[L] == 2) >= 2 and 6 in layers and 2 in layers
    assert any((M * L) % pad != 0 for M, L in cases.ML_CASES) and any((M * L) % pad != 0 and share[L] > 1 for M, L in cases.ML_CASES)
    assert ("ml", 33, 3) in cases.FP64_CASES


def test_vertex_counts_bracket_every_ownership_unit():
    c = _constants()
    # variant = lanes * 100 + source * 10 + log2(V) (launch_kind)
    assert cases.V_DEFORM32 == 2 ** (c["default_variant"] % 10), "V_DEFORM32: the default variant's vertices per lane moved"
    assert re.search(r"constexpr int V = %d;" % cases.V_DEFORM64, _source("fd_eval.hip")), "V_DEFORM64: k_deform64's V moved"
    wave = 64
    assert c["kBlock"] == 4 * wave, "mfma_wave_of / valu_wave_members and the gate runs assume four waves of 64 per workgroup"
    units = {"a tile": c["kRecPad"], "a wave": wave, "a matrix-pipe workgroup": c["kBlock"],
             "a k_deform64 workgroup": c["kBlock"] * cases.V_DEFORM64, "a k_deform32 workgroup": c["kBlock"] * cases.V_DEFORM32}
    for name, u in units.items():
        assert {u - 1, u, u + 1} <= set(cases.N_LIST), f"N_LIST: {u - 1}, {u}, {u + 1} around {name} of {u} vertices"
    assert cases.N_MESH > max(units.values()), "N_MESH: more than one workgroup of every kernel"
    assert 1 in cases.N_LIST and max(cases.N_LIST) == cases.N_MESH
    assert cases.N_BATCH % 64 != 0 and cases.N_BATCH > 2 * c["kBlock"]
    for M in (16, 33, 400):
        P, tan = cases.mesh(M)
        rest, _ = cases.rig(M)
        assert P.shape == (cases.N_MESH, 3) and all(t.shape == P.shape for t in tan)
        assert np.array_equal(P[-cases.N_REST:], rest[np.arange(cases.N_REST) % M])      # d2 == 0 occurs


def test_gate_patterns():
    d2 = cases.gate_dist2()
    live = cases.is_live(d2)
    r2 = cases.RADIUS2
    assert d2.dtype == np.float32 and d2.shape == (cases.N_MESH,)
    by_wave = {}
    for v in range(cases.N_MESH):
        by_wave.setdefault(cases.mfma_wave_of(v), []).append(bool(live[v]))
    full = {k: v for k, v in by_wave.items() if len(v) == 64}
    # one whole matrix-pipe wave gated with the other waves of its group live
    assert any(not any(full[(g, w)]) and all(any(full[(g, o)]) for o in range(4) if o != w) for g, w in full)
    # one whole group of 256 gated
    assert any(all(not any(full[(g, w)]) for w in range(4)) for g in range(cases.N_MESH // 256))
    # a wave with exactly one live lane
    assert any(sum(f) == 1 for f in full.values())
    # every fourth vertex exactly on radius2, and live
    on = d2 == r2
    quarter = np.arange(cases.N_MESH) % 4 == 0
    assert on.sum() >= 100 and np.array_equal(on, quarter & live & (d2 != np.float32(-1.0)))
    assert (d2[~live] > r2).all() and (d2 == np.nextafter(r2, np.float32(np.inf))).any()      # one ulp past the radius is gated
    # the capture's "not reached" value, live
    assert (d2 == np.float32(-1.0)).sum() == len(cases.CAPTURE_MISS) and live[d2 == np.float32(-1.0)].all()
    # the VALU kernels' lane layout (vertex = base + v * 256 + tid) gets a fully gated wave next to live ones too
    for V in (cases.V_DEFORM32, cases.V_DEFORM64):
        waves = [cases.valu_wave_members(0, w, V) for w in range(4)]
        assert all(len(m) == 64 * V for m in waves)
        dead = [w for w, m in enumerate(waves) if not live[m].any()]
        assert dead and len(dead) < 4, V
    # about a third of the ragged attribute is gated, and neither a whole wave nor a whole slot of it
    rag = cases.is_live(cases.ragged_dist2())
    assert 0.25 < (~rag).mean() < 0.42
    assert all(rag[64 * w:64 * w + 64].any() for w in range(cases.N_MESH // 64))


def test_cases_name_known_kinds_and_launches():
    kinds = {"thin_plate", "qnn", "gaussian", "biharmonic", "cubic", "ml"}
    for case in cases.FP64_CASES + cases.TERM_CASES + cases.BATCH_CASES:
        assert case[0] in kinds and (len(case) == 3) == (case[0] == "ml")
    names = [n for n, *_ in cases.LAUNCHES]
    assert names == ["tps_mfma_resident", "tps_mfma_chunked", "valu_qnn", "fp64_thin_plate"]
    c = _constants()
    pad = c["kRecPad"]
    (_, k0, m0, f0), (_, k1, m1, f1), (_, k2, m2, f2), (_, k3, m3, f3) = cases.LAUNCHES
    assert k0 == k1 == k3 == "thin_plate" and not f0 and not f1 and not f2 and f3
    assert c["mfma_from"] <= _mpad(m0, pad) <= c["kTileChunk"] * pad < _mpad(m1, pad)
    assert k2 != "thin_plate"
    assert len(cases.BATCH_POSES) == 3 and cases.BATCH_POSES[0] == cases.POSE
    assert cases.kernel_params("ml", 33, 3) == [1.0, 3, 0.1] and cases.kernel_params("qnn", 65) == [1.0, 5.0]
