"""The shapes tests/test_gpu_eval_shapes.py walks the one-frame evaluation through (csrc/fd_eval.hip: k_deform32,
k_deform32_tps_mfma, k_deform64, their _batch forms and the multilayer SHARE variants), and the rigs, mesh and
attributes it walks them with.  tests/test_eval_shape_table.py reads the launch constants out of the sources and checks
that the lists below still sit on their edges: whoever moves a constant is told to move the table.

A plain module (no fixture): `import eval_shape_cases as cases`.  numpy and facedeform_amd.synth only; deterministic.

Kinds are named here ("thin_plate", "qnn", "gaussian", "biharmonic", "cubic", "ml"); the GPU test maps the names to the
engine's and the oracle's constants.

Centre counts, by the edge they sit on (Mpad = M rounded up to kRecPad = 16 records; a matrix-pipe tile is 16 centres):
  thin-plate  47, 48 | 49      the last k_deform32 sizes (Mpad 48) | the first matrix-pipe size (Mpad 64, 15 padded centres)
              63, 64 | 65, 80  four full tiles | a fifth tile of one centre, and full
              384 | 385, 400 | 401   kTileChunk = 24 tiles resident | a second chunk of one tile | of two tiles
              768 | 769        two full chunks | three
              16               one record group: k_deform32's shortest loop
  k_deform32  16, 17 (Mpad 16, 32)   one pass of eight records twice | four passes, no flush before the last
              56, 63, 64 (Mpad 64)   the flush at (j + 8) & 63 == 0 and the one at j + 8 >= Mpad in the same pass
              65, 72 (Mpad 80)       a 16-record tail after a flush
              127, 128 | 129 (Mpad 128 | 144)   two flushes | and a tail
  multilayer  (M, layers): records M * layers -- 66, 99, 132, 120, 264, only the last but one a multiple of 16;
              layers 2 and 6 share a centre's distances between two records, 4 between four, 8 between eight, 3 takes
              the general kernel."""
import functools

import numpy as np

from facedeform_amd import synth

POSE = 2                      # synth.deformed_rig(rest, POSE)
# (kind, M, term) -> another pose index, for the rigs whose fp32 estimate (fd_fp32_holds at the case's bar) fails at POSE;
# measured on MI355X, estimate / budget at POSE -> at the pose taken: thin-plate 768 and 769 1.05 -> 0.43, thin-plate 385
# without a term 1.45 -> 0.71, cubic 56 .. 72 1.18 .. 1.40 -> 0.76 .. 0.78.  (Every other fp32 rig of the table is below
# 1 at POSE, the nearest thin-plate 400 and 401 at 0.98.)
POSE_OVERRIDE = {("thin_plate", 768, 0): 5, ("thin_plate", 769, 0): 5, ("thin_plate", 385, 2): 5,
                 ("cubic", 56, 0): 5, ("cubic", 63, 0): 5, ("cubic", 64, 0): 5, ("cubic", 65, 0): 5, ("cubic", 72, 0): 5}

THIN_PLATE_M = (16, 47, 48, 49, 63, 64, 65, 80, 384, 385, 400, 401, 768, 769)
VALU_M = (16, 17, 56, 63, 64, 65, 72, 127, 128, 129)           # QNN, Gaussian, biharmonic: k_deform32 at every size
CUBIC_M = tuple(m for m in VALU_M if m <= 72)                  # above that cubic's fp32 estimate does not hold: fp64 only
ML_CASES = ((33, 2), (33, 3), (33, 4), (20, 6), (33, 8))       # (M, layers)
ML_RADIUS, ML_LAMBDA = 1.0, 0.1
FP64_CASES = (("thin_plate", 16), ("thin_plate", 49), ("thin_plate", 65), ("thin_plate", 385), ("thin_plate", 769),
              ("qnn", 17), ("qnn", 65), ("qnn", 129), ("cubic", 127), ("cubic", 129), ("ml", 33, 3))
BF16_TILE_M = (49, 385, 769)                                   # Engine(variant=200): the bf16 x 3 tile form
TERM_CASES = (("thin_plate", 49), ("thin_plate", 385), ("qnn", 65))       # each with the constant and the zero term

N_MESH = 1025
N_REST = 64                                                    # rest points at the end of the mesh: d2 == 0 in every kernel
N_LIST = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
# the four launches of the vertex-count and gate tests: (name, kind, M, fp64)
LAUNCHES = (("tps_mfma_resident", "thin_plate", 64, False), ("tps_mfma_chunked", "thin_plate", 400, False),
            ("valu_qnn", "qnn", 33, False), ("fp64_thin_plate", "thin_plate", 64, True))

BATCH_CASES = (("thin_plate", 48), ("thin_plate", 49), ("thin_plate", 385), ("thin_plate", 400), ("qnn", 65))
BATCH_POSES = (POSE, 0, 1)                                     # context 0 is the one held to the oracle
N_BATCH = 577

RADIUS2 = np.float32(0.36)
FALLOFFRATE = 1.5
SENTINEL = np.float32(-777.25)                                 # what untouched output rows hold; no result comes near it

# vertices per workgroup slot of the VALU kernels: vertex = block * 256 * V + v * 256 + tid, v < V
V_DEFORM32 = 4                # kDefaultVariant = 102: packed lanes, V = 4
V_DEFORM64 = 2


def kernel_params(kind, M, layers=0):
    return {"qnn": [1.0, 5.0], "gaussian": [1.2 / M ** (1.0 / 3.0)], "ml": [ML_RADIUS, layers, ML_LAMBDA]}.get(kind, [])


def pose_of(kind, M, term=0):
    return POSE_OVERRIDE.get((kind, M, term), POSE)


@functools.lru_cache(maxsize=None)
def _rig(M, pose):
    rest = synth.control_points(M, "head")
    deform = synth.deformed_rig(rest, pose)
    for a in (rest, deform):
        a.setflags(write=False)
    return rest, deform


def rig(M, pose=POSE):
    """(rest, deformed) float32 (M, 3), read-only"""
    return _rig(int(M), int(pose))


@functools.lru_cache(maxsize=None)
def _mesh(M):
    rest, _ = rig(M)
    P = np.concatenate([synth.head_mesh(3000)[::2][:N_MESH - N_REST], rest[np.arange(N_REST) % M]]).astype(np.float32)
    tan = synth.tangent_frames(P)
    for a in (P,) + tan:
        a.setflags(write=False)
    return P, tan


def mesh(M):
    """(P, (tu, tv, nrm)): 961 vertices of the head and the rig's first 64 rest points (repeating when it has fewer), so
    N = 1025 and a vertex sits exactly on a centre in every kernel; tangent frames for all of them.  Read-only."""
    return _mesh(int(M))


@functools.lru_cache(maxsize=None)
def ragged_dist2():
    """dist2 for the centre-count, vertex-count and batch tests: uniform in [0, 1.5 radius2), about a third gated, no
    structure a wave or a workgroup could line up with"""
    d2 = (np.random.default_rng(1025).random(N_MESH) * 1.5 * float(RADIUS2)).astype(np.float32)
    d2.setflags(write=False)
    return d2


# ---- gate patterns ------------------------------------------------------------------------------
GATED_WAVE = range(64, 128)              # one matrix-pipe wave of group 0; waves 0, 2 and 3 of the group live
GATED_GROUP = range(256, 512)            # matrix-pipe group 1, all four waves
ONE_LIVE_WAVE, ONE_LIVE_LANE = range(640, 704), 37
# with GATED_WAVE and 320..383 of GATED_GROUP these gate wave 1 of k_deform32's first workgroup in all four of its
# slots (tid + 256 v), and wave 1 of both k_deform64 workgroups (two slots each)
GATED_SLOTS = (range(576, 640), range(832, 896))
CAPTURE_MISS = (5, 130, 131, 200, 897, 1000)           # dist2 = -1.0: what the capture writes for a point it did not reach


@functools.lru_cache(maxsize=None)
def gate_dist2():
    """dist2 (N_MESH,) with every pattern the gate tests ask for.  Live vertices draw from [0, 0.8 radius2); every fourth
    vertex that is live sits exactly on radius2 (the gate is `>`: it stays live, with fall-off 0)."""
    r2 = float(RADIUS2)
    rng = np.random.default_rng(64)
    d2 = (rng.random(N_MESH) * 0.8 * r2).astype(np.float32)
    gated = np.zeros(N_MESH, bool)
    for run in (GATED_WAVE, GATED_GROUP, ONE_LIVE_WAVE) + GATED_SLOTS:
        gated[list(run)] = True
    gated[ONE_LIVE_WAVE[0] + ONE_LIVE_LANE] = False
    d2[gated] = (r2 * (1.001 + rng.random(int(gated.sum())))).astype(np.float32)
    d2[GATED_WAVE[0]] = np.nextafter(RADIUS2, np.float32(np.inf))          # one ulp past the radius: gated
    on = ~gated & (np.arange(N_MESH) % 4 == 0)
    d2[on] = RADIUS2
    d2[list(CAPTURE_MISS)] = np.float32(-1.0)
    d2.setflags(write=False)
    return d2


def is_live(dist2, radius2=RADIUS2):
    """the gate of src/SOP_FaceDeform.cpp:408 on fp32 values: a vertex is skipped only if dist2 > radius2"""
    return ~(np.asarray(dist2, np.float32) > np.float32(radius2))


def mfma_wave_of(v):
    """(group, wave) of the matrix-pipe kernel for vertex v: a wave owns 64 consecutive vertices, a workgroup four waves"""
    return v // 256, (v // 64) % 4


def valu_wave_members(block, wave, V, N=N_MESH):
    """the vertices wave `wave` of workgroup `block` of k_deform32 / k_deform64 owns (vertex = base + v * 256 + tid)"""
    base = block * 256 * V
    idx = [base + v * 256 + 64 * wave + lane for v in range(V) for lane in range(64)]
    return [i for i in idx if i < N]
