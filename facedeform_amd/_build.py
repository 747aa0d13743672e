"""Build libfacedeform_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
CSRC = os.path.join(_PKG, "csrc")
LIB_DIR = os.path.join(_PKG, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libfacedeform_hip.so")
SOURCES = ["fd_eval.hip", "fd_eval_shared.hip", "fd_build.hip", "fd_nullspace.hip", "fd_build_reg.hip", "fd_build_ml_shared.hip", "fd_build_qnn_shared.hip", "fd_capi.hip", "fd_morph.hip", "fd_capture.hip", "fd_vectors.hip", "fd_invert.hip", "fd_adjoint.hip", "fd_adjoint_points.hip", "fd_adjoint_shot.hip", "fd_adjoint_points_shot.hip", "fd_gram.hip", "fd_bake.hip", "fd_vectors_shared.hip", "fd_eval_shared64.hip", "fd_vectors_shared64.hip", "fd_eval_shared_ml.hip", "fd_vectors_shared_ml.hip", "fd_eval_shared_ml64.hip", "fd_vectors_shared_ml64.hip", "fd_sop_host.cpp"]
# per-file extras: keep the bf16 MFMA results of the evaluation kernel in VGPRs (the default puts
# them in AGPRs and pays one v_accvgpr_read per value)
EXTRA_FLAGS = {"fd_eval.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
               # no packed fp32 in the shared-rig kernel at all (the SLP vectoriser pairs scalar multiplies and adds into
               # v_pk_* again): packed arithmetic under its matrix instructions is what gave launch-to-launch differences
               # (DESIGN.md 4.1c); same speed, and the Gaussian instantiation loses its four spills
               "fd_eval_shared.hip": ["-fno-slp-vectorize"],
               "fd_eval_shared_ml.hip": ["-fno-slp-vectorize"],      # the same kernel form, the same reason
               # the fp64 exp / log constants stay inside the K loop: hoisted, nine register pairs sit under the epilogue of
               # the 32-frame instantiations of both files, which then spill; with this every instantiation
               # has no scratch
               "fd_vectors_shared64.hip": ["-mllvm", "-disable-machine-licm"],
               "fd_vectors_shared_ml64.hip": ["-mllvm", "-disable-machine-licm"],
               # likewise under 96 accumulator registers: hoisted, the constants of the Gaussian and thin-plate instantiations
               # cost two SGPR spills and thirty VGPRs
               "fd_adjoint_shot.hip": ["-mllvm", "-disable-machine-licm"],
               # and here: hoisted, the exp constants of the Gaussian instantiation that also returns grad_f cost four SGPR
               # spills
               "fd_adjoint_points.hip": ["-mllvm", "-disable-machine-licm"],
               # the same constants under the 3 NQ operand registers of the shot form
               "fd_adjoint_points_shot.hip": ["-mllvm", "-disable-machine-licm"]}
HEADERS = [os.path.join(CSRC, "fd_internal.h"), os.path.join(CSRC, "fd_tuning.h"), os.path.join(CSRC, "fd_pack.h"), os.path.join(CSRC, "fd_eval_common.h"), os.path.join(CSRC, "fd_transport.h"), os.path.join(CSRC, "fd_eval_point.h"), os.path.join(CSRC, "fd_shot_launch.h"), os.path.join(CSRC, "fd_vectors_shot.h"), os.path.join(CSRC, "fd_shared64.h"), os.path.join(CSRC, "fd_shared_ml64.h"), os.path.join(CSRC, "fd_shared_ml.h"), os.path.join(CSRC, "fd_shared_common.h"), os.path.join(CSRC, "fd_shared_plan.h"), os.path.join(CSRC, "fd_shared_solve.h"), os.path.join(CSRC, "fd_shot_dev.h"), os.path.join(CSRC, "fd_fit_host.h"), os.path.join(CSRC, "fd_owned.h"), os.path.join(CSRC, "fd_operator.h"), os.path.join(CSRC, "fd_adjoint_points_shot.h"), os.path.join(CSRC, "fd_bake_plan.h"), os.path.join(_ROOT, "include", "facedeform_hip.h")]


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def is_stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into one shared library."""
    if not force and not is_stale():
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    obj_dir = os.path.join(_PKG, "build")
    os.makedirs(obj_dir, exist_ok=True)
    cc = hipcc_path()
    common = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I", os.path.join(_ROOT, "include")]
    common += os.environ.get("FD_EXTRA_HIPCC_FLAGS", "").split()       # experiments (-DFD_...): python -m facedeform_amd._build
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(obj_dir, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        cmd = [cc] + common + EXTRA_FLAGS.get(src, []) + ["-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out.decode(errors='replace')}")
    tmp = LIB_PATH + ".tmp"
    link = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs
    subprocess.check_call(link)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force=True, verbose=True))
