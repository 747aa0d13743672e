"""CPU: the C ABI of fdsop_cook_shot -- all frames of a shot through the node in one call (include/facedeform_hip.h,
facedeform_amd/csrc/fd_sop_host.cpp): the exported symbols, the struct's layout, the argument checks that come before any
device work, and the host-side cook logic (rig counts, clamps) as fdsop_cook has it."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from facedeform_amd import capi
from facedeform_amd.sop import FaceDeformSOP


def test_symbols_exported_and_declared(hip_lib):
    text = open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()
    for name in ("fdsop_cook_shot", "fdsop_shot_paths"):
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name)
    assert "int fdsop_cook_shot(fdsop_node *node, const fdsop_geo *geo, const fdsop_shot *shot);" in text
    assert "const char *fdsop_shot_paths(const fdsop_node *node);" in text
    assert hip_lib.fd_abi_version() == 9          # additive: the ABI version does not move
    assert "#define FD_ABI_VERSION 9" in text
    assert hasattr(FaceDeformSOP, "cook_shot")


def test_struct_layout_matches_header():
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(capi.FdsopShot) == 4 + 4 + 7 * p
    assert capi.FdsopShot.nframes.offset == 4 and capi.FdsopShot.deform_P.offset == 8
    assert capi.FdsopShot.frame_severity.offset == 8 + 3 * p and capi.FdsopShot.tangentv_out.offset == 8 + 6 * p
    assert C.sizeof(capi.FdsopGeo) == 26 * 8     # fdsop_geo is not touched


def _tiny_inputs():
    mesh = np.arange(12, dtype=np.float32).reshape(4, 3)
    rest = np.eye(4, 3, dtype=np.float32)
    return mesh, rest


def _raw_shot(hip_lib, mesh, rest, frames, outs, struct_size=None, nframes=None, null_deform=False, null_out=False):
    """fdsop_cook_shot on hand-made tables; returns (severity, message lines, frame severities)."""
    node = hip_lib.fdsop_create(None)
    fp = capi._f32p
    geo = capi.FdsopGeo()
    geo.npoints = mesh.shape[0]
    geo.P = mesh.ctypes.data_as(fp)
    geo.rest_npoints = geo.deform_npoints = rest.shape[0]
    geo.rest_P = rest.ctypes.data_as(fp)
    geo.rig_ntris = -1
    F = len(frames)
    t_def = (C.c_void_p * max(1, F))(*[None if a is None else a.ctypes.data for a in frames])
    t_out = (C.c_void_p * max(1, F))(*[None if a is None else a.ctypes.data for a in outs])
    sev = (C.c_int * max(1, F))(*([-1] * max(1, F)))
    pp = C.POINTER(C.c_void_p)
    shot = capi.FdsopShot(C.sizeof(capi.FdsopShot) if struct_size is None else struct_size, F if nframes is None else nframes,
                          None if null_deform else C.cast(t_def, pp), None if null_out else C.cast(t_out, pp), None, sev,
                          None, None, None)
    rc = hip_lib.fdsop_cook_shot(node, C.byref(geo), C.byref(shot))
    lines = hip_lib.fdsop_messages(node).decode().splitlines()
    engine = hip_lib.fdsop_engine(node)
    hip_lib.fdsop_destroy(node)
    return rc, lines, list(sev), engine


@pytest.mark.parametrize("case", ["struct_size", "nframes_zero", "nframes_negative", "null_deform_table", "null_out_table",
                                  "null_deform_entry", "null_out_entry"])
def test_bad_arguments_are_refused_before_any_device_work(hip_lib, case):
    mesh, rest = _tiny_inputs()
    frames = [rest + 0.1, rest + 0.2]
    outs = [np.full_like(mesh, 7.0), np.full_like(mesh, 7.0)]
    kw = {}
    if case == "struct_size":
        kw["struct_size"] = C.sizeof(capi.FdsopShot) - 8
    elif case == "nframes_zero":
        kw["nframes"] = 0
    elif case == "nframes_negative":
        kw["nframes"] = -2
    elif case == "null_deform_table":
        kw["null_deform"] = True
    elif case == "null_out_table":
        kw["null_out"] = True
    elif case == "null_deform_entry":
        frames[1] = None
    elif case == "null_out_entry":
        outs[0] = None
    rc, lines, _, engine = _raw_shot(hip_lib, mesh, rest, frames, outs, **kw)
    assert rc == capi.FDSOP_ERROR
    assert len(lines) == 1 and lines[0].startswith("error\tInvalid")
    assert not engine                                  # no engine was created: nothing reached the device
    for o in outs:
        if o is not None:
            assert np.all(o == 7.0)                    # and nothing was written


def test_null_node_and_paths(hip_lib):
    assert hip_lib.fdsop_cook_shot(None, None, None) == capi.FDSOP_ERROR
    assert hip_lib.fdsop_shot_paths(None) == b""
    node = FaceDeformSOP()
    assert node.L.fdsop_shot_paths(node.node) == b""


def test_mismatched_rigs_error_text_once_and_every_frame_passed_through(hip_lib):
    node = FaceDeformSOP()
    mesh, rest = _tiny_inputs()
    res = node.cook_shot(mesh, rest, [rest[:3], rest[:3] + 0.5, rest[:3] - 0.5])
    assert res.severity == capi.FDSOP_ERROR
    assert res.errors == ["Rest and deform geometry should match."]      # reference :232, once for the shot
    assert len(res.frames) == 3
    for fr in res.frames:
        assert fr.severity == capi.FDSOP_ERROR
        assert np.array_equal(fr.P, mesh)                                  # every output is the copy of input 0
    # one frame is fdsop_cook itself
    one = node.cook_shot(mesh, rest, [rest[:3]])
    assert one.errors == ["Rest and deform geometry should match."] and one.frames[0].severity == capi.FDSOP_ERROR
    assert np.array_equal(one.frames[0].P, mesh)


@pytest.mark.parametrize("F", [1, 3])
def test_clamps_match_reference_through_cook_shot(hip_lib, F):
    node = FaceDeformSOP()
    for tok, v in (("qcoef", 0.0), ("zcoef", -3.0), ("radius", 0.0), ("lambda", 0.0), ("layers", 0), ("maxedges", -2)):
        node.set(tok, v)
    mesh, rest = _tiny_inputs()
    node.cook_shot(mesh, rest, [rest] * F)          # fails later without a GPU; the clamps are applied first
    assert node.effective("qcoef") == pytest.approx(np.float32(0.1))
    assert node.effective("zcoef") == pytest.approx(np.float32(0.1))
    assert node.effective("radius") == pytest.approx(np.float32(0.01))
    assert node.effective("lambda") == pytest.approx(np.float32(0.01))
    assert node.effective("layers") == 1 and node.effective("maxedges") == 1
    node.set("radius", 2.5)
    node.cook_shot(mesh, rest, [rest] * F)
    assert node.effective("radius") == 2.5


def test_cook_shot_checks_its_output_arrays(hip_lib):
    node = FaceDeformSOP()
    mesh, rest = _tiny_inputs()
    with pytest.raises(ValueError):
        node.cook_shot(mesh, rest, [rest, rest], out_P=[np.empty_like(mesh)])                    # one array per frame
    with pytest.raises(ValueError):
        node.cook_shot(mesh, rest, [rest, rest], out_P=[np.empty((4, 3), np.float64)] * 2)        # float32 only
    with pytest.raises(ValueError):
        node.cook_shot(mesh, rest, [rest, rest[:3]])                                              # one count for all frames


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "facedeform_hip.h")).read()
    decl = text[text.index("all frames of a shot through the node in one call"):text.index("typedef struct fdsop_shot {")]
    for phrase in ("frame k is the k-th of F consecutive fdsop_cook calls", "rig_rest_unchanged = mesh_unchanged = 1",
                   "F = 1 IS fdsop_cook, bit for bit", "fd_fp32_holds(report_k, 1e-5)", "once per rig", "Sequential route",
                   "fd_batch_set_shared_lu", "two sets", "frame <k>: <text>"):
        assert phrase in decl, phrase
