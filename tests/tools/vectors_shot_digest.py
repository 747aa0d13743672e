"""One SHA-256 per case over the outputs of the four shot vector calls (fd_batch_deform_vectors_shared{,_fp64,_ml,_ml_fp64}_dev),
to compare two builds of the library bit for bit:

    python tests/tools/vectors_shot_digest.py > listing.txt          # in each of the two trees; the listings must be equal

Fixed seed, N = 1000 vertices of the head mesh, dist2 uniform on [0, radius2 / 0.9) so that about a tenth of the vertices are
gated, linear term.  Models: one-layer fp32 thin-plate and QNN; fp64 thin-plate, Gaussian, QNN, biharmonic and cubic; the
multilayer model in both precisions with L in {1, 2, 3, 5, 8}.  Each at F in {1, 4, 5, 12, 13, 17, 32} frames of one rest rig
and M in {32, 256} centres, once with all four vector outputs and projection frames ("all") and once with the normal only and
no projection frames ("normal").  A digest covers, frame by frame, P_out, fd_falloff and the vector outputs asked for.  A
case below the call's *_min_frames threshold runs the per-context launches (kernel column "-").  A tool, not a test."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from facedeform_amd import capi, synth   # noqa: E402

N, RADIUS2, RATE = 1000, 0.36, 1.7
FRAMES = (1, 4, 5, 12, 13, 17, 32)
CENTRES = (32, 256)
ML = capi.KERNEL_GAUSSIAN_ML
ONE32 = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]
ONE64 = ONE32 + [("gaussian", capi.KERNEL_GAUSSIAN, [0.35]), ("biharmonic", capi.KERNEL_BIHARMONIC, []), ("cubic", capi.KERNEL_CUBIC, [])]
LAYERS = (1, 2, 3, 5, 8)
#          label, call, precision, kernel-name function (M, F) -> str, kind, parameters
CONFIGS = [("fp32 " + n, "deform_vectors_shared_dev", capi.EVAL_FP32, lambda M, F, k=k: capi.fd_shared_vectors_kernel_name(M, F, k), k, p)
           for n, k, p in ONE32]
CONFIGS += [("fp64 " + n, "deform_vectors_shared_fp64_dev", capi.EVAL_FP64, lambda M, F, k=k: capi.fd_shared_vectors_fp64_kernel_name(M, F, k), k, p)
            for n, k, p in ONE64]
CONFIGS += [("fp32 ml L=%d" % L, "deform_vectors_shared_ml_dev", capi.EVAL_FP32, lambda M, F, L=L: capi.fd_shared_vectors_ml_kernel_name(M, L, F),
             ML, [1.0, L, 0.1]) for L in LAYERS]
CONFIGS += [("fp64 ml L=%d" % L, "deform_vectors_shared_ml_fp64_dev", capi.EVAL_FP64,
             lambda M, F, L=L: capi.fd_shared_vectors_ml_fp64_kernel_name(M, L, F), ML, [1.0, L, 0.1]) for L in LAYERS]


def main():
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    dev = torch.device("cuda", 0)
    Fmax = max(FRAMES)
    P = synth.head_mesh(20_000)[::20][:N].copy()
    n0 = P.astype(np.float64) / np.array([0.75, 1.0, 0.85]) ** 2
    n0 /= np.linalg.norm(n0, axis=1, keepdims=True)
    u = np.cross(n0, [0.3, 0.2, 1.0]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n0, u)
    tu, tv, nrm = (1.3 * u).astype(np.float32), (0.8 * v).astype(np.float32), n0.astype(np.float32)
    dist2 = (np.random.default_rng(5).random(N) * RADIUS2 / 0.9).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_P, d_tu, d_tv, d_nrm, d_d2, d_Nv = (t(a) for a in (P, tu, tv, nrm, dist2, np.cross(tu, tv).astype(np.float32)))
    print("# %d of %d vertices gated" % (int((dist2 > RADIUS2).sum()), N))
    for label, call, precision, kernel_name, kind, params in CONFIGS:
        for M in CENTRES:
            rest = synth.control_points(M, "head")
            deltas = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(Fmax)]).astype(np.float32)
            d_rest, d_del = t(rest), t(deltas)
            engines = []
            for _ in range(Fmax):
                e = capi.Engine(device=0, precision=precision)
                e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
                engines.append(e)
            full = capi.Batch(engines)
            full.set_points_dev([d_rest.data_ptr()] * Fmax, [d_del.data_ptr() + f * M * 12 for f in range(Fmax)], M)
            full.build_async()
            built = sum(r.terminationtype == 1 for r in full.build_result())
            for F in FRAMES:
                batch = capi.Batch(engines[:F])
                for mode in ("all", "normal"):
                    mk = lambda w: [torch.full((N, w) if w else (N,), -7.0, device=dev) for _ in range(F)]
                    ptr = lambda ts: [x.data_ptr() for x in ts]
                    oP, ofall, oN = mk(3), mk(0), mk(3)
                    outs = [oP, ofall, oN]
                    kw = dict(d_dist2=d_d2.data_ptr(), d_falloff=ptr(ofall), d_N=d_Nv.data_ptr(), d_N_out=ptr(oN), radius2=RADIUS2, falloffrate=RATE)
                    if mode == "all":
                        otu, otv, oA = mk(3), mk(3), mk(9)
                        outs += [otu, otv, oA]
                        kw.update(d_tangents=(d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr()), d_vtu=d_tu.data_ptr(), d_vtu_out=ptr(otu),
                                  d_vtv=d_tv.data_ptr(), d_vtv_out=ptr(otv), d_jacobian=ptr(oA))
                    torch.cuda.synchronize()
                    getattr(batch, call)(N, d_P.data_ptr(), ptr(oP), **kw)
                    torch.cuda.synchronize()
                    h = hashlib.sha256()
                    for f in range(F):
                        for o in outs:
                            h.update(o[f].cpu().numpy().tobytes())
                    print("%-16s M=%-3d F=%-2d %-6s built=%d/%d %-30s %s" % (label, M, F, mode, built, Fmax,
                                                                        kernel_name(M, F) or "-", h.hexdigest()), flush=True)
                batch.close()
            full.close()
            for e in engines:
                e.close()


if __name__ == "__main__":
    main()
