"""One SHA-256 per case over P_out, fd_falloff and the transported normal of fd_batch_deform_vectors_shared_dev, to compare two
builds of the library bit for bit across every variant of the shared-rig fp32 launch's plan (csrc/fd_shared_plan.h):

    python tests/tools/shared_plan_digest.py > listing.txt          # in each of the two trees; the listings must be equal

Fixed seed, N = 1025 vertices of the head mesh (full vertex groups and a partial one in every variant), linear term.  Thin-plate
and QNN; F in {1, 4, 5, 12, 13, 16, 17, 20, 21, 24, 28, 32} frames of one rest rig; M in {32, 256} centres and the two residency
boundaries of tests/golden/shared_plan_table.txt, 352 | 368 (at 32 frames) and 512 | 528 (at 20).  Each once with dist2
uniform on [0, radius2 / 0.9) -- about a tenth of the vertices gated -- and projection frames ("general": the general
epilogue), and once with neither ("plain": the straight-line epilogue for the full groups).  A digest covers, frame by frame,
P_out, fd_falloff and N_out.  A tool, not a test."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from facedeform_amd import capi, synth   # noqa: E402

N, RADIUS2, RATE = 1025, 0.36, 1.7
FRAMES = (1, 4, 5, 12, 13, 16, 17, 20, 21, 24, 28, 32)
CENTRES = (32, 256, 352, 368, 512, 528)
KINDS = [("thin_plate", capi.KERNEL_THIN_PLATE, []), ("qnn", capi.KERNEL_GAUSSIAN_QNN, [1.0, 5.0])]


def main():
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    dev = torch.device("cuda", 0)
    Fmax = max(FRAMES)
    P = synth.head_mesh(20_500)[::20][:N].copy()
    n0 = P.astype(np.float64) / np.array([0.75, 1.0, 0.85]) ** 2
    n0 /= np.linalg.norm(n0, axis=1, keepdims=True)
    u = np.cross(n0, [0.3, 0.2, 1.0]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n0, u)
    tu, tv, nrm = (1.3 * u).astype(np.float32), (0.8 * v).astype(np.float32), n0.astype(np.float32)
    dist2 = (np.random.default_rng(5).random(N) * RADIUS2 / 0.9).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_P, d_tu, d_tv, d_nrm, d_d2, d_Nv = (t(a) for a in (P, tu, tv, nrm, dist2, np.cross(tu, tv).astype(np.float32)))
    print("# %d of %d vertices gated" % (int((dist2 > RADIUS2).sum()), N))
    for label, kind, params in KINDS:
        for M in CENTRES:
            rest = synth.control_points(M, "head")
            deltas = np.stack([synth.smooth_deltas(rest, f % 8) * np.float32(1.0 + 0.25 * (f // 8)) for f in range(Fmax)]).astype(np.float32)
            d_rest, d_del = t(rest), t(deltas)
            engines = []
            for _ in range(Fmax):
                e = capi.Engine(device=0, precision=capi.EVAL_FP32)
                e.set_kernel(kind, params); e.set_term(capi.TERM_LINEAR)
                engines.append(e)
            full = capi.Batch(engines)
            full.set_points_dev([d_rest.data_ptr()] * Fmax, [d_del.data_ptr() + f * M * 12 for f in range(Fmax)], M)
            full.build_async()
            built = sum(r.terminationtype == 1 for r in full.build_result())
            for F in FRAMES:
                batch = capi.Batch(engines[:F])
                for mode in ("general", "plain"):
                    mk = lambda w: [torch.full((N, w) if w else (N,), -7.0, device=dev) for _ in range(F)]
                    ptr = lambda ts: [x.data_ptr() for x in ts]
                    oP, ofall, oN = mk(3), mk(0), mk(3)
                    kw = dict(d_falloff=ptr(ofall), d_N=d_Nv.data_ptr(), d_N_out=ptr(oN), radius2=RADIUS2, falloffrate=RATE)
                    if mode == "general":
                        kw.update(d_dist2=d_d2.data_ptr(), d_tangents=(d_tu.data_ptr(), d_tv.data_ptr(), d_nrm.data_ptr()))
                    torch.cuda.synchronize()
                    batch.deform_vectors_shared_dev(N, d_P.data_ptr(), ptr(oP), **kw)
                    torch.cuda.synchronize()
                    h = hashlib.sha256()
                    for f in range(F):
                        for o in (oP, ofall, oN):
                            h.update(o[f].cpu().numpy().tobytes())
                    print("%-10s M=%-3d F=%-2d %-7s built=%d/%d %-26s %-29s %s" % (
                        label, M, F, mode, built, Fmax, capi.fd_shared_kernel_name(M, F, kind) or "-",
                        capi.fd_shared_vectors_kernel_name(M, F, kind) or "-", h.hexdigest()), flush=True)
                batch.close()
            full.close()
            for e in engines:
                e.close()


if __name__ == "__main__":
    main()
