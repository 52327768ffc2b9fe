"""Cost of the full-seed backward pass (seeds on x, s, z, y and the objective), by the method of
scripts/backward_timing.py: B = 4096 at N = 10 and 20, HIP events, warmed up, the legs alternating in one
process, median of 30 x 10 calls.

Legs on this build: the x-only adjoint and srbd_mpc_backward, and the same two with a full seed (`all`: every
cotangent given). With --parent-lib (a libsrbd_mpc.so built from the parent commit) the x-only legs are also
timed on that library, twice (parent_a, parent_b: their distance is the spread of the measurement), and the
x-only outputs of the two libraries are compared bit for bit. Prints one JSON line per horizon.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from biped_pympc_amd import _native, solver  # noqa: E402
from biped_pympc_amd.utils.synthetic import make_workload  # noqa: E402


def _parent(path):
    """The two x-only entries of another build, bound by hand (their signatures are this build's)."""
    L = ctypes.CDLL(path)
    P, dp = ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p
    L.srbd_pdipm_backward.restype = ctypes.c_int
    L.srbd_pdipm_backward.argtypes = [ctypes.c_int, ctypes.c_int, P, dp, P, dp, ctypes.c_void_p]
    L.srbd_mpc_backward.restype = ctypes.c_int
    L.srbd_mpc_backward.argtypes = [ctypes.c_int, ctypes.c_int, P, P, dp, dp, P, dp, ctypes.c_void_p]
    L.srbd_build_id.restype = ctypes.c_char_p
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizons", type=int, nargs="+", default=[10, 20])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--parent-lib", default=None, help="libsrbd_mpc.so of the parent commit")
    args = ap.parse_args()
    B = args.batch
    par = _parent(args.parent_lib) if args.parent_lib else None
    for N in args.horizons:
        wl = make_workload(B, N, seed=7, random_gait=True)
        ins = [torch.from_numpy(a).cuda() for a in wl.inputs]
        H, f, A, b, G, d = solver.qp_former(ins, N)
        qp = [H, G, A, f, d, b]
        it = [t.clone() for t in solver.mpc_solve(ins, N, 10)[:4]]
        rng = np.random.default_rng(1)
        g = torch.from_numpy(rng.standard_normal((B, 24 * N))).cuda()
        full = {"grad_s": torch.from_numpy(rng.standard_normal((B, 16 * N))).cuda(),
                "grad_z": torch.from_numpy(rng.standard_normal((B, 16 * N))).cuda(),
                "grad_y": torch.from_numpy(rng.standard_normal((B, 14 * N))).cuda(),
                "grad_objective": torch.from_numpy(rng.standard_normal(B)).cuda()}
        grads = solver.pdipm_backward(qp, it, g, N)
        in_grads = solver.qp_former_backward(ins, grads, N)
        ws = torch.empty(_native.lib().srbd_mpc_backward_workspace_doubles(N, B), dtype=torch.float64, device="cuda")
        legs = {
            "adjoint_x": lambda: solver.pdipm_backward(qp, it, g, N, outputs=grads),
            "adjoint_all": lambda: solver.pdipm_backward(qp, it, g, N, outputs=grads, **full),
            "mpc_backward_x": lambda: solver.mpc_backward(ins, it, g, N, outputs=in_grads, workspace=ws),
            "mpc_backward_all": lambda: solver.mpc_backward(ins, it, g, N, outputs=in_grads, workspace=ws, **full),
        }
        bits = None
        if par is not None:
            p_grads, p_in = [torch.empty_like(t) for t in grads], [torch.empty_like(t) for t in in_grads]
            a_qp, a_g, a_ig = solver._ptrs(qp + it), solver._ptrs(p_grads), solver._ptrs(p_in)
            a_ins, a_it = solver._ptrs(ins), solver._ptrs(it)

            def p_adjoint():
                rc = par.srbd_pdipm_backward(N, B, a_qp, g.data_ptr(), a_g, None, solver._stream_ptr())
                assert rc == 0, rc

            def p_mpc():
                rc = par.srbd_mpc_backward(N, B, a_ins, a_it, g.data_ptr(), ws.data_ptr(), a_ig, None,
                                           solver._stream_ptr())
                assert rc == 0, rc
            p_adjoint()
            new = [t.clone() for t in solver.pdipm_backward(qp, it, g, N)]
            p_mpc()
            new_in = [t.clone() for t in solver.mpc_backward(ins, it, g, N)]
            torch.cuda.synchronize()
            bits = (all(torch.equal(a, b) for a, b in zip(new, p_grads))
                    and all(torch.equal(a, b) for a, b in zip(new_in, p_in)))
            legs.update({"parent_a_adjoint_x": p_adjoint, "parent_a_mpc_backward_x": p_mpc,
                         "parent_b_adjoint_x": p_adjoint, "parent_b_mpc_backward_x": p_mpc})
        times = {k: [] for k in legs}
        for fn in legs.values():  # warm-up: every leg, every shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):  # the legs alternate inside every repetition
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.inner)
        med = {k: statistics.median(v) for k, v in times.items()}
        out = {"N": N, "B": B, "build_id": _native.build_id(), "reps": args.reps, "inner": args.inner,
               "median_ms": {k: round(v, 4) for k, v in med.items()},
               "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
               "all_over_x": {"adjoint": round(med["adjoint_all"] / med["adjoint_x"], 4),
                              "mpc_backward": round(med["mpc_backward_all"] / med["mpc_backward_x"], 4)}}
        if par is not None:
            out["parent_build_id"] = par.srbd_build_id().decode()
            out["x_only_bits_equal_parent"] = bits
            for leg in ("adjoint_x", "mpc_backward_x"):
                pa, pb = med["parent_a_" + leg], med["parent_b_" + leg]
                out[leg + "_vs_parent"] = {"new_over_parent_a": round(med[leg] / pa, 4),
                                           "parent_b_over_parent_a": round(pb / pa, 4)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
