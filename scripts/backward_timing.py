"""Time of the backward pass next to one forward Newton iteration of the LDS-resident solver (DESIGN.md
"Backward pass"): B = 4096 at N = 10 and 20, HIP events, warmed up, the legs alternating in one process.

One forward iteration = (t(K = 10) - t(K = 5)) / 5 of solver.pdipm under the "lds" solver path (launch,
load and epilogue cancel). The adjoint kernel is one factorisation, one solve and one refinement step,
so the structure predicts one to two forward iterations. Prints one JSON line per horizon.
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizons", type=int, nargs="+", default=[10, 20])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    args = ap.parse_args()
    B = args.batch
    for N in args.horizons:
        wl = make_workload(B, N, seed=7, random_gait=True)
        ins = [torch.from_numpy(a).cuda() for a in wl.inputs]
        H, f, A, b, G, d = solver.qp_former(ins, N)
        qp = [H, G, A, f, d, b]
        it = [t.clone() for t in solver.mpc_solve(ins, N, 10)[:4]]
        g = torch.from_numpy(np.random.default_rng(1).standard_normal((B, 24 * N))).cuda()
        out_f = solver._alloc_solver_outputs(B, N, "cuda")
        grads = solver.pdipm_backward(qp, it, g, N)
        in_grads = solver.qp_former_backward(ins, grads, N)
        ws = torch.empty(_native.lib().srbd_mpc_backward_workspace_doubles(N, B), dtype=torch.float64, device="cuda")
        legs = {
            "forward_lds_K5": lambda: solver.pdipm(qp, None, N, 5, outputs=out_f),
            "forward_lds_K10": lambda: solver.pdipm(qp, None, N, 10, outputs=out_f),
            "adjoint": lambda: solver.pdipm_backward(qp, it, g, N, outputs=grads),
            "former_backward": lambda: solver.qp_former_backward(ins, grads, N, outputs=in_grads),
            "mpc_backward": lambda: solver.mpc_backward(ins, it, g, N, outputs=in_grads, workspace=ws),
        }
        times = {k: [] for k in legs}
        with _native.solver_path("lds"):
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
        spread = {k: (min(v), max(v)) for k, v in times.items()}
        it_ms = (med["forward_lds_K10"] - med["forward_lds_K5"]) / 5.0
        print(json.dumps({
            "N": N, "B": B, "build_id": _native.build_id(), "reps": args.reps, "inner": args.inner,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_max_ms": {k: [round(a, 4), round(b, 4)] for k, (a, b) in spread.items()},
            "forward_iteration_ms": round(it_ms, 4),
            "adjoint_in_forward_iterations": round(med["adjoint"] / it_ms, 3),
            "mpc_backward_in_forward_iterations": round(med["mpc_backward"] / it_ms, 3),
        }), flush=True)


if __name__ == "__main__":
    main()
