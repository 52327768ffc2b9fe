"""Time of the multi-seed backward pass ("Several seeds at one iterate") with the method of
scripts/backward_timing.py: B = 4096 at N = 10 and 20, HIP events, warmed up, the legs alternating in one
process, the median of 30 repetitions of 10 calls.

  a  pdipm_backward_multi, M = 12 unit seeds on u0 (one factorisation, 12 solves, one launch)
  b  12 pdipm_backward calls on materialised seeds: the path without this entry point, the baseline
  c  mpc_feedback_gain end to end (qp_former, the adjoint kernel writing grad_b only, the former VJP)
  d  one forward fused step (mpc_solve) at K = 10

Prints one JSON line per horizon: the medians, a / b, c as a multiple of d, and the gain's workspace bytes
per env.
"""
import argparse
import json
import os
import statistics
import sys

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
    B, M = args.batch, 12
    for N in args.horizons:
        wl = make_workload(B, N, seed=7, random_gait=True)
        ins = [torch.from_numpy(a).cuda() for a in wl.inputs]
        H, f, A, b, G, d = solver.qp_former(ins, N)
        qp = [H, G, A, f, d, b]
        buffers = solver.MPCSolveBuffers.allocate(N, B, "cuda")
        it = [t.clone() for t in solver.mpc_solve(ins, N, 10)[:4]]
        unit = solver.unit_seeds(N, range(12 * N, 12 * N + 12))
        full = [unit[k].expand(B, -1).contiguous() for k in range(M)]  # what 12 single calls read
        multi = solver.pdipm_backward_multi(qp, it, unit, N)
        single = solver.pdipm_backward(qp, it, full[0], N)
        n_ws = _native.lib().srbd_mpc_backward_multi_workspace_doubles(N, B, M, 1)
        ws = torch.empty(n_ws, dtype=torch.float64, device="cuda")
        gain = torch.empty((B, 12, 12), dtype=torch.float64, device="cuda")

        def twelve():
            for k in range(M):
                solver.pdipm_backward(qp, it, full[k], N, outputs=single)

        legs = {
            "a_multi_12": lambda: solver.pdipm_backward_multi(qp, it, unit, N, outputs=multi),
            "b_12_single_calls": twelve,
            "c_feedback_gain": lambda: solver.mpc_feedback_gain(ins, it, N, seeds=unit, out=gain, workspace=ws),
            "d_forward_step_K10": lambda: solver.mpc_solve(ins, N, 10, buffers=buffers),
        }
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
        print(json.dumps({
            "N": N, "B": B, "M": M, "build_id": _native.build_id(), "reps": args.reps, "inner": args.inner,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
            "a_over_b": round(med["a_multi_12"] / med["b_12_single_calls"], 3),
            "c_in_forward_steps": round(med["c_feedback_gain"] / med["d_forward_step_K10"], 3),
            "gain_workspace_bytes_per_env": 8 * n_ws // B,
        }), flush=True)


if __name__ == "__main__":
    main()
