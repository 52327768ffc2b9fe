"""Time of the controller step's backward chain (srbd_mpc_step_backward: wrench VJP -> adjoint KKT solve and
former VJP -> input-preparation VJP) next to srbd_mpc_backward alone: B = 4096 at N = 10 and 20,
HIP events, warmed up, the legs alternating in one process -- the method of scripts/backward_timing.py.

The chain adds two small launches and the FP32 gradients' stores; `wrt` narrows the former-input cotangents the
middle materialises (the dt_mpc / residual request of an RL policy is timed next to the full one). Prints one
JSON line per horizon.
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

POLICY_FIELDS = ("dt_mpc", "residual_lin_accel", "residual_ang_accel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizons", type=int, nargs="+", default=[10, 20])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    args = ap.parse_args()
    B = args.batch
    rng = np.random.default_rng(1)
    for N in args.horizons:
        wl = make_workload(B, N, seed=7, random_gait=True, residuals=True)
        ins = [torch.from_numpy(a).cuda() for a in wl.inputs]
        it = [t.clone() for t in solver.mpc_solve(ins, N, 10)[:4]]
        # the FP32 tensors the preparation's VJP reads; the former inputs above stand for what a step wrote
        rot = torch.from_numpy(np.linalg.qr(rng.normal(size=(B, 3, 3)))[0].astype(np.float32)).cuda()
        vb = torch.from_numpy(rng.uniform(-1, 1, (B, 3)).astype(np.float32)).cuda()
        wb = torch.from_numpy(rng.uniform(-1, 1, (B, 3)).astype(np.float32)).cuda()
        dt = ins[4].reshape(B).float().contiguous()
        first = torch.zeros(B, dtype=torch.bool, device="cuda")
        p = _native.MPCPrep()
        p.rotation_body, p.desired_velocity_b, p.desired_angular_velocity_b = rot.data_ptr(), vb.data_ptr(), wb.data_ptr()
        p.dt_mpc, p.first_run = dt.data_ptr(), first.data_ptr()
        p.I_body[:] = [0.5413, 0, 0, 0, 0.52, 0, 0, 0, 0.0691]
        p.step_dt, p.literal_layout, p.q_len = 0.01, 1, 13
        gw = torch.from_numpy(rng.standard_normal((B, 2, 6)).astype(np.float32)).cuda()
        g = solver.u0_wrench_backward(it[0], rot, gw, N)[0]
        in_grads = solver.mpc_backward(ins, it, g, N)
        L = _native.lib()
        ws_b = torch.empty(L.srbd_mpc_backward_workspace_doubles(N, B), dtype=torch.float64, device="cuda")
        ws_s = torch.empty(L.srbd_mpc_step_backward_workspace_doubles(N, B, 0), dtype=torch.float64, device="cuda")
        all_fields = _native.PREP_GRAD_NAMES
        outs = {n: torch.empty((B,) + _native.prep_grad_shape(n, N), dtype=torch.float32, device="cuda") for n in all_fields}

        def step_backward(fields):
            ptrs = _native.ptr_array([outs[n].data_ptr() if n in fields else 0 for n in all_fields])
            rc = L.srbd_mpc_step_backward(N, B, ctypes.byref(p), solver._ptrs(ins), solver._ptrs(it), gw.data_ptr(), 0,
                                          None, None, None, None, None, ws_s.data_ptr(), ptrs, None, solver._stream_ptr())
            _native.check(rc, "srbd_mpc_step_backward")

        legs = {
            "mpc_backward": lambda: solver.mpc_backward(ins, it, g, N, outputs=in_grads, workspace=ws_b),
            "step_backward_all": lambda: step_backward(all_fields),
            "step_backward_policy": lambda: step_backward(POLICY_FIELDS),
            "wrench_backward": lambda: solver.u0_wrench_backward(it[0], rot, gw, N, grad_x=g),
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
            "N": N, "B": B, "build_id": _native.build_id(), "reps": args.reps, "inner": args.inner,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
            "step_backward_all_over_mpc_backward": round(med["step_backward_all"] / med["mpc_backward"], 3),
            "step_backward_policy_over_mpc_backward": round(med["step_backward_policy"] / med["mpc_backward"], 3),
        }), flush=True)


if __name__ == "__main__":
    main()
