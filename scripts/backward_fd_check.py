"""CPU check of what a backward-pass gradient means at a K-iteration iterate: the adjoint
gradient (tests/_backward_ref.py, the reference of the GPU kernels) against central differences of the
WHOLE solve, oracle.qp_former -> K Mehrotra iterations from the cold start, for L = w^T u0.
Usage: python scripts/backward_fd_check.py [K] [N ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from biped_pympc_amd import layout  # noqa: E402
from biped_pympc_amd.utils.synthetic import make_workload  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import _backward_ref as br  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 35
for N in [int(a) for a in sys.argv[2:]] or [2, 5]:
    wl = make_workload(1, N, seed=30 + N, random_gait=True, residuals=True)
    P = wl.inputs
    rng = np.random.default_rng(3)
    w = rng.standard_normal(12)
    g = np.zeros((1, 24 * N))
    g[0, 12 * N:12 * N + 12] = w

    def loss(Pp):
        return float(oracle.mpc_solve(N, K, Pp)[0][0, 12 * N:12 * N + 12] @ w)
    it = oracle.mpc_solve(N, K, P)[:4]
    grads = br.mpc_backward_batch(N, P, it, g)
    for i in (0, 3, 4, 13, 14, 10, 11, 15, 16):
        a = np.abs(P[i])
        dv = rng.standard_normal(P[i].shape) * np.where(a > 0, a, 1.0)
        an = float((grads[i] * dv).sum())
        fds = []
        for t in (1e-5, 5e-6):
            Pp = [q.copy() for q in P]
            Pm = [q.copy() for q in P]
            Pp[i] = P[i] + t * dv
            Pm[i] = P[i] - t * dv
            fds.append((loss(Pp) - loss(Pm)) / (2 * t))
        print(f"N={N} K={K} {layout.FORMER_IN_NAMES[i]:>20}: analytic {an: .6e}  fd {fds[0]: .6e} {fds[1]: .6e}  "
              f"rel diff {abs(fds[1] - an) / max(abs(an), 1e-300):.2e}")
