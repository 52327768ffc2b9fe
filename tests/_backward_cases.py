"""The cases of the backward-pass GPU tests (tests/test_gpu_backward.py) and their CPU reference, computed
once per (horizon, gait, K) and shared (TEST INFRASTRUCTURE ONLY).

Inputs: make_workload(16, N, seed=900 + N), fixed and randomised gait; iterates from oracle.pdipm after K
iterations from the GPU caller's cold start; two seeds per case, one random on the u0 block only and one
random on all of x. The horizons are the smallest at which each code path first appears: 1 (no coupling
block), 2 (first coupling, the last-stage column rule), 3 (an interior stage), 10 (the deployed horizon),
32 (largest LDS footprint; the 2N and 3N task loops wrap past 64 lanes).
"""
from __future__ import annotations

import functools

import numpy as np

from biped_pympc_amd.utils.synthetic import make_workload, solver_init
from oracle import oracle
from tests import _backward_ref as br
from tests._util import rel_err_rows

HORIZONS = [1, 2, 3, 10, 32]
GAITS = ["fixed", "random"]
BATCH = 16
# the project's SOLVER_CASES (tests/test_gpu_parity.py): the backward is one solve with the forward's
# factorisation, at the iterate K iterations reach
CASES = [(1, 1e-10), (5, 1e-9), (10, 1e-7), (20, 1e-5)]
NAMES = ["grad_H", "grad_f", "grad_A", "grad_b", "grad_G", "grad_d"]


@functools.lru_cache(maxsize=None)
def workload(N: int, gait: str):
    """(former inputs, QP in the solver's input order [H, G, A, f, d, b]) as numpy arrays. `gait` names the
    workload: "fixed" / "random" (make_workload), or "generic" (tests/_generic.py adjoint_workload: per-env
    scalars, asymmetric inertia, a generic linearisation point); iterate, reference and reduced_floor below
    take the same name."""
    if gait == "generic":
        from tests import _generic
        return _generic.adjoint_workload(N)
    wl = make_workload(BATCH, N, seed=900 + N, random_gait=(gait == "random"))
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    return wl.inputs, [H, G, A, f, d, b]


@functools.lru_cache(maxsize=None)
def iterate(N: int, gait: str, K: int):
    _, qp = workload(N, gait)
    return [np.asarray(v) for v in oracle.pdipm(N, K, qp + list(solver_init(qp[4], N)))[:4]]


@functools.lru_cache(maxsize=None)
def seeds(N: int):
    """[seed on the u0 block only, seed on all of x], each (BATCH, 24N)."""
    rng = np.random.default_rng(1900 + N)
    g_all = rng.standard_normal((BATCH, 24 * N))
    g_u0 = np.zeros_like(g_all)
    g_u0[:, 12 * N:12 * N + 12] = rng.standard_normal((BATCH, 12))
    return [g_u0, g_all]


@functools.lru_cache(maxsize=None)
def reference(N: int, gait: str, K: int):
    """Per seed, the six reference gradients (BATCH, width) of the dense refined adjoint."""
    _, qp = workload(N, gait)
    it = iterate(N, gait, K)
    sd = seeds(N)
    rows = [br.pdipm_backward_seeds(N, [a[e] for a in qp] + [v[e] for v in it], [g[e] for g in sd])
            for e in range(BATCH)]
    return [[np.stack([rows[e][k][o] for e in range(BATCH)]) for o in range(6)] for k in range(len(sd))]


@functools.lru_cache(maxsize=None)
def reduced_floor(N: int, gait: str, K: int):
    """Per seed, (6, BATCH): the per-env, per-output norm-wise distance between the plain-FP64 reduced
    elimination and the refined dense adjoint -- the FP64 floor of the elimination the kernel runs."""
    _, qp = workload(N, gait)
    it = iterate(N, gait, K)
    ref = reference(N, gait, K)
    out = []
    for k, g in enumerate(seeds(N)):
        red = br.pdipm_backward_batch(N, qp + it, g, reduced=True)
        out.append(np.stack([rel_err_rows(red[o], ref[k][o]) for o in range(6)]))
    return out
