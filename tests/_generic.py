"""The generic workload of the parity tests (TEST INFRASTRUCTURE ONLY): former inputs on which no two envs
share a scalar, the inertia is not symmetric and no product of the former is exact.

make_workload's inputs are special: dt, mass, mu, Q and R are batch constants, I_world = R I_body R^T is
exactly symmetric, and the linearisation point (x, u) is all ones with mu = 1. A kernel that reads another
env's scalar, decodes I_world transposed, uses I^-1 where I^-T belongs, or rounds the products of former_f /
former_d differently from the oracle passes every test drawn from it. generic_former_inputs removes each of
these coincidences; tests/test_generic_inputs.py holds, on the oracle alone, that the inputs it returns do
expose such errors.

The solver cases that compare the GPU with oracle.mpc_solve at a fixed tolerance (solver_case_inputs) follow
the seed rule of tests/test_sweep_floor.py: seed = SOLVER_SEED_BASE + N + 100 j for the first j >= 0 at which
every env's floor between the two CPU restatements is at most a quarter of the tolerance at every K used; the
adjoint cases (adjoint_workload) the same rule on the reduced-elimination floor. The j found are recorded
here as constants and held on the CPU by tests/test_generic_inputs.py.
"""
from __future__ import annotations

import functools

import numpy as np

from biped_pympc_amd.utils.synthetic import Q_DEFAULT, R_DEFAULT, make_workload, solver_init


def generic_former_inputs(B: int, N: int, seed: int, solvable: bool = True) -> list:
    """The 17 former inputs (B, nnz_in[i]) float64: make_workload(B, N, seed, random_gait=True,
    residuals=True) with, per env and from an independent generator,

      dt ~ U[0.02, 0.05]          unmasks a read of another env's (or another wave's) dt
      mass ~ U[8, 20]             ... of another env's mass
      mu ~ U[0.3, 1.2]            ... of another env's mu; mu != 1 makes the products mu * fz of former_d round
      Q, R = defaults * exp(U[-1, 1]) per entry
                                  ... of another env's weights; q (x - x_ref) - q x and r u - r u then round
      x ~ N(0, 1), u ~ N(0, 30)   the linearisation point: a read of inputs 1 and 2 is no longer a constant,
                                  and every product of former_f and former_d is inexact
      I_world += 0.02 * 0.0691 * U[-1, 1]^(3x3)
                                  asymmetric (and still invertible: the perturbation is 2 % of the smallest
                                  principal moment): a transposed decode, or I^-1 where I^-T belongs, shows

    and with solvable=False (the former and its VJP alone; such a QP is not a contact problem any more)

      R_body += 0.05 * U[-1, 1]^9 not orthonormal: R^T where R^-1 was meant, or a transposed decode, shows
      contact table ~ U[0, 1]     fractional: d = Fmax * ct is a product that rounds, and a flag test
                                  (ct != 0) in place of the product shows
    """
    wl = make_workload(B, N, seed, random_gait=True, residuals=True)
    P = [a.copy() for a in wl.inputs]
    rng = np.random.default_rng([seed, 0x6E67])  # independent of make_workload's stream
    P[4] = rng.uniform(0.02, 0.05, (B, 1))
    P[5] = rng.uniform(8.0, 20.0, (B, 1))
    P[6] = rng.uniform(0.3, 1.2, (B, 1))
    P[13] = Q_DEFAULT[None, :] * np.exp(rng.uniform(-1.0, 1.0, (B, 12)))
    P[14] = R_DEFAULT[None, :] * np.exp(rng.uniform(-1.0, 1.0, (B, 12)))
    P[1] = rng.standard_normal((B, 12 * N))
    P[2] = 30.0 * rng.standard_normal((B, 12 * N))
    P[8] = P[8] + 0.02 * 0.0691 * rng.uniform(-1.0, 1.0, (B, 9))
    if not solvable:
        P[7] = P[7] + 0.05 * rng.uniform(-1.0, 1.0, (B, 9))
        P[12] = rng.uniform(0.0, 1.0, (B, 2 * N))
    return [np.ascontiguousarray(a, np.float64) for a in P]


def d_row_terms(N: int, P) -> np.ndarray:
    """(B, 16N): |t1| + |t2| of every row of d = G z - ineq(z), t1 and t2 the row's two products at the
    linearisation point u (former_d: rows k = 0..3 of a foot -+fx|fy and mu fz, 4 and 5 l fz and my, 6 fz
    alone, 7 fz and Fmax ct). Rows 0..6 cancel to rounding level, row 7 is Fmax ct."""
    from biped_pympc_amd import layout
    u, mu, ct = np.asarray(P[2]), np.asarray(P[6]), np.asarray(P[12])
    B = u.shape[0]
    u = u.reshape(B, N, 12)
    out = np.empty((B, N, 2, 8))
    for f in range(2):
        fx, fy, fz = (np.abs(u[:, :, 3 * f + k]) for k in range(3))
        my = np.abs(u[:, :, 7 + 3 * f])
        mfz = np.abs(mu * fz)
        out[:, :, f, 0] = out[:, :, f, 1] = fx + mfz
        out[:, :, f, 2] = out[:, :, f, 3] = fy + mfz
        out[:, :, f, 4] = layout.LT * fz + my
        out[:, :, f, 5] = layout.LH * fz + my
        out[:, :, f, 6] = fz
        out[:, :, f, 7] = fz + np.abs(layout.F_MAX * ct[:, N * f:N * f + N])
    return out.reshape(B, 16 * N)


def d_cancelling_rows(N: int) -> np.ndarray:
    """(16N,) bool: the seven rows per foot and stage whose value is an exact zero in exact arithmetic."""
    return np.arange(16 * N) % 8 != 7


def g_mu_entries(N: int) -> np.ndarray:
    """(28N,) bool: the CCS entries of G that hold -mu (friction rows 0..3 of a foot, its fz column)."""
    from biped_pympc_amd import layout
    Gp, Gi = layout.ccs_G(N)
    Gc = np.repeat(np.arange(len(Gp) - 1), np.diff(Gp)) % 12
    return (Gc % 3 == 2) & (Gc < 6) & (np.asarray(Gi) % 8 < 4)


# ---- the solver cases (tests/test_gpu_generic.py, fused step vs oracle.mpc_solve) ----

SOLVER_HORIZONS = [1, 3, 10, 16, 20, 32]  # the LDS step, then 1, 1, 2, 2 and 3 waves per QP
SOLVER_BATCH = 16
SOLVER_SEED_BASE = 2300
# j of the seed rule per horizon (0 where not listed); tests/test_generic_inputs.py holds it
SOLVER_SEED_J: dict = {}


def solver_case_seed(N: int, j: int | None = None) -> int:
    return SOLVER_SEED_BASE + N + 100 * (SOLVER_SEED_J.get(N, 0) if j is None else j)


@functools.lru_cache(maxsize=None)
def solver_case_inputs(N: int, j: int | None = None):
    """(the 17 former inputs, the 10 solver inputs of the cold start) of the solver case at horizon N."""
    from oracle import oracle
    P = generic_former_inputs(SOLVER_BATCH, N, solver_case_seed(N, j), solvable=True)
    H, f, A, b, G, d = oracle.qp_former(N, P)
    return P, [H, G, A, f, d, b, *solver_init(d, N)]


# ---- the adjoint cases (tests/test_gpu_generic.py, adjoint kernel vs the dense refined reference) ----

ADJOINT_HORIZONS = [1, 2, 3, 10]
ADJOINT_KS = [1, 5]
ADJOINT_SEED_BASE = 2900
ADJOINT_SEED_J: dict = {}


def adjoint_seed(N: int, j: int | None = None) -> int:
    return ADJOINT_SEED_BASE + N + 100 * (ADJOINT_SEED_J.get(N, 0) if j is None else j)


@functools.lru_cache(maxsize=None)
def adjoint_workload(N: int, j: int | None = None):
    """(former inputs, QP in the solver's input order) as tests/_backward_cases.py workload returns them."""
    from oracle import oracle
    from tests import _backward_cases as C
    P = generic_former_inputs(C.BATCH, N, adjoint_seed(N, j), solvable=True)
    H, f, A, b, G, d = oracle.qp_former(N, P)
    return P, [H, G, A, f, d, b]
