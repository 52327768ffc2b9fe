"""The multi-seed backward tests' reference and floor (TEST INFRASTRUCTURE ONLY), computed once per
(horizon, gait, K) of tests/_backward_cases.py and shared by tests/test_backward_multi_ref.py (CPU) and
tests/test_gpu_backward_multi.py.

Seeds: the 12 unit vectors on the u0 block of x (the rows of the feedback gain d u0 / d x0).
Reference chain: the dense refined adjoint (tests/_backward_ref.py adjoint_dense, one LU for the 12
columns) -> qp_gradients -> former_vjp, per env and per seed row.
Floor: ``adjoint_reduced_refined`` restates what the kernel does -- the reduced elimination in plain FP64
followed by ONE refinement step against the full K, residual and correction in plain FP64 too -- and its
distance to the reference chain, per env and seed row, is the FP64 floor of that algorithm on a problem.
(The unrefined ``adjoint_reduced`` is no valid floor for unit seeds: on the x-moment columns u[6], u[9]
it is off by up to 2e-3.)
"""
from __future__ import annotations

import functools

import numpy as np

from tests import _backward_cases as C
from tests import _backward_ref as br

M_GAIN = 12
ASSERTED = (0, 3, 16)  # x0 (the gain), x_ref, residual_ang_accel: asserted against the CASES tolerance


def u0_rows(N: int):
    return list(range(12 * N, 12 * N + 12))


def unit_seed_block(N: int) -> np.ndarray:
    """(12, 24N): the unit vectors on the u0 block."""
    g = np.zeros((M_GAIN, 24 * N))
    g[np.arange(M_GAIN), u0_rows(N)] = 1.0
    return g


def adjoint_reduced_refined(N, Hv, Gv, Av, s, z, g):
    """The kernel's algorithm in plain FP64: reduced elimination, then one refinement step whose residual
    is taken against the full K (all four rows) and whose correction goes through the same reduced
    elimination with the same factors. g: (24N, k) columns. Returns (lx, ls, lz, ly), columns."""
    from scipy.linalg import lu_factor, lu_solve
    H, G, A = br.dense_qp(N, Hv, Gv, Av)
    nz, m, p = 24 * N, 16 * N, 14 * N
    s, z = np.asarray(s, np.float64), np.asarray(z, np.float64)
    W = (z / s + br.DELTA)[:, None]
    D = 1.0 / (1.0 + br.DELTA * W)
    lam = D * W
    Hb = H + br.BETA * np.eye(nz)
    lu = lu_factor(np.block([[Hb + G.T @ (lam * G), A.T], [A, -br.DELTA * np.eye(p)]]), check_finite=False)

    def reduced(e1, e2, e3, e4):
        q = D * (e2 - W * e3)
        sol = lu_solve(lu, np.concatenate([e1 - G.T @ q, e4]), check_finite=False)
        dx, dy = sol[:nz], sol[nz:]
        gd = G @ dx
        return dx, e3 + br.DELTA * q + (br.DELTA * lam - 1.0) * gd, q + lam * gd, dy

    g = np.asarray(g, np.float64)
    k = g.shape[1]
    zm, zp = np.zeros((m, k)), np.zeros((p, k))
    lx, ls, lz, ly = reduced(g, zm, zm, zp)
    e1 = g - (Hb @ lx + G.T @ lz + A.T @ ly)
    e2 = -(W * ls + lz)
    e3 = -(G @ lx + ls - br.DELTA * lz)
    e4 = -(A @ lx - br.DELTA * ly)
    cx, cs, cz, cy = reduced(e1, e2, e3, e4)
    return lx + cx, ls + cs, lz + cz, ly + cy


def _chain(N, ins, qp, it, e, lam):
    """lam (columns) of env e -> (17 former-input gradients, each (k, width))."""
    x, _, z, y = (np.asarray(v[e], np.float64) for v in it)
    P = [np.asarray(a)[e] for a in ins]
    rows = [br.former_vjp(N, P, br.qp_gradients(N, [v[:, k] for v in lam], x, z, y)) for k in range(lam[0].shape[1])]
    return [np.stack([r[i] for r in rows]) for i in range(17)]


@functools.lru_cache(maxsize=None)
def _both(N: int, gait: str, K: int):
    ins, qp = C.workload(N, gait)
    it = C.iterate(N, gait, K)
    g = unit_seed_block(N).T
    ref, red = [], []
    for e in range(C.BATCH):
        Hv, Gv, Av = qp[0][e], qp[1][e], qp[2][e]
        ref.append(_chain(N, ins, qp, it, e, br.adjoint_dense(N, Hv, Gv, Av, it[1][e], it[2][e], g)))
        red.append(_chain(N, ins, qp, it, e, adjoint_reduced_refined(N, Hv, Gv, Av, it[1][e], it[2][e], g)))
    stack = lambda rows: [np.stack([r[i] for r in rows]) for i in range(17)]  # noqa: E731
    return stack(ref), stack(red)


def unit_reference(N: int, gait: str, K: int):
    """The reference Jacobians d u0 / d input: 17 arrays (BATCH, 12, width)."""
    return _both(N, gait, K)[0]


def row_err(a, b) -> np.ndarray:
    """Norm-wise relative error per env and per seed row: (B, M) from two (B, M, width) arrays. A row
    whose reference is exactly zero (a former input the solution does not depend on) compares absolutely."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max(axis=2)
    return np.abs(a - b).max(axis=2) / np.where(scale > 0.0, scale, 1.0)


def unit_floor(N: int, gait: str, K: int):
    """Per former input, (BATCH, 12): the distance of the plain-FP64 restatement of the kernel's algorithm
    from the reference chain."""
    ref, red = _both(N, gait, K)
    return [row_err(red[i], ref[i]) for i in range(17)]
