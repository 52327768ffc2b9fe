"""NumPy reference of the backward pass with seeds on every output of a solve (TEST INFRASTRUCTURE ONLY):
cotangents g_x, g_s, g_z, g_y of (x, s, z, y) and g_J of the objective J = 1/2 x^T H x + f^T x.

The adjoint is the solution of the dense KKT of ``tests/_backward_ref.py`` with the full right-hand side
    K [lx; ls; lz; ly] = [g_x + g_J (H o x + f); g_s; g_z; g_y]
(LU plus refinement with a longdouble residual, as there). The six gradient formulas of
``_backward_ref.qp_gradients`` are unchanged -- ls enters none -- and J's explicit dependence on the data
adds g_J 1/2 x^2 to grad_H and g_J x to grad_f. ``adjoint_reduced_full`` restates the reduced elimination
the kernels run in plain FP64 (no refinement): its distance to the dense solve is that elimination's floor.

One seed set per (N, env), from fixed generators: the kinds ``s``, ``z``, ``y``, ``objective`` (that
cotangent alone) and ``all`` (x, s, z, y and J together).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import _backward_cases as C
from tests import _backward_ref as br
from tests._util import rel_err_rows

KINDS = ["s", "z", "y", "objective", "all"]
FIELDS = ["x", "s", "z", "y", "objective"]  # a seed: dict field -> array (missing: zero)


def widths(N: int) -> dict:
    return {"x": 24 * N, "s": 16 * N, "z": 16 * N, "y": 14 * N, "objective": 1}


def full_rhs(N, Hv, f, x, seed: dict) -> np.ndarray:
    """[g_x + g_J (H o x + f); g_s; g_z; g_y] of one env."""
    w = widths(N)
    gx = np.zeros(w["x"]) if seed.get("x") is None else np.asarray(seed["x"], np.float64).copy()
    gJ = seed.get("objective")
    if gJ is not None:
        gx = gx + float(np.asarray(gJ).reshape(-1)[0]) * (np.asarray(Hv, np.float64) * x + np.asarray(f, np.float64))
    rest = [np.zeros(w[k]) if seed.get(k) is None else np.asarray(seed[k], np.float64) for k in ("s", "z", "y")]
    return np.concatenate([gx] + rest)


def adjoint_dense_full(N, Hv, Gv, Av, f, x, s, z, seeds: list) -> list:
    """Per seed (lx, ls, lz, ly): the refined dense solve with the full right-hand side, one factorisation."""
    H, G, A = br.dense_qp(N, Hv, Gv, Av)
    K = br.dense_kkt(N, H, G, A, np.asarray(s, np.float64), np.asarray(z, np.float64))
    rhs = np.stack([full_rhs(N, Hv, f, x, sd) for sd in seeds], axis=1)
    sol = br.solve_refined(K, rhs, matvec=br.kkt_matvec_ld(N, Hv, Gv, Av, s, z))
    return [br.split(N, sol[:, k]) for k in range(len(seeds))]


def adjoint_reduced_full(N, Hv, Gv, Av, f, x, s, z, seed: dict):
    """The reduced elimination in plain FP64 (no refinement): v = D^-1 (g_s - W g_z),
    [[Phi, A^T], [A, -dI]] [lx; ly] = [g~ - G^T v; g_y], lz = v + Lam G lx, ls = g_z - G lx + d lz."""
    H, G, A = br.dense_qp(N, Hv, Gv, Av)
    nz, m, p = 24 * N, 16 * N, 14 * N
    r = full_rhs(N, Hv, f, x, seed)
    gt, gs, gz, gy = r[:nz], r[nz:nz + m], r[nz + m:nz + 2 * m], r[nz + 2 * m:]
    W = np.asarray(z, np.float64) / np.asarray(s, np.float64) + br.DELTA
    D = 1.0 + br.DELTA * W
    lam = W / D
    v = (gs - W * gz) / D
    Phi = H + br.BETA * np.eye(nz) + G.T @ (lam[:, None] * G)
    M = np.block([[Phi, A.T], [A, -br.DELTA * np.eye(p)]])
    sol = np.linalg.solve(M, np.concatenate([gt - G.T @ v, gy]))
    lx, ly = sol[:nz], sol[nz:]
    glx = G @ lx
    lz = v + lam * glx
    return lx, gz - glx + br.DELTA * lz, lz, ly


def qp_gradients_full(N, lam, x, z, y, seed: dict) -> list:
    """[grad_H, grad_f, grad_A, grad_b, grad_G, grad_d]: the adjoint's six, plus the objective's direct terms."""
    g = br.qp_gradients(N, lam, x, z, y)
    gJ = seed.get("objective")
    if gJ is not None:
        gJ = float(np.asarray(gJ).reshape(-1)[0])
        g[0] = g[0] + gJ * (0.5 * x * x)
        g[1] = g[1] + gJ * x
    return g


def pdipm_backward_full(N, solver_inputs, seeds: list, reduced: bool = False) -> list:
    """Reference of srbd_pdipm_backward_seeds for one env: solver_inputs = the ten 1-D arrays of srbd_pdipm,
    seeds = a list of seed dicts. Returns one gradient list per seed."""
    Hv, Gv, Av, f = solver_inputs[:4]
    x, s, z, y = (np.asarray(v, np.float64) for v in solver_inputs[6:10])
    if reduced:
        lams = [adjoint_reduced_full(N, Hv, Gv, Av, f, x, s, z, sd) for sd in seeds]
    else:
        lams = adjoint_dense_full(N, Hv, Gv, Av, f, x, s, z, seeds)
    return [qp_gradients_full(N, lam, x, z, y, sd) for lam, sd in zip(lams, seeds)]


# ------------------------------------------------------------------ the cases' seeds and references ----

@functools.lru_cache(maxsize=None)
def seed_arrays(N: int) -> dict:
    """field -> (BATCH, width) float64 (objective: (BATCH,)), from a fixed generator per horizon."""
    rng = np.random.default_rng(2900 + N)
    w = widths(N)
    out = {k: rng.standard_normal((C.BATCH, w[k])) for k in ("x", "s", "z", "y")}
    out["objective"] = rng.standard_normal(C.BATCH)
    return out


def seed_set(N: int, kind: str) -> dict:
    """The batch's seed of one kind: field -> array, only the fields the kind gives."""
    a = seed_arrays(N)
    return dict(a) if kind == "all" else {kind: a[kind]}


def env_seed(N: int, kind: str, e: int) -> dict:
    return {k: v[e] for k, v in seed_set(N, kind).items()}


@functools.lru_cache(maxsize=None)
def reference(N: int, gait: str, K: int) -> dict:
    """kind -> the six reference gradients (BATCH, width) of the dense refined adjoint."""
    _, qp = C.workload(N, gait)
    it = C.iterate(N, gait, K)
    rows = [pdipm_backward_full(N, [a[e] for a in qp] + [v[e] for v in it], [env_seed(N, k, e) for k in KINDS])
            for e in range(C.BATCH)]
    return {k: [np.stack([rows[e][i][o] for e in range(C.BATCH)]) for o in range(6)] for i, k in enumerate(KINDS)}


@functools.lru_cache(maxsize=None)
def reduced_floor(N: int, gait: str, K: int) -> dict:
    """kind -> (6, BATCH): the per-env, per-output norm-wise distance between the plain-FP64 reduced
    elimination and the refined dense adjoint."""
    _, qp = C.workload(N, gait)
    it = C.iterate(N, gait, K)
    ref = reference(N, gait, K)
    out = {}
    for k in KINDS:
        red = [pdipm_backward_full(N, [a[e] for a in qp] + [v[e] for v in it], [env_seed(N, k, e)], reduced=True)[0]
               for e in range(C.BATCH)]
        out[k] = np.stack([rel_err_rows(np.stack([r[o] for r in red]), ref[k][o]) for o in range(6)])
    return out
