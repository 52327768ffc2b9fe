"""Shared helpers for the parity tests (compare against the oracle; never used by the product)."""
import numpy as np


def rel_err(a, b) -> float:
    """max |a - b| / max(max |b|, 1e-300) over the whole array (norm-wise relative error)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    return float(np.abs(a - b).max()) / scale if b.size else 0.0


def rel_err_rows(a, b) -> np.ndarray:
    """Per-env norm-wise relative error (rows of a batched (B, n) array)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = np.maximum(np.abs(b).max(axis=1), 1e-300)
    return np.abs(a - b).max(axis=1) / scale


# The horizon sweep of tests/test_gpu_parity.py test_every_register_horizon_solver_matches_oracle: the
# register horizons no other solver parity test runs on "auto", its batch, its (K, tolerance) pairs (the
# K = 1 and K = 5 tolerances of SOLVER_CASES) and its seed. tests/test_sweep_floor.py holds the seed rule
# on the CPU.
SWEEP_HORIZONS = [N for N in range(2, 33) if N not in (2, 3, 5, 10, 15, 16, 20, 25, 32)]
SWEEP_BATCH = 16
SWEEP_CASES = [(1, 1e-10), (3, 1e-9)]


def sweep_seed(N: int) -> int:
    return 700 + N


def sweep_solver_inputs(N: int):
    """The 10 batched solver inputs of the sweep at horizon N (randomized-gait workload, cold iterate)."""
    from biped_pympc_amd.utils.synthetic import make_workload, solver_init
    from oracle import oracle
    wl = make_workload(SWEEP_BATCH, N, seed=sweep_seed(N), random_gait=True)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    x, s, z, y = solver_init(d, N)
    return [H, G, A, f, d, b, x, s, z, y]


def dense_floor_env(N: int, K: int, ins, e: int):
    """FP64 floor of one env's solve: per-output (x, s, z, y) relative distance between the two CPU
    restatements of the solver -- the C oracle (sparse LDL^T) and oracle/pdipm_dense.py (dense LU) --
    on the solver inputs `ins` (10 batched arrays) of env e. A GPU result within a few times this is at
    the precision the problem admits (used where a fixed tolerance meets an ill-conditioned env)."""
    from oracle import oracle
    from oracle.pdipm_dense import pdipm_dense
    one = [np.asarray(a)[e:e + 1] for a in ins]
    ref = oracle.pdipm(N, K, one)
    den = pdipm_dense(N, K, *[a[0] for a in one])
    return [float(rel_err_rows(np.asarray(den[k])[None], ref[k]).max()) for k in range(4)]
