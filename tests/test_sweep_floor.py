"""The seed rule of the register-horizon sweep (tests/test_gpu_parity.py
test_every_register_horizon_solver_matches_oracle), held on the CPU.

The sweep compares the GPU with the oracle at the fixed K = 1 / K = 5 tolerances of SOLVER_CASES. That is
only a statement about the kernels while the problem itself admits the tolerance: for every env of every
horizon, the floor between the two CPU restatements (the C oracle's sparse LDL^T and the dense LU of
oracle/pdipm_dense.py; tests/_util.py dense_floor_env) must be at most a quarter of the tolerance at both
K. A change to the synthetic workload that breaks this fails here, on the CPU, instead of surfacing as a
GPU parity failure; the answer is another seed (sweep_seed), never a wider tolerance.
"""
import pytest

from tests._util import SWEEP_BATCH, SWEEP_CASES, SWEEP_HORIZONS, dense_floor_env, sweep_solver_inputs


@pytest.mark.slow
@pytest.mark.parametrize("N", SWEEP_HORIZONS)
def test_sweep_seed_keeps_the_floor_under_a_quarter_of_the_tolerance(N):
    ins = sweep_solver_inputs(N)
    for K, tol in SWEEP_CASES:
        worst = max(max(dense_floor_env(N, K, ins, e)) for e in range(SWEEP_BATCH))
        print(f"N={N} K={K}: worst floor {worst:.3e} (tolerance {tol:.0e})")
        assert worst <= tol / 4.0, (N, K, worst)
