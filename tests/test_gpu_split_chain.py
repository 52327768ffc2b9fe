"""Kernel-level parity of the register kernels' column-split block chains (RegCtx::factor_chain,
solve_chain) against the oracle: the fused step and the plain solver at N = 2 (nb = 0: group 1
never active), 3 (nb = nf), 10 (the bench horizon) and 11 (the first two-wave horizon), B = 3, K = 1, 5.

Tolerances are those of tests/test_gpu_parity.py for the same cases, imported: SOLVER_CASES per K (and
U0_TOL) on the workloads of test_solver_matches_oracle (N = 10), test_runtime_horizon_solver_matches_oracle
(N = 2, 3: SOLVER_CASES or 4x the recorded floor between the two CPU restatements where that is higher)
and test_every_register_horizon_solver_matches_oracle (N = 11; K = 5 has no case there: SOLVER_CASES'
K = 5 entry on the same inputs) -- the first three envs of each; the fused step as
test_mpc_solve_end_to_end.
"""
import os

import numpy as np
import pytest
import torch

from biped_pympc_amd import solver
from biped_pympc_amd.utils.synthetic import make_workload, solver_init
from oracle import oracle
from tests._util import rel_err_rows, sweep_solver_inputs
from tests.test_gpu_parity import GOLDEN, SOLVER_CASES, U0_TOL

pytestmark = pytest.mark.gpu
B = 3
HORIZONS = [2, 3, 10, 11]
KS = [1, 5]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def _cuda(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _solver_inputs(N, K):
    if N == 11:
        return [np.asarray(a)[:B] for a in sweep_solver_inputs(N)]
    wl = make_workload(64, N, seed=100 + K, random_gait=(K % 2 == 0)) if N == 10 else \
        make_workload(48, N, seed=500 + N, random_gait=True)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    x, s, z, y = solver_init(d, N)
    return [np.asarray(a)[:B] for a in (H, G, A, f, d, b, x, s, z, y)]


def _tol(N, K, v):
    tol = dict(SOLVER_CASES)[K]
    if N in (2, 3):
        fl = np.asarray(np.load(os.path.join(GOLDEN, "dense_floor_runtime.npz"))[f"N{N}_K{K}_{v}"])
        tol = np.maximum(tol, 4.0 * (fl[:B] if fl.ndim else fl))
    return tol


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", HORIZONS)
def test_plain_solver_matches_oracle(N, K):
    ins = _solver_inputs(N, K)
    ref = oracle.pdipm(N, K, ins)
    out = solver.pdipm(_cuda(ins[:6]), _cuda(ins[6:]), N, K)
    torch.cuda.synchronize()
    for k, v in enumerate("xszy"):
        o = out[k].cpu().numpy()
        assert np.all(np.isfinite(o)), (N, K, v)
        err = rel_err_rows(o, ref[k])
        print(f"N={N} K={K} {v}: worst rel err {err.max():.3e}")
        assert np.all(err <= _tol(N, K, v)), (N, K, v, err.max())
    u0 = rel_err_rows(out[0].cpu().numpy()[:, 12 * N:12 * N + 12], ref[0][:, 12 * N:12 * N + 12])
    assert u0.max() <= U0_TOL
    assert np.all(np.isfinite(out[5].cpu().numpy()))  # no fallback sentinel left behind


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", HORIZONS)
def test_fused_step_matches_oracle_and_plain(N, K):
    wl = make_workload(B, N, seed=3 + N)
    ref = oracle.mpc_solve(N, K, wl.inputs, y0=1.0)
    ins = _cuda(wl.inputs)
    fused = [t.clone() for t in solver.mpc_solve(ins, N, K, y0=1.0, fused=True)]
    plain = solver.mpc_solve(ins, N, K, y0=1.0, fused=False)
    torch.cuda.synchronize()
    for a, c in zip(fused, plain):
        assert torch.equal(a, c)
    x = fused[0].cpu().numpy()
    err = rel_err_rows(x, ref[0])
    print(f"N={N} K={K} fused x: worst rel err {err.max():.3e}")
    assert np.all(np.isfinite(x))
    assert err.max() <= dict(SOLVER_CASES)[K]
    assert rel_err_rows(x[:, 12 * N:12 * N + 12], ref[0][:, 12 * N:12 * N + 12]).max() <= U0_TOL
