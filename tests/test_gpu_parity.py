"""GPU parity: HIP kernels (through the C-ABI) vs the CPU oracle on identical seeded inputs.

Mirrors the reference's only parity harness, ``biped_pympc/cusadi/run_cusadi_function_test.py``
(batched device evaluation vs per-env CPU evaluation, error per output), with the oracle in place
of CasADi (absent here; see oracle/srbd_oracle.c). Tolerances are norm-wise relative errors
(max |gpu - oracle| / max |oracle| per output); the bar from BASELINE.json is 1e-4 on the QP
solution, the former is checked at 1e-12.
"""
import os

import numpy as np
import pytest
import torch

from biped_pympc_amd import layout, solver
from biped_pympc_amd.utils.synthetic import make_workload, solver_init
from oracle import oracle
from tests._util import (SWEEP_CASES, SWEEP_HORIZONS, dense_floor_env, rel_err, rel_err_rows,
                         sweep_solver_inputs)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (run them through gpurun)")


def _cuda(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


@pytest.mark.parametrize("N,random_gait", [(10, False), (10, True), (20, False), (1, False), (32, True)])
def test_former_matches_oracle(N, random_gait):
    wl = make_workload(256, N, seed=11 + N, random_gait=random_gait, residuals=random_gait)
    ref = oracle.qp_former(N, wl.inputs)
    out = solver.qp_former(_cuda(wl.inputs), N)
    torch.cuda.synchronize()
    for k, (o, r) in enumerate(zip(out, ref)):
        err = rel_err(o.cpu().numpy(), r)
        assert err <= 1e-12, f"output {k} rel err {err:.3e}"


# (K, tolerance on x/s/z/y, worst env of 64; norm-wise relative per env). The GPU solves the same
# Newton systems by a different exact elimination (twisted block-tridiagonal dual Schur complement
# with explicit 12x12 inverses, plus one step of iterative refinement on the full KKT per iteration)
# than the oracle's sparse LDL^T. Two exact FP64 eliminations of the same KKT do not agree better
# than the IPM's own sensitivity allows: the oracle vs the independent dense-LU restatement
# (oracle/pdipm_dense.py) differ by up to 1.4e-12 (K = 1), 7e-12 (K = 5), 1.2e-8 (K = 10) and
# 4.2e-7 (K = 20) on these workloads (N = 20, seed 100, worst of 64 envs;
# profiles/r02/refinement_parity.txt). The GPU sits at that floor: worst 2.9e-12 / 8.1e-11 /
# 2.8e-8 / 9.4e-7. The K = 10 and 20 tolerances are set a few times above the measured floor;
# BASELINE's bar is 1e-4.
SOLVER_CASES = [(1, 1e-10), (5, 1e-9), (10, 1e-7), (20, 1e-5)]
# first-stage input u0 at K = 10 (what the controller applies), relative to max |u0| of the env:
# worst measured 1.3e-7 (N = 20, 509 randomized-gait envs, test_ragged_batches)
U0_TOL = 1e-6


@pytest.mark.parametrize("N", [10, 20])
@pytest.mark.parametrize("K,tol", SOLVER_CASES)
def test_solver_matches_oracle(N, K, tol):
    B = 64
    wl = make_workload(B, N, seed=100 + K, random_gait=(K % 2 == 0))
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    x, s, z, y = solver_init(d, N)
    ins = [H, G, A, f, d, b, x, s, z, y]
    ref = oracle.pdipm(N, K, ins)
    out = solver.pdipm(_cuda(ins[:6]), _cuda(ins[6:]), N, K)
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in out]
    names = ["x", "s", "z", "y", "residuals", "mu"]
    for k in range(4):
        errs = rel_err_rows(out[k], ref[k])
        assert np.all(np.isfinite(out[k])), names[k]
        assert errs.max() <= tol, f"{names[k]}: worst env rel err {errs.max():.3e} (median {np.median(errs):.1e})"
    u0_err = rel_err_rows(out[0][:, 12 * N:12 * N + 12], ref[0][:, 12 * N:12 * N + 12])
    assert u0_err.max() <= U0_TOL


@pytest.mark.parametrize("path", ["auto", "lds", "general"])
@pytest.mark.parametrize("K", [1, 5, 10, 20])
@pytest.mark.parametrize("N", [1, 2, 3, 5, 15, 16, 25, 32])
def test_runtime_horizon_solver_matches_oracle(N, K, path):
    """Horizons other than 10 and 20 under every solver path: "auto" runs the register kernel at
    the horizons it is instantiated for (2..32: N = 2, 3, 5 one wave per QP, 15, 16 two, 25, 32 three;
    regN.hpp) and the runtime-N LDS-resident kernel (pdipm_srbd_kernel<0>) at N = 1; "lds" always the latter,
    including the degenerate twisted recursions of N = 1, 2; "general" the CCS-table kernel. Per env
    at the SOLVER_CASES tolerance, or 4x the FP64 floor between the two CPU restatements where that
    is higher (tests/golden/make_runtime_floor.py: one N = 3 env's z differs by 1e-4 between them at
    K = 20)."""
    from biped_pympc_amd import _native
    B = 48
    wl = make_workload(B, N, seed=500 + N, random_gait=True)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    x, s, z, y = solver_init(d, N)
    ins = [H, G, A, f, d, b, x, s, z, y]
    ref = oracle.pdipm(N, K, ins)
    with _native.solver_path(path):
        out = solver.pdipm(_cuda(ins[:6]), _cuda(ins[6:]), N, K)
        torch.cuda.synchronize()
    floor = np.load(os.path.join(GOLDEN, "dense_floor_runtime.npz"))
    for k, v in enumerate("xszy"):
        o = out[k].cpu().numpy()
        assert np.all(np.isfinite(o))
        tol = np.maximum(dict(SOLVER_CASES)[K], 4.0 * floor[f"N{N}_K{K}_{v}"])
        err = rel_err_rows(o, ref[k])
        assert np.all(err <= tol), (N, K, v, err.max())
    assert np.all(np.isfinite(out[5].cpu().numpy()))  # no fallback sentinel left behind


# the register horizons that neither test_solver_matches_oracle (10, 20) nor
# test_runtime_horizon_solver_matches_oracle (2, 3, 5, 15, 16, 25, 32) runs on "auto" (tests/_util.py)
assert SWEEP_CASES == [(1, dict(SOLVER_CASES)[1]), (3, dict(SOLVER_CASES)[5])]


@pytest.mark.parametrize("K,tol", SWEEP_CASES)
@pytest.mark.parametrize("N", SWEEP_HORIZONS)
def test_every_register_horizon_solver_matches_oracle(N, K, tol):
    """The register kernels are 31 separately scheduled template instances (N = 2..32); this runs the
    22 the two tests above leave out, on "auto" (the register kernel), B = 16 randomized-gait envs, per
    env against oracle.pdipm at the K = 1 tolerance of SOLVER_CASES for K = 1 and its K = 5 tolerance for
    K = 3. Seed rule: seed = 700 + N + 100 j for the first j >= 0 at which every env's floor between the two
    CPU restatements (tests/_util.py dense_floor_env: the oracle vs oracle/pdipm_dense.py) is at most a
    quarter of the tolerance at both K -- so the tolerance is never the floor's. The rule is held on the
    CPU by tests/test_sweep_floor.py on these very inputs (tests/_util.py sweep_solver_inputs): j = 0 at
    all 22 horizons; worst floors 1.4e-11 (K = 1, N = 30) and 1.6e-10 (K = 3, N = 31)."""
    ins = sweep_solver_inputs(N)
    ref = oracle.pdipm(N, K, ins)
    out = solver.pdipm(_cuda(ins[:6]), _cuda(ins[6:]), N, K)
    torch.cuda.synchronize()
    for k, v in enumerate("xszy"):
        o = out[k].cpu().numpy()
        assert np.all(np.isfinite(o)), (N, K, v)
        err = rel_err_rows(o, ref[k])
        assert np.all(err <= tol), (N, K, v, err.max())
    assert np.all(np.isfinite(out[5].cpu().numpy()))  # no fallback sentinel left behind


@pytest.mark.parametrize("path", ["auto", "lds", "general"])
@pytest.mark.parametrize("K", [5, 20])
@pytest.mark.parametrize("N", [1, 10, 20, 32])
def test_cpu_path_dual_init_y0_zero(N, K, path):
    """The reference CPU path's iterate init -- x = 0, s = max(d, 1), z = 1 and y = 0
    (mpc_controller_casadi.py:182-199 via initialize_pdipm_variables, sparse_pdipm_solver.py:537-558;
    the GPU caller uses y = 1, mpc_controller_cusadi.py:141) -- on the HIP path:
    the cold-started solver (srbd_pdipm_cold, y0 = 0) and the fused former + solve
    (srbd_mpc_solve_fused, y0 = 0) vs the oracle started the same way, every env, under every solver
    path, at K = 5 (BASELINE config 1) and K = 20 (the CPU path's MAX_ITER, mpc_controller_casadi.py:31).
    Per env: the SOLVER_CASES tolerance, or 4x that env's FP64 floor between the two CPU
    restatements where that is higher (tests/golden/make_y0_floor.py: at N = 1, K = 20 one env's z
    differs by 5.8e-4 between them)."""
    from biped_pympc_amd import _native
    B = 48
    wl = make_workload(B, N, seed=300 + N, random_gait=True, residuals=True)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    ins = [H, G, A, f, d, b, *solver_init(d, N, y0=0.0)]
    assert not ins[9].any()
    ref = oracle.pdipm(N, K, ins)
    ref_fused = oracle.mpc_solve(N, K, wl.inputs, y0=0.0)
    with _native.solver_path(path):
        cold = [t.clone() for t in solver.pdipm(_cuda(ins[:6]), None, N, K, y0=0.0)]
        fused = solver.mpc_solve(_cuda(wl.inputs), N, K, y0=0.0)
        torch.cuda.synchronize()
    floor = np.load(os.path.join(GOLDEN, "dense_floor_y0.npz"))
    tol = dict(SOLVER_CASES)[K]
    for out, r in ((cold, ref), (fused, ref_fused)):
        for k, v in enumerate("xszy"):
            o = out[k].cpu().numpy()
            assert np.all(np.isfinite(o))
            err = rel_err_rows(o, r[k])
            assert np.all(err <= np.maximum(tol, 4.0 * floor[f"N{N}_K{K}_{v}"])), (v, err.max())
    # y = 0 really reached the kernels: the y = 1 start gives a different iterate
    other = solver.pdipm(_cuda(ins[:6]), None, N, K, y0=1.0)
    torch.cuda.synchronize()
    assert not torch.equal(other[3], cold[3])


def test_cold_start_matches_explicit_init():
    N, B, K = 10, 128, 10
    wl = make_workload(B, N, seed=7)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    x, s, z, y = solver_init(d, N, y0=1.0)
    qp = _cuda([H, G, A, f, d, b])
    warm = solver.pdipm(qp, _cuda([x, s, z, y]), N, K)
    cold = solver.pdipm(qp, None, N, K, y0=1.0)
    torch.cuda.synchronize()
    for a, c in zip(warm, cold):
        assert torch.equal(a, c)


def test_mpc_solve_end_to_end():
    """Fused stream (former -> cold PDIPM, K = 10) vs the oracle's full GPU-caller step."""
    N, B, K = 10, 256, 10
    wl = make_workload(B, N, seed=3)
    ref = oracle.mpc_solve(N, K, wl.inputs, y0=1.0)
    out = solver.mpc_solve(_cuda(wl.inputs), N, K, y0=1.0)
    torch.cuda.synchronize()
    x = out[0].cpu().numpy()
    u_gpu, u_ref = x[:, 12 * N:12 * N + 12], ref[0][:, 12 * N:12 * N + 12]
    # the K = 10 tolerances of the solver tests (SOLVER_CASES, U0_TOL)
    assert rel_err_rows(u_gpu, u_ref).max() <= U0_TOL
    assert rel_err_rows(x, ref[0]).max() <= dict(SOLVER_CASES)[K]


@pytest.mark.parametrize("N,random_gait", [(10, False), (10, True), (20, True), (5, True), (1, True), (3, False),
                                           (16, True), (9, False), (32, True), (11, True), (15, True),
                                           (21, False), (25, True)])
def test_fused_step_equals_former_plus_solver(N, random_gait):
    """srbd_mpc_solve_fused builds the stage blocks in the solver from the former inputs with the
    former's own device code, so it reproduces former + solver bit for bit (the register kernels at
    every N in 2..32 -- 3, 5, 9, 10, 11, 15, 16, 20, 21, 25, 32 here; the LDS-resident one-launch
    step kernel, mpc_step_lds.hpp, at N = 1)."""
    B, K = 200, 10
    wl = make_workload(B, N, seed=900 + N, random_gait=random_gait, residuals=random_gait)
    ins = _cuda(wl.inputs)
    fused = [t.clone() for t in solver.mpc_solve(ins, N, K, fused=True)]
    plain = solver.mpc_solve(ins, N, K, fused=False)
    torch.cuda.synchronize()
    for a, c in zip(fused, plain):
        assert torch.equal(a, c)


FUSED_LISTED = (10, 20, 5, 1, 3, 16, 9, 32, 11, 15, 21, 25)  # test_fused_step_equals_former_plus_solver


@pytest.mark.parametrize("N", [N for N in range(1, 33) if N not in FUSED_LISTED])
def test_fused_step_equals_former_plus_solver_every_other_horizon(N):
    """The same bit-for-bit check at the 20 horizons the test above does not list (each register
    horizon has its own fused and CCS kernel instance), small: B = 8, K = 2; randomized gait and
    residual outputs at the even horizons, the standing gait at the odd ones."""
    B, K = 8, 2
    rg = N % 2 == 0
    wl = make_workload(B, N, seed=900 + N, random_gait=rg, residuals=rg)
    ins = _cuda(wl.inputs)
    fused = [t.clone() for t in solver.mpc_solve(ins, N, K, fused=True)]
    plain = solver.mpc_solve(ins, N, K, fused=False)
    torch.cuda.synchronize()
    for a, c in zip(fused, plain):
        assert torch.equal(a, c)


def test_iteration_schedule_composes():
    """4 calls x 5 iterations (the reference GPU schedule, mpc_controller_cusadi.py:144-169) equal
    one call x 20 iterations: the solver keeps no hidden state."""
    N, B = 10, 64
    wl = make_workload(B, N, seed=5)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    qp = _cuda([H, G, A, f, d, b])
    it = _cuda(list(solver_init(d, N)))
    one = solver.pdipm(qp, it, N, 20)
    cur = it
    for _ in range(4):
        o = solver.pdipm(qp, cur, N, 5)
        cur = [t.clone() for t in o[:4]]
    torch.cuda.synchronize()
    for a, c in zip(one[:4], cur):
        assert torch.equal(a, c)


@pytest.mark.parametrize("N,K", [(10, 10), (20, 10), (10, 20)])
def test_fast_and_general_kernels_agree(N, K):
    """The stage-invariant fast kernel and the general kernel solve the same systems."""
    from biped_pympc_amd import _native
    B = 128
    wl = make_workload(B, N, seed=31 + K, random_gait=True)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    qp = _cuda([H, G, A, f, d, b])
    it = _cuda(list(solver_init(d, N)))
    fast = solver.pdipm(qp, it, N, K)
    with _native.solver_path("general"):
        gen = solver.pdipm(qp, it, N, K)
    torch.cuda.synchronize()
    tol = dict(SOLVER_CASES)[K]
    for k in range(4):
        e = rel_err_rows(fast[k].cpu().numpy(), gen[k].cpu().numpy())
        assert e.max() <= tol, (k, e.max())


@pytest.mark.parametrize("path", ["general", "lds"])
@pytest.mark.parametrize("N", [10, 20])
def test_mpc_solve_under_a_solver_path(N, path):
    """mpc_solve (fused by default) inside a non-auto solver path runs former + that solver kernel:
    it needs and gets the QP workspace, and agrees with the fused step at the K = 10 tolerance."""
    from biped_pympc_amd import _native
    K, B = 10, 64
    wl = make_workload(B, N, seed=60 + N, random_gait=True)
    ins = _cuda(wl.inputs)
    fused = [t.clone() for t in solver.mpc_solve(ins, N, K)]
    with _native.solver_path(path):
        assert _native.current_solver_path() == _native.SOLVER_PATHS[path]
        other = solver.mpc_solve(ins, N, K)
        torch.cuda.synchronize()
    assert _native.current_solver_path() == 0
    for k in range(4):
        e = rel_err_rows(other[k].cpu().numpy(), fused[k].cpu().numpy())
        assert e.max() <= dict(SOLVER_CASES)[K], (k, e.max())


# (N, solver path, B, K): B = 600 QPs of which 400 are not stage-invariant take the in-launch
# fallback's scratch pool (pdipm.hpp pdipm_general_scratch: by default one slot per resident workgroup,
# 2048 on an MI355X, so these do not contend -- test_mixed_batch_with_a_capped_pool makes them);
# N = 20 / 25 / 32 run multi-wave register QPs whose waves share the slot through LDS; "lds" runs the
# LDS-resident kernel (pdipm_srbd_kernel) and its fallback
MIXED_CASES = [(10, "auto", 96, 10), (1, "auto", 600, 5), (5, "auto", 600, 5), (10, "auto", 600, 5),
               (20, "auto", 600, 5), (25, "auto", 600, 5), (32, "auto", 600, 5), (5, "lds", 600, 5),
               (20, "lds", 600, 5)]


@pytest.mark.parametrize("N,path,B,K", MIXED_CASES)
def test_mixed_batch_routes_non_invariant_qps_to_the_general_kernel(N, path, B, K):
    _mixed_batch_check(N, path, B, K)


@pytest.mark.parametrize("N,path,B,K", [(10, "auto", 600, 5), (20, "auto", 600, 5), (32, "auto", 600, 5),
                                        (5, "lds", 600, 5)])
def test_mixed_batch_with_a_capped_pool(N, path, B, K):
    """srbd_set_scratch_slots(3): 400 fallback QPs queue on 3 slots -- the slot search (s_sleep, wrap
    at n) and the lock hand-over between workgroups that reuse a slot -- with the same results."""
    from biped_pympc_amd import _native
    _native.set_scratch_slots(3)
    try:
        _mixed_batch_check(N, path, B, K)
        assert _native.scratch_pool()["slots"] == 3
    finally:
        _native.set_scratch_slots(0)


def test_capped_pool_shared_by_two_streams():
    """Two mixed batches in flight at once on two streams over one 3-slot pool: both match the
    oracle (no slot is handed to two workgroups; the lock words serialise them)."""
    from biped_pympc_amd import _native
    _native.set_scratch_slots(3)
    try:
        cases = [_mixed_inputs(10, 600, seed) for seed in (91, 92)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = []
        torch.cuda.synchronize()
        for (ins, _), st in zip(cases, streams):
            with torch.cuda.stream(st):
                outs.append(solver.pdipm(_cuda(ins[:6]), _cuda(ins[6:]), 10, 5))
        torch.cuda.synchronize()
        for (ins, _), out in zip(cases, outs):
            ref = oracle.pdipm(10, 5, ins)
            for k in range(4):
                e = rel_err_rows(out[k].cpu().numpy(), ref[k])
                assert e.max() <= 1e-7, (k, e.max())
        pool = _native.scratch_pool()
        assert pool["slots"] == 3 and pool["bytes"] > 0
        _native.release_device()
        assert _native.scratch_pool() == {"slots": 0, "bytes": 0}
    finally:
        _native.set_scratch_slots(0)
    _native.prepare_device()  # the default pool again, before any capture test
    assert _native.scratch_pool()["slots"] >= 256


def test_pool_resized_and_released_while_another_thread_solves():
    """One host thread solves mixed batches (fallback QPs use the scratch pool) while another resizes
    and releases the pool: a launch holds the pool from attach to enqueue (srbd_mpc.hip g_pool_rw), so
    no kernel runs on a freed pool and every solve matches the oracle."""
    import threading
    from biped_pympc_amd import _native
    ins, _ = _mixed_inputs(10, 600, 93)
    ref = oracle.pdipm(10, 5, ins)
    dev_in = (_cuda(ins[:6]), _cuda(ins[6:]))
    outs, errors = [], []
    torch.cuda.synchronize()

    def solve():
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(24):
                    outs.append([t.clone() for t in solver.pdipm(*dev_in, 10, 5)[:4]])
            st.synchronize()
        except Exception as ex:  # noqa: BLE001 -- reported below
            errors.append(ex)

    def churn():
        try:
            for k in range(24):
                _native.set_scratch_slots(3 if k % 2 == 0 else 0)
                if k % 3 == 2:
                    _native.release_device()
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    try:
        th = [threading.Thread(target=solve), threading.Thread(target=churn)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=90)
        assert not any(t.is_alive() for t in th) and not errors, errors
        torch.cuda.synchronize()
        assert len(outs) == 24
        for out in outs:
            for k in range(4):
                e = rel_err_rows(out[k].cpu().numpy(), ref[k])
                assert e.max() <= 1e-7, (k, e.max())
    finally:
        _native.set_scratch_slots(0)
    _native.prepare_device()
    assert _native.scratch_pool()["slots"] >= 256


def _mixed_inputs(N, B, seed=77):
    wl = make_workload(B, N, seed=seed)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    A = A.copy()
    G = G.copy()
    sA = min(N - 1, 4)
    if N >= 2:
        A[::3, 36 * sA + 7] *= 1.0 + 1e-3   # perturb one stage's -A_d entry in every third QP
    else:
        A[::3, layout.Dims(N).nnz_A - 1] *= 1.0 + 1e-3  # (N = 1: an x-moment entry of u_0)
    G[1::3, 28 * min(N - 1, 5) + 6] *= 0.9  # and one stage's G entry in others
    x, s, z, y = solver_init(d, N)
    return [H, G, A, f, d, b, x, s, z, y], wl


def _mixed_batch_check(N, path, B, K):
    from biped_pympc_amd import _native
    ins, _ = _mixed_inputs(N, B)
    ref = oracle.pdipm(N, K, ins)
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    with _native.solver_path(path):
        out = solver.pdipm(_cuda(ins[:6]), _cuda(ins[6:]), N, K, status=st)
    torch.cuda.synchronize()
    tol = dict(SOLVER_CASES)[K]
    floors = {}
    for k in range(4):
        e = rel_err_rows(out[k].cpu().numpy(), ref[k])
        assert np.all(np.isfinite(out[k].cpu().numpy()))
        # a perturbed QP can be far worse conditioned than the SRBD QPs SOLVER_CASES was set on (one
        # N = 20 env: 8.9e-9 in z at K = 5): an env above tol must sit within 4x its own FP64 floor
        # between the two CPU restatements (sparse LDL^T oracle vs dense LU)
        for env in np.flatnonzero(e > tol):
            if env not in floors:
                floors[env] = dense_floor_env(N, K, ins, env)
            assert e[env] <= 4.0 * floors[env][k], (k, env, e[env], floors[env][k])
    assert np.all(np.isfinite(out[5].cpu().numpy()))  # no fallback sentinel left behind
    # status: bit 2 exactly on the QPs that are not stage-invariant (N = 1 has a single stage, so
    # every QP is stage-invariant and the perturbed ones are solved by the fast kernel)
    flagged = np.zeros(B, bool)
    if N >= 2:
        flagged[::3] = True
        flagged[1::3] = True
    got = st.cpu().numpy()
    assert np.array_equal((got & _native.STATUS_FALLBACK) != 0, flagged)
    assert np.all((got & ~_native.STATUS_FALLBACK) == 0), np.unique(got)


@pytest.mark.parametrize("fn_kind", ["qp_former", "pdipm"])
def test_cusadi_dropin_random_inputs(fn_kind):
    """run_cusadi_function_test.py's harness: random (B, nnz_in) FP64 inputs through the drop-in
    CusadiFunction (ctypes -> lib<name>.so evaluate) vs per-env CPU evaluation (the oracle)."""
    from biped_pympc_amd.cusadi import CusadiFunction, pdipm_function, qp_former_function
    N, B = 10, 256
    fn = qp_former_function(N) if fn_kind == "qp_former" else pdipm_function(N, 5)
    g = torch.Generator().manual_seed(0)
    inputs = [torch.rand((B, fn.nnz_in(i)), generator=g, dtype=torch.float64) for i in range(fn.n_in())]
    if fn_kind == "qp_former":
        # keep the 3x3 inertia invertible and the mass/dt positive, as any physical input is
        inputs[8] = (torch.eye(3, dtype=torch.float64).reshape(1, 9) * 0.5 + 0.1 * inputs[8])
    else:
        inputs[7] += 0.1  # slacks and duals strictly positive (interior point)
        inputs[8] += 0.1
    cf = CusadiFunction(fn, B)
    cf.evaluate([t.cuda().contiguous() for t in inputs])
    torch.cuda.synchronize()
    assert cf.eval_time > 0
    np_in = [t.numpy() for t in inputs]
    ref = oracle.qp_former(N, np_in) if fn_kind == "qp_former" else oracle.pdipm(N, 5, np_in)
    for k in range(fn.n_out()):
        err = rel_err_rows(cf.outputs_sparse[k].cpu().numpy(), ref[k])
        # uniformly random QP data (no stage structure, uncontrolled conditioning; the general
        # kernel): worst z 2.8e-9 of 256 envs at K = 5 measured, vs 7e-12 on SRBD QPs
        assert err.max() <= (1e-12 if fn_kind == "qp_former" else 1e-8), (k, err.max())
    dense = cf.getDenseOutput(2 if fn_kind == "qp_former" else 0).cpu().numpy()
    if fn_kind == "qp_former":
        assert np.allclose(dense, layout.to_dense(ref[2], *layout.ccs_A(N), (14 * N, 24 * N)), atol=1e-12)


def test_cusadi_outputs_dense_allocated_only_when_read():
    """CusadiFunction.outputs_dense holds no device memory until an entry is read; a read entry is
    the reference's zeroed (B, size1, size2) tensor (CusadiFunction.py:77-81, never written there)
    and stays the same tensor; evaluate / getDenseOutput allocate none of them."""
    from biped_pympc_amd.cusadi import CusadiFunction, qp_former_function
    N, B = 10, 512
    fn = qp_former_function(N)
    dense_bytes = sum(B * fn.size1_out(i) * fn.size2_out(i) * 8 for i in range(fn.n_out()))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    cf = CusadiFunction(fn, B)
    wl = make_workload(B, N, seed=12)
    cf.evaluate(_cuda(wl.inputs))
    cf.getDenseOutput(2)
    torch.cuda.synchronize()
    assert cf.outputs_dense.allocated == []
    assert torch.cuda.memory_allocated() - before < dense_bytes / 4
    h = cf.outputs_dense[0]
    assert h.shape == (B, fn.size1_out(0), fn.size2_out(0)) and h.dtype == torch.float64
    assert not h.any() and cf.outputs_dense[0] is h and cf.outputs_dense.allocated == [0]
    assert len(cf.outputs_dense) == fn.n_out() and len(list(cf.outputs_dense)) == fn.n_out()


def test_api_rejects_bad_buffers():
    """Wrong widths, dtypes or host tensors are refused before any launch (the C-ABI trusts sizes)."""
    N, B = 10, 8
    wl = make_workload(B, N, seed=2)
    ins = _cuda(wl.inputs)
    d = layout.Dims(N)
    bad_out = [torch.empty((B, w + 1), dtype=torch.float64, device="cuda") for w in d.former_out_nnz]
    with pytest.raises(ValueError):
        solver.qp_former(ins, N, outputs=bad_out)
    with pytest.raises(TypeError):
        solver.qp_former([t.cpu() for t in ins], N)
    with pytest.raises(TypeError):
        solver.qp_former([t.float() for t in ins], N)
    H, f, A, b, G, dd = solver.qp_former(ins, N)
    qp = [H, G, A, f, dd, b]
    with pytest.raises(ValueError):
        solver.pdipm(qp, None, N, 1, outputs=[torch.empty((B, 3), dtype=torch.float64, device="cuda")] * 6)
    bufs = solver.MPCSolveBuffers.allocate(N, B, "cuda")
    bufs.outputs[0] = torch.empty((B, 5), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        solver.mpc_solve(ins, N, 1, buffers=bufs)


@pytest.mark.parametrize("N", [10, 20])
@pytest.mark.parametrize("B", [1, 3, 13, 509])
def test_ragged_batches(N, B):
    """Batch sizes that fill neither a former workgroup (4 envs) nor the 8 XCDs evenly: the
    XCD-contiguous env map (srbd_common.hpp xcd_item) and the grid tails must cover every env once."""
    K = 10
    wl = make_workload(B, N, seed=4000 + B, random_gait=True, residuals=True)
    ins = _cuda(wl.inputs)
    ref = oracle.mpc_solve(N, K, wl.inputs, y0=1.0)
    fused = [t.clone() for t in solver.mpc_solve(ins, N, K, y0=1.0, fused=True)]
    plain = solver.mpc_solve(ins, N, K, y0=1.0, fused=False)
    torch.cuda.synchronize()
    for a, c in zip(fused, plain):
        assert torch.equal(a, c)
    x = fused[0].cpu().numpy()
    assert np.all(np.isfinite(x))
    u_gpu, u_ref = x[:, 12 * N:12 * N + 12], ref[0][:, 12 * N:12 * N + 12]
    assert rel_err_rows(u_gpu, u_ref).max() <= U0_TOL
    # per env: the K = 10 tolerance, or 4x the spread between the two CPU restatements (sparse
    # LDL^T oracle vs dense LU, tests/golden/make_dense_floor.py) where that FP64 floor is higher
    # (one env of the N = 20, 509-env workload sits at 1.1e-7 between them)
    floor = np.load(os.path.join(GOLDEN, "dense_floor_ragged.npz"))[f"N{N}_B{B}"]
    err = rel_err_rows(x, ref[0])
    assert np.all(err <= np.maximum(dict(SOLVER_CASES)[K], 4.0 * floor)), (err.max(), floor[err.argmax()])


@pytest.mark.parametrize("N,B,random_gait", [(10, 4096, False), (20, 4096, False), (10, 8192, False),
                                              (10, 4096, True)])
def test_full_size_properties(N, B, random_gait):
    """BASELINE configs 2-5 at their full per-GPU sizes, through size-independent properties:
    a QP's solution does not depend on its batch position or the batch size (a permuted batch and
    a sub-batch reproduce the same rows bit for bit), every iterate is finite and strictly
    interior, the barrier parameter fell below its cold-start value in every env (s0 = max(d, 1),
    z0 = 1, so mu0 >= 1), and a strided sample of 64 envs matches the oracle at the K = 10
    tolerances."""
    K = 10
    wl = make_workload(B, N, seed=7000 + B + N, random_gait=random_gait, residuals=random_gait)
    ins = _cuda(wl.inputs)
    full = [t.clone() for t in solver.mpc_solve(ins, N, K, y0=1.0)]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B + N)).cuda()
    permuted = [t.clone() for t in solver.mpc_solve([t[perm].contiguous() for t in ins], N, K, y0=1.0)]
    head = solver.mpc_solve([t[:B // 8].contiguous() for t in ins], N, K, y0=1.0)
    torch.cuda.synchronize()
    for a, p, h in zip(full, permuted, head):
        assert torch.equal(a[perm], p)
        assert torch.equal(a[:B // 8], h)
    x, s, z, y, res, mu = [t.cpu().numpy() for t in full]
    for v in (x, s, z, y, res, mu):
        assert np.all(np.isfinite(v))
    assert s.min() > 0.0 and z.min() > 0.0
    assert mu.max() < 1.0, f"barrier parameter did not fall in every env: max mu {mu.max():.3e}"
    idx = np.arange(0, B, B // 64)
    ref = oracle.mpc_solve(N, K, [np.ascontiguousarray(a[idx]) for a in wl.inputs], y0=1.0)
    u_gpu, u_ref = x[idx, 12 * N:12 * N + 12], ref[0][:, 12 * N:12 * N + 12]
    assert rel_err_rows(u_gpu, u_ref).max() <= U0_TOL
    assert rel_err_rows(x[idx], ref[0]).max() <= dict(SOLVER_CASES)[K]


@pytest.mark.parametrize("fused,reps", [(True, 2197), (False, 440)])
def test_batches_past_32_bit_element_offsets(fused, reps):
    """Maximum sizes: a batch whose arrays hold more than 2^31 elements, so every env row past that
    point is reached only through 64-bit offsets (the kernels form them as (size_t)env * width). The
    fused step at 2197 x 4096 = 8,998,912 envs (x: 240 per env, 2.16e9 elements, 51 GB of solution);
    former + CCS solver at 440 x 4096 = 1,802,240 envs (A: 1196 per env, 2.16e9 elements in the
    workspace). A 4096-env workload is tiled on the device and every env of the big batch must
    reproduce its 4096-env solve bit for bit (a QP's solution does not depend on its batch position),
    the 4096-env solve matches the oracle on a strided sample. Sized for one MI355X (288 GB HBM):
    ~66 GB (fused) / ~52 GB (CCS)."""
    N, K, B0 = 10, 10, 4096
    d = layout.Dims(N)
    width = d.nz if fused else d.nnz_A
    assert reps * B0 * width > 2**31  # the test's premise
    free, _ = torch.cuda.mem_get_info()
    need = reps * B0 * 8 * (sum(d.former_in_nnz) + sum(d.solver_out_nnz)
                            + (0 if fused else sum(d.former_out_nnz)))
    if need > 0.8 * free:
        pytest.skip(f"needs {need / 2**30:.0f} GiB of device memory, {free / 2**30:.0f} GiB free")
    wl = make_workload(B0, N, seed=9100 + int(fused), random_gait=True, residuals=True)
    small_in = _cuda(wl.inputs)
    small = [t.clone() for t in solver.mpc_solve(small_in, N, K, y0=1.0, fused=fused)]
    idx = np.arange(0, B0, B0 // 16)
    ref = oracle.mpc_solve(N, K, [np.ascontiguousarray(a[idx]) for a in wl.inputs], y0=1.0)
    assert rel_err_rows(small[0][idx].cpu().numpy(), ref[0]).max() <= dict(SOLVER_CASES)[K]
    big_in = [t.repeat(reps, 1) for t in small_in]
    del small_in
    big = solver.mpc_solve(big_in, N, K, y0=1.0, fused=fused)
    torch.cuda.synchronize()
    del big_in
    for b, s_ in zip(big, small):
        assert b.shape[0] == reps * B0
        assert bool((b.view(reps, B0, -1) == s_.view(1, B0, -1)).all()), "env rows differ from the 4096-env solve"
    del big
    torch.cuda.empty_cache()


def _tol_for(K):  # SOLVER_CASES extended to every K (scripts/parity_fuzz.py)
    return 1e-10 if K <= 1 else 1e-9 if K <= 5 else 1e-7 if K <= 10 else 1e-5


@pytest.mark.parametrize("mode", ["adaptive", "every_iteration"])
def test_fuzz_regressions(mode):
    """Envs the randomised parity campaign (scripts/parity_fuzz.py) found off the reference's trajectory
    on the register kernels (tests/golden/fuzz_regressions.npz, make_fuzz_regressions.py). Group
    "adaptive": ill-conditioned iterates (W = z / s of 4.5e3 .. 1.2e8, some with every s above the 1e-8
    clamp) that drifted 1e2 .. 1e6 x the FP64 floor before the predictor was refined there; the default
    mode must hold them within 4x their floor. Group "strict": envs 5 .. 400 x the floor in the adaptive
    mode, at the floor when every iteration refines its predictor (srbd_set_refinement(1)). Group "stiff"
    (strict mode, on the solver path each env failed on): z 1e3 .. 4e5 x the floor at clamped rows until
    the foot blocks were applied through LDL^T solves. Group "unchecked" (both modes): the round-5 _ccs
    campaign's ok cases whose above-tolerance envs it never floor-checked (seed 56036: 6.3e-3 in u0 on the
    LDS-resident kernel), floor-checked since (scripts/parity_floor.py). The floor: the larger distance of the
    AMD-ordered LDL^T and dense LU from the checker. Per output
    x, s, z, y: max(the K tolerance, 4 x floor); u0: max(U0_TOL, 4 x its floor)."""
    from biped_pympc_amd import _native
    z = np.load(os.path.join(GOLDEN, "fuzz_regressions.npz"))
    groups = ("adaptive", "unchecked") if mode == "adaptive" else ("adaptive", "strict", "stiff", "unchecked")
    keys = sorted({k.split("_")[0] for k in z.files if k.startswith(groups)})
    assert len(keys) == (16 if mode == "adaptive" else 29)
    paths = {v: k for k, v in _native.SOLVER_PATHS.items()}
    for key in keys:
        N, K, seed, env, path = (int(v) for v in z[f"{key}_NK"])
        ins = [z[f"{key}_in{j}"][None] for j in range(10)]
        with _native.refinement(mode), _native.solver_path(paths[path]):
            out = solver.pdipm(_cuda(ins[:6]), _cuda(ins[6:]), N, K)
            torch.cuda.synchronize()
        floor = z[f"{key}_floor"]
        for j in range(4):
            e = rel_err_rows(out[j].cpu().numpy(), z[f"{key}_ref{j}"][None])[0]
            assert e <= max(_tol_for(K), 4.0 * floor[j]), (key, seed, env, j, e, floor[j])
        u = slice(12 * N, 12 * N + 12)
        eu = rel_err_rows(out[0].cpu().numpy()[:, u], z[f"{key}_ref0"][None, u])[0]
        assert eu <= max(U0_TOL, 4.0 * floor[4]), (key, seed, env, "u0", eu, floor[4])
    assert _native.current_refinement() == 0


def test_refinement_mode_is_per_call_and_exact():
    """Both refinement modes on the benchmark workload agree within the K = 10 tolerance, the mode
    reaches the fused step and the CCS solver (every_iteration changes bits), and the default restores."""
    from biped_pympc_amd import _native
    N, K, B = 10, 10, 300
    wl = make_workload(B, N, seed=4242)
    ins = _cuda(wl.inputs)
    a = [t.clone() for t in solver.mpc_solve(ins, N, K)]
    with _native.refinement("every_iteration"):
        assert _native.current_refinement() == 1
        b = [t.clone() for t in solver.mpc_solve(ins, N, K)]
    c = solver.mpc_solve(ins, N, K)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    assert not torch.equal(a[2], b[2])
    ref = oracle.mpc_solve(N, K, wl.inputs)
    for k in range(4):
        assert rel_err_rows(a[k].cpu().numpy(), ref[k]).max() <= dict(SOLVER_CASES)[K]
        assert rel_err_rows(b[k].cpu().numpy(), ref[k]).max() <= dict(SOLVER_CASES)[K]
    with pytest.raises(RuntimeError):
        _native.check(_native.lib().srbd_set_refinement(2), "srbd_set_refinement")


@pytest.mark.parametrize("N", [10, 20, 5])
def test_refinement_policy_words(N):
    """srbd_set_refinement_policy: the word of mode 0 (the predictor at the initial iterate, all z = 1, + the
    W >= 1e4 vote) and of mode 1 (every iteration) reproduce the modes bit for bit on the fused step and the
    CCS solver; round 5's mode 0 (the W vote alone) differs from today's and stays within the tolerance, and
    so does a position-based word (the first iteration of every call); unknown bits and a NaN threshold are
    refused; leaving the context returns to mode 0."""
    from biped_pympc_amd import _native
    K, B = 10, 128
    wl = make_workload(B, N, seed=4343, random_gait=True)
    ins = _cuda(wl.inputs)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    qp = _cuda([H, G, A, f, d, b])

    def both():
        fused = [t.clone() for t in solver.mpc_solve(ins, N, K)[:4]]
        ccs = [t.clone() for t in solver.pdipm(qp, None, N, K)[:4]]
        torch.cuda.synchronize()
        return fused + ccs
    mode0 = both()
    with _native.refinement("every_iteration"):
        mode1 = both()
    with _native.refinement_policy(_native.REFINE_AFFINE_AT_INIT, 1e4):
        assert _native.current_refinement() == 2
        p0 = both()
    with _native.refinement_policy(_native.refine_affine_first(1), 1e3):
        f1 = both()
    with _native.refinement_policy(_native.REFINE_AFFINE_ALL, 1e3):
        p1 = both()
    with _native.refinement_policy(0, 1e3):
        r5 = both()
    assert _native.current_refinement() == 0
    assert all(torch.equal(x, y) for x, y in zip(mode0, p0))
    assert all(torch.equal(x, y) for x, y in zip(mode1, p1))
    assert not all(torch.equal(x, y) for x, y in zip(mode0, r5))
    ref = oracle.mpc_solve(N, K, wl.inputs)
    for k in range(4):
        assert rel_err_rows(r5[k].cpu().numpy(), ref[k]).max() <= dict(SOLVER_CASES)[K]
        assert rel_err_rows(f1[k].cpu().numpy(), ref[k]).max() <= dict(SOLVER_CASES)[K]
    L = _native.lib()
    assert L.srbd_set_refinement_policy(1 << 24, 1e3) != 0 and "unknown policy bits" in _native.last_error()
    assert L.srbd_set_refinement_policy(0, float("nan")) != 0
    assert _native.current_refinement() == 0


def test_empty_batch_is_a_no_op():
    N = 10
    wl = make_workload(1, N, seed=1)
    empty = [torch.from_numpy(np.ascontiguousarray(a[:0])).cuda() for a in wl.inputs]
    out = solver.mpc_solve(empty, N, 10)
    former = solver.qp_former(empty, N)
    torch.cuda.synchronize()
    assert all(t.shape[0] == 0 for t in out) and all(t.shape[0] == 0 for t in former)


@pytest.mark.parametrize("N", [10, 20])
def test_golden_fixtures_on_the_hip_path(N):
    """The committed fixtures (tests/golden/srbd_oracle_N{N}.npz: the reference's two demo points
    srbd_constraints.py:244-282 and generate_solver_function.py:19-58, two standing and two
    randomized-gait robots, with the oracle's outputs stored at generation time) through the HIP
    path: the former bit-level, the cold-started solver and the fused step at every stored K."""
    import os
    g = np.load(os.path.join(GOLDEN, f"srbd_oracle_N{N}.npz"))
    inputs = [g[f"in{k}"] for k in range(17)]
    former = solver.qp_former(_cuda(inputs), N)
    torch.cuda.synchronize()
    for name, o in zip("H f A b G d".split(), former):
        assert rel_err(o.cpu().numpy(), g[name]) <= 1e-12, name
    qp = _cuda([g["H"], g["G"], g["A"], g["f"], g["d"], g["b"]])
    # K{K}_*: the GPU caller's init y0 = 1; Y0_K{K}_*: the reference CPU path's y0 = 0
    for y0, prefix in ((1.0, ""), (0.0, "Y0_")):
        for K, tol in SOLVER_CASES:
            cold = [t.clone() for t in solver.pdipm(qp, None, N, K, y0=y0)]
            fused = solver.mpc_solve(_cuda(inputs), N, K, y0=y0)
            torch.cuda.synchronize()
            for k, name in enumerate(["x", "s", "z", "y"]):
                ref = g[f"{prefix}K{K}_{name}"]
                for out in (cold, fused):
                    e = rel_err_rows(out[k].cpu().numpy(), ref)
                    assert e.max() <= tol, (y0, K, name, e.max())
            np.testing.assert_allclose(fused[5].cpu().numpy(), g[f"{prefix}K{K}_mu"], rtol=1e-6)


@pytest.mark.parametrize("N", [10, 20, 5])
@pytest.mark.parametrize("K,tol", [(1, 1e-10), (10, 1e-7)])
def test_ccs_entry_from_arbitrary_x_init(N, K, tol):
    """srbd_pdipm_ccs: the reference's _ccs solver init (sparse_pdipm_solver.py:30-35 and
    initialize_pdipm_variables :537-558, restated in numpy here exactly as the reference writes
    it: s = max(h - G x_init, 1), z = 1, y = 0) followed by K iterations, vs the oracle."""
    B = 48
    wl = make_workload(B, N, seed=700 + N + K, random_gait=True)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    dims = layout.Dims(N)
    x0 = np.random.default_rng(N + K).normal(0, 5.0, (B, dims.nz))
    Gd = layout.to_dense(G, *layout.ccs_G(N), (dims.n_ineq, dims.nz))
    s0 = np.maximum(d - np.einsum("bij,bj->bi", Gd, x0), 1.0)
    it = [x0, s0, np.ones((B, dims.n_ineq)), np.zeros((B, dims.n_eq))]
    ref = oracle.pdipm(N, K, [H, G, A, f, d, b, *it])
    out = solver.pdipm_ccs(_cuda([H, G, A, f, d, b]), _cuda([x0])[0], N, K)
    torch.cuda.synchronize()
    # y starts at 0 here, and after one iteration it is the first dual step of the delta-regularised
    # equality rows: the two CPU restatements (sparse LDL^T oracle, dense LU) already disagree by up
    # to 1.2e-9 (N = 10) / 7.8e-9 (N = 5) on these envs (scripts/ccs_floor.py), so y gets 3e-8 at K = 1
    for k in range(4):
        e = rel_err_rows(out[k].cpu().numpy(), ref[k])
        assert e.max() <= (max(tol, 3e-8) if k == 3 else tol), (k, e.max())
    assert np.all(np.isfinite(out[5].cpu().numpy()))


@pytest.mark.parametrize("N", [10, 20])
def test_fused_step_qp_vectors_only_on_request(N):
    """srbd_mpc_solve_fused keeps f, b, d on chip by default; keep_qp writes them, equal to the
    former's own rows, and the solution is the same either way. The QP workspace the default path
    never writes is not allocated by it either (MPCSolveBuffers allocates it on first use)."""
    B = 37
    wl = make_workload(B, N, seed=800 + N, random_gait=True)
    ins = _cuda(wl.inputs)
    qp = solver.qp_former(ins, N)
    lean = solver.MPCSolveBuffers.allocate(N, B, "cuda")
    first = [t.clone() for t in solver.mpc_solve(ins, N, 10, buffers=lean)]
    assert not lean.workspace_allocated
    bufs = solver.MPCSolveBuffers.allocate(N, B, "cuda")
    bufs.workspace.fill_(3.0)
    a = [t.clone() for t in solver.mpc_solve(ins, N, 10, buffers=bufs)]
    torch.cuda.synchronize()
    assert bool((bufs.workspace == 3.0).all())
    c = solver.mpc_solve(ins, N, 10, buffers=bufs, keep_qp=True)
    torch.cuda.synchronize()
    for x, y, z in zip(a, c, first):
        assert torch.equal(x, y) and torch.equal(x, z)
    views = bufs.qp_views()
    for k in (1, 3, 5):  # f, b, d
        assert torch.equal(views[k], qp[k]), k


def test_solver_call_captured_in_a_hip_graph():
    """srbd_pdipm (stage-invariant kernel with its in-launch fallback) captured in a HIP graph after
    srbd_prepare_device(): the replay gives the eager call's bits (include/srbd_mpc.h: the pool must
    exist before a capture)."""
    from biped_pympc_amd import _native
    _native.prepare_device()
    N, K, B = 10, 5, 64
    wl = make_workload(B, N, seed=81)
    qp = _cuda(oracle.qp_former(N, wl.inputs))
    sol_qp = [qp[0], qp[4], qp[2], qp[1], qp[5], qp[3]]
    eager = [t.clone() for t in solver.pdipm(sol_qp, None, N, K)]
    out = solver._alloc_solver_outputs(B, N, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        solver.pdipm(sol_qp, None, N, K, outputs=out)  # warm-up on the capture's side stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        solver.pdipm(sol_qp, None, N, K, outputs=out)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in range(6):
        assert torch.equal(out[k], eager[k]), k


def test_library_bound_before_torch_still_finds_the_device():
    """A fresh process that binds libsrbd_mpc.so before anything imported torch -- what
    __graft_entry__.build() followed by smoke() in one process does -- still runs the kernels: _native.lib()
    maps torch's bundled HIP runtime first. Mapped the other way round, the process held two runtimes and
    every launch of the library failed with HIP error 100 (no device). This test is about the process's
    load order, hence the one child process."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; from biped_pympc_amd import _native; assert 'torch' not in sys.modules; "
            "assert _native.lib().srbd_abi_version() == 1; import __graft_entry__ as g; g.smoke()")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "smoke ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
