"""The QP objective J = 0.5 x^T H x + f^T x from every solver kernel family (include/srbd_mpc.h
srbd_solve_info; the reference's MPC cost, mpc_controller_qpth.py:136, mpc_wrapper.py:151-153).

The tolerance is derived, not measured: a kernel that forms each of the 24N terms with at most 4
roundings and adds them in any order has |J - J_exact| <= gamma_{24N+4} S (tests/_objective_ref.py).
J_exact and S are always computed, exactly, from the x the SAME GPU call returned and the H and f it
used, so solver parity does not enter. J is pre-filled with NaN: an env the kernel did not write fails.
"""
import functools

import numpy as np
import pytest
import torch

from biped_pympc_amd import _native, solver
from biped_pympc_amd.utils.synthetic import make_controller, make_workload
from oracle import oracle
from tests import _objective_ref as R

pytestmark = pytest.mark.gpu

PATHS = ["auto", "lds", "general"]


def _cuda(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _nan(B, dtype=torch.float64):
    return torch.full((B,), float("nan"), dtype=dtype, device="cuda")


def _np(t):
    return t.cpu().numpy()


def _assert_within_bound(J, H, f, x, tag):
    ratios = R.bound_ratios(_np(J), _np(H), _np(f), _np(x))
    print(f"{tag}: |J - J_exact| / (gamma S): max {ratios.max():.3e} over {ratios.size} envs")
    assert np.all(ratios <= 1.0), (tag, np.flatnonzero(~(ratios <= 1.0)), ratios.max())


# ---- 1. every kernel family, every wave count ------------------------------------------------

# the LDS step kernel (1), the smallest register horizon (2), the first and last horizons of the one-
# (.., 10), two- (11, ..), three- (22, ..) and four-wave (25, 32) register layouts
@pytest.mark.parametrize("N", [1, 2, 10, 11, 22, 25, 32])
@pytest.mark.parametrize("path", PATHS)
def test_mpc_solve_objective_within_bound(N, path):
    B, K = 48, 5
    wl = make_workload(B, N, seed=600 + N, random_gait=True)
    ins = _cuda(wl.inputs)
    J = _nan(B)
    with _native.solver_path(path):
        qp = solver.qp_former(ins, N)  # H (and f) as the kernels form them
        bufs = solver.MPCSolveBuffers.allocate(N, B)
        out = solver.mpc_solve(ins, N, K, 1.0, buffers=bufs, keep_qp=True, objective=J)
        f_used = bufs.qp_views()[1]  # the f this very call wrote
    torch.cuda.synchronize()
    assert torch.equal(f_used, qp[1])
    _assert_within_bound(J, qp[0], f_used, out[0], f"mpc_solve N={N} {path}")


# ---- 2. the plain solver entries -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _solver_case(N):
    B = 32
    wl = make_workload(B, N, seed=650 + N, random_gait=True)
    H, f, A, b, G, d = oracle.qp_former(N, wl.inputs)
    warm = oracle.mpc_solve(N, 3, wl.inputs, y0=1.0)[:4]  # the oracle's K = 3 iterate
    return [H, G, A, f, d, b], warm


# N = 20: the CCS register kernel reads f of its slots t > 0 from memory, not from registers
@pytest.mark.parametrize("N", [1, 5, 20])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("entry", ["warm", "cold", "ccs"])
def test_solver_entries_objective_within_bound(N, path, entry):
    K = 4
    qp_np, warm = _solver_case(N)
    qp = _cuda(qp_np)
    B = qp_np[0].shape[0]
    J = _nan(B)
    with _native.solver_path(path):
        if entry == "warm":
            out = solver.pdipm(qp, _cuda(warm), N, K, objective=J)
        elif entry == "cold":
            out = solver.pdipm(qp, None, N, K, 1.0, objective=J)
        else:
            out = solver.pdipm_ccs(qp, _cuda([0.5 * warm[0]])[0], N, K, objective=J)
    torch.cuda.synchronize()
    _assert_within_bound(J, qp[0], qp[3], out[0], f"{entry} N={N} {path}")


# ---- 3. QPs that are not stage-invariant -----------------------------------------------------

def _mixed_batch(N, B):
    """Two thirds of the envs not stage-invariant, as tests/test_gpu_parity.py's mixed batch: one
    stage's -A_d entry perturbed in every third QP, one stage's G entry in the next; here those envs
    also get one stage of H scaled (x and u blocks), so their J needs every stage's own H."""
    wl = make_workload(B, N, seed=77)
    H, f, A, b, G, d = (a.copy() for a in oracle.qp_former(N, wl.inputs))
    A[::3, 36 * min(N - 1, 4) + 7] *= 1.0 + 1e-3
    G[1::3, 28 * min(N - 1, 5) + 6] *= 0.9
    planted = np.zeros(B, bool)
    planted[::3] = True
    planted[1::3] = True
    sH = min(N - 1, 2)
    H[planted, 12 * sH:12 * sH + 12] *= 1.5
    H[planted, 12 * N + 12 * sH:12 * N + 12 * sH + 12] *= 2.0
    x = np.zeros((B, 24 * N))
    s = np.maximum(d, 1.0)
    z = np.ones((B, 16 * N))
    y = np.ones((B, 14 * N))
    return [H, G, A, f, d, b, x, s, z, y], planted


@pytest.mark.parametrize("N,path", [(5, "auto"), (10, "auto"), (20, "auto"), (5, "lds")])
def test_non_invariant_qps_objective_uses_every_stage(N, path):
    B, K = 96, 3
    ins, planted = _mixed_batch(N, B)
    J = _nan(B)
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    dev = _cuda(ins)
    with _native.solver_path(path):
        out = solver.pdipm(dev[:6], dev[6:], N, K, status=st, objective=J)
    torch.cuda.synchronize()
    assert np.array_equal((_np(st) & _native.STATUS_FALLBACK) != 0, planted)
    _assert_within_bound(J, dev[0], dev[3], out[0], f"mixed N={N} {path}")
    # the planted envs tell a kernel that takes stage 0's H for every stage: that J is out of bound
    H0 = ins[0].copy()
    H0[:, :12 * N] = np.tile(H0[:, :12], N)
    H0[:, 12 * N:] = np.tile(H0[:, 12 * N:12 * N + 12], N)
    x = _np(out[0])
    J0 = np.einsum("be,be->b", 0.5 * H0 * x + ins[3], x)
    assert np.all(R.bound_ratios(J0[planted], ins[0][planted], ins[3][planted], x[planted]) > 1.0)


# ---- 4. asking changes nothing ---------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 10, 20])
@pytest.mark.parametrize("path", PATHS)
def test_asking_for_the_objective_changes_no_output_bit(N, path):
    B, K = 48, 5
    ins = _cuda(make_workload(B, N, seed=700 + N, random_gait=True).inputs)
    J1, J2 = _nan(B), _nan(B)
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    with _native.solver_path(path):
        a = solver.mpc_solve(ins, N, K, 1.0, buffers=solver.MPCSolveBuffers.allocate(N, B))
        b = solver.mpc_solve(ins, N, K, 1.0, buffers=solver.MPCSolveBuffers.allocate(N, B), objective=J1)
        c = solver.mpc_solve(ins, N, K, 1.0, buffers=solver.MPCSolveBuffers.allocate(N, B), status=st,
                             objective=J2)
    torch.cuda.synchronize()
    for k in range(6):
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], c[k]), k
    assert torch.equal(J1, J2) and bool(torch.isfinite(J1).all())
    assert bool((st >= 0).all())  # the status word was written alongside


# ---- 5. fused = unfused ----------------------------------------------------------------------

@pytest.mark.parametrize("N", [3, 10, 21])
def test_fused_objective_equals_former_then_solver_bit_for_bit(N):
    """One RegCtx method serves the fused and the CCS register kernel: the same terms in the same
    order, so J agrees the way x already does (N = 21: the CCS kernel addresses f from its kernel
    argument; N = 10 holds f's first slot in registers and re-reads none)."""
    B, K = 48, 5
    ins = _cuda(make_workload(B, N, seed=720 + N, random_gait=True).inputs)
    J1, J2 = _nan(B), _nan(B)
    with _native.solver_path("auto"):
        a = solver.mpc_solve(ins, N, K, 1.0, buffers=solver.MPCSolveBuffers.allocate(N, B), fused=True,
                             objective=J1)
        H, f, A, b, G, d = solver.qp_former(ins, N)
        c = solver.pdipm([H, G, A, f, d, b], None, N, K, 1.0, objective=J2)
    torch.cuda.synchronize()
    assert torch.equal(a[0], c[0])
    assert torch.equal(J1, J2)


# ---- 6. controller ---------------------------------------------------------------------------

def _cost_controller(B, N, compute_cost, seed=5):
    c = make_controller(B, N, seed=seed, device="cuda", n_iter=10)
    c.cfg.compute_cost = compute_cost
    c.cfg.keep_solution = True
    return c


@pytest.mark.parametrize("N", [1, 10])
def test_controller_cost_is_the_objective_of_its_solution(N):
    B, ndof = 32, 5
    c1, c2, c3, c4 = (_cost_controller(B, N, on) for on in (True, True, False, True))
    w1, cost1 = c1.run()
    w2, cost2 = c2.run_three_kernel()
    w3, cost3 = c3.run()
    rng = np.random.default_rng(3)
    jac = torch.from_numpy(rng.normal(size=(B, 2, 6, ndof)).astype(np.float32))
    cb = torch.from_numpy((rng.uniform(size=(B, 2)) < 0.7).astype(np.float32))
    w4, cost4, tau = c4.run_with_torque(jac, cb)
    J = _nan(B)
    sol = solver.mpc_solve(c1.former_inputs, N, 10, c1.cfg.y0, objective=J)
    torch.cuda.synchronize()
    assert cost1.dtype == torch.float32 and cost1.shape == (B,) and cost1 is c1.cost
    assert bool(torch.isfinite(cost1).all()) and bool((cost1 != 0).any())
    assert torch.equal(sol[0], c1.solution[0])
    assert torch.equal(cost1, J.float())  # J rounded once to float32
    assert torch.equal(cost1, cost2) and torch.equal(w1, w2)
    assert torch.equal(cost3, torch.zeros_like(cost3)) and torch.equal(w3, w1)
    assert torch.equal(cost4, cost1) and torch.equal(w4, w1) and bool(torch.isfinite(tau).all())
    # and J itself is within the bound of the solution the step kept
    qp = solver.qp_former(c1.former_inputs, N)
    _assert_within_bound(J, qp[0], qp[1], c1.solution[0], f"controller N={N}")


# ---- 7. graph --------------------------------------------------------------------------------

def test_graphed_step_fills_cost_and_bakes_compute_cost_in():
    from biped_pympc_amd.controller import GraphedMPCStep
    B, N = 32, 10
    c1, c2 = _cost_controller(B, N, True), _cost_controller(B, N, True)
    c1.cfg.keep_solution = c2.cfg.keep_solution = False
    g = GraphedMPCStep(c2)
    c2.cost.fill_(float("nan"))  # (the warm-up launch wrote it)
    storage = c2.cost.data_ptr()
    for step in range(2):
        w1, cost1 = c1.run()
        w2, cost2 = g()
        torch.cuda.synchronize()
        assert cost2.data_ptr() == storage
        assert torch.equal(w1, w2) and torch.equal(cost1, cost2), step
        assert bool(torch.isfinite(cost2).all())
        for c in (c1, c2):
            c.state_estimate_data.root_position.add_(0.01)
    c2.cfg.compute_cost = False
    with pytest.raises(RuntimeError, match="compute_cost"):
        g()


# ---- 8. validation ---------------------------------------------------------------------------

def test_objective_argument_is_validated_before_any_launch():
    N, B, K = 5, 8, 2
    wl = make_workload(B, N, seed=1)
    ins = _cuda(wl.inputs)
    H, f, A, b, G, d = solver.qp_former(ins, N)
    qp = [H, G, A, f, d, b]
    x0 = torch.zeros((B, 24 * N), dtype=torch.float64, device="cuda")
    bad = {
        "float32": torch.zeros(B, dtype=torch.float32, device="cuda"),
        "length": torch.zeros(B + 1, dtype=torch.float64, device="cuda"),
        "cpu": torch.zeros(B, dtype=torch.float64),
        "strided": torch.zeros(2 * B, dtype=torch.float64, device="cuda")[::2],
        "shape": torch.zeros((B, 1), dtype=torch.float64, device="cuda"),
    }
    sentinel = 7.0
    for name, t in bad.items():
        for call in (lambda o: solver.pdipm(qp, None, N, K, 1.0, outputs=outs, objective=o),
                     lambda o: solver.pdipm_ccs(qp, x0, N, K, outputs=outs, objective=o),
                     lambda o: solver.mpc_solve(ins, N, K, 1.0, buffers=bufs, objective=o)):
            bufs = solver.MPCSolveBuffers.allocate(N, B)
            outs = bufs.outputs
            for o in outs:
                o.fill_(sentinel)
            with pytest.raises((ValueError, TypeError)):
                call(t)
            torch.cuda.synchronize()
            assert all(bool((o == sentinel).all()) for o in outs), name  # nothing was launched
