"""GPU parity of the former, the fused step and the backward pass on generic inputs (tests/_generic.py): every
env has its own dt, mass, mu, Q and R, I_world is not symmetric, the linearisation point (x, u) is random and
mu != 1, so no product of former_f / former_d is exact -- and, for the former and its VJP alone, R_body is not
orthonormal and the contact table is fractional. tests/test_generic_inputs.py holds on the CPU that these
inputs expose a transposed inertia decode and a read of another env's scalar, and holds the seed rule and the
reference-only floors the tolerances below rest on.

Tolerances (none is taken from a kernel's output):
  former, former VJP   1e-12 per env and output, the former's parity bound (tests/test_gpu_parity.py)
  H, the -mu entries   bit for bit (they are copies of inputs)
  cancelling rows      |d| <= 8 u (|t1| + |t2|), |f_u| <= 2 u |R u|, u = 2^-53: each of gz and iq is a two-term
                       sum rounded at most three times (two products, one sum), so each is within 3 u of the
                       row's exact value (|t1| + |t2| bounds it) and their rounded difference within 8 u; r u - r u
                       is at most the two roundings of the product
  fused step           SWEEP_CASES (1e-10 at K = 1, 1e-9 at K = 3) per env; the floor between the two CPU
                       restatements is at most a quarter of it on every env (seed rule, j = 0 everywhere)
  objective            the bound of tests/_objective_ref.py
  adjoint              CASES of tests/_backward_cases.py (1e-10 at K = 1, 1e-9 at K = 5) per env and output;
                       the reduced-elimination floor stays within it on every env
  autograd             1e-9: the adjoint's K = 5 tolerance (the former VJP adds 1e-12), as the existing
                       autograd test
Worst measured errors are in the docstring of each test.
"""
import functools

import numpy as np
import pytest
import torch

from biped_pympc_amd import _native, layout, solver
from oracle import oracle
from tests import _backward_cases as C
from tests import _backward_ref as br
from tests import _generic as G
from tests import _objective_ref as OR
from tests._util import SWEEP_CASES, rel_err_rows

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
QP_NAMES = ["H", "f", "A", "b", "G", "d"]


def _cuda(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in arrs]


def _np(t):
    return t.cpu().numpy()


def _worst(err):
    return f"{err.max():.3e} (env {int(err.argmax())})"


# ---- a. the former against the oracle ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _former_case(N, B):
    P = G.generic_former_inputs(B, N, seed=2400 + N, solvable=False)
    return P, oracle.qp_former(N, P)


# N = 1: no x blocks; 2: the first coupling; 3: the 24N loops first wrap past 64 lanes; 6: the 12N loops first
# wrap; 32: the largest. B = 67: 17 workgroups of four envs, the last one partial
@pytest.mark.parametrize("N", [1, 2, 3, 6, 32])
def test_former_matches_oracle_on_generic_inputs(N):
    """Worst per-env error against the oracle over the six outputs (tolerance 1e-12; always b, the deepest
    expression): N = 1 1.4e-14 (env 10), N = 2 1.4e-14 (env 46), N = 3 2.7e-14 (env 2), N = 6 1.5e-14 (env 21),
    N = 32 4.5e-14 (env 44); f 4.9e-16, A 2.2e-16, d 3.1e-16 at most, H and G exact. Cancelling rows of d:
    exact zeros at every horizon (gz and iq come out as the same bits); u part of f: worst
    |f| / (2 u |R u|) 0.496 (r u - r u contracts to the rounding residue of the product, where the oracle has an
    exact zero)."""
    B = 67
    P, ref = _former_case(N, B)
    out = [_np(t) for t in solver.qp_former(_cuda(P), N)]
    torch.cuda.synchronize()
    for k, name in enumerate(QP_NAMES):
        err = rel_err_rows(out[k], ref[k])
        print(f"former N={N} {name}: worst per-env rel err {_worst(err)}, tol 1e-12")
        assert np.all(err <= 1e-12), (name, err.max(), int(err.argmax()))
    nx = 12 * N
    # H is Q / R themselves and the friction entries of G are -mu: copies, so bit for bit
    assert np.array_equal(out[0][:, :nx], np.tile(P[13], (1, N))), "H (Q part)"
    assert np.array_equal(out[0][:, nx:], np.tile(P[14], (1, N))), "H (R part)"
    is_mu = G.g_mu_entries(N)
    assert is_mu.sum() == 8 * N
    assert np.array_equal(out[4][:, is_mu], np.broadcast_to(-P[6], (B, 8 * N))), "G (-mu entries)"
    assert np.array_equal(out[4][:, ~is_mu], ref[4][:, ~is_mu]), "G (constant entries)"
    # what cancels in exact arithmetic stays at rounding level
    terms = G.d_row_terms(N, P)
    rows = G.d_cancelling_rows(N)
    ratio_d = np.abs(out[5][:, rows]) / (8.0 * U * terms[:, rows])
    ratio_f = np.abs(out[1][:, nx:]) / (2.0 * U * np.abs(np.tile(P[14], (1, N)) * P[2]))
    print(f"former N={N}: cancelling rows of d, worst |d| / bound {ratio_d.max():.3f}; "
          f"u part of f, worst |f| / bound {ratio_f.max():.3f}")
    assert np.all(ratio_d <= 1.0), (ratio_d.max(), np.unravel_index(ratio_d.argmax(), ratio_d.shape))
    assert np.all(ratio_f <= 1.0), (ratio_f.max(), np.unravel_index(ratio_f.argmax(), ratio_f.shape))


# ---- b. the fused step equals former + solver, bit for bit -------------------------------------------

def _assert_fused_equals_plain(N, B, K, seed):
    ins = _cuda(G.generic_former_inputs(B, N, seed=seed, solvable=True))
    fused = [t.clone() for t in solver.mpc_solve(ins, N, K, fused=True)]
    plain = solver.mpc_solve(ins, N, K, fused=False)
    torch.cuda.synchronize()
    for name, a, c in zip(["x", "s", "z", "y", "residuals", "mu"], fused, plain):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, c), (N, name, int((a != c).any(dim=1).sum()), (a - c).abs().max().item())


@pytest.mark.parametrize("N", range(1, 33))
def test_fused_step_equals_former_plus_solver_on_generic_inputs(N):
    """Every horizon has its own fused and CCS kernel instance (the LDS one-launch step, mpc_step_lds.hpp, at
    N = 1; the register kernels at 2..32), each of which inlines former_f / former_d / former_model: on inputs
    where these round, all six outputs still agree bit for bit with qp_former_kernel + the solver."""
    _assert_fused_equals_plain(N, B=8, K=2, seed=2500 + N)


@pytest.mark.parametrize("N", [10, 20])
def test_fused_step_equals_former_plus_solver_on_generic_inputs_ragged(N):
    """The deployed horizons at B = 67 (a partial last workgroup of every kernel) and K = 10."""
    _assert_fused_equals_plain(N, B=67, K=10, seed=2600 + N)


# ---- c. the fused step against the oracle -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _solver_ref(N, K):
    P, _ = G.solver_case_inputs(N)
    return oracle.mpc_solve(N, K, P, y0=1.0)


def _assert_solution(out, ref, tol, tag):
    for k, v in enumerate("xszy"):
        o = _np(out[k])
        assert np.all(np.isfinite(o)), (tag, v)
        err = rel_err_rows(o, ref[k])
        print(f"{tag} {v}: worst per-env rel err {_worst(err)}, tol {tol:.0e}")
        assert np.all(err <= tol), (tag, v, err.max(), int(err.argmax()))
    assert np.all(np.isfinite(_np(out[5])))  # no fallback sentinel left behind


@pytest.mark.parametrize("K,tol", SWEEP_CASES)
@pytest.mark.parametrize("N", G.SOLVER_HORIZONS)
def test_fused_step_matches_oracle_on_generic_inputs(N, K, tol):
    """srbd_mpc_solve_fused against oracle.mpc_solve, per env: the LDS step (N = 1), then 1, 1, 2, 2 and 3 waves
    per QP (3, 10, 16, 20, 32). Worst error over x, s, z, y (K = 1 / K = 3, tolerance 1e-10 / 1e-9): N = 1
    4.4e-12 (y, env 3) / 2.7e-12 (x, env 3), N = 3 1.5e-11 (x, env 12) / 3.2e-12 (x, env 12), N = 10 7.5e-12
    (y, env 4) / 1.1e-11 (x, env 0), N = 16 4.2e-12 (x, env 2) / 8.9e-12 (y, env 3), N = 20 2.9e-12 (x, env 5) /
    5.9e-12 (x, env 5), N = 32 1.6e-11 (x, env 4) / 5.0e-11 (x, env 15): at the floor between the two CPU
    restatements (tests/test_generic_inputs.py)."""
    P, _ = G.solver_case_inputs(N)
    out = solver.mpc_solve(_cuda(P), N, K, y0=1.0)
    torch.cuda.synchronize()
    _assert_solution(out, _solver_ref(N, K), tol, f"fused N={N} K={K}")


@pytest.mark.parametrize("K,tol", SWEEP_CASES)
@pytest.mark.parametrize("path", ["lds", "general"])
@pytest.mark.parametrize("N", [3, 10])
def test_two_kernel_step_matches_oracle_on_generic_inputs(N, path, K, tol):
    """qp_former_kernel + the LDS-resident / the general solver kernel on the same cases. Worst error (K = 1 /
    K = 3): lds N = 3 1.5e-11 / 3.1e-12 (x, env 12), N = 10 7.5e-12 (y, env 4) / 9.9e-12 (x, env 0); general
    N = 3 1.5e-11 / 3.0e-12 (x, env 12), N = 10 7.5e-12 (y, env 4) / 9.9e-12 (x, env 0)."""
    P, _ = G.solver_case_inputs(N)
    with _native.solver_path(path):
        out = solver.mpc_solve(_cuda(P), N, K, y0=1.0, fused=False)
        torch.cuda.synchronize()
    _assert_solution(out, _solver_ref(N, K), tol, f"{path} N={N} K={K}")


@pytest.mark.parametrize("N", [3, 10])
def test_fused_step_objective_within_bound_on_generic_inputs(N):
    """J of the fused step against the exact rational value at the returned x, with the H and f the kernels
    formed (f's u part is rounding residue here, not zero). Worst |J - J_exact| / (gamma S), 1 passes: N = 3
    1.1e-2 (env 1), N = 10 2.1e-3 (env 10)."""
    K = 3
    P, _ = G.solver_case_inputs(N)
    ins = _cuda(P)
    J = torch.full((G.SOLVER_BATCH,), float("nan"), dtype=torch.float64, device="cuda")
    qp = solver.qp_former(ins, N)
    bufs = solver.MPCSolveBuffers.allocate(N, G.SOLVER_BATCH)
    out = solver.mpc_solve(ins, N, K, 1.0, buffers=bufs, keep_qp=True, objective=J)
    torch.cuda.synchronize()
    f_used = bufs.qp_views()[1]
    assert torch.equal(f_used, qp[1])
    ratios = OR.bound_ratios(_np(J), _np(qp[0]), _np(f_used), _np(out[0]))
    print(f"objective N={N}: worst |J - J_exact| / (gamma S) {_worst(ratios)}")
    assert np.all(ratios <= 1.0), ratios


# ---- d. the former VJP kernel against the reference -------------------------------------------------

@pytest.mark.parametrize("N,B", [(1, 16), (2, 16), (3, 16), (6, 16), (32, 16), (3, 67)])
def test_former_vjp_kernel_matches_reference_on_generic_inputs(N, B):
    """srbd_qp_former_backward against br.former_vjp_batch (checked against central differences of the oracle
    at such points, tests/test_generic_inputs.py) with asymmetric inertia -- phase C's -I^-T g I^-T --, a
    non-orthonormal R_body and per-env scalars. Worst per-env error over the 15 inputs (tolerance 1e-12):
    (1, 16) 2.0e-15 (dt), (2, 16) 1.6e-13 (dt, env 13), (3, 16) 1.9e-15 (body_pos), (6, 16) 1.2e-14 (m),
    (32, 16) 2.0e-14 (mu), (3, 67) 7.5e-13 (m, env 33); I_world 9.3e-16 at most. The scalar inputs are one sum
    over every entry of a random cotangent, compared entry-wise: env 33's mass gradient cancels 11430-fold
    (sum |terms| / |sum|), so 7.5e-13 is a third of a unit roundoff per term."""
    P = G.generic_former_inputs(B, N, seed=2700 + N + B, solvable=False)
    rng = np.random.default_rng(2750 + N + B)
    cot = [rng.standard_normal((B, w)) for w in layout.Dims(N).former_out_nnz]
    ref = br.former_vjp_batch(N, P, cot)
    got = solver.qp_former_backward(_cuda(P), _cuda(cot), N)
    torch.cuda.synchronize()
    for i, name in enumerate(layout.FORMER_IN_NAMES):
        if i in (1, 2):
            assert torch.all(got[i] == 0.0), name
            continue
        err = rel_err_rows(_np(got[i]), ref[i])
        print(f"former VJP N={N} B={B} {name}: worst per-env rel err {_worst(err)}, tol 1e-12")
        assert np.all(err <= 1e-12), (name, err.max(), int(err.argmax()))


# ---- e. the adjoint kernel against the dense refined reference --------------------------------------

@pytest.mark.parametrize("K", G.ADJOINT_KS)
@pytest.mark.parametrize("N", G.ADJOINT_HORIZONS)
def test_adjoint_kernel_matches_reference_on_generic_inputs(N, K):
    """srbd_pdipm_backward on QPs the oracle former built from generic inputs (every env its own H, -mu and
    model blocks), at the oracle's K-iteration iterate, both seeds, per env and output. Worst error (K = 1 /
    K = 5, tolerance 1e-10 / 1e-9): N = 1 2.1e-11 (grad_b, env 15) / 1.1e-11 (grad_b, env 0), N = 2 1.7e-11 /
    7.9e-11 (grad_b, env 13), N = 3 5.1e-12 (grad_b, env 4) / 1.2e-12 (grad_G, env 2), N = 10 2.6e-12 (grad_b,
    env 3) / 4.3e-12 (grad_G, env 0)."""
    tol = dict(C.CASES)[K]
    _, qp = C.workload(N, "generic")
    ref = C.reference(N, "generic", K)
    dqp, dit = _cuda(qp), _cuda(C.iterate(N, "generic", K))
    for k, (seed, g) in enumerate(zip(["u0", "all"], _cuda(C.seeds(N)))):
        st = torch.full((C.BATCH,), -1, dtype=torch.int32, device="cuda")
        got = solver.pdipm_backward(dqp, dit, g, N, status=st)
        torch.cuda.synchronize()
        assert torch.all(st == 0), st
        for o, name in enumerate(C.NAMES):
            err = rel_err_rows(_np(got[o]), ref[k][o])
            print(f"adjoint N={N} K={K} seed={seed} {name}: worst per-env rel err {_worst(err)}, tol {tol:.0e}")
            assert np.all(err <= tol), (seed, name, err.max(), int(err.argmax()))


# ---- f. composition and autograd ---------------------------------------------------------------------

def test_mpc_backward_equals_the_three_calls_on_generic_inputs():
    N, K = 3, 5
    ins = _cuda(C.workload(N, "generic")[0])
    it = _cuda(C.iterate(N, "generic", K))
    g = _cuda(C.seeds(N))[1]
    qp = solver.qp_former(ins, N)  # H, f, A, b, G, d
    grads = solver.pdipm_backward([qp[0], qp[4], qp[2], qp[1], qp[5], qp[3]], it, g, N)
    chain = solver.qp_former_backward(ins, grads, N)
    st = torch.full((C.BATCH,), -1, dtype=torch.int32, device="cuda")
    one = solver.mpc_backward(ins, it, g, N, status=st)
    torch.cuda.synchronize()
    assert torch.all(st == 0)
    for i in range(17):
        assert torch.equal(one[i], chain[i]), layout.FORMER_IN_NAMES[i]


@pytest.mark.parametrize("N", [3, 10])
def test_autograd_of_mass_mu_rotation_and_inertia_matches_the_reference_chain(N):
    """torch.autograd.grad through mpc_solve_autograd for dt, mass, mu, R_body, I_world and Q against the
    reference chain (oracle former -> dense refined adjoint -> NumPy former VJP) at the iterate the GPU
    returned, K = 5. Worst per-env error (tolerance 1e-9): N = 3 2.3e-11 (m, env 2; I_world 1.9e-12), N = 10
    5.1e-11 (I_world, env 15; m 1.6e-11, mu 2.5e-12, R_body 6.6e-12)."""
    K, tol = 5, 1e-9
    ins_np = C.workload(N, "generic")[0]
    want = [4, 5, 6, 7, 8, 13]
    ins = _cuda(ins_np)
    for i in want:
        ins[i].requires_grad_(True)
    x = solver.mpc_solve_autograd(ins, N, K)
    rng = np.random.default_rng(2970 + N)
    w = torch.from_numpy(rng.standard_normal((C.BATCH, 12))).cuda()
    loss = (x[:, 12 * N:12 * N + 12] * w).sum()
    grads = torch.autograd.grad(loss, [ins[i] for i in want])
    it = solver.mpc_solve([t.detach() for t in ins], N, K)[:4]
    torch.cuda.synchronize()
    assert torch.equal(it[0], x.detach())
    g = np.zeros((C.BATCH, 24 * N))
    g[:, 12 * N:12 * N + 12] = _np(w)
    ref = br.mpc_backward_batch(N, ins_np, [_np(t) for t in it], g)
    for i, gr in zip(want, grads):
        assert gr.shape == ins[i].shape
        err = rel_err_rows(_np(gr), ref[i])
        print(f"autograd N={N} {layout.FORMER_IN_NAMES[i]}: worst per-env rel err {_worst(err)}, tol {tol:.0e}")
        assert np.all(err <= tol), (layout.FORMER_IN_NAMES[i], err.max(), int(err.argmax()))
