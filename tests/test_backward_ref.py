"""The backward pass's reference (tests/_backward_ref.py) against central differences, on the CPU.

Adjoint formulas: the iterate of a K-iteration solve is made an exact root of the frozen-residual KKT
map F (the map whose Jacobian at the iterate is the solver's Newton matrix K: the complementarity row
scaled by the iterate's own 1 / s, the regularisation terms beta, delta in place) by subtracting F's value
there; the root of the perturbed data is re-solved by Newton and L = g^T x differenced. Former VJP:
central differences of oracle.qp_former.

The check calibrates itself: with two step sizes t and t / 2,
    |fd(t) - analytic| <= 10 |fd(t) - fd(t / 2)| + 1e-12 * magnitude,
magnitude = sum_i |grad_i dv_i| (the size of the terms the derivative is summed from). Perturbations are
scaled per entry, dv_i = xi_i |theta_i| (xi ~ N(0, 1); an entry that is exactly zero moves by xi_i): a
uniform step is too coarse for the 1e-5 entries of R and for near-degenerate h.
"""
import numpy as np
import pytest

from biped_pympc_amd import layout
from biped_pympc_amd.utils.synthetic import make_workload, solver_init
from oracle import oracle
from tests import _backward_ref as br


def _dv(rng, theta):
    a = np.abs(theta)
    return rng.standard_normal(theta.shape) * np.where(a > 0, a, 1.0)


def _accept(fd_t, fd_h, analytic, magnitude):
    return abs(fd_t - analytic) <= 10.0 * abs(fd_t - fd_h) + 1e-12 * magnitude


# ------------------------------------------------------------------ adjoint formulas ----

class _Root:
    """The frozen-residual KKT root through the iterate w0 = (x, s, z, y) of the data theta0."""

    def __init__(self, N, theta, w0):
        self.N, self.w0 = N, [np.asarray(v, np.float64) for v in w0]
        self.s0 = self.w0[1].copy()
        self.c = self.F(theta, self.w0)

    def F(self, theta, w):
        Hv, f, Av, b, Gv, d = theta
        H, G, A = br.dense_qp(self.N, Hv, Gv, Av)
        x, s, z, y = w
        return np.concatenate([
            H @ x + br.BETA * x + f + G.T @ z + A.T @ y,
            s * z / self.s0 + br.DELTA * s,
            G @ x + s - d - br.DELTA * z,
            A @ x - b - br.DELTA * y])

    def solve(self, theta):
        Hv, f, Av, b, Gv, d = theta
        H, G, A = br.dense_qp(self.N, Hv, Gv, Av)
        N = self.N
        nz, m = 24 * N, 16 * N
        w = np.concatenate(self.w0)
        for _ in range(30):
            x, s, z, y = br.split(N, w)
            K = br.dense_kkt(N, H, G, A, self.s0, z)  # row 2: (z / s0 + delta) ds + (s / s0) dz
            K[nz:nz + m, nz + m:nz + 2 * m] = np.diag(s / self.s0)
            r = self.F(theta, (x, s, z, y)) - self.c
            step = br.solve_refined(K, -r, steps=1)
            w = w + step
            if np.abs(step).max() <= 1e-15 * np.abs(w).max():
                break
        return br.split(N, w)[0]


def _adjoint_case(former_inputs):
    N, K = 2, 5
    H, f, A, b, G, d = [a[1] for a in oracle.qp_former(N, former_inputs)]
    it = solver_init(d[None], N)
    out = oracle.pdipm(N, K, [H, G, A, f, d, b] + [v[0] for v in it])
    w0 = [np.asarray(out[k]).reshape(-1) for k in range(4)]
    rng = np.random.default_rng(7)
    g = rng.standard_normal(24 * N)
    theta = [H, f, A, b, G, d]
    grads = br.pdipm_backward(N, [H, G, A, f, d, b] + w0, g)
    return N, theta, w0, g, grads


@pytest.fixture(scope="module")
def adjoint_case():
    return _adjoint_case(make_workload(2, 2, seed=41, random_gait=True, residuals=True).inputs)


@pytest.fixture(scope="module")
def adjoint_case_generic():
    """The same N = 2, K = 5 case with the QP of a generic env (tests/_generic.py: its own dt, mass, mu, Q, R,
    asymmetric inertia, a generic linearisation point)."""
    from tests._generic import generic_former_inputs
    return _adjoint_case(generic_former_inputs(2, 2, seed=41, solvable=True))


@pytest.mark.parametrize("which", ["H", "f", "A", "b", "G", "d", "all"])
def test_adjoint_gradients_match_central_differences_of_the_frozen_root(adjoint_case, which):
    _check_adjoint_against_central_differences(adjoint_case, which)


@pytest.mark.parametrize("which", ["H", "f", "A", "b", "G", "d", "all"])
def test_adjoint_gradients_match_central_differences_at_a_generic_point(adjoint_case_generic, which):
    _check_adjoint_against_central_differences(adjoint_case_generic, which)


def _check_adjoint_against_central_differences(case, which):
    N, theta, w0, g, grads = case
    root = _Root(N, theta, w0)
    assert np.abs(root.solve(theta) - w0[0]).max() <= 1e-12 * np.abs(w0[0]).max()  # w0 is the root
    rng = np.random.default_rng(100 + sum(map(ord, which)))
    names = ["H", "f", "A", "b", "G", "d"]
    dv = [_dv(rng, th) if which in (n, "all") else np.zeros_like(th) for n, th in zip(names, theta)]
    analytic = sum(float(gr @ v) for gr, v in zip(grads, dv))
    magnitude = sum(float(np.abs(gr * v).sum()) for gr, v in zip(grads, dv))

    def fd(t):
        xp = root.solve([th + t * v for th, v in zip(theta, dv)])
        xm = root.solve([th - t * v for th, v in zip(theta, dv)])
        return float(g @ (xp - xm)) / (2.0 * t)
    # d = 500 on the force-limit rows while the smallest slack of this iterate is 3e-6: the root is
    # strongly curved in d, and a step of 1e-4 |d| sits outside the quadratic regime of the central
    # difference (fd(t) and fd(t / 2) then agree with each other to 1 % and with nothing else); 1e-8 |d|
    # is of the size of that slack
    t = 1e-8 if which in ("d", "all") else 1e-4
    fd_t, fd_h = fd(t), fd(t / 2)
    print(f"{which}: analytic {analytic:.12e} fd(t) {fd_t:.12e} fd(t/2) {fd_h:.12e} magnitude {magnitude:.3e}")
    assert magnitude > 0.0
    assert _accept(fd_t, fd_h, analytic, magnitude)


def test_reduced_elimination_agrees_with_the_dense_adjoint(adjoint_case):
    N, theta, w0, g, grads = adjoint_case
    H, f, A, b, G, d = theta
    red = br.pdipm_backward(N, [H, G, A, f, d, b] + w0, g, reduced=True)
    for a, r in zip(red, grads):
        assert np.abs(a - r).max() <= 1e-9 * np.abs(r).max()  # K = 5: the project's SOLVER_CASES bound


@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_reduced_elimination_floor_is_within_the_gpu_tolerance_on_the_gpu_cases(N):
    """The reference alone, on the exact inputs of tests/test_gpu_backward.py: the plain-FP64 reduced
    elimination stays within the SOLVER_CASES tolerance on every env, output and seed, so the GPU test
    excludes no env and needs no per-env floor. (N = 32, 27 s here: worst 1.5e-12 / 2.4e-11 / 4.3e-10 /
    3.0e-6 against 1e-10 / 1e-9 / 1e-7 / 1e-5.)"""
    from tests import _backward_cases as C
    for gait in C.GAITS:
        for K, tol in C.CASES:
            worst = max(float(f.max()) for f in C.reduced_floor(N, gait, K))
            print(f"N={N} {gait} K={K}: worst floor {worst:.3e} (tol {tol:.0e})")
            assert worst <= tol


# ------------------------------------------------------------------ former VJP ----

REQUIRED = [0, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16]  # x0, x_ref, dt, m, mu, positions, ct, Q, R, residuals
WELCOME = [7, 8]  # R_body, I_world


@pytest.fixture(scope="module", params=[1, 3])
def former_case(request):
    N = request.param
    wl = make_workload(1, N, seed=60 + N, random_gait=True, residuals=True)
    P = [a[0].copy() for a in wl.inputs]
    rng = np.random.default_rng(5 + N)
    cot = [rng.standard_normal(w) for w in layout.Dims(N).former_out_nnz]
    return N, P, cot, br.former_vjp(N, P, cot)


@pytest.mark.parametrize("i", REQUIRED + WELCOME + [1, 2])
def test_former_vjp_matches_central_differences_of_the_oracle(former_case, i):
    N, P, cot, vjp = former_case
    rng = np.random.default_rng(900 + i)
    dv = _dv(rng, P[i])
    analytic = float(vjp[i] @ dv)
    magnitude = float(np.abs(vjp[i] * dv).sum())

    def fd(t):
        def outs(sign):
            Q = [a.copy() for a in P]
            Q[i] = P[i] + sign * t * dv
            return oracle.qp_former(N, Q)
        op, om = outs(1.0), outs(-1.0)
        return sum(float(c @ (a - b)) for c, a, b in zip(cot, op, om)) / (2.0 * t)
    t = 1e-3
    fd_t, fd_h = fd(t), fd(t / 2)
    print(f"N={N} input {layout.FORMER_IN_NAMES[i]}: analytic {analytic:.12e} fd(t) {fd_t:.12e} "
          f"fd(t/2) {fd_h:.12e} magnitude {magnitude:.3e}")
    if i in (1, 2):  # the linearisation point: the QP does not depend on it
        assert analytic == 0.0 and np.all(vjp[i] == 0.0)
        scale = sum(float(np.abs(c * a).sum()) for c, a in zip(cot, oracle.qp_former(N, P)))
        assert abs(fd_t) <= 1e-12 * scale / t
        return
    assert magnitude > 0.0
    assert _accept(fd_t, fd_h, analytic, magnitude)
