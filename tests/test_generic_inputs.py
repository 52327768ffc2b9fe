"""The generic workload (tests/_generic.py) and the references the GPU tests of tests/test_gpu_generic.py
lean on, held on the CPU.

1. The inputs cannot hide the errors they are for (the oracle alone): a transposed I_world, another env's
   dt / mass / mu / Q / R each move the QP of every env by far more than any parity tolerance, and the
   linearisation point moves nothing.
2. The seed rule of the solver cases (tests/test_sweep_floor.py's rule, on the generic inputs).
3. The NumPy former VJP (tests/_backward_ref.py) against central differences of the oracle at generic
   points: asymmetric inertia, a non-orthonormal R_body, fractional contact.
4. The adjoint's reduced-elimination floor on the generic adjoint cases.
(The adjoint reference against central differences at a generic point: tests/test_backward_ref.py.)
"""
import numpy as np
import pytest

from biped_pympc_amd import layout
from oracle import oracle
from tests import _backward_ref as br
from tests import _generic as G
from tests._util import SWEEP_CASES, dense_floor_env, rel_err_rows
from tests.test_backward_ref import _accept, _dv

NAMES = ["H", "f", "A", "b", "G", "d"]


# ------------------------------------------------------------------ 1. the inputs ----

@pytest.fixture(scope="module", params=[True, False], ids=["solvable", "former_only"])
def generic3(request):
    N, B = 3, 16
    P = G.generic_former_inputs(B, N, seed=2100, solvable=request.param)
    return N, B, P, oracle.qp_former(N, P)


def _moved(out, ref):
    """(6, B): per output and env, the norm-wise relative change; for H the largest entry-wise relative
    change instead (H is the weights themselves, spread over 250 .. 1e-5, and the GPU test compares it bit for
    bit: a norm-wise measure would let Q's scale cover a wrong R)."""
    mv = np.stack([rel_err_rows(o, r) for o, r in zip(out, ref)])
    mv[0] = (np.abs(out[0] - ref[0]) / np.abs(ref[0])).max(axis=1)
    return mv


def test_transposed_inertia_moves_A_or_b_of_every_env(generic3):
    N, B, P, ref = generic3
    Q = list(P)
    Q[8] = np.ascontiguousarray(P[8].reshape(B, 3, 3).transpose(0, 2, 1).reshape(B, 9))
    assert not np.array_equal(Q[8], P[8])
    mv = _moved(oracle.qp_former(N, Q), ref)
    worst = np.maximum(mv[2], mv[3])
    print(f"transposed I_world: smallest change of A or b over the envs {worst.min():.3e}")
    assert np.all(worst > 1e-6), worst


@pytest.mark.parametrize("i", [4, 5, 6, 13, 14])
def test_another_envs_scalar_moves_every_other_env(generic3, i):
    N, B, P, ref = generic3
    Q = list(P)
    Q[i] = np.ascontiguousarray(np.broadcast_to(P[i][0:1], P[i].shape))
    mv = _moved(oracle.qp_former(N, Q), ref).max(axis=0)
    print(f"{layout.FORMER_IN_NAMES[i]} of env 0 everywhere: smallest change over envs 1.. {mv[1:].min():.3e}")
    assert mv[0] == 0.0
    assert np.all(mv[1:] > 1e-6), mv


def test_the_linearisation_input_u_moves_nothing(generic3):
    """The QP does not depend on u. H, f, A and G do not change by a bit (the oracle's r u - r u and its
    Jacobians are exact). b = A z - eq(z) and d = G z - ineq(z) cancel the u terms in floating point: what
    is left of u there is rounding noise, held below 1e-12 per env -- the former's own parity bound, six
    orders under the 1e-6 the two tests above ask for (measured: b 1.4e-14, d 1.3e-16)."""
    N, B, P, ref = generic3
    Q = list(P)
    Q[2] = np.ones_like(P[2])
    out = oracle.qp_former(N, Q)
    for k in (0, 1, 2, 4):
        assert np.array_equal(out[k], ref[k]), NAMES[k]
    for k in (3, 5):
        err = rel_err_rows(out[k], ref[k])
        print(f"u = 1: {NAMES[k]} moved by {err.max():.3e}")
        assert np.all(err <= 1e-12), (NAMES[k], err.max())
    # the oracle's cancelling rows of d are exact zeros at the generic u as well
    assert np.all(ref[5][:, G.d_cancelling_rows(N)] == 0.0)


# ------------------------------------------------------------------ 2. the seed rule ----

@pytest.mark.slow
@pytest.mark.parametrize("N", G.SOLVER_HORIZONS)
def test_solver_case_seed_keeps_the_floor_under_a_quarter_of_the_tolerance(N):
    """seed = 2300 + N + 100 j, the first j >= 0 at which every env's floor between the two CPU restatements
    (tests/_util.py dense_floor_env) is at most a quarter of the SWEEP_CASES tolerance at K = 1 and K = 3:
    j = 0 at all six horizons. Worst floors (K = 1 / K = 3): N = 1 4.4e-12 / 2.5e-12, N = 3 1.5e-11 /
    3.1e-12, N = 10 7.6e-12 / 9.9e-12, N = 16 3.7e-12 / 8.4e-12, N = 20 3.5e-12 / 6.0e-12, N = 32 1.5e-11 /
    2.4e-11, against 2.5e-11 / 2.5e-10."""
    assert G.SOLVER_SEED_J.get(N, 0) == 0  # no earlier j to show failing
    _, ins = G.solver_case_inputs(N)
    for K, tol in SWEEP_CASES:
        worst = max(max(dense_floor_env(N, K, ins, e)) for e in range(G.SOLVER_BATCH))
        print(f"N={N} K={K}: worst floor {worst:.3e} (tolerance {tol:.0e})")
        assert worst <= tol / 4.0, (N, K, worst)


# ------------------------------------------------------------------ 3. former VJP ----

# Round-off of the difference quotient. fd(t) = sum_i cot_i (out_i(P + t dv) - out_i(P - t dv)) / (2 t). An
# output value of the oracle carries at most k = 51 roundings (the longest chain, a row of b = A z - eq(z):
# I^-1 6 (cofactor 2, determinant 3, quotient 1), torque and I^-1 tau + a_ang 5 more, (dt / 2) k_1 and
# x + . 2, R omega of the next stage 4, the RK4 sum 2 k_2, its three additions, (dt / 6) s and x + . 7,
# eq = x_next - . 1, then the entry times z and up to 25 column accumulations of A z 26, and b = A z - eq 1;
# the constants dt / 2 and dt / 6 are formed once). Each of the two evaluations is therefore off by at most
# k u |out_i|, u = 2^-53, and the quotient by (2 k u / (2 t)) sum |cot_i out_i| = (k / 2) 2^-52 sum / t. The
# term below takes c = k = 51: the factor two left over covers the rounding of P +- t dv itself (one u on
# the input, at most two on a map that is at most quadratic in it) and the cancellation inside b and d,
# whose terms exceed the entry. The difference, the product with cot, the sum and the division round
# relative to fd itself; the rule's 1e-12 magnitude term covers them.
C_ROUNDOFF = 51


def _accept_roundoff(fd_t, fd_h, analytic, magnitude, scale, t):
    return abs(fd_t - analytic) <= (10.0 * abs(fd_t - fd_h) + 1e-12 * magnitude
                                    + C_ROUNDOFF * 2.0 ** -52 * scale / t)


@pytest.fixture(scope="module", params=[1, 3])
def former_case(request):
    N = request.param
    P = [a[1].copy() for a in G.generic_former_inputs(2, N, seed=2200 + N, solvable=False)]
    rng = np.random.default_rng(2205 + N)
    cot = [rng.standard_normal(w) for w in layout.Dims(N).former_out_nnz]
    out = oracle.qp_former(N, P)
    scale = sum(float(np.abs(c * a).sum()) for c, a in zip(cot, out))
    return N, P, cot, br.former_vjp(N, P, cot), scale


def test_former_case_is_generic(former_case):
    N, P, _, _, _ = former_case
    Iw, R = P[8].reshape(3, 3), P[7].reshape(3, 3)
    assert np.abs(Iw - Iw.T).max() > 1e-4 and np.abs(R @ R.T - np.eye(3)).max() > 1e-3
    assert np.all((P[12] > 0.0) & (P[12] < 1.0)) and np.all(P[1] != 1.0) and np.all(P[2] != 1.0)


@pytest.mark.parametrize("i", range(17))
def test_former_vjp_matches_central_differences_at_a_generic_point(former_case, i):
    """The rule of tests/test_backward_ref.py plus a round-off term (C_ROUNDOFF above): where the map is
    exactly linear in an input (dt at N = 1, body_pos, residual_ang_accel), fd(t) and fd(t / 2) agree to
    round-off, the truncation estimate 10 |fd(t) - fd(t / 2)| vanishes and only the round-off of the quotient
    is left. The existing cases keep the rule without it. The sum of the term runs over the output entries the
    perturbation reaches (the others are the same bits in both evaluations), which only tightens it: the term is
    at most 1.2e-8 of the gradient's magnitude (residual_ang_accel at N = 1), so the rule still checks eight
    digits. At these two points every input also passes without the term (printed)."""
    N, P, cot, vjp, scale = former_case
    rng = np.random.default_rng(900 + i)
    dv = _dv(rng, P[i])
    analytic = float(vjp[i] @ dv)
    magnitude = float(np.abs(vjp[i] * dv).sum())

    touched = [0.0]

    def fd(t):
        def outs(sign):
            Q = [a.copy() for a in P]
            Q[i] = P[i] + sign * t * dv
            return oracle.qp_former(N, Q)
        op, om = outs(1.0), outs(-1.0)
        # an entry the perturbation does not reach is the same bits in both evaluations and adds an exact
        # zero, round-off included: the term's sum runs over the entries that moved
        touched[0] = max(touched[0], sum(float(np.abs(c * a)[a != b].sum()) for c, a, b in zip(cot, op, om)))
        return sum(float(c @ (a - b)) for c, a, b in zip(cot, op, om)) / (2.0 * t)
    t = 1e-3
    fd_t, fd_h = fd(t), fd(t / 2)
    scale = min(scale, touched[0]) if i not in (1, 2) else scale
    roundoff = C_ROUNDOFF * 2.0 ** -52 * scale / t
    print(f"N={N} input {layout.FORMER_IN_NAMES[i]}: analytic {analytic:.12e} fd(t) {fd_t:.12e} "
          f"fd(t/2) {fd_h:.12e} magnitude {magnitude:.3e} round-off term {roundoff:.3e} "
          f"|fd(t) - analytic| {abs(fd_t - analytic):.3e} passes without it: {_accept(fd_t, fd_h, analytic, magnitude)}")
    if i in (1, 2):  # the linearisation point: the QP does not depend on it
        assert analytic == 0.0 and np.all(vjp[i] == 0.0)
        assert abs(fd_t) <= 1e-12 * scale / t
        return
    assert magnitude > 0.0
    assert _accept_roundoff(fd_t, fd_h, analytic, magnitude, scale, t)


# ------------------------------------------------------------------ 4. adjoint floor ----

@pytest.mark.parametrize("N", G.ADJOINT_HORIZONS)
def test_reduced_elimination_floor_on_the_generic_adjoint_cases(N):
    """The reference alone, on the inputs of tests/test_gpu_generic.py's adjoint test (seed = 2900 + N + 100 j,
    j = 0 at every horizon): the plain-FP64 reduced elimination stays within the CASES tolerance on every env,
    output and seed. Worst (K = 1 / K = 5, against 1e-10 / 1e-9): N = 1 1.1e-11 / 4.5e-10, N = 2 2.5e-12 /
    1.9e-11, N = 3 5.3e-13 / 6.9e-12, N = 10 2.0e-12 / 7.6e-12."""
    from tests import _backward_cases as C
    assert G.ADJOINT_SEED_J.get(N, 0) == 0
    for K in G.ADJOINT_KS:
        tol = dict(C.CASES)[K]
        worst = max(float(f.max()) for f in C.reduced_floor(N, "generic", K))
        print(f"N={N} generic K={K}: worst floor {worst:.3e} (tol {tol:.0e})")
        assert worst <= tol
