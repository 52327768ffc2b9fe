"""The references of tests/_step_backward_ref.py against central differences of the forward restatements
(oracle.mpc_io.prepare_inputs, u0_wrench, stance_torque). No GPU.

Every map is at most quadratic in one input (I_world = R I_body R^T and the wrench's R^T u are the quadratic /
bilinear ones), so a central difference carries no truncation error and the acceptance rule is the round-off
term alone:
    |fd - analytic| <= C 2^-24 sum |cot out| / t,
the sum over the output entries the perturbation reaches (the others have the same bits in both evaluations).
C counts the FP32 roundings between the perturbed input and an output entry in the restatement: each of the two
evaluations is off by at most C u |out|, u = 2^-24 (first order), and the quotient by 2 C u sum |cot out| / (2 t).
Steps t are powers of two, and no select (first_run, stationary) may flip between P - t dv and P + t dv.
"""
import numpy as np
import pytest

from oracle import mpc_io
from tests import _step_backward_ref as R
from tests.test_controller import random_robot

f32, f64 = np.float32, np.float64

# Longest chain of the preparation: I_world = (R I_body) R^T, two three-term products of 3 multiplications and
# 2 additions each = 10 roundings, plus the rounding of the perturbed input P +- t dv itself.
C_ROUNDOFF = 11
# u0 -> wrench: the cast of x (or the rounding of R +- t dv) and one three-term product (5); the negation is exact.
C_WRENCH = 6
# wrench -> torque adds the six-term product J^T w: 6 multiplications and 5 additions.
C_TORQUE = C_WRENCH + 11

BATCH = 8
T_STEP = 2.0 ** -6
T_STEP_VELOCITY = 2.0 ** -8  # desired_velocity_b: the stationary envs sit at v_x = 0 and must stay below 1e-2


def _prep_case(N, seed):
    st, cmd, ctrl, params, _, _ = random_robot(BATCH, seed, N, gait=False)
    rng = np.random.default_rng(seed + 1)
    vb = cmd["desired_velocity_b"]
    moving = np.abs(vb[:, 0]) >= 1e-2
    vb[moving, 0] = np.where(vb[moving, 0] < 0, -1.0, 1.0) * np.maximum(np.abs(vb[moving, 0]), 0.05)
    vb[:, 2] = rng.uniform(-0.2, 0.2, BATCH).astype(f32)  # the kernel reads all three components
    table = rng.uniform(0.05, 0.95, (BATCH, N, 2)).astype(f32)  # fractional: no entry at a corner
    first, stat = ctrl["first_run"], np.abs(vb[:, 0]) < 1e-2
    assert {(bool(a), bool(b)) for a, b in zip(first, stat)} == {(False, False), (False, True), (True, False), (True, True)}
    cot = [rng.standard_normal((BATCH, w)) for w in R.FORMER_WIDTHS(N)]
    cot_wpd = rng.standard_normal((BATCH, 3)).astype(f32)
    cot_yaw = rng.standard_normal(BATCH).astype(f32)
    return st, cmd, ctrl, params, table, cot, cot_wpd, cot_yaw


def _forward(N, st, cmd, ctrl, params, table, literal):
    ins, new = mpc_io.prepare_inputs(N, st, cmd, ctrl, params, contact_table=table, literal=literal)
    return ins + [new["world_position_desired"].astype(f64), new["yaw_desired"].astype(f64)[:, None]]


def _where(name, st, cmd, ctrl, params):
    for d in (st, cmd, ctrl, params):
        if name in d:
            return d
    raise KeyError(name)


def _fd(outs_p, outs_m, cots, t, chain):
    """Per env: the central difference of sum cot out, and the rule's sum over the entries that moved."""
    B = outs_p[0].shape[0]
    fd, scale = np.zeros(B), np.zeros(B)
    for op, om, c, k in zip(outs_p, outs_m, cots, chain):
        op, om, c = op.reshape(B, -1), om.reshape(B, -1), np.asarray(c, f64).reshape(B, -1)
        fd += (c * (op - om)).sum(axis=1) / (2.0 * t)
        scale += k * (np.abs(c) * np.maximum(np.abs(op), np.abs(om)) * (op != om)).sum(axis=1)
    return fd, scale * 2.0 ** -24 / t


@pytest.fixture(scope="module", params=[(1, True), (3, True), (3, False), (32, True), (32, False)],
                ids=lambda p: f"N{p[0]}-{'literal' if p[1] else 'corrected'}")
def prep_case(request):
    N, literal = request.param
    case = _prep_case(N, 4100 + N)
    st, cmd, ctrl, params, table, cot, cot_wpd, cot_yaw = case
    vjp = R.prepare_vjp(N, st, cmd, ctrl["first_run"], params, cot, literal, cot_wpd, cot_yaw)
    return N, literal, case, vjp


@pytest.mark.parametrize("name", R.FIELDS)
def test_prepare_vjp_matches_central_differences(prep_case, name):
    N, literal, (st, cmd, ctrl, params, table, cot, cot_wpd, cot_yaw), vjp = prep_case
    t = T_STEP_VELOCITY if name == "desired_velocity_b" else T_STEP
    rng = np.random.default_rng(97 + R.FIELDS.index(name))
    base = table if name == "contact_table" else _where(name, st, cmd, ctrl, params)[name]
    dv = rng.uniform(-1.0, 1.0, base.shape)
    outs = []
    for sign in (1.0, -1.0):
        dicts = [dict(d) for d in (st, cmd, ctrl, params)]
        tab = table
        moved = (base.astype(f64) + sign * t * dv).astype(f32)
        if name == "contact_table":
            tab = moved
        else:
            _where(name, *dicts)[name] = moved
        # no select flips: first_run is not perturbed, stationary is a function of v_x alone
        assert np.array_equal(R.forward_intermediates(dicts[0], dicts[1])[2], R.forward_intermediates(st, cmd)[2])
        outs.append(_forward(N, *dicts, tab, literal))
    fd, bound = _fd(outs[0], outs[1], cot + [cot_wpd, cot_yaw[:, None]], t, [C_ROUNDOFF] * 19)
    analytic = (vjp[name].reshape(BATCH, -1) * dv.reshape(BATCH, -1)).sum(axis=1)
    err = np.abs(fd - analytic)
    print(f"N={N} literal={literal} {name}: worst |fd - analytic| = {(err / np.maximum(bound, 1e-300)).max():.3f} "
          f"of the round-off term (C = {C_ROUNDOFF}), worst relative to the gradient "
          f"{(err / np.maximum(np.abs(analytic), 1e-300)).max():.2e}")
    assert np.all(err <= bound), (err, bound)  # an env the perturbation does not reach: 0 <= 0


def test_entries_the_table_marks_zero_are_exact_zeros(prep_case):
    N, literal, (st, cmd, ctrl, params, *_), vjp = prep_case
    first = ctrl["first_run"].astype(bool)
    stat = R.forward_intermediates(st, cmd)[2]
    assert np.all(vjp["desired_angular_velocity_b"][:, :2] == 0.0)
    assert np.all(vjp["world_position_desired"][:, 2] == 0.0)
    assert np.all(vjp["world_position_desired"][first] == 0.0) and np.all(vjp["yaw_desired"][first] == 0.0)
    assert np.all(vjp["yaw_desired"][~first] != 0.0) and np.all(vjp["world_position_desired"][~first, :2] != 0.0)
    assert first.any() and (~first).any() and stat.any() and (~stat).any()
    for name in R.FIELDS:
        assert vjp[name].shape[1:] == {"rotation_body": (3, 3), "foot_position": (2, 3), "desired_height": (),
                                       "yaw_desired": (), "contact_table": (N, 2), "dt_mpc": ()}.get(name, (3,)), name


def test_null_cotangents_are_zeros_and_magnitude_bounds_the_value(prep_case):
    N, literal, (st, cmd, ctrl, params, table, cot, cot_wpd, cot_yaw), vjp = prep_case
    some = [c if i in (3, 4) else None for i, c in enumerate(cot)]
    zeros = [c if i in (3, 4) else np.zeros_like(c) for i, c in enumerate(cot)]
    a = R.prepare_vjp(N, st, cmd, ctrl["first_run"], params, some, literal)
    b = R.prepare_vjp(N, st, cmd, ctrl["first_run"], params, zeros, literal, np.zeros((BATCH, 3), f32), np.zeros(BATCH, f32))
    mag = R.prepare_vjp(N, st, cmd, ctrl["first_run"], params, cot, literal, cot_wpd, cot_yaw, absolute=True)
    for name in R.FIELDS:
        assert np.array_equal(a[name], b[name]), name
        assert np.all(np.abs(vjp[name]) <= mag[name] * (1 + 1e-12)), name


# ---- the wrench / torque tail ----

def _wrench_case(N, seed, ndof=5):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 50, (BATCH, 24 * N))
    Rm = np.linalg.qr(rng.normal(size=(BATCH, 3, 3)))[0].astype(f32)
    J = rng.normal(0, 0.3, (BATCH, 2, 6, ndof)).astype(f32)
    cb = np.ones((BATCH, 2), f32)
    cb[::2, 1] = 0.0  # one swing leg in half the envs
    gw = rng.standard_normal((BATCH, 2, 6)).astype(f32)
    gt = rng.standard_normal((BATCH, 2, ndof)).astype(f32)
    return x, Rm, J, cb, gw, gt


@pytest.mark.parametrize("torque", [False, True])
@pytest.mark.parametrize("N", [1, 3, 32])
def test_wrench_vjp_matches_central_differences(N, torque):
    x, Rm, J, cb, gw, gt = _wrench_case(N, 4300 + N)
    gx, gR = R.wrench_vjp(N, x, Rm, gw, *((gt, J, cb) if torque else ()))
    u0 = slice(12 * N, 12 * N + 12)
    assert np.all(gx[:, :12 * N] == 0.0) and np.all(gx[:, 12 * N + 12:] == 0.0)
    assert np.all(gx[:, 12 * N + 6] == 0.0) and np.all(gx[:, 12 * N + 9] == 0.0)
    assert np.all(gx[:, u0][:, [0, 1, 2, 3, 4, 5, 7, 8, 10, 11]] != 0.0)

    def forward(xv, Rv):
        w = mpc_io.u0_wrench(N, xv, Rv)
        return [w.astype(f64), mpc_io.stance_torque(w, J, cb).astype(f64)] if torque else [w.astype(f64)]
    rng = np.random.default_rng(4400 + N)
    t = T_STEP
    for name, grad in (("x", gx), ("rotation_body", gR)):
        dv = rng.uniform(-1.0, 1.0, (x if name == "x" else Rm).shape)
        if name == "x":
            outs = [forward(x + s * t * dv, Rm) for s in (1.0, -1.0)]
        else:
            outs = [forward(x, (Rm.astype(f64) + s * t * dv).astype(f32)) for s in (1.0, -1.0)]
        fd, bound = _fd(outs[0], outs[1], [gw, gt], t, [C_WRENCH, C_TORQUE])
        analytic = (grad.reshape(BATCH, -1) * dv.reshape(BATCH, -1)).sum(axis=1)
        err = np.abs(fd - analytic)
        print(f"N={N} torque={torque} {name}: worst |fd - analytic| = {(err / bound).max():.3f} of the round-off term")
        assert np.all(err <= bound), (name, err, bound)
    mx, mR = R.wrench_vjp(N, x, Rm, gw, *((gt, J, cb) if torque else ()), absolute=True)
    assert np.all(np.abs(gx) <= mx * (1 + 1e-12)) and np.all(np.abs(gR) <= mR * (1 + 1e-12))
