"""The backward pass of the controller step on the GPU: the wrench / torque VJP (srbd_u0_wrench_backward), the
input-preparation VJP (srbd_prepare_inputs_backward), their chain through the QP (srbd_mpc_step_backward) and the
controller's backward() / run_autograd().

References: tests/_step_backward_ref.py (NumPy FP64; tests/test_step_backward_ref.py holds them against central
differences of the forward restatements). Bounds: the two kernels sum at most a few dozen FP64 terms, so their
FP64 values sit within 1e-12 of the *magnitude* (the same sums over absolute values: the former VJP's bound);
an FP32 output adds its one rounding, 2^-24 |ref|. The chain is compared at the iterate and the former inputs
the GPU step itself returned, with the adjoint's tolerance of the K that produced the iterate
(tests/_backward_cases.py CASES) plus two FP32 roundings, 2^-23, norm-wise per env and output, no env excluded.

Shapes: N in {1, 3, 6, 32} (12N = 12, 36, 72, 384: under one pass of the stage reduction's 60 lanes, under one,
just over one, seven; 2N = 64 fills a wave of the contact-table loop exactly) and B in {1, 16, 67} (three idle
waves; whole workgroups; a partial last workgroup).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from biped_pympc_amd import _native, solver
from tests import _backward_cases as C
from tests import _step_backward_ref as R
from tests.test_controller import _controller, random_robot

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
HORIZONS = [1, 3, 6, 32]
BATCHES = [1, 16, 67]
TOL_K5 = dict(C.CASES)[5]
NDOF = 5


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


# ---- 1. the wrench / torque VJP -------------------------------------------------------------------

def _wrench_case(N, B):
    rng = np.random.default_rng(5000 + 100 * N + B)
    x = rng.normal(0, 50, (B, 24 * N))
    Rm = np.linalg.qr(rng.normal(size=(B, 3, 3)))[0].astype(f32)
    J = rng.normal(0, 0.3, (B, 2, 6, NDOF)).astype(f32)
    cb = np.ones((B, 2), f32)
    cb[::2, 1] = 0.0  # one swing leg in half the envs
    gw = rng.standard_normal((B, 2, 6)).astype(f32)
    gt = rng.standard_normal((B, 2, NDOF)).astype(f32)
    return x, Rm, J, cb, gw, gt


@pytest.mark.parametrize("torque", [False, True])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", HORIZONS)
def test_wrench_vjp_matches_the_reference(N, B, torque):
    x, Rm, J, cb, gw, gt = _wrench_case(N, B)
    extra = (gt, J, cb) if torque else ()
    gx = torch.full((B, 24 * N), float("nan"), dtype=torch.float64, device="cuda")
    got_x, got_R = solver.u0_wrench_backward(_cuda(x), _cuda(Rm), _cuda(gw), N, *(_cuda(a) for a in extra), grad_x=gx)
    only_x, none_R = solver.u0_wrench_backward(_cuda(x), _cuda(Rm), _cuda(gw), N, *(_cuda(a) for a in extra),
                                               want_rotation=False)
    torch.cuda.synchronize()
    ref_x, ref_R = R.wrench_vjp(N, x, Rm, gw, *extra)
    mag_x, mag_R = R.wrench_vjp(N, x, Rm, gw, *extra, absolute=True)
    ex, eR = np.abs(_np(got_x) - ref_x), np.abs(_np(got_R) - ref_R)
    print(f"N={N} B={B} torque={torque}: worst error / magnitude: grad_x {(ex / np.maximum(mag_x, 1e-300)).max():.2e} "
          f"grad_rotation_body {(eR / mag_R).max():.2e} (bound 1e-12)")
    assert np.all(ex <= 1e-12 * mag_x) and np.all(eR <= 1e-12 * mag_R)
    g = _np(got_x)
    assert np.all(g[:, :12 * N] == 0.0) and np.all(g[:, 12 * N + 12:] == 0.0)  # exact zeros, the whole row written
    assert np.all(g[:, 12 * N + 6] == 0.0) and np.all(g[:, 12 * N + 9] == 0.0)
    assert np.all(g[:, 12 * N:12 * N + 6] != 0.0)
    assert none_R is None and torch.equal(only_x, got_x)
    if torque:  # the torque's cotangent reaches only the stance legs
        plain = solver.u0_wrench_backward(_cuda(x), _cuda(Rm), _cuda(gw), N)[0]
        both_swing = solver.u0_wrench_backward(_cuda(x), _cuda(Rm), _cuda(gw), N, _cuda(gt), _cuda(J),
                                               _cuda(np.zeros_like(cb)))[0]
        assert torch.equal(both_swing, plain) and not torch.equal(got_x, plain)


# ---- 2. the input-preparation VJP -----------------------------------------------------------------

def _prep_struct(t: dict, params, literal, gait=False):
    """An MPCPrep of what srbd_prepare_inputs_backward reads, from CUDA tensors (kept alive by `t`)."""
    p = _native.MPCPrep()
    for name in ("rotation_body", "desired_velocity_b", "desired_angular_velocity_b", "dt_mpc", "first_run"):
        setattr(p, name, t[name].data_ptr())
    if gait:
        p.gait_phase = t["dt_mpc"].data_ptr()  # a mode flag to the backward entries: never read
    p.I_body[:] = [float(v) for v in np.asarray(params["I_body"], f32).reshape(-1)]
    p.step_dt = float(params["step_dt"])
    p.literal_layout = int(literal)
    p.q_len = 13
    return p


@functools.lru_cache(maxsize=None)
def _prep_case(N, B):
    st, cmd, ctrl, params, _, _ = random_robot(B, 5200 + 100 * N + B, N, gait=False)
    rng = np.random.default_rng(5300 + 100 * N + B)
    cmd["desired_velocity_b"][:, 2] = rng.uniform(-0.2, 0.2, B).astype(f32)
    cot = [rng.standard_normal((B, w)) for w in R.FORMER_WIDTHS(N)]
    gwpd, gyaw = rng.standard_normal((B, 3)).astype(f32), rng.standard_normal(B).astype(f32)
    direct = rng.standard_normal((B, 9))
    t = {"rotation_body": _cuda(st["rotation_body"]), "desired_velocity_b": _cuda(cmd["desired_velocity_b"]),
         "desired_angular_velocity_b": _cuda(cmd["desired_angular_velocity_b"]), "dt_mpc": _cuda(params["dt_mpc"]),
         "first_run": _cuda(ctrl["first_run"])}
    return st, cmd, ctrl, params, cot, gwpd, gyaw, direct, t


def _check_prep(got: dict, ref: dict, mag: dict, what: str):
    for name, g in got.items():
        g = _np(g).astype(f64)
        assert g.shape == ref[name].shape, name
        err, bound = np.abs(g - ref[name]), 2.0 ** -24 * np.abs(ref[name]) + 1e-12 * mag[name]
        assert np.all(err <= bound), (what, name, float((err - bound).max()))


@pytest.mark.parametrize("literal", [True, False])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", HORIZONS)
def test_prep_vjp_matches_the_reference(N, B, literal):
    st, cmd, ctrl, params, cot, gwpd, gyaw, direct, t = _prep_case(N, B)
    first = ctrl["first_run"]
    if B > 1:
        stat = R.forward_intermediates(st, cmd)[2]
        assert len({(bool(a), bool(b)) for a, b in zip(first, stat)}) == 4  # mixed first_run / stationary
    p = _prep_struct(t, params, literal)
    dcot = [_cuda(c) for c in cot]
    ref_args = (N, st, cmd, first, params)
    # every cotangent, the state cotangents and the direct term
    full = solver.prepare_inputs_backward(p, dcot, N, B, R.FIELDS, _cuda(gwpd), _cuda(gyaw), _cuda(direct))
    # without the state cotangents and the direct term
    plain = solver.prepare_inputs_backward(p, dcot, N, B, R.FIELDS)
    # null input cotangents are zeros
    some = [c if i in (3, 7) else None for i, c in enumerate(dcot)]
    zeros = [c if i in (3, 7) else torch.zeros_like(c) for i, c in enumerate(dcot)]
    nulls = solver.prepare_inputs_backward(p, some, N, B, R.FIELDS, _cuda(gwpd))
    zeroed = solver.prepare_inputs_backward(p, zeros, N, B, R.FIELDS, _cuda(gwpd), _cuda(np.zeros(B, f32)),
                                            _cuda(np.zeros((B, 9))))
    # a subset of the outputs has the bits of the full request
    subset = ("dt_mpc", "rotation_body", "contact_table", "root_position")
    part = solver.prepare_inputs_backward(p, dcot, N, B, subset, _cuda(gwpd), _cuda(gyaw), _cuda(direct))
    torch.cuda.synchronize()
    _check_prep(full, R.prepare_vjp(*ref_args, cot, literal, gwpd, gyaw, direct),
                R.prepare_vjp(*ref_args, cot, literal, gwpd, gyaw, direct, absolute=True), "full")
    _check_prep(plain, R.prepare_vjp(*ref_args, cot, literal), R.prepare_vjp(*ref_args, cot, literal, absolute=True),
                "plain")
    ncot = [c if i in (3, 7) else None for i, c in enumerate(cot)]
    _check_prep(nulls, R.prepare_vjp(*ref_args, ncot, literal, gwpd), R.prepare_vjp(*ref_args, ncot, literal, gwpd, absolute=True),
                "nulls")
    assert set(full) == set(R.FIELDS) and set(part) == set(subset)
    for name in R.FIELDS:
        assert full[name].dtype == torch.float32
        assert torch.equal(nulls[name], zeroed[name]), name
        if name in part:
            assert torch.equal(part[name], full[name]), name
    # the entries the table marks zero
    fr = _cuda(first)
    assert torch.all(full["desired_angular_velocity_b"][:, :2] == 0) and torch.all(full["world_position_desired"][:, 2] == 0)
    assert torch.all(full["yaw_desired"][fr] == 0) and torch.all(full["world_position_desired"][fr] == 0)


def test_prep_vjp_refuses_the_contact_table_gradient_in_gait_mode():
    N, B = 3, 16
    st, cmd, ctrl, params, cot, *_, t = _prep_case(N, B)
    p = _prep_struct(t, params, True, gait=True)
    dcot = [_cuda(c) for c in cot]
    with pytest.raises(RuntimeError, match="contact_table"):
        solver.prepare_inputs_backward(p, dcot, N, B, R.FIELDS)
    rest = [n for n in R.FIELDS if n != "contact_table"]
    got = solver.prepare_inputs_backward(p, dcot, N, B, rest)
    want = solver.prepare_inputs_backward(_prep_struct(t, params, True), dcot, N, B, rest)
    torch.cuda.synchronize()
    assert all(torch.equal(got[n], want[n]) for n in rest)


# ---- 3 / 4. the chain: srbd_mpc_step_backward, MPCControllerHIP.backward --------------------------

B_STEP = 16


def _torque(B, seed):
    rng = np.random.default_rng(seed)
    J = rng.normal(0, 0.3, (B, 2, 6, NDOF)).astype(f32)
    cb = np.ones((B, 2), f32)
    cb[::2, 1] = 0.0
    cb[1::4, 0] = 0.0
    return J, cb, rng.standard_normal((B, 2, 6)).astype(f32), rng.standard_normal((B, 2, NDOF)).astype(f32)


def _step_controller(N, gait, literal=True, differentiable=True, K=5):
    """A controller and the numpy inputs of its step: randomised gait or a fractional contact table,
    non-zero residual accelerations, mixed first_run / stationary envs."""
    st, cmd, ctrl, params, gait_args, table = random_robot(B_STEP, 5500 + N, N, gait=gait)
    table = np.random.default_rng(5600 + N).uniform(0.05, 0.95, table.shape).astype(f32)
    c = _controller(B_STEP, N, st, cmd, ctrl, params, gait_args, table, literal)
    c.cfg.keep_solution, c.cfg.differentiable, c.cfg.pdipm_iterations = True, differentiable, K
    return c, (st, cmd, ctrl, params)


@pytest.mark.parametrize("N", [3, 10])
def test_step_backward_has_the_bits_of_the_three_calls(N):
    c, (st, cmd, ctrl, params) = _step_controller(N, gait=False)
    c.run()
    J, cb, gw, gt = (_cuda(a) for a in _torque(B_STEP, 5700 + N))
    rec = c._step_record
    x = c.solution[0]
    rot = rec.tensors["rotation_body"]
    seed, direct = solver.u0_wrench_backward(x, rot, gw, N, gt, J, cb)
    st3 = torch.full((B_STEP,), -1, dtype=torch.int32, device="cuda")
    fin = solver.mpc_backward(c.former_inputs, list(c.solution[:4]), seed, N, status=st3)
    for wrt in (R.FIELDS, ("dt_mpc", "residual_lin_accel")):
        chain = solver.prepare_inputs_backward(rec.prep, fin, N, B_STEP, wrt, grad_rotation_body_direct=direct)
        st1 = torch.full((B_STEP,), -1, dtype=torch.int32, device="cuda")
        mask = sum(1 << R.FIELDS.index(n) for n in wrt)
        ws = torch.full((_native.lib().srbd_mpc_step_backward_workspace_doubles(N, B_STEP, mask),), float("nan"),
                        dtype=torch.float64, device="cuda")
        one = solver.mpc_step_backward(rec.prep, c.former_inputs, list(c.solution[:4]), gw, N, wrt, gt, J, cb,
                                       status=st1, workspace=ws)
        via = c.backward(gw, gt, J, cb, wrt=wrt)
        torch.cuda.synchronize()
        assert set(one) == set(wrt) == set(via)
        assert torch.all(st1 == 0) and torch.equal(st1, st3)
        for name in wrt:
            assert torch.equal(one[name], chain[name]) and torch.equal(via[name], chain[name]), name
            assert torch.isfinite(one[name]).all(), name


@pytest.mark.parametrize("gait", [True, False], ids=["gait", "table"])
@pytest.mark.parametrize("N", [3, 10])
def test_controller_backward_matches_the_reference_chain(N, gait):
    """backward() against the reference chain at the iterate and former inputs the GPU step returned, norm-wise
    per env and output: ||got - ref|| <= (tol_K + 2^-23) ||magnitude||, tol_K = 1e-9 at K = 5 plus two FP32
    roundings. Measured on an MI355X over the four cases: worst 5.5e-08 (one FP32 rounding; bound 1.2e-07)."""
    c, (st, cmd, ctrl, params) = _step_controller(N, gait)
    wrench = c.run()[0].clone()
    J, cb, gw, gt = _torque(B_STEP, 5800 + N)
    status = torch.full((B_STEP,), -1, dtype=torch.int32, device="cuda")
    got = c.backward(_cuda(gw), _cuda(gt), _cuda(J), _cuda(cb), status=status)
    torch.cuda.synchronize()
    assert torch.all(status == 0), status
    assert torch.equal(c.foot_wrench, wrench)  # the backward pass leaves the step's outputs alone
    assert set(got) == set(R.FIELDS) - ({"contact_table"} if gait else set())
    fin, it = [_np(t) for t in c.former_inputs], [_np(t) for t in c.solution[:4]]
    args = (N, st, cmd, ctrl["first_run"], params, fin, it, gw, True, gt, J, cb)
    ref, mag = R.step_vjp(*args), R.step_vjp(*args, absolute=True)
    bound = TOL_K5 + 2.0 ** -23
    worst = 0.0
    for name, g in got.items():
        g = _np(g).astype(f64).reshape(B_STEP, -1)
        assert g.dtype == f64 and _np(got[name]).dtype == f32
        err = np.linalg.norm(g - ref[name].reshape(B_STEP, -1), axis=1)
        scale = np.linalg.norm(mag[name].reshape(B_STEP, -1), axis=1)
        ratio = (err / np.maximum(scale, 1e-300)).max() / bound if np.any(scale > 0) else 0.0
        worst = max(worst, ratio)
        print(f"N={N} gait={gait} {name}: worst ||got - ref|| / ||magnitude|| = {ratio * bound:.3e} (bound {bound:.3e})")
        assert np.all(err <= bound * scale), (name, ratio)
    for name in ("dt_mpc", "residual_lin_accel", "residual_ang_accel", "rotation_body", "foot_position"):
        assert np.all(np.abs(_np(got[name]).reshape(B_STEP, -1)).max(axis=1) > 0), name  # the chain reaches every env


def test_backward_needs_a_differentiable_step():
    N = 3
    c, _ = _step_controller(N, gait=True, differentiable=False)
    c.run()
    gw = torch.ones((B_STEP, 2, 6), device="cuda")
    with pytest.raises(RuntimeError, match="differentiable"):
        c.backward(gw)
    with pytest.raises(RuntimeError, match="differentiable"):
        c.run_autograd()
    c, _ = _step_controller(N, gait=True)
    with pytest.raises(RuntimeError, match="differentiable"):  # no step yet
        c.backward(gw)
    c.cfg.keep_solution = False
    c.run()
    with pytest.raises(RuntimeError, match="keep_solution"):
        c.backward(gw)
    c.cfg.keep_solution = True
    with pytest.raises(ValueError, match="unknown field"):
        c.run_autograd(yaw_desired=c.yaw_desired)
    with pytest.raises(ValueError, match="set_gait"):
        c.run_autograd(contact_table=c.contact_table)
    c.run()
    with pytest.raises(RuntimeError, match="contact_table"):
        c.backward(gw, wrt=["contact_table"])


# ---- 5. autograd ----------------------------------------------------------------------------------

AUTOGRAD_NAMES = ("residual_lin_accel", "residual_ang_accel", "dt_mpc", "foot_position", "rotation_body")


@pytest.mark.parametrize("N", [3, 10])
def test_run_autograd_gradients_are_backwards_tensors(N):
    c, _ = _step_controller(N, gait=True)
    se = c.state_estimate_data
    src = {"residual_lin_accel": c.residual_lin_accel, "residual_ang_accel": c.residual_ang_accel, "dt_mpc": c.dt_mpc,
           "foot_position": se.foot_position, "rotation_body": se.rotation_body}
    leaves = {n: src[n].clone().requires_grad_(True) for n in AUTOGRAD_NAMES}
    w = c.run_autograd(**leaves)
    assert w.requires_grad and w.shape == (B_STEP, 2, 6) and w.data_ptr() != c.foot_wrench.data_ptr()
    assert torch.equal(w.detach(), c.foot_wrench)
    gw = torch.from_numpy(np.random.default_rng(5900 + N).standard_normal((B_STEP, 2, 6)).astype(f32)).cuda()
    want = {n: t.clone() for n, t in c.backward(gw, wrt=AUTOGRAD_NAMES).items()}
    c.run()  # a second step before the graph is differentiated: new solution, first_run cleared, knot points moved
    c.run()
    grads = torch.autograd.grad((w * gw).sum(), [leaves[n] for n in AUTOGRAD_NAMES])
    torch.cuda.synchronize()
    for n, g in zip(AUTOGRAD_NAMES, grads):
        assert g.dtype == torch.float32 and g.shape == leaves[n].shape, n
        assert torch.equal(g, want[n]), n
        assert g.abs().max() > 0, n
    # the example of the documentation: a subset of the overrides requires grad
    a_lin, dt = leaves["residual_lin_accel"], leaves["dt_mpc"]
    w2 = c.run_autograd(residual_lin_accel=a_lin, dt_mpc=dt, residual_ang_accel=src["residual_ang_accel"])
    g_lin, g_dt = torch.autograd.grad(w2.square().sum(), [a_lin, dt])
    assert g_lin.shape == a_lin.shape and g_dt.shape == dt.shape and torch.isfinite(g_lin).all()
    with pytest.raises(RuntimeError):  # once_differentiable
        w3 = c.run_autograd(dt_mpc=dt)
        (g3,) = torch.autograd.grad(w3.sum(), [dt], create_graph=True)
        torch.autograd.grad(g3.sum(), [dt])


# ---- 6. invariance --------------------------------------------------------------------------------

def test_gradients_do_not_depend_on_batch_size_position_or_stream():
    N = 10
    c, _ = _step_controller(N, gait=False)
    c.run()
    rec = c._step_record
    J, cb, gw, gt = (_cuda(a) for a in _torque(B_STEP, 6000))
    params = {"I_body": _np(c.I_body), "step_dt": rec.prep.step_dt}
    tens = dict(rec.tensors, first_run=rec.first_run_prev)
    fin, it = c.former_inputs, list(c.solution[:4])
    base = solver.mpc_step_backward(_prep_struct(tens, params, True), fin, it, gw, N, R.FIELDS, gt, J, cb)
    assert all(torch.equal(base[n], v) for n, v in c.backward(gw, gt, J, cb).items())
    idx = torch.arange(67, device="cuda") % B_STEP
    idx[66] = 0  # env 0 at position 0 and at position 66 of 67
    g = lambda t: t[idx].contiguous()  # noqa: E731
    big_t = {n: g(t) for n, t in tens.items()}
    big = solver.mpc_step_backward(_prep_struct(big_t, params, True), [g(t) for t in fin], [g(t) for t in it], g(gw), N,
                                   R.FIELDS, g(gt), g(J), g(cb))
    one_t = {n: t[5:6].contiguous() for n, t in tens.items()}
    one = solver.mpc_step_backward(_prep_struct(one_t, params, True), [t[5:6].contiguous() for t in fin],
                                   [t[5:6].contiguous() for t in it], gw[5:6].contiguous(), N, R.FIELDS,
                                   gt[5:6].contiguous(), J[5:6].contiguous(), cb[5:6].contiguous())
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        side = solver.mpc_step_backward(_prep_struct(tens, params, True), fin, it, gw, N, R.FIELDS, gt, J, cb)
    torch.cuda.synchronize()
    for n in R.FIELDS:
        assert torch.equal(big[n], base[n][idx]) and torch.equal(big[n][66], base[n][0]), n
        assert torch.equal(one[n][0], base[n][5]) and torch.equal(side[n], base[n]), n


@pytest.mark.parametrize("gait", [True, False])
def test_differentiable_changes_no_bit_of_the_step(gait):
    N = 10
    on, _ = _step_controller(N, gait, differentiable=True, K=20)
    off, _ = _step_controller(N, gait, differentiable=False, K=20)
    first = on.first_run.clone()
    for _ in range(2):
        w_on, w_off = on.run()[0], off.run()[0]
        torch.cuda.synchronize()
        assert torch.equal(w_on, w_off)
        assert torch.equal(on.world_position_desired, off.world_position_desired)
        assert torch.equal(on.yaw_desired, off.yaw_desired) and not on.first_run.any()
        assert torch.equal(on._first_run_prev, first)
        first = torch.zeros_like(first)
    for a, b in zip(on.solution, off.solution):
        assert torch.equal(a, b)
