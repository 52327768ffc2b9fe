"""NumPy FP64 references of the backward pass of the controller step's FP32 ends (TEST INFRASTRUCTURE ONLY):
the VJP of the u0 -> wrench / stance-torque tail (``wrench_vjp``), the VJP of the input preparation
(``prepare_vjp``) and their chain through the QP (``step_vjp``: wrench_vjp -> the dense refined adjoint and
``former_vjp`` of tests/_backward_ref.py -> prepare_vjp).

The forward maps are ``oracle.mpc_io.u0_wrench`` / ``stance_torque`` / ``prepare_inputs``. Their FP32 values are
widened to FP64 and the selects (first_run, stationary) are constants of the derivative, as in
csrc/mpc_io_backward.hpp. With ``absolute=True`` a function returns the same sums over the absolute values of
every term -- the *magnitude* the tests scale their FP64 bound with.
"""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64

# the 15 gradients, SRBD_PREP_GRAD_* order (include/srbd_mpc.h)
FIELDS = ("root_euler", "root_position", "root_angular_velocity_w", "root_velocity_w", "rotation_body",
          "foot_position", "desired_velocity_b", "desired_angular_velocity_b", "desired_height",
          "world_position_desired", "yaw_desired", "contact_table", "dt_mpc", "residual_lin_accel",
          "residual_ang_accel")
# former inputs each gradient reads (srbd_prep_grad_deps)
DEPS = {"root_euler": (0, 3), "root_position": (0, 3, 9), "root_angular_velocity_w": (0,), "root_velocity_w": (0,),
        "rotation_body": (3, 7, 8), "foot_position": (10, 11), "desired_velocity_b": (3,),
        "desired_angular_velocity_b": (3,), "desired_height": (3,), "world_position_desired": (3,),
        "yaw_desired": (3,), "contact_table": (12,), "dt_mpc": (3, 4), "residual_lin_accel": (15,),
        "residual_ang_accel": (16,)}
FORMER_WIDTHS = lambda N: (12, 12 * N, 12 * N, 12 * N, 1, 1, 1, 9, 9, 3, 3, 3, 2 * N, 12, 12, 3, 3)  # noqa: E731


def _w(a):  # an FP32 forward value, widened
    return np.asarray(a, f32).astype(f64)


def wrench_vjp(N, x, rotation_body, grad_wrench, grad_tau=None, J=None, contact_bool=None, absolute=False):
    """(grad_x (B, 24N), grad_rotation_body (B, 9)) of u0_wrench (and stance_torque with grad_tau)."""
    a = np.abs if absolute else (lambda v: v)
    sgn = 1.0 if absolute else -1.0
    B = np.asarray(x).shape[0]
    u = np.asarray(x, f64)[:, 12 * N:12 * N + 12].astype(f32).astype(f64)
    u[:, 6] = 0.0
    u[:, 9] = 0.0
    u = a(u)
    R = a(_w(rotation_body))
    gw = a(_w(grad_wrench).reshape(B, 12)).copy()
    if grad_tau is not None:
        add = np.einsum("bljk,blk->blj", a(_w(J)), a(_w(grad_tau)))
        gw += (add * (np.asarray(contact_bool)[:, :, None] != 0)).reshape(B, 12)
    gu = np.zeros((B, 12))
    gR = np.zeros((B, 3, 3))
    for b, src in enumerate((0, 6, 3, 9)):
        blk = gw[:, 3 * b:3 * b + 3]
        gu[:, src:src + 3] = sgn * np.einsum("bki,bi->bk", R, blk)
        gR += sgn * u[:, src:src + 3, None] * blk[:, None, :]
    gu[:, 6] = 0.0
    gu[:, 9] = 0.0
    gx = np.zeros((B, 24 * N))
    gx[:, 12 * N:12 * N + 12] = gu
    return gx, gR.reshape(B, 9)


def forward_intermediates(st, cmd):
    """(vw0, vw1, stationary) with the forward's own FP32 ops (oracle.mpc_io.prepare_inputs)."""
    Rm = np.asarray(st["rotation_body"], f32)
    vb = np.asarray(cmd["desired_velocity_b"], f32)
    vw = [(Rm[:, i, 0] * vb[:, 0] + Rm[:, i, 1] * vb[:, 1]) + Rm[:, i, 2] * vb[:, 2] for i in range(2)]
    return vw[0], vw[1], np.abs(vb[:, 0]) < f32(1e-2)


def prepare_vjp(N, st, cmd, first_run, params, g, literal=True, grad_wpd_out=None, grad_yaw_out=None,
                grad_rotation_body_direct=None, absolute=False):
    """dict field -> FP64 gradient with the field's shape. g: 17 cotangents of the former inputs ((B, width)
    or None = zero); first_run: the flag BEFORE the step; params: dt_mpc, I_body, step_dt."""
    a = np.abs if absolute else (lambda v: v)
    first = np.asarray(first_run).astype(bool)
    B = first.shape[0]
    G = [np.zeros((B, w)) if gi is None else a(np.asarray(gi, f64).reshape(B, w))
         for gi, w in zip(g, FORMER_WIDTHS(N))]
    gx = G[3].reshape(B, N, 12)
    S = gx.sum(axis=1)
    T = (np.arange(N, dtype=f64)[None, :, None] * gx).sum(axis=1)
    vw0, vw1, stat = forward_intermediates(st, cmd)
    vw0, vw1 = a(_w(vw0)), a(_w(vw1))
    R, vb = a(_w(st["rotation_body"])), a(_w(cmd["desired_velocity_b"]))
    wz = a(_w(cmd["desired_angular_velocity_b"])[:, 2])
    dt, c, Ib = a(_w(params["dt_mpc"])), abs(float(f32(params["step_dt"]))), a(_w(params["I_body"]))
    gw = np.zeros((B, 3)) if grad_wpd_out is None else a(_w(grad_wpd_out))
    gy = np.zeros(B) if grad_yaw_out is None else a(_w(grad_yaw_out))
    gyaw = S[:, 2] + gy
    gv = [dt * T[:, 3] + S[:, 9], dt * T[:, 4] + S[:, 10]]
    out = {}
    eu = G[0][:, 0:3].copy()
    eu[:, 2] += np.where(first, gyaw, 0.0)
    rp = G[0][:, 3:6] + G[9]
    for k in range(2):
        rp[:, k] += np.where(stat & ~first, 0.0, S[:, 3 + k]) + np.where(first, gw[:, k], 0.0)
    out["root_euler"], out["root_position"] = eu, rp
    out["root_angular_velocity_w"], out["root_velocity_w"] = G[0][:, 6:9].copy(), G[0][:, 9:12].copy()
    gR = np.zeros((B, 3, 3))
    gR[:, 0, :] = gv[0][:, None] * vb
    gR[:, 1, :] = gv[1][:, None] * vb
    g7 = G[7].reshape(B, 3, 3)
    gR += g7 if literal else np.swapaxes(g7, 1, 2)
    Gam = G[8].reshape(B, 3, 3)
    gR += np.einsum("bim,bmn,jn->bij", Gam, R, Ib) + np.einsum("bmi,bmn,nj->bij", Gam, R, Ib)
    if grad_rotation_body_direct is not None:
        gR += a(np.asarray(grad_rotation_body_direct, f64).reshape(B, 3, 3))
    out["rotation_body"] = gR
    out["foot_position"] = np.stack([G[10], G[11]], axis=1)
    dv = gv[0][:, None] * R[:, 0, :] + gv[1][:, None] * R[:, 1, :]
    for k in range(2):
        dv[:, k] += np.where(stat, c * S[:, 3 + k], 0.0) + c * gw[:, k]
    out["desired_velocity_b"] = dv
    dw = np.zeros((B, 3))
    dw[:, 2] = c * gyaw + dt * T[:, 2] + S[:, 8]
    out["desired_angular_velocity_b"] = dw
    out["desired_height"] = S[:, 5] + gw[:, 2]
    wpd = np.zeros((B, 3))
    for k in range(2):
        wpd[:, k] = np.where(stat & ~first, S[:, 3 + k], 0.0) + np.where(first, 0.0, gw[:, k])
    out["world_position_desired"] = wpd
    out["yaw_desired"] = np.where(first, 0.0, gyaw)
    out["contact_table"] = (G[12].reshape(B, N, 2) if literal else np.swapaxes(G[12].reshape(B, 2, N), 1, 2)).copy()
    out["dt_mpc"] = G[4][:, 0] + wz * T[:, 2] + vw0 * T[:, 3] + vw1 * T[:, 4]
    out["residual_lin_accel"], out["residual_ang_accel"] = G[15].copy(), G[16].copy()
    return out


def step_vjp(N, st, cmd, first_run, params, former_inputs, iterate, grad_wrench, literal=True, grad_tau=None,
             J=None, contact_bool=None, absolute=False):
    """The chain at the given former inputs and iterate [x, s, z, y]: wrench_vjp -> dense refined adjoint and
    former_vjp (tests/_backward_ref.py) -> prepare_vjp. absolute: the magnitude of the last map at the chain's own
    former-input cotangents, with the magnitude of the wrench's direct rotation_body term."""
    from tests import _backward_ref as br
    gx, _ = wrench_vjp(N, iterate[0], st["rotation_body"], grad_wrench, grad_tau, J, contact_bool)
    _, direct = wrench_vjp(N, iterate[0], st["rotation_body"], grad_wrench, grad_tau, J, contact_bool, absolute)
    g = br.mpc_backward_batch(N, [np.asarray(t, f64) for t in former_inputs], [np.asarray(t, f64) for t in iterate], gx)
    return prepare_vjp(N, st, cmd, first_run, params, g, literal, grad_rotation_body_direct=direct, absolute=absolute)
