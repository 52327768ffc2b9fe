"""Every rejection of the forward C-ABI entries, pinned: return code and full message text.

The argument checks of libsrbd_mpc.so run before anything touches the GPU and report through
srbd_last_error(), so the table below runs without one. Other people's logs match on these texts,
the order quirks included (srbd_pdipm_cold and the argument checks shared with srbd_pdipm report as
"srbd_pdipm", the srbd_mpc_step family as "srbd_mpc_step", srbd_mpc_solve's former stage as
"srbd_qp_former", srbd_u0_wrench as "srbd_u0_wrench_torque"; srbd_pdipm_info looks at x_init before
the horizon). No row reaches a kernel launch: each is either rejected or an empty batch, which
succeeds whatever its (zero-size) buffers point to. Two cases of the issue's list have no such row:
a null in srbd_mpc_solve's output table is found only after the former has been launched, and an
empty batch of the two srbd_evaluate_* entries still records its timing events on the device.
"""
import ctypes
import math

import pytest

from biped_pympc_amd import _native

_BUF = ctypes.create_string_buffer(64)  # a non-null address; no row lets the library read it
P = ctypes.addressof(_BUF)
INVALID = 1  # hipErrorInvalidValue
INVALID_DEVICE = 101  # hipErrorInvalidDevice


_LABELS = {}  # id(argument) -> what it is, for the test ids


def T(n, null=None):
    """A table of n non-null pointers, slot `null` null (None: no null slot, "all": every slot)."""
    t = _native.ptr_array([0 if null == "all" or i == null else P for i in range(n)])
    _LABELS[id(t)] = (t, f"null[{null}]")
    return t


def prep(full=True, **fields):
    """srbd_mpc_prep with every required array set (the schedule as a contact table), or all null."""
    p = _native.MPCPrep()
    if full:
        for name in _native.STATE_FIELDS + _native.COMMAND_FIELDS + (
                "world_position_desired", "yaw_desired", "first_run", "contact_table", "dt_mpc",
                "residual_lin_accel", "residual_ang_accel"):
            setattr(p, name, P)
        p.q_len = 12
    for k, v in fields.items():
        setattr(p, k, v)
    ref = ctypes.pointer(p)
    _LABELS[id(ref)] = (ref, ("" if full else "empty") + ",".join(f"{k}:{v and 1}" for k, v in fields.items()))
    return ref


# entry -> (parameter names in the header's order, arguments no check objects to)
_PDIPM = dict(horizon=10, n_iter=5, batch=4, inputs=T(10), outputs=T(6), stream=None)
_PDIPM_INFO = dict(_PDIPM, init_mode=0, y0=1.0, info=None, status=None)
_FUSED = dict(horizon=10, n_iter=5, batch=4, y0=1.0, former_inputs=T(17), qp_workspace=P, outputs=T(6), status=None,
              info=None, stream=None)
_STEP = dict(horizon=10, n_iter=5, batch=4, y0=1.0, prep=prep(), former_inputs=T(17), outputs=T(6), foot_wrench=P,
             ndof=12, contact_jacobian=P, contact_bool=P, tau=P, status=None, info=None, stream=None)
_WRENCH = dict(horizon=10, batch=4, x=P, rotation_body=P, foot_wrench=P, ndof=12, contact_jacobian=P, contact_bool=P,
               tau=P, stream=None)
_EVAL = dict(horizon=10, n_iter=5, inputs=P, work=None, outputs=P, batch=4)
ENTRIES = {
    "srbd_qp_former": ("horizon batch inputs outputs stream", dict(_PDIPM, inputs=T(17))),
    "srbd_pdipm": ("horizon n_iter batch inputs outputs stream", _PDIPM),
    "srbd_pdipm_cold": ("horizon n_iter batch y0 inputs outputs stream", dict(_PDIPM, y0=1.0)),
    "srbd_pdipm_ccs": ("horizon n_iter batch inputs outputs stream", _PDIPM),
    "srbd_pdipm_ex": ("horizon n_iter batch init_mode y0 inputs outputs status stream", _PDIPM_INFO),
    "srbd_pdipm_info": ("horizon n_iter batch init_mode y0 inputs outputs info stream", _PDIPM_INFO),
    "srbd_mpc_solve": ("horizon n_iter batch y0 former_inputs qp_workspace outputs stream", _FUSED),
    "srbd_mpc_solve_fused": ("horizon n_iter batch y0 former_inputs qp_workspace outputs stream", _FUSED),
    "srbd_mpc_solve_fused_ex": ("horizon n_iter batch y0 former_inputs qp_workspace outputs status stream", _FUSED),
    "srbd_mpc_solve_fused_info": ("horizon n_iter batch y0 former_inputs qp_workspace outputs info stream", _FUSED),
    "srbd_mpc_step": ("horizon n_iter batch y0 prep former_inputs outputs foot_wrench ndof contact_jacobian "
                      "contact_bool tau stream", _STEP),
    "srbd_mpc_step_ex": ("horizon n_iter batch y0 prep former_inputs outputs foot_wrench ndof contact_jacobian "
                         "contact_bool tau status stream", _STEP),
    "srbd_mpc_step_info": ("horizon n_iter batch y0 prep former_inputs outputs foot_wrench ndof contact_jacobian "
                           "contact_bool tau info stream", _STEP),
    "srbd_prepare_inputs": ("horizon batch prep former_inputs stream", _STEP),
    "srbd_u0_wrench": ("horizon batch x rotation_body foot_wrench stream", _WRENCH),
    "srbd_u0_wrench_torque": ("horizon batch x rotation_body foot_wrench ndof contact_jacobian contact_bool tau "
                              "stream", _WRENCH),
    "srbd_dense_scatter": ("batch nnz rc inverse_index values dense stream",
                           dict(batch=4, nnz=8, rc=16, inverse_index=P, values=P, dense=P, stream=None)),
    "srbd_evaluate_qp_former": ("horizon inputs work outputs batch", _EVAL),
    "srbd_evaluate_pdipm": ("horizon n_iter inputs work outputs batch", _EVAL),
    "srbd_set_solver_path": ("path", {}),
    "srbd_set_refinement": ("mode", {}),
    "srbd_set_refinement_policy": ("flags w", {}),
    "srbd_set_scratch_slots": ("slots", {}),
}

OK = None  # a row that succeeds: an empty batch
ROWS = []  # (entry, what differs from the entry's good arguments, message or OK)


def rows(entry, message, *cases):
    ROWS.extend((entry, case, message) for case in cases)


def bad_scalars(entry, message, *more, base={}):
    """The cases every entry with a horizon and a batch has; `more`: its other scalars and tables."""
    rows(entry, message, *[dict(base, **c) for c in (dict(horizon=0), dict(horizon=33), dict(batch=-1), *more)])


# ---- the former ----
bad_scalars("srbd_qp_former", "srbd_qp_former: bad arguments", dict(inputs=None), dict(outputs=None),
            dict(batch=0, inputs=None), dict(batch=0, outputs=None))
rows("srbd_qp_former", "srbd_qp_former: null input", dict(inputs=T(17, 0)), dict(inputs=T(17, 16)))
rows("srbd_qp_former", "srbd_qp_former: null output", dict(outputs=T(6, 0)), dict(outputs=T(6, 5)))
rows("srbd_qp_former", OK, dict(batch=0, inputs=T(17, "all"), outputs=T(6, "all")))

# ---- the solver entries: their shared checks report as srbd_pdipm ----
def solver_rows(e, mode, last):
    """`mode`: what selects the start (init_mode of _ex / _info); `last`: the last input slot it reads."""
    bad_scalars(e, "srbd_pdipm: bad arguments", dict(n_iter=0), dict(outputs=None), base=mode)
    rows(e, "srbd_pdipm: null input", dict(mode, inputs=T(10, 0)), dict(mode, inputs=T(10, last)))
    rows(e, "srbd_pdipm: null output", dict(mode, outputs=T(6, 0)), dict(mode, outputs=T(6, 5)),
         dict(mode, inputs=T(10, 9 if last < 9 else None), outputs=T(6, 5)))  # slots past `last` are not read
    rows(e, OK, dict(mode, batch=0, inputs=T(10, "all"), outputs=T(6, "all")))


def x_init_rows(e, who, mode):
    """The CCS start: x_init (slot 6) is looked at before the horizon, n_iter and the output table ..."""
    rows(e, who + ": null x_init", dict(mode, inputs=None), dict(mode, inputs=T(10, 6)), dict(mode, inputs=T(10, "all")),
         dict(mode, horizon=40, inputs=T(10, 6)), dict(mode, horizon=40, inputs=None),
         dict(mode, n_iter=0, inputs=T(10, 6)), dict(mode, batch=0, inputs=None), dict(mode, batch=-1, inputs=None))
    # ... its slot only in a non-empty batch
    rows(e, "srbd_pdipm: bad arguments", dict(mode, batch=-1, inputs=T(10, 6)), dict(mode, horizon=40))


for e in ("srbd_pdipm", "srbd_pdipm_cold"):
    solver_rows(e, {}, 9 if e == "srbd_pdipm" else 5)  # QP + iterate (warm start), QP only (cold start)
    rows(e, "srbd_pdipm: bad arguments", dict(inputs=None))
solver_rows("srbd_pdipm_ccs", {}, 5)  # QP + x_init
x_init_rows("srbd_pdipm_ccs", "srbd_pdipm_ccs", {})
for e in ("srbd_pdipm_ex", "srbd_pdipm_info"):
    for init_mode, last in ((0, 9), (1, 5), (2, 5)):
        solver_rows(e, dict(init_mode=init_mode), last)
        if init_mode != 2:
            rows(e, "srbd_pdipm: bad arguments", dict(init_mode=init_mode, inputs=None))
    x_init_rows(e, "srbd_pdipm_info", dict(init_mode=2))
    rows(e, "srbd_pdipm_info: init_mode 0, 1 or 2", dict(init_mode=-1), dict(init_mode=3),
         dict(init_mode=3, horizon=40, inputs=None), dict(init_mode=3, batch=0))

# ---- former + solver in two launches: the stages report under their own names ----
rows("srbd_mpc_solve", "srbd_mpc_solve: bad arguments", dict(horizon=0), dict(horizon=33), dict(qp_workspace=None),
     dict(batch=0, qp_workspace=None))
rows("srbd_mpc_solve", "srbd_qp_former: bad arguments", dict(batch=-1), dict(former_inputs=None))
rows("srbd_mpc_solve", "srbd_qp_former: null input", dict(former_inputs=T(17, 0)), dict(former_inputs=T(17, 16)),
     dict(n_iter=0, former_inputs=T(17, 16)))
rows("srbd_mpc_solve", "srbd_pdipm: bad arguments", dict(batch=0, n_iter=0), dict(batch=0, outputs=None))
rows("srbd_mpc_solve", OK, dict(batch=0, former_inputs=T(17, "all"), outputs=T(6, "all")))

# ---- the fused solve (the solver path is auto): null outputs are "not written", so never rejected ----
for e in ("srbd_mpc_solve_fused", "srbd_mpc_solve_fused_ex", "srbd_mpc_solve_fused_info"):
    rows(e, "srbd_mpc_solve_fused: bad horizon", dict(horizon=0), dict(horizon=33), dict(horizon=33, n_iter=0))
    rows(e, "srbd_mpc_solve_fused: bad arguments", dict(n_iter=0), dict(batch=-1), dict(former_inputs=None),
         dict(outputs=None), dict(batch=0, former_inputs=None))
    rows(e, "srbd_mpc_solve_fused: null input", dict(former_inputs=T(17, 0)), dict(former_inputs=T(17, 16)),
         dict(former_inputs=T(17, 16), qp_workspace=None))
    rows(e, OK, dict(batch=0, former_inputs=T(17, "all"), outputs=T(6, "all"), qp_workspace=None))

# ---- the controller step ----
for e in ("srbd_mpc_step", "srbd_mpc_step_ex", "srbd_mpc_step_info"):
    rows(e, "srbd_mpc_step: bad horizon", dict(horizon=0), dict(horizon=33), dict(horizon=33, prep=None))
    rows(e, "srbd_mpc_step: bad arguments", dict(n_iter=0), dict(batch=-1), dict(prep=None), dict(ndof=0),
         dict(ndof=65), dict(batch=0, ndof=0))
    rows(e, "srbd_mpc_step: null foot_wrench / contact_jacobian / contact_bool", dict(foot_wrench=None),
         dict(contact_jacobian=None), dict(contact_bool=None), dict(foot_wrench=None, prep=prep(full=False)))
    rows(e, "srbd_mpc_step: missing array or bad q_len", dict(prep=prep(full=False)), dict(prep=prep(q_len=11)),
         dict(prep=prep(root_euler=None)), dict(prep=prep(residual_ang_accel=None)),
         dict(prep=prep(contact_table=None)), dict(prep=prep(gait_phase=P)),
         dict(prep=prep(full=False), former_inputs=T(17, 0)))
    rows(e, "srbd_mpc_step: null former_inputs entry", dict(former_inputs=T(17, 0)), dict(former_inputs=T(17, 16)),
         dict(former_inputs=T(17, 16), tau=None, ndof=0, outputs=None))
    rows(e, OK, dict(batch=0, prep=prep(full=False), former_inputs=None, outputs=None, foot_wrench=None,
                     contact_jacobian=None, contact_bool=None, tau=None, ndof=0),
         dict(batch=0, former_inputs=T(17, "all"), contact_jacobian=None))

bad_scalars("srbd_prepare_inputs", "srbd_prepare_inputs: bad arguments", dict(prep=None), dict(former_inputs=None),
            dict(batch=0, prep=None))
rows("srbd_prepare_inputs", "srbd_prepare_inputs: missing array or bad q_len", dict(prep=prep(full=False)),
     dict(prep=prep(q_len=14)), dict(prep=prep(dt_mpc=None), former_inputs=T(17, 0)))
rows("srbd_prepare_inputs", "srbd_prepare_inputs: null output", dict(former_inputs=T(17, 0)),
     dict(former_inputs=T(17, 16)))
rows("srbd_prepare_inputs", OK, dict(batch=0, prep=prep(full=False), former_inputs=T(17, "all")))

# ---- wrench / torque epilogue: both report as srbd_u0_wrench_torque ----
for e in ("srbd_u0_wrench", "srbd_u0_wrench_torque"):
    bad_scalars(e, "srbd_u0_wrench_torque: bad arguments", dict(x=None), dict(rotation_body=None),
                dict(foot_wrench=None))
    rows(e, OK, dict(batch=0, x=None, rotation_body=None, foot_wrench=None, contact_jacobian=None, contact_bool=None))
rows("srbd_u0_wrench_torque", "srbd_u0_wrench_torque: bad arguments", dict(ndof=0), dict(ndof=65),
     dict(contact_jacobian=None), dict(contact_bool=None), dict(batch=0, ndof=0))
rows("srbd_u0_wrench_torque", OK, dict(batch=0, tau=None, ndof=0, x=None))

rows("srbd_dense_scatter", "srbd_dense_scatter: bad arguments (batch <= 65535 per call)", dict(batch=-1), dict(nnz=-1),
     dict(rc=-1), dict(batch=65536), dict(inverse_index=None), dict(dense=None), dict(values=None),
     dict(batch=0, rc=-1))
rows("srbd_dense_scatter", OK, dict(batch=0, inverse_index=None, values=None, dense=None),
     dict(rc=0, inverse_index=None, values=None, dense=None), dict(batch=0, rc=0, nnz=0))

# ---- the CusADi-style blocking calls return -1.0f ----
rows("srbd_evaluate_qp_former", "srbd_evaluate_qp_former: bad horizon/batch/pointer table", dict(horizon=0),
     dict(horizon=33), dict(batch=-1), dict(inputs=None), dict(outputs=None), dict(batch=0, inputs=None))
rows("srbd_evaluate_pdipm", "srbd_evaluate_pdipm: bad horizon/n_iter/batch/pointer table", dict(horizon=0),
     dict(horizon=33), dict(n_iter=0), dict(batch=-1), dict(inputs=None), dict(outputs=None),
     dict(batch=0, outputs=None))

# ---- the per-device setters ----
rows("srbd_set_solver_path", "srbd_set_solver_path: 0 (auto), 1 (general) or 2 (LDS-resident fast)", dict(path=-1),
     dict(path=3))
rows("srbd_set_refinement", "srbd_set_refinement: 0 (ill-conditioned iterates) or 1 (every iteration)", dict(mode=-1),
     dict(mode=2))
rows("srbd_set_refinement_policy", "srbd_set_refinement_policy: unknown policy bits or a NaN threshold",
     dict(flags=1 << 30, w=1.0), dict(flags=4, w=1.0), dict(flags=0, w=math.nan))
rows("srbd_set_scratch_slots", "srbd_set_scratch_slots: slots >= 0 (0 = one per resident workgroup)", dict(slots=-1))
# accepted values, where no HIP device is current
NO_DEVICE_ROWS = [
    ("srbd_set_solver_path", dict(path=0)), ("srbd_set_solver_path", dict(path=2)),
    ("srbd_set_refinement", dict(mode=0)), ("srbd_set_refinement", dict(mode=1)),
    ("srbd_set_refinement_policy", dict(flags=1, w=1e3)), ("srbd_set_refinement_policy", dict(flags=0xFFFF03, w=0.0)),
    ("srbd_set_scratch_slots", dict(slots=0)), ("srbd_set_scratch_slots", dict(slots=8)),
]


def _call(entry, case):
    names, good = ENTRIES[entry]
    args = dict(good, **case)
    return getattr(_native.lib(), entry)(*[args[n] for n in names.split()])


def _id(row):
    return row[0] + "-" + "-".join(f"{k}={_LABELS[id(v)][1] if id(v) in _LABELS else v}" for k, v in row[1].items())


def test_the_table_covers_every_forward_entry():
    assert {r[0] for r in ROWS} == set(ENTRIES)
    for entry, case, message in ROWS:  # a row differs from the good arguments, and only an empty one succeeds
        names, good = ENTRIES[entry]
        assert case and set(case) <= set(good) | set(names.split()), (entry, case)
        if message is OK:
            assert case.get("batch") == 0 or case.get("rc") == 0, (entry, case)


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_forward_entry_rejects_or_skips_an_empty_batch(row):
    entry, case, message = row
    rc = _call(entry, case)
    if message is OK:
        assert rc == 0, _native.last_error()
    else:
        assert rc == (-1.0 if entry.startswith("srbd_evaluate") else INVALID)
        assert _native.last_error() == message + " (code 1: invalid argument)"


@pytest.mark.parametrize("row", NO_DEVICE_ROWS, ids=_id)
def test_setters_need_a_current_device(row):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is current: the setter would succeed")
    entry, case = row
    assert _call(entry, case) == INVALID_DEVICE
    assert _native.last_error() == entry + ": no current HIP device (code 101: invalid device ordinal)"


def test_workspace_sizes():
    """H, f, A, b, G, d of one QP are 24N, 24N, 122N - 24, 14N, 28N and 16N doubles; the backward
    workspace adds, per seed, the gradients the requested inputs read (x_ref: f; R: H; mask 0: all)."""
    L = _native.lib()
    for N, per_qp in ((1, 204), (10, 2256), (32, 7272)):
        assert per_qp == 24 * N + 24 * N + (122 * N - 24) + 14 * N + 28 * N + 16 * N
        for B in (0, 1, 7, 4096):
            assert L.srbd_mpc_workspace_doubles(N, B) == B * per_qp
        for B, M in ((7, 1), (5, 3)):
            assert L.srbd_mpc_backward_multi_workspace_doubles(N, B, M, 0) == B * per_qp * (1 + M)
            assert L.srbd_mpc_backward_multi_workspace_doubles(N, B, M, 1 << 3) == B * (per_qp + M * 24 * N)
            assert L.srbd_mpc_backward_multi_workspace_doubles(N, B, M, 1 << 14) == B * (per_qp + M * 24 * N)
    assert L.srbd_mpc_workspace_doubles(0, 4) == 0 and L.srbd_mpc_workspace_doubles(33, 4) == 0
    assert L.srbd_mpc_workspace_doubles(10, -1) == 0
    assert L.srbd_mpc_backward_multi_workspace_doubles(10, 4, 0, 0) == 0
