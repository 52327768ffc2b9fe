"""ctypes binding of libsrbd_mpc.so (include/srbd_mpc.h).

The HIP library is the only compute path: if it is missing this module raises; there is no CPU
or PyTorch fallback for the kernels.
"""
from __future__ import annotations

import ctypes
import os

from biped_pympc_amd.build import LIB_DIR

_LIB_NAME = "libsrbd_mpc.so"
_lib = None

_c_dp = ctypes.c_void_p  # device pointers travel as void*


class NativeLibraryMissing(RuntimeError):
    pass


def lib_path() -> str:
    # SRBD_LIB may point at a diagnostic build (scripts/phase_profile.py); default: the product lib
    return os.environ.get("SRBD_LIB") or os.path.join(LIB_DIR, _LIB_NAME)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise NativeLibraryMissing(
            f"{path} not found: build it with `python -m biped_pympc_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the SRBD-MPC kernels.")
    # torch first: it maps the HIP runtime bundled with it, which libsrbd_mpc.so then shares. Mapped the
    # other way round (build() and smoke() in one process) the process holds two HIP runtimes and the
    # library's own finds no device (every launch fails with code 100).
    import torch  # noqa: F401
    L = ctypes.CDLL(path)
    if os.environ.get("SRBD_LIB"):  # an earlier build (A/B runs): bind what it exports
        L = _Tolerant(L)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)  # a plain CDLL raises for a missing symbol; _Tolerant binds a raising stub
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


# the 15 gradients of srbd_prepare_inputs_backward in SRBD_PREP_GRAD_* order (include/srbd_mpc.h): the
# field of srbd_mpc_prep each belongs to, and its per-env shape at horizon N
PREP_GRAD_NAMES = ("root_euler", "root_position", "root_angular_velocity_w", "root_velocity_w", "rotation_body",
                   "foot_position", "desired_velocity_b", "desired_angular_velocity_b", "desired_height",
                   "world_position_desired", "yaw_desired", "contact_table", "dt_mpc", "residual_lin_accel",
                   "residual_ang_accel")


def prep_grad_shape(name: str, N: int) -> tuple:
    return {"rotation_body": (3, 3), "foot_position": (2, 3), "desired_height": (), "yaw_desired": (),
            "contact_table": (N, 2), "dt_mpc": ()}.get(name, (3,))


class _Tolerant:
    """A library handle whose missing symbols bind to a stub raising on call (SRBD_LIB pointing at a
    build from an earlier tree, for scripts/ab_bench.sh)."""

    class _Missing:
        def __init__(self, name):
            self.name = name

        def __call__(self, *a):
            raise NativeLibraryMissing(f"{self.name} is not exported by {lib_path()}")

    def __init__(self, L):
        object.__setattr__(self, "_L", L)

    def __getattr__(self, name):
        try:
            return getattr(self._L, name)
        except AttributeError:
            stub = _Tolerant._Missing(name)
            object.__setattr__(self, name, stub)
            return stub


# the leading fields of srbd_mpc_prep: the controller reads them off its state estimate and its command
STATE_FIELDS = ("root_euler", "root_position", "root_angular_velocity_w", "root_velocity_w", "rotation_body",
                "foot_position")
COMMAND_FIELDS = ("desired_velocity_b", "desired_angular_velocity_b", "desired_height")


class MPCPrep(ctypes.Structure):
    """ctypes mirror of ``srbd_mpc_prep`` (include/srbd_mpc.h); device pointers as void*."""
    _fields_ = [(n, _c_dp) for n in STATE_FIELDS + COMMAND_FIELDS + (
        "world_position_desired", "yaw_desired", "first_run", "gait_phase", "ssp_durations",
        "dsp_durations", "contact_table", "dt_mpc", "residual_lin_accel", "residual_ang_accel")] + [
        ("I_body", ctypes.c_float * 9), ("mass", ctypes.c_double), ("mu", ctypes.c_double),
        ("Q", ctypes.c_float * 13), ("q_len", ctypes.c_int), ("R", ctypes.c_float * 12),
        ("step_dt", ctypes.c_float), ("literal_layout", ctypes.c_int)]


class BackwardSeeds(ctypes.Structure):
    """ctypes mirror of ``srbd_backward_seeds`` (include/srbd_mpc.h): the cotangents of a solve's outputs,
    device pointers as void* (None: zero), and whether the seed rows are shared by every env."""
    _fields_ = [("grad_x", _c_dp), ("grad_s", _c_dp), ("grad_z", _c_dp), ("grad_y", _c_dp),
                ("grad_objective", _c_dp), ("shared", ctypes.c_int)]


SEED_KINDS = ("x", "s", "z", "y", "objective")  # the outputs of a solve a cotangent may be given on


class SolveInfo(ctypes.Structure):
    """ctypes mirror of ``srbd_solve_info`` (include/srbd_mpc.h): the per-problem extras of a solve,
    device pointers as void* (None: not computed)."""
    _fields_ = [("status", _c_dp), ("objective", _c_dp), ("objective_f32", _c_dp)]


def solve_info(status=None, objective=None, objective_f32=None):
    """A ``SolveInfo`` of the given device pointers, or None when all are None (the plain entry points)."""
    if status is None and objective is None and objective_f32 is None:
        return None
    return SolveInfo(status, objective, objective_f32)


# The C signatures lib() binds, name -> (restype, argtypes), each written out as include/srbd_mpc.h declares it
# (tests/test_native_abi.py counts the parameters against the header). I, D, Z, U: int, double, size_t,
# unsigned; V: a device pointer or the hipStream_t; A: a host array of device pointers.
_I, _D, _Z, _U, _V = ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p
_A = ctypes.POINTER(_c_dp)
_IP = ctypes.POINTER(ctypes.c_int)
_PREP, _INFO, _SEEDS = ctypes.POINTER(MPCPrep), ctypes.POINTER(SolveInfo), ctypes.POINTER(BackwardSeeds)
SIGNATURES = {
    "srbd_abi_version": (_I, []),
    "srbd_last_error": (ctypes.c_char_p, []),
    "srbd_build_id": (ctypes.c_char_p, []),
    "srbd_evaluate_qp_former": (ctypes.c_float, [_I, _V, _V, _V, _I]),
    "srbd_evaluate_pdipm": (ctypes.c_float, [_I, _I, _V, _V, _V, _I]),
    # forward: former, solver (plain / status word / extras struct), the fused solve
    "srbd_qp_former": (_I, [_I, _I, _A, _A, _V]),
    "srbd_pdipm": (_I, [_I, _I, _I, _A, _A, _V]),
    "srbd_pdipm_cold": (_I, [_I, _I, _I, _D, _A, _A, _V]),
    "srbd_pdipm_ccs": (_I, [_I, _I, _I, _A, _A, _V]),
    "srbd_pdipm_ex": (_I, [_I, _I, _I, _I, _D, _A, _A, _V, _V]),
    "srbd_pdipm_info": (_I, [_I, _I, _I, _I, _D, _A, _A, _INFO, _V]),
    "srbd_mpc_workspace_doubles": (_Z, [_I, _I]),
    "srbd_mpc_solve": (_I, [_I, _I, _I, _D, _A, _V, _A, _V]),
    "srbd_mpc_solve_fused": (_I, [_I, _I, _I, _D, _A, _V, _A, _V]),
    "srbd_mpc_solve_fused_ex": (_I, [_I, _I, _I, _D, _A, _V, _A, _V, _V]),
    "srbd_mpc_solve_fused_info": (_I, [_I, _I, _I, _D, _A, _V, _A, _INFO, _V]),
    # per-device state and host-only introspection
    "srbd_solver_lds_bytes": (_Z, [_I]),
    "srbd_set_solver_path": (_I, [_I]),
    "srbd_get_solver_path": (_I, []),
    "srbd_set_refinement": (_I, [_I]),
    "srbd_get_refinement": (_I, []),
    "srbd_set_refinement_policy": (_I, [_I, _D]),
    "srbd_prepare_device": (_I, []),
    "srbd_release_device": (_I, []),
    "srbd_set_scratch_slots": (_I, [_I]),
    "srbd_scratch_pool_bytes": (_Z, []),
    "srbd_scratch_pool_slots": (_I, []),
    "srbd_scratch_slot_bytes": (_Z, []),
    "srbd_pattern_ccs": (_I, [_I, _I, _IP, _IP]),
    # the controller step and its parts
    "srbd_prepare_inputs": (_I, [_I, _I, _PREP, _A, _V]),
    "srbd_mpc_step": (_I, [_I, _I, _I, _D, _PREP, _A, _A, _V, _I, _V, _V, _V, _V]),
    "srbd_mpc_step_ex": (_I, [_I, _I, _I, _D, _PREP, _A, _A, _V, _I, _V, _V, _V, _V, _V]),
    "srbd_mpc_step_info": (_I, [_I, _I, _I, _D, _PREP, _A, _A, _V, _I, _V, _V, _V, _INFO, _V]),
    "srbd_u0_wrench": (_I, [_I, _I, _V, _V, _V, _V]),
    "srbd_u0_wrench_torque": (_I, [_I, _I, _V, _V, _V, _I, _V, _V, _V, _V]),
    "srbd_dense_scatter": (_I, [_I, _I, _I, _V, _V, _V, _V]),
    # the backward pass: adjoint KKT solve, former VJP and their composition, for grad_x alone (one seed / M
    # seeds) and for cotangents of every output of a solve (srbd_backward_seeds)
    "srbd_pdipm_backward": (_I, [_I, _I, _A, _V, _A, _V, _V]),
    "srbd_pdipm_backward_multi": (_I, [_I, _I, _I, _A, _V, _Z, _A, _V, _V]),
    "srbd_pdipm_backward_seeds": (_I, [_I, _I, _I, _A, _SEEDS, _A, _V, _V]),
    "srbd_qp_former_backward": (_I, [_I, _I, _A, _A, _A, _V]),
    "srbd_qp_former_backward_multi": (_I, [_I, _I, _I, _A, _A, _A, _V]),
    "srbd_former_grad_deps": (_U, [_I]),
    "srbd_mpc_backward_workspace_doubles": (_Z, [_I, _I]),
    "srbd_mpc_backward_multi_workspace_doubles": (_Z, [_I, _I, _I, _U]),
    "srbd_mpc_backward": (_I, [_I, _I, _A, _A, _V, _V, _A, _V, _V]),
    "srbd_mpc_backward_multi": (_I, [_I, _I, _I, _A, _A, _V, _Z, _V, _A, _V, _V]),
    "srbd_mpc_backward_seeds": (_I, [_I, _I, _I, _A, _A, _SEEDS, _V, _A, _V, _V]),
    # the backward pass of the controller step's FP32 ends: wrench / torque VJP, input-preparation VJP, the chain
    # (the _cost entry takes grad_cost after grad_wrench)
    "srbd_u0_wrench_backward": (_I, [_I, _I, _V, _V, _V, _I, _V, _V, _V, _V, _V, _V]),
    "srbd_prepare_inputs_backward": (_I, [_I, _I, _PREP, _A, _V, _V, _V, _A, _V]),
    "srbd_prep_grad_deps": (_U, [_I]),
    "srbd_mpc_step_backward_workspace_doubles": (_Z, [_I, _I, _U]),
    "srbd_mpc_step_backward": (_I, [_I, _I, _PREP, _A, _A, _V, _I, _V, _V, _V, _V, _V, _V, _A, _V, _V]),
    "srbd_mpc_step_backward_cost_workspace_doubles": (_Z, [_I, _I, _U]),
    "srbd_mpc_step_backward_cost": (_I, [_I, _I, _PREP, _A, _A, _V, _V, _I, _V, _V, _V, _V, _V, _V, _A, _V, _V]),
}


def ptr_array(ptrs) -> ctypes.Array:
    arr_t = _c_dp * len(ptrs)
    return arr_t(*[int(p) if p else None for p in ptrs])


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().srbd_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed: {msg}")


SOLVER_PATHS = {"auto": 0, "general": 1, "lds": 2}

# per-problem status word bits (include/srbd_mpc.h SRBD_STATUS_*)
STATUS_NONFINITE, STATUS_STEP_FLOOR, STATUS_FALLBACK = 1, 2, 4
STATUS_UNSUPPORTED = 8  # backward pass: the QP is not stage-invariant, its gradients are NaN


def current_solver_path() -> int:
    """Solver path code in effect for the current HIP device (0 = auto)."""
    return lib().srbd_get_solver_path()


class solver_path:
    """Context manager selecting the solver kernels: "auto" (stage-invariant kernels -- the
    register-resident ones at N = 2..32, the LDS-resident one at N = 1 -- plus the in-launch general
    fallback for a QP that is not stage-invariant), "general" (general kernel only) or "lds" (the
    LDS-resident stage-invariant kernel at every horizon). For the HIP device current on entry; on exit
    the previous path of that device is restored. For tests/benchmarks. ``srbd_mpc_step`` (the
    one-launch controller step) ignores the path."""

    def __init__(self, path: str):
        self.code = SOLVER_PATHS[path]
        self._prev = None
        self._device = None

    def __enter__(self):
        import torch
        self._device = torch.cuda.current_device()
        self._prev = current_solver_path()
        check(lib().srbd_set_solver_path(self.code), "srbd_set_solver_path")
        return self

    def __exit__(self, *exc):
        import torch
        with torch.cuda.device(self._device):
            check(lib().srbd_set_solver_path(self._prev), "srbd_set_solver_path")


REFINEMENT_MODES = {"adaptive": 0, "every_iteration": 1}


def current_refinement() -> int:
    """Affine-refinement mode in effect for the current HIP device (0 = adaptive, the default)."""
    return lib().srbd_get_refinement()


class refinement:
    """Context manager selecting the register kernels' affine-direction refinement (srbd_set_refinement):
    "adaptive" (default: iterations with an ill-conditioned iterate) or "every_iteration" (closer to the
    FP64 floor of the reference's elimination, ~15 % slower at N = 10). For the HIP device
    current on entry; the previous mode of that device is restored on exit."""

    def __init__(self, mode: str):
        self.code = REFINEMENT_MODES[mode]
        self._prev = None
        self._device = None

    def __enter__(self):
        import torch
        self._device = torch.cuda.current_device()
        self._prev = current_refinement()
        check(lib().srbd_set_refinement(self.code), "srbd_set_refinement")
        return self

    def __exit__(self, *exc):
        import torch
        with torch.cuda.device(self._device):  # (an explicit policy before: back to mode 0)
            check(lib().srbd_set_refinement(self._prev if self._prev in (0, 1) else 0), "srbd_set_refinement")


# srbd_set_refinement_policy's word (include/srbd_mpc.h SRBD_REFINE_*)
REFINE_AFFINE_ALL = 1
REFINE_AFFINE_AT_INIT = 2  # at an iterate whose duals are all 1 (a solve's initial iterate)


def refine_affine_first(k: int) -> int:
    return (int(k) & 255) << 8


def refine_affine_last(k: int) -> int:
    return (int(k) & 255) << 16


class refinement_policy:
    """Context manager setting an explicit refinement policy (srbd_set_refinement_policy(flags, w)) on the
    current HIP device -- diagnostics and A/B campaigns (scripts/parity_fuzz.py); on exit the previous
    mode is restored (a previous explicit policy is not: it returns to its mode 0 / 1 default)."""

    def __init__(self, flags: int, w: float = 1e3):
        self.flags, self.w = int(flags), float(w)
        self._prev = None
        self._device = None

    def __enter__(self):
        import torch
        self._device = torch.cuda.current_device()
        self._prev = current_refinement()
        check(lib().srbd_set_refinement_policy(self.flags, self.w), "srbd_set_refinement_policy")
        return self

    def __exit__(self, *exc):
        import torch
        with torch.cuda.device(self._device):
            check(lib().srbd_set_refinement(self._prev if self._prev in (0, 1) else 0), "srbd_set_refinement")


def build_id() -> str:
    """Source hash the loaded libsrbd_mpc.so was built from (build.py source_hash)."""
    try:
        return lib().srbd_build_id().decode()
    except NativeLibraryMissing:
        return "unknown"


def prepare_device() -> None:
    """srbd_prepare_device() on the current HIP device: allocate the solver's per-device pool now.
    Call it before capturing a solver call in a HIP graph (the first solver call on a device
    allocates it otherwise, which a capture does not allow)."""
    check(lib().srbd_prepare_device(), "srbd_prepare_device")


def release_device() -> None:
    """srbd_release_device(): free the current device's pool (device synchronised first)."""
    check(lib().srbd_release_device(), "srbd_release_device")


def set_scratch_slots(slots: int) -> None:
    """srbd_set_scratch_slots(slots): cap the current device's pool (0 = one slot per resident
    workgroup, the default)."""
    check(lib().srbd_set_scratch_slots(int(slots)), "srbd_set_scratch_slots")


def scratch_pool() -> dict:
    """The current device's pool: {"slots", "bytes"} (0 / 0 before it is allocated)."""
    return {"slots": int(lib().srbd_scratch_pool_slots()), "bytes": int(lib().srbd_scratch_pool_bytes())}


def last_error() -> str:
    return lib().srbd_last_error().decode(errors="replace")
