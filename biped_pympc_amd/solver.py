"""Torch-facing API over libsrbd_mpc.so (extended C-ABI, caller's current HIP stream).

PyTorch supplies device memory and the stream only; all arithmetic runs in the HIP kernels.
Tensors are batched row-major ``(B, nnz)`` FP64 on the GPU, exactly the CusADi layout
(reference ``biped_pympc/cusadi/src/CusadiFunction.py:71-76``).
"""
from __future__ import annotations

import ctypes

import torch

from biped_pympc_amd import _native
from biped_pympc_amd.layout import Dims


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _check_batch(tensors, widths, B: int, what: str):
    for i, (t, w) in enumerate(zip(tensors, widths)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float64:
            raise TypeError(f"{what}: input {i} must be a CUDA float64 tensor")
        if t.device.index != torch.cuda.current_device():  # launches go to the current device's stream
            raise ValueError(f"{what}: input {i} is on {t.device}, the current device is "
                             f"cuda:{torch.cuda.current_device()}")
        if t.numel() != B * w:
            raise ValueError(f"{what}: input {i} has {t.numel()} elements, expected {B}x{w}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: input {i} must be contiguous (CusADi row layout)")


def qp_former(inputs: list[torch.Tensor], N: int, outputs: list[torch.Tensor] | None = None):
    """17 former inputs -> [H, f, A, b, G, d] nonzeros (B, nnz) (srbd_constraints.py:20-81)."""
    d = Dims(N)
    B = inputs[0].shape[0]
    _check_batch(inputs, d.former_in_nnz, B, "qp_former")
    if outputs is None:
        outputs = [torch.empty((B, w), dtype=torch.float64, device=inputs[0].device)
                   for w in d.former_out_nnz]
    _check_batch(outputs, d.former_out_nnz, B, "qp_former outputs")
    L = _native.lib()
    rc = L.srbd_qp_former(N, B, _native.ptr_array([t.data_ptr() for t in inputs]),
                          _native.ptr_array([t.data_ptr() for t in outputs]), _stream_ptr())
    _native.check(rc, "srbd_qp_former")
    return outputs


def _check_status(status, B: int, what: str):
    """status: None, or an int32 (B,) CUDA tensor on the current device for the per-problem status
    word (include/srbd_mpc.h SRBD_STATUS_*: 1 non-finite result, 2 step length at its floor in the
    last iteration, 4 general fallback taken)."""
    if status is None:
        return None
    if (not status.is_cuda or status.dtype != torch.int32 or status.numel() != B or not status.is_contiguous()
            or status.device.index != torch.cuda.current_device()):
        raise ValueError(f"{what}: status must be a contiguous int32 CUDA tensor of {B} elements on the current device")
    return status.data_ptr()


def _check_objective(objective, B: int, what: str, dtype=torch.float64, name: str = "objective"):
    """objective: None, or a contiguous ``dtype`` (B,) CUDA tensor on the current device for the QP
    objective J = 0.5 x^T H x + f^T x of the returned x (include/srbd_mpc.h srbd_solve_info)."""
    if objective is None:
        return None
    if not isinstance(objective, torch.Tensor) or not objective.is_cuda or objective.dtype != dtype:
        raise TypeError(f"{what}: {name} must be a CUDA {dtype} tensor")
    if (objective.dim() != 1 or objective.numel() != B or not objective.is_contiguous()
            or objective.device.index != torch.cuda.current_device()):
        raise ValueError(f"{what}: {name} must be a contiguous ({B},) tensor on the current device")
    return objective.data_ptr()


def _alloc_solver_outputs(B: int, N: int, device) -> list[torch.Tensor]:
    return [torch.empty((B, w), dtype=torch.float64, device=device) for w in Dims(N).solver_out_nnz]


def pdipm(qp: list[torch.Tensor], iterate: list[torch.Tensor] | None, N: int, n_iter: int,
          y0: float = 1.0, outputs: list[torch.Tensor] | None = None, status: torch.Tensor | None = None,
          objective: torch.Tensor | None = None):
    """Sparse PDIPM, n_iter Mehrotra iterations (sparse_pdipm_solver.py:357-534).

    qp: [Q_val, G_val, A_val, f, h, b]; iterate: [x, s, z, y] or None for the GPU caller's cold
    start (x=0, s=max(h,1), z=1, y=y0; mpc_controller_cusadi.py:138-141).
    Returns [x, s, z, y, residuals(4), mu(1)]; ``status`` (int32 (B,), optional) receives the
    per-problem status word, ``objective`` (float64 (B,), optional) the QP objective
    0.5 x^T H x + f^T x of the returned x.
    """
    d = Dims(N)
    B = qp[0].shape[0]
    ins = list(qp) + (list(iterate) if iterate is not None else [None] * 4)
    _check_batch(ins, d.solver_in_nnz, B, "pdipm")
    obj = _check_objective(objective, B, "pdipm")
    if outputs is None:
        outputs = _alloc_solver_outputs(B, N, qp[0].device)
    _check_batch(outputs, d.solver_out_nnz, B, "pdipm outputs")
    L = _native.lib()
    ptrs = _native.ptr_array([t.data_ptr() if t is not None else 0 for t in ins])
    outp = _native.ptr_array([t.data_ptr() for t in outputs])
    st = _check_status(status, B, "pdipm")
    if obj is not None:
        info = _native.solve_info(st, obj)
        rc = L.srbd_pdipm_info(N, n_iter, B, 1 if iterate is None else 0, float(y0), ptrs, outp, info, _stream_ptr())
    elif st is not None:
        rc = L.srbd_pdipm_ex(N, n_iter, B, 1 if iterate is None else 0, float(y0), ptrs, outp, st, _stream_ptr())
    elif iterate is None:
        rc = L.srbd_pdipm_cold(N, n_iter, B, float(y0), ptrs, outp, _stream_ptr())
    else:
        rc = L.srbd_pdipm(N, n_iter, B, ptrs, outp, _stream_ptr())
    _native.check(rc, "srbd_pdipm")
    return outputs


def pdipm_ccs(qp: list[torch.Tensor], x_init: torch.Tensor, N: int, n_iter: int,
              outputs: list[torch.Tensor] | None = None, status: torch.Tensor | None = None,
              objective: torch.Tensor | None = None):
    """The reference's ``_ccs`` solver (sparse_pdipm_solver_ccs, sparse_pdipm_solver.py:4-35): n_iter
    Mehrotra iterations from x = x_init, s = max(h - G x_init, 1), z = 1, y = 0
    (initialize_pdipm_variables, :537-558). qp: [Q_val, G_val, A_val, f, h, b]; x_init (B, 24N).
    Returns [x, s, z, y, residuals(4), mu(1)] (the reference Function returns x); ``status`` and
    ``objective`` as ``pdipm``."""
    d = Dims(N)
    B = qp[0].shape[0]
    ins = list(qp) + [x_init, None, None, None]
    _check_batch(ins, d.solver_in_nnz, B, "pdipm_ccs")
    obj = _check_objective(objective, B, "pdipm_ccs")
    if outputs is None:
        outputs = _alloc_solver_outputs(B, N, qp[0].device)
    _check_batch(outputs, d.solver_out_nnz, B, "pdipm_ccs outputs")
    ptrs = _native.ptr_array([t.data_ptr() if t is not None else 0 for t in ins])
    outp = _native.ptr_array([t.data_ptr() for t in outputs])
    st = _check_status(status, B, "pdipm_ccs")
    if obj is not None:
        rc = _native.lib().srbd_pdipm_info(N, n_iter, B, 2, 0.0, ptrs, outp, _native.solve_info(st, obj),
                                           _stream_ptr())
    elif st is not None:
        rc = _native.lib().srbd_pdipm_ex(N, n_iter, B, 2, 0.0, ptrs, outp, st, _stream_ptr())
    else:
        rc = _native.lib().srbd_pdipm_ccs(N, n_iter, B, ptrs, outp, _stream_ptr())
    _native.check(rc, "srbd_pdipm_ccs")
    return outputs


class MPCSolveBuffers:
    """Preallocated device buffers for repeated ``mpc_solve`` calls (no allocation per step).

    ``outputs`` are allocated up front; the QP ``workspace`` (H, f, A, b, G, d: 18 KB per env at
    N = 10) only on first use -- the two-kernel form, ``keep_qp`` or ``qp_views`` -- since the fused
    step never writes it (at 8192 envs it is 148 MB of HBM the default path would hold for nothing)."""

    def __init__(self, N: int, B: int, device, outputs: list, workspace: torch.Tensor | None = None):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.N, self.B, self.device, self.outputs = N, B, dev, outputs
        self._workspace = workspace

    @classmethod
    def allocate(cls, N: int, B: int, device="cuda") -> "MPCSolveBuffers":
        return cls(N, B, device, _alloc_solver_outputs(B, N, device))

    @property
    def workspace_allocated(self) -> bool:
        return self._workspace is not None

    @property
    def workspace(self) -> torch.Tensor:
        if self._workspace is None:
            n = _native.lib().srbd_mpc_workspace_doubles(self.N, self.B)
            self._workspace = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
        return self._workspace

    def qp_views(self) -> list[torch.Tensor]:
        """[H, f, A, b, G, d] views into the workspace (filled by the former)."""
        d = Dims(self.N)
        out, o = [], 0
        for w in d.former_out_nnz:
            out.append(self.workspace[o:o + self.B * w].view(self.B, w))
            o += self.B * w
        return out


def mpc_solve(former_inputs: list[torch.Tensor], N: int, n_iter: int, y0: float = 1.0,
              buffers: MPCSolveBuffers | None = None, fused: bool = True, keep_qp: bool = False,
              status: torch.Tensor | None = None, objective: torch.Tensor | None = None,
              objective_f32: torch.Tensor | None = None):
    """qp_former + cold-started PDIPM in one stream with no host synchronisation.

    Equivalent to the GPU caller's step (mpc_controller_cusadi.py:99-169) with the Newton
    iteration count as a runtime argument. Returns [x, s, z, y, residuals, mu].
    ``fused`` (default): one kernel forms the QP in registers / LDS and solves it
    (``srbd_mpc_solve_fused``; the register-resident step kernel at every N in 2..32, the
    LDS-resident step kernel at N = 1): no QP data reaches memory, unless ``keep_qp`` (then f, b, d go to their
    ``buffers.workspace`` slots); ``False`` runs the former and the solver as two kernels with the
    full QP in the workspace. Both give the same bits. ``status`` (int32 (B,), optional) receives
    the per-problem status word, ``objective`` (float64 (B,), optional) the QP objective
    0.5 x^T H x + f^T x of the returned x -- the reference's MPC cost -- and ``objective_f32`` (float32
    (B,), optional) the same value rounded once to float32 (the controller's ``cost``).
    """
    d = Dims(N)
    B = former_inputs[0].shape[0]
    _check_batch(former_inputs, d.former_in_nnz, B, "mpc_solve")
    obj = _check_objective(objective, B, "mpc_solve")
    obj32 = _check_objective(objective_f32, B, "mpc_solve", torch.float32, "objective_f32")
    if buffers is None or buffers.B != B or buffers.N != N:
        buffers = MPCSolveBuffers.allocate(N, B, former_inputs[0].device)
    _check_batch(buffers.outputs, d.solver_out_nnz, B, "mpc_solve outputs")
    if buffers.device != former_inputs[0].device:
        raise ValueError(f"mpc_solve: buffers on {buffers.device}, inputs on {former_inputs[0].device}")
    L = _native.lib()
    # the fused kernel runs under the auto solver path (any horizon); otherwise the former writes the
    # whole QP into the workspace for the solver kernel
    one_kernel = fused and _native.current_solver_path() == 0
    args = (N, n_iter, B, float(y0), _native.ptr_array([t.data_ptr() for t in former_inputs]),
            buffers.workspace.data_ptr() if (keep_qp or not one_kernel) else None,
            _native.ptr_array([t.data_ptr() for t in buffers.outputs]))
    st = _check_status(status, B, "mpc_solve")
    info = _native.solve_info(None if obj is None and obj32 is None else st, obj, obj32)
    if info is not None or st is not None:  # the two-kernel form runs under the non-auto branch alike
        if not fused and one_kernel:
            raise ValueError("mpc_solve: status / objective with fused=False needs a non-auto solver path")
    if info is not None:
        rc = L.srbd_mpc_solve_fused_info(*args, info, _stream_ptr())
    elif st is not None:
        rc = L.srbd_mpc_solve_fused_ex(*args, st, _stream_ptr())
    else:
        rc = (L.srbd_mpc_solve_fused if fused else L.srbd_mpc_solve)(*args, _stream_ptr())
    _native.check(rc, "srbd_mpc_solve")
    return buffers.outputs


# ---- backward pass: gradients of a loss on a solve's outputs through the QP solve and the former ----

def _optional_outputs(outputs, widths, B: int, device, what: str, M: int | None = None, want=None):
    """(B, width) outputs, or (B, M, width) for M seeds: None -> those in `want` (default all)
    allocated; a list -> its tensors, None entries stay unwritten (NULL)."""
    if outputs is None:
        outputs = [torch.empty((B, w) if M is None else (B, M, w), dtype=torch.float64, device=device)
                   if want is None or i in want else None for i, w in enumerate(widths)]
    _check_batch(outputs, [(M or 1) * w for w in widths], B, what)
    return list(outputs)


def _ptrs(tensors):
    return _native.ptr_array([t.data_ptr() if t is not None else 0 for t in tensors])


def _require_qp_and_iterate(ins, what: str) -> None:
    if any(ins[i] is None for i in (0, 1, 2, 6, 7, 8, 9)):
        raise ValueError(f"{what}: Q_val, G_val, A_val and the iterate x, s, z, y are required")


def _workspace(workspace, n: int, device, what: str) -> torch.Tensor:
    """The caller's workspace checked against the `n` doubles the C entry asks for, or a new one."""
    if workspace is None:
        workspace = torch.empty(max(n, 1), dtype=torch.float64, device=device)
    if not workspace.is_cuda or workspace.dtype != torch.float64 or workspace.numel() < n or not workspace.is_contiguous():
        raise ValueError(f"{what}: workspace must be a contiguous CUDA float64 tensor of >= {n} elements")
    return workspace


def _seed_widths(N: int) -> tuple:
    return (24 * N, 16 * N, 16 * N, 14 * N, 1)  # x, s, z, y, objective


def _seed_struct(seeds, B: int, N: int, what: str, multi: bool):
    """The five cotangents (grad_x, grad_s, grad_z, grad_y, grad_objective; None: zero) -> (the C-ABI's
    ``srbd_backward_seeds``, M). Single form: each holds B rows of its width (grad_objective (B,) or (B, 1)).
    Multi form: every given one is (M, width), shared by every env, or (B, M, width), with one M and one
    sharing for all (grad_objective: (M, 1) or (B, M, 1))."""
    names = ["grad_" + k for k in _native.SEED_KINDS]
    if all(t is None for t in seeds):
        raise ValueError(f"{what}: no seed given ({', '.join(names)} are all None)")
    M, shared = 1, None
    for t, w, name in zip(seeds, _seed_widths(N), names):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64:
            raise TypeError(f"{what}: {name} must be a CUDA float64 tensor")
        if t.device.index != torch.cuda.current_device():
            raise ValueError(f"{what}: {name} is on {t.device}, the current device is cuda:{torch.cuda.current_device()}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if not multi:
            if t.numel() != B * w or t.shape[0] != B:
                raise ValueError(f"{what}: {name} must be ({B}, {w}), got {tuple(t.shape)}")
            continue
        if t.dim() == 2 and t.shape[1] == w and t.shape[0] >= 1:
            m_t, sh_t = t.shape[0], True
        elif t.dim() == 3 and t.shape[0] == B and t.shape[2] == w and t.shape[1] >= 1:
            m_t, sh_t = t.shape[1], False
        else:
            raise ValueError(f"{what}: {name} must be (M, {w}) (shared by every env) or ({B}, M, {w}), M >= 1, "
                             f"got {tuple(t.shape)}")
        if shared is None:
            M, shared = m_t, sh_t
        elif (m_t, sh_t) != (M, shared):
            raise ValueError(f"{what}: every seed must have the same M and the same sharing; {name} is "
                             f"{tuple(t.shape)}")
    sd = _native.BackwardSeeds(*[None if t is None else t.data_ptr() for t in seeds], 1 if shared else 0)
    return sd, M


def _only_x(seeds) -> bool:
    return seeds[0] is not None and all(t is None for t in seeds[1:])


def pdipm_backward(qp: list, iterate: list[torch.Tensor], grad_x: torch.Tensor | None, N: int,
                   status: torch.Tensor | None = None, outputs: list | None = None, *,
                   grad_s: torch.Tensor | None = None, grad_z: torch.Tensor | None = None,
                   grad_y: torch.Tensor | None = None, grad_objective: torch.Tensor | None = None):
    """The adjoint KKT solve at ``iterate`` = [x, s, z, y] of the QP ``qp`` = [Q_val, G_val, A_val, f, h, b]
    (h, b are not read and may be None; f only with ``grad_objective``) for the seed ``grad_x`` = dL/dx
    (B, 24N) and, optionally, the cotangents of the solve's other outputs: ``grad_s`` and ``grad_z`` (B, 16N),
    ``grad_y`` (B, 14N) and ``grad_objective`` (B,), that of J = 0.5 x^T H x + f^T x. A None seed is zero
    (``grad_x`` may be None when another is given); with ``grad_x`` alone the result has today's bits.

    Returns [grad_H, grad_f, grad_A, grad_b, grad_G, grad_d] in qp_former's output order and CCS widths
    (every nonzero is its own parameter). ``outputs``: preallocated tensors, None entries are skipped.
    ``status`` (int32 (B,), optional): _native.STATUS_UNSUPPORTED for a QP that is not stage-invariant
    (its gradients are NaN), STATUS_NONFINITE for a non-finite adjoint. The gradient at a non-converged
    iterate is the exact derivative of the linearised KKT conditions at that iterate (as in qpth)."""
    d = Dims(N)
    B = iterate[0].shape[0]
    seeds = [grad_x, grad_s, grad_z, grad_y, grad_objective]
    ins = list(qp) + list(iterate)
    _check_batch(ins + [grad_x], d.solver_in_nnz + (d.nz,), B, "pdipm_backward")
    _require_qp_and_iterate(ins, "pdipm_backward")
    outs = _optional_outputs(outputs, d.former_out_nnz, B, iterate[0].device, "pdipm_backward outputs")
    st = _check_status(status, B, "pdipm_backward")
    if _only_x(seeds):
        rc = _native.lib().srbd_pdipm_backward(N, B, _ptrs(ins), grad_x.data_ptr(), _ptrs(outs), st, _stream_ptr())
        _native.check(rc, "srbd_pdipm_backward")
        return outs
    sd, _ = _seed_struct(seeds, B, N, "pdipm_backward", multi=False)
    if grad_objective is not None and ins[3] is None:
        raise ValueError("pdipm_backward: grad_objective needs f (qp[3])")
    rc = _native.lib().srbd_pdipm_backward_seeds(N, B, 1, _ptrs(ins), ctypes.byref(sd), _ptrs(outs), st, _stream_ptr())
    _native.check(rc, "srbd_pdipm_backward_seeds")
    return outs


def qp_former_backward(former_inputs: list[torch.Tensor], qp_grads: list, N: int, outputs: list | None = None):
    """The vector-Jacobian product of ``qp_former``: ``qp_grads`` = [grad_H, grad_f, grad_A, grad_b, grad_G,
    grad_d] (None: a zero gradient) -> the gradients of the 17 former inputs (their order and widths).
    Those of x and u (inputs 1, 2) are zero: the QP does not depend on the linearisation point.
    ``outputs``: preallocated tensors, None entries are skipped."""
    d = Dims(N)
    B = former_inputs[0].shape[0]
    _check_batch(former_inputs, d.former_in_nnz, B, "qp_former_backward")
    _check_batch(qp_grads, d.former_out_nnz, B, "qp_former_backward gradients")
    outs = _optional_outputs(outputs, d.former_in_nnz, B, former_inputs[0].device, "qp_former_backward outputs")
    rc = _native.lib().srbd_qp_former_backward(N, B, _ptrs(former_inputs), _ptrs(qp_grads), _ptrs(outs),
                                               _stream_ptr())
    _native.check(rc, "srbd_qp_former_backward")
    return outs


def mpc_backward(former_inputs: list[torch.Tensor], iterate: list[torch.Tensor], grad_x: torch.Tensor | None, N: int,
                 status: torch.Tensor | None = None, outputs: list | None = None,
                 workspace: torch.Tensor | None = None, *, grad_s: torch.Tensor | None = None,
                 grad_z: torch.Tensor | None = None, grad_y: torch.Tensor | None = None,
                 grad_objective: torch.Tensor | None = None):
    """``srbd_mpc_backward``: qp_former -> pdipm_backward -> qp_former_backward in one call (same bits),
    from the former inputs, the iterate [x, s, z, y] of the solve and ``grad_x`` -- and, optionally, the
    cotangents of s, z, y and of the objective (the MPC cost), as ``pdipm_backward``. Returns the gradients of
    the 17 former inputs (``outputs``: preallocated tensors, None entries are skipped). ``workspace``:
    float64, srbd_mpc_backward_workspace_doubles(N, B) elements (allocated when None)."""
    d = Dims(N)
    B = former_inputs[0].shape[0]
    dev = former_inputs[0].device
    seeds = [grad_x, grad_s, grad_z, grad_y, grad_objective]
    _check_batch(former_inputs, d.former_in_nnz, B, "mpc_backward")
    _check_batch(list(iterate) + [grad_x], d.solver_in_nnz[6:] + (d.nz,), B, "mpc_backward iterate")
    outs = _optional_outputs(outputs, d.former_in_nnz, B, dev, "mpc_backward outputs")
    L = _native.lib()
    workspace = _workspace(workspace, L.srbd_mpc_backward_workspace_doubles(N, B), dev, "mpc_backward")
    st = _check_status(status, B, "mpc_backward")
    if _only_x(seeds):
        rc = L.srbd_mpc_backward(N, B, _ptrs(former_inputs), _ptrs(iterate), grad_x.data_ptr(), workspace.data_ptr(),
                                 _ptrs(outs), st, _stream_ptr())
        _native.check(rc, "srbd_mpc_backward")
        return outs
    sd, _ = _seed_struct(seeds, B, N, "mpc_backward", multi=False)
    rc = L.srbd_mpc_backward_seeds(N, B, 1, _ptrs(former_inputs), _ptrs(iterate), ctypes.byref(sd),
                                   workspace.data_ptr(), _ptrs(outs), st, _stream_ptr())
    _native.check(rc, "srbd_mpc_backward_seeds")
    return outs


# ---- several seeds at one iterate: solution Jacobians and the u0 feedback gain ----
# The KKT matrix of the adjoint system depends on the QP and the iterate only, so M seeds share one
# factorisation (srbd_pdipm_backward_multi). Everything below is the derivative of the linearised KKT
# conditions at the iterate: exact at convergence, and at a non-converged iterate the
# derivative of the Newton step's linear system, as the single-seed entries above.

def _seed_block(grad_x: torch.Tensor, B: int, N: int, what: str):
    """grad_x (M, 24N), shared by every env, or (B, M, 24N), per env -> (M, the C-ABI's env stride)."""
    nz = 24 * N
    if not isinstance(grad_x, torch.Tensor) or not grad_x.is_cuda or grad_x.dtype != torch.float64:
        raise TypeError(f"{what}: grad_x must be a CUDA float64 tensor")
    if grad_x.device.index != torch.cuda.current_device():
        raise ValueError(f"{what}: grad_x is on {grad_x.device}, the current device is cuda:{torch.cuda.current_device()}")
    if not grad_x.is_contiguous():
        raise ValueError(f"{what}: grad_x must be contiguous")
    if grad_x.dim() == 2 and grad_x.shape[1] == nz and grad_x.shape[0] >= 1:
        return grad_x.shape[0], 0
    if grad_x.dim() == 3 and grad_x.shape[0] == B and grad_x.shape[2] == nz and grad_x.shape[1] >= 1:
        return grad_x.shape[1], grad_x.shape[1] * nz
    raise ValueError(f"{what}: grad_x must be (M, {nz}) (shared by every env) or ({B}, M, {nz}), M >= 1, "
                     f"got {tuple(grad_x.shape)}")


def pdipm_backward_multi(qp: list, iterate: list[torch.Tensor], grad_x: torch.Tensor | None, N: int,
                         status: torch.Tensor | None = None, outputs: list | None = None, *,
                         grad_s: torch.Tensor | None = None, grad_z: torch.Tensor | None = None,
                         grad_y: torch.Tensor | None = None, grad_objective: torch.Tensor | None = None):
    """``pdipm_backward`` for M seeds at one iterate with one factorisation and M solves.

    ``grad_s``, ``grad_z``, ``grad_y``, ``grad_objective``: the cotangents of the solve's other outputs, as
    ``pdipm_backward``; every given seed has the same M and the same sharing, (M, width) or (B, M, width)
    with widths 24N, 16N, 16N, 14N and 1. ``grad_x`` may be None when another is given.

    ``grad_x`` of shape (M, 24N) is shared by every env (unit seeds: no (B, M, 24N) tensor is needed);
    (B, M, 24N) is per env. Returns [grad_H, grad_f, grad_A, grad_b, grad_G, grad_d], each (B, M, width);
    row [b, k] has the bits ``pdipm_backward`` returns for env b and seed k alone. ``outputs``:
    preallocated (B, M, width) tensors, None entries are skipped. ``status`` (int32 (B,), optional):
    STATUS_UNSUPPORTED for a QP that is not stage-invariant (all its M rows are NaN), STATUS_NONFINITE
    when the adjoint of any of its seeds is non-finite. The result is the derivative of the linearised
    KKT conditions at the iterate: exact at convergence."""
    d = Dims(N)
    B = iterate[0].shape[0]
    ins = list(qp) + list(iterate)
    _check_batch(ins, d.solver_in_nnz, B, "pdipm_backward_multi")
    _require_qp_and_iterate(ins, "pdipm_backward_multi")
    seeds = [grad_x, grad_s, grad_z, grad_y, grad_objective]
    if _only_x(seeds):
        M, stride = _seed_block(grad_x, B, N, "pdipm_backward_multi")
    else:
        sd, M = _seed_struct(seeds, B, N, "pdipm_backward_multi", multi=True)
        if grad_objective is not None and ins[3] is None:
            raise ValueError("pdipm_backward_multi: grad_objective needs f (qp[3])")
    outs = _optional_outputs(outputs, d.former_out_nnz, B, iterate[0].device, "pdipm_backward_multi outputs", M)
    st = _check_status(status, B, "pdipm_backward_multi")
    if _only_x(seeds):
        rc = _native.lib().srbd_pdipm_backward_multi(N, B, M, _ptrs(ins), grad_x.data_ptr(), stride, _ptrs(outs), st,
                                                     _stream_ptr())
        _native.check(rc, "srbd_pdipm_backward_multi")
        return outs
    rc = _native.lib().srbd_pdipm_backward_seeds(N, B, M, _ptrs(ins), ctypes.byref(sd), _ptrs(outs), st, _stream_ptr())
    _native.check(rc, "srbd_pdipm_backward_seeds")
    return outs


def qp_former_backward_multi(former_inputs: list[torch.Tensor], qp_grads: list, N: int, outputs: list | None = None):
    """``qp_former_backward`` over seed rows: ``qp_grads`` = six (B, M, width) tensors (None: a zero
    gradient, at least one given) -> the gradients of the 17 former inputs, each (B, M, width); row
    [b, k] uses env b's former inputs and has the bits of the single-seed call on that row.
    ``outputs``: preallocated tensors, None entries are skipped."""
    d = Dims(N)
    B = former_inputs[0].shape[0]
    _check_batch(former_inputs, d.former_in_nnz, B, "qp_former_backward_multi")
    given = [(g, w) for g, w in zip(qp_grads, d.former_out_nnz) if g is not None]
    if not given:
        raise ValueError("qp_former_backward_multi: at least one QP gradient is needed (it carries the seed count)")
    g0, w0 = given[0]
    if g0.dim() != 3 or g0.shape[0] != B or g0.shape[2] != w0 or g0.shape[1] < 1:
        raise ValueError(f"qp_former_backward_multi: gradients must be ({B}, M, width), got {tuple(g0.shape)}")
    M = g0.shape[1]
    _check_batch(qp_grads, [M * w for w in d.former_out_nnz], B, "qp_former_backward_multi gradients")
    outs = _optional_outputs(outputs, d.former_in_nnz, B, former_inputs[0].device, "qp_former_backward_multi outputs",
                             M)
    rc = _native.lib().srbd_qp_former_backward_multi(N, B, M, _ptrs(former_inputs), _ptrs(qp_grads), _ptrs(outs),
                                                     _stream_ptr())
    _native.check(rc, "srbd_qp_former_backward_multi")
    return outs


def _input_mask(wrt) -> int:
    mask = 0
    for i in wrt:
        if not 0 <= int(i) < 17:
            raise ValueError(f"wrt: former-input index {i} outside 0..16")
        mask |= 1 << int(i)
    return mask


def mpc_backward_multi(former_inputs: list[torch.Tensor], iterate: list[torch.Tensor], grad_x: torch.Tensor | None,
                       N: int, wrt=None, status: torch.Tensor | None = None, outputs: list | None = None,
                       workspace: torch.Tensor | None = None, *, grad_s: torch.Tensor | None = None,
                       grad_z: torch.Tensor | None = None, grad_y: torch.Tensor | None = None,
                       grad_objective: torch.Tensor | None = None):
    """``srbd_mpc_backward_multi``: qp_former (once per env) -> pdipm_backward_multi -> qp_former_backward_multi
    in one call (same bits), for the M seeds ``grad_x`` ((M, 24N) shared, or (B, M, 24N)).

    ``wrt``: the former-input indices wanted (None: all 17). Returns a list of 17 with (B, M, width)
    gradients at those indices and None elsewhere: the others are neither computed nor allocated, and
    only the QP gradients the wanted inputs read are held in the workspace
    (``srbd_mpc_backward_multi_workspace_doubles``). ``outputs``: preallocated tensors instead (None
    entries are skipped; ``wrt`` is then taken from it). ``grad_s``, ``grad_z``, ``grad_y``,
    ``grad_objective``: cotangents of the solve's other outputs, as ``pdipm_backward_multi``. The result is
    the derivative of the linearised KKT conditions at the iterate: exact at convergence."""
    d = Dims(N)
    B = former_inputs[0].shape[0]
    dev = former_inputs[0].device
    _check_batch(former_inputs, d.former_in_nnz, B, "mpc_backward_multi")
    _check_batch(list(iterate), d.solver_in_nnz[6:], B, "mpc_backward_multi iterate")
    seeds = [grad_x, grad_s, grad_z, grad_y, grad_objective]
    if _only_x(seeds):
        M, stride = _seed_block(grad_x, B, N, "mpc_backward_multi")
    else:
        sd, M = _seed_struct(seeds, B, N, "mpc_backward_multi", multi=True)
    if outputs is not None:
        wrt = [i for i, t in enumerate(outputs) if t is not None]
    want = set(range(17)) if wrt is None else {int(i) for i in wrt}
    mask = _input_mask(want)
    if mask == 0:
        raise ValueError("mpc_backward_multi: no former input requested")
    outs = _optional_outputs(outputs, d.former_in_nnz, B, dev, "mpc_backward_multi outputs", M, want)
    L = _native.lib()
    workspace = _workspace(workspace, L.srbd_mpc_backward_multi_workspace_doubles(N, B, M, mask), dev,
                           "mpc_backward_multi")
    st = _check_status(status, B, "mpc_backward_multi")
    if _only_x(seeds):
        rc = L.srbd_mpc_backward_multi(N, B, M, _ptrs(former_inputs), _ptrs(iterate), grad_x.data_ptr(), stride,
                                       workspace.data_ptr(), _ptrs(outs), st, _stream_ptr())
        _native.check(rc, "srbd_mpc_backward_multi")
        return outs
    rc = L.srbd_mpc_backward_seeds(N, B, M, _ptrs(former_inputs), _ptrs(iterate), ctypes.byref(sd),
                                   workspace.data_ptr(), _ptrs(outs), st, _stream_ptr())
    _native.check(rc, "srbd_mpc_backward_seeds")
    return outs


def unit_seeds(N: int, rows, device="cuda", of: str = "x") -> torch.Tensor:
    """(len(rows), width) float64: the unit vectors of the solve's output ``of`` (x: 24N, s and z: 16N, y: 14N)
    at the indices ``rows`` (seeds shared by every env). ``of="objective"``: the (1, 1) seed 1.0, ``rows`` is
    ignored."""
    if of not in _native.SEED_KINDS:
        raise ValueError(f"of: one of {', '.join(_native.SEED_KINDS)}, got {of!r}")
    if of == "objective":
        return torch.ones((1, 1), dtype=torch.float64, device=device)
    w = _seed_widths(N)[_native.SEED_KINDS.index(of)]
    rows = [int(r) for r in rows]
    if not rows or any(not 0 <= r < w for r in rows):
        raise ValueError(f"rows: at least one index into {of}, each in 0..{w - 1}")
    g = torch.zeros((len(rows), w), dtype=torch.float64, device=device)
    g[torch.arange(len(rows), device=device), torch.tensor(rows, device=device)] = 1.0
    return g


def mpc_jacobian(former_inputs: list[torch.Tensor], iterate: list[torch.Tensor], N: int, rows, wrt,
                 status: torch.Tensor | None = None, seeds: torch.Tensor | None = None,
                 outputs: list | None = None, workspace: torch.Tensor | None = None, of: str = "x"):
    """Jacobians of solution components: for each former-input index in ``wrt``, (B, len(rows), width) =
    d x[rows] / d input (a list of 17, None elsewhere). ``rows`` are indices into x (24N: the states
    x_1..x_N, then the inputs u_0..u_{N-1}). One factorisation per env and len(rows) solves, with unit
    seeds shared by every env (``seeds``: ``unit_seeds(N, rows)`` kept by the caller, e.g. for graph
    capture). ``of``: the output differentiated, one of x, s, z, y, objective -- ``rows`` index into it
    (s and z: 16N, y: 14N); ``of="objective"`` ignores ``rows`` and returns (B, 1, width), the gradient of the
    MPC cost. The Jacobian is that of the linearised KKT conditions at the iterate: exact at
    convergence."""
    if of not in _native.SEED_KINDS:
        raise ValueError(f"mpc_jacobian: of must be one of {', '.join(_native.SEED_KINDS)}, got {of!r}")
    n_rows = 1 if of == "objective" else len(list(rows))
    if seeds is None:
        seeds = unit_seeds(N, rows, former_inputs[0].device, of)
    elif seeds.dim() != 2 or seeds.shape[0] != n_rows:
        raise ValueError("mpc_jacobian: seeds must be unit_seeds(N, rows, of=of)")
    kw = {} if of == "x" else {"grad_" + of: seeds}
    return mpc_backward_multi(former_inputs, iterate, seeds if of == "x" else None, N, wrt=wrt, status=status,
                              outputs=outputs, workspace=workspace, **kw)


def mpc_feedback_gain(former_inputs: list[torch.Tensor], iterate: list[torch.Tensor], N: int,
                      status: torch.Tensor | None = None, seeds: torch.Tensor | None = None,
                      out: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """The first-order feedback gain K = d u0 / d x0, (B, 12, 12) with K[b, i, j] = d u0_i / d x0_j in the
    QP's own coordinates: between two MPC solves the caller can apply u ~ u0 + K (x - x0) at the control
    rate. Twelve unit seeds on the u0 block, one factorisation per env; only grad_b is materialised
    (12 * 14N doubles per env next to the QP). K is the derivative of the linearised KKT conditions at the
    iterate, so the gain is exact at convergence. ``seeds`` (``unit_seeds(N, range(12N,
    12N + 12))``), ``out`` (B, 12, 12) and ``workspace`` may be preallocated (graph capture)."""
    outs = [None] * 17
    outs[0] = out if out is not None else torch.empty((former_inputs[0].shape[0], 12, 12), dtype=torch.float64,
                                                      device=former_inputs[0].device)
    return mpc_jacobian(former_inputs, iterate, N, range(12 * N, 12 * N + 12), [0], status=status, seeds=seeds,
                        outputs=outs, workspace=workspace)[0]


class _MPCSolveFunction(torch.autograd.Function):
    """x = mpc_solve(former_inputs): forward ``srbd_mpc_solve_fused``, backward ``srbd_mpc_backward`` on the
    saved iterate (the adjoint KKT solve and the former's vector-Jacobian product)."""

    @staticmethod
    def forward(ctx, N, n_iter, y0, *former_inputs):
        ins = [t.detach().contiguous() for t in former_inputs]
        x, s, z, y = mpc_solve(ins, N, n_iter, y0)[:4]
        ctx.N = N
        ctx.shapes = [t.shape for t in former_inputs]
        ctx.save_for_backward(*ins, x, s, z, y)
        return x.clone()  # the saved x stays what the backward pass linearises at

    @staticmethod
    def backward(ctx, grad_x):
        saved = ctx.saved_tensors
        ins, iterate = list(saved[:17]), list(saved[17:])
        d = Dims(ctx.N)
        B = ins[0].shape[0]
        need = ctx.needs_input_grad[3:]
        outs = [torch.empty((B, w), dtype=torch.float64, device=grad_x.device) if n else None
                for w, n in zip(d.former_in_nnz, need)]
        mpc_backward(ins, iterate, grad_x.contiguous(), ctx.N, outputs=outs)
        return (None, None, None) + tuple(o.view(s) if o is not None else None for o, s in zip(outs, ctx.shapes))


class _MPCSolveOutputsFunction(torch.autograd.Function):
    """The named outputs of mpc_solve(former_inputs), among x, s, z, y and the objective: forward ``srbd_mpc_solve_fused`` (``_info`` for the objective),
    backward ``srbd_mpc_backward`` / ``srbd_mpc_backward_seeds`` on the saved iterate (the adjoint KKT solve and
    the former's vector-Jacobian product) with whichever cotangents autograd supplies."""

    @staticmethod
    def forward(ctx, N, n_iter, y0, outputs, *former_inputs):
        ins = [t.detach().contiguous() for t in former_inputs]
        B = ins[0].shape[0]
        J = torch.empty(B, dtype=torch.float64, device=ins[0].device) if "objective" in outputs else None
        x, s, z, y = mpc_solve(ins, N, n_iter, y0, objective=J)[:4]
        ctx.N = N
        ctx.outputs = outputs
        ctx.shapes = [t.shape for t in former_inputs]
        ctx.save_for_backward(*ins, x, s, z, y)
        ctx.set_materialize_grads(False)  # an unused output's cotangent stays None: a NULL seed
        res = {"x": x, "s": s, "z": z, "y": y}
        # copies: the saved iterate stays what the backward pass linearises at
        return tuple(J if k == "objective" else res[k].clone() for k in outputs)

    @staticmethod
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        ins, iterate = list(saved[:17]), list(saved[17:])
        d = Dims(ctx.N)
        B = ins[0].shape[0]
        need = ctx.needs_input_grad[4:]
        seeds = {"grad_" + k: (None if g is None else g.contiguous()) for k, g in zip(ctx.outputs, grads)}
        if all(g is None for g in seeds.values()):
            return (None,) * (4 + len(ins))
        outs = [torch.empty((B, w), dtype=torch.float64, device=ins[0].device) if n else None
                for w, n in zip(d.former_in_nnz, need)]
        mpc_backward(ins, iterate, seeds.pop("grad_x", None), ctx.N, outputs=outs, **seeds)
        return (None, None, None, None) + tuple(o.view(s) if o is not None else None
                                                for o, s in zip(outs, ctx.shapes))


def mpc_solve_autograd(former_inputs: list[torch.Tensor], N: int, n_iter: int, y0: float = 1.0,
                       outputs=("x",)):
    """The differentiable MPC QP layer: ``x`` (B, 24N) of ``mpc_solve`` (qp_former + cold-started PDIPM,
    one fused kernel) as a ``torch.autograd.Function``. ``torch.autograd.grad(loss(x), inp)`` works for
    every former input that requires grad (x and u, the linearisation point, get zeros; inputs without
    ``requires_grad`` get None). ``outputs``: the default returns x alone; any other choice returns a tuple
    of the named outputs among x, s, z, y and objective (J = 0.5 x^T H x + f^T x, the MPC cost, (B,)), and
    a loss may use any of them. The gradient is that of the linearised KKT conditions at the returned
    iterate: exact at convergence, and within 0.1-1 % of finite differences of the solve at 35
    iterations."""
    outputs = tuple(outputs)
    if not outputs or len(set(outputs)) != len(outputs) or any(k not in _native.SEED_KINDS for k in outputs):
        raise ValueError(f"mpc_solve_autograd: outputs must be distinct names out of {', '.join(_native.SEED_KINDS)}")
    if outputs == ("x",):
        return _MPCSolveFunction.apply(N, n_iter, float(y0), *former_inputs)
    return _MPCSolveOutputsFunction.apply(N, n_iter, float(y0), outputs, *former_inputs)


# ---- backward pass of the controller step's FP32 ends (include/srbd_mpc.h: wrench cotangent -> FP32 inputs) ----

def _f32_arg(t, shape, what: str, name: str):
    """None, or a contiguous float32 CUDA tensor of `shape` on the current device -> its pointer."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f"{what}: {name} must be a CUDA float32 tensor")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device.index != torch.cuda.current_device():
        raise ValueError(f"{what}: {name} must be a contiguous {tuple(shape)} tensor on the current device, "
                         f"got {tuple(t.shape)} on {t.device}")
    return t.data_ptr()


def _torque_cotangent(B: int, grad_tau, contact_jacobian, contact_bool, what: str):
    """(ndof, J pointer, contact pointer, grad_tau pointer) of the optional stance-torque cotangent."""
    if grad_tau is None:
        return 0, None, None, None
    if contact_jacobian is None or contact_bool is None:
        raise ValueError(f"{what}: grad_tau needs contact_jacobian and contact_bool")
    if grad_tau.dim() != 3 or grad_tau.shape[2] < 1:
        raise ValueError(f"{what}: grad_tau must be ({B}, 2, ndof)")
    ndof = grad_tau.shape[2]
    return (ndof, _f32_arg(contact_jacobian, (B, 2, 6, ndof), what, "contact_jacobian"),
            _f32_arg(contact_bool, (B, 2), what, "contact_bool"), _f32_arg(grad_tau, (B, 2, ndof), what, "grad_tau"))


def u0_wrench_backward(x: torch.Tensor, rotation_body: torch.Tensor, grad_wrench: torch.Tensor, N: int,
                       grad_tau: torch.Tensor | None = None, contact_jacobian: torch.Tensor | None = None,
                       contact_bool: torch.Tensor | None = None, want_rotation: bool = True,
                       grad_x: torch.Tensor | None = None):
    """``srbd_u0_wrench_backward``: the VJP of the u0 -> foot wrench (-> stance torque) epilogue. ``x`` (B, 24N)
    float64 the solution, ``rotation_body`` (B, 3, 3) and ``grad_wrench`` (B, 2, 6) float32; ``grad_tau``
    (B, 2, ndof) float32 with ``contact_jacobian`` (B, 2, 6, ndof) and ``contact_bool`` (B, 2) adds the torque's
    cotangent. Returns ``(grad_x, grad_rotation_body)``: (B, 24N) float64, zero outside the u0 block and at its
    entries 6 and 9, and (B, 9) float64, the wrench's direct dependence on rotation_body (None without
    ``want_rotation``)."""
    what = "u0_wrench_backward"
    B = x.shape[0]
    _check_batch([x], [24 * N], B, what)
    if grad_x is None:
        grad_x = torch.empty((B, 24 * N), dtype=torch.float64, device=x.device)
    _check_batch([grad_x], [24 * N], B, what + " grad_x")
    gR = torch.empty((B, 9), dtype=torch.float64, device=x.device) if want_rotation else None
    ndof, J, cb, gt = _torque_cotangent(B, grad_tau, contact_jacobian, contact_bool, what)
    rc = _native.lib().srbd_u0_wrench_backward(
        N, B, x.data_ptr(), _f32_arg(rotation_body, (B, 3, 3), what, "rotation_body"),
        _f32_arg(grad_wrench, (B, 2, 6), what, "grad_wrench"), ndof, J, cb, gt, grad_x.data_ptr(),
        None if gR is None else gR.data_ptr(), _stream_ptr())
    _native.check(rc, "srbd_u0_wrench_backward")
    return grad_x, gR


def _prep_grad_outputs(B: int, N: int, wrt, device, what: str):
    """wrt: names out of _native.PREP_GRAD_NAMES -> (dict name -> new float32 tensor, pointer array of 15, mask)."""
    names = _native.PREP_GRAD_NAMES
    unknown = [n for n in wrt if n not in names]
    if unknown:
        raise ValueError(f"{what}: unknown field(s) {unknown}; known: {', '.join(names)}")
    out = {n: torch.empty((B,) + _native.prep_grad_shape(n, N), dtype=torch.float32, device=device)
           for n in names if n in wrt}
    if not out:
        raise ValueError(f"{what}: no gradient requested")
    mask = sum(1 << i for i, n in enumerate(names) if n in out)
    return out, _native.ptr_array([out[n].data_ptr() if n in out else 0 for n in names]), mask


def prepare_inputs_backward(prep, input_grads: list, N: int, B: int, wrt, grad_wpd_out: torch.Tensor | None = None,
                            grad_yaw_out: torch.Tensor | None = None,
                            grad_rotation_body_direct: torch.Tensor | None = None) -> dict:
    """``srbd_prepare_inputs_backward``: the 17 FP64 former-input cotangents (None: zero) -> float32 gradients of
    the controller tensors named in ``wrt`` (``_native.PREP_GRAD_NAMES``), as a dict. ``prep``: the
    ``_native.MPCPrep`` of the step, its ``first_run`` the flag before the step."""
    import ctypes
    what = "prepare_inputs_backward"
    _check_batch(input_grads, Dims(N).former_in_nnz, B, what)
    _check_batch([grad_rotation_body_direct], [9], B, what + " grad_rotation_body_direct")
    device = torch.device("cuda", torch.cuda.current_device())
    out, ptrs, _ = _prep_grad_outputs(B, N, wrt, device, what)
    rc = _native.lib().srbd_prepare_inputs_backward(
        N, B, ctypes.byref(prep), _ptrs(input_grads), _f32_arg(grad_wpd_out, (B, 3), what, "grad_wpd_out"),
        _f32_arg(grad_yaw_out, (B,), what, "grad_yaw_out"),
        None if grad_rotation_body_direct is None else grad_rotation_body_direct.data_ptr(), ptrs, _stream_ptr())
    _native.check(rc, "srbd_prepare_inputs_backward")
    return out


def mpc_step_backward(prep, former_inputs: list[torch.Tensor], iterate: list[torch.Tensor],
                      grad_wrench: torch.Tensor | None, N: int, wrt, grad_tau: torch.Tensor | None = None,
                      contact_jacobian: torch.Tensor | None = None, contact_bool: torch.Tensor | None = None,
                      grad_wpd_out: torch.Tensor | None = None, grad_yaw_out: torch.Tensor | None = None,
                      status: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                      grad_cost: torch.Tensor | None = None) -> dict:
    """``srbd_mpc_step_backward``: wrench VJP -> adjoint KKT solve and former VJP -> input-preparation VJP in one
    call (the bits of the three calls), from what a controller step with ``keep_solution`` wrote. Only the
    former-input cotangents the fields in ``wrt`` read are computed. ``grad_cost`` (B,) float32: the cotangent
    of the step's MPC cost (``srbd_mpc_step_backward_cost``); ``grad_wrench`` may then be None. Returns a dict
    of float32 gradients."""
    what = "mpc_step_backward"
    d = Dims(N)
    B = former_inputs[0].shape[0]
    dev = former_inputs[0].device
    _check_batch(former_inputs, d.former_in_nnz, B, what)
    _check_batch(list(iterate), d.solver_in_nnz[6:], B, what + " iterate")
    if grad_wrench is None and grad_cost is None:
        raise ValueError(f"{what}: grad_wrench and grad_cost are both None")
    out, ptrs, mask = _prep_grad_outputs(B, N, wrt, dev, what)
    L = _native.lib()
    ndof, J, cb, gt = _torque_cotangent(B, grad_tau, contact_jacobian, contact_bool, what)
    if grad_cost is not None:
        workspace = _workspace(workspace, L.srbd_mpc_step_backward_cost_workspace_doubles(N, B, mask), dev, what)
        rc = L.srbd_mpc_step_backward_cost(
            N, B, ctypes.byref(prep), _ptrs(former_inputs), _ptrs(iterate),
            _f32_arg(grad_wrench, (B, 2, 6), what, "grad_wrench"), _f32_arg(grad_cost, (B,), what, "grad_cost"),
            ndof, J, cb, gt, _f32_arg(grad_wpd_out, (B, 3), what, "grad_wpd_out"),
            _f32_arg(grad_yaw_out, (B,), what, "grad_yaw_out"), workspace.data_ptr(), ptrs,
            _check_status(status, B, what), _stream_ptr())
        _native.check(rc, "srbd_mpc_step_backward_cost")
        return out
    workspace = _workspace(workspace, L.srbd_mpc_step_backward_workspace_doubles(N, B, mask), dev, what)
    rc = L.srbd_mpc_step_backward(
        N, B, ctypes.byref(prep), _ptrs(former_inputs), _ptrs(iterate),
        _f32_arg(grad_wrench, (B, 2, 6), what, "grad_wrench"), ndof, J, cb, gt,
        _f32_arg(grad_wpd_out, (B, 3), what, "grad_wpd_out"), _f32_arg(grad_yaw_out, (B,), what, "grad_yaw_out"),
        workspace.data_ptr(), ptrs, _check_status(status, B, what), _stream_ptr())
    _native.check(rc, "srbd_mpc_step_backward")
    return out
