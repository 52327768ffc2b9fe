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


def _tensor_ptr(t, dtype, shape, what: str, name, device: int | None = None):
    """The one check of a tensor argument: None -> None, else the device pointer of ``t`` once it is a CUDA
    tensor of ``dtype`` on the current device (launches go to its stream), contiguous, and of ``shape`` -- a
    tuple, an element count (the CusADi row layout: any shape of that many elements), or None when the
    caller reads the shape itself. ``name``: the argument's name, or its index in a list of inputs.
    ``device``: the current device's index, for a caller that looked it up once for many tensors."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
        raise TypeError(f"{what}: {_arg_name(name)} must be a CUDA {dtype} tensor")
    if t.device.index != (torch.cuda.current_device() if device is None else device):
        raise ValueError(f"{what}: {_arg_name(name)} is on {t.device}, the current device is "
                         f"cuda:{torch.cuda.current_device()}")
    if shape is not None and (t.numel() != shape if isinstance(shape, int) else tuple(t.shape) != tuple(shape)):
        expected = f"{shape} elements" if isinstance(shape, int) else f"shape {tuple(shape)}"
        raise ValueError(f"{what}: {_arg_name(name)} must have {expected}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {_arg_name(name)} must be contiguous")
    return t.data_ptr()


def _arg_name(name) -> str:
    return name if isinstance(name, str) else f"input {name}"


def _check_batch(tensors, widths, B: int, what: str) -> list:
    """float64 tensors of B rows of their width (None entries allowed) -> their pointers (None for None)."""
    dev = torch.cuda.current_device()
    return [_tensor_ptr(t, torch.float64, B * w, what, i, dev) for i, (t, w) in enumerate(zip(tensors, widths))]


def _ptrs(tensors):
    return _native.ptr_array([t.data_ptr() if t is not None else 0 for t in tensors])


def qp_former(inputs: list[torch.Tensor], N: int, outputs: list[torch.Tensor] | None = None):
    """17 former inputs -> [H, f, A, b, G, d] nonzeros (B, nnz) (srbd_constraints.py:20-81)."""
    d = Dims(N)
    B = inputs[0].shape[0]
    ins = _check_batch(inputs, d.former_in_nnz, B, "qp_former")
    if outputs is None:
        outputs = [torch.empty((B, w), dtype=torch.float64, device=inputs[0].device)
                   for w in d.former_out_nnz]
    outp = _check_batch(outputs, d.former_out_nnz, B, "qp_former outputs")
    rc = _native.lib().srbd_qp_former(N, B, _native.ptr_array(ins), _native.ptr_array(outp), _stream_ptr())
    _native.check(rc, "srbd_qp_former")
    return outputs


def _alloc_solver_outputs(B: int, N: int, device) -> list[torch.Tensor]:
    return [torch.empty((B, w), dtype=torch.float64, device=device) for w in Dims(N).solver_out_nnz]


def _pdipm(what: str, qp, start, init_mode: int, N: int, n_iter: int, y0: float, outputs, status, objective):
    """``srbd_pdipm_info`` for ``pdipm`` (init_mode 0: from the iterate, 1: cold start with y = y0) and
    ``pdipm_ccs`` (2: from x_init); ``start`` holds solver inputs 6..9. Without ``status`` and ``objective`` the
    extras struct is NULL: the entry then runs what srbd_pdipm / _cold / _ccs run."""
    d = Dims(N)
    B = qp[0].shape[0]
    ins = _check_batch(list(qp) + list(start), d.solver_in_nnz, B, what)
    obj = _tensor_ptr(objective, torch.float64, (B,), what, "objective")
    if outputs is None:
        outputs = _alloc_solver_outputs(B, N, qp[0].device)
    outp = _check_batch(outputs, d.solver_out_nnz, B, what + " outputs")
    st = _tensor_ptr(status, torch.int32, B, what, "status")
    rc = _native.lib().srbd_pdipm_info(N, n_iter, B, init_mode, float(y0), _native.ptr_array(ins),
                                       _native.ptr_array(outp), _native.solve_info(st, obj), _stream_ptr())
    _native.check(rc, "srbd_" + what)
    return outputs


def pdipm(qp: list[torch.Tensor], iterate: list[torch.Tensor] | None, N: int, n_iter: int,
          y0: float = 1.0, outputs: list[torch.Tensor] | None = None, status: torch.Tensor | None = None,
          objective: torch.Tensor | None = None):
    """Sparse PDIPM, n_iter Mehrotra iterations (sparse_pdipm_solver.py:357-534).

    qp: [Q_val, G_val, A_val, f, h, b]; iterate: [x, s, z, y] or None for the GPU caller's cold
    start (x=0, s=max(h,1), z=1, y=y0; mpc_controller_cusadi.py:138-141).
    Returns [x, s, z, y, residuals(4), mu(1)]; ``status`` (int32 (B,), optional) receives the
    per-problem status word (include/srbd_mpc.h SRBD_STATUS_*: 1 non-finite result, 2 step length at its
    floor in the last iteration, 4 general fallback taken), ``objective`` (float64 (B,), optional) the QP
    objective 0.5 x^T H x + f^T x of the returned x.
    """
    if iterate is None:
        return _pdipm("pdipm", qp, [None] * 4, 1, N, n_iter, y0, outputs, status, objective)
    return _pdipm("pdipm", qp, iterate, 0, N, n_iter, y0, outputs, status, objective)


def pdipm_ccs(qp: list[torch.Tensor], x_init: torch.Tensor, N: int, n_iter: int,
              outputs: list[torch.Tensor] | None = None, status: torch.Tensor | None = None,
              objective: torch.Tensor | None = None):
    """The reference's ``_ccs`` solver (sparse_pdipm_solver_ccs, sparse_pdipm_solver.py:4-35): n_iter
    Mehrotra iterations from x = x_init, s = max(h - G x_init, 1), z = 1, y = 0
    (initialize_pdipm_variables, :537-558). qp: [Q_val, G_val, A_val, f, h, b]; x_init (B, 24N).
    Returns [x, s, z, y, residuals(4), mu(1)] (the reference Function returns x); ``status`` and
    ``objective`` as ``pdipm``."""
    return _pdipm("pdipm_ccs", qp, [x_init, None, None, None], 2, N, n_iter, 0.0, outputs, status, objective)


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
    (``srbd_mpc_solve_fused_info``; the register-resident step kernel at every N in 2..32, the
    LDS-resident step kernel at N = 1): no QP data reaches memory, unless ``keep_qp`` (then f, b, d go to their
    ``buffers.workspace`` slots); ``False`` runs the former and the solver as two kernels with the
    full QP in the workspace (``srbd_mpc_solve``; under a non-auto solver path ``fused`` runs these two
    kernels as well). Both give the same bits. ``status`` (int32 (B,), optional) receives
    the per-problem status word, ``objective`` (float64 (B,), optional) the QP objective
    0.5 x^T H x + f^T x of the returned x -- the reference's MPC cost -- and ``objective_f32`` (float32
    (B,), optional) the same value rounded once to float32 (the controller's ``cost``); under the auto
    solver path these three need ``fused``.
    """
    d = Dims(N)
    B = former_inputs[0].shape[0]
    ins = _check_batch(former_inputs, d.former_in_nnz, B, "mpc_solve")
    obj = _tensor_ptr(objective, torch.float64, (B,), "mpc_solve", "objective")
    obj32 = _tensor_ptr(objective_f32, torch.float32, (B,), "mpc_solve", "objective_f32")
    if buffers is None or buffers.B != B or buffers.N != N:
        buffers = MPCSolveBuffers.allocate(N, B, former_inputs[0].device)
    outp = _check_batch(buffers.outputs, d.solver_out_nnz, B, "mpc_solve outputs")
    if buffers.device != former_inputs[0].device:
        raise ValueError(f"mpc_solve: buffers on {buffers.device}, inputs on {former_inputs[0].device}")
    L = _native.lib()
    # srbd_mpc_solve (no extras) only for the two-kernel form under the auto solver path; the _info entry
    # runs the fused kernel under that path and the same two kernels, with the extras, under any other
    auto = _native.current_solver_path() == 0
    two_kernels = auto and not fused
    info = _native.solve_info(_tensor_ptr(status, torch.int32, B, "mpc_solve", "status"), obj, obj32)
    if two_kernels and info is not None:
        raise ValueError("mpc_solve: status / objective with fused=False needs a non-auto solver path")
    args = (N, n_iter, B, float(y0), _native.ptr_array(ins),  # (the one fused kernel writes no QP unless asked)
            buffers.workspace.data_ptr() if (keep_qp or not (auto and fused)) else None, _native.ptr_array(outp))
    if two_kernels:
        rc = L.srbd_mpc_solve(*args, _stream_ptr())
    else:
        rc = L.srbd_mpc_solve_fused_info(*args, info, _stream_ptr())
    _native.check(rc, "srbd_mpc_solve")
    return buffers.outputs


# ---- backward pass: gradients of a loss on a solve's outputs through the QP solve and the former ----
# Every wrapper below builds a srbd_backward_seeds and calls the *_seeds entry; with grad_x alone that entry
# runs the kernels' x-only instantiation, and one seed per env the single-seed kernel.

def _optional_outputs(outputs, widths, B: int, device, what: str, M: int | None = None, want=None):
    """(B, width) outputs, or (B, M, width) for M seeds: None -> those in `want` (default all)
    allocated; a list -> its tensors, None entries stay unwritten (NULL). Returns (list, pointer array)."""
    if outputs is None:
        outputs = [torch.empty((B, w) if M is None else (B, M, w), dtype=torch.float64, device=device)
                   if want is None or i in want else None for i, w in enumerate(widths)]
    return list(outputs), _native.ptr_array(_check_batch(outputs, [(M or 1) * w for w in widths], B, what))


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
    M, shared, ptrs = 1, None, []
    for t, w, name in zip(seeds, _seed_widths(N), names):
        ptrs.append(_tensor_ptr(t, torch.float64, None if multi else B * w, what, name))
        if t is None or not multi:
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
    return _native.BackwardSeeds(*ptrs, 1 if shared else 0), M


def _pdipm_backward(what: str, multi: bool, qp, iterate, seeds, N: int, status, outputs):
    d = Dims(N)
    B = iterate[0].shape[0]
    ins = list(qp) + list(iterate)
    inp = _check_batch(ins, d.solver_in_nnz, B, what)
    if any(ins[i] is None for i in (0, 1, 2, 6, 7, 8, 9)):
        raise ValueError(f"{what}: Q_val, G_val, A_val and the iterate x, s, z, y are required")
    sd, M = _seed_struct(seeds, B, N, what, multi)
    if seeds[4] is not None and ins[3] is None:
        raise ValueError(f"{what}: grad_objective needs f (qp[3])")
    outs, outp = _optional_outputs(outputs, d.former_out_nnz, B, iterate[0].device, what + " outputs",
                                   M if multi else None)
    rc = _native.lib().srbd_pdipm_backward_seeds(N, B, M, _native.ptr_array(inp), ctypes.byref(sd), outp,
                                                 _tensor_ptr(status, torch.int32, B, what, "status"), _stream_ptr())
    _native.check(rc, "srbd_pdipm_backward_seeds")
    return outs


def pdipm_backward(qp: list, iterate: list[torch.Tensor], grad_x: torch.Tensor | None, N: int,
                   status: torch.Tensor | None = None, outputs: list | None = None, *,
                   grad_s: torch.Tensor | None = None, grad_z: torch.Tensor | None = None,
                   grad_y: torch.Tensor | None = None, grad_objective: torch.Tensor | None = None):
    """The adjoint KKT solve at ``iterate`` = [x, s, z, y] of the QP ``qp`` = [Q_val, G_val, A_val, f, h, b]
    (h, b are not read and may be None; f only with ``grad_objective``) for the seed ``grad_x`` = dL/dx
    (B, 24N) and, optionally, the cotangents of the solve's other outputs: ``grad_s`` and ``grad_z`` (B, 16N),
    ``grad_y`` (B, 14N) and ``grad_objective`` (B,), that of J = 0.5 x^T H x + f^T x. A None seed is zero: it
    gives the bits an all-zero tensor gives (``grad_x`` may be None when another is given).

    Returns [grad_H, grad_f, grad_A, grad_b, grad_G, grad_d] in qp_former's output order and CCS widths
    (every nonzero is its own parameter). ``outputs``: preallocated tensors, None entries are skipped.
    ``status`` (int32 (B,), optional): _native.STATUS_UNSUPPORTED for a QP that is not stage-invariant
    (its gradients are NaN), STATUS_NONFINITE for a non-finite adjoint. The gradient at a non-converged
    iterate is the exact derivative of the linearised KKT conditions at that iterate (as in qpth)."""
    return _pdipm_backward("pdipm_backward", False, qp, iterate, [grad_x, grad_s, grad_z, grad_y, grad_objective],
                           N, status, outputs)


def qp_former_backward(former_inputs: list[torch.Tensor], qp_grads: list, N: int, outputs: list | None = None):
    """The vector-Jacobian product of ``qp_former``: ``qp_grads`` = [grad_H, grad_f, grad_A, grad_b, grad_G,
    grad_d] (None: a zero gradient) -> the gradients of the 17 former inputs (their order and widths).
    Those of x and u (inputs 1, 2) are zero: the QP does not depend on the linearisation point.
    ``outputs``: preallocated tensors, None entries are skipped."""
    d = Dims(N)
    B = former_inputs[0].shape[0]
    ins = _check_batch(former_inputs, d.former_in_nnz, B, "qp_former_backward")
    grads = _check_batch(qp_grads, d.former_out_nnz, B, "qp_former_backward gradients")
    outs, outp = _optional_outputs(outputs, d.former_in_nnz, B, former_inputs[0].device, "qp_former_backward outputs")
    rc = _native.lib().srbd_qp_former_backward(N, B, _native.ptr_array(ins), _native.ptr_array(grads), outp,
                                               _stream_ptr())
    _native.check(rc, "srbd_qp_former_backward")
    return outs


def _input_mask(wrt) -> int:
    mask = 0
    for i in wrt:
        if not 0 <= int(i) < 17:
            raise ValueError(f"wrt: former-input index {i} outside 0..16")
        mask |= 1 << int(i)
    return mask


def _mpc_backward(what: str, multi: bool, former_inputs, iterate, seeds, N: int, wrt, status, outputs, workspace):
    d = Dims(N)
    B = former_inputs[0].shape[0]
    dev = former_inputs[0].device
    ins = _check_batch(former_inputs, d.former_in_nnz, B, what)
    it = _check_batch(list(iterate), d.solver_in_nnz[6:], B, what + " iterate")
    sd, M = _seed_struct(seeds, B, N, what, multi)
    if outputs is not None:
        wrt = [i for i, t in enumerate(outputs) if t is not None]
    want = set(range(17)) if wrt is None else {int(i) for i in wrt}
    mask = _input_mask(want)
    L = _native.lib()
    if not multi:  # the QP and all six gradients, whatever is asked for: with nothing asked for, only status is written
        n = L.srbd_mpc_backward_workspace_doubles(N, B)
    elif mask == 0:
        raise ValueError(f"{what}: no former input requested")
    else:
        n = L.srbd_mpc_backward_multi_workspace_doubles(N, B, M, mask)
    outs, outp = _optional_outputs(outputs, d.former_in_nnz, B, dev, what + " outputs", M if multi else None, want)
    workspace = _workspace(workspace, n, dev, what)
    rc = L.srbd_mpc_backward_seeds(N, B, M, _native.ptr_array(ins), _native.ptr_array(it), ctypes.byref(sd),
                                   workspace.data_ptr(), outp, _tensor_ptr(status, torch.int32, B, what, "status"),
                                   _stream_ptr())
    _native.check(rc, "srbd_mpc_backward_seeds")
    return outs


def mpc_backward(former_inputs: list[torch.Tensor], iterate: list[torch.Tensor], grad_x: torch.Tensor | None, N: int,
                 status: torch.Tensor | None = None, outputs: list | None = None,
                 workspace: torch.Tensor | None = None, *, grad_s: torch.Tensor | None = None,
                 grad_z: torch.Tensor | None = None, grad_y: torch.Tensor | None = None,
                 grad_objective: torch.Tensor | None = None):
    """qp_former -> pdipm_backward -> qp_former_backward in one call (``srbd_mpc_backward_seeds``; the bits of
    the three calls), from the former inputs, the iterate [x, s, z, y] of the solve and ``grad_x`` -- and,
    optionally, the cotangents of s, z, y and of the objective (the MPC cost), as ``pdipm_backward``. Returns
    the gradients of the 17 former inputs (``outputs``: preallocated tensors, None entries are skipped; with
    all 17 None only ``status`` is written). ``workspace``: float64,
    srbd_mpc_backward_workspace_doubles(N, B) elements (allocated when None)."""
    return _mpc_backward("mpc_backward", False, former_inputs, iterate, [grad_x, grad_s, grad_z, grad_y, grad_objective],
                         N, None, status, outputs, workspace)


# ---- several seeds at one iterate: solution Jacobians and the u0 feedback gain ----
# The KKT matrix of the adjoint system depends on the QP and the iterate only, so M seeds share one
# factorisation. Everything below is the derivative of the linearised KKT conditions at the iterate
# (DESIGN.md 6c): exact at convergence, and at a non-converged iterate the derivative of the Newton step's
# linear system, as the single-seed functions above.

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
    return _pdipm_backward("pdipm_backward_multi", True, qp, iterate,
                           [grad_x, grad_s, grad_z, grad_y, grad_objective], N, status, outputs)


def qp_former_backward_multi(former_inputs: list[torch.Tensor], qp_grads: list, N: int, outputs: list | None = None):
    """``qp_former_backward`` over seed rows: ``qp_grads`` = six (B, M, width) tensors (None: a zero
    gradient, at least one given) -> the gradients of the 17 former inputs, each (B, M, width); row
    [b, k] uses env b's former inputs and has the bits of the single-seed call on that row.
    ``outputs``: preallocated tensors, None entries are skipped."""
    what = "qp_former_backward_multi"
    d = Dims(N)
    B = former_inputs[0].shape[0]
    ins = _check_batch(former_inputs, d.former_in_nnz, B, what)
    given = [(g, w) for g, w in zip(qp_grads, d.former_out_nnz) if g is not None]
    if not given:
        raise ValueError(f"{what}: at least one QP gradient is needed (it carries the seed count)")
    g0, w0 = given[0]
    if g0.dim() != 3 or g0.shape[0] != B or g0.shape[2] != w0 or g0.shape[1] < 1:
        raise ValueError(f"{what}: gradients must be ({B}, M, width), got {tuple(g0.shape)}")
    M = g0.shape[1]
    grads = _check_batch(qp_grads, [M * w for w in d.former_out_nnz], B, what + " gradients")
    outs, outp = _optional_outputs(outputs, d.former_in_nnz, B, former_inputs[0].device, what + " outputs", M)
    rc = _native.lib().srbd_qp_former_backward_multi(N, B, M, _native.ptr_array(ins), _native.ptr_array(grads), outp,
                                                     _stream_ptr())
    _native.check(rc, "srbd_qp_former_backward_multi")
    return outs


def mpc_backward_multi(former_inputs: list[torch.Tensor], iterate: list[torch.Tensor], grad_x: torch.Tensor | None,
                       N: int, wrt=None, status: torch.Tensor | None = None, outputs: list | None = None,
                       workspace: torch.Tensor | None = None, *, grad_s: torch.Tensor | None = None,
                       grad_z: torch.Tensor | None = None, grad_y: torch.Tensor | None = None,
                       grad_objective: torch.Tensor | None = None):
    """qp_former (once per env) -> pdipm_backward_multi -> qp_former_backward_multi in one call
    (``srbd_mpc_backward_seeds``; the bits of the three calls), for the M seeds ``grad_x`` ((M, 24N) shared,
    or (B, M, 24N)).

    ``wrt``: the former-input indices wanted (None: all 17; at least one). Returns a list of 17 with
    (B, M, width) gradients at those indices and None elsewhere: the others are neither computed nor
    allocated, and only the QP gradients the wanted inputs read are held in the workspace
    (``srbd_mpc_backward_multi_workspace_doubles``). ``outputs``: preallocated tensors instead (None
    entries are skipped; ``wrt`` is then taken from it). ``grad_s``, ``grad_z``, ``grad_y``,
    ``grad_objective``: cotangents of the solve's other outputs, as ``pdipm_backward_multi``. The result is
    the derivative of the linearised KKT conditions at the iterate: exact at convergence."""
    return _mpc_backward("mpc_backward_multi", True, former_inputs, iterate,
                         [grad_x, grad_s, grad_z, grad_y, grad_objective], N, wrt, status, outputs, workspace)


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


class _MPCSolveOutputsFunction(torch.autograd.Function):
    """The named outputs of mpc_solve(former_inputs), among x, s, z, y and the objective: forward ``mpc_solve``,
    backward ``mpc_backward`` on the saved iterate (the adjoint KKT solve and the former's vector-Jacobian
    product) with whichever cotangents autograd supplies."""

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
    res = _MPCSolveOutputsFunction.apply(N, n_iter, float(y0), outputs, *former_inputs)
    return res[0] if outputs == ("x",) else res


# ---- backward pass of the controller step's FP32 ends (include/srbd_mpc.h: wrench cotangent -> FP32 inputs) ----

def _torque_cotangent(B: int, grad_tau, contact_jacobian, contact_bool, what: str):
    """(ndof, J pointer, contact pointer, grad_tau pointer) of the optional stance-torque cotangent."""
    if grad_tau is None:
        return 0, None, None, None
    if contact_jacobian is None or contact_bool is None:
        raise ValueError(f"{what}: grad_tau needs contact_jacobian and contact_bool")
    if grad_tau.dim() != 3 or grad_tau.shape[2] < 1:
        raise ValueError(f"{what}: grad_tau must be ({B}, 2, ndof)")
    ndof = grad_tau.shape[2]
    return (ndof, _tensor_ptr(contact_jacobian, torch.float32, (B, 2, 6, ndof), what, "contact_jacobian"),
            _tensor_ptr(contact_bool, torch.float32, (B, 2), what, "contact_bool"),
            _tensor_ptr(grad_tau, torch.float32, (B, 2, ndof), what, "grad_tau"))


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
    if grad_x is None:
        grad_x = torch.empty((B, 24 * N), dtype=torch.float64, device=x.device)
    gR = torch.empty((B, 9), dtype=torch.float64, device=x.device) if want_rotation else None
    ndof, J, cb, gt = _torque_cotangent(B, grad_tau, contact_jacobian, contact_bool, what)
    rc = _native.lib().srbd_u0_wrench_backward(
        N, B, _tensor_ptr(x, torch.float64, B * 24 * N, what, "x"),
        _tensor_ptr(rotation_body, torch.float32, (B, 3, 3), what, "rotation_body"),
        _tensor_ptr(grad_wrench, torch.float32, (B, 2, 6), what, "grad_wrench"), ndof, J, cb, gt,
        _tensor_ptr(grad_x, torch.float64, B * 24 * N, what, "grad_x"), None if gR is None else gR.data_ptr(),
        _stream_ptr())
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
    what = "prepare_inputs_backward"
    grads = _check_batch(input_grads, Dims(N).former_in_nnz, B, what)
    device = torch.device("cuda", torch.cuda.current_device())
    out, ptrs, _ = _prep_grad_outputs(B, N, wrt, device, what)
    rc = _native.lib().srbd_prepare_inputs_backward(
        N, B, ctypes.byref(prep), _native.ptr_array(grads),
        _tensor_ptr(grad_wpd_out, torch.float32, (B, 3), what, "grad_wpd_out"),
        _tensor_ptr(grad_yaw_out, torch.float32, (B,), what, "grad_yaw_out"),
        _tensor_ptr(grad_rotation_body_direct, torch.float64, B * 9, what, "grad_rotation_body_direct"), ptrs,
        _stream_ptr())
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
    ins = _check_batch(former_inputs, d.former_in_nnz, B, what)
    it = _check_batch(list(iterate), d.solver_in_nnz[6:], B, what + " iterate")
    if grad_wrench is None and grad_cost is None:
        raise ValueError(f"{what}: grad_wrench and grad_cost are both None")
    out, ptrs, mask = _prep_grad_outputs(B, N, wrt, dev, what)
    L = _native.lib()
    ndof, J, cb, gt = _torque_cotangent(B, grad_tau, contact_jacobian, contact_bool, what)
    entry = "srbd_mpc_step_backward_cost" if grad_cost is not None else "srbd_mpc_step_backward"
    workspace = _workspace(workspace, getattr(L, entry + "_workspace_doubles")(N, B, mask), dev, what)
    args = [N, B, ctypes.byref(prep), _native.ptr_array(ins), _native.ptr_array(it),
            _tensor_ptr(grad_wrench, torch.float32, (B, 2, 6), what, "grad_wrench"), ndof, J, cb, gt,
            _tensor_ptr(grad_wpd_out, torch.float32, (B, 3), what, "grad_wpd_out"),
            _tensor_ptr(grad_yaw_out, torch.float32, (B,), what, "grad_yaw_out"), workspace.data_ptr(), ptrs,
            _tensor_ptr(status, torch.int32, B, what, "status"), _stream_ptr()]
    if grad_cost is not None:  # the _cost entry takes grad_cost after grad_wrench
        args.insert(6, _tensor_ptr(grad_cost, torch.float32, (B,), what, "grad_cost"))
    _native.check(getattr(L, entry)(*args), entry)
    return out
