"""The C entries the Python layer does not call: srbd_pdipm / _cold / _ccs / _ex, srbd_mpc_solve_fused / _ex,
srbd_mpc_step / _ex, srbd_mpc_backward / _multi. The wrappers go through the most general entry of each family
(srbd_pdipm_info, srbd_mpc_solve_fused_info, srbd_mpc_step_info, srbd_mpc_backward_seeds); in C the others
forward to the same code with null extras, so each is called here directly and must give the wrapper's bits,
status words included. The aliasing is host-level: one small shape (N = 3, B = 6, K = 3, the random-gait
workload of tests/_backward_cases.py) covers it.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from biped_pympc_amd import _native, layout, solver
from tests import _backward_cases as C
from tests.test_controller import _controller, random_robot

pytestmark = pytest.mark.gpu

N, B, K, Y0 = 3, 6, 3, 1.0


def _cuda(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a[:B])).cuda() for a in arrs]


@functools.lru_cache(maxsize=None)
def _case():
    """(former inputs, QP in the solver's order, iterate after K iterations, grad_x) of the first B envs."""
    ins, qp = C.workload(N, "random")
    return _cuda(ins), _cuda(qp), _cuda(C.iterate(N, "random", K)), _cuda([C.seeds(N)[1]])[0]


def _status():
    return torch.full((B,), -1, dtype=torch.int32, device="cuda")


def _nan(widths, M=None):
    return [torch.full((B, w) if M is None else (B, M, w), float("nan"), dtype=torch.float64, device="cuda")
            for w in widths]


def _call(name, *args):
    _native.check(getattr(_native.lib(), name)(*args, solver._stream_ptr()), name)


def _same(got, want, what):
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (what, i)
        assert torch.isfinite(a).all(), (what, i)


@pytest.mark.parametrize("init_mode", [0, 1, 2])
def test_pdipm_plain_and_ex_entries_equal_the_wrapper(init_mode):
    _, qp, it, _ = _case()
    start = [list(it), [None] * 4, [it[0], None, None, None]][init_mode]
    st_w, st_ex = _status(), _status()
    if init_mode == 2:
        want = solver.pdipm_ccs(qp, it[0], N, K, status=st_w)
    else:
        want = solver.pdipm(qp, it if init_mode == 0 else None, N, K, Y0, status=st_w)
    ins = solver._ptrs(list(qp) + start)
    plain, ex = _nan(layout.Dims(N).solver_out_nnz), _nan(layout.Dims(N).solver_out_nnz)
    if init_mode == 0:
        _call("srbd_pdipm", N, K, B, ins, solver._ptrs(plain))
    elif init_mode == 1:
        _call("srbd_pdipm_cold", N, K, B, Y0, ins, solver._ptrs(plain))
    else:
        _call("srbd_pdipm_ccs", N, K, B, ins, solver._ptrs(plain))
    _call("srbd_pdipm_ex", N, K, B, init_mode, Y0, ins, solver._ptrs(ex), st_ex.data_ptr())
    _same(plain, want, "plain")
    _same(ex, want, "ex")
    assert torch.equal(st_ex, st_w) and torch.all(st_w >= 0)


def test_mpc_solve_fused_and_ex_entries_equal_the_wrapper():
    ins, _, _, _ = _case()
    st_w, st_ex = _status(), _status()
    want = [t.clone() for t in solver.mpc_solve(ins, N, K, Y0, status=st_w)]
    _same(solver.mpc_solve(ins, N, K, Y0), want, "wrapper without status")
    plain, ex = _nan(layout.Dims(N).solver_out_nnz), _nan(layout.Dims(N).solver_out_nnz)
    _call("srbd_mpc_solve_fused", N, K, B, Y0, solver._ptrs(ins), None, solver._ptrs(plain))
    _call("srbd_mpc_solve_fused_ex", N, K, B, Y0, solver._ptrs(ins), None, solver._ptrs(ex), st_ex.data_ptr())
    _same(plain, want, "plain")
    _same(ex, want, "ex")
    assert torch.equal(st_ex, st_w) and torch.all(st_w >= 0)


@pytest.mark.parametrize("entry", ["srbd_mpc_step", "srbd_mpc_step_ex"])
def test_mpc_step_and_ex_entries_equal_run(entry):
    c = _controller(B, N, *random_robot(B, 77, N, gait=True))
    c.cfg.keep_solution = True
    c.cfg.pdipm_iterations = K
    ex = entry.endswith("_ex")
    st_w, st_ex = _status(), _status()
    c.status = st_w if ex else None
    state = ("world_position_desired", "yaw_desired", "first_run")
    before = [getattr(c, n).clone() for n in state]
    wrench = c.run()[0].clone()
    want = [wrench] + [t.clone() for t in c.former_inputs + c.solution] + [getattr(c, n).clone() for n in state]
    for n, t in zip(state, before):  # the step advanced the knot-point state and cleared first_run
        getattr(c, n).copy_(t)
    keep: list = []
    prep = c._prep_struct(keep)
    d = layout.Dims(N)
    fin, outs = _nan(d.former_in_nnz), _nan(d.solver_out_nnz)
    w = torch.full((B, 2, 6), float("nan"), dtype=torch.float32, device="cuda")
    args = (N, K, B, float(c.cfg.y0), ctypes.byref(prep), solver._ptrs(fin), solver._ptrs(outs), w.data_ptr(), 0,
            None, None, None)
    _call(entry, *args, *([st_ex.data_ptr()] if ex else []))
    _same([w] + fin + outs + [getattr(c, n) for n in state], want, entry)
    if ex:
        assert torch.equal(st_ex, st_w) and torch.all(st_w >= 0)


def test_mpc_backward_entry_equals_the_wrapper():
    ins, _, it, g = _case()
    L = _native.lib()
    st_w, st_c = _status(), _status()
    want = solver.mpc_backward(ins, it, g, N, status=st_w)
    ws = torch.empty(L.srbd_mpc_backward_workspace_doubles(N, B), dtype=torch.float64, device="cuda")
    got = _nan(layout.Dims(N).former_in_nnz)
    _call("srbd_mpc_backward", N, B, solver._ptrs(ins), solver._ptrs(it), g.data_ptr(), ws.data_ptr(),
          solver._ptrs(got), st_c.data_ptr())
    _same(got, want, "srbd_mpc_backward")
    assert torch.equal(st_c, st_w) and torch.all(st_w == 0)


@pytest.mark.parametrize("shared", [True, False])
def test_mpc_backward_multi_entry_equals_the_wrapper(shared):
    ins, _, it, g = _case()
    L, M = _native.lib(), 2
    seeds = g[:M].contiguous() if shared else torch.stack([g, g.flip(0)], dim=1).contiguous()
    st_w, st_c = _status(), _status()
    want = solver.mpc_backward_multi(ins, it, seeds, N, status=st_w)
    ws = torch.empty(L.srbd_mpc_backward_multi_workspace_doubles(N, B, M, 0), dtype=torch.float64, device="cuda")
    got = _nan(layout.Dims(N).former_in_nnz, M)
    _call("srbd_mpc_backward_multi", N, B, M, solver._ptrs(ins), solver._ptrs(it), seeds.data_ptr(),
          0 if shared else M * 24 * N, ws.data_ptr(), solver._ptrs(got), st_c.data_ptr())
    _same(got, want, "srbd_mpc_backward_multi")
    assert torch.equal(st_c, st_w) and torch.all(st_w == 0)
