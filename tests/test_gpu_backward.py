"""The backward pass on the GPU: the adjoint kernel (srbd_pdipm_backward), the former's vector-Jacobian
product (srbd_qp_former_backward), their composition (srbd_mpc_backward) and the autograd layer, against
the NumPy reference of tests/_backward_ref.py (checked against central differences on the CPU,
tests/test_backward_ref.py).

Tolerances. Adjoint kernel: the project's SOLVER_CASES for the K that produced the iterate (1e-10 / 1e-9 /
1e-7 / 1e-5) -- the backward is one solve with the forward's factorisation -- per env and per output,
norm-wise; no env is excluded. On these exact inputs a plain-FP64 NumPy restatement of the reduced
elimination (tests/_backward_cases.py reduced_floor) stays within that tolerance on every env at every
horizon run here, N = 32 included (worst, K = 1 / 5 / 10 / 20: 4.7e-12 / 4.7e-11 / 4.6e-9 / 6.3e-8 at
N <= 10, held by tests/test_backward_ref.py; 1.5e-12 / 2.4e-11 / 4.3e-10 / 3.0e-6 at N = 32), so the
tolerance needs no per-env floor. Former VJP kernel: 1e-12, the former's parity bound.
"""
import functools

import numpy as np
import pytest
import torch

from biped_pympc_amd import _native, layout, solver
from tests import _backward_cases as C
from tests import _backward_ref as br
from tests._util import rel_err_rows

pytestmark = pytest.mark.gpu


def _cuda(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in arrs]


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _dev_case(N, gait, K):
    """(QP, iterate, seeds) on the device."""
    _, qp = C.workload(N, gait)
    return _cuda(qp), _cuda(C.iterate(N, gait, K)), _cuda(C.seeds(N))


@functools.lru_cache(maxsize=None)
def _gpu_grads(N, gait, K, k):
    qp, it, sd = _dev_case(N, gait, K)
    st = torch.full((C.BATCH,), -1, dtype=torch.int32, device="cuda")
    out = solver.pdipm_backward(qp, it, sd[k], N, status=st)
    torch.cuda.synchronize()
    assert torch.all(st == 0), st
    return out


# ---- 1. the adjoint kernel against the reference ------------------------------------------------

@pytest.mark.parametrize("K,tol", C.CASES)
@pytest.mark.parametrize("gait", C.GAITS)
@pytest.mark.parametrize("N", C.HORIZONS)
def test_adjoint_kernel_matches_reference(N, gait, K, tol):
    ref = C.reference(N, gait, K)
    for k, seed in enumerate(["u0", "all"]):
        got = _gpu_grads(N, gait, K, k)
        for o, name in enumerate(C.NAMES):
            err = rel_err_rows(_np(got[o]), ref[k][o])
            print(f"N={N} {gait} K={K} seed={seed} {name}: max rel err {err.max():.3e} (env {err.argmax()}), tol {tol:.0e}")
            assert np.all(err <= tol), (seed, name, err.max(), int(err.argmax()))


# ---- 2. the entry points agree, bit for bit -----------------------------------------------------

@pytest.mark.parametrize("N", [3, 10])
def test_mpc_backward_equals_the_three_calls(N):
    K = 5
    ins_np, _ = C.workload(N, "random")
    ins = _cuda(ins_np)
    it = _cuda(C.iterate(N, "random", K))
    g = _cuda(C.seeds(N))[0]
    qp = solver.qp_former(ins, N)  # H, f, A, b, G, d
    grads = solver.pdipm_backward([qp[0], qp[4], qp[2], qp[1], qp[5], qp[3]], it, g, N)
    chain = solver.qp_former_backward(ins, grads, N)
    st = torch.full((C.BATCH,), -1, dtype=torch.int32, device="cuda")
    one = solver.mpc_backward(ins, it, g, N, status=st)
    torch.cuda.synchronize()
    assert torch.all(st == 0)
    for i in range(17):
        assert torch.equal(one[i], chain[i]), layout.FORMER_IN_NAMES[i]


# ---- 3. the former VJP kernel against the reference ---------------------------------------------

# B = 67: 17 workgroups of four envs, the last one partial (the grid tail); B = 1: three idle waves
@pytest.mark.parametrize("N,B", [(N, 16) for N in C.HORIZONS] + [(3, 67), (3, 1)])
def test_former_vjp_kernel_matches_reference(N, B):
    from biped_pympc_amd.utils.synthetic import make_workload
    wl = make_workload(B, N, seed=950 + N, random_gait=True, residuals=True)
    rng = np.random.default_rng(960 + N)
    cot = [rng.standard_normal((B, w)) for w in layout.Dims(N).former_out_nnz]
    ref = br.former_vjp_batch(N, wl.inputs, cot)
    got = solver.qp_former_backward(_cuda(wl.inputs), _cuda(cot), N)
    torch.cuda.synchronize()
    for i, name in enumerate(layout.FORMER_IN_NAMES):
        if i in (1, 2):
            assert torch.all(got[i] == 0.0), name
            continue
        err = rel_err_rows(_np(got[i]), ref[i])
        print(f"N={N} B={B} {name}: max rel err {err.max():.3e}")
        assert np.all(err <= 1e-12), (name, err.max(), int(err.argmax()))


# ---- 4. autograd ----------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [3, 10])
def test_autograd_matches_the_reference_chain(N):
    """torch.autograd.grad through mpc_solve_autograd against the reference chain at the iterate the GPU
    solve returned (K = 5: the adjoint's 1e-9 of SOLVER_CASES; the former VJP adds 1e-12)."""
    K, tol = 5, 1e-9
    ins_np, _ = C.workload(N, "random")
    want = [0, 3, 4, 13, 14, 15, 16]  # x0, x_ref, dt, Q, R, residual accelerations
    ins = _cuda(ins_np)
    for i in want:
        ins[i].requires_grad_(True)
    x = solver.mpc_solve_autograd(ins, N, K)
    rng = np.random.default_rng(970 + N)
    w = torch.from_numpy(rng.standard_normal((C.BATCH, 12))).cuda()
    loss = (x[:, 12 * N:12 * N + 12] * w).sum()
    grads = torch.autograd.grad(loss, [ins[i] for i in want])
    it = solver.mpc_solve([t.detach() for t in ins], N, K)[:4]
    torch.cuda.synchronize()
    assert torch.equal(it[0], x.detach())
    g = np.zeros((C.BATCH, 24 * N))
    g[:, 12 * N:12 * N + 12] = _np(w)
    ref = br.mpc_backward_batch(N, ins_np, [_np(t) for t in it], g)
    for i, gr in zip(want, grads):
        assert gr.shape == ins[i].shape
        err = rel_err_rows(_np(gr), ref[i])
        print(f"N={N} {layout.FORMER_IN_NAMES[i]}: max rel err {err.max():.3e}")
        assert np.all(err <= tol), (layout.FORMER_IN_NAMES[i], err.max())


def test_autograd_inputs_without_requires_grad_get_none():
    N, K = 3, 5
    ins = _cuda(C.workload(N, "random")[0])
    ins[15].requires_grad_(True)
    x = solver.mpc_solve_autograd(ins, N, K)
    x[:, 12 * N:12 * N + 12].sum().backward()
    torch.cuda.synchronize()
    assert ins[15].grad is not None and torch.isfinite(ins[15].grad).all() and ins[15].grad.abs().max() > 0
    assert all(ins[i].grad is None for i in range(17) if i != 15)
    # the Function itself hands None to every input that did not ask (and to N, n_iter, y0, outputs)

    class Ctx:
        N = 3
        outputs = ("x",)
        needs_input_grad = (False,) * 4 + tuple(i == 15 for i in range(17))
        shapes = [t.shape for t in ins]
        saved_tensors = tuple(t.detach() for t in ins) + tuple(solver.mpc_solve([t.detach() for t in ins], N, K)[:4])
    outs = solver._MPCSolveOutputsFunction.backward(Ctx, torch.ones_like(x))
    torch.cuda.synchronize()
    assert len(outs) == 21 and all(o is None for j, o in enumerate(outs) if j != 19)
    g = torch.zeros_like(x)
    g[:, 12 * N:12 * N + 12] = 1.0
    assert torch.equal(solver._MPCSolveOutputsFunction.backward(Ctx, g)[19], ins[15].grad)


# ---- 5. determinism -------------------------------------------------------------------------------

def test_gradients_do_not_depend_on_batch_size_position_or_stream():
    N, K, k = 10, 10, 1
    qp, it, sd = _dev_case(N, "random", K)
    base = _gpu_grads(N, "random", K, k)
    idx = torch.arange(67, device="cuda") % C.BATCH
    idx[66] = 0  # env 0 at position 0 and at position 66 of 67
    big = solver.pdipm_backward([t[idx].contiguous() for t in qp], [t[idx].contiguous() for t in it],
                                sd[k][idx].contiguous(), N)
    one = solver.pdipm_backward([t[:1].contiguous() for t in qp], [t[:1].contiguous() for t in it],
                                sd[k][:1].contiguous(), N)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = solver.pdipm_backward(qp, it, sd[k], N)
    with torch.cuda.stream(s2):
        b = solver.pdipm_backward(qp, it, sd[k], N)
    torch.cuda.synchronize()
    for o in range(6):
        assert torch.equal(big[o], base[o][idx]), C.NAMES[o]  # every row of the 67, the grid tail included
        assert torch.equal(big[o][66], base[o][0]) and torch.equal(one[o][0], base[o][0]), C.NAMES[o]
        assert torch.equal(a[o], base[o]) and torch.equal(b[o], base[o]), C.NAMES[o]


# ---- 6. NULL outputs --------------------------------------------------------------------------------

@pytest.mark.parametrize("keep", [(0,), (2, 3), (1, 4, 5)])
def test_null_outputs_are_skipped_and_change_no_bit_of_the_others(keep):
    N, K, k = 3, 5, 1
    qp, it, sd = _dev_case(N, "fixed", K)
    base = _gpu_grads(N, "fixed", K, k)
    outs = [torch.full_like(base[o], float("nan")) if o in keep else None for o in range(6)]
    got = solver.pdipm_backward([qp[0], qp[1], qp[2], None, None, None], it, sd[k], N, outputs=outs)  # f, h, b unread
    torch.cuda.synchronize()
    for o in range(6):
        if o in keep:
            assert torch.equal(got[o], base[o]), C.NAMES[o]
        else:
            assert got[o] is None


# ---- 7. a batch with a QP that is not stage-invariant -----------------------------------------------

def test_unsupported_qp_gets_nan_and_its_status_bit_neighbours_unchanged():
    N, K, k, bad = 3, 5, 1, 5
    qp, it, sd = _dev_case(N, "random", K)
    base = _gpu_grads(N, "random", K, k)
    H = qp[0].clone()
    H[bad, 12:24] *= 1.5  # stage 1 of the x weights: no longer stage-invariant
    st = torch.full((C.BATCH,), -1, dtype=torch.int32, device="cuda")
    got = solver.pdipm_backward([H] + qp[1:], it, sd[k], N, status=st)
    torch.cuda.synchronize()
    want = torch.zeros(C.BATCH, dtype=torch.int32, device="cuda")
    want[bad] = _native.STATUS_UNSUPPORTED
    assert torch.equal(st, want), st
    others = [e for e in range(C.BATCH) if e != bad]
    for o in range(6):
        assert torch.isnan(got[o][bad]).all(), C.NAMES[o]
        assert torch.equal(got[o][others], base[o][others]), C.NAMES[o]


# ---- 8. capture -------------------------------------------------------------------------------------

def test_mpc_backward_replays_from_a_hip_graph():
    _native.prepare_device()
    N, K = 10, 5
    ins = _cuda(C.workload(N, "random")[0])
    it = _cuda(C.iterate(N, "random", K))
    g = _cuda(C.seeds(N))[0]
    ws = torch.empty(_native.lib().srbd_mpc_backward_workspace_doubles(N, C.BATCH), dtype=torch.float64, device="cuda")
    eager = [t.clone() for t in solver.mpc_backward(ins, it, g, N, workspace=ws)]
    out = [torch.empty_like(t) for t in eager]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        solver.mpc_backward(ins, it, g, N, outputs=out, workspace=ws)  # warm-up on the capture's side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        solver.mpc_backward(ins, it, g, N, outputs=out, workspace=ws)
    for t in out:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for i in range(17):
        assert torch.equal(out[i], eager[i]), layout.FORMER_IN_NAMES[i]


# ---- 9. the composition's single-seed entry: no output requested, and its workspace bound -----------

def test_mpc_backward_with_every_output_null_writes_the_status_only():
    """srbd_mpc_backward accepts 17 null input_grads (srbd_mpc_backward_multi rejects them): it runs the
    chain and the status words are those of the adjoint solve."""
    N, K = 3, 5
    ins = _cuda(C.workload(N, "random")[0])
    it = _cuda(C.iterate(N, "random", K))
    g = _cuda(C.seeds(N))[0]
    st = torch.full((C.BATCH,), -1, dtype=torch.int32, device="cuda")
    outs = solver.mpc_backward(ins, it, g, N, status=st, outputs=[None] * 17)
    torch.cuda.synchronize()
    assert outs == [None] * 17
    assert torch.all(st == 0), st


def test_mpc_backward_stays_inside_the_documented_workspace():
    """All 17 outputs (so all six QP gradients) with a workspace of exactly
    srbd_mpc_backward_workspace_doubles(N, B) doubles: the 1024 doubles behind it keep their sentinel."""
    N, K, guard = 2, 5, 1024
    ins = _cuda(C.workload(N, "random")[0])
    it = _cuda(C.iterate(N, "random", K))
    g = _cuda(C.seeds(N))[0]
    n = _native.lib().srbd_mpc_backward_workspace_doubles(N, C.BATCH)
    sentinel = -0x5A5A5A5A5A5A5A5B
    buf = torch.full((n + guard,), sentinel, dtype=torch.int64, device="cuda").view(torch.float64)
    st = torch.full((C.BATCH,), -1, dtype=torch.int32, device="cuda")
    outs = solver.mpc_backward(ins, it, g, N, status=st, workspace=buf[:n])
    torch.cuda.synchronize()
    assert torch.all(st == 0), st
    assert all(o is not None and torch.isfinite(o).all() for o in outs)
    assert torch.all(buf[n:].view(torch.int64) == sentinel)
    assert not torch.all(buf[:n].view(torch.int64) == sentinel)  # the workspace itself was used
