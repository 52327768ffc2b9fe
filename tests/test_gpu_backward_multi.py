"""The multi-seed backward pass on the GPU: one factorisation and M solves per QP
(srbd_pdipm_backward_multi), the former VJP over seed rows (srbd_qp_former_backward_multi), their
composition (srbd_mpc_backward_multi), solution Jacobians and the u0 feedback gain.

The main criterion needs no tolerance: seed k's outputs are, bit for bit, what the single-seed entry
returns for that seed alone (1-3). Accuracy (4) is measured against the reference chain of
tests/_backward_multi_cases.py (dense refined adjoint -> former_vjp) with the CASES tolerance of the K that
produced the iterate, norm-wise per env and per seed row, no env excluded; tests/test_backward_multi_ref.py
holds the plain-FP64 floor of the kernel's algorithm at a tenth of that tolerance on the same inputs.
"""
import functools

import numpy as np
import pytest
import torch

from biped_pympc_amd import _native, layout, solver
from tests import _backward_cases as C
from tests import _backward_multi_cases as MC

pytestmark = pytest.mark.gpu


def _cuda(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in arrs]


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _dev_case(N, gait, K):
    """(former inputs, QP in the solver's order, iterate, [g_u0, g_all]) on the device."""
    ins, qp = C.workload(N, gait)
    return _cuda(ins), _cuda(qp), _cuda(C.iterate(N, gait, K)), _cuda(C.seeds(N))


def _status():
    return torch.full((C.BATCH,), -1, dtype=torch.int32, device="cuda")


def _three_seeds(N):
    g_u0, g_all = _dev_case(N, "random", 5)[3]
    return torch.stack([g_all, g_u0, g_all], dim=1).contiguous(), [g_all, g_u0, g_all]


# ---- 1. bit-identity with the single-seed entry ---------------------------------------------------

@pytest.mark.parametrize("N", C.HORIZONS)
def test_each_seed_row_has_the_bits_of_the_single_seed_call(N):
    _, qp, it, (g_u0, g_all) = _dev_case(N, "random", 5)
    single = {id(g): solver.pdipm_backward(qp, it, g, N) for g in (g_u0, g_all)}
    st = _status()
    one = solver.pdipm_backward_multi(qp, it, g_all[:, None, :].contiguous(), N, status=st)  # M = 1
    torch.cuda.synchronize()
    assert torch.all(st == 0), st
    for o, name in enumerate(C.NAMES):
        assert one[o].shape == (C.BATCH, 1, single[id(g_all)][o].shape[1])
        assert torch.equal(one[o][:, 0], single[id(g_all)][o]), name
    block, parts = _three_seeds(N)  # M = 3, per-env stride
    st = _status()
    got = solver.pdipm_backward_multi(qp, it, block, N, status=st)
    torch.cuda.synchronize()
    assert torch.all(st == 0), st
    for o, name in enumerate(C.NAMES):
        for k, g in enumerate(parts):
            assert torch.equal(got[o][:, k], single[id(g)][o]), (name, k)
        assert torch.equal(got[o][:, 2], got[o][:, 0]), name  # no state leaks from seed 1 into seed 2


@pytest.mark.parametrize("N", [3, 10])
def test_shared_unit_seeds_equal_twelve_single_calls_on_materialised_seeds(N):
    _, qp, it, _ = _dev_case(N, "random", 5)
    unit = solver.unit_seeds(N, MC.u0_rows(N))  # (12, 24N), stride 0
    assert torch.equal(unit, torch.from_numpy(MC.unit_seed_block(N)).cuda())
    got = solver.pdipm_backward_multi(qp, it, unit, N)
    for k in range(12):
        single = solver.pdipm_backward(qp, it, unit[k].expand(C.BATCH, -1).contiguous(), N)
        for o, name in enumerate(C.NAMES):
            assert torch.equal(got[o][:, k], single[o]), (name, k)


# ---- 2. the former VJP over seed rows -------------------------------------------------------------

# B = 67: the last workgroup of four rows is partial; B = 1: M = 3 rows, one wave idle
@pytest.mark.parametrize("N,B", [(3, 16), (3, 67), (3, 1), (32, 16)])
def test_former_vjp_over_seed_rows_equals_the_single_call_on_repeated_inputs(N, B):
    from biped_pympc_amd.utils.synthetic import make_workload
    M = 3
    ins = _cuda(make_workload(B, N, seed=950 + N, random_gait=True, residuals=True).inputs)
    rng = np.random.default_rng(2960 + N)
    cot = _cuda([rng.standard_normal((B, M, w)) for w in layout.Dims(N).former_out_nnz])
    got = solver.qp_former_backward_multi(ins, cot, N)
    rep = [t.repeat_interleave(M, dim=0).contiguous() for t in ins]
    want = solver.qp_former_backward(rep, [c.view(B * M, -1) for c in cot], N)
    part = solver.qp_former_backward_multi(ins, [None, None, None, cot[3], None, None], N,
                                           outputs=[torch.empty(B, M, 12, dtype=torch.float64, device="cuda")] + [None] * 16)
    want_part = solver.qp_former_backward(rep, [None, None, None, cot[3].view(B * M, -1), None, None], N)
    torch.cuda.synchronize()
    for i, name in enumerate(layout.FORMER_IN_NAMES):
        assert got[i].shape[:2] == (B, M)
        assert torch.equal(got[i].view(B * M, -1), want[i]), name
    assert torch.equal(part[0].view(B * M, -1), want_part[0]) and all(p is None for p in part[1:])


# ---- 3. composition -------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [3, 10])
def test_mpc_backward_multi_equals_the_three_calls_and_wrt_changes_no_bit(N):
    ins, _, it, _ = _dev_case(N, "random", 5)
    block, _ = _three_seeds(N)
    M = block.shape[1]
    qp = solver.qp_former(ins, N)  # H, f, A, b, G, d
    grads = solver.pdipm_backward_multi([qp[0], qp[4], qp[2], qp[1], qp[5], qp[3]], it, block, N)
    chain = solver.qp_former_backward_multi(ins, grads, N)
    st = _status()
    full = solver.mpc_backward_multi(ins, it, block, N, status=st)
    torch.cuda.synchronize()
    assert torch.all(st == 0)
    for i, name in enumerate(layout.FORMER_IN_NAMES):
        assert torch.equal(full[i], chain[i]), name
    # x0 only: the QP plus M * 14N doubles per env, same bits
    ws_fn = _native.lib().srbd_mpc_backward_multi_workspace_doubles
    n_small, n_full = ws_fn(N, C.BATCH, M, 1), ws_fn(N, C.BATCH, M, 0)
    assert n_small == _native.lib().srbd_mpc_workspace_doubles(N, C.BATCH) + C.BATCH * M * 14 * N < n_full
    ws = torch.full((n_small,), float("nan"), dtype=torch.float64, device="cuda")
    only = solver.mpc_backward_multi(ins, it, block, N, wrt=[0], workspace=ws)
    some = solver.mpc_backward_multi(ins, it, block, N, wrt=[3, 13, 16])
    torch.cuda.synchronize()
    assert torch.equal(only[0], full[0]) and all(t is None for t in only[1:])
    for i in range(17):
        if i in (3, 13, 16):
            assert torch.equal(some[i], full[i]), layout.FORMER_IN_NAMES[i]
        else:
            assert some[i] is None


def test_jacobian_and_gain_are_the_unit_seed_rows():
    N = 3
    ins, _, it, _ = _dev_case(N, "random", 5)
    rows = [0, 12 * N + 2, 24 * N - 1]
    jac = solver.mpc_jacobian(ins, it, N, rows, wrt=[0, 15])
    full = solver.mpc_backward_multi(ins, it, solver.unit_seeds(N, rows), N)
    gain = solver.mpc_feedback_gain(ins, it, N)
    want = solver.mpc_backward_multi(ins, it, solver.unit_seeds(N, MC.u0_rows(N)), N, wrt=[0])[0]
    torch.cuda.synchronize()
    assert jac[0].shape == (C.BATCH, 3, 12) and jac[15].shape == (C.BATCH, 3, 3)
    assert torch.equal(jac[0], full[0]) and torch.equal(jac[15], full[15])
    assert all(jac[i] is None for i in range(17) if i not in (0, 15))
    assert gain.shape == (C.BATCH, 12, 12) and torch.equal(gain, want)


# ---- 4. accuracy of the gain and of the Jacobians of x_ref and residual_ang_accel -----------------

@pytest.mark.parametrize("K,tol", C.CASES)
@pytest.mark.parametrize("gait", C.GAITS)
@pytest.mark.parametrize("N", C.HORIZONS)
def test_gain_and_jacobians_match_the_reference_chain(N, gait, K, tol):
    ins, _, it, _ = _dev_case(N, gait, K)
    st = _status()
    got = solver.mpc_jacobian(ins, it, N, MC.u0_rows(N), wrt=range(17), status=st)
    torch.cuda.synchronize()
    assert torch.all(st == 0), st
    ref = MC.unit_reference(N, gait, K)
    errs = {i: MC.row_err(_np(got[i]), ref[i]) for i in range(17) if i not in (1, 2)}
    for i, err in errs.items():
        e, k = np.unravel_index(err.argmax(), err.shape)
        print(f"N={N} {gait} K={K} d u0 / d {layout.FORMER_IN_NAMES[i]}: max rel err {err.max():.3e} "
              f"(env {e}, seed row {k}){f', tol {tol:.0e}' if i in MC.ASSERTED else ''}")
    assert torch.all(got[1] == 0.0) and torch.all(got[2] == 0.0)
    for i in MC.ASSERTED:
        assert np.all(errs[i] <= tol), (layout.FORMER_IN_NAMES[i], errs[i].max())


# ---- 5. behaviour ---------------------------------------------------------------------------------

def test_unsupported_qp_gets_nan_in_all_its_rows_and_its_status_bit_neighbours_unchanged():
    N, bad = 3, 5
    _, qp, it, _ = _dev_case(N, "random", 5)
    block, _ = _three_seeds(N)
    base = solver.pdipm_backward_multi(qp, it, block, N)
    H = qp[0].clone()
    H[bad, 12:24] *= 1.5  # stage 1 of the x weights: no longer stage-invariant
    st = _status()
    got = solver.pdipm_backward_multi([H] + qp[1:], it, block, N, status=st)
    torch.cuda.synchronize()
    want = torch.zeros(C.BATCH, dtype=torch.int32, device="cuda")
    want[bad] = _native.STATUS_UNSUPPORTED
    assert _native.STATUS_UNSUPPORTED == 8 and torch.equal(st, want), st
    others = [e for e in range(C.BATCH) if e != bad]
    for o, name in enumerate(C.NAMES):
        assert torch.isnan(got[o][bad]).all(), name  # all M rows
        assert torch.equal(got[o][others], base[o][others]), name


@pytest.mark.parametrize("keep", [(3,), (0, 2), (1, 4, 5)])
def test_null_outputs_are_skipped_and_change_no_bit_of_the_others(keep):
    N = 3
    _, qp, it, _ = _dev_case(N, "fixed", 5)
    block, _ = _three_seeds(N)
    base = solver.pdipm_backward_multi(qp, it, block, N)
    outs = [torch.full_like(base[o], float("nan")) if o in keep else None for o in range(6)]
    got = solver.pdipm_backward_multi([qp[0], qp[1], qp[2], None, None, None], it, block, N, outputs=outs)
    torch.cuda.synchronize()
    for o in range(6):
        if o in keep:
            assert torch.equal(got[o], base[o]), C.NAMES[o]
        else:
            assert got[o] is None


def test_rows_do_not_depend_on_batch_size_position_or_stream():
    N, K = 10, 10
    _, qp, it, _ = _dev_case(N, "random", K)
    block, _ = _three_seeds(N)
    unit = solver.unit_seeds(N, MC.u0_rows(N))
    base, base_unit = solver.pdipm_backward_multi(qp, it, block, N), solver.pdipm_backward_multi(qp, it, unit, N)
    idx = torch.arange(67, device="cuda") % C.BATCH
    idx[66] = 0  # env 0 at position 0 and at position 66 of 67
    big_qp, big_it = [t[idx].contiguous() for t in qp], [t[idx].contiguous() for t in it]
    big = solver.pdipm_backward_multi(big_qp, big_it, block[idx].contiguous(), N)
    big_unit = solver.pdipm_backward_multi(big_qp, big_it, unit, N)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = solver.pdipm_backward_multi(qp, it, block, N)
    with torch.cuda.stream(s2):
        b = solver.pdipm_backward_multi(qp, it, block, N)
    torch.cuda.synchronize()
    for o, name in enumerate(C.NAMES):
        assert torch.equal(big[o], base[o][idx]) and torch.equal(big_unit[o], base_unit[o][idx]), name
        assert torch.equal(big[o][66], base[o][0]), name
        assert torch.equal(a[o], base[o]) and torch.equal(b[o], base[o]), name


def test_feedback_gain_replays_from_a_hip_graph():
    _native.prepare_device()
    N, K = 10, 5
    ins, _, it, _ = _dev_case(N, "random", K)
    seeds = solver.unit_seeds(N, MC.u0_rows(N))
    ws = torch.empty(_native.lib().srbd_mpc_backward_multi_workspace_doubles(N, C.BATCH, 12, 1), dtype=torch.float64,
                     device="cuda")
    eager = solver.mpc_feedback_gain(ins, it, N).clone()
    out = torch.empty_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        solver.mpc_feedback_gain(ins, it, N, seeds=seeds, out=out, workspace=ws)  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        solver.mpc_feedback_gain(ins, it, N, seeds=seeds, out=out, workspace=ws)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_controller_feedback_gain_is_the_gain_of_its_last_step():
    from tests.test_controller import _controller, random_robot
    N, B = 10, 16
    args = random_robot(B, 61, N, gait=True)
    c = _controller(B, N, *args)
    c.run()
    with pytest.raises(RuntimeError, match="keep_solution"):
        c.feedback_gain()
    c = _controller(B, N, *args)
    c.cfg.keep_solution = True
    with pytest.raises(RuntimeError, match="keep_solution"):  # no step yet
        c.feedback_gain()
    wrench = c.run()[0].clone()
    gain = c.feedback_gain()
    want = solver.mpc_feedback_gain(c.former_inputs, list(c.solution[:4]), N)
    torch.cuda.synchronize()
    assert gain.shape == (B, 12, 12) and gain.dtype == torch.float64
    assert torch.equal(gain, want) and torch.isfinite(gain).all() and gain.abs().max() > 0
    assert torch.equal(c.foot_wrench, wrench)  # the gain leaves the step's outputs alone
