"""Seeds on every output of a solve (x, s, z, y, the objective), on the CPU: the reference of
tests/_backward_full_ref.py against central differences, its reduced elimination against its dense solve on
the GPU tests' inputs, and the new entry points at the C-ABI boundary (no compute call is made here).

Central differences: the frozen-residual root of tests/test_backward_ref.py, extended to return all of
(x, s, z, y); the loss is g_x^T x + g_s^T s + g_z^T z + g_y^T y + g_J J(theta, x), J = 1/2 x^T H x + f^T x
with the perturbed H and f. The acceptance rule, the step sizes and the perturbations are that file's.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from biped_pympc_amd import _native
from biped_pympc_amd.utils.synthetic import make_workload
from tests import _backward_cases as C
from tests import _backward_full_ref as fr
from tests import _backward_ref as br
from tests.test_backward_ref import _Root, _accept, _adjoint_case, _dv
from tests.test_step_backward_abi import _prep

ROOT = Path(__file__).resolve().parents[1]
ONE = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced


# ------------------------------------------------------------------ formulas against central differences ----

class _FullRoot(_Root):
    """_Root whose solve returns the whole root (x, s, z, y)."""

    def solve_all(self, theta):
        Hv, f, Av, b, Gv, d = theta
        H, G, A = br.dense_qp(self.N, Hv, Gv, Av)
        N = self.N
        nz, m = 24 * N, 16 * N
        w = np.concatenate(self.w0)
        for _ in range(30):
            x, s, z, y = br.split(N, w)
            K = br.dense_kkt(N, H, G, A, self.s0, z)
            K[nz:nz + m, nz + m:nz + 2 * m] = np.diag(s / self.s0)
            step = br.solve_refined(K, -(self.F(theta, (x, s, z, y)) - self.c), steps=1)
            w = w + step
            if np.abs(step).max() <= 1e-15 * np.abs(w).max():
                break
        return br.split(N, w)


def _case(former_inputs):
    N, theta, w0, _, _ = _adjoint_case(former_inputs)
    rng = np.random.default_rng(11)
    w = fr.widths(N)
    seed = {k: rng.standard_normal(w[k]) for k in ("x", "s", "z", "y")}
    seed["objective"] = rng.standard_normal(1)
    return N, theta, w0, seed


@pytest.fixture(scope="module")
def full_case():
    return _case(make_workload(2, 2, seed=41, random_gait=True, residuals=True).inputs)


@pytest.fixture(scope="module")
def full_case_generic():
    from tests._generic import generic_former_inputs
    return _case(generic_former_inputs(2, 2, seed=41, solvable=True))


SEED_KINDS = ["x", "s", "z", "y", "objective", "all"]
DATA = ["H", "f", "A", "b", "G", "d", "all"]


def _check(case, kind, which):
    N, theta, w0, seed_all = case
    seed = dict(seed_all) if kind == "all" else {kind: seed_all[kind]}
    H, f, A, b, G, d = theta
    grads = fr.pdipm_backward_full(N, [H, G, A, f, d, b] + w0, [seed])[0]
    root = _FullRoot(N, theta, w0)
    rng = np.random.default_rng(100 + sum(map(ord, which)))
    dv = [_dv(rng, th) if which in (n, "all") else np.zeros_like(th) for n, th in zip(DATA[:6], theta)]
    analytic = sum(float(gr @ v) for gr, v in zip(grads, dv))
    magnitude = sum(float(np.abs(gr * v).sum()) for gr, v in zip(grads, dv))

    ld = np.longdouble

    def loss(th):
        # summed in longdouble: J ~ 3e2 as one double is quantised at 3e-14, which over 2 t = 2e-8 is 1e-6 of
        # noise that fd(t) - fd(t / 2) does not see (both differences round to whole ulps of J)
        x, s, z, y = (v.astype(ld) for v in root.solve_all(th))
        out = sum((seed[k].astype(ld) @ v for k, v in zip(("x", "s", "z", "y"), (x, s, z, y)) if k in seed), ld(0))
        if "objective" in seed:
            out += ld(seed["objective"][0]) * (ld(0.5) * (x @ (th[0].astype(ld) * x)) + th[1].astype(ld) @ x)
        return out

    def fd(t):
        up, dn = ([th + sign * t * v for th, v in zip(theta, dv)] for sign in (1.0, -1.0))
        return float((loss(up) - loss(dn)) / ld(2 * t))
    t = 1e-8 if which in ("d", "all") else 1e-4  # tests/test_backward_ref.py: the root is strongly curved in d
    fd_t, fd_h = fd(t), fd(t / 2)
    print(f"seed {kind}, data {which}: analytic {analytic:.12e} fd(t) {fd_t:.12e} fd(t/2) {fd_h:.12e} "
          f"magnitude {magnitude:.3e}")
    assert magnitude > 0.0
    assert _accept(fd_t, fd_h, analytic, magnitude)


@pytest.mark.parametrize("which", DATA)
@pytest.mark.parametrize("kind", SEED_KINDS)
def test_full_seed_gradients_match_central_differences_of_the_frozen_root(full_case, kind, which):
    _check(full_case, kind, which)


@pytest.mark.parametrize("which", DATA)
@pytest.mark.parametrize("kind", SEED_KINDS)
def test_full_seed_gradients_match_central_differences_at_a_generic_point(full_case_generic, kind, which):
    _check(full_case_generic, kind, which)


def test_an_x_seed_alone_is_the_x_only_reference(full_case):
    N, theta, w0, seed = full_case
    H, f, A, b, G, d = theta
    ins = [H, G, A, f, d, b] + w0
    old = br.pdipm_backward(N, ins, seed["x"])
    new = fr.pdipm_backward_full(N, ins, [{"x": seed["x"]}])[0]
    for a, r in zip(new, old):
        assert np.array_equal(a, r)


# ------------------------------------------------------------------ the reduced elimination's floor ----

@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_reduced_floor_with_full_seeds_is_within_the_gpu_tolerance_on_the_gpu_cases(N):
    """The reference alone on the inputs of tests/test_gpu_backward_full.py: the plain-FP64 reduced elimination
    with the full right-hand side stays within the case's tolerance for every env, output and seed kind, so the
    GPU test excludes no env. (N = 32, minutes here: K = 5 worst 5.9e-11 against 1e-9; at K = 20, fixed gait,
    a z seed sits at 1.6e-5, above 1e-5 -- which is why the GPU accuracy test keeps N = 32 at K = 5.)"""
    for gait in C.GAITS:
        for K, tol in C.CASES:
            floor = fr.reduced_floor(N, gait, K)
            for kind in fr.KINDS:
                worst = float(floor[kind].max())
                print(f"N={N} {gait} K={K} {kind}: worst floor {worst:.3e} (tol {tol:.0e}, ratio {worst / tol:.3f})")
                assert worst <= tol


# ------------------------------------------------------------------ the C-ABI boundary ----

SYMBOLS = ["srbd_pdipm_backward_seeds", "srbd_mpc_backward_seeds", "srbd_mpc_step_backward_cost",
           "srbd_mpc_step_backward_cost_workspace_doubles"]


def _seeds(shared=0, **given):
    return _native.BackwardSeeds(*[8 if given.get(k) else None for k in ("x", "s", "z", "y", "objective")], shared)


def test_the_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "srbd_mpc.h").read_text()
    raw = ctypes.CDLL(_native.lib_path())
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(raw, name), name
    assert "typedef struct srbd_backward_seeds" in header
    assert "out of scope" not in header


def test_seeds_entries_bad_arguments_return_errors_without_touching_the_gpu():
    L = _native.lib()
    n17, n10, n6, n4 = (_native.ptr_array([0] * k) for k in (17, 10, 6, 4))
    N, M = 10, 3
    sx = ctypes.byref(_seeds(x=1))
    f = L.srbd_pdipm_backward_seeds
    for args in [(0, 4, M, n10, sx, n6), (33, 4, M, n10, sx, n6), (N, -1, M, n10, sx, n6), (N, 4, 0, n10, sx, n6),
                 (N, 4, M, None, sx, n6), (N, 4, M, n10, None, n6), (N, 4, M, n10, sx, None)]:
        assert f(*args, None, None) != 0, args[:3]
        assert "srbd_pdipm_backward_seeds: bad arguments" in _native.last_error()
    assert f(N, 1 << 30, 4, n10, sx, n6, None, None) != 0
    assert "overflows" in _native.last_error()
    assert f(N, 4, M, n10, sx, n6, None, None) != 0
    assert "null input" in _native.last_error()
    no_f = _native.ptr_array([8, 8, 8, 0, 0, 0, 8, 8, 8, 8])  # f, h, b null
    assert f(N, 4, M, no_f, ctypes.byref(_seeds()), n6, None, None) != 0
    assert "no seed given" in _native.last_error()
    for kind in ("s", "z", "y"):  # each alone is a seed; the null-input check is reached with the full QP only
        assert f(N, 4, M, n10, ctypes.byref(_seeds(**{kind: 1})), n6, None, None) != 0
        assert "null input" in _native.last_error()
    assert f(N, 4, M, no_f, ctypes.byref(_seeds(x=1, objective=1)), n6, None, None) != 0
    assert "grad_objective needs f" in _native.last_error()
    assert f(N, 0, M, n10, ctypes.byref(_seeds()), n6, None, None) == 0
    assert f(N, 0, M, n10, ctypes.byref(_seeds(shared=1, z=1)), n6, None, None) == 0
    g = L.srbd_mpc_backward_seeds
    want_x0 = _native.ptr_array([8] + [0] * 16)
    for args in [(40, 4, M, n17, n4, sx, ONE, want_x0), (N, -1, M, n17, n4, sx, ONE, want_x0),
                 (N, 4, 0, n17, n4, sx, ONE, want_x0), (N, 4, M, None, n4, sx, ONE, want_x0),
                 (N, 4, M, n17, None, sx, ONE, want_x0), (N, 4, M, n17, n4, None, ONE, want_x0),
                 (N, 4, M, n17, n4, sx, ONE, None)]:
        assert g(*args, None, None) != 0, args[:3]
        assert "srbd_mpc_backward_seeds: bad arguments" in _native.last_error()
    assert g(N, 1 << 30, 4, n17, n4, sx, ONE, want_x0, None, None) != 0
    assert "overflows" in _native.last_error()
    assert g(N, 4, M, n17, n4, sx, None, want_x0, None, None) != 0
    assert "null workspace" in _native.last_error()
    it = _native.ptr_array([8] * 4)
    assert g(N, 4, M, n17, it, ctypes.byref(_seeds()), ONE, want_x0, None, None) != 0
    assert "no seed given" in _native.last_error()
    assert g(N, 0, M, n17, n4, ctypes.byref(_seeds()), None, n17, None, None) == 0


def test_step_backward_cost_bad_arguments_and_workspace():
    L = _native.lib()
    f = L.srbd_mpc_step_backward_cost
    n17, n4, n15 = _native.ptr_array([8] * 17), _native.ptr_array([8] * 4), _native.ptr_array([8] * 15)
    bp = ctypes.byref(_prep())
    N = 10
    tail = (ONE, ONE, 0, None, None, None, None, None, ONE, n15)  # grad_wrench, grad_cost, ..., workspace, grads
    for args in [(0, 4, bp, n17, n4) + tail, (33, 4, bp, n17, n4) + tail, (N, -1, bp, n17, n4) + tail,
                 (N, 4, None, n17, n4) + tail, (N, 4, bp, None, n4) + tail, (N, 4, bp, n17, None) + tail,
                 (N, 4, bp, n17, n4) + tail[:-1] + (None,)]:
        assert f(*args, None, None) != 0, args[:2]
        assert "srbd_mpc_step_backward_cost: bad arguments" in _native.last_error()
    assert f(N, 4, bp, n17, n4, None, None, 0, None, None, None, None, None, ONE, n15, None, None) != 0
    assert "grad_wrench and grad_cost are both null" in _native.last_error()
    assert f(N, 4, bp, n17, n4, None, ONE, 5, ONE, ONE, ONE, None, None, ONE, n15, None, None) != 0
    assert "grad_tau needs grad_wrench" in _native.last_error()
    assert f(N, 4, bp, n17, n4, None, ONE, 0, None, None, None, None, None, None, n15, None, None) != 0
    assert "null workspace" in _native.last_error()
    assert f(N, 4, bp, n17, n4, None, ONE, 0, None, None, None, None, None, ONE, _native.ptr_array([0] * 15),
             None, None) != 0
    assert "no prep gradient requested" in _native.last_error()
    assert f(N, 0, bp, n17, n4, None, None, 0, None, None, None, None, None, None, n15, None, None) == 0
    ws, old = L.srbd_mpc_step_backward_cost_workspace_doubles, L.srbd_mpc_step_backward_workspace_doubles
    for Nn, Bn, mask in [(10, 4096, 0), (1, 3, 1 << 13), (32, 7, (1 << 12) | (1 << 4))]:
        assert ws(Nn, Bn, mask) == old(Nn, Bn, mask) + Bn  # the old layout, then the widened cost cotangent
    assert ws(0, 4, 0) == 0 and ws(33, 4, 0) == 0 and ws(10, -1, 0) == 0
