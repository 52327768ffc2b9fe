"""The controller step's backward entry points at the C-ABI boundary, without a GPU: the symbols exist, bad
arguments return an error code and a message, an empty batch is a successful no-op, the dependency table is
the one of csrc/mpc_io_backward.hpp and the workspace holds only what the requested gradients read. No compute
call is made here."""
import ctypes
import re
from pathlib import Path

import pytest

from biped_pympc_amd import _native, layout
from tests import _step_backward_ref as R

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ["srbd_u0_wrench_backward", "srbd_prepare_inputs_backward", "srbd_prep_grad_deps",
           "srbd_mpc_step_backward_workspace_doubles", "srbd_mpc_step_backward"]
ONE = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced


def _prep(gait=False, **null):
    p = _native.MPCPrep()
    for name, _ in _native.MPCPrep._fields_[:19]:
        setattr(p, name, 8)
    p.gait_phase = 8 if gait else None
    for name in null:
        setattr(p, name, None)
    p.q_len = 13
    return p


def test_the_five_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "srbd_mpc.h").read_text()
    raw = ctypes.CDLL(_native.lib_path())
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(raw, name), name
    for i, name in enumerate(_native.PREP_GRAD_NAMES):
        assert re.search(rf"#define SRBD_PREP_GRAD_{name.upper()} {i}\b", header), name
    assert "#define SRBD_PREP_GRAD_COUNT 15" in header and _native.PREP_GRAD_NAMES == R.FIELDS


def test_wrench_backward_bad_arguments():
    f = _native.lib().srbd_u0_wrench_backward
    N = 10
    for args in [(0, 4, ONE, ONE, ONE, 0, None, None, None, ONE, ONE), (33, 4, ONE, ONE, ONE, 0, None, None, None, ONE, ONE),
                 (N, -1, ONE, ONE, ONE, 0, None, None, None, ONE, ONE)]:
        assert f(*args, None) != 0, args[:2]
        assert "srbd_u0_wrench_backward: bad arguments" in _native.last_error()
    for args in [(N, 4, None, ONE, ONE, 0, None, None, None, ONE, ONE), (N, 4, ONE, None, ONE, 0, None, None, None, ONE, ONE),
                 (N, 4, ONE, ONE, None, 0, None, None, None, ONE, ONE), (N, 4, ONE, ONE, ONE, 0, None, None, None, None, ONE)]:
        assert f(*args, None) != 0
        assert "srbd_u0_wrench_backward: null" in _native.last_error()
    for ndof, J, cb in [(5, None, ONE), (5, ONE, None), (0, ONE, ONE), (-1, ONE, ONE), (65, ONE, ONE)]:
        assert f(N, 4, ONE, ONE, ONE, ndof, J, cb, ONE, ONE, ONE, None) != 0, (ndof, J, cb)
        assert "grad_tau needs" in _native.last_error()
    assert f(N, 0, None, None, None, 0, None, None, None, None, None, None) == 0


def test_prepare_inputs_backward_bad_arguments():
    f = _native.lib().srbd_prepare_inputs_backward
    n17, n15 = _native.ptr_array([0] * 17), _native.ptr_array([8] * 15)
    p = _prep()
    N = 10
    for args in [(0, 4, ctypes.byref(p), n17, None, None, None, n15), (33, 4, ctypes.byref(p), n17, None, None, None, n15),
                 (N, -1, ctypes.byref(p), n17, None, None, None, n15), (N, 4, None, n17, None, None, None, n15),
                 (N, 4, ctypes.byref(p), None, None, None, None, n15), (N, 4, ctypes.byref(p), n17, None, None, None, None)]:
        assert f(*args, None) != 0, args[:2]
        assert "srbd_prepare_inputs_backward: bad arguments" in _native.last_error()
    for name in ("rotation_body", "desired_velocity_b", "desired_angular_velocity_b", "dt_mpc", "first_run"):
        q = _prep(**{name: True})
        assert f(N, 4, ctypes.byref(q), n17, None, None, None, n15, None) != 0, name
        assert "srbd_prepare_inputs_backward: null" in _native.last_error()
    g = _prep(gait=True)  # the schedule comes from the gait phase: no contact_table gradient
    assert f(N, 4, ctypes.byref(g), n17, None, None, None, n15, None) != 0
    assert "contact_table" in _native.last_error() and "gait_phase" in _native.last_error()
    assert f(N, 0, ctypes.byref(p), n17, None, None, None, n15, None) == 0
    no_table = _native.ptr_array([0 if i == 11 else 8 for i in range(15)])
    assert f(N, 0, ctypes.byref(g), n17, None, None, None, no_table, None) == 0


def test_step_backward_bad_arguments():
    f = _native.lib().srbd_mpc_step_backward
    n17, n4, n15 = _native.ptr_array([8] * 17), _native.ptr_array([8] * 4), _native.ptr_array([8] * 15)
    p = _prep()
    bp = ctypes.byref(p)
    N = 10
    tail = (ONE, 0, None, None, None, None, None, ONE, n15)
    for args in [(0, 4, bp, n17, n4) + tail, (33, 4, bp, n17, n4) + tail, (N, -1, bp, n17, n4) + tail,
                 (N, 4, None, n17, n4) + tail, (N, 4, bp, None, n4) + tail, (N, 4, bp, n17, None) + tail,
                 (N, 4, bp, n17, n4) + tail[:-1] + (None,)]:
        assert f(*args, None, None) != 0, args[:2]
        assert "srbd_mpc_step_backward: bad arguments" in _native.last_error()
    for ndof, J, cb in [(5, None, ONE), (5, ONE, None), (0, ONE, ONE)]:
        assert f(N, 4, bp, n17, n4, ONE, ndof, J, cb, ONE, None, None, ONE, n15, None, None) != 0
        assert "grad_tau needs" in _native.last_error()
    g = _prep(gait=True)
    assert f(N, 4, ctypes.byref(g), n17, n4, *tail, None, None) != 0
    assert "contact_table" in _native.last_error()
    assert f(N, 4, bp, n17, n4, ONE, 0, None, None, None, None, None, ONE, _native.ptr_array([0] * 15), None, None) != 0
    assert "no prep gradient requested" in _native.last_error()
    assert f(N, 4, bp, n17, n4, ONE, 0, None, None, None, None, None, None, n15, None, None) != 0  # workspace
    assert "null workspace" in _native.last_error()
    assert f(N, 4, bp, n17, n4, None, 0, None, None, None, None, None, ONE, n15, None, None) != 0  # grad_wrench
    assert f(N, 4, bp, n17, _native.ptr_array([8, 8, 0, 8]), *tail, None, None) != 0  # iterate
    q = _prep(first_run=True)
    assert f(N, 4, ctypes.byref(q), n17, n4, *tail, None, None) != 0
    assert "first_run" in _native.last_error()
    assert f(N, 0, bp, n17, n4, None, 0, None, None, None, None, None, None, n15, None, None) == 0


@pytest.mark.parametrize("field", range(15))
def test_prep_grad_deps_is_the_table_of_the_prep_vjp(field):
    want = sum(1 << i for i in R.DEPS[R.FIELDS[field]])
    assert _native.lib().srbd_prep_grad_deps(field) == want, R.FIELDS[field]


def test_prep_grad_deps_examples_and_range():
    L = _native.lib()
    assert L.srbd_prep_grad_deps(R.FIELDS.index("dt_mpc")) == (1 << 3) | (1 << 4)
    assert L.srbd_prep_grad_deps(R.FIELDS.index("rotation_body")) == (1 << 3) | (1 << 7) | (1 << 8)
    assert L.srbd_prep_grad_deps(-1) == 0 and L.srbd_prep_grad_deps(15) == 0
    names = layout.FORMER_IN_NAMES
    assert names[3] == "x_ref" and names[4] == "dt" and "contact" in names[12]


def _former_mask(prep_mask):
    m = 0
    for f in range(15):
        if prep_mask >> f & 1:
            m |= sum(1 << i for i in R.DEPS[R.FIELDS[f]])
    return m


@pytest.mark.parametrize("N,Bn", [(10, 4096), (1, 3), (32, 7)])
def test_workspace_is_seed_direct_term_cotangents_and_the_backward_workspace(N, Bn):
    L = _native.lib()
    ws = L.srbd_mpc_step_backward_workspace_doubles
    widths = layout.Dims(N).former_in_nnz
    masks = [1 << f for f in range(15)] + [(1 << 12) | (1 << 13), (1 << 4) | (1 << 11), (1 << 15) - 1]
    for pm in masks:
        fm = _former_mask(pm)
        want = Bn * (24 * N + 9 + sum(w for i, w in enumerate(widths) if fm >> i & 1))
        want += L.srbd_mpc_backward_multi_workspace_doubles(N, Bn, 1, fm)
        assert ws(N, Bn, pm) == want, pm
    assert ws(N, Bn, 0) == ws(N, Bn, (1 << 15) - 1)
    # monotone in the mask
    for f in range(15):
        for g in range(15):
            assert ws(N, Bn, 1 << f) <= ws(N, Bn, (1 << f) | (1 << g)) <= ws(N, Bn, 0)
    assert ws(N, Bn, (1 << 12) | (1 << 13)) < ws(N, Bn, 0)  # dt_mpc, residual_lin_accel: far less than everything
    for bad in [(0, Bn), (33, Bn), (N, -1)]:
        assert ws(*bad, 0) == 0, bad
