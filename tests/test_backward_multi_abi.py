"""The multi-seed backward entry points at the C-ABI boundary, without a GPU: the symbols exist, bad
arguments return an error code and a message, an empty batch is a successful no-op, the dependency table
is the one of qp_former_backward.hpp and the workspace holds the QP plus only the gradients the requested
inputs read. No compute call is made here."""
import ctypes
import re
from pathlib import Path

import pytest

from biped_pympc_amd import _native, layout

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ["srbd_pdipm_backward_multi", "srbd_qp_former_backward_multi", "srbd_former_grad_deps",
           "srbd_mpc_backward_multi_workspace_doubles", "srbd_mpc_backward_multi"]
H, F, A, B_, G, D = 1, 2, 4, 8, 16, 32  # grad_H, grad_f, grad_A, grad_b, grad_G, grad_d


def test_the_five_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "srbd_mpc.h").read_text()
    raw = ctypes.CDLL(_native.lib_path())
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(raw, name), name


def test_bad_arguments_return_errors_without_touching_the_gpu():
    L = _native.lib()
    n17, n10, n6, n4 = (_native.ptr_array([0] * k) for k in (17, 10, 6, 4))
    one = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced
    N, M = 10, 12
    full = M * 24 * N
    # srbd_pdipm_backward_multi
    for args in [(0, 4, M, n10, one, 0, n6), (33, 4, M, n10, one, 0, n6), (N, -1, M, n10, one, 0, n6),
                 (N, 4, 0, n10, one, 0, n6), (N, 4, -3, n10, one, 0, n6), (N, 4, M, None, one, 0, n6),
                 (N, 4, M, n10, one, 0, None)]:
        assert L.srbd_pdipm_backward_multi(*args, None, None) != 0, args[:3]
        assert "srbd_pdipm_backward_multi: bad arguments" in _native.last_error()
    for stride in (1, 24 * N, full - 1, full + 24 * N):  # neither 0 nor n_seeds * 24N
        assert L.srbd_pdipm_backward_multi(N, 4, M, n10, one, stride, n6, None, None) != 0
        assert "grad_x_env_stride" in _native.last_error()
    assert L.srbd_pdipm_backward_multi(N, 1 << 30, 4, n10, one, 0, n6, None, None) != 0  # 2^32 rows
    assert "overflows" in _native.last_error()
    for stride in (0, full):
        assert L.srbd_pdipm_backward_multi(N, 4, M, n10, one, stride, n6, None, None) != 0
        assert "null input" in _native.last_error()
    some = _native.ptr_array([8, 8, 8, 0, 0, 0, 8, 8, 8, 8])  # f, h, b may be null; grad_x may not
    assert L.srbd_pdipm_backward_multi(N, 4, M, some, None, 0, n6, None, None) != 0
    assert "null grad_x" in _native.last_error()
    assert L.srbd_pdipm_backward_multi(N, 0, M, n10, None, 0, n6, None, None) == 0
    assert L.srbd_pdipm_backward_multi(N, 0, M, n10, None, full, n6, None, None) == 0
    # srbd_qp_former_backward_multi
    for args in [(0, 4, M, n17, n6, n17), (N, -1, M, n17, n6, n17), (N, 4, 0, n17, n6, n17),
                 (N, 4, M, None, n6, n17), (N, 4, M, n17, None, n17), (N, 4, M, n17, n6, None)]:
        assert L.srbd_qp_former_backward_multi(*args, None) != 0, args[:3]
        assert "srbd_qp_former_backward_multi: bad arguments" in _native.last_error()
    assert L.srbd_qp_former_backward_multi(N, 1 << 30, 2, n17, n6, n17, None) != 0
    assert "overflows" in _native.last_error()
    assert L.srbd_qp_former_backward_multi(N, 4, M, n17, n6, n17, None) != 0
    assert "null input" in _native.last_error()
    assert L.srbd_qp_former_backward_multi(N, 0, M, n17, n6, n17, None) == 0
    # srbd_mpc_backward_multi
    want_x0 = _native.ptr_array([8] + [0] * 16)
    for args in [(40, 4, M, n17, n4, one, 0, one, want_x0), (N, -1, M, n17, n4, one, 0, one, want_x0),
                 (N, 4, 0, n17, n4, one, 0, one, want_x0), (N, 4, M, None, n4, one, 0, one, want_x0),
                 (N, 4, M, n17, None, one, 0, one, want_x0), (N, 4, M, n17, n4, one, 0, one, None)]:
        assert L.srbd_mpc_backward_multi(*args, None, None) != 0, args[:3]
        assert "srbd_mpc_backward_multi: bad arguments" in _native.last_error()
    assert L.srbd_mpc_backward_multi(N, 4, M, n17, n4, one, 24 * N, one, want_x0, None, None) != 0
    assert "grad_x_env_stride" in _native.last_error()
    assert L.srbd_mpc_backward_multi(N, 1 << 30, 4, n17, n4, one, 0, one, want_x0, None, None) != 0
    assert "overflows" in _native.last_error()
    assert L.srbd_mpc_backward_multi(N, 4, M, n17, n4, one, 0, None, want_x0, None, None) != 0
    assert "null workspace" in _native.last_error()
    assert L.srbd_mpc_backward_multi(N, 4, M, n17, n4, None, 0, one, want_x0, None, None) != 0  # null grad_x
    assert L.srbd_mpc_backward_multi(N, 4, M, n17, n4, one, 0, one, want_x0, None, None) != 0  # null iterate
    assert L.srbd_mpc_backward_multi(N, 0, M, n17, n4, None, 0, None, n17, None, None) == 0


DEPS = {0: B_, 1: 0, 2: 0, 3: F, 4: A | B_, 5: A | B_, 6: G, 7: A | B_, 8: A | B_, 9: A | B_, 10: A | B_,
        11: A | B_, 12: D, 13: H | F, 14: H, 15: A | B_, 16: A | B_}


@pytest.mark.parametrize("i", range(17))
def test_former_grad_deps_is_the_table_of_the_former_vjp(i):
    assert _native.lib().srbd_former_grad_deps(i) == DEPS[i], layout.FORMER_IN_NAMES[i]


def test_former_grad_deps_names_and_range():
    names = layout.FORMER_IN_NAMES
    assert names[0] == "x0" and names[3] == "x_ref" and "contact" in names[12] and names[6] == "mu"
    assert names[13] == "Q" and names[14] == "R"
    L = _native.lib()
    assert L.srbd_former_grad_deps(-1) == 0 and L.srbd_former_grad_deps(17) == 0


@pytest.mark.parametrize("N,Bn,M", [(10, 4096, 12), (1, 3, 1), (32, 7, 5)])
def test_workspace_is_the_qp_plus_the_needed_gradients(N, Bn, M):
    L = _native.lib()
    ws = L.srbd_mpc_backward_multi_workspace_doubles
    qp = L.srbd_mpc_workspace_doubles(N, Bn)
    widths = layout.Dims(N).former_out_nnz  # H, f, A, b, G, d
    assert qp == Bn * sum(widths)
    assert ws(N, Bn, M, 0) == qp + Bn * M * sum(widths)  # all 17 inputs: all six gradients
    assert ws(N, Bn, M, (1 << 17) - 1) == ws(N, Bn, M, 0)
    assert ws(N, Bn, M, 1 << 0) == qp + Bn * M * 14 * N  # x0 only: grad_b
    assert ws(N, Bn, M, 1 << 3) == qp + Bn * M * 24 * N  # x_ref: grad_f
    assert ws(N, Bn, M, 1 << 13) == qp + Bn * M * 48 * N  # Q: grad_H and grad_f
    assert ws(N, Bn, M, (1 << 0) | (1 << 16)) == qp + Bn * M * (122 * N - 24 + 14 * N)  # x0, residual: A, b
    assert ws(N, Bn, M, (1 << 1) | (1 << 2)) == qp  # x and u read nothing
    if M == 1:
        assert ws(N, Bn, 1, 0) == L.srbd_mpc_backward_workspace_doubles(N, Bn)
    for bad in [(0, Bn, M), (33, Bn, M), (N, -1, M), (N, Bn, 0), (N, 1 << 30, 4)]:
        assert ws(*bad, 0) == 0, bad


def test_gain_workspace_at_the_deployed_horizon():
    """The gain (x0 only) at N = 10, M = 12: the QP (2256 doubles) plus 12 * 140 doubles per env -- not the
    12 x 2256 doubles of all six gradients."""
    assert _native.lib().srbd_mpc_backward_multi_workspace_doubles(10, 1, 12, 1) == 2256 + 12 * 140
