"""The backward entry points at the C-ABI boundary, without a GPU: bad arguments return an error code
and a message, an empty batch is a successful no-op, the workspace size is the QP plus its gradients.
No compute call is made here."""
import ctypes

from biped_pympc_amd import _native


def test_backward_bad_arguments_return_errors_without_touching_the_gpu():
    L = _native.lib()
    n17, n10, n6, n4 = (_native.ptr_array([0] * k) for k in (17, 10, 6, 4))
    one = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced
    # srbd_pdipm_backward
    assert L.srbd_pdipm_backward(0, 4, n10, one, n6, None, None) != 0
    assert "srbd_pdipm_backward: bad arguments" in _native.last_error()
    assert L.srbd_pdipm_backward(33, 4, n10, one, n6, None, None) != 0
    assert L.srbd_pdipm_backward(10, -1, n10, one, n6, None, None) != 0
    assert L.srbd_pdipm_backward(10, 4, None, one, n6, None, None) != 0
    assert L.srbd_pdipm_backward(10, 4, n10, one, None, None, None) != 0
    assert L.srbd_pdipm_backward(10, 4, n10, one, n6, None, None) != 0
    assert "null input" in _native.last_error()
    some = _native.ptr_array([8, 8, 8, 0, 0, 0, 8, 8, 8, 8])  # f, h, b may be null; grad_x may not
    assert L.srbd_pdipm_backward(10, 4, some, None, n6, None, None) != 0
    assert "null grad_x" in _native.last_error()
    assert L.srbd_pdipm_backward(10, 0, n10, None, n6, None, None) == 0
    # srbd_qp_former_backward
    assert L.srbd_qp_former_backward(0, 4, n17, n6, n17, None) != 0
    assert "srbd_qp_former_backward: bad arguments" in _native.last_error()
    assert L.srbd_qp_former_backward(10, 4, n17, None, n17, None) != 0
    assert L.srbd_qp_former_backward(10, 4, n17, n6, None, None) != 0
    assert L.srbd_qp_former_backward(10, 4, n17, n6, n17, None) != 0
    assert "null input" in _native.last_error()
    assert L.srbd_qp_former_backward(10, 0, n17, n6, n17, None) == 0
    # srbd_mpc_backward
    assert L.srbd_mpc_backward(40, 4, n17, n4, one, one, n17, None, None) != 0
    assert "srbd_mpc_backward: bad arguments" in _native.last_error()
    assert L.srbd_mpc_backward(10, 4, n17, None, one, one, n17, None, None) != 0
    assert L.srbd_mpc_backward(10, 4, n17, n4, one, None, n17, None, None) != 0
    assert "null workspace" in _native.last_error()
    assert L.srbd_mpc_backward(10, 4, n17, n4, one, one, n17, None, None) != 0  # null iterate
    assert L.srbd_mpc_backward(10, 0, n17, n4, None, None, n17, None, None) == 0


def test_backward_workspace_is_the_qp_and_its_gradients():
    L = _native.lib()
    assert L.srbd_mpc_backward_workspace_doubles(10, 4096) == 2 * L.srbd_mpc_workspace_doubles(10, 4096)
    assert L.srbd_mpc_backward_workspace_doubles(10, 4096) == 2 * 4096 * 2256
    assert L.srbd_mpc_backward_workspace_doubles(0, 4) == 0 and L.srbd_mpc_backward_workspace_doubles(33, 4) == 0
    for N in (1, 2, 10, 32):  # an upper bound of what the one-seed composition carves for any request
        for B in (1, 16, 4096):
            assert L.srbd_mpc_backward_multi_workspace_doubles(N, B, 1, 0) <= L.srbd_mpc_backward_workspace_doubles(N, B)
    assert _native.STATUS_UNSUPPORTED == 8
