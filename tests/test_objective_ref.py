"""The exact objective reference (tests/_objective_ref.py) against the reference's own formula, and
the parts of the objective feature that need no GPU: the new C-ABI symbols and the config default.

qpth returns 0.5 x^T H x + f^T x with a dense H (mpc_controller_qpth.py:136); evaluated in float64
that is at most 3 roundings per term and two sums of 24N terms, inside the bound the GPU kernels are
held to (gamma_{24N+4} S, tests/_objective_ref.py).
"""
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from biped_pympc_amd import _native, build, layout
from biped_pympc_amd.utils.synthetic import make_workload
from oracle import oracle
from tests import _objective_ref as R


def test_gamma_and_exact_value_on_a_hand_case():
    assert R.gamma(1) == Fraction(1, 2 ** 53 - 1)
    assert R.gamma(244) == Fraction(244, 2 ** 53 - 244)
    # J = (1/2 * 3 * 2 + 1) * 2 + (1/2 * 0.5 * (-4) + 0.25) * (-4) = 8 + 3 = 11; S = 6 + 2 + 4 + 1 = 13
    J, S = R.objective_exact([[3.0, 0.5]], [[1.0, 0.25]], [[2.0, -4.0]])
    assert J == [Fraction(11)] and S == [Fraction(13)]
    # values no float64 sum could hold: 2^60 + 2^-60 - 2^60 keeps the small term
    J, S = R.objective_exact([[0.0, 0.0, 0.0]], [[2.0 ** 60, 2.0 ** -60, -2.0 ** 60]], [[1.0, 1.0, 1.0]])
    assert J == [Fraction(1, 2 ** 60)] and S == [2 ** 61 + Fraction(1, 2 ** 60)]
    r = R.bound_ratios([11.0, 11.0 + 2.0 ** -40], [[3.0, 0.5]] * 2, [[1.0, 0.25]] * 2, [[2.0, -4.0]] * 2)
    assert r[0] == 0.0 and r[1] > 1.0
    assert np.isinf(R.bound_ratios([np.nan], [[3.0]], [[1.0]], [[2.0]])[0])


@pytest.mark.parametrize("N", [1, 10])
def test_dense_formula_on_oracle_solutions_is_within_the_bound(N):
    B, K = 8, 5
    wl = make_workload(B, N, seed=40 + N, random_gait=True)
    H, f = oracle.qp_former(N, wl.inputs)[:2]
    x = oracle.mpc_solve(N, K, wl.inputs, y0=1.0)[0]
    assert np.all(np.isfinite(x)) and np.abs(x).max() > 0.0
    Hp, Hi = layout.ccs_H(N)
    J = np.empty(B)
    for e in range(B):
        Hd = layout.to_dense(H[e], Hp, Hi, (24 * N, 24 * N))
        assert np.array_equal(Hd, np.diag(H[e]))  # H's CCS pattern is the diagonal
        J[e] = 0.5 * x[e] @ Hd @ x[e] + f[e] @ x[e]
    ratios = R.bound_ratios(J, H, f, x)
    print(f"N={N}: |J - J_exact| / (gamma S) max {ratios.max():.3e}")
    assert np.all(ratios <= 1.0), ratios
    # the bound is tight enough to tell a wrong formula, e.g. x^T H x without the 1/2
    assert np.all(R.bound_ratios(J + 0.5 * np.einsum("be,be,be->b", x, H, x), H, f, x) > 1.0)


def test_library_exports_the_info_entry_points():
    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path()], capture_output=True, text=True,
                         check=True)
    exports = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
    assert {"srbd_pdipm_info", "srbd_mpc_solve_fused_info", "srbd_mpc_step_info"} <= exports
    # the earlier generations stay
    assert {"srbd_pdipm_ex", "srbd_mpc_solve_fused_ex", "srbd_mpc_step_ex", "srbd_pdipm", "srbd_mpc_step"} <= exports


def test_solve_info_mirror_and_config_default():
    import ctypes

    from biped_pympc_amd.controller import MPCConf
    assert MPCConf().compute_cost is False
    assert [n for n, _ in _native.SolveInfo._fields_] == ["status", "objective", "objective_f32"]
    assert ctypes.sizeof(_native.SolveInfo) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert _native.solve_info() is None
    info = _native.solve_info(None, 64, None)
    assert info.status is None and info.objective == 64 and info.objective_f32 is None
