"""CPU validation of tests/_prim_ref.py: every NumPy float64 restatement against its exact or
high-precision reference, under the very bounds tests/test_gpu_primitives.py applies to the HIP
primitives -- so the inputs are known to be passable before a GPU is involved, and a failure on the
GPU is the primitive's, not the test's. No GPU, no native library.
"""
import numpy as np
import pytest

from tests import _prim_ref as R

ROWS = 256  # 16-lane rows per accuracy draw (64 wavefronts)


@pytest.mark.parametrize("name", list(R.WAVE_PRIMS))
def test_routing_operands_are_exact_and_poison_free(name):
    """The small-integer operands: the float64 sum of the terms is the integer sum (every product and
    partial sum below 2^53), and no legitimate lane's reference carries a poison term."""
    _, nin, nout, terms = R.WAVE_PRIMS[name]
    x = R.routing_inputs(name, 16, seed=5)
    t, _ = terms(x)
    ref = R.float_sum(t)
    tot, mag = R.exact_sum(t)
    assert np.all(np.frompyfunc(lambda m: m < (1 << (53 + 2 * R._S)), 1, 1)(mag[:, :12]).astype(bool))
    assert np.all(R.to_int(ref[:, :12]) * (1 << R._S) == tot[:, :12])
    assert np.all(np.abs(ref[:, :12]) < R.POISON)
    assert np.all(ref[:, :12] == np.round(ref[:, :12]))


@pytest.mark.parametrize("name", list(R.WAVE_PRIMS))
def test_wave_primitive_restatement_within_its_bound(name):
    """Term-by-term float64 summation (multiply and add rounded separately) of the random FP64 draws
    stays within gamma_{n+1} sum |c_j v_j| of the exact sum."""
    _, nin, nout, terms = R.WAVE_PRIMS[name]
    x = R.accuracy_inputs(name, ROWS, seed=21)
    t, n = terms(x)
    ok, worst = R.within_gamma(R.float_sum(t), t, n + 1)
    assert ok.all(), (name, worst)
    nz = sum(((np.asarray(a) != 0) & (np.asarray(b) != 0)).astype(int) + np.zeros(ok.shape, dtype=int) for a, b in t)
    assert nz.max() == n, (name, nz.max())  # the stated term count is the primitive's, not an upper bound


@pytest.mark.parametrize("name", list(R.ROW_PRIMS))
def test_row_primitive_restatement_within_its_bound(name):
    _, nin, n, _ = R.ROW_PRIMS[name]
    x, idx = R.row_inputs(name, 4096, seed=22)
    t = R.row_terms(name, x, idx)
    ok, worst = R.within_gamma(R.float_sum(t), t, n + 1)
    assert ok.all(), (name, worst)
    # n is exactly the largest number of structural nonzeros of one output under the documented pattern:
    # a term count can be neither under- nor over-stated (an over-stated one would loosen the bound)
    nz = sum(((np.asarray(a) != 0) & (np.asarray(b) != 0)).astype(int) for a, b in t)
    assert nz.max() == n, (name, nz.max())


def test_bound_rejects_a_dropped_term_and_a_lost_digit():
    """The accuracy bound can fail: a result without its smallest term, or off by 2^-40 relative."""
    x = R.accuracy_inputs("dot_bc12", 16, seed=3)
    t, n = R.dot_bc12_terms(x)
    good = R.float_sum(t)
    assert R.within_gamma(good, t, n + 1)[0].all()
    assert not R.within_gamma(R.float_sum(t[:-1]), t, n + 1)[0].all()
    mag = sum(np.abs(a * b) for a, b in t)
    assert not R.within_gamma(good + mag * 2.0 ** -40, t, n + 1)[0].any()


def test_wave_sum_restatement_within_gamma6():
    v = R.wave_inputs(seed=31)
    ok, worst = R.within_gamma(R.wave_sum_restated(v), [(v[:, l], 1.0) for l in range(64)], 6)
    assert ok.all(), worst


def test_rcp3_inputs_are_normal_and_cover_the_claim():
    d = R.rcp3_inputs()
    assert d.size == (1 << 22) + 2 * (1001 + 2 * 4096)
    a = np.abs(d)
    assert np.all(np.isfinite(d)) and a.min() >= 2.0 ** -500 and a.max() <= 2.0 ** 500
    inv = 1.0 / d
    assert np.all(np.abs(inv) >= 2.0 ** -500)  # no subnormal reciprocal either
    assert R.ulp_distance(np.float64(1.0), np.nextafter(1.0, 2.0)) == 1


def test_gauss_jordan_restatement_meets_the_input_condition():
    """The restatement's own forward error stays below 12 kappa u on every class (a condition on the
    inputs of the GPU test, which holds the kernel to 4x the restatement's error), it inverts diagonal
    blocks exactly, and it is row-for-row the kernel's recurrence: independent per block."""
    for kap in R.KAPPAS:
        D = R.gj_inverse_restated(R.spd_blocks()[kap])
        fwd, res = R.inverse_errors(kap, D)
        assert fwd <= 12.0 * kap * R.U, (kap, fwd)
        assert fwd >= 1e-3 * kap * R.U, (kap, fwd)  # the class is as ill-conditioned as it says
        assert res <= 12.0 * 12.0 * kap * R.U, (kap, res)
    A = R.diagonal_blocks()
    D = R.gj_inverse_restated(A)
    d = np.einsum("bii->bi", A)
    assert np.array_equal(np.einsum("bii->bi", D), 1.0 / d)
    off = D.copy()
    off[:, np.arange(12), np.arange(12)] = 0.0
    assert np.all(off == 0.0)


def test_ldlt_restatement_is_backward_stable_and_exact_on_exact_blocks():
    a, v = R.foot_blocks()
    assert a.shape == (256, 10)
    fac, x = R.ldlt4_restated(a, v)
    ok, worst = R.ldlt4_backward_ok(a, v, fac, x)
    assert ok.all(), worst
    # the bound can fail: a solution off by 1e-9 relative is not a backward-stable solve of these blocks
    assert not R.ldlt4_backward_ok(a, v, fac, x * (1.0 + 1e-9))[0].all()
    # blocks whose pivots are known exactly: the stored slots are the correctly rounded reciprocals
    a, v, d = R.exact_pivot_blocks()
    fac, x = R.ldlt4_restated(a, v)
    for j in range(4):
        assert np.array_equal(fac[:, R.sym_idx(j, j)], 1.0 / d[:, j]), j
    odd = d[np.arange(256), np.arange(256) % 4]
    assert np.all(odd % 2 == 1) and np.all(odd > 1)  # reciprocals that do need rounding
