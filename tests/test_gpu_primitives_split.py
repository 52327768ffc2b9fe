"""GPU tests of the column-split chain primitives (csrc/dpp_rows.hpp, csrc/pdipm_srbd_reg.hpp), one
primitive per kernel, through tests/csrc/prim_harness_split.hip.

A split primitive holds a 12x12 block's columns {0,1,2,6,7,8} in half A of the wave (lanes 0..31: the
two twisted groups in DPP rows 0 and 1) and {3,4,5,9,10,11} in half B (lanes 32..63), lanes i and
i + 32 sharing a row. Each is compared with the primitive it replaces, run through the existing
harness (tests/csrc/prim_harness.hip) on the same operands:
  * the inverse, v_rows and the rows-6..8 term bit for bit (the same FMA sequence per element);
  * the dots: both halves return the same bits, exact on small integers, and within
    gamma_13 sum |c_j v_j| of the exact sum on random FP64 (12 or 13 terms in another association --
    the bound form of tests/test_gpu_primitives.py, from the operation count).
Lane sets: both groups, or one group alone (both of its halves: the launchers refuse a half alone).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _prim_ref as R

pytestmark = pytest.mark.gpu

ACOLS, BCOLS = [0, 1, 2, 6, 7, 8], [3, 4, 5, 9, 10, 11]
COLS = np.array([ACOLS, BCOLS])
BOTH, G0, G1 = (1 << 64) - 1, 0x0000FFFF0000FFFF, 0xFFFF0000FFFF0000
MASKS = [BOTH, G0, G1]
OLD = {BOTH: 0xFFFFFFFF, G0: 0x0000FFFF, G1: 0xFFFF0000}  # the same groups on lanes 0..31


@pytest.fixture(scope="module")
def libs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from biped_pympc_amd import build as b
    out = []
    for want, path, idf in ((b.prim_harness_hash(), b.PRIM_HARNESS_LIB, "prim_harness_id"),
                            (b.prim_harness_split_hash(), b.PRIM_SPLIT_LIB, "prim_harness_split_id")):
        have = b.prim_harness_embedded_id(path)
        if have != want:
            pytest.fail(f"{path}: embedded id {have}, sources hash to {want}: rebuild it "
                        "(__graft_entry__.build()); a stale harness would test old code")
        L = ctypes.CDLL(path)
        getattr(L, idf).restype = ctypes.c_char_p
        assert getattr(L, idf)().decode() == "srbd-prim-id:" + want
        out.append(L)
    torch.zeros(1, device="cuda")
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _call(lib, fn, x, nout, mask, extra=()):
    """x (W, 64, NIN) -> (W, 64, NOUT); lanes that stored nothing keep NaN."""
    W = x.shape[0]
    xin = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    out = torch.full((W * 64 * nout,), float("nan"), dtype=torch.float64, device="cuda")
    rc = getattr(lib, fn)(ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_int(W),
                          ctypes.c_ulonglong(mask), *extra)
    assert rc == 0, (fn, rc)
    return out.cpu().numpy().reshape(W, 64, nout)


def _active(mask):
    return np.array([(mask >> l) & 1 for l in range(64)], dtype=bool)


def _to_split(x):
    """(W, 32, 12 + k) whole-row operands on lanes 0..31 -> (W, 64, 6 + k): each half takes its columns
    of the first 12 operands, the rest is copied to both halves."""
    return np.concatenate([np.concatenate([x[:, :, COLS[h]], x[:, :, 12:]], axis=2) for h in (0, 1)], axis=1)


def _from_split(o):
    """(W, 64, 6) -> (W, 32, 12): a row reassembled from its two halves."""
    W = o.shape[0]
    full = np.empty((W, 32, 12))
    full[:, :, ACOLS] = o[:, :32]
    full[:, :, BCOLS] = o[:, 32:]
    return full


def test_launchers_refuse_a_half_alone(libs):
    for fn in ("phs_inverse", "phs_v_rows", "phs_rows678", "phs_rows678_neg", "phs_dot", "phs_dot_sub"):
        for mask in (0xFFFFFFFF, 0x0000FFFF, 1 << 63):
            assert getattr(libs[1], fn)(None, None, ctypes.c_int(1), ctypes.c_ulonglong(mask)) == -1


# ---------------------------------------------------------------------------- 12x12 inverse ----
@pytest.fixture(scope="module")
def inverse_blocks():
    return np.concatenate([R.spd_blocks()[k] for k in R.KAPPAS] + [R.diagonal_blocks()])


def _inverse_both(libs, b0, b1, mask):
    """The block pair through inverse_rows12<false> (lanes 0..31) and through the split sweep (64 lanes):
    ((W, 32, 12), (W, 32, 12) reassembled, raw (W, 64, 6))."""
    x = R.inverse_lane_layout(b0, b1)  # (W, 64, 12), lanes 32..63 NaN
    W = len(x)
    xin = torch.from_numpy(x).cuda()
    out = torch.full((W * 64 * 12,), float("nan"), dtype=torch.float64, device="cuda")
    rc = libs[0].ph_inverse_rows12(ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_int(W),
                                   ctypes.c_ulonglong(OLD[mask]), ctypes.c_int(0))
    assert rc == 0
    old = out.cpu().numpy().reshape(W, 64, 12)[:, :32]
    xs = x.copy()
    xs[:, 32:] = xs[:, :32]  # lanes i and i + 32 hold the same row
    raw = _call(libs[1], "phs_inverse", xs, 6, mask)
    return old, _from_split(raw), raw


def test_split_inverse_equals_inverse_rows12_bit_for_bit(libs, inverse_blocks):
    """All SPD classes (kappa 1e1 .. 1e12) and the diagonal blocks: with another block in the other
    group, the results of both groups equal inverse_rows12<false>'s bit for bit, and the shadow lanes
    12..15 of every DPP row repeat lane 11."""
    A = inverse_blocks
    old, new, raw = _inverse_both(libs, A, np.roll(A, 17, axis=0), BOTH)
    assert np.all(np.isfinite(old))
    assert np.array_equal(_bits(new), _bits(old))
    for row in range(4):
        for l in range(12, 16):
            assert np.array_equal(_bits(raw[:, 16 * row + l]), _bits(raw[:, 16 * row + 11])), (row, l)


def test_split_inverse_does_not_depend_on_group_or_neighbour(libs, inverse_blocks):
    A = inverse_blocks
    base = _inverse_both(libs, A, np.roll(A, 17, axis=0), BOTH)[1][:, :16]
    _, n, raw = _inverse_both(libs, A, None, G0)  # group 0 alone, the other group NaN and inactive
    assert np.array_equal(_bits(n[:, :16]), _bits(base))
    assert np.all(np.isnan(raw[:, ~_active(G0)]))
    _, n, raw = _inverse_both(libs, None, A, G1)
    assert np.array_equal(_bits(n[:, 16:]), _bits(base))
    assert np.all(np.isnan(raw[:, ~_active(G1)]))
    _, n, _ = _inverse_both(libs, np.roll(A, 5, axis=0), A, BOTH)
    assert np.array_equal(_bits(n[:, 16:]), _bits(base))


# ------------------------------------------------------- v_rows and the rows-6..8 term ----
def _poison(rng, shape):
    return R.POISON * rng.integers(1, 2 ** 9, size=shape).astype(np.float64)


def _v_rows_split_operands(x, rng):
    """v_rows operands (W, 32, 17) = Dr[12], d, a0, a1, a2, b on lanes 0..31 -> v_rows_split's
    (W, 64, 10) = Dl[6], d, x0, x1, x2: half A keeps its lanes' (d, a0, a1, a2); in half B lane c < 3 of a
    DPP row holds row c + 3's d and its b in x_c (0 in the other two), lanes 6..8 row 9..11's d; every
    operand no formula may read is poison."""
    W = x.shape[0]
    s = np.empty((W, 64, 10))
    s[:, :32, :6] = x[:, :, ACOLS]
    s[:, 32:, :6] = x[:, :, BCOLS]
    s[:, :32, 6:] = x[:, :, 12:16]
    s[:, 32:, 6:] = _poison(rng, (W, 32, 4))
    for g in (0, 1):
        for c in range(3):
            s[:, 32 + 16 * g + c, 6] = x[:, 16 * g + c + 3, 12]
            s[:, 32 + 16 * g + c, 7:] = 0.0
            s[:, 32 + 16 * g + c, 7 + c] = x[:, 16 * g + c + 3, 16]
            s[:, 32 + 16 * g + 6 + c, 6] = x[:, 16 * g + 9 + c, 12]
    return s


@pytest.mark.parametrize("mask", MASKS)
def test_split_v_rows_equals_v_rows(libs, mask):
    """Small-integer routing operands, poison in lanes 12..15; bit equality with v_rows on the same
    operands in every legitimate active lane, and no poison term in any."""
    rng = np.random.default_rng(71)
    x = R.routing_inputs("v_rows", 64, seed=71).reshape(32, 32, 17)  # 32 waves x 2 groups
    old = _call(libs[0], "ph_v_rows", np.concatenate([x, np.zeros_like(x)], axis=1), 12, OLD[mask])[:, :32]
    new = _from_split(_call(libs[1], "phs_v_rows", _v_rows_split_operands(x, rng), 6, mask))
    legit = (_active(mask)[:32]) & (np.arange(32) % 16 < 12)
    assert legit.any() and np.all(np.isfinite(old[:, legit]))
    assert np.array_equal(_bits(new[:, legit]), _bits(old[:, legit]))
    assert np.all(np.abs(new[:, legit]) < R.POISON)
    ref = R.float_sum(R.v_rows_terms(x.reshape(64, 16, 17))[0]).reshape(32, 32, 12)
    assert np.array_equal(_bits(new[:, legit]), _bits(ref[:, legit]))


def test_split_v_rows_halves_do_not_read_each_other(libs):
    """Either half's result with the other half all poison."""
    rng = np.random.default_rng(72)
    x = R.routing_inputs("v_rows", 64, seed=72).reshape(32, 32, 17)
    s = _v_rows_split_operands(x, rng)
    base = _call(libs[1], "phs_v_rows", s, 6, BOTH)
    legit = np.arange(32) % 16 < 12
    for h in (0, 1):
        p = s.copy()
        other = slice(32, 64) if h == 0 else slice(0, 32)
        p[:, other] = _poison(rng, p[:, other].shape)
        got = _call(libs[1], "phs_v_rows", p, 6, BOTH)[:, 32 * h:32 * h + 32]
        assert np.array_equal(_bits(got[:, legit]), _bits(base[:, 32 * h:32 * h + 32][:, legit]))
        assert np.all(np.abs(got[:, legit]) < R.POISON)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("neg", [False, True])
def test_split_rows678_equals_fmac_rows678_4(libs, neg, mask):
    """Six slots per lane against fmac_rows678_4 on slots 0..3 and 2..5 of the same operands; the two
    halves hold different problems, lanes 12..15 poison."""
    rng = np.random.default_rng(73)
    x = rng.integers(1, 2 ** 9, size=(32, 64, 15)).astype(np.float64)  # x[6], v[6], c6, c7, c8
    for row in range(4):
        x[:, 16 * row + 12:16 * row + 16] = _poison(rng, (32, 4, 15))
    new = _call(libs[1], "phs_rows678_neg" if neg else "phs_rows678", x, 6, mask)
    act = _active(mask)
    legit = act & (np.arange(64) % 16 < 12)
    assert np.all(np.isnan(new[:, ~act]))
    assert np.all(np.abs(new[:, legit]) < R.POISON)
    fn = "ph_rows678_neg" if neg else "ph_rows678"
    for h in (0, 1):  # the old harness runs lanes 0..31: one half of the wave at a time
        xh = x[:, 32 * h:32 * h + 32]
        for lo in (0, 2):
            o = np.concatenate([xh[:, :, lo:lo + 4], xh[:, :, 6 + lo:10 + lo], xh[:, :, 12:]], axis=2)
            old = _call(libs[0], fn, np.concatenate([o, np.zeros_like(o)], axis=1), 4, OLD[mask])[:, :32]
            lg = legit[32 * h:32 * h + 32]
            assert np.array_equal(_bits(new[:, 32 * h:32 * h + 32][:, lg, lo:lo + 4]), _bits(old[:, lg]))


# ------------------------------------------------------------------------------------ dots ----
def _dot_operands(name, x):
    """dot_bc12 / dot_bc12_sub operands (W * 2, 16, 13 or 14) -> (W, 64, 7 or 8)"""
    return _to_split(x.reshape(-1, 32, x.shape[-1]))


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", ["dot_bc12", "dot_bc12_sub"])
def test_split_dots_route_exactly(libs, name, mask):
    """Small integers (every partial sum exact): bit equality with the integer reference, the same bits in
    both halves, no poison term (lanes 12..15 hold poison)."""
    _, nin, _, terms = R.WAVE_PRIMS[name]
    x = R.routing_inputs(name, 64, seed=74)
    ref = R.float_sum(terms(x)[0]).reshape(32, 32)
    got = _call(libs[1], "phs_dot" if name == "dot_bc12" else "phs_dot_sub", _dot_operands(name, x), 1, mask)[..., 0]
    act = _active(mask)
    legit = act[:32] & (np.arange(32) % 16 < 12)
    assert np.all(np.isnan(got[:, ~act]))
    assert np.array_equal(_bits(got[:, :32][:, legit]), _bits(ref[:, legit]))
    assert np.array_equal(_bits(got[:, 32:][:, legit]), _bits(ref[:, legit]))
    assert np.all(np.abs(got[:, :32][:, legit]) < R.POISON)


@pytest.mark.parametrize("name", ["dot_bc12", "dot_bc12_sub"])
def test_split_dots_accuracy_and_identical_halves(libs, name):
    """Random FP64: both halves return identical bits (shadow lanes included, which repeat lane 11 where
    they hold row 11), and |err| <= gamma_13 sum |c_j v_j| against the exact sum (dot_bc12_sub: init
    included in the sum). A term passes through at most 6 roundings here (its FMA, one more FMA of its
    accumulator, two additions of the accumulators, the cross-half addition), so gamma_13, the bound of the
    unsplit 12-term dot, holds for both forms."""
    _, nin, _, terms = R.WAVE_PRIMS[name]
    x = R.accuracy_inputs(name, 256, seed=21)
    x[:, 12:, :] = x[:, 11:12, :]
    t, n = terms(x)
    got = _call(libs[1], "phs_dot" if name == "dot_bc12" else "phs_dot_sub", _dot_operands(name, x), 1, BOTH)[..., 0]
    assert np.all(np.isfinite(got))
    assert np.array_equal(_bits(got[:, :32]), _bits(got[:, 32:]))
    g = got[:, :32].reshape(256, 16)
    for l in range(12, 16):
        assert np.array_equal(_bits(g[:, l]), _bits(g[:, 11]))
    ok, worst = R.within_gamma(g, t, 13)
    print(f"{name} split: worst |err| / (gamma_13 sum|c v|) = {worst:.3f}")
    assert ok.all(), (name, worst)
