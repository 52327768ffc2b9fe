"""GPU tests of the building blocks of the DPP row kernels, one primitive per kernel.

Every other GPU test goes through a whole solver, where refinement against the full KKT and the parity
tolerances absorb a primitive that loses a few digits, routes a lane wrongly in a rarely reached case
or leaks between the two 16-lane groups of a wave. Here each primitive of csrc/dpp_rows.hpp,
csrc/srbd_common.hpp, csrc/pdipm.hpp (sym_idx .. ldlt_solve) and the free functions of
csrc/pdipm_srbd_reg.hpp runs alone, through tests/csrc/prim_harness.hip (product headers unchanged,
one `extern "C"` launcher per primitive), and is compared with the exact references of
tests/_prim_ref.py:
  * routing: small integers, every product and partial sum exact in FP64, bit equality with the
    integer reference in every active lane; the four 16-lane rows of a wave differ, lanes 12..15 hold
    poison, and each lane set of the call sites (both groups, one group alone) is run;
  * accuracy on random FP64: |err| <= gamma_{n+1} sum |c_j v_j| against the exact sum, n the number of
    terms of the primitive -- from the operation count, no measured number;
  * rcp3, the 12x12 Gauss-Jordan inverse, the 4x4 LDL^T foot solves and the integer helpers against
    what their comments claim.
The harness library carries the hash of its source and of every csrc/*.hpp: a library built from other
sources FAILS these tests (it must never test old code). Every test launches its kernels once.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _prim_ref as R

pytestmark = pytest.mark.gpu

FULL, BOTH, G0, G1 = (1 << 64) - 1, 0xFFFFFFFF, 0x0000FFFF, 0xFFFF0000
# lane sets of the call sites: `lane < 32` with both 16-lane groups active or one of them alone
# (factor_chain / solve_chain: `act` is per group); the whole wave for the primitives that have no
# lane-constant operand (their four rows then hold four different problems)
CHAIN_MASKS = [FULL, BOTH, G0, G1]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from biped_pympc_amd import build as b
    want, have = b.prim_harness_hash(), b.prim_harness_embedded_id()
    if have != want:
        pytest.fail(f"{b.PRIM_HARNESS_LIB}: embedded id {have}, sources hash to {want}: "
                    "rebuild it (__graft_entry__.build()); a stale harness would test old code")
    L = ctypes.CDLL(b.PRIM_HARNESS_LIB)
    L.prim_harness_id.restype = ctypes.c_char_p
    assert L.prim_harness_id().decode() == "srbd-prim-id:" + want
    torch.zeros(1, device="cuda")  # the context the launchers run in
    return L


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _wave_call(lib, fn, x, nout, mask=None, extra=()):
    """Run a wave launcher on x (R, 16, NIN) -- R a multiple of 4 -- and return (R, 16, NOUT) (NOUT = 1
    squeezed); lanes that stored nothing keep NaN."""
    rows = x.shape[0]
    assert rows % 4 == 0
    xin = _dev(x)
    out = torch.full((rows * 16 * nout,), float("nan"), dtype=torch.float64, device="cuda")
    args = [_ptr(xin), _ptr(out), ctypes.c_int(rows // 4)]
    if mask is not None:
        args.append(ctypes.c_ulonglong(mask))
    rc = getattr(lib, fn)(*args, *extra)
    assert rc == 0, (fn, rc)
    o = out.cpu().numpy().reshape(rows, 16, nout)
    return o[..., 0] if nout == 1 else o


def _row_active(rows, mask):
    """(R, 16) bool: lane l of row r (row r % 4 of its wave) is in the mask."""
    lane = (np.arange(rows)[:, None] % 4) * 16 + np.arange(16)[None, :]
    return np.array([(mask >> int(l)) & 1 for l in lane.ravel()], dtype=bool).reshape(lane.shape)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------- lane movers ----
@pytest.mark.parametrize("mask", CHAIN_MASKS)
def test_bc16_and_row_shifts_route_exactly(lib, mask):
    rows = 32
    rng = np.random.default_rng(41)
    v = 1.0 + np.arange(rows * 16, dtype=np.float64).reshape(rows, 16)  # 1 + lane + 64 wave: all distinct
    v[:, 12:] = R.POISON * rng.integers(1, 512, size=(rows, 4))
    act = _row_active(rows, mask)
    got = _wave_call(lib, "ph_bc16", v[..., None], 12, mask)
    assert np.array_equal(_bits(got[act]), _bits(R.bc16_ref(v)[act]))
    assert np.all(np.abs(got[act]) < R.POISON)  # no broadcast index reaches a shadow lane
    assert np.all(np.isnan(got[~act]))
    got = _wave_call(lib, "ph_shift6", v[..., None], 2, mask)
    assert np.array_equal(_bits(got[act][:, 0]), _bits(R.shl6_ref(v)[act]))
    assert np.array_equal(_bits(got[act][:, 1]), _bits(R.shr6_ref(v)[act]))
    assert np.all(np.isnan(got[~act]))


@pytest.mark.parametrize("mask", CHAIN_MASKS)
@pytest.mark.parametrize("name", list(R.WAVE_PRIMS))
def test_wave_primitive_routes_exactly(lib, name, mask):
    """Small-integer operands, poison in lanes 12..15: bit equality with the integer reference in every
    active legitimate lane, no poison term in any of them, nothing stored by an inactive lane."""
    fn, nin, nout, terms = R.WAVE_PRIMS[name]
    x = R.routing_inputs(name, 32, seed=51)
    ref = R.float_sum(terms(x)[0])
    got = _wave_call(lib, fn, x, nout, mask)
    act = _row_active(32, mask)
    legit = act & (np.arange(16)[None, :] < 12)
    assert np.array_equal(_bits(got[legit]), _bits(ref[legit])), name
    assert np.all(np.abs(got[legit]) < R.POISON), name
    assert np.all(np.isnan(got[~act])), name


@pytest.mark.parametrize("mask", [BOTH, G0, G1])
@pytest.mark.parametrize("name", ["dot_bc12", "dot_bc12_sub", "v_rows", "fmac_rows678_4<false>",
                                  "fmac_rows678_4<true>", "couple_cw_sub", "shl6"])
def test_shadow_lanes_repeat_row_11(lib, name, mask):
    """Where the product loads row 11 into lanes 12..15 (r = min(lane & 15, 11): the Dr rows, coupling
    rows and right-hand sides of RegCtx::factor_chain, pdipm_srbd_reg.hpp:793, :873, and of
    RegCtx::solve_chain, :1094), every primitive of the chains gives lane 11's result there bit for bit.
    couple_cty2 is not among them: it shifts by -6 rows, so lane 12 reads row 6 where lane 11 reads row 5;
    its only consumer, dot_bc12_sub, broadcasts from lanes 0..11."""
    if name == "shl6":
        fn, nin, nout = "ph_shift6", 1, 2
        x = R.random_fp64(np.random.default_rng(52), (32, 16, 1))
    else:
        fn, nin, nout, terms = R.WAVE_PRIMS[name]
        x = R.accuracy_inputs(name, 32, seed=52)
    x[:, 12:, :] = x[:, 11:12, :]
    got = _wave_call(lib, fn, x, nout, mask)
    if name == "shl6":
        got = got[..., 0]
    act = _row_active(32, mask)[:, 0]
    assert act.any() and np.all(np.isfinite(got[act]))
    for l in range(12, 16):
        assert np.array_equal(_bits(got[act, l]), _bits(got[act, 11])), (name, l)


@pytest.mark.parametrize("name", list(R.WAVE_PRIMS))
def test_wave_primitive_accuracy(lib, name):
    fn, nin, nout, terms = R.WAVE_PRIMS[name]
    x = R.accuracy_inputs(name, 256, seed=21)  # 256 draws (16-lane rows), the CPU-validated ones
    t, n = terms(x)
    got = _wave_call(lib, fn, x, nout, FULL)
    assert np.all(np.isfinite(got))
    ok, worst = R.within_gamma(got, t, n + 1)
    print(f"{name}: worst |err| / (gamma_{n + 1} sum|c v|) = {worst:.3f}")
    assert ok.all(), (name, worst)


@pytest.mark.parametrize("name", list(R.ROW_PRIMS))
def test_row_primitive_accuracy(lib, name):
    """Products over the compact M / C, N and G blocks against the dense expansion of the documented
    pattern; the padding no formula may read holds NaN. `cel` (a lookup, n = 1) must be exact."""
    fn, nin, n, _ = R.ROW_PRIMS[name]
    T = 4096
    x, idx = R.row_inputs(name, T, seed=22)
    xin, iin = _dev(x), _dev(idx, torch.int32)
    out = torch.full((T,), float("nan"), dtype=torch.float64, device="cuda")
    rc = getattr(lib, fn)(_ptr(xin), _ptr(iin), _ptr(out), ctypes.c_int(T))
    assert rc == 0
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got)), name
    t = R.row_terms(name, x, idx)
    ok, worst = R.within_gamma(got, t, n + 1)
    print(f"{name}: worst |err| / (gamma_{n + 1} sum|c v|) = {worst:.3f}")
    assert ok.all(), (name, worst)
    if name == "cel":
        assert np.array_equal(_bits(got), _bits(np.asarray(t[0][0])))


# -------------------------------------------------------------------------- wave reductions ----
def test_wave_sum(lib):
    rng = np.random.default_rng(61)
    vi = rng.integers(1, 2 ** 20, size=(64, 64)).astype(np.float64)  # exact: routing
    got = _wave_call(lib, "ph_wave_sum", vi.reshape(256, 16, 1), 1).reshape(64, 64)
    assert np.array_equal(got, np.broadcast_to(vi.sum(axis=1)[:, None], (64, 64)))
    # one marked lane at a time: every lane is counted exactly once
    one = np.eye(64) * np.exp2(np.arange(64) % 50)[None, :]
    got = _wave_call(lib, "ph_wave_sum", one.reshape(256, 16, 1), 1).reshape(64, 64)
    assert np.array_equal(got, np.broadcast_to(one.sum(axis=1)[:, None], (64, 64)))
    v = R.wave_inputs(seed=31)
    got = _wave_call(lib, "ph_wave_sum", v.reshape(256, 16, 1), 1).reshape(64, 64)
    assert np.array_equal(_bits(got), _bits(np.broadcast_to(got[:, :1], (64, 64))))  # wave-uniform
    ok, worst = R.within_gamma(got[:, 0], [(v[:, l], 1.0) for l in range(64)], 6)
    print(f"wave_sum: worst |err| / (gamma_6 sum|v|) = {worst:.3f}")
    assert ok.all(), worst


def test_wave_min_and_min2(lib):
    rng = np.random.default_rng(62)
    v = R.random_fp64(rng, (64, 64))           # no zeros: no mixed-sign zeros
    v[1] = np.abs(v[1])
    v[2] = np.inf
    v[3] = np.inf
    v[3, 37] = 5.0
    w =np.roll(v, 7, axis=0)[:, ::-1].copy()
    got = _wave_call(lib, "ph_wave_min", v.reshape(256, 16, 1), 1).reshape(64, 64)
    assert np.array_equal(_bits(got), _bits(np.broadcast_to(v.min(axis=1)[:, None], (64, 64))))
    assert np.all(got[2] == np.inf)
    gw = _wave_call(lib, "ph_wave_min", w.reshape(256, 16, 1), 1).reshape(64, 64)
    assert np.array_equal(_bits(gw), _bits(np.broadcast_to(w.min(axis=1)[:, None], (64, 64))))
    both = np.stack([v, w], axis=-1)           # (64, 64, 2)
    g2 = _wave_call(lib, "ph_wave_min2", both.reshape(256, 16, 2), 2).reshape(64, 64, 2)
    assert np.array_equal(_bits(g2[..., 0]), _bits(got)) and np.array_equal(_bits(g2[..., 1]), _bits(gw))
    # each lane position holds the minimum once (a lane the tree skipped would show)
    m = np.full((64, 64), 3.0) - 4.0 * np.eye(64)
    gm = _wave_call(lib, "ph_wave_min", m.reshape(256, 16, 1), 1).reshape(64, 64)
    assert np.all(gm == -1.0)


# ------------------------------------------------------------------------------------- rcp3 ----
# Measured on the MI355X (this test, seed 2024): see DESIGN.md 3.3.
RCP3_RECORDED_MISMATCHES = 0


def test_rcp3_is_correctly_rounded(lib):
    """Bit equality with IEEE 1 / d (NumPy) on 2^22 log-uniform magnitudes in [2^-500, 2^500], the powers
    of two and the neighbourhoods of 1 and 2 -- the claim of srbd_common.hpp's rcp3 comment."""
    d = R.rcp3_inputs()
    xin = _dev(d)
    out = torch.empty_like(xin)
    assert lib.ph_rcp3(_ptr(xin), _ptr(out), ctypes.c_size_t(d.size)) == 0
    got, ref = out.cpu().numpy(), 1.0 / d
    assert np.all(np.isfinite(got)) and np.array_equal(np.signbit(got), np.signbit(ref))
    ulps = R.ulp_distance(got, ref)
    bad = np.flatnonzero(ulps)
    print(f"rcp3: {bad.size} of {d.size} differ from IEEE 1/d, worst {int(ulps.max())} ulp")
    for i in bad[:2]:
        print(f"  d = {d[i].hex()}  rcp3 = {got[i].hex()}  1/d = {ref[i].hex()}")
    assert ulps.max() <= 1
    assert bad.size <= RCP3_RECORDED_MISMATCHES


# ---------------------------------------------------------------------------- 12x12 inverse ----
@pytest.fixture(scope="module")
def inverse_runs(lib):
    """Every inverse_rows12 launch of this module, once: all SPD classes and the diagonal blocks in one
    batch, for <false> and <true>, with the block in group 0 beside another block in group 1, in group 0
    alone, in group 1 alone. Returns {(swp, placement): (B, 16, 12)} rows of the block's group."""
    A = np.concatenate([R.spd_blocks()[k] for k in R.KAPPAS] + [R.diagonal_blocks()])
    B = len(A)
    other = np.roll(A, 17, axis=0)  # the neighbour group's block: a different one
    runs = {}
    for swp in (0, 1):
        def go(b0, b1, mask):
            x = R.inverse_lane_layout(b0, b1)
            xin = _dev(x)
            out = torch.full((B * 64 * 12,), float("nan"), dtype=torch.float64, device="cuda")
            rc = lib.ph_inverse_rows12(_ptr(xin), _ptr(out), ctypes.c_int(B), ctypes.c_ulonglong(mask),
                                       ctypes.c_int(swp))
            assert rc == 0
            return out.cpu().numpy().reshape(B, 64, 12)
        o = go(A, other, BOTH)
        runs[swp, "g0_pair"], runs[swp, "g1_pair_other"] = o[:, 0:16], o[:, 16:32]
        assert np.all(np.isnan(o[:, 32:]))
        o = go(A, None, G0)
        runs[swp, "g0_alone"] = o[:, 0:16]
        assert np.all(np.isnan(o[:, 16:]))
        o = go(None, A, G1)
        runs[swp, "g1_alone"] = o[:, 16:32]
        assert np.all(np.isnan(o[:, :16])) and np.all(np.isnan(o[:, 32:]))
        o = go(other, A, BOTH)
        runs[swp, "g1_pair"] = o[:, 16:32]
    assert lib.ph_inverse_rows12(None, None, ctypes.c_int(1), ctypes.c_ulonglong(1 << 32), ctypes.c_int(0)) == -1
    return runs


def test_inverse_rows12_bits_do_not_depend_on_sweep_group_or_neighbour(inverse_runs):
    """<true> equals <false> bit for bit; a block's result is the same in group 0 or group 1, whatever
    block the other group holds and when the other group is inactive; lanes 12..15 repeat lane 11."""
    base = inverse_runs[0, "g0_pair"]
    assert np.all(np.isfinite(base))
    for key, o in inverse_runs.items():
        if key[1] == "g1_pair_other":
            continue
        assert np.array_equal(_bits(o), _bits(base)), key
    oth = inverse_runs[0, "g1_pair_other"]
    assert np.array_equal(_bits(oth), _bits(inverse_runs[1, "g1_pair_other"]))
    assert np.array_equal(_bits(oth), _bits(np.roll(base, 17, axis=0)))
    for l in range(12, 16):
        assert np.array_equal(_bits(base[:, l]), _bits(base[:, 11]))


def test_inverse_rows12_of_a_diagonal_is_exact(inverse_runs):
    A = R.diagonal_blocks()
    D = inverse_runs[0, "g0_pair"][-len(A):, :12]
    d = np.einsum("bii->bi", A)
    assert np.array_equal(_bits(np.einsum("bii->bi", D)), _bits(1.0 / d))
    off = D.copy()
    off[:, np.arange(12), np.arange(12)] = 0.0
    assert np.all(off == 0.0)  # +0 or -0


def test_inverse_rows12_accuracy_against_the_restatement(inverse_runs):
    """Per condition class: max |D - A^-1| / max |A^-1| and max |A D - I| (mpmath) at most 4x the same
    quantity of the NumPy restatement on the same blocks (the project's floor rule; here it covers FMA
    versus separate rounding and the deferred row scaling). The restatement's own error is below
    12 kappa u (tests/test_prim_ref.py). Measured ratios: DESIGN.md 7b."""
    n = R.BLOCKS_PER_CLASS
    for c, kap in enumerate(R.KAPPAS):
        D = inverse_runs[0, "g0_pair"][c * n:(c + 1) * n, :12]
        gf, gr = R.inverse_errors(kap, D)
        rf, rr = R.inverse_errors(kap, R.gj_inverse_restated(R.spd_blocks()[kap]))
        print(f"inverse_rows12 kappa {kap:.0e}: forward {gf:.2e} (restated {rf:.2e}, ratio {gf / rf:.2f}); "
              f"residual {gr:.2e} (restated {rr:.2e}, ratio {gr / rr:.2f})")
        assert rf <= 12.0 * kap * R.U
        assert gf <= 4.0 * rf and gr <= 4.0 * rr, (kap, gf, rf, gr, rr)


# --------------------------------------------------------------------------- 4x4 foot blocks ----
def _ldlt(lib, a, v, mem):
    x = np.concatenate([a, v], axis=1)
    xin = _dev(x)
    out = torch.full((x.size,), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.ph_ldlt4(_ptr(xin), _ptr(out), ctypes.c_int(len(x)), ctypes.c_int(mem)) == 0
    o = out.cpu().numpy().reshape(len(x), 14)
    return o[:, :10], o[:, 10:]


@pytest.mark.parametrize("mem", [0, 1], ids=["ldlt_factor<4,true>+ldlt_solve", "ldlt_factor<4,false>+ldlt_solve_p"])
def test_foot_ldlt_is_backward_stable(lib, mem):
    """|v - A x| <= gamma_{3n+2} (|L||D||L^T|) |x| componentwise (n = 4; the standard LDL^T solve bound with
    one more rounding for the reciprocal multiply), on diag(phi) + sum W_k g_k g_k^T with W up to 1e12."""
    a, v = R.foot_blocks()
    fac, x = _ldlt(lib, a, v, mem)
    assert np.all(np.isfinite(fac)) and np.all(np.isfinite(x))
    ok, worst = R.ldlt4_backward_ok(a, v, fac, x)
    print(f"ldlt4 mem={mem}: worst residual / bound = {worst:.3f}")
    assert ok.all(), worst
    # d_0 = a_00 exactly: its slot is the correctly rounded reciprocal
    assert np.array_equal(_bits(fac[:, 0]), _bits(1.0 / a[:, 0]))


@pytest.mark.parametrize("mem", [0, 1], ids=["rcp3", "ieee"])
def test_foot_ldlt_reciprocal_slots_are_correctly_rounded(lib, mem):
    """On blocks whose pivots d_j are known exactly (every operation of the factorisation exact), the
    diagonal slots hold the correctly rounded 1 / d_j: via rcp3 for <4, true>, IEEE division for <4, false>."""
    a, v, d = R.exact_pivot_blocks()
    fac, x = _ldlt(lib, a, v, mem)
    for j in range(4):
        assert np.array_equal(_bits(fac[:, R.sym_idx(j, j)]), _bits(1.0 / d[:, j])), j
    rf, rx = R.ldlt4_restated(a, v)
    off = [R.sym_idx(r, c) for r in range(4) for c in range(r)]
    assert np.array_equal(fac[:, off], rf[:, off])  # L: every operation exact
    assert np.array_equal(fac[:, off] * 8.0, np.round(fac[:, off] * 8.0))


# --------------------------------------------------------------------------- integer helpers ----
def test_div12_div6_exhaustive(lib):
    """div12(c) == c // 12 for every 0 <= c < 2^17 and div6(c) == c // 6 for every 0 <= c < 2^16, the
    ranges their comment documents. (This test found both short of them: c * 43691 >> 19 wrapped its
    32-bit product from c = 98304 on, and the int that HIP's __umul24 returns made div6's shift arithmetic
    from c = 49153 on; the kernels pass c < 1024.)"""
    bad = {}
    for fn, n, q in (("ph_div12", 1 << 17, 12), ("ph_div6", 1 << 16, 6)):
        out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        assert getattr(lib, fn)(_ptr(out), ctypes.c_int(n)) == 0
        wrong = torch.nonzero(out.cpu() != torch.arange(n, dtype=torch.int32) // q).ravel()
        if wrong.numel():
            bad[fn] = (int(wrong.numel()), int(wrong[0]))
    assert not bad, f"(count, first wrong c): {bad}"


def test_m24(lib):
    g = torch.arange(1 << 12, dtype=torch.int32, device="cuda")
    a = [g.repeat_interleave(1 << 12)]
    b = [g.repeat(1 << 12)]
    i = torch.arange(1 << 16, dtype=torch.int32, device="cuda")
    for c in (6, 12, 13, 16, 24, 28, 36, 78, 80, 86, 122, 255):  # 12 i, 78 i, m24(lane, ...) past 2^12
        a.append(i)
        b.append(torch.full_like(i, c))
        a.append(torch.full_like(i, c))
        b.append(i)
    a, b = torch.cat(a).contiguous(), torch.cat(b).contiguous()
    out = torch.full_like(a, -1)
    assert lib.ph_m24(_ptr(a), _ptr(b), _ptr(out), ctypes.c_size_t(a.numel())) == 0
    assert torch.equal(out, a * b)


def test_foot_maps_are_mutually_inverse(lib):
    out = torch.full((32,), -9, dtype=torch.int32, device="cuda")
    assert lib.ph_foot(_ptr(out)) == 0
    o = out.cpu().numpy()
    foot_of, foot_pos, colj = o[:12], o[12:24], o[24:32].reshape(2, 4)
    assert sorted(colj.ravel().tolist()) == [0, 1, 2, 3, 4, 5, 7, 10]
    for f in range(2):
        for p in range(4):
            j = colj[f, p]
            assert (foot_of[j], foot_pos[j]) == (f, p) and j == R.foot_colj(f, p)
    assert [j for j in range(12) if foot_of[j] < 0] == [6, 8, 9, 11]
