"""CPU references for the building blocks of the DPP row kernels (tests/test_gpu_primitives.py).

For every primitive wrapped by tests/csrc/prim_harness.hip this module holds
  * its meaning as a list of product terms over a dense expansion of its operands (`*_terms`): summed
    in exact integer arithmetic (`exact_sum`) it is the reference of the accuracy tests, summed in
    float64 on small integers (every product and partial sum exact) that of the routing tests;
  * where a bound needs one, a plain NumPy float64 restatement of the same recurrence with separate
    multiply and add and the same pivot order (`gj_inverse_restated`, `ldlt4_restated`);
  * the input generators and the bounds, shared by the CPU validation (tests/test_prim_ref.py) and
    the GPU tests, so the inputs are known to be passable before a GPU is involved.

Layout of a wave primitive's operands: (R, 16, NIN) -- R 16-lane DPP rows (four per wavefront), lane
l of a row, operand k; the harness reads them as in + NIN * thread. u = 2^-53, gamma_n = n u / (1 - n u).
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -53
POISON = float(2 ** 30)  # a routed poison operand is a multiple of this; legitimate integers stay < 2^9


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------ exact integer arithmetic ----
_S = 160  # a double x is the integer x * 2^_S (inputs down to 2^-100 in magnitude, or zero)


def to_int(x, scale=_S):
    """float64 array -> object array of Python integers x * 2^scale (exact; asserts it is)."""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(np.isfinite(x))
    m, e = np.frexp(x)
    mi = np.ldexp(m, 53).astype(np.int64)
    sh = e.astype(np.int64) - 53 + scale
    assert np.all((sh >= 0) | (mi == 0)), "operand below the exact range"
    sh = np.where(mi == 0, 0, sh)
    p2 = np.array([1 << int(s) for s in sh.ravel()], dtype=object).reshape(sh.shape)
    return mi.astype(object) * p2


def exact_sum(terms):
    """(sum_k a_k b_k, sum_k |a_k b_k|) as integers scaled by 2^(2 _S), from a list of (a, b) float64
    arrays broadcastable against each other."""
    tot, mag = 0, 0
    for a, b in terms:
        p = to_int(a) * to_int(b)
        tot = tot + p
        mag = mag + abs(p)
    return tot, mag


def float_sum(terms):
    """The same sum in float64: exact when every operand is a small integer."""
    tot = 0.0
    for a, b in terms:
        tot = tot + np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    return tot


def within_gamma(got, terms, n):
    """|got - exact| <= gamma_n sum |a_k b_k| elementwise, decided in integers
    (gamma_n = n / (2^53 - n)). Returns (ok array, worst err / bound)."""
    tot, mag = exact_sum(terms)
    err = abs(to_int(got) * (1 << _S) - tot)
    ok = np.frompyfunc(lambda e, m: e * ((1 << 53) - n) <= n * m, 2, 1)(err, mag).astype(bool)
    ratio = np.frompyfunc(lambda e, m: float(e * ((1 << 53) - n)) / float(n * m) if m else (0.0 if e == 0 else np.inf),
                          2, 1)(err, mag).astype(np.float64)
    return ok, float(ratio.max())


# ------------------------------------------------------------------------------ lane movers ----
def bc16_ref(v):
    """v (R, 16) -> (R, 16, 12): out[r, l, k] = v[r, k]."""
    return np.broadcast_to(v[:, None, :12], (v.shape[0], 16, 12)).copy()


def shl6_ref(v):
    """lane l <- lane l + 6 of its row; past the row's end the bound-controlled read gives 0."""
    out = np.zeros_like(v)
    out[:, :10] = v[:, 6:]
    return out


def shr6_ref(v):
    out = np.zeros_like(v)
    out[:, 6:] = v[:, :10]
    return out


# ------------------------------------------------------- term lists of the wave primitives ----
# each returns (terms, n): n the number of terms of one output element
def dot_bc12_terms(x):  # c[12], v
    return [(x[..., j], x[:, j, 12][:, None]) for j in range(12)], 12


def dot_bc12_sub_terms(x):  # c[12], v, init
    return [(x[..., 13], 1.0)] + [(-x[..., j], x[:, j, 12][:, None]) for j in range(12)], 13


def rows678_terms(x, neg):  # x[4], v[4], c6, c7, c8 -> 4 outputs
    s = -1.0 if neg else 1.0
    return [(x[..., 0:4], 1.0)] + [(s * x[:, 6 + k, 4:8][:, None, :], x[..., 8 + k][..., None]) for k in range(3)], 4


def v_rows_terms(x):  # Dr[12], d, a0, a1, a2, b -> V[12]
    R = x.shape[0]
    Dr = x[..., :12]
    d = x[:, :12, 12][:, None, :]                      # C[c][c], held by lane c
    terms = [(Dr, d)]
    for k in range(3):                                 # rows c < 3: + Dr[6 + k] C[c][6 + k]
        a = np.zeros((R, 1, 12))
        a[:, 0, :3] = x[:, :3, 13 + k]
        terms.append((Dr[..., 6 + k][..., None], a))
    b = np.zeros((R, 1, 12))                           # rows 3 <= c < 6: + Dr[c + 6] C[c][c + 6]
    b[:, 0, 3:6] = x[:, 3:6, 16]
    pick = np.zeros((R, 16, 12))
    pick[..., 3:6] = Dr[..., 9:12]
    terms.append((pick, b))
    return terms, 4


def couple_cw_sub_terms(x):  # d, b, a0, a1, a2, w, base: base - (C w)_r
    w = x[..., 5]
    return [(x[..., 6], 1.0), (-x[..., 0], w), (-x[..., 1], shl6_ref(w))] + \
           [(-x[..., 2 + k], w[:, 6 + k][:, None]) for k in range(3)], 6


def couple_cty2_terms(x):  # d, b, a0, a1, a2, y: (C^T y)_r
    y = x[..., 5]
    return [(x[..., 0], y), (x[..., 1], shr6_ref(y))] + [(x[..., 2 + k], y[:, k][:, None]) for k in range(3)], 5


WAVE_PRIMS = {  # name -> (launcher, NIN, NOUT, terms)
    "dot_bc12": ("ph_dot_bc12", 13, 1, dot_bc12_terms),
    "dot_bc12_sub": ("ph_dot_bc12_sub", 14, 1, dot_bc12_sub_terms),
    "fmac_rows678_4<false>": ("ph_rows678", 11, 4, functools.partial(rows678_terms, neg=False)),
    "fmac_rows678_4<true>": ("ph_rows678_neg", 11, 4, functools.partial(rows678_terms, neg=True)),
    "v_rows": ("ph_v_rows", 17, 12, v_rows_terms),
    "couple_cw_sub": ("ph_couple_cw_sub", 7, 1, couple_cw_sub_terms),
    "couple_cty2": ("ph_couple_cty2", 6, 1, couple_cty2_terms),
}


def couple_pattern(name, x):
    """The product's coupling rows (RegCtx::factor_chain, pdipm_srbd_reg.hpp:800-804, and
    RegCtx::solve_chain, :1103-1116): C w has a* on rows r < 3 and b on rows 3..5; C^T y has a* on rows
    6..8 and b on rows >= 9; zero elsewhere."""
    l = np.arange(16)
    if name == "couple_cw_sub":
        ma, mb = l < 3, (l >= 3) & (l < 6)
    elif name == "couple_cty2":
        ma, mb = (l >= 6) & (l < 9), (l >= 9) & (l < 12)
    else:
        return x
    x = x.copy()
    x[:, ~mb, 1] = 0.0
    for k in range(3):
        x[:, ~ma, 2 + k] = 0.0
    return x


def routing_inputs(name, rows, seed):
    """Small-integer operands (every product and partial sum exact in FP64): legitimate values in
    [1, 2^9), different in every lane and every 16-lane row; lanes 12..15 hold poison, multiples of 2^30."""
    _, nin, _, _ = WAVE_PRIMS[name]
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 2 ** 9, size=(rows, 16, nin)).astype(np.float64)
    x[:, 12:, :] = POISON * rng.integers(1, 2 ** 9, size=(rows, 4, nin))
    return couple_pattern(name, x)


def random_fp64(rng, shape):
    """Mixed sign, magnitudes log-uniform over 2^-20 .. 2^20 (sign-cancelling sums included)."""
    return rng.choice([-1.0, 1.0], size=shape) * np.exp2(rng.uniform(-20.0, 20.0, size=shape))


def accuracy_inputs(name, rows, seed):
    _, nin, _, _ = WAVE_PRIMS[name]
    return random_fp64(np.random.default_rng(seed), (rows, 16, nin))


# ------------------------------------------------- products over the compact blocks (memory) ----
kNdS, kGfPad, kGfSize = 13, 4, 68  # pdipm_srbd_reg.hpp


def expand_compact(mc):
    """(T, 24) compact M / C block -> dense (T, 12, 12): [0..11] the diagonal, [12 + 3 r + k] = (r, 6 + k)
    for r < 3, [21 + r - 3] = (r, r + 6) for 3 <= r < 6 (pdipm_srbd_reg.hpp header)."""
    M = np.zeros((mc.shape[0], 12, 12))
    for r in range(12):
        M[:, r, r] = mc[:, r]
    for r in range(3):
        for k in range(3):
            M[:, r, 6 + k] = mc[:, 12 + 3 * r + k]
    for r in range(3, 6):
        M[:, r, r + 6] = mc[:, 21 + r - 3]
    return M


def foot_colj(f, a):
    return a + 3 * f if a < 3 else 7 + 3 * f


def g_other(k):
    return 0 if k < 2 else (1 if k < 4 else (3 if k < 6 else 0))


def g_row(k):
    return 4 * k + kGfPad * (k >> 3)


def nd_pattern():
    """Structural nonzeros of the stage u-block N (12 x 12): rows {0,1,2,6,7,8} dense, rows 3 + p and
    9 + p only the force columns p and 3 + p."""
    P = np.zeros((12, 12), dtype=bool)
    P[[0, 1, 2, 6, 7, 8], :] = True
    for p in range(3):
        for c in (p, 3 + p):
            P[3 + p, c] = P[9 + p, c] = True
    return P


def gf_pattern():
    """(16, 4) structural nonzeros of G's rows over the foot positions (fx, fy, fz, my)."""
    P = np.zeros((16, 4), dtype=bool)
    for k in range(16):
        P[k, 2] = True
        if (k & 7) < 6:
            P[k, g_other(k & 7)] = True
    return P


ROW_PRIMS = {  # name -> (launcher, NIN, n terms, index choices)
    "drow12": ("ph_drow12", 24, 12, [0]),
    "mrow_slot<0>": ("ph_mrow_slot0", 36, 4, [0, 1, 2, 6, 7, 8]),
    "mrow_slot<1>": ("ph_mrow_slot1", 36, 2, [3, 4, 5, 9, 10, 11]),
    "mcol": ("ph_mcol", 36, 4, list(range(12))),
    "ncol<true>": ("ph_ncol_force", 12 * kNdS + 12, 8, list(range(12))),
    "ncol<false>": ("ph_ncol", 12 * kNdS + 12, 6, [6, 7, 8, 9, 10, 11]),  # the force rows are compiled out
    "grow4": ("ph_grow4", kGfSize + 12, 2, list(range(16))),
    "cel": ("ph_cel", 24, 1, list(range(144))),
}


def row_inputs(name, T, seed, poison=np.nan):
    """(x (T, NIN), idx (T,)) random FP64 operands of a memory primitive; the slots its documented
    pattern leaves out hold structural zeros where the product stores zeros, and `poison` in the padding
    no formula may read (N's 13th column, the gap between G's two feet)."""
    _, nin, _, choices = ROW_PRIMS[name]
    rng = np.random.default_rng(seed)
    x = random_fp64(rng, (T, nin))
    idx = np.array([choices[t % len(choices)] for t in range(T)], dtype=np.int32)
    if name.startswith("ncol"):
        nd = x[:, :12 * kNdS].reshape(T, 12, kNdS).copy()
        nd[:, :, :12] *= nd_pattern()[None]
        nd[:, :, 12] = poison
        x[:, :12 * kNdS] = nd.reshape(T, 12 * kNdS)
    if name == "grow4":
        gf = x[:, :kGfSize]
        keep = np.zeros(kGfSize, dtype=bool)
        P = gf_pattern()
        for k in range(16):
            keep[g_row(k):g_row(k) + 4] = True
        pad = ~keep
        for k in range(16):
            gf[:, g_row(k):g_row(k) + 4] *= P[k][None]
        gf[:, pad] = poison
    return x, idx


def row_terms(name, x, idx):
    """Terms of one output per thread from the dense expansion of the compact operands."""
    T = x.shape[0]
    t = np.arange(T)
    if name == "drow12":
        return [(x[:, j], x[:, 12 + j]) for j in range(12)]
    if name.startswith("mrow_slot"):
        M, v = expand_compact(x[:, :24]), x[:, 24:36]
        return [(M[t, idx, c], v[:, c]) for c in range(12)]
    if name == "mcol":
        M, v = expand_compact(x[:, :24]), x[:, 24:36]
        return [(M[t, r, idx], v[:, r]) for r in range(12)]
    if name.startswith("ncol"):
        Nd, v = x[:, :12 * kNdS].reshape(T, 12, kNdS), x[:, 12 * kNdS:]
        return [(Nd[t, r, idx], v[:, r]) for r in range(12)]
    if name == "grow4":
        gf, xu = x[:, :kGfSize], x[:, kGfSize:]
        G = np.zeros((T, 12))  # dense row idx[t] of G over the 12 u columns
        for k in range(16):
            sel = idx == k
            for o in range(4):
                if gf_pattern()[k, o]:
                    G[sel, foot_colj(k >> 3, o)] = gf[sel, g_row(k) + o]
        return [(G[:, c], xu[:, c]) for c in range(12)]
    if name == "cel":
        M = expand_compact(x[:, :24])
        return [(M[t, idx // 12, idx % 12], 1.0)]
    raise KeyError(name)


# -------------------------------------------------------------------------------------- rcp3 ----
def rcp3_inputs(seed=2024):
    """2^22 values of log-uniform magnitude in [2^-500, 2^500] and random sign; the exact powers of two
    of that range; 1 + k 2^-52 and 2 - k 2^-52 for k = 1..4096; the last three in both signs."""
    rng = np.random.default_rng(seed)
    n = 1 << 22
    d = rng.choice([-1.0, 1.0], size=n) * np.exp2(rng.uniform(-500.0, 500.0, size=n))
    p2 = np.ldexp(1.0, np.arange(-500, 501))
    k = np.arange(1, 4097, dtype=np.float64)
    edge = np.concatenate([p2, 1.0 + k * 2.0 ** -52, 2.0 - k * 2.0 ** -52])
    return np.concatenate([d, edge, -edge])


def ulp_distance(a, b):
    """Distance in units in the last place between finite doubles of the same sign."""
    return np.abs(np.asarray(a).view(np.int64) - np.asarray(b).view(np.int64))


# ------------------------------------------------------------------------- 12 x 12 inverse ----
KAPPAS = (1e1, 1e4, 1e8, 1e12)
BLOCKS_PER_CLASS = 64


@functools.lru_cache(maxsize=None)
def spd_blocks(seed=7):
    """{kappa: (64, 12, 12)} SPD blocks Q diag(lambda) Q^T, symmetrised, lambda log-spaced over kappa."""
    rng = np.random.default_rng(seed)
    out = {}
    for kap in KAPPAS:
        A = np.empty((BLOCKS_PER_CLASS, 12, 12))
        for b in range(BLOCKS_PER_CLASS):
            Q, _ = np.linalg.qr(rng.standard_normal((12, 12)))
            lam = np.logspace(0.0, np.log10(kap), 12) * np.exp2(rng.integers(-8, 9))
            M = (Q * lam) @ Q.T
            A[b] = 0.5 * (M + M.T)
        out[kap] = A
    return out


def diagonal_blocks(seed=8, n=16):
    """The identity and n - 1 random positive diagonals (magnitudes over 2^-30 .. 2^30)."""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, 12, 12))
    A[0] = np.eye(12)
    for b in range(1, n):
        A[b][np.diag_indices(12)] = np.exp2(rng.uniform(-30.0, 30.0, size=12))
    return A


def gj_inverse_restated(A):
    """NumPy float64 restatement of inverse_rows12 (dpp_rows.hpp): Gauss-Jordan on the diagonal in
    pivot order 0..11, rows kept unscaled with a deferred scale 1 / pivot, multiply and add rounded
    separately, the reciprocal by IEEE division. A (B, 12, 12) -> (B, 12, 12)."""
    S = np.array(A, dtype=np.float64, copy=True)
    sc = np.ones(S.shape[:2])
    for k in range(12):
        pk = S[:, k, :].copy()
        inv = 1.0 / pk[:, k]
        t = S[:, :, k] * inv[:, None]
        t[:, k] = 0.0                                   # the pivot lane's update is a no-op
        for j in range(12):
            if j != k:
                S[:, :, j] = S[:, :, j] - pk[:, j][:, None] * t
        S[:, :, k] = t
        S[:, k, k] = -1.0
        sc[:, k] = inv
    return S * (-sc)[:, :, None]


@functools.lru_cache(maxsize=None)
def spd_inverses_mp(seed=7):
    """{kappa: list of mpmath matrices A^-1} at 240 bits (computed once per process)."""
    import mpmath as mp
    out = {}
    with mp.workprec(240):
        for kap, A in spd_blocks(seed).items():
            out[kap] = [mp.inverse(mp.matrix(a.tolist())) for a in A]
    return out


def inverse_errors(kap, D, seed=7):
    """(max |D - A^-1| / max |A^-1|, max |A D - I|) over the class's blocks, evaluated in mpmath."""
    import mpmath as mp
    A = spd_blocks(seed)[kap]
    fwd, res = 0.0, 0.0
    with mp.workprec(240):
        eye = mp.eye(12)
        for a, d, inv in zip(A, D, spd_inverses_mp(seed)[kap]):
            dm = mp.matrix(d.tolist())
            e = dm - inv
            fwd = max(fwd, float(max(abs(v) for v in e) / max(abs(v) for v in inv)))
            r = mp.matrix(a.tolist()) * dm - eye
            res = max(res, float(max(abs(v) for v in r)))
    return fwd, res


def inverse_lane_layout(blocks0, blocks1):
    """(W, 64, 12) operands of W wavefronts: group 0 (lanes 0..15) holds blocks0[w], group 1 (lanes
    16..31) blocks1[w], one row per lane, lanes 12..15 of a group shadowing row 11; lanes 32..63 (never
    active) hold NaN. A None argument leaves that group NaN."""
    W = len(blocks0 if blocks0 is not None else blocks1)
    x = np.full((W, 64, 12), np.nan)
    rows = np.minimum(np.arange(16), 11)
    if blocks0 is not None:
        x[:, 0:16, :] = blocks0[:, rows, :]
    if blocks1 is not None:
        x[:, 16:32, :] = blocks1[:, rows, :]
    return x


# ----------------------------------------------------------------------------- 4 x 4 foot blocks ----
def sym_idx(a, b):
    return a * (a + 1) // 2 + b if a >= b else b * (b + 1) // 2 + a


def foot_blocks(seed=11, n=256):
    """(a (n, 10) packed lower, v (n, 4)): diag(phi) + sum_k W_k g_k g_k^T over a foot's 8 inequality rows
    (g_k: fz and row k's other column, g_other), phi log-uniform in [1e-8, 1e2], W_k log-uniform in
    [1e-4, 1e12] -- the regime of pdipm.hpp ldlt_factor's comment."""
    rng = np.random.default_rng(seed)
    phi = 10.0 ** rng.uniform(-8.0, 2.0, size=(n, 4))
    A = np.zeros((n, 4, 4))
    for c in range(4):
        A[:, c, c] = phi[:, c]
    for k in range(8):
        W = 10.0 ** rng.uniform(-4.0, 12.0, size=n)
        g = np.zeros((n, 4))
        g[:, 2] = rng.uniform(-1.0, 1.0, size=n)
        if k < 6:
            g[:, g_other(k)] = rng.uniform(-1.0, 1.0, size=n)
        A += W[:, None, None] * g[:, :, None] * g[:, None, :]
    A = 0.5 * (A + A.transpose(0, 2, 1))
    a = np.stack([A[:, r, c] for r in range(4) for c in range(r + 1)], axis=1)
    v = random_fp64(rng, (n, 4))
    return a, v


def exact_pivot_blocks(seed=12, n=256):
    """(a (n, 10), v (n, 4), d (n, 4)): blocks L D L^T whose factorisation is exact in FP64 whatever the
    contraction: every pivot but one (j = block % 4) is a power of two, that one an odd integer < 2^20
    with a zero column below it in L, and L's other entries are small dyadic rationals. The computed d_j
    are then exactly `d`, so the stored reciprocal slots must be the correctly rounded 1 / d_j."""
    rng = np.random.default_rng(seed)
    L = np.zeros((n, 4, 4))
    d = np.exp2(rng.integers(-6, 7, size=(n, 4)).astype(np.float64))
    for b in range(n):
        j = b % 4
        d[b, j] = float(2 * rng.integers(1, 2 ** 19) + 1)
        L[b] = np.tril(rng.integers(-8, 9, size=(4, 4)) / 8.0, -1)
        L[b, :, j] = 0.0
        L[b][np.diag_indices(4)] = 1.0
    A = np.einsum("bik,bk,bjk->bij", L, d, L)  # exact: small dyadic operands
    a = np.stack([A[:, r, c] for r in range(4) for c in range(r + 1)], axis=1)
    v = rng.integers(-64, 65, size=(n, 4)).astype(np.float64)
    return a, v, d


def ldlt4_restated(a, v):
    """NumPy float64 restatement of ldlt_factor<4> + ldlt_solve<4> (pdipm.hpp): the same recurrences,
    multiply and add rounded separately, reciprocals by IEEE division. Returns (factors (n, 10), x (n, 4))."""
    a = np.array(a, dtype=np.float64, copy=True)
    n = 4
    d = np.zeros((a.shape[0], n))
    P = lambda i, j: i * (i + 1) // 2 + j  # noqa: E731
    for j in range(n):
        dj = a[:, P(j, j)].copy()
        for k in range(j):
            dj = dj - a[:, P(j, k)] * a[:, P(j, k)] * d[:, k]
        d[:, j] = dj
        inv = 1.0 / dj
        for i in range(j + 1, n):
            w = a[:, P(i, j)].copy()
            for k in range(j):
                w = w - a[:, P(i, k)] * a[:, P(j, k)] * d[:, k]
            a[:, P(i, j)] = w * inv
        a[:, P(j, j)] = inv
    x = np.zeros((a.shape[0], n))
    for i in range(n):
        y = np.array(v[:, i], copy=True)
        for k in range(i):
            y = y - a[:, P(i, k)] * x[:, k]
        x[:, i] = y
    for i in range(n):
        x[:, i] = x[:, i] * a[:, P(i, i)]
    for i in range(n - 1, -1, -1):
        for k in range(i + 1, n):
            x[:, i] = x[:, i] - a[:, P(k, i)] * x[:, k]
    return a, x


def ldlt4_backward_ok(a, v, fac, x):
    """Componentwise backward error of the 4 x 4 LDL^T solves, in mpmath:
    |v - A x| <= gamma_{3 n + 2} (|L| |D| |L^T|) |x| with n = 4, L the computed unit lower factor and
    D = 1 / (the stored reciprocal slots). Returns (ok (n,), worst residual / bound)."""
    import mpmath as mp
    n = 4
    g = None
    ok = np.zeros(a.shape[0], dtype=bool)
    worst = 0.0
    with mp.workprec(240):
        g = mp.mpf(3 * n + 2) * mp.mpf(2) ** -53
        g = g / (1 - g)
        for b in range(a.shape[0]):
            A = mp.matrix(n, n)
            L = mp.eye(n)
            D = mp.zeros(n, n)
            for r in range(n):
                for c in range(n):
                    A[r, c] = mp.mpf(float(a[b, sym_idx(r, c)]))
                for c in range(r):
                    L[r, c] = mp.mpf(float(fac[b, sym_idx(r, c)]))
                D[r, r] = 1 / mp.mpf(float(fac[b, sym_idx(r, r)]))
            xm = mp.matrix([mp.mpf(float(t)) for t in x[b]])
            vm = mp.matrix([mp.mpf(float(t)) for t in v[b]])
            res = vm - A * xm
            La = L.apply(abs)
            bound = g * (La * D.apply(abs) * La.T * xm.apply(abs))
            good = True
            for r in range(n):
                good = good and abs(res[r]) <= bound[r]
                if bound[r] != 0:
                    worst = max(worst, float(abs(res[r]) / bound[r]))
            ok[b] = good
    return ok, worst


# --------------------------------------------------------------------------- wave reductions ----
def wave_sum_restated(v):
    """NumPy float64 restatement of wave_sum's DPP tree (srbd_common.hpp wave_reduce) on (W, 64): quad
    swaps, half-row and row mirrors, then row 0 into row 1 and row 2 into row 3 (row_bcast:15), rows
    0 + 1 into row 3 (row_bcast:31); lane 63 holds the result. Six levels of additions."""
    l = np.arange(64)
    v = np.asarray(v, dtype=np.float64)
    v = v + v[:, l ^ 1]
    v = v + v[:, l ^ 2]
    v = v + v[:, (l & ~7) | (7 - (l & 7))]
    v = v + v[:, (l & ~15) | (15 - (l & 15))]
    r = v[:, 15::16]
    return (r[:, 3] + r[:, 2]) + (r[:, 1] + r[:, 0])


def wave_inputs(seed, W=64):
    return random_fp64(np.random.default_rng(seed), (W, 64))
