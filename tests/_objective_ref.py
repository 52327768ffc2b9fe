"""Exact reference of the QP objective J = sum_e (H_e x_e / 2 + f_e) x_e (include/srbd_mpc.h
srbd_solve_info) and the rounding bound a kernel's J is held to (test infrastructure only).

H is the 24N nonzeros of the QP's Hessian (its CCS pattern is the diagonal), f the linear term, x a
primal iterate, all float64. The exact value is formed in ``fractions.Fraction`` from the floats'
exact binary values, so it has no rounding at all; S = sum_e (|H_e x_e^2 / 2| + |f_e x_e|) is the
scale the error of any floating-point evaluation is proportional to.

The bound: an evaluation that forms each of the 24N terms with at most 4 roundings and adds them in
any order has |J - J_exact| <= gamma_k S with k = 24N + 4, gamma_k = k u / (1 - k u), u = 2^-53
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1 and section 4.2: each
term carries at most 4 + (24N - 1) factors (1 + delta), |delta| <= u).
"""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)


def gamma(k: int) -> Fraction:
    return (k * U) / (1 - k * U)


def objective_exact(H, f, x):
    """Per env (rows of the (B, 24N) arrays): (J_exact, S) as lists of Fraction."""
    H, f, x = (np.atleast_2d(np.asarray(a, np.float64)) for a in (H, f, x))
    assert H.shape == f.shape == x.shape, (H.shape, f.shape, x.shape)
    Js, Ss = [], []
    for he, fe, xe in zip(H.tolist(), f.tolist(), x.tolist()):
        J = S = Fraction(0)
        for h, fv, xv in zip(he, fe, xe):
            xq = Fraction(xv)
            quad = Fraction(h) * xq * xq / 2
            lin = Fraction(fv) * xq
            J += quad + lin
            S += abs(quad) + abs(lin)
        Js.append(J)
        Ss.append(S)
    return Js, Ss


def bound_ratios(J, H, f, x) -> np.ndarray:
    """|J - J_exact| / (gamma_{24N+4} S) per env, evaluated exactly; <= 1 passes. A non-finite J
    gives inf; an env with S = 0 gives 0 if J is exactly J_exact (= 0), inf otherwise."""
    J = np.asarray(J, np.float64).reshape(-1)
    Je, S = objective_exact(H, f, x)
    assert len(Je) == J.size, (len(Je), J.size)
    g = gamma(np.atleast_2d(x).shape[1] + 4)
    out = np.empty(J.size)
    for e, (j, je, s) in enumerate(zip(J.tolist(), Je, S)):
        if not np.isfinite(j):
            out[e] = np.inf
            continue
        err = abs(Fraction(j) - je)
        out[e] = float(err / (g * s)) if s != 0 else (0.0 if err == 0 else np.inf)
        if err > g * s and out[e] <= 1.0:  # the comparison itself is exact: never rounded into the bound
            out[e] = np.nextafter(1.0, 2.0)
    return out
