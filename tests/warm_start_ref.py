"""The selection rule of altro_batch_warm_start in plain Python, and the inputs the tests of the warm start share.
Shared by tests/test_warm_start_api.py (the rule on hand-made arrays; the GPU tests' inputs are decidable and exercise the
choice) and tests/test_warm_start_gpu.py (the device against the rule and against the numpy yardstick of evaluate_ref).

The rule: merit = fma(rho, c_max, J) with ONE rounding; best = +Inf, chosen = -1; the incumbent (last column, when included) is
visited first, then the candidates 0 .. ncand-1 in turn; a candidate takes over only if merit < best.  -2 marks an instance the
active mask leaves out.  The fused multiply-add is computed exactly in rationals and rounded once (float(Fraction) is
correctly rounded); a non-finite operand needs no rounding, IEEE arithmetic gives its value."""
from fractions import Fraction

import numpy as np

import evaluate_ref as ER

RHOS = (0.0, 1e3, 1e6)
CASES = {
    "16-box(12,4)": (ER.case_16_box, {}),
    "16-soc(6,3)": (ER.case_16_soc, {}),
    "wide-rows(20,5)": (ER.case_wide_rows, dict(shared=("dyn", "cost", "box", 1, 2))),
    "wide-ltv(12,12)": (ER.case_wide_ltv, dict(per_knot_dyn=True)),
    "wide-cone(7,3)": (ER.case_wide_cone, dict(shared=("box", 2))),
    "wide-box(30,25)": (ER.case_wide_box, dict(shared=("dyn", "box"))),
    "wide-limits(64,32)": (ER.case_wide_limits, {}),
}
"""the cases of tests/test_evaluate_gpu.py"""


def fma(a, b, c):
    """a * b + c rounded once"""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return float("inf") if Fraction(a) * Fraction(b) + Fraction(c) > 0 else float("-inf")


def merits(J, c, rho):
    J, c = np.asarray(J, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return np.array([[fma(rho, c[b, q], J[b, q]) for q in range(J.shape[1])] for b in range(J.shape[0])]).reshape(J.shape)


def select(J, c, rho, include_current, active=None):
    """chosen (B,) int32 of J, c (B, ncand + include_current)"""
    J = np.asarray(J, dtype=np.float64)
    M = merits(J, c, rho)
    B, nc1 = J.shape
    ncand = nc1 - (1 if include_current else 0)
    out = np.empty(B, dtype=np.int32)
    for b in range(B):
        best, w = float("inf"), -1
        for q in ([ncand] if include_current else []) + list(range(ncand)):
            if M[b, q] < best:
                best, w = M[b, q], q
        out[b] = -2 if active is not None and not active[b] else w
    return out


def yardstick(cs, U, Uinc):
    """numpy scores of the candidates U (B, nc, N-1, m) with the incumbent's controls Uinc (B, N-1, m) as the last column:
    (J, bound 3, c_max, bound 4), each (B, nc + 1)"""
    Ua = np.concatenate([U, Uinc[:, None]], axis=1)
    X = ER.rollout(cs, Ua)
    J, Jb = ER.cost(cs, X, Ua)
    c, cb = ER.violation(cs, X, Ua)
    return J, Jb, c, cb


def decided(cs, U, Uinc, rho):
    """(winner per instance by the numpy yardstick, incumbent = index nc; gap between the best and the second-best merit;
    2 * the largest summed rounding bound 3 + rho * bound 4 of the instance's columns)"""
    J, Jb, c, cb = yardstick(cs, U, Uinc)
    M = J + rho * c
    order = np.argsort(M, axis=1)
    best, second = np.take_along_axis(M, order[:, :1], 1)[:, 0], np.take_along_axis(M, order[:, 1:2], 1)[:, 0]
    return order[:, 0], second - best, 2 * (Jb + rho * cb).max(axis=1)


def six_candidates(cs, Uinc):
    """the GPU tests' candidates (B, 6, N-1, m): the three of ER.candidates(cs, 5), a copy of candidate 0, a copy of the
    incumbent's controls, and one holding a NaN"""
    U3 = ER.candidates(cs, 5)
    bad = U3[:, 2].copy()
    bad[:, cs.N // 2, 0] = np.nan
    return np.ascontiguousarray(np.stack([U3[:, 0], U3[:, 1], U3[:, 2], U3[:, 0], Uinc, bad], axis=1))


def expected_of_six(win3, ncand=6):
    """winner among the six candidates + incumbent from the yardstick's winner among the three + incumbent (index 3): the
    duplicates (3, 4) lose their ties and the NaN candidate (5) never wins"""
    return np.where(win3 == 3, ncand, win3).astype(np.int32)
