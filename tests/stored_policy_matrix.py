"""The calls that read what a solve leaves behind (propagate_covariance, cost_to_go, solution_vjp / solution_jvp,
solution_vjp_data, get_gain_active_set, simulate_policy, eval_policy) on the one-wave-per-instance backend as a table: the shapes
at which k_cov_wide, k_ctg_wide and the sensitivity kernels take a path the shape lists of their own test files do not reach.
Shared by tests/test_stored_policy_matrix.py (the LDS sizes, the dispatch, and the conditions on the INPUTS, on the CPU oracle
alone) and tests/test_stored_policy_matrix_gpu.py (the device against the numpy yardsticks of those files).

 - covw_lds_doubles / ctgw_lds_doubles restate covariance.h and cost_to_go.h; LDS holds the bytes each case is in the table for.
 - CASES: batch 3, N = 5, one solve each, every case "shared" (one row of weights and bounds for the batch) and "pi".
     wide(40,6)   np = 48 with state padding, mq = 8; BOX on the controls and three LINEAR rows on knots 1 .. N-1 (sc with
                  np = 48; the three-tile strip of gemm_rows under the leading dimensions of both kernels, Mm's odd np + 1
                  included); cost-to-go just UNDER the 64 KB a kernel gets unasked, covariance just over.  Its box-only copy
                  (BOXONLY) runs what refuses rows: cost_to_go mode 1, solution_vjp_data, get_gain_active_set.
     wide(48,13)  n = np = 48, no pad, mq = 16; state bounds up to the terminal knot; [A | B] does not fit the LDS of the sweeps
                  (49 * 61 * 8 B * 4 > 64 KB): k_sens_wide reads the dynamics from memory, sens-data runs one wave a block.
     wide(12,20)  np = 16 < mp = 32: Tt of k_cov_wide is sized by mp, Y = K S is two 16-row strips over one tile; mq = 20;
                  m > 16: no factors of Quu, the second such shape beside (30, 25); state bounds up to the terminal knot.
     wide(48,32)  np = 48, mp = mq = 32: the largest shape the solve fits; above 64 KB and below (64, 16).
 - guard(): what the inputs must satisfy for a comparison on them to mean anything.
Seeds and bounds below were tuned on the ORACLE until the guards hold; nothing here depends on the device."""
import functools

import numpy as np

import evaluate_ref as ER
import solution_data_ref as DR
from helpers import REF_OPTS
from wide_matrix import _pad16, at_penalty_cap

B, N = 3, 5
OPTS = dict(REF_OPTS, iterations=60)      # test_covariance_gpu.OPTS: the options of make_solver
LDS_UNASKED = 65536                       # the dynamic LDS a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize
BOXONLY = "-box"


def covw_lds_doubles(n, m):
    """covariance.h covw_lds_doubles: Mt, S [np][np], Tt [max(np, mp)][np], Kl, Bl [mq][np], Kt [np][mp]"""
    np_, mp, mq = _pad16(n), _pad16(m), (m + 3) & ~3
    return 2 * np_ * np_ + max(np_, mp) * np_ + 2 * mq * np_ + np_ * mp


def ctgw_lds_doubles(n, m):
    """cost_to_go.h ctgw_lds_doubles: Pm, Tt [np][np], Mm [np][np + 1], Kl, Bl [mq][np]"""
    np_, mq = _pad16(n), (m + 3) & ~3
    return 2 * np_ * np_ + np_ * (np_ + 1) + 2 * mq * np_


# (n, m) -> (bytes of k_cov_wide, bytes of k_ctg_wide): the sizes each case is in the table for, and (64, 16) of the sibling files
LDS = {(40, 6): (67584, 61824), (48, 13): (73728, 67968), (12, 20): (17408, 11392), (48, 32): (92160, 80256), (64, 16): (122880, 115200)}

# Tuning, all of it on the oracle (tests/test_stored_policy_matrix.py holds the result).  seed: of evaluate_ref.make_case; the
# control bounds are 0.5 + 0.5 * random per instance ("pi") or 0.9 ("shared"): every instance of every case ends with a control on
# its bound at the first seed tried.  xb: the state bound (upper on the even states, lower on every third), on knots 1 .. N-1.
# What made the values of test_covariance_gpu.build miss:
#  - its state bound of 6 (wide(30,25)) leaves every state side slack here; from knot 0 on, a bound below 3.5 is violated by the
#    given x_0 of some instance, which then ends at the penalty cap (status 3 or 4).  From knot 1 on, 2.0 at (48, 13) puts 14 to 20
#    state sides in the set of every instance, and 1.5 at (12, 20) some in one instance ("shared") or two ("pi"), all solved in
#    at most 30 of the 60 iterations.
#  - its LINEAR offset of 6 (wide(17,5): A z <= 6 + random) leaves all three rows of (40, 6) slack; at 2 one instance of "shared"
#    still has a zero dual block; at 1 every instance has a nonzero one.
TUNE = {
    "wide(40,6)": dict(n=40, m=6, seed=61, xb=None, rows=True),
    "wide(48,13)": dict(n=48, m=13, seed=62, xb=2.0, rows=False),
    "wide(12,20)": dict(n=12, m=20, seed=63, xb=1.5, rows=False),
    "wide(48,32)": dict(n=48, m=32, seed=64, xb=None, rows=False),
}
ROWS_OFFSET = 1.0       # the LINEAR rows of wide(40,6): A z <= ROWS_OFFSET + random
CASES = list(TUNE)
RUNS = [(s, pi) for s in CASES for pi in (False, True)]
IDS = [s + ("-pi" if pi else "-shared") for s, pi in RUNS]
ROWS_CASES = [s for s in CASES if TUNE[s]["rows"]]
BOX_RUNS = [(s + BOXONLY if s in ROWS_CASES else s, pi) for s, pi in RUNS]      # every case without rows: what mode 1 and the getter take
BOX_IDS = [s + ("-pi" if pi else "-shared") for s, pi in BOX_RUNS]


def shape(name):
    t = TUNE[name[:-len(BOXONLY)] if name.endswith(BOXONLY) else name]
    return t["n"], t["m"]


def build(name, pi):
    """(Case, to_problem keywords, index of the constraint sc is asked for or None, None), as test_covariance_gpu.build"""
    if name.endswith(BOXONLY):
        cs, kw, _, _ = build(name[:-len(BOXONLY)], pi)
        cs.cons = cs.cons[:1]
        return cs, kw, None, None
    t = TUNE[name]
    n, m = t["n"], t["m"]
    sh = () if pi else ("cost", "box")
    cs = ER.make_case(B, n, m, N, t["seed"], per_instance_cost=pi)
    ub = 0.5 + 0.5 * np.random.default_rng(t["seed"] + 100).random((B, m)) if pi else 0.9
    if t["xb"] is not None:
        ER.add_box(cs, ub, x_bnd=t["xb"], k0=1, k1=N - 1)
    else:
        ER.add_box(cs, ub)
    if not t["rows"]:
        return cs, dict(shared=sh), None, None
    rng = np.random.default_rng(t["seed"] + 200)
    A = np.concatenate([0.02 * rng.standard_normal((B, N - 1, 3, n)), rng.standard_normal((B, N - 1, 3, m))], axis=-1)
    ER.add_rows(cs, "lin", A, -ROWS_OFFSET - rng.random((B, N - 1, 3)), 1, N - 1)
    return cs, dict(shared=sh), 1, None


@functools.lru_cache(maxsize=None)
def guard(name, pi):
    """The case on the oracle, solved with the options of the handles: dict(status (B,), iterations (B,), capped, on_bound (B,):
    a control at its bound with a positive dual on that side, state_sides (B,): state sides of the box with a positive dual,
    lin (B,): a nonzero dual on the LINEAR block (None without one))."""
    import oracle_py as oracle
    oracle.build()
    cs, _, con, _ = build(name, pi)
    n = cs.n
    out = dict(status=[], iterations=[], capped=False, on_bound=[], state_sides=[], lin=[] if con is not None else None)
    for b in range(cs.B):
        o = ER.oracle_of(oracle, cs, b)
        o.set_opts(oracle.default_opts(**OPTS))
        o.set_controls(cs.Uref[b])
        so = o.solve()
        out["status"].append(so.status); out["iterations"].append(so.iterations)
        out["capped"] = out["capped"] or at_penalty_cap(so)
        box = cs.cons[0]
        one = ER.sub_case(cs, b)
        lhi, llo = DR.stack_duals(one, o.duals(0).reshape(1, box.k1 - box.k0 + 1, 2, n + cs.m))
        U = o.controls()
        hi, lo = box.zmax[b, n:], box.zmin[b, n:]
        at_hi = (U >= hi - 1e-6 * np.abs(hi)) & (lhi[0, :-1, n:] > 0)
        at_lo = (U <= lo + 1e-6 * np.abs(lo)) & (llo[0, :-1, n:] > 0)
        out["on_bound"].append(bool(at_hi.any() or at_lo.any()))
        out["state_sides"].append(int((lhi[0, :, :n] > 0).sum() + (llo[0, :, :n] > 0).sum()))
        if con is not None:
            out["lin"].append(bool(np.any(o.duals(con) != 0.0)))
    return {k: (np.array(v) if isinstance(v, list) else v) for k, v in out.items()}
