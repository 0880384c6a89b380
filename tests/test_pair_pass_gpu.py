"""Pair backward pass (solve_dpp16.h backward_split<2>): when exactly two rows of a wave need a backward pass, each of the two
instances runs on two DPP rows.  Every element is the same chain of FMAs as in the four-row pass, so a run with the pass
and a run with `no_pair` must agree bit for bit.

(12, 4), N = 12, seven MPC steps fused in one launch, grouping off so that wave w holds instances 4w..4w+3.  Two
instances of each wave get control bounds tight enough that their active set keeps changing (a backward pass in nearly
every solve); the other two get bounds that never bind and run on reused gains after their first pass.  Six waves place
the tight pair at every pair of row positions.  Every comparison first asserts that pair passes ran: an equality test
with zero pair passes proves nothing."""
import itertools

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import problems as P
from altro_mpc_icra2021_amd.mpc import REF_OPTS
from test_gpu_parity import RTOL, check_against_oracle, rel_err   # the headline parity test's constants

pytestmark = pytest.mark.gpu

n, m, N, S = 12, 4, 12, 7
SEED = None     # chosen by the `case` fixture on the CPU oracle
POS = list(itertools.combinations(range(4), 2))    # (0,1), (0,2), (0,3), (1,2), (1,3), (2,3)
TIGHT, LOOSE = 0.5, 1e3
_runs = {}


def problem(B=24, seed=None):
    pb = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=SEED if seed is None else seed)
    ub = np.full(B, LOOSE)
    for w, (a, b) in enumerate(POS):
        if 4 * w + b >= B:
            a, b = 0, 1      # a padded last wave: its live rows are the tight pair
        for r in (a, b):
            ub[4 * w + r] = TIGHT
    q = P.RandomLinearBatch(**{k: getattr(pb, k) for k in ("n", "m", "N", "dt", "A", "Bm", "Xtrack", "Utrack", "noise")})
    q.Qk, q.Rk, q.Qfk, q.u_bnd = np.full((B, n), pb.Qk), np.full((B, m), pb.Rk), np.full((B, n), pb.Qfk), ub
    return q


def oracle_for(oracle, pb, b):
    o = oracle.OracleSolver(n, m, N, pb.dt)
    o.set_dynamics(pb.A[b], pb.Bm[b])
    o.set_cost(pb.Qk[b], pb.Rk[b], pb.Qfk[b])
    zmin = np.r_[np.full(n, -np.inf), np.full(m, -pb.u_bnd[b])]
    o.add_box(zmin, -zmin, 0, N - 2)
    o.set_opts(oracle.default_opts(**REF_OPTS))
    Xr, Ur = pb.window(0)
    o.set_reference(Xr[b], Ur[b])
    o.set_initial_state(Xr[b, 0])
    o.set_controls(Ur[b])
    return o


@pytest.fixture(scope="module")
def case(oracle):
    """The seed of the case, searched on the CPU oracle so that the construction does not hang on luck on the GPU: in every
    MPC step every tight instance takes at least three iterations from a shifted start whose set of active control bounds
    is not the one it ends the step with (so both tight rows of a wave open every step with a backward pass, in the same
    turn), and no bound of a loose instance is ever active (two iterations a step: a first-order sweep on the stored
    gains, then the costate confirmation)."""
    global SEED
    from helpers import mpc_update
    for seed in range(3, 11):
        pb = problem(seed=seed)
        good = True
        for b in range(24):
            o = oracle_for(oracle, pb, b)
            o.solve()
            prev = None
            for i in range(S):
                mpc_update(o, pb, b, i)
                so = o.solve()
                act = np.abs(o.controls()) >= pb.u_bnd[b] * (1 - 1e-6)
                if pb.u_bnd[b] == TIGHT:
                    good &= so.iterations >= 3 and act.any() and (prev is None or not np.array_equal(act[:-1], prev[1:]))
                else:
                    good &= not act.any() and so.iterations <= 2
                good &= so.status == 1
                prev = act
            if not good:
                break
        if good:
            SEED = seed
            _runs.clear()
            return seed
    pytest.fail("no seed in 3..10 gives the case its two kinds of instances")


def snapshot(mp, log=False):
    sv = mp.solver
    st = altro.stats(sv)
    K, d = altro.gains(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), lam=altro.get_duals(sv), x0=mp.x0(), K=K, d=d, F=altro.gain_factors(sv),
               alpha=altro.alpha_trace(sv), pair=altro.wave_passes(sv)[:, 0].copy(), lone=altro.wave_cycles(sv)[:, 7].copy())
    for k in ("iterations", "iterations_outer", "status", "cost", "c_max", "cost_trace", "cmax_trace"):
        out[k] = np.asarray(getattr(st, k)).copy()
    if log:
        lg = mp.log()
        for k, v in (lg.items() if isinstance(lg, dict) else vars(lg).items()):
            if isinstance(v, np.ndarray):
                out["log_" + k] = v.copy()
    return out


def run(monkeypatch, no_pair, B=24, strict=0, no_qz=False, log=False, inactive=None, separate=False, park=False):
    key = (no_pair, B, strict, no_qz, log, inactive, separate, park)
    if key in _runs:
        return _runs[key]
    with monkeypatch.context() as mk:
        mk.setenv("ALTRO_NO_GROUP", "1")
        if no_pair:
            mk.setenv("ALTRO_NO_PAIR", "1")
        if no_qz:
            mk.setenv("ALTRO_NO_QZ_PASS", "1")
        pb = problem(B)
        mp = altro.mpc.BatchMPC(pb, opts=altro.SolverOptions(**dict(REF_OPTS, strict=strict)))
        if park:    # the loose rows sit the whole run out, the initial solve included
            mp.set_active((pb.u_bnd == TIGHT).astype(np.int32))
        mp.initial_solve()
        if log:
            mp.enable_log(S)
        if inactive is not None or B % 4:
            # (a mask also parks the padded slots of the last wave, which otherwise run as copies of the last instance
            #  and need every pass it needs: with B = 22 the wave's two live rows are then the only ones in need)
            act = np.ones(B, dtype=np.int32)
            if inactive is not None:
                act[inactive] = 0
            mp.set_active(act)
        pairs = np.zeros(-(-B // 4), dtype=np.int64)
        if separate:
            for i in range(S):
                mp.run_async(1, first=i)
                mp.synchronize()
                pairs += altro.wave_passes(mp.solver)[:, 0]
        else:
            mp.run_async(S, first=0)
            mp.synchronize()
        out = snapshot(mp, log)
        if separate:
            out["pair"] = pairs
    _runs[key] = out
    return out


def assert_same(a, b, skip=("pair", "lone")):
    assert set(a) == set(b)
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def on_off(monkeypatch, **kw):
    a, b = run(monkeypatch, False, **kw), run(monkeypatch, True, **kw)
    print("pair passes per wave: on %s, off %s" % (a["pair"].tolist(), b["pair"].tolist()))
    assert np.all(a["pair"] >= 1), "every wave must run at least one pair pass"
    assert np.all(b["pair"] == 0)
    assert_same(a, b)
    return a


def test_all_six_row_positions_equal_the_four_row_pass(monkeypatch, case):
    on_off(monkeypatch)


@pytest.mark.parametrize("kw", [dict(strict=1, park=True), dict(no_qz=True), dict(log=True), dict(B=22), dict(inactive=3)],
                         ids=["strict", "no_qz_pass", "mpc_log", "padded_last_wave", "masked_row"])
def test_variants_equal_the_four_row_pass(monkeypatch, case, kw):
    """strict = 1 (the symmetrising pass), the form that expands the cost anew instead of reading Qz, the per-step log, a
    padded last wave whose two live rows form a pair (B = 22: instances 20, 21, the padded slots parked by an all-ones
    mask) and a wave with one unconstrained row masked inactive (instance 3: wave 0, tight pair at rows 0, 1).  Every
    one of the six waves must report pair passes in every variant.

    strict = 1 runs with the loose rows parked (inactive from before the initial solve).  With them in the wave the count
    hangs on rounding: without gain reuse a loose row iterates twice a step, the second time at its optimum, where the
    line search compares two differences at rounding level; where it fails the row is left with rho > 0 for the rest of
    the step, and `with_rho` is a property of the wave, so the two tight rows run the regularised four-row pass from
    then on.  Measured on seeds 3..12 of this case: between one and four of the six waves ran neither a pair nor a lone
    pass in the whole launch, never the same ones, and the CPU oracle (which has the searches fail in nearly every
    loose row) does not predict which.  test_strict_with_the_loose_rows_in_the_wave keeps that case for the equality."""
    on_off(monkeypatch, **kw)


def test_strict_with_the_loose_rows_in_the_wave(monkeypatch, case):
    """the six-wave case as it is under strict = 1: equal bit for bit; pair passes must have run, in which waves is luck
    (see test_variants_equal_the_four_row_pass)"""
    a, b = run(monkeypatch, False, strict=1), run(monkeypatch, True, strict=1)
    print("pair passes per wave: on %s" % a["pair"].tolist())
    assert a["pair"].sum() >= 1 and np.all(b["pair"] == 0)
    assert_same(a, b)


def test_fused_launch_equals_single_step_launches(monkeypatch, case):
    a, b = run(monkeypatch, False), run(monkeypatch, False, separate=True)
    assert np.all(a["pair"] >= 1) and np.all(b["pair"] >= 1)
    assert_same(a, b)      # (alpha, cost and c_max traces: those of the last solve in both)


def test_one_wave_matches_the_oracle(monkeypatch, case, oracle):
    """wave 1 (tight pair at rows 0 and 2) against the CPU oracle stepped through the reference's MPC update order, at the
    tolerances of test_gain_row_feedforward_gpu.test_run_and_gains_match_the_oracle."""
    from helpers import mpc_update
    a = run(monkeypatch, False)
    assert a["pair"][1] >= 1
    pb = problem()
    st = type("St", (), {k: a[k] for k in ("iterations", "iterations_outer", "status", "cost", "c_max", "cost_trace", "cmax_trace")})
    for b in range(4, 8):
        o = oracle_for(oracle, pb, b)
        so = o.solve()
        for i in range(S):
            mpc_update(o, pb, b, i)
            so = o.solve()
        check_against_oracle(st, a["X"], a["U"], b, o, so)
        Ko, do = o.gains()
        assert rel_err(a["K"][b], Ko) <= RTOL
        assert np.abs(a["d"][b] - do).max() <= RTOL * max(1.0, np.abs(do).max())
