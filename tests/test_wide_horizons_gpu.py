"""The horizon axis of the one-wave-per-instance kernel (solve_wide.h) on the device: the table of tests/wide_horizons.py
(tests/test_wide_horizons.py holds its inputs, its coverage of the loop edges and the dispatch, without a GPU).

 a. oracle parity at every (class, N): the initial solve and three MPC steps against one oracle per instance at the tolerances of
    test_gpu_parity.check_against_oracle, the duals of every block after every solve at the same RTOL (the constrained classes
    through check_duals_and_gains), the x0 of every step to 1e-12; then the three steps as ONE fused launch on a twin, bit for bit.
 b. the sweeps ran where the table says: at every SWEEP_HORIZONS case the class's counter (gain reuse or costate confirmation),
    summed over the loop and a warm re-solve, is above zero, and the re-solve matches the oracle.
 c. a strict = 1 twin at the same cases: both counters zero, parity with the oracle, and the largest difference from the default
    run printed and held to ULP_BOUND.
 d. sets_differ beyond its first trip: a solve that starts from a trajectory whose set differs from the stored pass's at one knot
    >= 16 alone runs a backward pass, where a twin with nothing changed runs on the stored gains; both match the oracle.
 e. the shifted duals of every block after every single step: part of a (row-linrows holds a row range that starts at knot 1).
Every handle is asserted to be on the wide backend (wave_cycles is empty there).  Runs are cached per case."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
import lane16_matrix as lm
import wide_horizons as wh
from altro_mpc_icra2021_amd.mpc import REF_OPTS
from test_gpu_parity import RTOL, check_against_oracle, rel_err
from test_wide_matrix_gpu import check_duals_and_gains
from wide_matrix import at_penalty_cap

pytestmark = pytest.mark.gpu

STAT = ("iterations", "iterations_outer", "status", "cost", "c_max", "cost_trace", "cmax_trace")
SWEEP_CASES = [(c.name, N) for c in wh.CLASSES if c.counter for N in wh.SWEEP_HORIZONS if (c.name, N) in wh.CASES]
_runs = {}


def make_mpc(pr, strict=0):
    pb, N = pr.pb, pr.N
    if pr.tp is not None:
        mp = altro.mpc.TrackMPC(lm.track_gpu_problem(altro, pr.tp), altro.SolverOptions(**dict(pr.tp.opts, strict=strict)), pb.Xtrack, pb.Utrack, pb.noise)
    elif pr.dyn is not None:
        A, Bm, d = pr.dyn
        prob = altro.mpc.gen_tracking_problem(pb)
        prob.model = altro.LinearModel(A[:, :N - 1], Bm[:, :N - 1], d[:, :N - 1], dt=pb.dt, per_knot=True)
        mp = altro.mpc.TrackMPC(prob, altro.SolverOptions(**dict(REF_OPTS, strict=strict)), pb.Xtrack, pb.Utrack, pb.noise)
        altro.set_dynamics_track(mp.solver, A, Bm, d, step_stride=1)
    else:
        mp = altro.mpc.BatchMPC(pb, altro.SolverOptions(**dict(REF_OPTS, strict=strict)))
    assert altro.wave_cycles(mp.solver).size == 0, "the wide backend"
    return mp


def everything(mp, pr):
    """every output of the handle and every counter since it was made"""
    sv, st = mp.solver, altro.stats(mp.solver)
    K, d = altro.gains(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), x0=mp.x0(), K=K, d=d, reuse=altro.reuse_counter(sv), confirm=altro.confirm_counter(sv))
    out.update({k: np.asarray(getattr(st, k)).copy() for k in STAT})
    out.update({"work%d" % i: w for i, w in enumerate(altro.work_counters(sv))})
    for ci, kind in enumerate(wh.kinds_of(pr)):
        out["duals_" + kind] = altro.get_duals(sv, ci)
    return out


def check_solve(mp, pr, orcs, sos, what):
    """check_against_oracle and the duals of every block at RTOL for every instance; the largest error of X, U and the duals"""
    sv = mp.solver
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    worst = 0.0
    for b, (o, so) in enumerate(zip(orcs, sos)):
        assert not at_penalty_cap(so), what
        check_against_oracle(st, X, U, b, o, so)
        worst = max(worst, rel_err(X[b], o.states()), rel_err(U[b], o.controls()))
        for ci, kind in enumerate(wh.kinds_of(pr)):
            lam_o, lam_g = o.duals(o.con_ids[ci]), altro.get_duals(sv, ci)[b].reshape(-1)
            el = np.abs(lam_g - lam_o).max() / max(1.0, np.abs(lam_o).max())
            assert el <= RTOL, (what, b, kind, el)
            worst = max(worst, el)
    if pr.tp is not None:
        check_duals_and_gains(sv, pr.tp, orcs, tag=what)
    return worst


def run(oracle, case, strict=0, fused=False, resolve=False):
    """The loop of a case: the initial solve, then STEPS steps as single launches, each solve held to the oracle (x0 of a step to
    1e-12), or as one fused launch; with resolve, x0 then moves by 0.02 standard normal and the handle solves again, against the
    oracle too.  NS(loop: everything() after the loop, worst: largest error against the oracle, after_resolve)."""
    key = (case, strict, fused, resolve)
    if key in _runs:
        return _runs[key]
    pr = wh.problem(case)
    mp = make_mpc(pr, strict)
    sv = mp.solver
    r = NS(pr=pr, worst=0.0, iters=[])
    mp.initial_solve()
    if fused:
        mp.run_async(wh.STEPS, first=0)
        mp.synchronize()
    else:
        orcs = wh.oracles(oracle, pr)
        r.worst = check_solve(mp, pr, orcs, [o.solve() for o in orcs], "initial solve")
        for i in range(wh.STEPS):
            mp.step(i)
            X, x0g = altro.states(sv), mp.x0()
            for b, o in enumerate(orcs):
                x0 = wh.oracle_step(o, pr, b, i)
                assert np.abs(x0 - x0g[b]).max() <= 1e-12 * max(1.0, np.abs(x0).max()), (i, b)
                assert np.array_equal(X[b, 0], x0g[b])
            r.worst = max(r.worst, check_solve(mp, pr, orcs, [o.solve() for o in orcs], "step %d" % i))
            r.iters.append(altro.stats(sv).iterations.tolist())
    r.loop = everything(mp, pr)
    if resolve:
        assert not fused
        x1 = mp.x0() + wh.resolve_move(pr.N, mp.x0().shape)
        altro.set_initial_state(sv, x1)
        altro.solve(sv)
        for b, o in enumerate(orcs):
            o.set_initial_state(x1[b])
        r.worst = max(r.worst, check_solve(mp, pr, orcs, [o.solve() for o in orcs], "warm re-solve"))
        r.after_resolve = everything(mp, pr)
    sv.close()
    _runs[key] = r
    return r


# ---------------------------------------------------------------------------------------------------------------------
# a. parity and the fused launch (e: the duals of every block after every single step)
@pytest.mark.parametrize("case", wh.CASES, ids=wh.case_id)
def test_loop_matches_oracle_and_fused_equals_single_steps(oracle, case):
    """Every solve of the loop against the oracle -- statuses, both iteration counts, cost, c_max, both traces, X, U, the duals of
    every block (after a step: the shifted ones), the gains of the constrained classes -- then the three steps as ONE fused launch
    on a twin: every output and every counter, bit for bit."""
    r = run(oracle, case, resolve=case[1] in wh.SWEEP_HORIZONS and bool(wh.CLASS[case[0]].counter))
    print("%s: largest error of X, U, duals over the loop %.2e; iterations of the steps %s; reuse %s, confirm %s" % (
        wh.case_id(case), r.worst, r.iters, r.loop["reuse"].tolist(), r.loop["confirm"].tolist()))
    f = run(oracle, case, fused=True)
    assert np.all(r.loop["status"] == altro.SOLVE_SUCCEEDED)
    for k in r.loop:
        assert np.array_equal(r.loop[k], f.loop[k]), ("fused", k)


# ---------------------------------------------------------------------------------------------------------------------
# b. the sweeps at their edge horizons
@pytest.mark.parametrize("case", SWEEP_CASES, ids=wh.case_id)
def test_sweeps_run_at_their_edge_horizons_and_match_oracle(oracle, case):
    """At every horizon that is an edge of grad_pass, adjoint_row, adjoint_lds or shift_column: over the loop and a warm re-solve
    (x0 moved by 0.02 standard normal) iterations ran on the stored gains (row-reuse, simple-4, simple-8: reuse_counter) or were
    confirmed by the costate sweep (row-confirm, row-ltv, row-linrows: confirm_counter), and every solve, the re-solve included,
    matches the oracle.  A counter of zero fails."""
    cls = wh.CLASS[case[0]]
    r = run(oracle, case, resolve=True)
    a = r.after_resolve
    print("%s: reuse %s, confirm %s over the loop and the re-solve (the loop alone: %s, %s); backward passes %s; largest error %.2e" % (
        wh.case_id(case), a["reuse"].tolist(), a["confirm"].tolist(), r.loop["reuse"].tolist(), r.loop["confirm"].tolist(), a["work0"].tolist(), r.worst))
    assert a[cls.counter].sum() > 0, cls.counter
    other = "confirm" if cls.counter == "reuse" else "reuse"
    assert a[other].sum() == 0, (other, "the class takes one kind of sweep only")


# ---------------------------------------------------------------------------------------------------------------------
# c. strict = 1: no sweep at all
@pytest.mark.parametrize("case", SWEEP_CASES, ids=wh.case_id)
def test_strict_twin_runs_no_sweep_and_agrees(oracle, case):
    """altro_opts.strict = 1 is the only switch of this backend that takes both sweeps away (it also takes the two default-mode
    shortcuts of ilqr() that are no sweeps: the confirmation of an iteration whose backward pass returned feedforward terms at
    rounding level, and the early end of a line search whose trial moved nothing -- so statuses and iteration counts are not
    compared between the twins directly; each is held to the oracle's, which holds them to each other).  Both counters zero over
    the loop and the re-solve; parity with the oracle; X, U and every dual block of the default run within ULP_BOUND of the
    strict run's -- the amount the oracle itself moves under one ulp of its inputs."""
    r, s = run(oracle, case, resolve=True), run(oracle, case, strict=1, resolve=True)
    assert s.after_resolve["reuse"].sum() == 0 and s.after_resolve["confirm"].sum() == 0
    worst = 0.0
    for a, b in ((r.loop, s.loop), (r.after_resolve, s.after_resolve)):
        for k in ["X", "U"] + [k for k in a if k.startswith("duals_")]:
            worst = max(worst, rel_err(a[k], b[k]))
    print("%s: default against strict, largest difference of X, U, duals %.2e; backward passes %d against %d; strict against the oracle %.2e" % (
        wh.case_id(case), worst, r.after_resolve["work0"].sum(), s.after_resolve["work0"].sum(), s.worst))
    assert r.after_resolve["work0"].sum() < s.after_resolve["work0"].sum(), "the sweeps replaced backward passes"
    assert worst <= wh.ULP_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# d. sets_differ beyond the first trip
@pytest.mark.parametrize("case", wh.TRIP_CASES, ids=wh.case_id)
def test_active_set_change_beyond_knot_16_forces_a_backward_pass(oracle, case):
    """N = 18 and 33 (N = 17: wide_horizons.TRIP_LEFT_OUT).  Two handles run the loop.  One solves again with nothing changed; the
    other first has ONE control at a knot >= 16, inactive in the solution, put 5 % beyond its bound (set_initial_trajectory, which
    does not drop the stored gains; wide_horizons.trip_start picks it on the oracle).  Where the first ran its solve without a
    backward pass the stored pass was usable and its set is the solution's, so the start of the second differs from it at that one
    late knot alone, and a sets_differ that stopped after its first trip would take the stored gains there too.  In the instances
    where, besides, both solves take one outer iteration (a pass after a penalty change runs regardless) -- at least one, asserted --
    the second handle ran a backward pass.  Every iteration is a pass, a reused pass or a confirmation, and both solves match
    the oracle."""
    t = wh.trip_start(oracle, case)
    assert t.ok
    pr = t.pr
    out = []
    for orcs, sos, change in ((t.same, t.so_same, False), (t.moved, t.so_moved, True)):
        mp = make_mpc(pr)
        sv = mp.solver
        mp.initial_solve()
        for i in range(wh.STEPS):
            mp.step(i)
        before = everything(mp, pr)
        if change:
            U = before["U"].copy()
            for b in range(wh.B):
                U[b, int(t.pick[b, 0]), int(t.pick[b, 1])] = t.pick[b, 2]
            altro.initial_controls(sv, U)
        altro.solve(sv)
        after = everything(mp, pr)
        worst = check_solve(mp, pr, orcs, sos, "second solve, start %s" % ("changed" if change else "unchanged"))
        sv.close()
        bw, gs, gc = (after[k] - before[k] for k in ("work0", "reuse", "confirm"))
        print("%s start %s: iterations %s, backward passes %s, reused %s, confirmed %s; largest error of X, U, duals %.2e" % (
            wh.case_id(case), "changed" if change else "unchanged", after["iterations"].tolist(), bw.tolist(), gs.tolist(), gc.tolist(), worst))
        assert np.array_equal(bw + gs + gc, after["iterations"])
        out.append(bw)
    held = (out[0] == 0) & t.one_outer
    print("%s: held in the instances %s" % (wh.case_id(case), np.nonzero(held)[0].tolist()))
    assert held.any(), "no instance ran the unchanged solve on the stored gains throughout"
    assert (out[1][held] >= 1).all()
