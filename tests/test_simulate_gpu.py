"""Closed-loop simulation of the stored policy under disturbances (altro_batch_simulate_policy_dev / altro_batch_simulate_policy)
on both backends.  No assertion of the byte-equality block is a measured tolerance: each is a byte equality against calls that
existed before -- eval_policy_dev for the controls, evaluate_dev's rollout form for one step and for whole trajectories, its
given form for J and c_max, numpy's one subtraction for dx_max.

Shapes: the cases of tests/warm_start_ref.py (batch 5, N = 9; (64, 32) at batch 2, N = 4, which the solve kernel refuses: its
gains stay invalid and its loop is open), plus (12, 4) forced onto the one-wave-per-instance backend.  Every case is solved once;
nsamp = 3 (15 rows: a partial wave, instances straddling waves), on 16-box also nsamp = 1 and 17.  Start states are
xbar_0 + 1e-2 (1 + |xbar_0|) randn, disturbances of the same relative size; the last sample starts 300 times further out, so
that the clamp bites.

The ALTRO_ERR_STATE case "the window runs past the stored reference" is not exercised: every call that advances the window
checks it first, so no sequence of public calls leaves a handle in that state (the tests of evaluate and warm_start, which
share the check, do not reach it either).

The row tables, LDS sizes and shapes these cases do not reach are in tests/scoring_matrix.py."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc, problems

import evaluate_ref as ER
import simulate_ref as SR
import warm_start_ref as WR
from test_warm_start_gpu import H, T, assert_twins, dev, everything, forced_wide, plane, same

pytestmark = pytest.mark.gpu
INV, STATE = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_STATE
OPTS = dict(mpc.REF_OPTS, iterations=60)
RUNS = [(name, False) for name in WR.CASES] + [("16-box(12,4)", True)]
IDS = [name + ("-forced-wide" if fw else "") for name, fw in RUNS]
S = 3
SENT = -12345.5


def solver_of(cs, kw, fw=False):
    with forced_wide(fw):
        return altro.ALTROSolver(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**OPTS))


def sim(sv, x0=None, w=None, nsamp=None, clamp=True, traj=True, host=False):
    """simulate_policy on numpy inputs with sentinels in every output: NS(J, c, dx, fb, X, U) as numpy; host: the host twin"""
    ns = x0.shape[1] if x0 is not None else w.shape[1] if w is not None else (nsamp or 1)
    shp = [(sv.B, ns)] * 3 + [(sv.B, ns, sv.N, sv.n), (sv.B, ns, sv.N - 1, sv.m)]
    if host:
        J, c, dx, X, U = (np.full(s, SENT) for s in shp)
        fb = np.full(sv.B, -77, dtype=np.int32)
        altro.simulate_policy(sv, x0, w, nsamp, clamp, (J, c, dx), fb, X if traj else None, U if traj else None)
        return NS(J=J, c=c, dx=dx, fb=fb, X=X if traj else None, U=U if traj else None)
    J, c, dx, X, U = (torch.full(s, SENT, dtype=torch.float64, device=dev()) for s in shp)
    fb = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
    altro.simulate_policy(sv, None if x0 is None else T(x0), None if w is None else T(w), nsamp, clamp, (J, c, dx), fb, X if traj else None,
                          U if traj else None)
    torch.cuda.synchronize()
    return NS(J=H(J), c=H(c), dx=H(dx), fb=H(fb), X=H(X) if traj else None, U=H(U) if traj else None)


def policy(sv, x, k, clamp):
    knot = torch.full((sv.B,), k, dtype=torch.int32, device=dev())
    return H(altro.eval_policy(sv, T(x), knot=knot, clamp=clamp))


def rollout(sv, U, x0=None):
    """Xout of evaluate_dev's rollout form"""
    Xo = torch.full(tuple(U.shape[:-2]) + (sv.N, sv.n), SENT, dtype=torch.float64, device=dev())
    c = torch.empty(tuple(U.shape[:-2]), dtype=torch.float64, device=dev())
    altro.evaluate(sv, T(U), x0=None if x0 is None else T(x0), out=(None, c, None), Xout=Xo)
    return H(Xo)


def given(sv, X, U):
    J, c = (torch.empty(tuple(U.shape[:-2]), dtype=torch.float64, device=dev()) for _ in range(2))
    altro.evaluate(sv, T(U), X=T(X), out=(J, c, None))
    return H(J), H(c)


def inputs(Xbar, seed, ns=S):
    """(x0 (B, ns, n), w (B, ns, N-1, n)): the last sample starts far out"""
    x0 = SR.disturbed_starts(Xbar[:, 0], ns, seed)
    x0[:, -1] = SR.disturbed_starts(Xbar[:, 0], 1, seed + 1, rel=3.0)[:, 0]
    return x0, SR.disturbances(Xbar, ns, seed + 2)


@functools.lru_cache(maxsize=None)
def ran(name, fw):
    """every device call a case's tests look at, made once on one solved handle"""
    make, kw = WR.CASES[name]
    cs = make()
    r = NS(cs=cs, kw=kw, solvable=name != "wide-limits(64,32)", ltv=bool(kw.get("per_knot_dyn")), clamp={})
    sv = solver_of(cs, kw, fw)
    try:
        if r.solvable:
            altro.solve(sv)
        r.Xbar, r.Ubar = plane(sv)
        r.K = altro.gains(sv)[0] if r.solvable else None
        r.x0, r.w = inputs(r.Xbar, 71)
        B, N = cs.B, cs.N
        for clamp in (0, 1):
            q = NS()
            q.full = sim(sv, r.x0, r.w, clamp=clamp)
            q.now = sim(sv, r.x0, None, clamp=clamp)
            q.nox0 = sim(sv, None, None, nsamp=S, clamp=clamp)
            q.quiet = sim(sv, r.x0, r.w, clamp=clamp, traj=False)
            q.host = sim(sv, r.x0, r.w, clamp=clamp, host=True)
            q.host_quiet = sim(sv, None, r.w, clamp=clamp, traj=False, host=True)
            q.dev_quiet = sim(sv, None, r.w, clamp=clamp, traj=False)
            q.alone = [sim(sv, r.x0[:, s:s + 1], r.w[:, s:s + 1], clamp=clamp) for s in range(S)]
            q.pol = np.stack([np.stack([policy(sv, q.full.X[:, s, k], k, clamp) for k in range(N - 1)], axis=1) for s in range(S)], axis=1)
            q.roll_now = np.stack([rollout(sv, np.ascontiguousarray(q.now.U[:, s]), r.x0[:, s]) for s in range(S)], axis=1)
            q.roll_nox0 = rollout(sv, q.nox0.U)
            q.given = given(sv, q.full.X, q.full.U)
            if not r.ltv:   # one step of the rollout form from x_k under u_k, w_k added in torch
                q.step = np.empty((B, S, N - 1, cs.n))
                U1 = np.zeros((B, N - 1, cs.m))
                for s in range(S):
                    for k in range(N - 1):
                        U1[:, 0] = q.full.U[:, s, k]
                        X1 = T(rollout(sv, U1, np.ascontiguousarray(q.full.X[:, s, k]))[:, 1])
                        q.step[:, s, k] = H(X1 + T(r.w[:, s, k]))
            r.clamp[clamp] = q
        r.after = plane(sv)
    finally:
        sv.close()
    return r


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_controls_are_the_bytes_of_eval_policy(name, fw):
    """1: Uout[:, s, k] == eval_policy_dev(x = Xout[:, s, k], knot = k, clamp), clamp 0 and 1; fb as eval_policy reports it; the
    far sample is clamped where the case bounds its controls and the gains are valid"""
    r = ran(name, fw)
    for clamp, q in r.clamp.items():
        assert same(q.full.U, q.pol), clamp
        assert q.full.fb.dtype == np.int32 and (q.full.fb == (1 if r.solvable else 0)).all()
        assert np.isfinite(q.full.X).all() and np.isfinite(q.full.U).all()
    u0, u1 = r.clamp[0].full.U, r.clamp[1].full.U
    box = next((c for c in r.cs.cons if c.kind == "box"), None)
    if box is not None:
        k0, k1 = box.k0, min(box.k1, r.cs.N - 2)
        lo, hi = box.zmin[:, None, None, r.cs.n:], box.zmax[:, None, None, r.cs.n:]
        assert (u1[:, :, k0:k1 + 1] >= lo).all() and (u1[:, :, k0:k1 + 1] <= hi).all()
        assert same(u1[:, :, k0], np.clip(u0[:, :, k0], lo[:, :, 0], hi[:, :, 0]))        # (knot k0: both runs are at the same x_0)
        if r.solvable:
            print(name, "controls the clamp moved:", int((u0 != u1).sum()), "of", u0.size)
            assert (u0[:, -1] != u1[:, -1]).any()
            assert (r.clamp[0].full.U != r.Ubar[:, None]).any()
    else:
        assert same(u0, u1)


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_states_are_the_bytes_of_the_rollout_form(name, fw):
    """2: without w, Xout == evaluate_dev's rollout Xout on U = Uout (x0 NULL: one call with ncand = nsamp; x0 given: one call
    per sample).  With x0 = NULL and no w every sample is the same"""
    r = ran(name, fw)
    for clamp, q in r.clamp.items():
        assert same(q.now.X, q.roll_now), clamp
        assert same(q.nox0.X, q.roll_nox0), clamp
        assert same(q.now.X[:, :, 0], r.x0)
        for s in range(1, S):
            assert same(q.nox0.X[:, s], q.nox0.X[:, 0]) and same(q.nox0.U[:, s], q.nox0.U[:, 0]) and same(q.nox0.J[:, s], q.nox0.J[:, 0])
        assert not same(q.now.X, q.full.X)


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_scores_are_the_bytes_of_the_given_form(name, fw):
    """3: J, c_max == evaluate_dev's given form on (Xout, Uout); without Xout / Uout the same J, c_max, dx_max come back"""
    r = ran(name, fw)
    for clamp, q in r.clamp.items():
        assert same(q.full.J, q.given[0]) and same(q.full.c, q.given[1]), clamp
        for a, b in ((q.quiet.J, q.full.J), (q.quiet.c, q.full.c), (q.quiet.dx, q.full.dx), (q.quiet.fb, q.full.fb)):
            assert same(a, b), clamp
        assert (q.full.J > 0).all() and (q.full.c >= 0).all()


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_one_step_with_a_disturbance(name, fw):
    """4: Xout[:, s, k+1] == X1 + w[:, s, k] added in torch, X1 knot 1 of a rollout-form evaluate_dev from x0 = Xout[:, s, k] whose
    first control is Uout[:, s, k] (time-invariant dynamics).  Per-knot dynamics: bound 1 of evaluate_ref.py, 2 (n+m+2) u S,
    plus one rounding of the addition, against numpy (the addition on numpy's side in extended precision)"""
    r = ran(name, fw)
    cs = r.cs
    for clamp, q in r.clamp.items():
        X, U = q.full.X, q.full.U
        assert same(X[:, :, 0], r.x0)
        if not r.ltv:
            assert same(X[:, :, 1:], q.step), clamp
            continue
        pred = np.einsum("bkij,bckj->bcki", cs.A, X[:, :, :-1]) + np.einsum("bkij,bckj->bcki", cs.Bm, U) + cs.f[:, None]
        Sx = (np.einsum("bkij,bckj->bcki", np.abs(cs.A), np.abs(X[:, :, :-1])) + np.einsum("bkij,bckj->bcki", np.abs(cs.Bm), np.abs(U))
              + np.abs(cs.f)[:, None])
        res = np.abs(X[:, :, 1:].astype(np.longdouble) - (pred.astype(np.longdouble) + r.w.astype(np.longdouble))).astype(np.float64)
        bound = ER.step_bound(cs, Sx) + ER.U_ * np.abs(X[:, :, 1:])
        print(name, clamp, "max residual / bound", (res / bound).max())
        assert np.finfo(np.longdouble).nmant >= 63
        assert (res <= bound).all()


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_dx_max_is_one_subtraction(name, fw):
    """5: dx_max == max |Xout - states| in numpy, exactly"""
    r = ran(name, fw)
    for clamp, q in r.clamp.items():
        for run in (q.full, q.now, q.nox0):
            assert same(run.dx, np.abs(run.X - r.Xbar[:, None]).max(axis=(2, 3))), clamp
        assert (q.full.dx[:, -1] > q.full.dx[:, 0]).all()


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_host_twin_writes_the_same_bytes(name, fw):
    """6"""
    r = ran(name, fw)
    for clamp, q in r.clamp.items():
        for k in ("J", "c", "dx", "fb", "X", "U"):
            a, b = getattr(q.host, k), getattr(q.full, k)
            assert a.dtype == b.dtype and same(a, b), (clamp, k)
        for k in ("J", "c", "dx", "fb"):
            assert same(getattr(q.host_quiet, k), getattr(q.dev_quiet, k)), (clamp, k)
        assert (q.host_quiet.J != SENT).all() and not same(q.host_quiet.J, q.host.J)


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_a_sample_alone_gets_the_same_bytes(name, fw):
    """7, first half: sample s with nsamp = 1; and nothing the caller can read of the trajectory changed over all the calls"""
    r = ran(name, fw)
    for clamp, q in r.clamp.items():
        for s, a in enumerate(q.alone):
            for k in ("J", "c", "dx", "X", "U"):
                assert same(getattr(a, k)[:, 0], getattr(q.full, k)[:, s]), (clamp, s, k)
            assert same(a.fb, q.full.fb)
    assert same(r.after[0], r.Xbar) and same(r.after[1], r.Ubar)


@pytest.mark.parametrize("name", ["16-box(12,4)", "16-soc(6,3)", "wide-cone(7,3)", "wide-ltv(12,12)"])
def test_instance_alone_on_a_batch_one_handle(name):
    """7, second half: instance b on a solved batch-1 handle holding its rows of data (same trajectory, same gains: checked
    first) gets the bytes it gets inside the batch"""
    r = ran(name, False)
    q = r.clamp[1].full
    for b in range(r.cs.B):
        sv = solver_of(ER.sub_case(r.cs, b), {k: v for k, v in r.kw.items() if k == "per_knot_dyn"})
        try:
            altro.solve(sv)
            Xb, Ub = plane(sv)
            assert same(Xb, r.Xbar[b:b + 1]) and same(Ub, r.Ubar[b:b + 1]) and same(altro.gains(sv)[0], r.K[b:b + 1]), ("the solves differ", b)
            a = sim(sv, r.x0[b:b + 1], r.w[b:b + 1], clamp=1)
        finally:
            sv.close()
        for k in ("J", "c", "dx", "fb", "X", "U"):
            assert same(getattr(a, k), getattr(q, k)[b:b + 1]), (b, k)


@pytest.mark.parametrize("nsamp", [1, 17])
def test_one_sample_and_more_rows_than_a_block(nsamp):
    """16-box with nsamp = 1 and nsamp = 17 (more rows per instance than the 16 of a 256-thread block): equalities 1, 3 and 5, and
    every sample the bytes it gets alone"""
    cs = ER.case_16_box()
    sv = solver_of(cs, {})
    try:
        altro.solve(sv)
        Xbar, _ = plane(sv)
        x0, w = inputs(Xbar, 83, nsamp)
        a = sim(sv, x0, w)
        assert a.J.shape == (cs.B, nsamp) and (a.fb == 1).all()
        J, c = given(sv, a.X, a.U)
        assert same(a.J, J) and same(a.c, c)
        assert same(a.dx, np.abs(a.X - Xbar[:, None]).max(axis=(2, 3)))
        for s in sorted({0, nsamp // 2, nsamp - 1}):
            for k in (0, cs.N // 2, cs.N - 2):
                assert same(a.U[:, s, k], policy(sv, a.X[:, s, k], k, True)), (s, k)
            one = sim(sv, x0[:, s:s + 1], w[:, s:s + 1])
            assert same(one.X[:, 0], a.X[:, s]) and same(one.U[:, 0], a.U[:, s]) and same(one.J[:, 0], a.J[:, s])
    finally:
        sv.close()


# ---------------------------------------------------------------------------------------------- behaviour
@pytest.mark.parametrize("name,fw", [("16-box(12,4)", False), ("16-soc(6,3)", False), ("wide-cone(7,3)", False), ("16-box(12,4)", True)])
def test_fixed_point(name, fw):
    """the handle's trajectory set to a rollout of its own controls (evaluate_dev with Xout, set_initial_trajectory_dev): with
    x0 = NULL and w = NULL the simulation returns Uout == ubar and Xout == xbar bit for bit and dx_max == 0, the gains valid"""
    make, kw = WR.CASES[name]
    cs = make()
    sv = solver_of(cs, kw, fw)
    try:
        altro.solve(sv)
        U = altro.controls(sv, out=torch.empty((sv.B, sv.N - 1, sv.m), dtype=torch.float64, device=dev()))
        X = altro.rollout(sv, U)
        with api._bracket(sv):
            api._initial_trajectory_dev(sv, X, U)
        box = next((c for c in cs.cons if c.kind == "box"), None)
        for clamp in (0, 1):
            a = sim(sv, nsamp=S, clamp=clamp)
            assert (a.fb == 1).all()
            if clamp and box is not None:      # (the solved controls respect their bounds only to the constraint tolerance)
                Uc = np.clip(H(U), box.zmin[:, None, cs.n:], box.zmax[:, None, cs.n:])
                assert same(a.U[:, :, 0], np.repeat(Uc[:, None, 0], S, axis=1))
                if not same(Uc, H(U)):
                    continue
            assert same(a.U, np.repeat(H(U)[:, None], S, axis=1)) and same(a.X, np.repeat(H(X)[:, None], S, axis=1)), clamp
            assert same(a.dx, np.zeros((sv.B, S)))
    finally:
        sv.close()


@pytest.mark.parametrize("fw", [False, True])
def test_no_valid_gains_is_the_open_loop(fw):
    """before the first solve, and after a setter that drops the stored gains: fb = 0, Uout is the handle's controls and Xout
    their rollout from the sample's x0 (byte equality 2)"""
    cs = ER.case_16_box()
    sv = solver_of(cs, {}, fw)
    try:
        def look(what):
            Xbar, Ubar = plane(sv)
            x0, _ = inputs(Xbar, 91)
            a = sim(sv, x0, None, clamp=0)
            assert (a.fb == 0).all(), what
            assert same(a.U, np.repeat(Ubar[:, None], S, axis=1)), what
            assert same(a.X, np.stack([rollout(sv, Ubar, x0[:, s]) for s in range(S)], axis=1)), what
            a1 = sim(sv, x0, None, clamp=1)
            box = cs.cons[0]
            assert same(a1.U, np.clip(a.U, box.zmin[:, None, None, cs.n:], box.zmax[:, None, None, cs.n:])), what
        look("before the first solve")
        altro.solve(sv)
        Xbar, _ = plane(sv)
        assert (sim(sv, inputs(Xbar, 91)[0], None).fb == 1).all()
        prob = ER.to_problem(altro, cs)
        altro.set_tracking_cost(sv, prob.obj.Q, prob.obj.R, prob.obj.Qf)     # the same weights: still drops the gains
        look("after set_tracking_cost")
    finally:
        sv.close()


@pytest.mark.parametrize("name,fw", [("16-box(12,4)", False), ("16-soc(6,3)", False), ("wide-cone(7,3)", False), ("16-box(12,4)", True)])
def test_nothing_the_library_owns_changes(name, fw):
    """everything a caller can read is the same before and after the call, and the following solve equals that of a twin that
    never made it"""
    make, kw = WR.CASES[name]
    cs = make()
    sv, tw = solver_of(cs, kw, fw), solver_of(cs, kw, fw)
    try:
        altro.solve(sv), altro.solve(tw)
        ncons = len(cs.cons)
        before = everything(sv, cs.x0, ncons)
        Xbar, _ = plane(sv)
        x0, w = inputs(Xbar, 95)
        sim(sv, x0, w, clamp=1)
        sim(sv, x0, w, clamp=0, traj=False, host=True)
        after = everything(sv, cs.x0, ncons)
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
        assert_twins(sv, tw, cs.x0, ncons, "before the next solve")
        for s in (sv, tw):
            altro.set_initial_state(s, x0[:, 0])
            altro.solve(s)
        assert_twins(sv, tw, cs.x0, ncons, "after the next solve")
    finally:
        sv.close(), tw.close()


@pytest.mark.parametrize("force_wide", [False, True])
def test_mpc_steps_after_the_call_equal_a_twin(monkeypatch, force_wide):
    """an MPC loop under staggered episode clocks: the simulation is scored against each instance's own window (J, c_max are the
    given form's bytes on a twin), and the steps that follow equal those of the twin that never made the call"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    pb = problems.gen_random_linear_batch(5, n=12, m=4, N=9, steps=8, seed=33, u_bnd=3.0)
    a, b = (mpc.BatchMPC(pb, altro.SolverOptions(**OPTS)) for _ in range(2))
    try:
        for mp in (a, b):
            mp.initial_solve()
            mp.set_clock(np.array([0, 1, 2, 0, 1]))
            mp.run_async(3, first=0)
            mp.synchronize()
        Xbar, _ = plane(a.solver)
        x0, w = inputs(Xbar, 97)
        r = sim(a.solver, x0, w)
        assert (r.fb == 1).all()
        J, c = given(b.solver, r.X, r.U)
        assert same(r.J, J) and same(r.c, c)
        assert list(api.get_clock(a.solver)[2]) == [3, 2, 1, 3, 2]
        for mp in (a, b):
            mp.run_async(2, first=3)
            mp.synchronize()
        assert_twins(a.solver, b.solver, pb.Xtrack[:, 0], 1, "after the next steps")
    finally:
        a.solver.close(), b.solver.close()


def test_nan_stays_in_its_sample():
    """a NaN in one sample's x0 reaches only that sample's outputs"""
    r = ran("16-box(12,4)", False)
    for fw in (False, True):
        sv = solver_of(r.cs, r.kw, fw)
        try:
            altro.solve(sv)
            ref = sim(sv, r.x0, r.w)
            x0 = r.x0.copy()
            x0[1, 1, 3] = np.nan
            a = sim(sv, x0, r.w)
        finally:
            sv.close()
        keep = np.ones((r.cs.B, S), dtype=bool)
        keep[1, 1] = False
        for k in ("J", "c", "dx", "X", "U"):
            assert same(getattr(a, k)[keep], getattr(ref, k)[keep]), (fw, k)
        assert np.isnan(a.J[1, 1]) and np.isnan(a.dx[1, 1]) and np.isnan(a.X[1, 1, 1:]).all() and same(a.fb, ref.fb)
        if not fw:
            assert same(ref.X, r.clamp[1].full.X)


@pytest.mark.parametrize("force_wide", [False, True])
def test_value_of_the_closed_loop(monkeypatch, force_wide):
    """unconstrained (4, 2), N = 9, clamp 0: J of the closed loop from a perturbed x0' is strictly below evaluate_dev's open-loop J
    of the handle's controls from x0', and within 10 x cost_tolerance of the cost of a twin solved from x0' (read through the
    own-trajectory form of evaluate_dev): the LQ policy is exactly optimal, the twin stops inside cost_tolerance of the optimum"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    cs = ER.make_case(5, 4, 2, 9, seed=41)
    sv, tw = solver_of(cs, {}), solver_of(cs, {})
    try:
        altro.solve(sv)
        x0p = cs.x0 + 0.5 * np.random.default_rng(42).standard_normal(cs.x0.shape)
        a = sim(sv, x0p[:, None], None, clamp=0)
        assert (a.fb == 1).all()
        Jo = torch.empty((cs.B,), dtype=torch.float64, device=dev())
        altro.evaluate(sv, T(plane(sv)[1]), x0=T(x0p), out=(Jo, None, None))
        altro.set_initial_state(tw, x0p)
        altro.solve(tw)
        Jt = torch.empty((cs.B,), dtype=torch.float64, device=dev())
        altro.evaluate(tw, out=(Jt, None, None))
        torch.cuda.synchronize()
        tol = OPTS["cost_tolerance"]
        print("closed loop", a.J[:, 0], "twin", H(Jt), "open loop", H(Jo), "gap", np.abs(a.J[:, 0] - H(Jt)).max(), "bound", 10 * tol)
        assert (a.J[:, 0] < H(Jo)).all()
        assert (np.abs(a.J[:, 0] - H(Jt)) <= 10 * tol).all()
    finally:
        sv.close(), tw.close()


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("force_wide", [False, True])
def test_refusals_launch_nothing(monkeypatch, force_wide):
    """every ALTRO_ERR_INVALID_ARG case of the contract, a host pointer, a buffer one element short and a tensor that is not on
    the solver's device: refused with a message, the sentinel in every output untouched, the handle usable afterwards"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    cs = ER.case_16_box()
    sv, tw = solver_of(cs, {}), solver_of(cs, {})
    try:
        altro.solve(sv), altro.solve(tw)
        L, B, N, n, m = sv._L, sv.B, sv.N, sv.n, sv.m
        gp = lambda t: C.c_void_p(t.data_ptr())
        Xbar, _ = plane(sv)
        x0n, wn = inputs(Xbar, 99)
        x0, w = T(x0n), T(wn)
        J, c, dx = (torch.full((B, S), SENT, dtype=torch.float64, device=dev()) for _ in range(3))
        fb = torch.full((B,), -77, dtype=torch.int32, device=dev())
        Xo = torch.full((B, S, N, n), SENT, dtype=torch.float64, device=dev())
        Uo = torch.full((B, S, N - 1, m), SENT, dtype=torch.float64, device=dev())
        host = np.zeros((B, S, N, n))
        hp = C.c_void_p(host.ctypes.data)
        paths = altro._lib.hip_runtimes()
        assert len(paths) == 1, paths
        rt = C.CDLL(paths[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        base, size = C.c_void_p(), C.c_size_t()
        assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(Xo)) == 0
        short = C.c_void_p(base.value + size.value - (B * S * N * n * 8 - 8))      # the last B * nsamp * N * n - 1 doubles of Xout's allocation
        W = L.altro_batch_simulate_policy_dev
        full = lambda **kw: [kw.get(k, d) for k, d in (("h", sv.h), ("nsamp", S), ("x0", gp(x0)), ("w", gp(w)), ("clamp", 1), ("J", gp(J)),
                                                      ("c", gp(c)), ("dx", gp(dx)), ("fb", gp(fb)), ("X", gp(Xo)), ("U", gp(Uo)))]
        calls = [full(nsamp=0), full(nsamp=-3), full(clamp=2), full(clamp=-1),
                 full(J=None, c=None, dx=None, fb=None, X=None, U=None),                      # every output NULL
                 full(x0=hp), full(w=hp), full(J=hp), full(c=hp), full(dx=hp), full(fb=hp), full(X=hp), full(U=hp),   # host pointers
                 full(X=short)]                                                               # one element short
        msgs = []
        for i, args in enumerate(calls):
            rc = W(*args)
            msg = (L.altro_last_error(sv.h) or b"").decode()
            assert rc == INV and msg, (i, rc, msg)
            msgs.append(msg)
        assert "shorter" in msgs[-1]
        assert W(*full(h=None)) == INV and (L.altro_last_error(None) or b"").decode()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        Jh = np.full((B, S), SENT)
        Z = L.altro_batch_simulate_policy
        assert Z(None, S, None, None, 1, Jh.ctypes.data_as(dp), None, None, None, None, None) == INV
        assert Z(sv.h, 0, None, None, 1, Jh.ctypes.data_as(dp), None, None, None, None, None) == INV
        assert Z(sv.h, S, None, None, 3, Jh.ctypes.data_as(dp), None, None, None, None, None) == INV
        assert Z(sv.h, S, None, None, 1, None, None, None, None, None, None) == INV
        # the wrapper refuses a tensor that is not on the solver's device before the library sees it
        with pytest.raises(ValueError):
            altro.simulate_policy(sv, x0.cpu(), w, out=(J, c, dx))
        with pytest.raises(ValueError):
            api._simulate_policy_dev(sv, x0.cpu(), w, None, True, (J, c, dx))
        if torch.cuda.device_count() > 1:
            with pytest.raises(ValueError):
                altro.simulate_policy(sv, x0.to(torch.device("cuda", 1)), w, out=(J, c, dx))
        torch.cuda.synchronize()
        altro.synchronize(sv)
        for t in (J, c, dx, Xo, Uo):
            assert (t == SENT).all()
        assert (fb == -77).all() and (Jh == SENT).all()
        assert_twins(sv, tw, cs.x0, 1, "after the refusals")
        assert W(*full(J=None, c=None, dx=None, X=None, U=None)) == 0                          # fb alone is fine
        assert W(*full(x0=None, w=None, fb=None, X=None, U=None, c=None, dx=None)) == 0      # J alone too
        torch.cuda.synchronize()
        assert (H(fb) == 1).all() and (J != SENT).all() and (c == SENT).all()
        altro.solve(sv), altro.solve(tw)
        assert_twins(sv, tw, cs.x0, 1, "after the next solve")
    finally:
        sv.close(), tw.close()


@pytest.mark.parametrize("n,m", [(12, 4), (7, 3)])
def test_state_errors(n, m):
    """a handle on which nothing but create has happened, then with dynamics and no cost, then with no reference:
    ALTRO_ERR_STATE from both forms, nothing written"""
    L = altro._lib.lib()
    B, N = 3, 6
    h = C.c_void_p()
    dims = altro._lib.Dims(B, n, m, N)
    assert L.altro_batch_create(C.byref(dims), None, 0, C.byref(h)) == 0
    try:
        J = torch.full((B, 2), 7.0, dtype=torch.float64, device=dev())
        fb = torch.full((B,), -77, dtype=torch.int32, device=dev())
        gp = lambda t: C.c_void_p(t.data_ptr())
        dp = C.POINTER(C.c_double)
        Jh = np.full((B, 2), 7.0)
        rng = np.random.default_rng(5)

        def refused(what):
            assert L.altro_batch_simulate_policy_dev(h, 2, None, None, 1, gp(J), None, None, gp(fb), None, None) == STATE, what
            assert (L.altro_last_error(h) or b"").decode(), what
            assert L.altro_batch_simulate_policy(h, 2, None, None, 1, Jh.ctypes.data_as(dp), None, None, None, None, None) == STATE, what
            torch.cuda.synchronize()
            assert (J == 7.0).all() and (fb == -77).all() and (Jh == 7.0).all(), what
        refused("nothing set")
        A, Bm = api._c(np.eye(n) + 0.1 * rng.standard_normal((n, n))), api._c(rng.standard_normal((n, m)))
        assert L.altro_batch_set_dynamics(h, api._p(A), api._p(Bm), None, 0, 0) == 0
        refused("no cost")
        assert L.altro_batch_set_tracking_cost(h, api._p(np.ones(n)), api._p(np.ones(m)), api._p(np.ones(n)), 0.1) == 0
        refused("no reference")
    finally:
        L.altro_batch_destroy(h)
