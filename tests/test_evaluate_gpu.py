"""Caller-supplied trajectories scored on the device (altro_batch_evaluate_dev / altro_batch_evaluate) on both backends.

Shapes: batch 5 with ncand = 3 -- 15 rows, a partial wave of the 16-lane kernels -- and N = 9, except the size limits (64, 32) at
batch 2, N = 4.  Per instance candidate 0 is small (inside every control constraint by construction), candidate 1 is pushed
outside the control bounds, candidate 2 is random; the CPU oracle judges which are feasible.

Tolerances are the derived rounding bounds of tests/evaluate_ref.py (its docstring has the derivations; u = 2^-53, nz = n + m,
T = N nz), none of them measured:
 1. rollout, one step at a time, against numpy on the kernel's own Xout: |x_{k+1} - (A x_k + B u_k + f)|_i <= 2 (nz + 2) u S_i,
    S_i = (|A||x_k| + |B||u_k| + |f|)_i -- never against a numpy rollout, whose error grows with ||A||^k; Xout[:, :, 0] == x0.
 2. defect of the given form on (Xout, U) <= max S-bound; on an X with one element moved by 1e-3 it equals numpy's within it.
 3. J against numpy on the same (X, U): |dJ| <= 2 (T + 8) u J.
 4. c_max against numpy: E = 2 (nz + 2) u (|A_r||z| + |b_r|) for rows, 2 u (|z| + |bound|) for BOX sides,
    sqrt(p) E + 16 u |v|_2 for a cone of dimension p.
 5. oracle: a fresh OracleSolver with zero duals per (instance, candidate) takes the controls; (X_orc, U) scored in the given
    form gives its c_max within bound 4 and, where the oracle finds the candidate feasible, its cost within bound 3.

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

pytestmark = pytest.mark.gpu
INV, STATE = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_STATE
OPTS = dict(mpc.REF_OPTS, iterations=60)

CASES = {
    "16-box(12,4)": (ER.case_16_box, {}),
    "16-soc(6,3)": (ER.case_16_soc, {}),
    "wide-rows(20,5)": (ER.case_wide_rows, dict(shared=("dyn", "cost", "box", 1, 2))),
    "wide-ltv(12,12)": (ER.case_wide_ltv, dict(per_knot_dyn=True)),
    "wide-cone(7,3)": (ER.case_wide_cone, dict(shared=("box", 2))),
    "wide-box(30,25)": (ER.case_wide_box, dict(shared=("dyn", "box"))),
    "wide-limits(64,32)": (ER.case_wide_limits, {}),
}
ORACLE_CASES = ["16-box(12,4)", "16-soc(6,3)", "wide-cone(7,3)"]


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev())


def H(t):
    return None if t is None else t.cpu().numpy()


def solver_of(cs, kw):
    return altro.ALTROSolver(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**OPTS))


def ev(sv, U=None, X=None, x0=None, Xout=False):
    """device form on numpy inputs: (J, c_max, defect[, Xout]) back as numpy"""
    Ut = None if U is None else T(U)
    Xo = None
    if Xout:
        Xo = torch.full(tuple(U.shape[:-2]) + (sv.N, sv.n), np.nan, dtype=torch.float64, device=dev())
    out = tuple(torch.full(tuple(U.shape[:-2]) if U is not None else (sv.B,), np.nan, dtype=torch.float64, device=dev()) for _ in range(3))
    J, c, d = altro.evaluate(sv, Ut, X=None if X is None else T(X), x0=None if x0 is None else T(x0), out=out, Xout=Xo)
    torch.cuda.synchronize()
    return (H(J), H(c), H(d)) + ((H(Xo),) if Xout else ())


@functools.lru_cache(maxsize=None)
def scored(name):
    """every device call a case's tests look at, made once"""
    make, kw = CASES[name]
    cs = make()
    U = ER.candidates(cs, 5)
    r = NS(cs=cs, U=U, kw=kw)
    sv = solver_of(cs, kw)
    try:
        r.J, r.c, r.d, r.X = ev(sv, U, Xout=True)                       # rollout form with Xout
        r.J0, r.c0, r.d0 = ev(sv, U)                                    # rollout form into the workspace
        r.Jg, r.cg, r.dg = ev(sv, U, X=r.X)                             # given form on (Xout, U)
        r.J2, r.c2, r.d2, r.X2 = ev(sv, U, Xout=True)                   # a second identical call
        r.alone = [ev(sv, U[:, c:c + 1], Xout=True) for c in range(U.shape[1])]
        Jh, ch, dh = (np.empty(U.shape[:2]) for _ in range(3))
        Xh = np.empty(r.X.shape)
        altro.evaluate(sv, U, out=(Jh, ch, dh), Xout=Xh)                # host twin, rollout form
        r.host = (Jh, ch, dh, Xh)
        r.hostg = altro.evaluate(sv, U, X=r.X)                          # host twin, given form
        r.x0b = cs.x0 + 0.25
        r.Jx, r.cx, r.dx, r.Xx = ev(sv, U, x0=r.x0b, Xout=True)          # a caller's x0
        r.Xp = r.X.copy()
        r.Xp[:, :, cs.N // 2, 1] += 1e-3
        r.Jp, r.cp, r.dp = ev(sv, U, X=r.Xp)
        r.one = (ev(sv, U[:, 1], Xout=True), ev(sv, U[:, 1], X=r.X[:, 1]))   # U (B, N-1, m): outputs (B,)
    finally:
        sv.close()
    return r


@functools.lru_cache(maxsize=None)
def judged(name, O):
    r = scored(name)
    return ER.oracle_scores(O, r.cs, r.U, per_knot_dyn=bool(r.kw.get("per_knot_dyn")))


def saw_both(name, O):
    """the candidates of the case hold at least one the oracle finds feasible and one it finds infeasible; where only controls
    are bounded, candidate 0 is feasible and candidate 1 infeasible by construction"""
    r = scored(name)
    _, _, co = judged(name, O)
    assert (co == 0.0).any() and (co > 0.0).any(), name
    if ER.controls_only_box(r.cs):
        assert (co[:, 0] == 0.0).all() and (co[:, 1] > 0.0).all(), name
    return co


@pytest.mark.parametrize("name", list(CASES))
def test_rollout_one_step_at_a_time(name, oracle):
    """bound 1 on the kernel's own Xout, and x_0 copied exactly (the handle's own x0 and a caller's)"""
    r = scored(name)
    saw_both(name, oracle)
    res, S = ER.step_residual(r.cs, r.X, r.U)
    print(name, "max residual / bound", (res / ER.step_bound(r.cs, S)).max())
    assert np.isfinite(r.X).all()
    assert (res <= ER.step_bound(r.cs, S)).all()
    assert (r.X[:, :, 0] == r.cs.x0[:, None]).all() and (r.Xx[:, :, 0] == r.x0b[:, None]).all()
    resx, Sx = ER.step_residual(r.cs, r.Xx, r.U)
    assert (resx <= ER.step_bound(r.cs, Sx)).all()
    assert r.d.tobytes() == np.zeros_like(r.d).tobytes() and r.d0.tobytes() == r.d.tobytes()      # +0.0 in the rollout form


@pytest.mark.parametrize("name", list(CASES))
def test_defect(name, oracle):
    """bound 2: the given form on what the rollout wrote, and on an X with one element of one knot moved by 1e-3"""
    r = scored(name)
    saw_both(name, oracle)
    _, bound = ER.defect(r.cs, r.X, r.U)
    print(name, "defect / bound", (r.dg / bound).max())
    assert (r.dg <= bound).all()
    want, boundp = ER.defect(r.cs, r.Xp, r.U)
    assert (want > 1e-4).all()
    assert (np.abs(r.dp - want) <= boundp).all(), np.abs(r.dp - want).max()


@pytest.mark.parametrize("name", list(CASES))
def test_cost_and_violation_match_numpy(name, oracle):
    """bounds 3 and 4 against numpy on the same doubles, for the rolled-out, the caller's-x0 and the perturbed trajectories;
    the oracle has found feasible and infeasible candidates among them"""
    r = scored(name)
    for X, J, c, what in ((r.X, r.J, r.c, "rollout"), (r.Xx, r.Jx, r.cx, "x0"), (r.Xp, r.Jp, r.cp, "perturbed")):
        Jn, Jb = ER.cost(r.cs, X, r.U)
        cn, cb = ER.violation(r.cs, X, r.U)
        print(name, what, "dJ / bound", (np.abs(J - Jn) / Jb).max(), "dc - bound", (np.abs(c - cn) - cb).max())
        assert (np.abs(J - Jn) <= Jb).all(), what
        assert (np.abs(c - cn) <= cb).all(), what
    saw_both(name, oracle)


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_oracle_semantics(name, oracle):
    """bound 5: the oracle's own states scored in the given form"""
    r = scored(name)
    Xo, Jo, co = judged(name, oracle)
    sv = solver_of(r.cs, r.kw)
    try:
        J, c, d = ev(sv, r.U, X=Xo)
    finally:
        sv.close()
    _, cb = ER.violation(r.cs, Xo, r.U)
    _, Jb = ER.cost(r.cs, Xo, r.U)
    assert (np.abs(c - co) <= cb).all(), np.abs(c - co).max()
    feas = saw_both(name, oracle) == 0.0
    assert (np.abs(J - Jo)[feas] <= Jb[feas]).all(), (np.abs(J - Jo)[feas] / Jb[feas]).max()
    assert (d <= ER.defect(r.cs, Xo, r.U)[1]).all()


@pytest.mark.parametrize("name", list(CASES))
def test_byte_equalities(name, oracle):
    """rollout form == given form on (Xout, U) in J and c_max; with and without Xout; a second identical call; every candidate
    alone (ncand = 1); the (B, N-1, m) shape; the host twin, both forms"""
    r = scored(name)
    saw_both(name, oracle)
    same = lambda a, b: a.tobytes() == b.tobytes()
    assert same(r.J, r.Jg) and same(r.c, r.cg)
    assert same(r.J, r.J0) and same(r.c, r.c0)
    assert same(r.J, r.J2) and same(r.c, r.c2) and same(r.d, r.d2) and same(r.X, r.X2)
    for c, (Ja, ca, da, Xa) in enumerate(r.alone):
        assert same(Ja[:, 0], np.ascontiguousarray(r.J[:, c])) and same(ca[:, 0], np.ascontiguousarray(r.c[:, c])), c
        assert same(Xa[:, 0], np.ascontiguousarray(r.X[:, c])), c
    (J1, c1, d1, X1), (J1g, c1g, d1g) = r.one
    assert J1.shape == (r.cs.B,) and same(J1, np.ascontiguousarray(r.J[:, 1])) and same(c1, np.ascontiguousarray(r.c[:, 1]))
    assert same(J1g, J1) and same(c1g, c1) and same(d1g, np.ascontiguousarray(r.dg[:, 1]))
    Jh, ch, dh, Xh = r.host
    assert same(Jh, r.J) and same(ch, r.c) and same(dh, r.d) and same(Xh, r.X)
    assert same(r.hostg[0], r.Jg) and same(r.hostg[1], r.cg) and same(r.hostg[2], r.dg)


@pytest.mark.parametrize("name", ["16-box(12,4)", "16-soc(6,3)", "wide-cone(7,3)", "wide-ltv(12,12)"])
def test_instance_alone_on_a_batch_one_handle(name, oracle):
    """instance b on a batch-1 handle holding its rows of data: the bytes it gets inside the batch"""
    r = scored(name)
    saw_both(name, oracle)
    for b in range(r.cs.B):
        sv = solver_of(ER.sub_case(r.cs, b), {k: v for k, v in r.kw.items() if k == "per_knot_dyn"})
        try:
            J, c, d, X = ev(sv, r.U[b:b + 1], Xout=True)
            Jg, cg, dg = ev(sv, r.U[b:b + 1], X=r.Xp[b:b + 1])
        finally:
            sv.close()
        assert J.tobytes() == r.J[b:b + 1].tobytes() and c.tobytes() == r.c[b:b + 1].tobytes() and X.tobytes() == r.X[b:b + 1].tobytes(), b
        assert Jg.tobytes() == r.Jp[b:b + 1].tobytes() and cg.tobytes() == r.cp[b:b + 1].tobytes() and dg.tobytes() == r.dp[b:b + 1].tobytes(), b


def test_rollout_wrapper_returns_the_states_of_the_rollout_form():
    """api.rollout on GPU tensors (twice: the second call reuses the solver's scratch output) and on numpy, and
    ExternalMPC.evaluate: the bytes of evaluate's Xout and scores"""
    r = scored("16-box(12,4)")
    sv = solver_of(r.cs, r.kw)
    try:
        Ut = T(r.U)
        for _ in range(2):
            X = altro.rollout(sv, Ut)
            torch.cuda.synchronize()
            assert tuple(X.shape) == r.X.shape and H(X).tobytes() == r.X.tobytes()
        X1 = altro.rollout(sv, T(r.U[:, 1]), x0=T(r.x0b))
        torch.cuda.synchronize()
        assert H(X1).tobytes() == np.ascontiguousarray(r.Xx[:, 1]).tobytes()
        assert altro.rollout(sv, r.U).tobytes() == r.X.tobytes()
        J, c, d = altro.ExternalMPC(sv).evaluate(Ut)
        torch.cuda.synchronize()
        assert H(J).tobytes() == r.J.tobytes() and H(c).tobytes() == r.c.tobytes()
    finally:
        sv.close()


# ---------------------------------------------------------------------------------------------- the solver's own trajectory
def random_linear(B, n, m, seed, u_bnd=3.0, steps=8, N=9):
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=steps, seed=seed, u_bnd=u_bnd)
    return pb


@pytest.mark.parametrize("force_wide", [False, True])
def test_own_trajectory_after_a_converged_solve(monkeypatch, force_wide):
    """evaluate(U = None) after a solve: c_max equals altro_batch_get_stats's within bound 4 and defect <= max S-bound, with
    bounds that are active (u_bnd = 1) and with bounds that never are (u_bnd = 50: every dual is zero after the solve, the
    reported cost has no AL term and J equals it within bound 3)"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    for u_bnd, slack in ((1.0, False), (50.0, True)):
        pb = random_linear(5, 12, 4, 31, u_bnd=u_bnd)
        prob = mpc.gen_tracking_problem(pb)
        prob.x0 = prob.x0 + 0.3 * np.random.default_rng(4).standard_normal(prob.x0.shape)
        sv = altro.ALTROSolver(prob, altro.SolverOptions(**mpc.REF_OPTS))
        try:
            altro.solve(sv)
            st = altro.stats(sv)
            print("u_bnd", u_bnd, "status", st.status, "iterations", st.iterations)
            assert (st.status == altro.SOLVE_SUCCEEDED).all()
            X, U = altro.states(sv)[:, None], altro.controls(sv)[:, None]
            J, c, d = ev(sv)
            Jh, ch, dh = altro.evaluate(sv)
            cs = ER.case_of_batch(pb, [0] * 5, prob.x0)
            cn, cb = ER.violation(cs, X, U)
            Jn, Jb = ER.cost(cs, X, U)
            assert J.shape == (5,) and J.tobytes() == Jh.tobytes() and c.tobytes() == ch.tobytes() and d.tobytes() == dh.tobytes()
            assert (np.abs(c - cn[:, 0]) <= cb[:, 0]).all() and (np.abs(J - Jn[:, 0]) <= Jb[:, 0]).all()
            assert (np.abs(c - st.c_max) <= cb[:, 0]).all(), np.abs(c - st.c_max).max()
            assert (d <= ER.defect(cs, X, U)[1][:, 0]).all()
            if slack:
                assert not altro.get_duals(sv, 0).any() and (c == 0.0).all()
                assert (np.abs(J - st.cost) <= Jb[:, 0]).all(), (np.abs(J - st.cost) / Jb[:, 0]).max()
            else:
                assert altro.get_duals(sv, 0).any()
        finally:
            sv.close()


# ---------------------------------------------------------------------------------------------- seen as the next solve sees it
@pytest.mark.parametrize("name", ["16-box(12,4)", "16-soc(6,3)", "wide-cone(7,3)"])
def test_sees_device_setters_earlier_on_the_stream(name):
    """set_reference_dev, set_bounds_dev (per-instance rows) and update_constraint_data_dev, then evaluate, nothing synchronised
    in between: J and c_max are those of the new data"""
    make, kw = CASES[name]
    cs = make()
    U = ER.candidates(cs, 6)
    rng = np.random.default_rng(21)
    sv = solver_of(cs, kw)
    try:
        before = ev(sv, U)
        cs.Xref = cs.Xref + 0.5 * rng.standard_normal(cs.Xref.shape)
        cs.Uref = cs.Uref + 0.2 * rng.standard_normal(cs.Uref.shape)
        ten = [T(cs.Xref), T(cs.Uref)]
        for i, c in enumerate(cs.cons):
            if c.kind == "box":
                ub = 0.3 + 0.4 * rng.random((cs.B, cs.m))
                c.zmin[:, cs.n:], c.zmax[:, cs.n:] = -ub, ub
                ten += [T(c.zmin), T(c.zmax)]
            else:
                c.A, c.b = c.A * (0.6 + rng.random(c.A.shape)), c.b * (0.6 + 0.8 * rng.random(c.b.shape))
                sh = i in kw.get("shared", ())
                if sh:   # one block for the batch: every instance gets instance 0's new rows
                    c.A[:], c.b[:] = c.A[0, 0], c.b[0, 0]
                ten += [T(c.A[0, 0] if sh else c.A), T(c.b[0, 0] if sh else c.b)]
        Ut = T(U)
        it = iter(ten)
        altro.update_trajectory(sv, next(it), next(it))
        for i, c in enumerate(cs.cons):
            if c.kind == "box":
                altro.set_bounds(sv, i, next(it), next(it))
            else:
                altro.update_constraint_data(sv, i, next(it), next(it))
        Xo = torch.empty(U.shape[:2] + (cs.N, cs.n), dtype=torch.float64, device=dev())
        J, c_, d = altro.evaluate(sv, Ut, Xout=Xo)
        torch.cuda.synchronize()
        J, c_, X = H(J), H(c_), H(Xo)
        Jn, Jb = ER.cost(cs, X, U)
        cn, cb = ER.violation(cs, X, U)
        assert (np.abs(J - Jn) <= Jb).all() and (np.abs(c_ - cn) <= cb).all()
        assert altro.dev_refusals(sv) == 0
        assert (np.abs(J - before[0]) > 100 * Jb).all() and (c_ != before[1]).any()     # (the new data is not the old)
    finally:
        sv.close()


@pytest.mark.parametrize("force_wide", [False, True])
def test_staggered_clocks_score_against_their_own_window(monkeypatch, force_wide):
    """three MPC steps under a clock with starts 0, 1, 2, 0, 1: each instance is scored against the window it holds"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    pb = random_linear(5, 12, 4, 33)
    mp = mpc.BatchMPC(pb, altro.SolverOptions(**OPTS))
    try:
        mp.initial_solve()
        mp.set_clock(np.array([0, 1, 2, 0, 1]))
        mp.run_async(3, first=0)
        mp.synchronize()
        win = api.get_clock(mp.solver)[2]
        assert list(win) == [3, 2, 1, 3, 2]
        cs = ER.case_of_batch(pb, win, mp.x0())
        U = ER.candidates(cs, 7)
        J, c, d, X = ev(mp.solver, U, Xout=True)
        Jn, Jb = ER.cost(cs, X, U)
        cn, cb = ER.violation(cs, X, U)
        assert (X[:, :, 0] == cs.x0[:, None]).all()
        assert (np.abs(J - Jn) <= Jb).all() and (np.abs(c - cn) <= cb).all()
        other = ER.case_of_batch(pb, [3] * 5, mp.x0())
        assert (np.abs(J - ER.cost(other, X, U)[0])[[1, 2, 4]] > 100 * Jb[[1, 2, 4]]).all()
        Jo, co, do = ev(mp.solver)                                      # own trajectory: the same windows
        Xs, Us = altro.states(mp.solver)[:, None], altro.controls(mp.solver)[:, None]
        Jn, Jb = ER.cost(cs, Xs, Us)
        assert (np.abs(Jo - Jn[:, 0]) <= Jb[:, 0]).all()
    finally:
        mp.solver.close()


def test_dynamics_track_blocks_of_the_current_window():
    """altro_mpc_set_dynamics_track (step_stride = 1), two MPC steps: the rollout and the defect use blocks 2 .. 2 + N - 2"""
    B, N, S = 5, 9, 3
    cs = ER.case_wide_ltv(B, N)
    rng = np.random.default_rng(41)
    nb = N + S + 1
    A = np.eye(12) + 0.3 * rng.standard_normal((B, nb, 12, 12)) / np.sqrt(12)
    Bm = 0.5 * rng.standard_normal((B, nb, 12, 12))
    f = 0.05 * rng.standard_normal((B, nb, 12))
    Xt, Ut = rng.standard_normal((B, nb, 12)), 0.3 * rng.standard_normal((B, nb - 1, 12))
    cs.A, cs.Bm, cs.f = A[:, :N - 1].copy(), Bm[:, :N - 1].copy(), f[:, :N - 1].copy()
    cs.Xref, cs.Uref, cs.x0 = Xt[:, :N].copy(), Ut[:, :N - 1].copy(), Xt[:, 0].copy()
    mp = mpc.TrackMPC(ER.to_problem(altro, cs, per_knot_dyn=True), altro.SolverOptions(**dict(OPTS, iterations=8)), Xt, Ut,
                      rng.standard_normal((S, B, 12)), (np.full(12, 1e-3),))
    try:
        altro.set_dynamics_track(mp.solver, A, Bm, f, step_stride=1)
        mp.initial_solve()
        mp.run_async(2, first=0)
        mp.synchronize()
        cs.A, cs.Bm, cs.f = A[:, 2:2 + N - 1].copy(), Bm[:, 2:2 + N - 1].copy(), f[:, 2:2 + N - 1].copy()
        cs.Xref, cs.Uref, cs.x0 = Xt[:, 2:2 + N].copy(), Ut[:, 2:2 + N - 1].copy(), mp.x0()
        U = ER.candidates(cs, 8)
        J, c, d, X = ev(mp.solver, U, Xout=True)
        res, Sb = ER.step_residual(cs, X, U)
        assert (res <= ER.step_bound(cs, Sb)).all()
        Jn, Jb = ER.cost(cs, X, U)
        cn, cb = ER.violation(cs, X, U)
        assert (np.abs(J - Jn) <= Jb).all() and (np.abs(c - cn) <= cb).all()
        Jg, cg, dg = ev(mp.solver, U, X=X)
        assert Jg.tobytes() == J.tobytes() and (dg <= ER.defect(cs, X, U)[1]).all()
    finally:
        mp.solver.close()


# ---------------------------------------------------------------------------------------------- owns nothing
def everything(sv, x):
    """all the library owns that a caller can read"""
    st = altro.stats(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), it=st.iterations, ito=st.iterations_outer, status=st.status, cost=st.cost,
               cmax=st.c_max, Jt=st.cost_trace, ct=st.cmax_trace, alpha=altro.alpha_trace(sv), dual=altro.get_duals(sv, 0))
    out["K"], out["d"] = altro.gains(sv)
    for k, v in zip(("bw", "ro", "tr"), altro.work_counters(sv)):
        out[k] = v
    for k, v in zip(("ns", "ni", "nok"), altro.solve_counters(sv)):
        out[k] = v
    out["conf"], out["reuse"] = altro.confirm_counter(sv), altro.reuse_counter(sv)
    fb = np.zeros(sv.B, dtype=np.int32)
    out["u"] = altro.eval_policy(sv, x, fb=fb)
    out["fb"] = fb
    return out


@pytest.mark.parametrize("force_wide", [False, True])
def test_owns_nothing(monkeypatch, force_wide):
    """twin handles run a solve and four MPC steps; one of them has evaluate calls in all three forms (device and host)
    between the steps: states, controls, duals, statistics, traces, counters, gains and the policy's fb are bit-identical.
    A mask with inactive instances does not change anybody's scores."""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    pb = random_linear(5, 12, 4, 35)
    a, b = (mpc.BatchMPC(pb, altro.SolverOptions(**mpc.REF_OPTS)) for _ in range(2))
    try:
        cs = ER.case_of_batch(pb, [0] * 5, a.x0())
        U = ER.candidates(cs, 9)
        for mp in (a, b):
            altro.timing_reset(mp.solver)
            mp.initial_solve()
        for i in range(4):
            X = ev(b.solver, U, Xout=True)[3]
            ev(b.solver, U)
            ev(b.solver, U, X=X)
            ev(b.solver)
            altro.evaluate(b.solver, U)
            altro.evaluate(b.solver)
            for mp in (a, b):
                mp.step(i)
            ea, eb = everything(a.solver, cs.x0), everything(b.solver, cs.x0)
            for k in ea:
                assert np.array_equal(ea[k], eb[k], equal_nan=True), (i, k)
        free = ev(b.solver, U) + ev(b.solver)
        b.set_active(np.array([1, 0, 1, 0, 0]))
        masked = ev(b.solver, U) + ev(b.solver)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(free, masked))
        a.set_active(np.array([1, 0, 1, 0, 0]))
        for mp in (a, b):
            mp.step(4)
        ea, eb = everything(a.solver, cs.x0), everything(b.solver, cs.x0)
        for k in ea:
            assert np.array_equal(ea[k], eb[k], equal_nan=True), ("masked", k)
    finally:
        a.solver.close(), b.solver.close()


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("force_wide", [False, True])
def test_refusals_launch_nothing(monkeypatch, force_wide):
    """every ALTRO_ERR_INVALID_ARG case of the contract, a host pointer and a buffer one element short: error 1 with a message,
    the sentinel in every output untouched, and the next solve equals a twin's"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    pb = random_linear(5, 12, 4, 37)
    prob = mpc.gen_tracking_problem(pb)
    sv, tw = (altro.ALTROSolver(prob, altro.SolverOptions(**mpc.REF_OPTS)) for _ in range(2))
    try:
        L, B, n, m, N, nc = sv._L, sv.B, sv.n, sv.m, sv.N, 3
        gp = lambda t: C.c_void_p(t.data_ptr())
        U = T(ER.candidates(ER.case_of_batch(pb, [0] * 5, prob.x0), 3))
        X = torch.zeros((B, nc, N, n), dtype=torch.float64, device=dev())
        x0 = T(prob.x0)
        SENT = -12345.5
        J, c, d = (torch.full((B, nc), SENT, dtype=torch.float64, device=dev()) for _ in range(3))
        Xo = torch.full((B, nc, N, n), SENT, dtype=torch.float64, device=dev())
        host = np.zeros((B, nc, N, n))
        hp = C.c_void_p(host.ctypes.data)
        paths = altro._lib.hip_runtimes()
        assert len(paths) == 1, paths
        rt = C.CDLL(paths[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        base, size = C.c_void_p(), C.c_size_t()
        assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(J)) == 0
        short = C.c_void_p(base.value + size.value - (B * nc * 8 - 8))       # the last B * ncand - 1 doubles of J's allocation
        E = L.altro_batch_evaluate_dev
        calls = [lambda: E(sv.h, 0, gp(U), None, None, gp(J), gp(c), gp(d), None),           # ncand < 1
                 lambda: E(sv.h, -2, gp(U), None, None, gp(J), gp(c), gp(d), None),
                 lambda: E(sv.h, 2, None, None, None, gp(J), gp(c), gp(d), None),            # own trajectory: ncand != 1
                 lambda: E(sv.h, 1, None, gp(X), None, gp(J), gp(c), gp(d), None),           # ... with X
                 lambda: E(sv.h, 1, None, None, gp(x0), gp(J), gp(c), gp(d), None),          # ... with x0
                 lambda: E(sv.h, 1, None, None, None, gp(J), gp(c), gp(d), gp(Xo)),          # ... with Xout
                 lambda: E(sv.h, nc, gp(U), gp(X), gp(x0), gp(J), gp(c), gp(d), None),       # X with x0
                 lambda: E(sv.h, nc, gp(U), gp(X), None, gp(J), gp(c), gp(d), gp(Xo)),       # X with Xout
                 lambda: E(sv.h, nc, gp(U), None, None, None, None, None, gp(Xo)),           # no output
                 lambda: E(sv.h, nc, hp, None, None, gp(J), gp(c), gp(d), gp(Xo)),           # host pointers
                 lambda: E(sv.h, nc, gp(U), hp, None, gp(J), gp(c), gp(d), None),
                 lambda: E(sv.h, nc, gp(U), None, hp, gp(J), gp(c), gp(d), None),
                 lambda: E(sv.h, nc, gp(U), None, None, gp(J), hp, gp(d), None),
                 lambda: E(sv.h, nc, gp(U), None, None, gp(J), gp(c), gp(d), hp),
                 lambda: E(sv.h, nc, gp(U), None, None, short, gp(c), gp(d), gp(Xo))]        # one element short
        msgs = []
        for i, call in enumerate(calls):
            rc = call()
            msg = (L.altro_last_error(sv.h) or b"").decode()
            assert rc == INV and msg, (i, rc, msg)
            msgs.append(msg)
        assert "shorter" in msgs[14]
        assert E(None, nc, gp(U), None, None, gp(J), gp(c), gp(d), None) == INV and (L.altro_last_error(None) or b"").decode()
        assert L.altro_batch_evaluate(None, 1, None, None, None, None, None, None, None) == INV
        assert L.altro_batch_evaluate(sv.h, 1, None, None, None, None, None, None, None) == INV
        assert L.altro_batch_evaluate(sv.h, 0, None, None, None, host.ctypes.data_as(C.POINTER(C.c_double)), None, None, None) == INV
        torch.cuda.synchronize()
        altro.synchronize(sv)
        for t in (J, c, d, Xo):
            assert (t == SENT).all()
        assert E(sv.h, nc, gp(U), None, None, gp(J), None, None, None) == 0                  # J alone is fine
        altro.solve(sv), altro.solve(tw)
        ea, eb = everything(sv, prob.x0), everything(tw, prob.x0)
        for k in ea:
            assert np.array_equal(ea[k], eb[k], equal_nan=True), k
        assert (H(J) != SENT).all() and (c == SENT).all()
    finally:
        sv.close(), tw.close()


@pytest.mark.parametrize("n,m", [(12, 4), (7, 3)])
def test_state_error_before_set_dynamics(n, m):
    """a handle on which nothing but create has happened: ALTRO_ERR_STATE from both forms, nothing written"""
    L = altro._lib.lib()
    B, N = 3, 6
    h = C.c_void_p()
    dims = altro._lib.Dims(B, n, m, N)
    assert L.altro_batch_create(C.byref(dims), None, 0, C.byref(h)) == 0
    try:
        U = torch.zeros((B, 1, N - 1, m), dtype=torch.float64, device=dev())
        J = torch.full((B, 1), 7.0, dtype=torch.float64, device=dev())
        gp = lambda t: C.c_void_p(t.data_ptr())
        assert L.altro_batch_evaluate_dev(h, 1, gp(U), None, None, gp(J), None, None, None) == STATE
        assert (L.altro_last_error(h) or b"").decode()
        assert L.altro_batch_evaluate_dev(h, 1, None, None, None, gp(J), None, None, None) == STATE
        Jh = np.full((B, 1), 7.0)
        dp = C.POINTER(C.c_double)
        assert L.altro_batch_evaluate(h, 1, np.zeros((B, 1, N - 1, m)).ctypes.data_as(dp), None, None, Jh.ctypes.data_as(dp), None, None, None) == STATE
        torch.cuda.synchronize()
        assert (J == 7.0).all() and (Jh == 7.0).all()
    finally:
        L.altro_batch_destroy(h)
