"""The table of tests/scoring_matrix.py on the device: every call built on the scoring core (evaluate, evaluate_grad, evaluate_al,
warm_start, simulate_policy) at the row tables, LDS sizes and shapes the seven cases of tests/evaluate_ref.py do not reach --
against the numpy yardsticks of the calls' own test files, whose helpers are imported, not restated.

Tolerances are the derived rounding bounds of tests/evaluate_ref.py (1 - 4), tests/evaluate_grad_ref.py (5 - 8) and
tests/evaluate_al_ref.py (A - G), none of them measured on the device; everything else is an equality of bytes.  err / bound is
printed for every array compared under a bound.

The guards of tests/test_scoring_matrix.py (on numpy and the oracle) are checked again where they depend on what the device
computed (the duals and the penalty of its own short solve, the status of the solve that provides gains).
"""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro

import evaluate_al_ref as AR
import evaluate_grad_ref as GR
import evaluate_ref as ER
import scoring_matrix as sm
import test_evaluate_al_gpu as TA
import test_evaluate_gpu as TE
import test_evaluate_grad_gpu as TG
import test_simulate_gpu as TM
import test_warm_start_gpu as TW
import warm_start_ref as WR
import wide_matrix as wm

pytestmark = pytest.mark.gpu
U_ = ER.U_
same = TW.same
RHO_WS = 1e3
S = TM.S


def test_the_oracle_guards_use_the_options_of_the_device_solves():
    """guard (h) of the CPU file solves on the oracle with scoring_matrix.AL_OPTS / SIM_OPTS: they are the options of the sibling
    files' device solves (projected_newton is a switch of the library alone: the polish, off for the short solve)"""
    assert sm.AL_OPTS == {k: v for k, v in TA.SOLVE.items() if k != "projected_newton"} and TA.SOLVE["projected_newton"] is False
    assert sm.SIM_OPTS == dict(TM.OPTS) and sm.sim_opts("wide(32,32)") is sm.SIM_OPTS
    assert {k: v for k, v in sm.QUADS_SIM_OPTS.items() if k != "iterations"} == {k: v for k, v in wm.ROWS_OPTS.items()}


def solver(name, opts):
    cs, _, kw = sm.build(name)
    return altro.ALTROSolver(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**opts))


def ratio(err, bound):
    """largest err / bound (0 where both are 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


def warm(sv, cs, U, inc):
    """the handle reset to (zero states, reference controls), the incumbent scored by evaluate, then the warm start: NS(chosen, J, c,
    plane (X, U), Ji, ci, Xi of the incumbent)"""
    TW.set_traj(sv, np.zeros((cs.B, cs.N, cs.n)), cs.Uref)
    Ji, ci, _, Xi = TE.ev(sv, np.ascontiguousarray(cs.Uref[:, None]), Xout=True)
    ch, J, c = TW.ws(sv, U, RHO_WS, inc=inc)
    return NS(chosen=ch, J=J, c=c, plane=TW.plane(sv), Ji=Ji, ci=ci, Xi=Xi)


@functools.lru_cache(maxsize=None)
def scored(name):
    """every device call on a handle that has not solved, made once: evaluate in its four forms, alone and on the host; evaluate_grad
    at rho = 10, 0 and 1 and the two points of a central difference; evaluate_al with zero duals and penalty 1; warm_start"""
    cs, names, kw = sm.build(name)
    U = sm.candidates(name)
    r = NS(cs=cs, U=U, names=names)
    sv = solver(name, TE.OPTS)
    try:
        r.J, r.c, r.d, r.X = TE.ev(sv, U, Xout=True)                      # rollout form with Xout
        r.J0, r.c0, r.d0 = TE.ev(sv, U)                                   # rollout form into the workspace
        r.Jg, r.cg, r.dg = TE.ev(sv, U, X=r.X)                            # given form on (Xout, U)
        r.Xp = r.X.copy()
        r.Xp[:, :, cs.N // 2, 1] += 1e-3
        r.Jp, r.cp, r.dp = TE.ev(sv, U, X=r.Xp)                           # given form on an X with one element moved
        r.alone = [TE.ev(sv, U[:, c:c + 1], Xout=True) for c in range(U.shape[1])]
        Jh, ch, dh = (np.empty(U.shape[:2]) for _ in range(3))
        Xh = np.empty(r.X.shape)
        altro.evaluate(sv, U, out=(Jh, ch, dh), Xout=Xh)                  # host twin
        r.host = (Jh, ch, dh, Xh)
        if name in sm.ORACLE_CASES:
            import oracle_py
            oracle_py.build()
            r.orc = ER.oracle_scores(oracle_py, cs, U, per_knot_dyn=bool(kw.get("per_knot_dyn")))
            r.on_orc = TE.ev(sv, U, X=r.orc[0])
        r.g = {rho: TG.eg(sv, U, rho=rho) for rho in (10.0, 0.0, 1.0)}
        rng = np.random.default_rng(8)
        r.D = rng.standard_normal(U.shape)
        X = r.g[10.0].X
        r.fdg = GR.merit_grad(cs, X, U, 10.0, direction=(GR.tangent(cs, r.D, None), r.D), state_err=GR.rollout_error(cs, X, U))
        r.h = GR.fd_step(r.fdg, 10.0, GR.merit(cs, X, U, 10.0)[1])
        r.pts = []
        for sgn in (1.0, -1.0):
            Up = np.ascontiguousarray(U + sgn * r.h[..., None, None] * r.D)
            r.pts.append((Up, TG.eg(sv, Up, rho=10.0, want=(1, 1, 0, 0))))
        assert (altro.penalty(sv) == 1.0).all()
        r.al0 = TA.al(sv, U)                                              # zero duals, penalty 1
        r.ws = {inc: warm(sv, cs, U, inc) for inc in (True, False)}
    finally:
        sv.close()
    return r


@functools.lru_cache(maxsize=None)
def solved(name):
    """the calls that need a solve, made once: evaluate_al under the duals drawn from a short solve's; simulate_policy (nsamp = 3)
    on the gains of one solve"""
    cs, names, kw = sm.build(name)
    U = sm.candidates(name)
    r = NS(cs=cs, U=U)
    sv = solver(name, TA.SOLVE)
    try:
        altro.solve(sv)
        r.al_status = altro.stats(sv).status.copy()
        r.mu = altro.penalty(sv)
        r.lam0 = TA.duals_of(sv, cs)
        r.lam = AR.draw_duals(cs, r.lam0, r.mu, 77)
        TA.install(sv, r.lam)
        r.al = TA.al(sv, U)
        r.ev = TE.ev(sv, U, Xout=True)
    finally:
        sv.close()
    sv = solver(name, sm.sim_opts(name))
    try:
        altro.solve(sv)
        st = altro.stats(sv)
        r.status, r.iterations, r.pen = st.status.copy(), st.iterations.copy(), altro.penalty(sv)
        r.Xbar, r.Ubar = TW.plane(sv)
        r.x0, r.w = TM.inputs(r.Xbar, 71)
        r.sim = {}
        for clamp in (0, 1):
            q = NS(full=TM.sim(sv, r.x0, r.w, clamp=clamp), now=TM.sim(sv, r.x0, None, clamp=clamp))
            q.pol = np.stack([np.stack([TM.policy(sv, q.full.X[:, s, k], k, clamp) for k in range(cs.N - 1)], axis=1) for s in range(S)], axis=1)
            q.roll_now = np.stack([TM.rollout(sv, np.ascontiguousarray(q.now.U[:, s]), r.x0[:, s]) for s in range(S)], axis=1)
            q.given = TM.given(sv, q.full.X, q.full.U)
            q.given_now = TM.given(sv, q.now.X, q.now.U)
            r.sim[clamp] = q
        r.after = TW.plane(sv)
    finally:
        sv.close()
    return r


# ---------------------------------------------------------------------------------------------- evaluate
@pytest.mark.parametrize("name", sm.CASES)
def test_evaluate_within_bounds_1_to_4(name):
    """bound 1 on the kernel's own Xout, x_0 copied exactly, +0 defect in the rollout form; bound 2 on (Xout, U) and on an X with one
    element moved; bounds 3 and 4 against numpy on the same doubles, rolled out and perturbed"""
    r = scored(name)
    cs = r.cs
    res, Sx = ER.step_residual(cs, r.X, r.U)
    print(name, "evaluate: step residual / bound", ratio(res, ER.step_bound(cs, Sx)))
    assert np.isfinite(r.X).all() and (res <= ER.step_bound(cs, Sx)).all()
    assert (r.X[:, :, 0] == cs.x0[:, None]).all()
    assert r.d.tobytes() == np.zeros_like(r.d).tobytes() and r.d0.tobytes() == r.d.tobytes()
    _, bound = ER.defect(cs, r.X, r.U)
    want, boundp = ER.defect(cs, r.Xp, r.U)
    print(name, "evaluate: defect / bound", ratio(r.dg, bound), "moved", ratio(np.abs(r.dp - want), boundp))
    assert (r.dg <= bound).all() and (want > 1e-4).all() and (np.abs(r.dp - want) <= boundp).all()
    for X, J, c, what in ((r.X, r.J, r.c, "rollout"), (r.Xp, r.Jp, r.cp, "moved")):
        Jn, Jb = ER.cost(cs, X, r.U)
        cn, cb = ER.violation(cs, X, r.U)
        print(name, "evaluate:", what, "dJ / bound", ratio(np.abs(J - Jn), Jb), "dc / bound", ratio(np.abs(c - cn), cb))
        assert np.isfinite(J).all() and np.isfinite(c).all()
        assert (np.abs(J - Jn) <= Jb).all(), what
        assert (np.abs(c - cn) <= cb).all(), what
    # the guards, on what the device computed: the arg-max block of the yardstick's c_max on the device's states is the table's
    g = sm.guards(name)
    win, _, _ = sm.deciders(cs, r.X, r.U)
    sure = g.cmax > 1e-6                                                  # (candidate 0 sits on the equality rows: c_max is rounding there)
    assert (win == g.winner)[sure].all() and sure[:, 1].all()


@pytest.mark.parametrize("name", sm.CASES)
def test_evaluate_byte_equalities_and_the_host_twin(name):
    """rollout then given equals direct; workspace equals Xout; every candidate alone equals the batch call; the host twin"""
    r = scored(name)
    assert same(r.J, r.Jg) and same(r.c, r.cg)
    assert same(r.J, r.J0) and same(r.c, r.c0)
    for c, (Ja, ca, da, Xa) in enumerate(r.alone):
        assert same(Ja[:, 0], r.J[:, c]) and same(ca[:, 0], r.c[:, c]) and same(Xa[:, 0], r.X[:, c]), c
    Jh, ch, dh, Xh = r.host
    assert same(Jh, r.J) and same(ch, r.c) and same(dh, r.d) and same(Xh, r.X)


@pytest.mark.parametrize("name", sm.ORACLE_CASES)
def test_evaluate_against_the_oracle(name):
    """the oracle's own states scored in the given form: its c_max within bound 4, its cost within bound 3 where it finds the
    candidate feasible, the defect of its states within bound 2"""
    r = scored(name)
    Xo, Jo, co = r.orc
    J, c, d = r.on_orc
    _, cb = ER.violation(r.cs, Xo, r.U)
    _, Jb = ER.cost(r.cs, Xo, r.U)
    print(name, "oracle: dc / bound", ratio(np.abs(c - co), cb), "infeasible", int((co > 0).sum()), "of", co.size)
    assert (np.abs(c - co) <= cb).all() and (co > 1e-3).any()
    feas = co == 0.0
    assert (np.abs(J - Jo)[feas] <= Jb[feas]).all()
    assert (d <= ER.defect(r.cs, Xo, r.U)[1]).all()


# ---------------------------------------------------------------------------------------------- evaluate_grad
@pytest.mark.parametrize("name", sm.CASES)
def test_evaluate_grad_within_bounds_5_to_7(name):
    """J and X are evaluate's bytes; P within bound 5, gU and gx0 within twice bound 6 of the yardstick on the device's own Xout at
    rho = 10; the rho = 0 branch: the gradient of J alone, P still there"""
    r = scored(name)
    for rho in (10.0, 0.0):
        g = r.g[rho]
        assert same(g.X, r.X) and same(g.J, r.J), rho
        y = GR.merit_grad(r.cs, g.X, r.U, rho)
        assert (y.margin >= 1e6).all()
        print(name, "evaluate_grad rho", rho, "dP / bound", ratio(np.abs(g.P - y.P), y.Pb), "dgU / bound", ratio(np.abs(g.gU - y.gU), 2 * y.gUb),
              "dgx0 / bound", ratio(np.abs(g.gx0 - y.gx0), 2 * y.gx0b))
        assert np.isfinite(g.P).all() and np.isfinite(g.gU).all() and np.isfinite(g.gx0).all()
        assert (np.abs(g.P - y.P) <= y.Pb).all()
        assert (np.abs(g.gU - y.gU) <= 2 * y.gUb).all()
        assert (np.abs(g.gx0 - y.gx0) <= 2 * y.gx0b).all()
        assert (y.gUb <= 1e-9 * np.abs(y.gU).max()).all()                 # (bounds of rounding size: a wrong term cannot hide)
    assert same(r.g[0.0].P, r.g[10.0].P) and (r.g[10.0].P[:, 1] > 0).all() and not same(r.g[0.0].gU, r.g[10.0].gU)
    if name == "wide-rows64(20,5)":         # guard (d) on the device's states: row 63 alone moves P by more than the bound just held
        cs, last = r.cs, r.cs.cons[-1]
        b2 = last.b.copy()
        b2[..., -1] += 1e-3
        y, y2 = GR.merit_grad(cs, r.X, r.U, 10.0), GR.merit_grad(cs, r.X, r.U, 10.0, cons=cs.cons[:-1] + [ER.Con("soc", last.k0, last.k1, A=last.A, b=b2)])
        assert (np.abs(y.P - y2.P) > y.Pb).any(axis=1).all()


@pytest.mark.parametrize("name", sm.CASES)
def test_evaluate_grad_central_difference(name):
    """the device's own J + 10 P at U +- h D against the device's <gU, D>, the step chosen from the yardstick's margins so that no row
    changes side: per point bounds 3 + 5 of M, bound 7 for the rounded states and one rounding of J + rho P, over 2h; twice bound
    6 (with 7) times |D|; bound 8 for cone values on the boundary branch (test_evaluate_grad_gpu's check)"""
    r = scored(name)
    g, h, full = r.fdg, r.h, r.g[10.0]
    assert (h > 0).all() and np.isfinite(h).all()
    M, err = [], 0.0
    for Up, p in r.pts:
        gp = GR.merit_grad(r.cs, p.X, Up, 10.0)
        assert (gp.margin >= 1e6).all()
        Mp = p.J + 10.0 * p.P
        err = err + GR.merit(r.cs, p.X, Up, 10.0)[1] + (np.abs(gp.Lx) * GR.rollout_error(r.cs, p.X, Up)).sum(axis=(2, 3)) + 2 * U_ * np.abs(Mp)
        M.append(Mp)
    fd = (M[0] - M[1]) / (2 * h)
    got, gb = (full.gU * r.D).sum(axis=(2, 3)), 2 * (g.gUb * np.abs(r.D)).sum(axis=(2, 3))
    tol = err / (2 * h) + gb + GR.fd_truncation(g, 10.0, h)
    print(name, "central difference: h", h.min(), h.max(), "|fd - <g, D>| / tol", ratio(np.abs(fd - got), tol), "tol / |<g, D>|", (tol / np.abs(got)).max())
    assert (np.abs(fd - got) <= tol).all()


# ---------------------------------------------------------------------------------------------- evaluate_al
@pytest.mark.parametrize("name", sm.CASES)
def test_evaluate_al_with_zero_duals_is_the_merit_at_rho_one(name):
    """zero duals and penalty 1 (a handle that has not solved): every output within its bound of the yardstick, and LA, gU, gx0
    agree with evaluate_grad's J + P, gU, gx0 at rho = 1 within the two yardsticks' bounds (test_evaluate_al_gpu's relation)"""
    r = scored(name)
    cs, a, e = r.cs, r.al0, r.g[1.0]
    assert same(a.Xout, r.X) and same(a.J, r.J)
    y = AR.al(cs, a.Xout, r.U, AR.zero_duals(cs), np.ones(cs.B))
    g = GR.merit_grad(cs, a.Xout, r.U, 1.0)
    print(name, "evaluate_al, zero duals: LARGEST error / bound", TA.check(name, cs, a, y, "zero duals"))
    assert (np.abs(a.LA - (e.J + e.P)) <= y.LAb + y.Jb + g.Pb + 2 * U_ * np.abs(a.LA)).all()
    assert (np.abs(a.gU - e.gU) <= 2 * y.gUb + 2 * g.gUb).all()
    assert (np.abs(a.gx0 - e.gx0) <= 2 * y.gx0b + 2 * g.gx0b).all()


@pytest.mark.parametrize("name", sm.SOLVED_CASES)
def test_evaluate_al_within_bounds_A_to_F(name):
    """under the duals drawn from the short solve's (evaluate_al_ref.draw_duals): Xout and J are evaluate's bytes, every output of
    evaluate_al_ref.OUTS within its bound of the yardstick on the device's own Xout; the inputs reach every branch; the short solve
    ended at its three outer iterations below the penalty cap"""
    r = solved(name)
    cs = r.cs
    assert same(r.al.Xout, r.ev[3]) and same(r.al.J, r.ev[0]) and same(r.ev[3], scored(name).X) and same(r.ev[0], scored(name).J)
    y = AR.al(cs, r.al.Xout, r.U, r.lam, r.mu)
    print(name, "mu", r.mu, "status", r.al_status, "branch counts", y.counts)
    assert (r.mu < sm.PENALTY_MAX).all() and (r.al_status == 3).all()
    assert AR.reaches_every_branch(cs, y.counts), y.counts
    for kind in {("eq" if c.eq else c.kind) for c in cs.cons}:         # guard (h): a nonzero dual of every kind in every instance
        has = np.zeros(cs.B, dtype=bool)
        for c, l in zip(cs.cons, r.lam0):
            if ("eq" if c.eq else c.kind) == kind:
                has |= (l.reshape(cs.B, -1) != 0).any(axis=1)
        assert has.all(), kind
    print(name, "evaluate_al: LARGEST error / bound", TA.check(name, cs, r.al, y, "candidates"))
    yk = AR.al(cs, r.al.Xout, r.U, r.lam, r.mu, direction=(GR.tangent(cs, scored(name).D, None), scored(name).D))
    assert (yk.hmax > 0).all()                                            # guard (f): the kink list of (G) is clear of every candidate


# ---------------------------------------------------------------------------------------------- warm_start
@pytest.mark.parametrize("name", sm.CASES)
def test_warm_start(name):
    """include_current both ways: J and c_max are evaluate's bytes for the same candidates (the incumbent's: evaluate on the held
    controls); chosen is the rule of warm_start_ref on those bytes; the installed plane is the rollout kernel's states and the
    controls of the winner"""
    r = scored(name)
    cs, nc = r.cs, r.U.shape[1]
    for inc, q in r.ws.items():
        assert q.J.shape == (cs.B, nc + inc) and same(q.J[:, :nc], r.J) and same(q.c[:, :nc], r.c), inc
        if inc:
            assert same(q.J[:, nc], q.Ji[:, 0]) and same(q.c[:, nc], q.ci[:, 0])
        assert q.chosen.dtype == np.int32 and list(q.chosen) == list(WR.select(q.J, q.c, RHO_WS, inc)), inc
        print(name, "include_current", inc, "chosen", list(q.chosen))
        assert (q.chosen >= 0).all()
        for b, w in enumerate(q.chosen):
            assert same(q.plane[0][b], r.X[b, w] if w < nc else q.Xi[b, 0]), (inc, b)
            assert same(q.plane[1][b], r.U[b, w] if w < nc else cs.Uref[b]), (inc, b)


# ---------------------------------------------------------------------------------------------- simulate_policy
@pytest.mark.parametrize("name", sm.SOLVED_CASES)
def test_simulate_policy(name):
    """nsamp = 3 under the byte equalities of test_simulate_gpu: controls are eval_policy's; without disturbance the states are
    evaluate's rollout of Uout; J and c_max are its given form; dx_max is one subtraction; the trajectory the handle holds is
    unchanged.  The solve that provides the gains ended with status 1 below the penalty cap (guard (h))"""
    r = solved(name)
    cs = r.cs
    print(name, "gains solve: status", r.status, "iterations", r.iterations, "penalty", r.pen)
    assert (r.status == 1).all() and (r.pen < sm.PENALTY_MAX).all()
    for clamp, q in r.sim.items():
        assert same(q.full.U, q.pol), clamp
        assert q.full.fb.dtype == np.int32 and (q.full.fb == 1).all() and np.isfinite(q.full.X).all() and np.isfinite(q.full.U).all()
        assert same(q.now.X, q.roll_now) and same(q.now.X[:, :, 0], r.x0) and not same(q.now.X, q.full.X), clamp
        assert same(q.full.J, q.given[0]) and same(q.full.c, q.given[1]), clamp
        assert same(q.now.J, q.given_now[0]) and same(q.now.c, q.given_now[1]), clamp
        for run in (q.full, q.now):
            assert same(run.dx, np.abs(run.X - r.Xbar[:, None]).max(axis=(2, 3))), clamp
        Jn, Jb = ER.cost(cs, q.full.X, q.full.U)
        cn, cb = ER.violation(cs, q.full.X, q.full.U)
        print(name, "simulate_policy clamp", clamp, "dJ / bound", ratio(np.abs(q.full.J - Jn), Jb), "dc / bound", ratio(np.abs(q.full.c - cn), cb))
        assert (np.abs(q.full.J - Jn) <= Jb).all() and (np.abs(q.full.c - cn) <= cb).all()
    box = cs.cons[0]
    k1 = min(box.k1, cs.N - 2)
    lo, hi = box.zmin[:, None, None, cs.n:], box.zmax[:, None, None, cs.n:]
    u0, u1 = r.sim[0].full.U, r.sim[1].full.U
    assert (u1[:, :, box.k0:k1 + 1] >= lo).all() and (u1[:, :, box.k0:k1 + 1] <= hi).all() and (u0 != u1).any()
    assert same(r.after[0], r.Xbar) and same(r.after[1], r.Ubar)


# ---------------------------------------------------------------------------------------------- split handles
def five(sv, cs, U, x0, w, order):
    """the five calls on one handle in the given order: {call: outputs as a tuple of arrays}"""
    out = {}
    for call in order:
        if call == "evaluate":
            e = TE.ev(sv, U, Xout=True)
            out[call] = e + TE.ev(sv, U, X=e[3])
        elif call == "grad":
            g = TG.eg(sv, U, rho=10.0)
            out[call] = (g.J, g.P, g.gU, g.gx0, g.X)
        elif call == "al":
            a = TA.al(sv, U)
            out[call] = tuple(getattr(a, k) for k in TA.FIELDS)
        elif call == "warm":
            ch, J, c = TW.ws(sv, U, RHO_WS, inc=False)
            out[call] = (ch, J, c) + TW.plane(sv)
        else:
            s = TM.sim(sv, x0, w, clamp=1)
            out[call] = (s.J, s.c, s.dx, s.fb, s.X, s.U)
    return out


@pytest.mark.parametrize("name", sm.SPLIT)
def test_split_handle_through_all_five_calls_interleaved(name):
    """One solved handle, a warm start first (so that every round begins at the plane the warm start installs), then the five calls
    in one order and again in another: evaluate, warm_start and simulate_policy ask for the plain slice (65 536 B at (32, 32)),
    evaluate_grad and evaluate_al for the padded one ((32, 32): none, 0 B; (32, 30): 65 472 B).  No launch is refused, the
    repeats are byte-equal to the first round, and evaluate's bytes are those of the handle that never solved: one kernel's LDS
    request does not depend on what ran before"""
    t = sm.TABLE[name]
    assert (sm.eval_lds(t["n"], t["m"], False), sm.eval_grad_lds(t["n"], t["m"], False)) == {"wide(32,32)": (65536, 0), "wide(32,30)": (63488, 65472)}[name]
    cs, _, _ = sm.build(name)
    U = sm.candidates(name)
    sv = solver(name, sm.sim_opts(name))
    try:
        altro.solve(sv)
        assert (altro.stats(sv).status == 1).all()
        x0, w = TM.inputs(TW.plane(sv)[0], 71)
        TW.ws(sv, U, RHO_WS, inc=False)
        first = five(sv, cs, U, x0, w, ("evaluate", "grad", "sim", "al", "warm"))
        again = five(sv, cs, U, x0, w, ("warm", "al", "evaluate", "sim", "grad"))
        assert altro.dev_refusals(sv) == 0
    finally:
        sv.close()
    for call in first:
        assert len(first[call]) == len(again[call])
        for i, (a, b) in enumerate(zip(first[call], again[call])):
            assert a.dtype == b.dtype and same(a, b), (call, i)
            assert np.isfinite(a).all(), (call, i)
    r = scored(name)
    J, c, d, X, Jg, cg, dg = first["evaluate"]
    assert same(J, r.J) and same(c, r.c) and same(X, r.X) and same(Jg, r.Jg) and same(dg, r.dg)
    assert same(first["grad"][1], r.g[10.0].P) and same(first["grad"][2], r.g[10.0].gU)
    assert (first["sim"][3] == 1).all()
