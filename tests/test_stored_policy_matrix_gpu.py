"""The table of tests/stored_policy_matrix.py on the device: every call that reads what a solve leaves behind, on the
one-wave-per-instance backend, at a padded state of 48, at mp > np, and just under and well over the 64 KB of LDS a kernel gets
unasked -- against the yardsticks of the calls' own test files (whose helpers are imported, not restated) under their rule:

  err = max |out - ref| / max |ref| per instance against the long-double yardstick must not exceed
  16 x max(err of the float64 yardstick against the same ref, 2^-52);

the bound comes from the two numpy runs, nothing of the device enters it, and err / bound is printed for every array.  simulate_policy
and eval_policy are held to the byte equalities of tests/test_simulate_gpu.py and to the rounding bound of tests/test_policy_gpu.py.

The guards of tests/test_stored_policy_matrix.py (on the oracle) are checked again on what the device solved: a case that
contradicts one fails here.

Two handles above 64 KB, interleaved (the last two tests): the dynamic-LDS allowance of a kernel is a property of the kernel, for
the whole process; a handle that asks for less than another handle's kernel launch needs must not leave the other without it."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

import solution_data_ref as DR
import stored_policy_matrix as sp
import test_cost_to_go_gpu as TG
import test_covariance_gpu as TC
import test_policy_gpu as TP
import test_simulate_gpu as TM
import test_solution_data_gpu as TD
import test_solution_sens_gpu as TS
import wide_matrix as wm
from test_warm_start_gpu import H, T, dev, everything, plane, same

pytestmark = pytest.mark.gpu
UNSUP = altro._lib.ERR_UNSUPPORTED
LD = np.longdouble
S = TM.S
ALL_RUNS = sp.RUNS + [q for q in sp.BOX_RUNS if q not in sp.RUNS]
ALL_IDS = [s + ("-pi" if pi else "-shared") for s, pi in ALL_RUNS]
DATA_RUNS = [(s, pi) for s, pi in sp.BOX_RUNS if sp.shape(s)[1] <= 16]       # solution_vjp_data keeps factors of Quu: m <= 16
DATA_IDS = [s + ("-pi" if pi else "-shared") for s, pi in DATA_RUNS]


@functools.lru_cache(maxsize=None)
def ran(name, pi):
    """every device call a case's tests look at, made once on one solved handle"""
    cs0, kw, con, _ = sp.build(name, pi)
    sv, cs = TC.make_solver(name, pi, cs0, kw)
    r = NS(cs=cs, kw=kw, pi=pi, con=con, box_only=len(cs.cons) == 1, nofac=cs.m > 16)
    try:
        st = altro.stats(sv)
        r.status, r.iterations = st.status.copy(), st.iterations.copy()
        r.before = everything(sv, cs.x0, len(cs.cons))
        r.Xbar, r.Ubar = r.X, r.U = plane(sv)
        r.Kraw = r.K = altro.gains(sv)[0]
        r.valid = TS.policy_fb(sv, r.Xbar[:, 0])
        r.duals, r.mu = altro.get_duals(sv, 0), altro.penalty(sv)
        r.lin_duals = altro.get_duals(sv, con) if con is not None else None
        r.g_first = altro.gain_active_set(sv, "numpy") if r.box_only else None      # (before any other call: the stored set is part of the handle)
        # propagate_covariance
        r.S0, r.W = TC.moments(cs, pi, 51)
        r.cov, r.cov_host = TC.cov(sv, cs, r.S0, r.W, con, TC.KAPPA), TC.cov(sv, cs, r.S0, r.W, con, TC.KAPPA, host=True)
        # cost_to_go
        r.m0, r.m0_host = TG.ctg(sv, 0), TG.ctg(sv, 0, host=True)
        if r.box_only:
            r.g = altro.gain_active_set(sv, "numpy")
            r.m1, r.m1_host = TG.ctg(sv, 1), TG.ctg(sv, 1, host=True)
        # solution_vjp / solution_jvp
        r.sd = sd = TS.seeds(cs, 61)
        if r.nofac:
            r.F = None
            with pytest.raises(altro.AltroError) as e:
                api.get_gain_factors_dev(sv)
            r.fac_code = e.value.code
            r.sens = dict(vjp=TS.call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), ("gx0",)), jvp=TS.call(sv, "jvp", dict(vx0=sd.vx0), TS.JVP_OUT))
            r.sens_host = dict(vjp=TS.call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), ("gx0",), host=True),
                               jvp=TS.call(sv, "jvp", dict(vx0=sd.vx0), TS.JVP_OUT, host=True))
            r.refused = []
            for op, ins, names in (("vjp", dict(gX=sd.gX, gU=sd.gU), TS.VJP_OUT), ("vjp", dict(gX=sd.gX), ("gXref",)), ("vjp", dict(gU=sd.gU), ("gUref",)),
                                   ("jvp", dict(vx0=sd.vx0, vXref=sd.vXref), TS.JVP_OUT), ("jvp", dict(vUref=sd.vUref), ("dU",))):
                for host in (False, True):
                    with pytest.raises(altro.AltroError) as e:
                        TS.call(sv, op, ins, names, host=host)
                    r.refused.append(e.value.code)
        else:
            r.F = H(api.get_gain_factors_dev(sv))
            full = dict(vx0=sd.vx0, vXref=sd.vXref, vUref=sd.vUref)
            r.sens = dict(vjp=TS.call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), TS.VJP_OUT), jvp=TS.call(sv, "jvp", full, TS.JVP_OUT),
                          vjp_gx=TS.call(sv, "vjp", dict(gX=sd.gX), TS.VJP_OUT), jvp_u=TS.call(sv, "jvp", dict(vUref=sd.vUref), TS.JVP_OUT))
            r.sens_host = dict(vjp=TS.call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), TS.VJP_OUT, host=True), jvp=TS.call(sv, "jvp", full, TS.JVP_OUT, host=True))
        r.jvp_e = TS.call(sv, "jvp", dict(vx0=np.ascontiguousarray(np.broadcast_to(np.eye(cs.n), (cs.B, cs.n, cs.n)))), ("dU",), ns=cs.n)
        # solution_vjp_data and the getter
        if r.box_only and not r.nofac:
            r.g_dev = TD.getter(sv)
            r.data = {pk: TD.call(sv, sd.gX, sd.gU, per_knot=pk) for pk in (False, True)}
            r.data_host = {pk: TD.call(sv, sd.gX, sd.gU, per_knot=pk, host=True) for pk in (False, True)}
        # simulate_policy, nsamp = 3, and what its bytes are held to; eval_policy at knot 0
        r.x0, r.w = TM.inputs(r.Xbar, 71)
        r.sim = {}
        for clamp in (0, 1):
            q = NS(full=TM.sim(sv, r.x0, r.w, clamp=clamp), now=TM.sim(sv, r.x0, None, clamp=clamp), host=TM.sim(sv, r.x0, r.w, clamp=clamp, host=True))
            q.pol = np.stack([np.stack([TM.policy(sv, q.full.X[:, s, k], k, clamp) for k in range(cs.N - 1)], axis=1) for s in range(S)], axis=1)
            q.roll_now = np.stack([TM.rollout(sv, np.ascontiguousarray(q.now.U[:, s]), r.x0[:, s]) for s in range(S)], axis=1)
            q.given = TM.given(sv, q.full.X, q.full.U)
            r.sim[clamp] = q
        x = r.Xbar[:, 0]
        r.xp = x + 1e-2 * (1.0 + np.abs(x)) * np.random.default_rng(7).standard_normal(x.shape)
        r.pol = {clamp: TP.policy(sv, r.xp, None, clamp) for clamp in (False, True)}
        r.pol_knot0 = TP.policy(sv, r.xp, np.zeros(cs.B, dtype=np.int32), False)
        r.pol_fixed = TP.policy(sv, x, None, False)
        r.pol_host = {}
        for clamp in (False, True):
            fbh = np.full(cs.B, -9, dtype=np.int32)
            r.pol_host[clamp] = (altro.eval_policy(sv, r.xp, None, clamp=clamp, fb=fbh), fbh)
        r.after = everything(sv, cs.x0, len(cs.cons))
        r.g_last = altro.gain_active_set(sv, "numpy") if r.box_only else None
    finally:
        sv.close()
    return r


@pytest.mark.parametrize("name,pi", ALL_RUNS, ids=ALL_IDS)
def test_the_device_solve_meets_the_guards_of_the_table(name, pi):
    """what tests/test_stored_policy_matrix.py holds on the oracle, on the handle the calls read: status 1 in every instance, the
    penalty below its cap, a control on its bound with a positive dual, a nonzero LINEAR dual, valid gains everywhere (the
    iteration counts of both are printed)"""
    r = ran(name, pi)
    cs, g = r.cs, sp.guard(name, pi)
    n = cs.n
    print(name, "status", r.status, "iterations", r.iterations, "oracle", g["iterations"], "penalty", r.mu)
    assert (r.status == 1).all() and (g["status"] == 1).all()
    assert (r.mu < wm.PENALTY_MAX).all() and (r.valid == 1).all()
    box = cs.cons[0]
    lhi, llo = DR.stack_duals(cs, r.duals)
    hi, lo = box.zmax[:, None, n:], box.zmin[:, None, n:]
    on = ((r.Ubar >= hi - 1e-6 * np.abs(hi)) & (lhi[:, :-1, n:] > 0)) | ((r.Ubar <= lo + 1e-6 * np.abs(lo)) & (llo[:, :-1, n:] > 0))
    assert on.reshape(cs.B, -1).any(axis=1).all(), "an instance without a control on its bound"
    if r.con is not None:
        assert (r.lin_duals.reshape(cs.B, -1) != 0).any(axis=1).all(), "an instance with a zero dual block on the LINEAR rows"
    base = name[:-len(sp.BOXONLY)] if name.endswith(sp.BOXONLY) else name
    if sp.TUNE[base]["xb"] is not None:
        assert (lhi[..., :n] > 0).any() or (llo[..., :n] > 0).any(), "no state side with a positive dual"


@pytest.mark.parametrize("name,pi", sp.RUNS, ids=sp.IDS)
def test_covariance(name, pi):
    """sx, su, dJ, Sout, the tightened box, and sc on the rows case, within the rule (test_covariance_gpu.check_accuracy)"""
    r = ran(name, pi)
    assert np.finfo(LD).nmant >= 63
    assert same(r.cov.fb, r.valid) and (r.cov.fb == 1).all()
    assert (r.cov.sc is not None) == (r.con is not None) and r.cov.zmin_t is not None and r.cov.Sout is not None
    w = TC.check_accuracy(r.cov, r.cs, r.Kraw * r.cov.fb[:, None, None, None], r.S0, r.W, r.con, TC.KAPPA, name + " covariance")
    print(name, "pi" if pi else "shared", "covariance: largest err / bound", w)
    S0 = np.broadcast_to(r.S0, (r.cs.B, r.cs.n, r.cs.n))
    assert same(r.cov.sx[:, 0], np.sqrt(np.einsum("bii->bi", S0))) and same(r.cov.Sout[:, 0], S0)
    lo, hi = r.cs.cons[0].zmin, r.cs.cons[0].zmax
    assert same(np.isfinite(r.cov.zmin_t), np.isfinite(lo)) and same(np.isfinite(r.cov.zmax_t), np.isfinite(hi))
    assert (r.cov.zmin_t <= r.cov.zmax_t).all() and (r.cov.zmin_t >= lo).all() and (r.cov.zmax_t <= hi).all() and (r.cov.zmin_t > lo).any()


@pytest.mark.parametrize("name,pi", sp.RUNS, ids=sp.IDS)
def test_cost_to_go_mode_0(name, pi):
    """P0, p0, v0, P, p, v of the plain cost within the rule (test_cost_to_go_gpu.check_accuracy)"""
    r = ran(name, pi)
    assert same(r.m0.fb, r.valid)
    y, y64 = TG.yardsticks(r, 0, r.Kraw * r.m0.fb[:, None, None, None])
    w = TG.check_accuracy(r.m0, y, y64, np.ones(r.cs.B, dtype=np.int32), name + " mode 0")
    print(name, "pi" if pi else "shared", "cost-to-go mode 0: largest err / bound", w)
    assert same(r.m0.P0, r.m0.P[:, 0]) and same(r.m0.p0, r.m0.p[:, 0]) and same(r.m0.v0, r.m0.v[:, 0])


@pytest.mark.parametrize("name,pi", sp.BOX_RUNS, ids=sp.BOX_IDS)
def test_cost_to_go_mode_1(name, pi):
    """the guard of test_cost_to_go_gpu (an instance with fb = 1 and a nonzero code, here every instance), then every output of
    the augmented-Lagrangian call within the rule"""
    r = ran(name, pi)
    g = r.g
    assert ((g["fb"] == 1) & (g["codes"].reshape(r.cs.B, -1) != 0).any(axis=1)).all(), "an instance without valid gains or without a side in the set"
    assert same(r.m1.fb, g["fb"])
    y, y64 = TG.yardsticks(r, 1, r.Kraw)
    w = TG.check_accuracy(r.m1, y, y64, g["fb"], name + " mode 1")
    print(name, "pi" if pi else "shared", "cost-to-go mode 1: largest err / bound", w)
    assert same(r.m1.P0, r.m1.P[:, 0]) and same(r.m1.p0, r.m1.p[:, 0]) and same(r.m1.v0, r.m1.v[:, 0])
    assert not same(r.m1.P0, r.m0.P0)


@pytest.mark.parametrize("name,pi", sp.RUNS, ids=sp.IDS)
def test_solution_sensitivity(name, pi):
    """VJP and JVP within the rule (test_solution_sens_gpu.refs / within); m > 16: the x0-only paths, UNSUPPORTED for the rest on both
    forms and for get_gain_factors_dev, as wide(30,25); the JVP of e_j gives column j of K_0 exactly"""
    r = ran(name, pi)
    ref, r64 = TS.refs(r, LD), TS.refs(r, np.float64)
    w = []
    for grp, got in r.sens.items():
        assert got["fb"].dtype == np.int32 and same(got["fb"], r.valid), grp
        for k in got:
            if k != "fb":
                w.append(TS.within(got[k], getattr(ref, grp)[k], getattr(r64, grp)[k], r.valid, "%s %s %s" % (name, grp, k)))
    print(name, "pi" if pi else "shared", "sensitivity: largest err / bound", max(w))
    if r.nofac:
        assert r.fac_code == UNSUP and r.refused == [UNSUP] * 10, (r.fac_code, r.refused)
    assert np.array_equal(r.jvp_e["dU"][:, :, 0, :], np.swapaxes(r.K[:, 0], -1, -2))


@pytest.mark.parametrize("name,pi", DATA_RUNS, ids=DATA_IDS)
def test_solution_data_and_the_getter(name, pi):
    """K and Quu recomputed from the getter's codes and mu_pass equal get_gains and the stored factors, and every output of
    solution_vjp_data, summed and per knot, is within the rule (test_solution_data_gpu.refs / within)"""
    r = ran(name, pi)
    g, cd = r.g, r.g["codes"]
    assert (g["fb"] == 1).all() and same(g["mu_pass"], r.mu) and cd.dtype == np.uint8 and (cd <= 3).all() and (cd[:, -1, r.cs.n:] == 0).all()
    for k in g:
        assert g[k].dtype == r.g_dev[k].dtype and same(g[k], r.g_dev[k]), k
    K, Quu = DR.riccati_codes(r.cs, cd, g["mu_pass"], LD)
    K64, Quu64 = DR.riccati_codes(r.cs, cd, g["mu_pass"], np.float64)
    w = [TD.within(r.K, K, K64, g["fb"], name + " K from codes"), TD.within(DR.quu_of_factors(r.F, np.float64), Quu, Quu64, g["fb"], name + " Quu from codes")]
    for pk, got in r.data.items():
        ref, r64 = TD.refs(r, LD, pk), TD.refs(r, np.float64, pk)
        assert same(got["fb"], g["fb"])
        for k in TD.OUTS:
            w.append(TD.within(got[k], ref[k], r64[k], g["fb"], "%s %s per_knot=%d" % (name, k, pk)))
    print(name, "pi" if pi else "shared", "solution data: largest err / bound", max(w), "sides in the set", int((cd != 0).sum()))


@pytest.mark.parametrize("name,pi", sp.RUNS, ids=sp.IDS)
def test_simulate_policy_and_eval_policy(name, pi):
    """simulate_policy with nsamp = 3 under the byte equalities of test_simulate_gpu (controls: eval_policy_dev; states without w:
    evaluate_dev's rollout form; J, c_max: its given form; dx_max: one subtraction); eval_policy at knot 0 within the rounding
    bound of test_policy_gpu against the host getters, the exact fixed point, knot NULL == knot 0"""
    r = ran(name, pi)
    cs = r.cs
    for clamp, q in r.sim.items():
        assert same(q.full.U, q.pol), clamp
        assert (q.full.fb == 1).all() and np.isfinite(q.full.X).all() and np.isfinite(q.full.U).all()
        assert same(q.now.X, q.roll_now) and same(q.now.X[:, :, 0], r.x0) and not same(q.now.X, q.full.X), clamp
        assert same(q.full.J, q.given[0]) and same(q.full.c, q.given[1]), clamp
        for run in (q.full, q.now):
            assert same(run.dx, np.abs(run.X - r.Xbar[:, None]).max(axis=(2, 3))), clamp
    u0, u1 = r.sim[0].full.U, r.sim[1].full.U
    box = cs.cons[0]
    k1 = min(box.k1, cs.N - 2)
    lo, hi = box.zmin[:, None, None, cs.n:], box.zmax[:, None, None, cs.n:]
    assert (u1[:, :, box.k0:k1 + 1] >= lo).all() and (u1[:, :, box.k0:k1 + 1] <= hi).all() and (u0[:, -1] != u1[:, -1]).any()
    (u, fb), (uk, fbk) = r.pol[False], r.pol_knot0
    U0, K0, dx = r.Ubar[:, 0], r.K[:, 0], r.xp - r.Xbar[:, 0]
    ref = U0 + np.einsum("baj,bj->ba", K0, dx)
    bound = 2 * (cs.n + 2) * 2.0 ** -53 * (np.abs(U0) + np.einsum("baj,bj->ba", np.abs(K0), np.abs(dx)))
    err = np.abs(u - ref)
    print(name, "eval_policy: max err / bound", float((err / bound).max()), "max |K dx|", float(np.abs(ref - U0).max()))
    assert (fb == 1).all() and np.abs(ref - U0).max() > 1e-6 and (err <= bound).all()
    assert same(u, uk) and same(fb, fbk)
    assert same(r.pol_fixed[0], U0) and (r.pol_fixed[1] == 1).all()
    if box.k0 == 0:
        assert same(r.pol[True][0], np.clip(u, box.zmin[:, cs.n:], box.zmax[:, cs.n:]))


@pytest.mark.parametrize("name,pi", ALL_RUNS, ids=ALL_IDS)
def test_host_twins_and_nothing_changes(name, pi):
    """the host twin of every call writes the bytes the `_dev` form writes; states, controls, duals, gains, statistics and counters
    are byte-identical before and after all the calls of the case (the refused ones included)"""
    r = ran(name, pi)
    for k in TC.NAMES + ("fb",):
        a, b = getattr(r.cov_host, k), getattr(r.cov, k)
        assert (a is None) == (b is None) and (a is None or (a.dtype == b.dtype and same(a, b))), k
    for full, host in ((r.m0, r.m0_host),) + (((r.m1, r.m1_host),) if r.box_only else ()):
        for k in TG.NAMES + ("fb",):
            a, b = getattr(host, k), getattr(full, k)
            assert a.dtype == b.dtype and same(a, b), k
    for grp, host in r.sens_host.items():
        assert set(host) == set(r.sens[grp])
        for k in host:
            assert host[k].dtype == r.sens[grp][k].dtype and same(host[k], r.sens[grp][k]), (grp, k)
    if r.box_only and not r.nofac:
        for pk in (False, True):
            for k in r.data[pk]:
                assert same(r.data[pk][k], r.data_host[pk][k]), (pk, k)
    for clamp, q in r.sim.items():
        for k in ("J", "c", "dx", "fb", "X", "U"):
            a, b = getattr(q.host, k), getattr(q.full, k)
            assert a.dtype == b.dtype and same(a, b), (clamp, k)
    for clamp in (False, True):
        assert same(r.pol_host[clamp][0], r.pol[clamp][0]) and same(r.pol_host[clamp][1], r.pol[clamp][1]), clamp
    for k in r.before:
        assert np.array_equal(r.before[k], r.after[k], equal_nan=True), k
    if r.box_only:      # the stored active set, which no other getter shows: before the first call, after two, after all
        for k in r.g:
            assert same(r.g_first[k], r.g[k]) and same(r.g_last[k], r.g[k]), k


# ---------------------------------------------------------------------------------------------- two handles above 64 KB
BIG, SECOND, UNDER = "wide(64,16)", "wide(48,32)", "wide(40,6)"


@pytest.fixture(scope="module")
def alive():
    """solved handles that stay alive side by side: name -> NS(sv, cs, con, ...), created on first use, closed at the end"""
    made = {}

    def get(name):
        if name not in made:
            cs0, kw, con, _ = (TC.build if name == BIG else sp.build)(name, True)
            sv, cs = TC.make_solver(name, True, cs0, kw)
            Xbar, Ubar = plane(sv)
            S0, W = TC.moments(cs, True, 51)
            made[name] = NS(sv=sv, cs=cs, con=con, Xbar=Xbar, Ubar=Ubar, Kraw=altro.gains(sv)[0], S0=S0, W=W)
        return made[name]
    yield get
    for h in made.values():
        h.sv.close()


def interleave(one, other, call, names, what):
    """`one`, `other`, `one` again: the second outputs of `one` equal its first byte for byte.  Returns (first of one, of other)"""
    a1, b, a2 = call(one), call(other), call(one)
    for k in names + ("fb",):
        x, y = getattr(a1, k), getattr(a2, k)
        assert (x is None) == (y is None) and (x is None or same(x, y)), (what, k)
    return a1, b


def test_two_live_handles_above_64_kb_covariance(alive):
    """k_cov_wide: (64, 16) needs 122 880 B of dynamic LDS, (48, 32) 92 160 B.  A, B, A and B, A, B on two live handles: no
    launch is refused, the repeated call writes the same bytes, and both handles' outputs are within the rule"""
    assert sp.LDS_UNASKED < sp.LDS[48, 32][0] < sp.LDS[64, 16][0]
    A, Bh = alive(BIG), alive(SECOND)
    call = lambda h: TC.cov(h.sv, h.cs, h.S0, h.W, h.con, TC.KAPPA)
    a, b = interleave(A, Bh, call, TC.NAMES, "A, B, A")
    b2, a2 = interleave(Bh, A, call, TC.NAMES, "B, A, B")
    for h, got, again, what in ((A, a, a2, BIG), (Bh, b, b2, SECOND)):
        for k in TC.NAMES + ("fb",):
            assert getattr(got, k) is None or same(getattr(got, k), getattr(again, k)), (what, k)
        w = TC.check_accuracy(got, h.cs, h.Kraw * got.fb[:, None, None, None], h.S0, h.W, h.con, TC.KAPPA, what + " interleaved covariance")
        print(what, "interleaved covariance: largest err / bound", w)


@pytest.mark.parametrize("other", [SECOND, UNDER])
def test_two_live_handles_above_64_kb_cost_to_go(alive, other):
    """k_ctg_wide: (64, 16) needs 115 200 B, (48, 32) 80 256 B, and (40, 6), 61 824 B, stays inside what a kernel gets unasked.
    A, B, A and B, A, B on two live handles: no launch is refused, the repeated call writes the same bytes, and both handles'
    outputs are within the rule"""
    assert sp.LDS[40, 6][1] < sp.LDS_UNASKED < sp.LDS[48, 32][1] < sp.LDS[64, 16][1]
    A, Bh = alive(BIG), alive(other)
    call = lambda h: TG.ctg(h.sv, 0)
    a, b = interleave(A, Bh, call, TG.NAMES, "A, B, A")
    b2, a2 = interleave(Bh, A, call, TG.NAMES, "B, A, B")
    for h, got, again, what in ((A, a, a2, BIG), (Bh, b, b2, other)):
        for k in TG.NAMES + ("fb",):
            assert same(getattr(got, k), getattr(again, k)), (what, k)
        y, y64 = TG.yardsticks(h, 0, h.Kraw * got.fb[:, None, None, None])
        w = TG.check_accuracy(got, y, y64, np.ones(h.cs.B, dtype=np.int32), what + " interleaved cost-to-go")
        print(what, "interleaved cost-to-go: largest err / bound", w)
