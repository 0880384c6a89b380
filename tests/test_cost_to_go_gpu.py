"""The quadratic cost-to-go of the stored policy (altro_batch_cost_to_go_dev / altro_batch_cost_to_go) on both
backends, against tests/cost_to_go_ref.py run in np.longdouble from the device's own gains, trajectory, active set, duals and
penalty.

Shapes: the eight cases and solved handles of tests/test_covariance_gpu.py (build, make_solver; N = 5 .. 8, batch 9 / 5 / 3), each
"shared" and "pi"; box-only copies of its wide-ltv(12,12) and wide(17,5), whose LINEAR rows make mode 1 unsupported there; and
(12, 4) at N = 3 and batch 5, the shortest recursion.  Mode 0 runs on all of them, mode 1 on the box-only ones.
The horizon axis of the 16-lane backend: the stored-set cases of tests/lane16_horizons.py, (12, 4) and (6, 6) at N = 17, 33 and
128, batch 2, "pi" (k_ctg16 reads the lane's two bits a knot as ASet word k >> 4, and at N <= 16 word 0 is the only one there is),
both modes, guarded by sides in the set at knots >= 16 and, at N = 128, >= 112; and (12, 4) at N = 130, where mode 1 is refused
and mode 0 is held to the rule.
The one-wave-per-instance backend at a padded state of 48 ((40, 6), (48, 13), (48, 32): the three-tile strip of gemm_rows under
k_ctg_wide's leading dimensions, just under and over 64 KB of LDS) and at m > n (12, 20) lives in tests/stored_policy_matrix.py
and tests/test_stored_policy_matrix_gpu.py, which import the checks of this file.

The accuracy bound of an output array, per instance: err = max |out - ref| / max |ref| against the long-double yardstick must
not exceed 16 x max(err of the float64 yardstick against the same ref, 2^-52).  The bound is computed here from the two numpy
runs; nothing of the device enters it.  A cross-check between device calls is held to the sum of the bounds of the arrays
involved, each carried through the identity to first and second order (|a'b - ref| <= beta_a max|a| |b|_1 + beta_b max|b| |a|_1 +
beta_a beta_b max|a| max|b| len).

Guard of mode 1: on every mode-1 case at least one instance has fb = 1 and a nonzero code in altro_batch_get_gain_active_set
(checked on the CPU oracle beforehand: every instance of every case here ends with a control at its bound and a positive dual,
so no case needed a tighter bound).

Both meanings of fb: a setter that drops the gains (open loop in mode 0, NaN rows in mode 1), and valid gains beside a held
penalty other than that of the stored pass (NaN rows in mode 1 only), reached by a second solve that the state limit ends before
its first backward pass (test_a_moved_penalty_gives_nan_rows_in_mode_1_only)."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

import cost_to_go_ref as CT
import covariance_ref as CR
import evaluate_ref as ER
import lane16_horizons as lh
import solution_data_ref as SD
import test_covariance_gpu as TC
from test_covariance_gpu import OPTS, make_solver
from test_warm_start_gpu import H, T, assert_twins, dev, everything, plane, same

pytestmark = pytest.mark.gpu
INV, STATE, UNSUP = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_STATE, altro._lib.ERR_UNSUPPORTED
LD = np.longdouble
EPS = 2.0 ** -52
SENT = -12345.5
NAMES = altro._lib.CTG_OUT_FIELDS
LTVBOX, W17BOX, SHORT = "wide-ltv(12,12)-box", "wide(17,5)-box", "16(12,4)N3"
LONG = list(lh.STORED_SET_CASES)       # the stored set beyond ASet word 0: (12, 4) and (6, 6) at N = 17, 33, 128, batch 2, "pi"
MODE1 = ("16-box(12,4)", "16(6,6)", "16(8,4)", "wide(64,16)", "wide(30,25)", LTVBOX, W17BOX, SHORT) + tuple(LONG)
SHAPES = TC.SHAPES + [LTVBOX, W17BOX, SHORT]
RUNS_SHORT = [(s, pi) for s in SHAPES for pi in (False, True)]
IDS_SHORT = [s + ("-pi" if pi else "-shared") for s, pi in RUNS_SHORT]
RUNS = RUNS_SHORT + [(s, True) for s in LONG]
IDS = [s + ("-pi" if pi else "-shared") for s, pi in RUNS]
RUNS1 = [(s, pi) for s, pi in RUNS if s in MODE1]
IDS1 = [s + ("-pi" if pi else "-shared") for s, pi in RUNS1]


def build(name, pi):
    """(Case, to_problem keywords)"""
    if name in (LTVBOX, W17BOX):
        cs, kw, _, _ = TC.build(name[:-len("-box")], pi)
        cs.cons = cs.cons[:1]
        return cs, dict(kw, shared=tuple(s for s in kw["shared"] if s != 1))
    if name in LONG:
        return lh.stored_set_case(name), dict(shared=())
    if name == SHORT:
        ub = 0.5 + np.random.default_rng(32).random((5, 4)) if pi else 0.9
        return ER.add_box(ER.make_case(5, 12, 4, 3, 31, per_instance_cost=pi), ub), dict(shared=() if pi else ("cost", "box"))
    cs, kw, _, _ = TC.build(name, pi)
    return cs, kw


def shapes(sv):
    B, N, n = sv.B, sv.N, sv.n
    return dict(P0=(B, n, n), p0=(B, n), v0=(B,), P=(B, N, n, n), p=(B, N, n), v=(B, N))


def ctg(sv, mode, names=NAMES, host=False):
    """cost_to_go with sentinels in every output asked for: NS of numpy arrays (None where not asked for), fb too"""
    shp = shapes(sv)
    if host:
        out = {k: np.full(shp[k], SENT) for k in names}
        out["fb"] = np.full(sv.B, -77, dtype=np.int32)
        got = altro.cost_to_go(sv, penalty=bool(mode), out=out)
    else:
        out = {k: torch.full(shp[k], SENT, dtype=torch.float64, device=dev()) for k in names}
        out["fb"] = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
        got = altro.cost_to_go(sv, penalty=bool(mode), out=out)
        torch.cuda.synchronize()
        got = {k: H(v) for k, v in got.items()}
    return NS(**{k: got.get(k) for k in NAMES + ("fb",)})


def beta(a64, ref):
    """the relative bound of the rule for one array, per instance"""
    return 16 * np.maximum(CR.rel_err(a64, ref), EPS)


def amax(a):
    return np.abs(np.asarray(a, dtype=np.float64)).reshape(len(a), -1).max(axis=1)


def l1(a):
    return np.abs(np.asarray(a, dtype=np.float64)).reshape(len(a), -1).sum(axis=1)


def check_accuracy(got, y, y64, valid, what):
    """the rule for every array `got` holds (y, y64: the yardstick in long double and in float64); instances with valid == 0 must
    be all NaN.  Returns the largest err / bound."""
    worst = 0.0
    ok = valid != 0
    for k in NAMES:
        g = getattr(got, k)
        if g is None:
            continue
        rf, r6 = (getattr(q, k[0]) for q in (y, y64))
        if k.endswith("0"):
            rf, r6 = rf[:, 0], r6[:, 0]
        assert g.shape == rf.shape and not (g == SENT).any(), (what, k)
        for b in np.nonzero(~ok)[0]:
            assert np.isnan(g[b]).all(), (what, k, b, "an instance that is not valid is all NaN")
        if not ok.any():
            continue
        assert np.isfinite(g[ok]).all(), (what, k)
        err, bound = CR.rel_err(g[ok], rf[ok]), beta(r6[ok], rf[ok])
        ratio = float((err / bound).max())
        print("%-34s %-3s err %.2e  float64 yardstick %.2e  err/bound %.3f" % (what, k, err.max(), (bound / 16).max(), ratio))
        assert (err <= bound).all(), (what, k, err, bound)
        if rf.ndim > 1:      # rows (the last axis: a matrix row of P, a knot of p or v) that are identically zero: exactly +0
            zero = np.abs(rf[ok]).max(axis=-1) == 0
            assert same(g[ok][zero], np.zeros(g[ok][zero].shape)), (what, k, "identically zero rows: exactly +0")
            zrows[0] += int(zero.sum())
        worst = max(worst, ratio)
    return worst


zrows = [0]     # identically zero rows check_accuracy has met (test_identically_zero_rows_are_exactly_plus_zero looks at it)


def yardsticks(r, mode, K):
    kw = dict(mode=1, codes=r.g["codes"], mu_pass=np.where(r.g["fb"] != 0, r.g["mu_pass"], 1.0), duals=r.duals, mu=r.mu) if mode else {}
    return CT.cost_to_go(r.cs, K, r.Xbar, r.Ubar, dtype=LD, **kw), CT.cost_to_go(r.cs, K, r.Xbar, r.Ubar, dtype=np.float64, **kw)


def loop_cost(cs, K, Xbar, Ubar, d, dtype):
    """J of the unclamped closed loop from xbar_0 + d, every operation in `dtype`: (B,)"""
    t = lambda a: np.asarray(a, dtype=dtype)
    A, Bm, f, K, Xb, Ub = t(cs.A), t(cs.Bm), t(cs.f), t(K), t(Xbar), t(Ubar)
    wx, wu = SD.weights(SD.theta_of(cs), cs, dtype)
    x = Xb[:, 0] + t(d)
    J = np.zeros(cs.B, dtype=dtype)
    half = dtype(0.5)
    for k in range(cs.N):
        ex = x - t(cs.Xref)[:, k]
        J = J + half * (wx[:, k] * ex * ex).sum(axis=1)
        if k < cs.N - 1:
            u = Ub[:, k] + np.einsum("baj,bj->ba", K[:, k], x - Xb[:, k])
            eu = u - t(cs.Uref)[:, k]
            J = J + half * (wu * eu * eu).sum(axis=1)
            x = np.einsum("bij,bj->bi", A[:, k], x) + np.einsum("bij,bj->bi", Bm[:, k], u) + f[:, k]
    return J


def tangent(cs, K, d, dtype):
    """(xi (B, N, n), nu (B, N-1, m)) of solution_jvp(vx0 = d): xi_0 = d, nu_k = K_k xi_k, xi_{k+1} = A_k xi_k + B_k nu_k"""
    t = lambda a: np.asarray(a, dtype=dtype)
    A, Bm, K = t(cs.A), t(cs.Bm), t(K)
    xi, nu = np.zeros((cs.B, cs.N, cs.n), dtype=dtype), np.zeros((cs.B, cs.N - 1, cs.m), dtype=dtype)
    xi[:, 0] = t(d)
    for k in range(cs.N - 1):
        nu[:, k] = np.einsum("baj,bj->ba", K[:, k], xi[:, k])
        xi[:, k + 1] = np.einsum("bij,bj->bi", A[:, k], xi[:, k]) + np.einsum("bia,ba->bi", Bm[:, k], nu[:, k])
    return xi, nu


def al_gradient(cs, X, U, duals, mu, dtype):
    """(gx0 (B, n), gU (B, N-1, m)) of evaluate_al at U == NULL on a box-only case: lam_{N-1} = lx, gU_k = lu_k + B_k' lam_{k+1},
    lam_k = lx_k + A_k' lam_{k+1}, gx0 = lam_0"""
    zc = np.zeros((cs.B, cs.N, cs.n + cs.m), dtype=np.uint8)
    _, l, _ = CT.local_terms(cs, X, U, 1, zc, np.ones(cs.B), duals, mu, dtype)
    A, Bm = np.asarray(cs.A, dtype=dtype), np.asarray(cs.Bm, dtype=dtype)
    n = cs.n
    lam = l[:, -1, :n]
    gU = np.zeros((cs.B, cs.N - 1, cs.m), dtype=dtype)
    for k in range(cs.N - 2, -1, -1):
        gU[:, k] = l[:, k, n:] + np.einsum("bia,bi->ba", Bm[:, k], lam)
        lam = l[:, k, :n] + np.einsum("bij,bi->bj", A[:, k], lam)
    return lam, gU


@functools.lru_cache(maxsize=None)
def ran(name, pi):
    """every device call a case's tests look at, made once on one solved handle"""
    cs0, kw = build(name, pi)
    sv, cs = make_solver(name, pi, cs0, kw)
    r = NS(cs=cs, kw=kw, pi=pi, mode1=name in MODE1)
    try:
        r.before = everything(sv, cs.x0, len(cs.cons))
        r.Xbar, r.Ubar = plane(sv)
        r.Kraw = altro.gains(sv)[0]
        fbp = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
        altro.eval_policy(sv, T(r.Xbar[:, 0]), fb=fbp)
        r.fb_policy = H(fbp)
        r.m0, r.m0_host, r.m0_quiet = ctg(sv, 0), ctg(sv, 0, host=True), ctg(sv, 0, NAMES[:3])
        r.d = 0.3 * np.random.default_rng(73).standard_normal((cs.B, cs.n))
        J = torch.full((sv.B, 1), SENT, dtype=torch.float64, device=dev())
        altro.simulate_policy(sv, T((r.Xbar[:, 0] + r.d)[:, None]), None, clamp=False, out=(J, None, None))
        r.S0, r.W = TC.moments(cs, pi, 51)
        cov = altro.propagate_covariance(sv, T(r.S0), T(r.W), out=dict(dJ=torch.full((sv.B,), SENT, dtype=torch.float64, device=dev())))
        torch.cuda.synchronize()
        r.Jsim, r.dJ = H(J)[:, 0], H(cov["dJ"])
        if r.mode1:
            r.g = altro.gain_active_set(sv, "numpy")
            r.duals, r.mu = altro.get_duals(sv, 0), altro.penalty(sv)
            r.m1, r.m1_host, r.m1_quiet = ctg(sv, 1), ctg(sv, 1, host=True), ctg(sv, 1, NAMES[:3])
            jv = altro.solution_jvp(sv, vx0=T(r.d))
            torch.cuda.synchronize()
            r.jvp = {k: H(v) for k, v in jv.items()}
            al = altro.evaluate_al(sv, out=("gx0", "gU"))
            r.gx0, r.gU = np.asarray(al["gx0"]).reshape(cs.B, cs.n), np.asarray(al["gU"]).reshape(cs.B, cs.N - 1, cs.m)
        r.after = everything(sv, cs.x0, len(cs.cons))
        # a setter that drops the stored gains
        prob = ER.to_problem(altro, cs, **kw)
        altro.set_tracking_cost(sv, prob.obj.Q, prob.obj.R, prob.obj.Qf)
        r.open0 = ctg(sv, 0)
        if r.mode1:
            r.g_open = altro.gain_active_set(sv, "numpy")
            r.open1 = ctg(sv, 1)
    finally:
        sv.close()
    return r


def assert_late_words_are_read(name, cs, g):
    """the guard of the long cases, from the getter alone: an instance with fb = 1 holds a nonzero code at a knot >= 16 (ASet word
    1 or later), at N = 128 at a knot >= 112 (the last word); and, over the instances with fb = 1, sides of every kind there
    (lane16_horizons.assert_late_sides).  Mode 1 of an instance with fb = 0 is NaN rows and reads no word at all"""
    N, ok = cs.N, g["fb"] == 1
    assert ok.any(), (name, "fb = 0 in every instance: the penalty held is not that of the stored pass (mu %s, mu_pass %s), mode 1 reads no "
                      "set here; pick another seed for lane16_horizons.STORED_SET_SEED on the oracle" % (g.get("mu"), g["mu_pass"]))
    first = 112 if N == lh.ASET_MAXN else lh.ASET_KNOTS
    late = (g["codes"][:, first:] != 0).reshape(cs.B, -1).any(axis=1)
    assert (ok & late).any(), (name, "no instance with valid gains and a side in the set at a knot >= %d" % first, g["fb"], late)
    lh.assert_late_sides(g["codes"][ok], cs.n, N)


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_mode_0_against_the_long_double_yardstick(name, pi):
    """every output of the plain-cost call within the rule; fb is eval_policy_dev's; P0, p0, v0 are knot 0 of the tracks"""
    r = ran(name, pi)
    assert np.finfo(LD).nmant >= 63
    assert r.m0.fb.dtype == np.int32 and same(r.m0.fb, r.fb_policy) and (r.m0.fb == 1).any(), r.m0.fb
    K = r.Kraw * r.m0.fb[:, None, None, None]       # (an instance without valid gains runs the open loop)
    y, y64 = yardsticks(r, 0, K)
    w = check_accuracy(r.m0, y, y64, np.ones(r.cs.B, dtype=np.int32), name + " mode 0")
    print(name, "pi" if pi else "shared", "mode 0 largest err / bound", w)
    assert same(r.m0.P0, r.m0.P[:, 0]) and same(r.m0.p0, r.m0.p[:, 0]) and same(r.m0.v0, r.m0.v[:, 0])


@pytest.mark.parametrize("name,pi", RUNS1, ids=IDS1)
def test_mode_1_against_the_long_double_yardstick(name, pi):
    """the guard (an instance with fb = 1 and a nonzero code, from the getter alone), then every output of the augmented-Lagrangian
    call within the rule, with the gains, codes, mu_pass, duals and penalty of the existing getters; instances the getter calls
    invalid are NaN here and finite in mode 0"""
    r = ran(name, pi)
    g = r.g
    assert ((g["fb"] == 1) & (g["codes"].reshape(r.cs.B, -1) != 0).any(axis=1)).any(), "no instance with valid gains and a side in the set"
    if name in LONG:
        assert_late_words_are_read(name, r.cs, g)
    assert same(r.m1.fb, g["fb"])
    y, y64 = yardsticks(r, 1, r.Kraw)
    w = check_accuracy(r.m1, y, y64, g["fb"], name + " mode 1")
    print(name, "pi" if pi else "shared", "mode 1 largest err / bound", w)
    assert same(r.m1.P0, r.m1.P[:, 0]) and same(r.m1.p0, r.m1.p[:, 0]) and same(r.m1.v0, r.m1.v[:, 0])
    moved = (g["fb"] == 0) & (r.fb_policy == 1)      # (should a plain solve leave one: the case has a test of its own below)
    for k in NAMES:
        assert np.isnan(getattr(r.m1, k)[moved]).all() and np.isfinite(getattr(r.m0, k)[moved]).all(), k
    assert not same(r.m1.P0, r.m0.P0)                # (a side in the set: the Hessians differ)


@pytest.mark.parametrize("name,pi", RUNS_SHORT, ids=IDS_SHORT)
def test_mode_0_cross_checks_simulation_and_covariance(name, pi):
    """J of simulate_policy_dev (clamp 0, w NULL) from xbar_0 + d, |d| ~ 0.3, equals v_0 + p_0'd + d'P_0 d / 2, and dJ of
    propagate_covariance_dev equals <P_0, Sigma0> / 2 + sum_{k >= 1} <P_k, W> / 2, each within the sum of the bounds of the arrays
    involved"""
    r = ran(name, pi)
    cs, d, m0 = r.cs, r.d, r.m0
    K = r.Kraw * m0.fb[:, None, None, None]
    y, y64 = yardsticks(r, 0, K)
    bP0, bp0, bv0, bP = beta(y64.P[:, 0], y.P[:, 0]), beta(y64.p[:, 0], y.p[:, 0]), beta(y64.v[:, 0], y.v[:, 0]), beta(y64.P, y.P)
    Jl, J64 = loop_cost(cs, K, r.Xbar, r.Ubar, d, LD), loop_cost(cs, K, r.Xbar, r.Ubar, d, np.float64)
    model = CT.quadratic(NS(P=m0.P, p=m0.p, v=m0.v), d, LD)
    bound = beta(J64, Jl) * amax(Jl) + bv0 * amax(y.v[:, 0]) + bp0 * amax(y.p[:, 0]) * l1(d) + 0.5 * bP0 * amax(y.P[:, 0]) * l1(d) ** 2
    gap = np.abs(np.asarray(r.Jsim, dtype=LD) - model).astype(np.float64)
    print(name, "simulation: gap", gap, "bound", bound)
    assert (gap <= bound).all()
    assert (np.abs(r.Jsim - m0.v0) > 1e-3 * m0.v0).all()        # (d moves the cost: the check is not one of v_0 alone)
    full = lambda a: np.broadcast_to(a, (cs.B, cs.n, cs.n))
    cl, c64 = CR.propagate(cs, K, r.S0, r.W, dtype=LD).dJ, CR.propagate(cs, K, r.S0, r.W).dJ
    tr = CT.trace_formula(m0.P, r.S0, r.W, LD)
    bound = beta(c64, cl) * amax(cl) + 0.5 * bP * amax(y.P) * (l1(full(r.S0)) + (cs.N - 1) * l1(full(r.W)))
    gap = np.abs(np.asarray(r.dJ, dtype=LD) - tr).astype(np.float64)
    print(name, "covariance: gap", gap, "bound", bound)
    assert (gap <= bound).all() and (r.dJ > 0).all()


@pytest.mark.parametrize("name,pi", RUNS1, ids=IDS1)
def test_mode_1_cross_checks_the_jvp_and_the_al_gradient(name, pi):
    """with dz = (dX, dU) of solution_jvp_dev(vx0 = d) and hz from the getter's codes and mu_pass: d'P_0 d = sum_k dz_k' hz_k dz_k;
    with (gx0, gU) of evaluate_al_dev at U == NULL: p_0'd = gx0'd + sum_k gU_k'dU_k -- on the instances both calls report valid"""
    r = ran(name, pi)
    cs, d, g = r.cs, r.d, r.g
    ok = (g["fb"] == 1) & (r.jvp["fb"] == 1)
    assert ok.any()
    y, y64 = yardsticks(r, 1, r.Kraw)
    bP0, bp0 = beta(y64.P[:, 0], y.P[:, 0]), beta(y64.p[:, 0], y.p[:, 0])
    (xl, nl), (x64, n64) = tangent(cs, r.Kraw, d, LD), tangent(cs, r.Kraw, d, np.float64)
    bx, bn = beta(x64, xl), beta(n64, nl)
    hx, hu = SD.hz_of(SD.theta_of(cs), cs, g["codes"], np.where(g["fb"] != 0, g["mu_pass"], 1.0), LD)
    dX, dU = np.asarray(r.jvp["dX"], dtype=LD), np.asarray(r.jvp["dU"], dtype=LD)
    lhs = np.einsum("bi,bij,bj->b", np.asarray(d, dtype=LD), np.asarray(r.m1.P0, dtype=LD), np.asarray(d, dtype=LD))
    rhs = (hx * dX * dX).sum(axis=(1, 2)) + (hu * dU * dU).sum(axis=(1, 2))
    sq = lambda b_, a, h: (2 * b_ + b_ * b_) * amax(a) * l1(np.asarray(h * np.abs(a), dtype=np.float64)) + b_ * b_ * amax(a) ** 2 * l1(h)
    bound = bP0 * amax(y.P[:, 0]) * l1(d) ** 2 + sq(bx, xl, hx) + sq(bn, nl, hu)
    gap = np.abs(lhs - rhs).astype(np.float64)
    print(name, "Hessian: gap", gap[ok], "bound", bound[ok])
    assert (gap[ok] <= bound[ok]).all() and (lhs[ok] > 0).all()
    (g0l, gUl), (g064, gU64) = al_gradient(cs, r.Xbar, r.Ubar, r.duals, r.mu, LD), al_gradient(cs, r.Xbar, r.Ubar, r.duals, r.mu, np.float64)
    bg0, bgU = beta(g064, g0l), beta(gU64, gUl)
    lhs = np.einsum("bi,bi->b", np.asarray(r.m1.p0, dtype=LD), np.asarray(d, dtype=LD))
    rhs = np.einsum("bi,bi->b", np.asarray(r.gx0, dtype=LD), np.asarray(d, dtype=LD)) + (np.asarray(r.gU, dtype=LD) * dU).sum(axis=(1, 2))
    bound = (bp0 * amax(y.p[:, 0]) + bg0 * amax(g0l)) * l1(d) + bgU * amax(gUl) * l1(nl) + bn * amax(nl) * l1(gUl) \
        + bgU * bn * amax(gUl) * amax(nl) * (cs.N - 1) * cs.m
    gap = np.abs(lhs - rhs).astype(np.float64)
    print(name, "gradient: gap", gap[ok], "bound", bound[ok])
    assert (gap[ok] <= bound[ok]).all()


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_both_meanings_of_fb(name, pi):
    """after a setter that drops the gains: mode 0 gives fb = 0 and the K = 0 recursion (within the rule), mode 1 fb = 0 and NaN rows"""
    r = ran(name, pi)
    assert (r.open0.fb == 0).all()
    y, y64 = yardsticks(r, 0, np.zeros_like(r.Kraw))
    check_accuracy(r.open0, y, y64, np.ones(r.cs.B, dtype=np.int32), name + " open loop")
    assert not same(r.open0.P0, r.m0.P0)
    if r.mode1:
        assert (r.g_open["fb"] == 0).all() and (r.open1.fb == 0).all()
        for k in NAMES:
            assert np.isnan(getattr(r.open1, k)).all(), k


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_host_twin_quiet_form_and_nothing_changes(name, pi):
    """the host twin writes the bytes the `_dev` form writes; with P, p, v NULL the other outputs are the same bytes; states,
    controls, duals, gains, statistics and counters are byte-identical before and after the calls"""
    r = ran(name, pi)
    for full, host, quiet in ((r.m0, r.m0_host, r.m0_quiet),) + (((r.m1, r.m1_host, r.m1_quiet),) if r.mode1 else ()):
        for k in NAMES + ("fb",):
            a, b, q = getattr(host, k), getattr(full, k), getattr(quiet, k)
            assert a.dtype == b.dtype and same(a, b), k
            assert (q is None) == (k in NAMES[3:]) and (q is None or same(q, b)), k
    for k in r.before:
        assert np.array_equal(r.before[k], r.after[k], equal_nan=True), k


@pytest.mark.parametrize("name,pi", [("16-box(12,4)", True), (W17BOX, True), ("16-soc(6,3)", True)])
def test_instance_alone_on_a_batch_one_handle(name, pi):
    """instance b on a solved batch-1 handle holding its rows of data (same trajectory, same gains: checked first) gets the bytes
    it gets inside the batch"""
    r = ran(name, pi)
    for b in range(r.cs.B):
        sub = ER.sub_case(r.cs, b)
        sv, _ = make_solver(name, pi, sub, {})
        try:
            Xb, Ub = plane(sv)
            assert same(Xb, r.Xbar[b:b + 1]) and same(Ub, r.Ubar[b:b + 1]) and same(altro.gains(sv)[0], r.Kraw[b:b + 1]), ("the solves differ", b)
            a0 = ctg(sv, 0)
            a1 = ctg(sv, 1) if r.mode1 else None
        finally:
            sv.close()
        for a, full in ((a0, r.m0),) + (((a1, r.m1),) if r.mode1 else ()):
            for k in NAMES + ("fb",):
                assert same(getattr(a, k), getattr(full, k)[b:b + 1]), (b, k)


@pytest.mark.parametrize("name,pi", [("16-box(12,4)", True), ("wide(64,16)", False)])
def test_the_following_solve_equals_a_twin(name, pi):
    """the solve that follows is byte-identical to that of a twin handle that never made the call"""
    cs, kw = build(name, pi)
    (sv, _), (tw, _) = make_solver(name, pi, cs, kw), make_solver(name, pi, cs, kw)
    try:
        for mode in (0, 1):
            ctg(sv, mode), ctg(sv, mode, host=True)
        assert_twins(sv, tw, cs.x0, len(cs.cons), "before the next solve")
        x0 = cs.x0 + 0.05
        for s in (sv, tw):
            altro.set_initial_state(s, x0)
            altro.solve(s)
        assert_twins(sv, tw, cs.x0, len(cs.cons), "after the next solve")
    finally:
        sv.close(), tw.close()


@pytest.mark.parametrize("name", ["16-box(12,4)", W17BOX])
def test_nan_stays_in_its_instance(name):
    """a NaN in one instance's reference stays a NaN in that instance's p and v (P does not see the reference) and reaches no other
    instance"""
    cs, kw = build(name, True)
    sv, cs = make_solver(name, True, cs, kw)
    try:
        dp = C.POINTER(C.c_double)
        Xr, Ur = np.ascontiguousarray(cs.Xref), np.ascontiguousarray(cs.Uref)
        assert sv._L.altro_batch_set_reference(sv.h, Xr.ctypes.data_as(dp), Ur.ctypes.data_as(dp)) == 0
        clean = ctg(sv, 0)
        Xn = Xr.copy()
        Xn[1, 2, 3] = np.nan
        assert sv._L.altro_batch_set_reference(sv.h, Xn.ctypes.data_as(dp), Ur.ctypes.data_as(dp)) == 0
        a = ctg(sv, 0)
    finally:
        sv.close()
    keep = np.arange(cs.B) != 1
    for k in NAMES + ("fb",):
        assert same(getattr(a, k)[keep], getattr(clean, k)[keep]), k
    assert same(a.P, clean.P) and np.isfinite(clean.p).all()
    assert np.isnan(a.p[1, :3, :]).any(axis=1).all() and np.isnan(a.p0[1]).any() and np.isnan(a.v[1, :3]).all() and np.isnan(a.v0[1])
    assert np.isfinite(a.p[1, 3:]).all() and np.isfinite(a.v[1, 3:]).all()


@pytest.mark.parametrize("name", ["16-box(12,4)", W17BOX])
def test_a_moved_penalty_gives_nan_rows_in_mode_1_only(name):
    """Valid gains beside a held penalty other than that of the stored pass.  The route: after the solve, an initial state beyond
    max_state_value for instance 1 (altro_batch_set_initial_state drops no gains), then another solve.  Its first open-loop
    rollout ends that instance's solve with the state limit before any backward pass runs, but after reset_penalties has put
    the penalty back to its initial value: the handle then holds the gains and mu_pass of the first solve beside another mu.
    Guarded from the existing getters alone (eval_policy's fb 1, the getter's fb 0, penalty != the earlier mu_pass); then mode 1
    gives fb = 0 and NaN rows for that instance, mode 0 fb = 1 and the outputs of the trajectory held, and every other instance
    both modes, all within the rule"""
    cs, kw = build(name, True)
    sv, cs = make_solver(name, True, cs, kw)
    try:
        g0 = altro.gain_active_set(sv, "numpy")
        x0 = cs.x0.copy()
        x0[1, 0] = 2e8
        altro.set_initial_state(sv, x0)
        altro.solve(sv)
        status = altro.stats(sv).status.copy()
        Xbar, Ubar = plane(sv)
        fbp = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
        altro.eval_policy(sv, T(Xbar[:, 0]), fb=fbp)
        fbp = H(fbp)
        g, mu, duals, Kraw = altro.gain_active_set(sv, "numpy"), altro.penalty(sv), altro.get_duals(sv, 0), altro.gains(sv)[0]
        m0, m1 = ctg(sv, 0), ctg(sv, 1)
    finally:
        sv.close()
    print(name, "status", status, "policy fb", fbp, "getter fb", g["fb"], "penalty", mu, "mu_pass before", g0["mu_pass"])
    assert g0["fb"][1] == 1 and fbp[1] == 1 and g["fb"][1] == 0 and mu[1] != g0["mu_pass"][1], "the route did not leave the state"
    assert np.isfinite(Xbar).all() and np.isfinite(Ubar).all()
    assert same(m1.fb, g["fb"]) and same(m0.fb, fbp)
    for k in NAMES:
        assert np.isnan(getattr(m1, k)[1]).all() and np.isfinite(getattr(m0, k)).all(), k
    r = NS(cs=cs, Xbar=Xbar, Ubar=Ubar, Kraw=Kraw, g=g, duals=duals, mu=mu)
    y, y64 = yardsticks(r, 0, Kraw * m0.fb[:, None, None, None])
    check_accuracy(m0, y, y64, np.ones(cs.B, dtype=np.int32), name + " moved penalty, mode 0")
    y, y64 = yardsticks(r, 1, Kraw)
    check_accuracy(m1, y, y64, g["fb"], name + " moved penalty, mode 1")


@pytest.mark.parametrize("name", ["16(8,4)", W17BOX])
def test_identically_zero_rows_are_exactly_plus_zero(name):
    """a state that carries no weight and feeds nothing (Q_i = Qf_i = 0, column i of A zero): in the open loop row i and column i of
    every P_k are identically zero in the yardstick (the guard) and exactly +0 on the device; the closed loop is held to the same
    per-row check wherever its yardstick, with the device's gains, has such rows"""
    cs, kw = build(name, True)
    i = 2
    cs.A, cs.Q, cs.Qf = cs.A.copy(), cs.Q.copy(), cs.Qf.copy()
    cs.A[:, :, :, i], cs.Q[:, i], cs.Qf[:, i] = 0.0, 0.0, 0.0
    sv, cs = make_solver(name, True, cs, kw)
    try:
        Xbar, Ubar = plane(sv)
        Kraw = altro.gains(sv)[0]
        m0 = ctg(sv, 0)
        prob = ER.to_problem(altro, cs, **kw)
        altro.set_tracking_cost(sv, prob.obj.Q, prob.obj.R, prob.obj.Qf)
        open0 = ctg(sv, 0)
    finally:
        sv.close()
    r = NS(cs=cs, Xbar=Xbar, Ubar=Ubar)
    y, y64 = yardsticks(r, 0, np.zeros_like(Kraw))
    assert (y.P[:, :, i, :] == 0).all() and (y.P[:, :, :, i] == 0).all() and (y.P != 0).any()
    met = zrows[0]
    check_accuracy(open0, y, y64, np.ones(cs.B, dtype=np.int32), name + " zero rows, open loop")
    assert (open0.fb == 0).all() and zrows[0] - met >= cs.B * (cs.N + 1)        # (row i of every P_k and of P0)
    zero = np.zeros((cs.B, cs.N, cs.n))
    assert same(open0.P[:, :, i, :], zero) and same(open0.P[:, :, :, i], zero)
    met = zrows[0]
    y, y64 = yardsticks(r, 0, Kraw * m0.fb[:, None, None, None])
    check_accuracy(m0, y, y64, np.ones(cs.B, dtype=np.int32), name + " zero rows, closed loop")
    print(name, "closed loop: column i of K zero:", bool((Kraw[..., i] == 0).all()), "zero rows met:", zrows[0] - met)


# ---------------------------------------------------------------------------------------------- refusals
def raw(sv, mode, names=NAMES, fb=True, ptr=None):
    """the `_dev` entry point itself on sentinel tensors: (return code, {name: tensor})"""
    shp = shapes(sv)
    o = {k: torch.full(shp[k], SENT, dtype=torch.float64, device=dev()) for k in names}
    f = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
    st = altro._lib.CtgOut(**{k: (ptr or (lambda t: t.data_ptr()))(t) for k, t in o.items()})
    rc = sv._L.altro_batch_cost_to_go_dev(sv.h, mode, C.byref(st), f.data_ptr() if fb else None)
    torch.cuda.synchronize()
    o["fb"] = f
    return rc, o


def untouched(o):
    return all((t == (-77 if k == "fb" else SENT)).all() for k, t in o.items())


@pytest.mark.parametrize("name", ["16-soc(6,3)", "wide(17,5)"])
def test_mode_1_is_refused_where_the_getter_is(name):
    """a handle with a LINEAR or SOC constraint: mode 1 answers UNSUPPORTED on both forms, exactly as the getter, nothing is written
    and the handle stays as it was; mode 0 runs"""
    cs0, kw = build(name, True)
    sv, cs = make_solver(name, True, cs0, kw)
    try:
        before = everything(sv, cs.x0, len(cs.cons))
        assert sv._L.altro_batch_get_gain_active_set_dev(sv.h, None, torch.zeros(sv.B, dtype=torch.float64, device=dev()).data_ptr(), None) == UNSUP
        rc, o = raw(sv, 1)
        assert rc == UNSUP and (sv._L.altro_last_error(sv.h) or b"").decode() and untouched(o)
        P0 = np.full(shapes(sv)["P0"], SENT)
        st = altro._lib.CtgOut(P0=P0.ctypes.data)
        assert sv._L.altro_batch_cost_to_go(sv.h, 1, C.byref(st), None) == UNSUP and (P0 == SENT).all()
        with pytest.raises(altro.AltroError):
            altro.cost_to_go(sv, penalty=True)
        after = everything(sv, cs.x0, len(cs.cons))
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
        rc, o = raw(sv, 0)
        assert rc == 0 and all((t != SENT).all() for k, t in o.items() if k != "fb") and (o["fb"] != -77).all()
    finally:
        sv.close()


def test_refusals_at_the_c_abi():
    """the argument rules of the header at the C-ABI itself: INVALID_ARG with nothing written and the handle unchanged and usable;
    an output one double short and a host pointer are refused; a 16-lane handle with N = 130 answers UNSUPPORTED for mode 1
    while its mode 0 succeeds and is finite"""
    cs = ER.add_box(ER.make_case(2, 12, 4, 6, 11), 0.9)
    sv = altro.ALTROSolver(ER.to_problem(altro, cs, shared=("cost", "box")), altro.SolverOptions(**OPTS))
    try:
        altro.solve(sv)
        L, h = sv._L, sv.h
        before = everything(sv, cs.x0, 1)
        fn, tw = L.altro_batch_cost_to_go_dev, L.altro_batch_cost_to_go
        for mode in (2, -1, 7):
            rc, o = raw(sv, mode)
            assert rc == INV and (L.altro_last_error(h) or b"").decode() and untouched(o), mode
        rc, o = raw(sv, 0, ())                                        # all six NULL (fb given)
        assert rc == INV and untouched(o)
        assert fn(h, 0, None, o["fb"].data_ptr()) == INV and untouched(o)
        st = altro._lib.CtgOut(v0=torch.zeros(2, dtype=torch.float64, device=dev()).data_ptr())
        assert fn(None, 0, C.byref(st), None) == INV and (L.altro_last_error(None) or b"").decode()
        v0h = np.full(2, SENT)
        sh = altro._lib.CtgOut(v0=v0h.ctypes.data)
        assert tw(None, 0, C.byref(sh), None) == INV and tw(h, 0, None, None) == INV and tw(h, 0, C.byref(altro._lib.CtgOut()), None) == INV
        assert tw(h, 3, C.byref(sh), None) == INV and (v0h == SENT).all()
        rc, o = raw(sv, 0, ("P0",), ptr=lambda t: v0h.ctypes.data)     # a host pointer
        assert rc == INV and untouched(o)
        paths = altro._lib.hip_runtimes()
        assert len(paths) == 1, paths
        rt = C.CDLL(paths[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]

        def short(t):      # the last doubles of the tensor's own allocation, one short
            base, size = C.c_void_p(), C.c_size_t()
            assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), C.c_void_p(t.data_ptr())) == 0
            return base.value + size.value - (t.numel() * 8 - 8)

        for k in NAMES:
            rc, o = raw(sv, 0, (k,), ptr=short)
            assert rc == INV and "shorter" in (L.altro_last_error(h) or b"").decode() and untouched(o), k
        altro.synchronize(sv)
        after = everything(sv, cs.x0, 1)
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
        for mode in (0, 1):
            rc, o = raw(sv, mode)
            assert rc == 0 and not untouched(o) and all((t != SENT).all() for k, t in o.items() if k != "fb")      # still usable
        rc, o = raw(sv, 0, ("v",), fb=False)                          # one output alone, fb NULL
        assert rc == 0 and (o["v"] != SENT).all() and (o["fb"] == -77).all()
    finally:
        sv.close()
    cl = ER.add_box(ER.make_case(2, 12, 4, 130, 12), 0.9)
    sv = altro.ALTROSolver(ER.to_problem(altro, cl, shared=("cost", "box")), altro.SolverOptions(**OPTS))
    try:
        altro.solve(sv)
        rc, o = raw(sv, 1)
        assert rc == UNSUP and untouched(o)
        rc, o = raw(sv, 0)
        assert rc == 0 and all(torch.isfinite(t).all() for k, t in o.items() if k != "fb") and (o["fb"] != -77).all()
    finally:
        sv.close()


def test_mode_0_beyond_the_stored_set_meets_the_rule():
    """a 16-lane handle at N = 130, two knots beyond the 128 the exact active set holds: mode 1 answers UNSUPPORTED and writes
    nothing, mode 0 reads no set and is within the rule on every output, on both forms.  (12, 4) at batch 2, "pi", the dynamics
    of evaluate_ref.make_case scaled by 0.75 as in lane16_horizons.stored_set_case (their eigenvalues reach 1.3 in modulus: 1e14
    over 129 knots), control bounds 0.5 and 0.6; seed 0: both instances SOLVE_SUCCEEDED on the oracle in 32 and 18 iterations"""
    cs = ER.make_case(2, 12, 4, 130, 0, per_instance_cost=True)
    cs.A = 0.75 * cs.A
    cs = ER.add_box(cs, lh.STORED_SET_UB + 0.1 * np.arange(2)[:, None] * np.ones((2, 4)))
    sv, cs = make_solver("16-box(12,4)-N130", True, cs, dict(shared=()))
    try:
        assert sv.N == 130 > lh.ASET_MAXN and altro.wave_cycles(sv).size != 0      # (the 16-lane backend)
        status = altro.stats(sv).status.copy()
        Xbar, Ubar = plane(sv)
        Kraw = altro.gains(sv)[0]
        before = everything(sv, cs.x0, 1)
        rc, o = raw(sv, 1)
        m0, host = ctg(sv, 0), ctg(sv, 0, host=True)
        after = everything(sv, cs.x0, 1)
    finally:
        sv.close()
    assert rc == UNSUP and untouched(o)
    assert (status == 1).all() and (m0.fb == 1).all(), (status, m0.fb)
    y, y64 = yardsticks(NS(cs=cs, Xbar=Xbar, Ubar=Ubar), 0, Kraw)
    w = check_accuracy(m0, y, y64, np.ones(cs.B, dtype=np.int32), "16-box(12,4)-N130 mode 0")
    print("16-box(12,4)-N130 mode 0 largest err / bound", w)
    for k in NAMES + ("fb",):
        assert same(getattr(host, k), getattr(m0, k)), k
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


@pytest.mark.parametrize("n,m", [(12, 4), (17, 5)])
def test_state_errors(n, m):
    """a handle on which nothing but create has happened, then with dynamics and no cost, then with no reference: ALTRO_ERR_STATE
    from both forms, nothing written"""
    L = altro._lib.lib()
    B, N = 3, 6
    h = C.c_void_p()
    dims = altro._lib.Dims(B, n, m, N)
    assert L.altro_batch_create(C.byref(dims), None, 0, C.byref(h)) == 0
    try:
        P0 = torch.full((B, n, n), 7.0, dtype=torch.float64, device=dev())
        fb = torch.full((B,), -77, dtype=torch.int32, device=dev())
        P0h = np.full((B, n, n), 7.0)
        rng = np.random.default_rng(5)

        def refused(what):
            for mode in (0, 1):
                assert L.altro_batch_cost_to_go_dev(h, mode, C.byref(altro._lib.CtgOut(P0=P0.data_ptr())), fb.data_ptr()) == STATE, what
                assert (L.altro_last_error(h) or b"").decode(), what
                assert L.altro_batch_cost_to_go(h, mode, C.byref(altro._lib.CtgOut(P0=P0h.ctypes.data)), None) == STATE, what
            torch.cuda.synchronize()
            assert (P0 == 7.0).all() and (fb == -77).all() and (P0h == 7.0).all(), what
        refused("nothing set")
        A, Bm = api._c(np.eye(n) + 0.1 * rng.standard_normal((n, n))), api._c(rng.standard_normal((n, m)))
        assert L.altro_batch_set_dynamics(h, api._p(A), api._p(Bm), None, 0, 0) == 0
        refused("no cost")
        assert L.altro_batch_set_tracking_cost(h, api._p(np.ones(n)), api._p(np.ones(m)), api._p(np.ones(n)), 0.1) == 0
        refused("no reference")
    finally:
        L.altro_batch_destroy(h)
