"""Closed-loop covariance of the stored policy (altro_batch_propagate_covariance_dev / altro_batch_propagate_covariance) on both
backends, against tests/covariance_ref.py run in np.longdouble.

Shapes, the smallest at which each code path can go wrong (N = 5 .. 8, one solve each):
  16-lane backend: (12, 4) with BOX at batch 9 (a padded wave and more than one wave); (6, 3) with a cone and a LINEAR row at
  batch 5 (evaluate_ref.case_16_soc's rows: sc for the SOC and for the LINEAR constraint); (6, 6) and (8, 4) with BOX at batch 5.
  one-wave-per-instance backend, batch 3: (12, 12) with per-knot dynamics and friction-pyramid rows on the controls, N = 6, after
  one MPC step so that the window is 1; (17, 5), padded to 32, with LINEAR rows up to the terminal knot; (64, 16); (30, 25) with
  state bounds up to the terminal knot.
Every shape runs twice: "shared" (one Sigma0 / W, one row of weights and bounds for the batch) and "pi" (one per instance).
Not in this list, and run by tests/test_stored_policy_matrix_gpu.py with the checks of this file (the table:
tests/stored_policy_matrix.py): a padded state of 48 -- (40, 6) with LINEAR rows, (48, 13), (48, 32): the three-tile strip of
gemm_rows under k_cov_wide's leading dimensions -- and mp > np, (12, 20), where Tt is sized by mp; there too, two live handles
above 64 KB of LDS called alternately.

The accuracy bound of an output array, per instance: err = max |out - ref| / max |ref| against the long-double yardstick must
not exceed 16 x max(err of the float64 yardstick against the same ref, 2^-52).  The bound is computed here from the two numpy
runs; nothing of the device enters it."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc

import covariance_ref as CR
import evaluate_ref as ER
from test_warm_start_gpu import H, T, assert_twins, dev, everything, plane, same

pytestmark = pytest.mark.gpu
INV, STATE = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_STATE
OPTS = dict(mpc.REF_OPTS, iterations=60)
LD = np.longdouble
EPS = 2.0 ** -52
SENT = -12345.5
KAPPA = 2.0
NAMES = ("sx", "su", "sc", "dJ", "zmin_t", "zmax_t", "Sout")


def build(name, pi):
    """(Case, to_problem keywords, index of the constraint sc is asked for or None, a second such index or None)"""
    u = lambda B, m, seed: 0.5 + np.random.default_rng(seed).random((B, m)) if pi else 0.9
    sh = () if pi else ("cost", "box")
    if name == "16-box(12,4)":
        return ER.add_box(ER.make_case(9, 12, 4, 6, 11, per_instance_cost=pi), u(9, 4, 12)), dict(shared=sh), None, None
    if name == "16-soc(6,3)":
        cs = ER.case_16_soc(B=5, N=7)
        if pi:
            cs.Q, cs.R = cs.Q * (1.0 + 0.1 * np.arange(5))[:, None], cs.R * (1.0 + 0.2 * np.arange(5))[:, None]
        return cs, dict(shared=() if pi else ("cost",)), 0, 1
    if name == "16(6,6)":
        return ER.add_box(ER.make_case(5, 6, 6, 5, 21, per_instance_cost=pi), u(5, 6, 22)), dict(shared=sh), None, None
    if name == "16(8,4)":
        return ER.add_box(ER.make_case(5, 8, 4, 8, 23, per_instance_cost=pi), u(5, 4, 24)), dict(shared=sh), None, None
    if name == "wide-ltv(12,12)":
        B, N, n, m = 3, 6, 12, 12
        cs = ER.add_box(ER.make_case(B, n, m, N, 14, per_knot_dyn=True, per_instance_cost=pi), u(B, m, 15) if pi else 0.8)
        # four friction pyramids on controls (3 q, 3 q + 1, 3 q + 2): |f_x| <= mu f_z + c, |f_y| <= mu f_z + c
        A = np.zeros((16, n + m))
        for q in range(4):
            for r, (col, sg) in enumerate(((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0))):
                A[4 * q + r, n + 3 * q + col], A[4 * q + r, n + 3 * q + 2] = sg, -0.6
        ER.add_rows(cs, "lin", A, np.full(16, -2.0), 0, N - 2)
        return cs, dict(per_knot_dyn=True, shared=sh + (1,)), 1, None
    if name == "wide(17,5)":
        B, N, n, m = 3, 5, 17, 5
        cs = ER.add_box(ER.make_case(B, n, m, N, 25, per_instance_cost=pi), u(B, m, 26))
        rng = np.random.default_rng(27)
        A = np.concatenate([0.02 * rng.standard_normal((B, N - 1, 3, n)), rng.standard_normal((B, N - 1, 3, m))], axis=-1)
        ER.add_rows(cs, "lin", A, -6.0 - rng.random((B, N - 1, 3)), 1, N - 1)
        return cs, dict(shared=sh), 1, None
    if name == "wide(64,16)":
        return ER.add_box(ER.make_case(3, 64, 16, 5, 28, per_instance_cost=pi), u(3, 16, 29)), dict(shared=sh), None, None
    if name == "wide(30,25)":
        cs = ER.make_case(3, 30, 25, 5, 15, per_instance_dyn=False, per_instance_cost=pi)
        return ER.add_box(cs, u(3, 25, 30) if pi else 1.0, x_bnd=6.0, k0=0, k1=4), dict(shared=sh + ("dyn",)), None, None
    raise KeyError(name)


SHAPES = ["16-box(12,4)", "16-soc(6,3)", "16(6,6)", "16(8,4)", "wide-ltv(12,12)", "wide(17,5)", "wide(64,16)", "wide(30,25)"]
RUNS = [(s, pi) for s in SHAPES for pi in (False, True)]
IDS = [s + ("-pi" if pi else "-shared") for s, pi in RUNS]


def moments(cs, pi, seed):
    """(Sigma0, W): symmetric positive semi-definite, (n, n) or (B, n, n); state deviations of about 0.05 at knot 0 whatever n,
    so that two deviations do not yet close the control bounds of the cases"""
    rng = np.random.default_rng(seed)
    lead = (cs.B,) if pi else ()
    scale = 0.05 / np.sqrt(cs.n)
    L0, Lw = scale * rng.standard_normal(lead + (cs.n, cs.n)), 0.1 * scale * rng.standard_normal(lead + (cs.n, cs.n))
    return np.ascontiguousarray(L0 @ np.swapaxes(L0, -1, -2)), np.ascontiguousarray(Lw @ np.swapaxes(Lw, -1, -2))


def make_solver(name, pi, cs=None, kw=None):
    """a solved handle of the case (the per-knot case: through TrackMPC, one MPC step, window 1) and the Case its covariance call
    sees"""
    if cs is None:
        cs, kw, _, _ = build(name, pi)
    if not kw.get("per_knot_dyn"):
        sv = altro.ALTROSolver(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**OPTS))
        altro.solve(sv)
        return sv, cs
    B, N, n, m = cs.B, cs.N, cs.n, cs.m
    rng = np.random.default_rng(41)
    nb = N + 3
    A = np.eye(n) + 0.3 * rng.standard_normal((B, nb, n, n)) / np.sqrt(n)
    Bm = 0.5 * rng.standard_normal((B, nb, n, m))
    f = 0.05 * rng.standard_normal((B, nb, n))
    Xt, Ut = rng.standard_normal((B, nb, n)), 0.3 * rng.standard_normal((B, nb - 1, m))
    cs.A, cs.Bm, cs.f = A[:, :N - 1].copy(), Bm[:, :N - 1].copy(), f[:, :N - 1].copy()
    cs.Xref, cs.Uref, cs.x0 = Xt[:, :N].copy(), Ut[:, :N - 1].copy(), Xt[:, 0].copy()
    mp = mpc.TrackMPC(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**OPTS), Xt, Ut, rng.standard_normal((2, B, n)), (np.full(n, 1e-3),))
    altro.set_dynamics_track(mp.solver, A, Bm, f, step_stride=1)
    mp.initial_solve()
    mp.step_async(0)
    mp.synchronize()
    cs.A, cs.Bm, cs.f = A[:, 1:N].copy(), Bm[:, 1:N].copy(), f[:, 1:N].copy()
    cs.Xref, cs.Uref, cs.x0 = Xt[:, 1:N + 1].copy(), Ut[:, 1:N].copy(), mp.x0()
    return mp.solver, cs


def cov(sv, cs, S0, W, con=None, kappa=None, host=False, Sout=True):
    """propagate_covariance on numpy inputs with sentinels in every output: NS of numpy arrays (None where not asked for)"""
    box = next((c for c in cs.cons if c.kind == "box"), None)
    shp = dict(sx=(sv.B, sv.N, sv.n), su=(sv.B, sv.N - 1, sv.m), dJ=(sv.B,), fb=(sv.B,))
    if Sout:
        shp["Sout"] = (sv.B, sv.N, sv.n, sv.n)
    if con is not None:
        c = cs.cons[con]
        shp["sc"] = (sv.B, c.k1 - c.k0 + 1, c.A.shape[2])
    if kappa is not None and box is not None:
        shp["zmin_t"] = shp["zmax_t"] = (sv.B, sv.n + sv.m)
    kap = kappa if "zmin_t" in shp else None
    if host:
        out = {k: np.full(s, -77, dtype=np.int32) if k == "fb" else np.full(s, SENT) for k, s in shp.items()}
        altro.propagate_covariance(sv, S0, W, con_id=con, kappa=kap, out=out)
        got = out
    else:
        out = {k: torch.full(s, -77, dtype=torch.int32, device=dev()) if k == "fb" else torch.full(s, SENT, dtype=torch.float64, device=dev())
               for k, s in shp.items()}
        altro.propagate_covariance(sv, None if S0 is None else T(S0), None if W is None else T(W), con_id=con, kappa=kap, out=out)
        torch.cuda.synchronize()
        got = {k: H(v) for k, v in out.items()}
    return NS(**{k: got.get(k) for k in NAMES + ("fb",)})


def yard(cs, K, S0, W, con=None, kappa=None, dtype=np.float64):
    box = next((c for c in cs.cons if c.kind == "box"), None)
    r = CR.propagate(cs, K, S0, W, rows=None if con is None else cs.cons[con], box=box if kappa is not None else None,
                     kappa=0.0 if kappa is None else kappa, dtype=dtype)
    r.Sout = r.S
    return r


def check_accuracy(got, cs, K, S0, W, con, kappa, what, report=()):
    """check 1 for every array `got` holds; returns the largest err / bound seen.  report: arrays whose figures are printed and
    not asserted"""
    ref, r64 = yard(cs, K, S0, W, con, kappa, LD), yard(cs, K, S0, W, con, kappa, np.float64)
    worst = 0.0
    for k in NAMES:
        g = getattr(got, k)
        if g is None:
            continue
        rf, r6 = getattr(ref, k), getattr(r64, k)
        assert g.shape == rf.shape and not (g == SENT).any(), (what, k)
        inf = ~np.isfinite(rf)
        assert np.array_equal(g[inf], rf[inf].astype(np.float64)), (what, k, "infinite sides stay")
        err, e64 = CR.rel_err(g, rf), CR.rel_err(r6, rf)
        bound = 16 * np.maximum(e64, EPS)
        zero = np.abs(np.where(inf, 0, rf)).reshape(cs.B, -1).max(axis=1) == 0
        assert k in report or (err <= bound).all(), (what, k, err, bound)
        for b in np.nonzero(zero)[0]:       # (identically zero: exactly +0.0)
            assert same(g[b][~inf[b]], np.zeros(int((~inf[b]).sum()))), (what, k, b)
        ratio = float((err / bound).max())
        print("%-28s %-7s err %.2e  float64 yardstick %.2e  bound %.2e  err/bound %.3f" % (what, k, err.max(), e64.max(), bound.min(), ratio))
        worst = max(worst, ratio)
    return worst


def dev_loop(cs, K, Xbar, Ubar, v, dtype):
    """|x_k - xbar_k| of the unclamped closed loop from xbar_0 + v, every operation in `dtype`: (B, N, n)"""
    t = lambda a: np.asarray(a, dtype=dtype)
    A, Bm, f, K, Xb, Ub = t(cs.A), t(cs.Bm), t(cs.f), t(K), t(Xbar), t(Ubar)
    x = Xb[:, 0] + t(v)
    D = np.zeros(Xb.shape, dtype=dtype)
    for k in range(cs.N):
        D[:, k] = np.abs(x - Xb[:, k])
        if k < cs.N - 1:
            u = Ub[:, k] + np.einsum("baj,bj->ba", K[:, k], x - Xb[:, k])
            x = np.einsum("bij,bj->bi", A[:, k], x) + np.einsum("bij,bj->bi", Bm[:, k], u) + f[:, k]
    return D


@functools.lru_cache(maxsize=None)
def ran(name, pi):
    """every device call a case's tests look at, made once on one solved handle"""
    cs0, kw, con, con2 = build(name, pi)
    sv, cs = make_solver(name, pi, cs0, kw)
    r = NS(cs=cs, kw=kw, con=con, con2=con2, pi=pi)
    try:
        box = next((c for c in cs.cons if c.kind == "box"), None)
        r.box = box
        r.before = everything(sv, cs.x0, len(cs.cons))
        r.Xbar, r.Ubar = plane(sv)
        r.Kraw = altro.gains(sv)[0]
        r.S0, r.W = moments(cs, pi, 51)
        fbp = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
        altro.eval_policy(sv, T(r.Xbar[:, 0]), fb=fbp)
        r.fb_policy = H(fbp)
        r.full = cov(sv, cs, r.S0, r.W, con, KAPPA)
        r.K = r.Kraw * r.full.fb[:, None, None, None]      # (an instance without valid gains runs the open loop)
        r.host = cov(sv, cs, r.S0, r.W, con, KAPPA, host=True)
        r.quiet = cov(sv, cs, r.S0, r.W, con, KAPPA, Sout=False)
        r.second = cov(sv, cs, r.S0, r.W, con2, None) if con2 is not None else None
        r.now = cov(sv, cs, r.S0, None, None, None)
        r.nos0 = cov(sv, cs, None, r.W, None, None)
        r.big = cov(sv, cs, r.S0, r.W, None, 1e6) if box is not None else None
        # rank one: Sigma0 = v v' (one v per instance), W NULL, against the simulation from xbar_0 + v
        r.v = 0.3 * np.random.default_rng(53).standard_normal((cs.B, cs.n))
        if not pi:      # shared matrices: one v for the batch
            r.v = np.repeat(r.v[:1], cs.B, axis=0)
        r.S1 = np.ascontiguousarray(np.einsum("bi,bj->bij", r.v, r.v) if pi else np.outer(r.v[0], r.v[0]))
        r.rank1 = cov(sv, cs, r.S1, None, None, None)
        Xo = torch.full((sv.B, 1, sv.N, sv.n), SENT, dtype=torch.float64, device=dev())
        altro.simulate_policy(sv, T((r.Xbar[:, 0] + r.v)[:, None]), None, clamp=False, out=(None, None, None), Xout=Xo)
        torch.cuda.synchronize()
        r.simdx = np.abs(H(Xo)[:, 0] - r.Xbar)
        r.after = everything(sv, cs.x0, len(cs.cons))
        # the tightened box goes back into the handle, and the next solve runs
        if box is not None:
            ref0 = api.dev_refusals(sv)
            altro.set_bounds(sv, cs.cons.index(box), T(r.full.zmin_t), T(r.full.zmax_t))
            r.refused = api.dev_refusals(sv) - ref0
            altro.solve(sv)
            r.status_after = altro.stats(sv).status.copy()
            r.dropped = cov(sv, cs, r.S0, r.W, con, None)       # (a solve made new gains: valid again)
        # a setter that drops the stored gains: the open loop
        prob = ER.to_problem(altro, cs, **kw)
        altro.set_tracking_cost(sv, prob.obj.Q, prob.obj.R, prob.obj.Qf)
        r.open = cov(sv, cs, r.S0, r.W, con, None)
    finally:
        sv.close()
    return r


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_accuracy_against_the_long_double_yardstick(name, pi):
    """1: every output array of every call within 16 x max(float64 yardstick's error, 2^-52) of the long-double yardstick;
    arrays that are identically zero are exactly +0.0 (sx at knot 0 without Sigma0).  The rank-one call (check 2's input) is held
    to the same bound on sx, dJ and Sout; its su is printed only: with Sigma = d d' it is |K d|, a cancelling sum whose error is
    relative to |K| |d| in the yardstick and on the device alike, and the ratio of two such errors is not bounded by 16 (seen:
    6.5e-15 against a float64 yardstick at 3.4e-16 on one instance of (12, 4))."""
    r = ran(name, pi)
    assert np.finfo(LD).nmant >= 63
    w = [check_accuracy(r.full, r.cs, r.K, r.S0, r.W, r.con, KAPPA, name + " full"),
         check_accuracy(r.now, r.cs, r.K, r.S0, None, None, None, name + " W null"),
         check_accuracy(r.nos0, r.cs, r.K, None, r.W, None, None, name + " Sigma0 null"),
         check_accuracy(r.rank1, r.cs, r.K, r.S1, None, None, None, name + " rank one", report=("su",))]
    if r.second is not None:
        w.append(check_accuracy(r.second, r.cs, r.K, r.S0, r.W, r.con2, None, name + " second constraint"))
    if r.big is not None:
        w.append(check_accuracy(r.big, r.cs, r.K, r.S0, r.W, None, 1e6, name + " kappa 1e6"))
    print(name, "pi" if pi else "shared", "largest err / bound", max(w))
    assert same(r.nos0.sx[:, 0], np.zeros((r.cs.B, r.cs.n))) and same(r.nos0.Sout[:, 0], np.zeros((r.cs.B, r.cs.n, r.cs.n)))


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_exact_cases_and_the_rank_one_cross_check(name, pi):
    """2: sx[:, 0] == sqrt(diag Sigma0) bit for bit, Sout[:, 0] == Sigma0; with Sigma0 = v v' and W NULL sx agrees with
    |x_k - xbar_k| of altro_batch_simulate_policy_dev(clamp = 0, x0 = xbar_0 + v) within the sum of the two calls' bounds against
    the long-double yardstick (16 x max(float64 error, 2^-52) each, of the covariance and of the closed loop)"""
    r = ran(name, pi)
    cs = r.cs
    S0 = np.broadcast_to(r.S0, (cs.B, cs.n, cs.n))
    assert same(r.full.sx[:, 0], np.sqrt(np.einsum("bii->bi", S0))) and same(r.full.Sout[:, 0], S0)
    K = r.K
    cref, c64 = yard(cs, K, r.S1, None, dtype=LD), yard(cs, K, r.S1, None)
    dref, d64 = dev_loop(cs, K, r.Xbar, r.Ubar, r.v, LD), dev_loop(cs, K, r.Xbar, r.Ubar, r.v, np.float64)
    bc = 16 * np.maximum(CR.rel_err(c64.sx, cref.sx), EPS) * np.abs(cref.sx).astype(np.float64).reshape(cs.B, -1).max(axis=1)
    bd = 16 * np.maximum(CR.rel_err(d64, dref), EPS) * np.abs(dref).astype(np.float64).reshape(cs.B, -1).max(axis=1)
    gap = np.abs(r.rank1.sx - r.simdx).reshape(cs.B, -1).max(axis=1)
    print(name, "rank one: gap", gap, "bound", bc + bd)
    assert (gap <= bc + bd).all()
    assert (r.simdx.reshape(cs.B, -1).max(axis=1) > 1e-3).all()


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_validity_flag(name, pi):
    """3: fb is eval_policy_dev's fb, at least one instance holds valid gains; after a setter that drops them fb = 0 everywhere,
    the outputs are the K = 0 recursion and su is exactly +0.0"""
    r = ran(name, pi)
    assert r.full.fb.dtype == np.int32 and same(r.full.fb, r.fb_policy) and (r.full.fb == 1).any(), r.full.fb
    for q in (r.host, r.quiet, r.now, r.nos0, r.rank1):
        assert same(q.fb, r.full.fb)
    assert (r.open.fb == 0).all()
    check_accuracy(r.open, r.cs, np.zeros_like(r.K), r.S0, r.W, r.con, None, name + " open loop")
    assert same(r.open.su, np.zeros_like(r.open.su))
    assert not same(r.open.sx, r.full.sx)


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_host_twin_and_quiet_form_write_the_same_bytes(name, pi):
    """4: the host twin writes the bytes the `_dev` form writes; without Sout the other outputs are the same bytes"""
    r = ran(name, pi)
    for k in NAMES + ("fb",):
        a, b = getattr(r.host, k), getattr(r.full, k)
        assert (a is None) == (b is None) and (a is None or (a.dtype == b.dtype and same(a, b))), k
        if k != "Sout":
            q = getattr(r.quiet, k)
            assert (q is None) == (b is None) and (q is None or same(q, b)), k
    assert r.quiet.Sout is None and r.host.sx is not None


@pytest.mark.parametrize("name,pi", [("16-box(12,4)", True), ("16-soc(6,3)", True), ("wide(17,5)", True), ("wide(30,25)", False)])
def test_instance_alone_on_a_batch_one_handle(name, pi):
    """5: instance b on a solved batch-1 handle holding its rows of data (same trajectory, same gains: checked first) gets the
    bytes it gets inside the batch"""
    r = ran(name, pi)
    S0, W = np.broadcast_to(r.S0, (r.cs.B, r.cs.n, r.cs.n)), np.broadcast_to(r.W, (r.cs.B, r.cs.n, r.cs.n))
    for b in range(r.cs.B):
        sub = ER.sub_case(r.cs, b)
        sv, _ = make_solver(name, pi, sub, {})
        try:
            Xb, Ub = plane(sv)
            assert same(Xb, r.Xbar[b:b + 1]) and same(Ub, r.Ubar[b:b + 1]) and same(altro.gains(sv)[0], r.Kraw[b:b + 1]), ("the solves differ", b)
            a = cov(sv, sub, np.array(S0[b:b + 1]), np.array(W[b:b + 1]), r.con, KAPPA)
        finally:
            sv.close()
        for k in NAMES + ("fb",):
            g = getattr(r.full, k)
            assert g is None or same(getattr(a, k), g[b:b + 1]), (b, k)


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_nothing_the_library_owns_changes(name, pi):
    """6, first half: states, controls, duals, gains, statistics and counters are byte-identical before and after the calls"""
    r = ran(name, pi)
    for k in r.before:
        assert np.array_equal(r.before[k], r.after[k], equal_nan=True), k


@pytest.mark.parametrize("name,pi", [("16-box(12,4)", True), ("16-soc(6,3)", False), ("wide(17,5)", True), ("wide(64,16)", False)])
def test_the_following_solve_equals_a_twin(name, pi):
    """6, second half: the solve that follows is byte-identical to that of a twin handle that never made the call"""
    cs, kw, con, _ = build(name, pi)
    (sv, _), (tw, _) = make_solver(name, pi, cs, kw), make_solver(name, pi, cs, kw)
    try:
        S0, W = moments(cs, pi, 51)
        cov(sv, cs, S0, W, con, KAPPA)
        cov(sv, cs, S0, W, con, KAPPA, host=True)
        assert_twins(sv, tw, cs.x0, len(cs.cons), "before the next solve")
        x0 = cs.x0 + 0.05
        for s in (sv, tw):
            altro.set_initial_state(s, x0)
            altro.solve(s)
        assert_twins(sv, tw, cs.x0, len(cs.cons), "after the next solve")
    finally:
        sv.close(), tw.close()


@pytest.mark.parametrize("name,pi", [(s, pi) for s, pi in RUNS if s != "16-soc(6,3)"], ids=[i for i in IDS if not i.startswith("16-soc")])
def test_tightened_box(name, pi):
    """7: zmin_t / zmax_t keep the BOX's pattern of finite sides and have lo' <= hi' (the accuracy is check 1), also with a kappa
    that collapses every two-sided interval to its midpoint; altro_batch_set_bounds_dev(per_instance = 1) refuses no row of them
    and the next solve runs"""
    r = ran(name, pi)
    lo, hi = r.box.zmin, r.box.zmax
    for q in (r.full, r.big):
        assert same(np.isfinite(q.zmin_t), np.isfinite(lo)) and same(np.isfinite(q.zmax_t), np.isfinite(hi))
        assert same(q.zmin_t[~np.isfinite(lo)], lo[~np.isfinite(lo)]) and same(q.zmax_t[~np.isfinite(hi)], hi[~np.isfinite(hi)])
        assert (q.zmin_t <= q.zmax_t).all()
        assert (q.zmin_t >= lo).all() and (q.zmax_t <= hi).all()
    two = np.isfinite(lo) & np.isfinite(hi)
    moved = two & (r.full.zmin_t > lo)
    assert moved.any() and (r.full.zmin_t < r.full.zmax_t)[moved].any()
    with np.errstate(invalid="ignore"):
        mid = 0.5 * (lo + hi)
        hit = two & (r.big.zmin_t == r.big.zmax_t)
    assert hit.any() and same(r.big.zmin_t[hit], mid[hit])
    assert r.refused == 0
    assert (r.status_after != 0).all()          # (every instance was solved again: none is left UNSOLVED)
    assert (r.dropped.fb == 1).any()


@pytest.mark.parametrize("name", ["16-box(12,4)", "wide(17,5)"])
def test_nan_stays_in_its_instance(name):
    """a NaN in one instance's Sigma0 stays a NaN in that instance's outputs and reaches no other instance"""
    r = ran(name, True)
    cs, kw, con, _ = build(name, True)
    sv, cs = make_solver(name, True, cs, kw)
    try:
        S0 = r.S0.copy()
        S0[1, 3, 3] = np.nan
        a = cov(sv, cs, S0, r.W, con, KAPPA)
    finally:
        sv.close()
    keep = np.arange(cs.B) != 1
    for k in NAMES + ("fb",):
        g = getattr(r.full, k)
        assert g is None or same(getattr(a, k)[keep], g[keep]), k
    assert np.isnan(a.sx[1, 0, 3]) and np.isnan(a.sx[1, 1:]).all() and np.isnan(a.dJ[1]) and np.isnan(a.Sout[1, 1:]).all()
    two = np.isfinite(r.box.zmin[1]) & np.isfinite(r.box.zmax[1])
    assert np.isnan(a.zmin_t[1][two]).all() and np.isnan(a.zmax_t[1][two]).all()


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name", ["16-box(12,4)", "16-soc(6,3)", "wide(17,5)"])
def test_refusals_launch_nothing(name):
    """8: every ALTRO_ERR_INVALID_ARG case of the header comment, a host pointer and a buffer one element short: refused with a
    message, the sentinel in every output untouched, the handle usable afterwards"""
    cs, kw, con, _ = build(name, True)
    (sv, _), (tw, _) = make_solver(name, True, cs, kw), make_solver(name, True, cs, kw)
    try:
        L, B, N, n, m = sv._L, sv.B, sv.N, sv.n, sv.m
        gp = lambda t: C.c_void_p(t.data_ptr())
        box = next((i for i, c in enumerate(cs.cons) if c.kind == "box"), None)
        S0n, Wn = moments(cs, True, 51)
        S0, W = T(S0n), T(Wn)
        full_t = lambda shape: torch.full(shape, SENT, dtype=torch.float64, device=dev())
        sx, su, dJ, zl, zh, So = full_t((B, N, n)), full_t((B, N - 1, m)), full_t((B,)), full_t((B, n + m)), full_t((B, n + m)), full_t((B, N, n, n))
        nsc = (cs.cons[con].k1 - cs.cons[con].k0 + 1, cs.cons[con].A.shape[2]) if con is not None else (1, 1)
        sc = full_t((B,) + nsc)
        fb = torch.full((B,), -77, dtype=torch.int32, device=dev())
        cid = sv.con_ids[con] if con is not None else -1
        host = np.zeros((B, N, n, n))
        hp = C.c_void_p(host.ctypes.data)
        paths = altro._lib.hip_runtimes()
        assert len(paths) == 1, paths
        rt = C.CDLL(paths[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        base, size = C.c_void_p(), C.c_size_t()
        assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(So)) == 0
        short = C.c_void_p(base.value + size.value - (B * N * n * n * 8 - 8))
        Wd = L.altro_batch_propagate_covariance_dev
        has_box = box is not None
        defaults = (("h", sv.h), ("S0", gp(S0)), ("W", gp(W)), ("pi", 1), ("con", cid), ("kappa", 1.0), ("sx", gp(sx)), ("su", gp(su)),
                    ("sc", gp(sc) if con is not None else None), ("dJ", gp(dJ)), ("fb", gp(fb)), ("zl", gp(zl) if has_box else None),
                    ("zh", gp(zh) if has_box else None), ("So", gp(So)))
        full = lambda **kw_: [kw_.get(k, d) for k, d in defaults]
        calls = [full(S0=None, W=None), full(sx=None, su=None, sc=None, dJ=None, fb=None, zl=None, zh=None, So=None, con=-1),
                 full(pi=2), full(pi=-1), full(kappa=-1.0), full(kappa=float("nan")), full(kappa=float("inf")),
                 full(zl=gp(zl), zh=None), full(zl=None, zh=gp(zh)),
                 full(con=-1, sc=gp(sc)), full(con=-2, sc=None), full(con=99), full(con=99, sc=None),
                 full(S0=hp), full(W=hp), full(sx=hp), full(su=hp), full(dJ=hp), full(fb=hp), full(So=hp), full(So=short)]
        if con is not None:
            calls += [full(sc=None), full(sc=hp)]
        if has_box:
            calls += [full(con=sv.con_ids[box], sc=gp(sc)), full(zl=hp), full(zh=hp)]
        else:
            calls += [full(zl=gp(zl), zh=gp(zh))]                       # the pair on a handle with no BOX
        for i, args in enumerate(calls):
            rc = Wd(*args)
            msg = (L.altro_last_error(sv.h) or b"").decode()
            assert rc == INV and msg, (i, rc, msg)
        assert Wd(*full(h=None)) == INV and (L.altro_last_error(None) or b"").decode()
        dp = C.POINTER(C.c_double)
        sxh = np.full((B, N, n), SENT)
        Z = L.altro_batch_propagate_covariance
        p_ = lambda a: a.ctypes.data_as(dp)
        none8 = [None] * 8
        assert Z(None, p_(S0n), None, 1, -1, 0.0, p_(sxh), *none8[1:]) == INV
        assert Z(sv.h, None, None, 1, -1, 0.0, p_(sxh), *none8[1:]) == INV
        assert Z(sv.h, p_(S0n), None, 1, -1, 0.0, *none8) == INV
        assert Z(sv.h, p_(S0n), None, 3, -1, 0.0, p_(sxh), *none8[1:]) == INV
        assert Z(sv.h, p_(S0n), None, 1, -1, -2.0, p_(sxh), *none8[1:]) == INV
        assert Z(sv.h, p_(S0n), None, 1, 99, 0.0, p_(sxh), *none8[1:]) == INV
        with pytest.raises(ValueError):
            altro.propagate_covariance(sv, S0.cpu(), W, out=dict(sx=sx))
        with pytest.raises(ValueError):
            api._propagate_covariance_dev(sv, S0.cpu(), W, out=dict(sx=sx))
        torch.cuda.synchronize()
        altro.synchronize(sv)
        for t in (sx, su, sc, dJ, zl, zh, So):
            assert (t == SENT).all()
        assert (fb == -77).all() and (sxh == SENT).all()
        assert_twins(sv, tw, cs.x0, len(cs.cons), "after the refusals")
        assert Wd(*full(sx=None, su=None, sc=None, dJ=None, zl=None, zh=None, So=None, con=-1)) == 0        # fb alone is fine
        assert Wd(*full(S0=None, su=None, sc=None, dJ=None, fb=None, zl=None, zh=None, So=None, con=-1)) == 0   # W and sx alone too
        torch.cuda.synchronize()
        assert (H(fb) == 1).any() and (sx != SENT).all() and (su == SENT).all()
        altro.solve(sv), altro.solve(tw)
        assert_twins(sv, tw, cs.x0, len(cs.cons), "after the next solve")
    finally:
        sv.close(), tw.close()


@pytest.mark.parametrize("n,m", [(12, 4), (17, 5)])
def test_state_errors(n, m):
    """a handle on which nothing but create has happened, then with dynamics and no cost, then with no reference:
    ALTRO_ERR_STATE from both forms, nothing written"""
    L = altro._lib.lib()
    B, N = 3, 6
    h = C.c_void_p()
    dims = altro._lib.Dims(B, n, m, N)
    assert L.altro_batch_create(C.byref(dims), None, 0, C.byref(h)) == 0
    try:
        sx = torch.full((B, N, n), 7.0, dtype=torch.float64, device=dev())
        fb = torch.full((B,), -77, dtype=torch.int32, device=dev())
        S0 = torch.eye(n, dtype=torch.float64, device=dev())
        gp = lambda t: C.c_void_p(t.data_ptr())
        dp = C.POINTER(C.c_double)
        sxh, S0h = np.full((B, N, n), 7.0), np.eye(n)
        rng = np.random.default_rng(5)

        def refused(what):
            assert L.altro_batch_propagate_covariance_dev(h, gp(S0), None, 0, -1, 0.0, gp(sx), None, None, None, gp(fb), None, None, None) == STATE, what
            assert (L.altro_last_error(h) or b"").decode(), what
            assert L.altro_batch_propagate_covariance(h, S0h.ctypes.data_as(dp), None, 0, -1, 0.0, sxh.ctypes.data_as(dp), None, None, None, None,
                                                      None, None, None) == STATE, what
            torch.cuda.synchronize()
            assert (sx == 7.0).all() and (fb == -77).all() and (sxh == 7.0).all(), what
        refused("nothing set")
        A, Bm = api._c(np.eye(n) + 0.1 * rng.standard_normal((n, n))), api._c(rng.standard_normal((n, m)))
        assert L.altro_batch_set_dynamics(h, api._p(A), api._p(Bm), None, 0, 0) == 0
        refused("no cost")
        assert L.altro_batch_set_tracking_cost(h, api._p(np.ones(n)), api._p(np.ones(m)), api._p(np.ones(n)), 0.1) == 0
        refused("no reference")
    finally:
        L.altro_batch_destroy(h)
