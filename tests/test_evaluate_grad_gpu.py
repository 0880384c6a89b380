"""Gradient of a candidate's merit on the device (altro_batch_evaluate_grad_dev / altro_batch_evaluate_grad, altro.merit) on
both backends.

Shapes: the cases of tests/test_evaluate_gpu.py as they are (batch 5, N = 9; (64, 32) at batch 2, N = 4), with the candidates
tests/test_evaluate_grad_api.py shows to be clear of every kink (seed 101; (7, 3) has a fourth candidate in the polar cone).

Tolerances are the derived bounds of tests/evaluate_grad_ref.py (its docstring has the derivations), none of them measured:
P within bound 5, gU and gx0 within twice bound 6, both against the numpy yardstick evaluated on the device's own Xout; finite
differences of the device's own J + rho P within bounds 3, 5, 6, 7 and 8.  Everything else is an equality of bytes.

The row tables, LDS sizes and shapes these cases do not reach are in tests/scoring_matrix.py."""
import ctypes as C
import functools
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc

import evaluate_ref as ER
import evaluate_grad_ref as GR
import test_evaluate_gpu as TE
import warm_start_ref as WR

pytestmark = pytest.mark.gpu
INV, STATE = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_STATE
CASES, T, H, dev, solver_of = TE.CASES, TE.T, TE.H, TE.dev, TE.solver_of
RHOS = (0.0, 1.0, 10.0)
OUTS = ("J", "P", "gU", "gx0")
U_ = ER.U_


def eg(sv, U, x0=None, rho=0.0, want=(1, 1, 1, 1), Xout=True):
    """device form on numpy inputs: NS(J, P, gU, gx0, X) back as numpy (None where not asked for); the outputs start as NaN"""
    lead = tuple(U.shape[:-2])
    shapes = (lead, lead, tuple(U.shape), lead + (sv.n,))
    out = tuple(torch.full(s, np.nan, dtype=torch.float64, device=dev()) if w else None for s, w in zip(shapes, want))
    Xo = torch.full(lead + (sv.N, sv.n), np.nan, dtype=torch.float64, device=dev()) if Xout else None
    got = altro.evaluate_grad(sv, T(U), x0=None if x0 is None else T(x0), rho=rho, out=out, Xout=Xo)
    torch.cuda.synchronize()
    return NS(X=H(Xo), **{k: H(t) for k, t in zip(OUTS, got)})


def same(a, b):
    return a.tobytes() == b.tobytes()


def same_outputs(a, b, what, keys=OUTS + ("X",)):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        if x is not None and y is not None:
            assert same(np.ascontiguousarray(x), np.ascontiguousarray(y)), (what, k)


@functools.lru_cache(maxsize=None)
def scored(name):
    """every device call a case's tests look at, made once"""
    make, kw = CASES[name]
    cs = make()
    U = GR.candidates_with_polar(cs, 101)
    r = NS(cs=cs, U=U, kw=kw)
    sv = solver_of(cs, kw)
    try:
        r.ev = TE.ev(sv, U, Xout=True)                                   # evaluate_dev: J, c_max, defect, Xout
        r.g = {rho: eg(sv, U, rho=rho) for rho in RHOS}
        r.again = eg(sv, U, rho=10.0)
        r.ws = eg(sv, U, rho=10.0, Xout=False)                           # states into the workspace
        r.alone = [eg(sv, U[:, c:c + 1], rho=10.0) for c in range(U.shape[1])]
        r.one = eg(sv, U[:, 1], rho=10.0)                                # U (B, N-1, m)
        r.x0 = eg(sv, U, x0=cs.x0, rho=10.0)
        r.subsets = {w: eg(sv, U, rho=10.0, want=w, Xout=bool(sum(w) % 2)) for w in itertools.product((0, 1), repeat=4) if any(w)}
        host = tuple(np.full(s, np.nan) for s in (U.shape[:2], U.shape[:2], U.shape, U.shape[:2] + (cs.n,)))
        Xh = np.full(U.shape[:2] + (cs.N, cs.n), np.nan)
        altro.evaluate_grad(sv, U, rho=10.0, out=host, Xout=Xh)          # host twin
        r.host = NS(X=Xh, **dict(zip(OUTS, host)))
        r.hostp = NS(X=None, **dict(zip(OUTS, altro.evaluate_grad(sv, U, x0=cs.x0, rho=10.0, out=(None, host[1].copy(), None, host[3].copy())))))
        # central differences of the device's own merit (test 3)
        rng = np.random.default_rng(8)
        X = r.g[10.0].X
        r.D, r.d0 = rng.standard_normal(U.shape), rng.standard_normal(U.shape[:2] + (cs.n,))
        r.fd = {}
        for what, D, d0 in (("U", r.D, None), ("x0", np.zeros(U.shape), r.d0)):
            g = GR.merit_grad(cs, X, U, 10.0, direction=(GR.tangent(cs, D, d0), D), state_err=GR.rollout_error(cs, X, U))
            h = GR.fd_step(g, 10.0, GR.merit(cs, X, U, 10.0)[1])
            pts = []
            for sgn in (1.0, -1.0):
                Up = np.ascontiguousarray(U + sgn * h[..., None, None] * D)
                if d0 is None:
                    pts.append((Up, eg(sv, Up, rho=10.0, want=(1, 1, 0, 0))))
                else:       # x0 is per instance: one call per candidate, each with its own perturbed state
                    per = [eg(sv, Up[:, c], x0=cs.x0 + sgn * h[:, c, None] * d0[:, c], rho=10.0, want=(1, 1, 0, 0)) for c in range(U.shape[1])]
                    pts.append((Up, NS(**{k: np.stack([getattr(p, k) for p in per], axis=1) for k in ("J", "P", "X")})))
            r.fd[what] = NS(g=g, h=h, pts=pts)
    finally:
        sv.close()
    return r


# ---------------------------------------------------------------------------------------------- 1: parity
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_evaluate_and_with_the_yardstick(name):
    """Xout and J are evaluate_dev's bytes for every rho; P within bound 5, gU and gx0 within twice bound 6 of the numpy
    yardstick on the device's own Xout; with rho = 0 the gradient is that of J alone and P is still there"""
    r = scored(name)
    Je, ce, de, Xe = r.ev
    for rho in RHOS:
        g = r.g[rho]
        assert same(g.X, Xe) and same(g.J, Je), rho
        y = GR.merit_grad(r.cs, g.X, r.U, rho)
        assert (y.margin >= 1e6).all()
        print(name, "rho", rho, "dP / bound", np.nanmax(np.abs(g.P - y.P) / y.Pb), "dgU / bound", (np.abs(g.gU - y.gU) / (2 * y.gUb)).max(),
              "dgx0 / bound", (np.abs(g.gx0 - y.gx0) / (2 * y.gx0b)).max(), "max |gU|", np.abs(y.gU).max())
        assert np.isfinite(g.P).all() and np.isfinite(g.gU).all() and np.isfinite(g.gx0).all()
        assert (np.abs(g.P - y.P) <= y.Pb).all()
        assert (np.abs(g.gU - y.gU) <= 2 * y.gUb).all()
        assert (np.abs(g.gx0 - y.gx0) <= 2 * y.gx0b).all()
        assert (y.gUb <= 1e-9 * np.abs(y.gU).max()).all()                 # (bounds of rounding size: a wrong term cannot hide)
    assert same(r.g[0.0].P, r.g[10.0].P) and (r.g[10.0].P[:, 1:3] > 0).any(axis=0).all()
    assert not same(r.g[0.0].gU, r.g[1.0].gU) and not same(r.g[1.0].gU, r.g[10.0].gU)


def residual_terms(cs):
    """how many residuals r one candidate's P = 1/2 sum r^2 has: per constraint and knot of its range, the two sides of every
    column a box holds there (state columns only at knot N-1), resp. the rows of a LINEAR / SOC block"""
    return sum(2 * (cs.n if k == cs.N - 1 else cs.n + cs.m) if c.kind == "box" else c.A.shape[2]
               for c in cs.cons for k in range(c.k0, c.k1 + 1))


@pytest.mark.parametrize("name", list(WR.CASES))
def test_largest_residual_behind_P_is_the_value_behind_c_max(name):
    """evaluate_dev (rollout form) and evaluate_grad_dev on the same U: c_max is the largest |r| and P = 1/2 sum r^2 over the
    same rows, so, with NO tolerance, c_max^2 <= 2 P (a sum of rounded non-negative squares never falls below its largest term,
    the halving is exact): it holds exactly when the largest |r| behind P is bit for bit the value behind c_max.  P == 0
    exactly where c_max == 0, and 2 P <= T c_max^2 (1 + (T + 2) u) for the T residual terms of the case (each square rounds
    once, at most T - 1 additions of two non-zero terms).  Not vacuous: at least a third of the rows have c_max > 0."""
    make, kw = WR.CASES[name]
    cs = make()
    U = GR.candidates_with_polar(cs, 5)
    sv = solver_of(cs, kw)
    try:
        J, c, d = TE.ev(sv, U)
        g = eg(sv, U, rho=10.0, want=(1, 1, 0, 0), Xout=False)
    finally:
        sv.close()
    assert same(g.J, J)
    assert np.isfinite(c).all() and np.isfinite(g.P).all()
    c2, P2, Tn = c * c, 2.0 * g.P, residual_terms(cs)
    print(name, "rows with c_max > 0:", int((c > 0).sum()), "of", c.size, "T", Tn, "min 2P / c_max^2", (P2[c > 0] / c2[c > 0]).min(),
          "max", (P2[c > 0] / c2[c > 0]).max())
    assert 3 * int((c > 0).sum()) >= c.size
    assert (c2 <= P2).all()
    assert ((g.P == 0.0) == (c == 0.0)).all()
    assert (P2 <= Tn * c2 * (1.0 + (Tn + 2) * U_)).all()


# ---------------------------------------------------------------------------------------------- 2: invariances
@pytest.mark.parametrize("name", list(CASES))
def test_invariances_bit_for_bit(name):
    """a second identical call; the states in the workspace instead of Xout; every candidate alone (ncand = 1); the (B, N-1, m)
    shape; x0 = None against the handle's state passed explicitly; every subset of NULL outputs; the host twin"""
    r = scored(name)
    full = r.g[10.0]
    same_outputs(full, r.again, "again")
    same_outputs(full, r.ws, "workspace")
    for c, a in enumerate(r.alone):
        same_outputs(NS(X=full.X[:, c:c + 1], **{k: getattr(full, k)[:, c:c + 1] for k in OUTS}), a, ("alone", c))
    assert r.one.J.shape == (r.cs.B,) and r.one.gx0.shape == (r.cs.B, r.cs.n)
    same_outputs(NS(X=full.X[:, 1], **{k: getattr(full, k)[:, 1] for k in OUTS}), r.one, "one")
    same_outputs(full, r.x0, "x0")
    assert len(r.subsets) == 15
    for w, s in r.subsets.items():
        assert all((getattr(s, k) is None) == (not on) for k, on in zip(OUTS, w)), w
        same_outputs(full, s, ("subset", w))
    same_outputs(full, r.host, "host")
    same_outputs(full, r.hostp, "host, P and gx0 only")


@pytest.mark.parametrize("name", ["16-box(12,4)", "16-soc(6,3)", "wide-cone(7,3)", "wide-ltv(12,12)"])
def test_instance_alone_on_a_batch_one_handle(name):
    """instance b on a batch-1 handle holding its rows of data: the bytes it gets inside the batch"""
    r = scored(name)
    full = r.g[10.0]
    for b in range(r.cs.B):
        sv = solver_of(ER.sub_case(r.cs, b), {k: v for k, v in r.kw.items() if k == "per_knot_dyn"})
        try:
            got = eg(sv, r.U[b:b + 1], rho=10.0)
        finally:
            sv.close()
        same_outputs(NS(X=full.X[b:b + 1], **{k: getattr(full, k)[b:b + 1] for k in OUTS}), got, ("batch-1", b))


# ---------------------------------------------------------------------------------------------- 3: finite differences
@pytest.mark.parametrize("name", list(CASES))
def test_device_central_differences(name):
    """the device's own J + 10 P at U +- h D (and x0 +- h d0) against the device's <gU, D> (<gx0, d0>), the step chosen from the
    margins so that no row changes side between the two points.  Tolerance: per point bounds 3 + 5 of M, bound 7 for the
    rounded states and one rounding of J + rho P, over 2h; twice bound 6 (with 7) times |D|; bound 8 for cone values on the
    boundary branch."""
    r = scored(name)
    full = r.g[10.0]
    for what in ("U", "x0"):
        f = r.fd[what]
        g, h = f.g, f.h
        assert (h > 0).all() and np.isfinite(h).all()
        M, err = [], 0.0
        for Up, p in f.pts:
            gp = GR.merit_grad(r.cs, p.X, Up, 10.0)
            assert (gp.margin >= 1e6).all()
            Mp = p.J + 10.0 * p.P
            err = err + GR.merit(r.cs, p.X, Up, 10.0)[1] + (np.abs(gp.Lx) * GR.rollout_error(r.cs, p.X, Up)).sum(axis=(2, 3)) + 2 * U_ * np.abs(Mp)
            M.append(Mp)
        fd = (M[0] - M[1]) / (2 * h)
        if what == "U":
            got, gb = (full.gU * r.D).sum(axis=(2, 3)), 2 * (g.gUb * np.abs(r.D)).sum(axis=(2, 3))
        else:
            got, gb = (full.gx0 * r.d0).sum(axis=-1), 2 * (g.gx0b * np.abs(r.d0)).sum(axis=-1)
        tol = err / (2 * h) + gb + GR.fd_truncation(g, 10.0, h)
        print(name, what, "h", h.min(), h.max(), "max |fd - <g, D>| / tol", (np.abs(fd - got) / tol).max(), "relative",
              (np.abs(fd - got) / np.abs(got)).max())
        assert (np.abs(fd - got) <= tol).all()
        assert (tol <= 1e-5 * np.abs(got)).all()                          # (the tolerance is far below the gradient)


# ---------------------------------------------------------------------------------------------- 4: handle unchanged
@pytest.mark.parametrize("name", ["16-box(12,4)", "wide-ltv(12,12)"])
def test_handle_unchanged(name):
    """a solve after the calls (device, host twin, merit) is bit-identical to one on a handle that never made them: states,
    controls, duals, statistics, traces, gains, counters"""
    make, kw = CASES[name]
    cs = make()
    U = ER.candidates(cs, 9)
    a, b = solver_of(cs, kw), solver_of(cs, kw)
    try:
        for rnd in range(2):
            eg(b, U, rho=10.0)
            eg(b, U, x0=cs.x0 + 0.1, rho=1.0, Xout=False)
            altro.evaluate_grad(b, U, rho=10.0)
            Ut = T(U).requires_grad_()
            altro.merit(b, Ut, rho=10.0).sum().backward()
            altro.solve(a), altro.solve(b)
            ea, eb = TE.everything(a, cs.x0), TE.everything(b, cs.x0)
            for k in ea:
                assert np.array_equal(ea[k], eb[k], equal_nan=True), (rnd, k)
    finally:
        a.close(), b.close()


# ---------------------------------------------------------------------------------------------- 5: sees the current data
@pytest.mark.parametrize("name", ["16-box(12,4)", "wide-cone(7,3)"])
def test_sees_bounds_set_on_the_device(name):
    """set_bounds_dev with per-instance rows, then the call, nothing synchronised in between: P and the gradient are those of
    the yardstick on the new bounds"""
    make, kw = CASES[name]
    cs = make()
    U = ER.candidates(cs, 6)
    rng = np.random.default_rng(21)
    sv = solver_of(cs, kw)
    try:
        before = eg(sv, U, rho=10.0)
        ten = []
        for i, c in enumerate(cs.cons):
            if c.kind == "box":
                ub = 0.3 + 0.4 * rng.random((cs.B, cs.m))
                c.zmin[:, cs.n:], c.zmax[:, cs.n:] = -ub, ub
                ten.append((i, T(c.zmin), T(c.zmax)))
        for i, lo, hi in ten:
            altro.set_bounds(sv, i, lo, hi)
        g = eg(sv, U, rho=10.0)
        y = GR.merit_grad(cs, g.X, U, 10.0)
        assert (np.abs(g.P - y.P) <= y.Pb).all() and (np.abs(g.gU - y.gU) <= 2 * y.gUb).all() and (np.abs(g.gx0 - y.gx0) <= 2 * y.gx0b).all()
        assert altro.dev_refusals(sv) == 0
        assert (np.abs(g.P - before.P)[:, 1:] > 100 * y.Pb[:, 1:]).all()    # (the new bounds are not the old)
    finally:
        sv.close()


@pytest.mark.parametrize("force_wide", [False, True])
def test_staggered_clocks_differentiate_their_own_window(monkeypatch, force_wide):
    """three MPC steps under a clock with starts 0, 1, 2, 0, 1: each instance's gradient is that of the window it holds"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    pb = TE.random_linear(5, 12, 4, 33)
    mp = mpc.BatchMPC(pb, altro.SolverOptions(**TE.OPTS))
    try:
        mp.initial_solve()
        mp.set_clock(np.array([0, 1, 2, 0, 1]))
        mp.run_async(3, first=0)
        mp.synchronize()
        win = api.get_clock(mp.solver)[2]
        assert list(win) == [3, 2, 1, 3, 2]
        cs = ER.case_of_batch(pb, win, mp.x0())
        U = ER.candidates(cs, 7)
        g = eg(mp.solver, U, rho=10.0)
        y = GR.merit_grad(cs, g.X, U, 10.0)
        assert (np.abs(g.P - y.P) <= y.Pb).all() and (np.abs(g.gU - y.gU) <= 2 * y.gUb).all() and (np.abs(g.gx0 - y.gx0) <= 2 * y.gx0b).all()
        other = GR.merit_grad(ER.case_of_batch(pb, [3] * 5, mp.x0()), g.X, U, 10.0)
        assert (np.abs(g.gx0 - other.gx0)[[1, 2, 4]].max(axis=(1, 2)) > 1e6 * y.gx0b[[1, 2, 4]].max(axis=(1, 2))).all()
    finally:
        mp.solver.close()


# ---------------------------------------------------------------------------------------------- 6: refusals
@pytest.mark.parametrize("force_wide", [False, True])
def test_refusals_launch_nothing(monkeypatch, force_wide):
    """every ALTRO_ERR_INVALID_ARG case of the contract, a host pointer and a buffer one element short: error 1 with a message,
    the sentinel in every output untouched; the handle's next call returns the bytes of a handle that was never refused"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    pb = TE.random_linear(5, 12, 4, 37)
    prob = mpc.gen_tracking_problem(pb)
    sv, tw = (altro.ALTROSolver(prob, altro.SolverOptions(**mpc.REF_OPTS)) for _ in range(2))
    try:
        L, B, n, m, N, nc = sv._L, sv.B, sv.n, sv.m, sv.N, 3
        gp = lambda t: C.c_void_p(t.data_ptr())
        Un = ER.candidates(ER.case_of_batch(pb, [0] * 5, prob.x0), 3)
        U, x0 = T(Un), T(prob.x0)
        SENT = -12345.5
        J, P = (torch.full((B, nc), SENT, dtype=torch.float64, device=dev()) for _ in range(2))
        gU = torch.full((B, nc, N - 1, m), SENT, dtype=torch.float64, device=dev())
        gx0 = torch.full((B, nc, n), SENT, dtype=torch.float64, device=dev())
        Xo = torch.full((B, nc, N, n), SENT, dtype=torch.float64, device=dev())
        host = np.zeros((B, nc, N, n))
        hp = C.c_void_p(host.ctypes.data)
        rt = C.CDLL(altro._lib.hip_runtimes()[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        base, size = C.c_void_p(), C.c_size_t()
        assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(gx0)) == 0
        short = C.c_void_p(base.value + size.value - (B * nc * n * 8 - 8))   # the last B * ncand * n - 1 doubles of gx0's allocation
        E = L.altro_batch_evaluate_grad_dev
        outs = (gp(J), gp(P), gp(gU), gp(gx0))
        calls = [lambda: E(sv.h, nc, None, None, 1.0, *outs, None),                      # NULL U
                 lambda: E(sv.h, 0, gp(U), None, 1.0, *outs, None),                      # ncand < 1
                 lambda: E(sv.h, -2, gp(U), None, 1.0, *outs, None),
                 lambda: E(sv.h, nc, gp(U), None, -1.0, *outs, None),                    # rho negative, NaN, infinite
                 lambda: E(sv.h, nc, gp(U), None, float("nan"), *outs, None),
                 lambda: E(sv.h, nc, gp(U), None, float("inf"), *outs, None),
                 lambda: E(sv.h, nc, gp(U), None, 1.0, None, None, None, None, gp(Xo)),  # no output
                 lambda: E(sv.h, nc, hp, None, 1.0, *outs, None),                        # host pointers
                 lambda: E(sv.h, nc, gp(U), hp, 1.0, *outs, None),
                 lambda: E(sv.h, nc, gp(U), None, 1.0, gp(J), gp(P), hp, gp(gx0), None),
                 lambda: E(sv.h, nc, gp(U), None, 1.0, *outs, hp),
                 lambda: E(sv.h, nc, gp(U), None, 1.0, gp(J), gp(P), gp(gU), short, gp(Xo))]   # one element short
        for i, call in enumerate(calls):
            rc = call()
            msg = (L.altro_last_error(sv.h) or b"").decode()
            assert rc == INV and msg, (i, rc, msg)
        assert "shorter" in msg
        assert E(None, nc, gp(U), None, 1.0, *outs, None) == INV and (L.altro_last_error(None) or b"").decode()
        dp = C.POINTER(C.c_double)
        Eh = L.altro_batch_evaluate_grad
        hj = np.full((B, nc), SENT)
        assert Eh(None, nc, Un.ctypes.data_as(dp), None, 1.0, hj.ctypes.data_as(dp), None, None, None, None) == INV
        assert Eh(sv.h, nc, None, None, 1.0, hj.ctypes.data_as(dp), None, None, None, None) == INV
        assert Eh(sv.h, 0, Un.ctypes.data_as(dp), None, 1.0, hj.ctypes.data_as(dp), None, None, None, None) == INV
        assert Eh(sv.h, nc, Un.ctypes.data_as(dp), None, -1.0, hj.ctypes.data_as(dp), None, None, None, None) == INV
        assert Eh(sv.h, nc, Un.ctypes.data_as(dp), None, 1.0, None, None, None, None, None) == INV
        torch.cuda.synchronize()
        altro.synchronize(sv)
        for t in (J, P, gU, gx0, Xo):
            assert (t == SENT).all()
        assert (hj == SENT).all()
        same_outputs(eg(sv, Un, rho=10.0), eg(tw, Un, rho=10.0), "after the refusals")
        altro.solve(sv), altro.solve(tw)
        ea, eb = TE.everything(sv, prob.x0), TE.everything(tw, prob.x0)
        for k in ea:
            assert np.array_equal(ea[k], eb[k], equal_nan=True), k
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
        g = torch.full((B, 1, N - 1, m), 7.0, dtype=torch.float64, device=dev())
        gp = lambda t: C.c_void_p(t.data_ptr())
        assert L.altro_batch_evaluate_grad_dev(h, 1, gp(U), None, 1.0, gp(J), None, gp(g), None, None) == STATE
        assert (L.altro_last_error(h) or b"").decode()
        Jh = np.full((B, 1), 7.0)
        dp = C.POINTER(C.c_double)
        assert L.altro_batch_evaluate_grad(h, 1, np.zeros((B, 1, N - 1, m)).ctypes.data_as(dp), None, 1.0, Jh.ctypes.data_as(dp), None, None, None, None) == STATE
        torch.cuda.synchronize()
        assert (J == 7.0).all() and (g == 7.0).all() and (Jh == 7.0).all()
    finally:
        L.altro_batch_destroy(h)


# ---------------------------------------------------------------------------------------------- 7: autograd
@pytest.mark.parametrize("name", ["16-soc(6,3)", "wide-rows(20,5)"])
def test_autograd(name):
    """merit(...).backward(w): U.grad == w[..., None, None] * gU and x0.grad == the candidate sum of w[..., None] * gx0, exactly;
    through U = (x0 @ W).view(...), W.grad == x0' (w gU) within the bound of a sum of B products, 2 (B + 1) u |x0|'|w gU|; the
    call runs on a non-default torch stream with nothing synchronised between the producer of U and the consumer of the
    gradient; ExternalMPC.merit is the same call"""
    r = scored(name)
    cs, full = r.cs, r.g[10.0]
    B, nc = r.U.shape[:2]
    rng = np.random.default_rng(5)
    w = rng.standard_normal((B, nc))
    sv = solver_of(cs, r.kw)
    try:
        Ut, x0t, wt = T(r.U).requires_grad_(), T(cs.x0).requires_grad_(), T(w)
        M = altro.merit(sv, Ut, x0=x0t, rho=10.0)
        assert M.grad_fn is not None and tuple(M.shape) == (B, nc)
        M.backward(wt)
        torch.cuda.synchronize()
        assert same(H(M.detach()), H(T(full.J) + 10.0 * T(full.P)))
        assert same(H(Ut.grad), H(wt[..., None, None] * T(full.gU)))
        assert same(H(x0t.grad), H((wt[..., None] * T(full.gx0)).sum(dim=1)))
        M1 = altro.ExternalMPC(sv).merit(T(r.U[:, 1]).requires_grad_(), rho=10.0)   # (B, N-1, m), x0 = None
        torch.cuda.synchronize()
        assert tuple(M1.shape) == (B,) and same(H(M1.detach()), H(T(full.J[:, 1]) + 10.0 * T(full.P[:, 1])))
        # U made from x0 by a linear map: the candidates are those of the case when W = pinv(x0) U (B <= n)
        flat = r.U.reshape(B, -1)
        Wn = np.linalg.pinv(cs.x0) @ flat
        Wt, xt = T(Wn).requires_grad_(), T(cs.x0)
        Uw = (xt @ Wt).view(r.U.shape)
        altro.merit(sv, Uw, rho=10.0).backward(wt)
        torch.cuda.synchronize()
        y = eg(sv, H(Uw.detach()), rho=10.0)
        G = (w[..., None, None] * y.gU).reshape(B, -1)
        want, bound = cs.x0.T @ G, 2 * (B + 1) * U_ * (np.abs(cs.x0).T @ np.abs(G))
        print(name, "dW / bound", (np.abs(H(Wt.grad) - want) / bound).max())
        assert (np.abs(H(Wt.grad) - want) <= bound).all()
        # stream-ordered: the producer of U and the consumer of U.grad share a non-default stream, and nothing waits in between
        half = T(0.5 * r.U)
        big = torch.randn(2048, 2048, device=dev())
        got = torch.zeros(r.U.shape, dtype=torch.float64, device=dev())
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream(dev())
        with torch.cuda.stream(s1):
            for _ in range(20):                                  # work ahead of the producer
                big = big @ big * 1e-3
            Us = (half + half).requires_grad_()                  # x + x is exact
            altro.merit(sv, Us, rho=10.0).backward(wt)
            got.copy_(Us.grad)
        s1.synchronize()
        assert same(H(got), H(Ut.grad))
        torch.cuda.synchronize()
    finally:
        sv.close()
