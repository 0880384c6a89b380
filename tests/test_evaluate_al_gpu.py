"""The solver's augmented Lagrangian on the device (altro_batch_evaluate_al_dev / altro_batch_evaluate_al,
altro_batch_get_penalty, altro.optimal_cost) on both backends.

Shapes: the cases of tests/test_evaluate_gpu.py as they are (batch 5, N = 9; (64, 32) at batch 2, N = 4) and a copy of
16-soc(6,3) whose LINEAR row is an equality.  Inputs: a solve with iterations_outer = 3, then of the duals it left a third kept,
a third zeroed and a third redrawn (evaluate_al_ref.draw_duals), then GR.candidates_with_polar's candidates -- the yardstick's
own branch counts say that every branch of the definition is reached.

Tolerances are the derived bounds of tests/evaluate_al_ref.py (its docstring has the derivations), none of them measured; the
measure is error over bound <= 1 against the numpy yardstick evaluated on the device's own Xout.  Everything else is an
equality of bytes, except the envelope identity, which is held instance by instance to 16 times the error the CPU oracle's
identical procedure shows.

The row tables, LDS sizes and shapes these cases do not reach are in tests/scoring_matrix.py."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc

import evaluate_ref as ER
import evaluate_grad_ref as GR
import evaluate_al_ref as AR
import test_evaluate_gpu as TE

pytestmark = pytest.mark.gpu
INV, STATE = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_STATE
T, H, dev = TE.T, TE.H, TE.dev
CASES = dict(TE.CASES)
CASES["16-soc-eq(6,3)"] = (AR.case_16_soc_eq, {})
FIELDS = altro._lib.AL_OUT_FIELDS
U_ = ER.U_
SOLVE = dict(iterations_outer=3, projected_newton=False)


def solver_of(cs, kw, **opts):
    return altro.ALTROSolver(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**dict(SOLVE, **opts)))


def shapes_of(sv, lead):
    n, m, N = sv.n, sv.m, sv.N
    return dict(LA=lead, J=lead, gU=lead + (N - 1, m), gx0=lead + (n,), gXref=lead + (N, n), gUref=lead + (N - 1, m), gQ=lead + (n,),
                gQf=lead + (n,), gR=lead + (m,), gzmin=lead + (n + m,), gzmax=lead + (n + m,), Xout=lead + (N, n))


def al(sv, U=None, x0=None, want=FIELDS):
    """device form on numpy inputs: NS of numpy arrays (None where not asked for); the outputs start as NaN"""
    lead = (sv.B,) if U is None else tuple(U.shape[:-2])
    sh = shapes_of(sv, lead)
    out = {k: torch.full(sh[k], np.nan, dtype=torch.float64, device=dev()) for k in want}
    got = altro.evaluate_al(sv, None if U is None else T(U), x0=None if x0 is None else T(x0), out=out)
    torch.cuda.synchronize()
    return NS(**{k: H(got.get(k)) for k in FIELDS})


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def same_outputs(a, b, what, keys=FIELDS):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        if x is not None and y is not None:
            assert same(x, y), (what, k)


def part(r, sl):
    return NS(**{k: (None if getattr(r, k) is None else getattr(r, k)[sl]) for k in FIELDS})


def duals_of(sv, cs):
    return [altro.get_duals(sv, i) for i in range(len(cs.cons))]


def install(sv, lam):
    for i, l in enumerate(lam):
        altro.set_duals(sv, l, i)


def check(name, cs, got, y, what):
    """every output within its derived bound of the yardstick; returns the largest error over bound"""
    worst = 0.0
    for k in AR.OUTS:
        g, w, b = getattr(got, k), getattr(y, k), AR.bound_of(y, k)
        assert np.isfinite(g).all(), (name, what, k)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.abs(g - w) == 0, 0.0, np.abs(g - w) / b)
        print(name, what, k, "max error / bound", ratio.max(), "max |value|", np.abs(w).max())
        assert (np.abs(g - w) <= b).all(), (name, what, k, ratio.max())
        # (bounds of rounding size, against the terms the output is made of: at a stationary point gU itself is ~0)
        scale = max(np.abs(w).max(), np.abs(y.Lx).max() if k in ("gU", "gx0") else 0.0)
        assert scale == 0 or (b <= 1e-8 * max(scale, 1.0)).all(), (name, what, k)
        worst = max(worst, float(ratio.max()))
    return worst


@functools.lru_cache(maxsize=None)
def scored(name):
    """every device call a case's tests look at, made once"""
    make, kw = CASES[name]
    cs = make()
    U = GR.candidates_with_polar(cs, 101)
    r = NS(cs=cs, U=U, kw=kw)
    sv = solver_of(cs, kw)
    try:
        try:
            altro.solve(sv)
            r.solved = True
        except altro.AltroError as e:       # (64, 32) is scored but not solved: the solve kernels' LDS limit.  Penalty 1, zero duals
            assert e.code == altro._lib.ERR_UNSUPPORTED and name == "wide-limits(64,32)"
            r.solved = False
        r.mu = altro.penalty(sv)
        r.mu_dev = H(altro.penalty(sv, out=torch.empty(cs.B, dtype=torch.float64, device=dev())))
        r.stats_cost = altro.stats(sv).cost.copy()
        r.lam0 = duals_of(sv, cs)
        r.Uheld = altro.controls(sv)
        r.held = al(sv)                                                  # U = NULL, x0 = NULL after the solve
        r.held_explicit = al(sv, U=H(altro.controls(sv, out=torch.empty((cs.B, cs.N - 1, cs.m), dtype=torch.float64, device=dev()))),
                             x0=cs.x0)
        r.lam = AR.draw_duals(cs, r.lam0, r.mu, 77)
        install(sv, r.lam)
        r.full = al(sv, U)
        r.ev = TE.ev(sv, U, Xout=True)                                   # evaluate_dev: J, c_max, defect, Xout
        r.again = al(sv, U)
        r.ws = al(sv, U, want=tuple(k for k in FIELDS if k != "Xout"))  # states into the workspace
        r.alone = [al(sv, U[:, c:c + 1]) for c in range(U.shape[1])]
        r.one = al(sv, U[:, 1])
        r.x0 = al(sv, U, x0=cs.x0)
        # every subset of null outputs, compared on the device
        Ut = T(U)
        ref = {k: T(getattr(r.full, k)) for k in FIELDS}
        bad = []
        names = FIELDS[:-1]
        for bits in range(1, 1 << len(names)):
            want = [k for i, k in enumerate(names) if (bits >> i) & 1] + (["Xout"] if bin(bits).count("1") % 2 else [])
            out = {k: torch.empty_like(ref[k]) for k in want}
            altro.evaluate_al(sv, Ut, out=out)
            if not all(torch.equal(out[k].view(torch.int64), ref[k].view(torch.int64)) for k in want):
                bad.append(bits)
        r.bad_subsets = bad
        host = {k: np.full(s, np.nan) for k, s in shapes_of(sv, U.shape[:2]).items()}
        altro.evaluate_al(sv, U, out=host)                               # host twin
        r.host = NS(**host)
        hp = altro.evaluate_al(sv, U, x0=cs.x0, out=("gx0", "gzmax"))
        r.hostp = NS(**{k: hp.get(k) for k in FIELDS})
        hh = altro.evaluate_al(sv, out=("LA", "gU"))                     # host twin, U = NULL under the drawn duals
        r.host_held = NS(**{k: hh.get(k) for k in FIELDS})
        r.held_drawn = al(sv)
    finally:
        sv.close()
    return r


# ---------------------------------------------------------------------------------------------- 1: parity
@pytest.mark.parametrize("name", list(CASES))
def test_every_output_within_its_bound_of_the_yardstick(name):
    """candidates under the drawn duals and U = NULL after the solve (the duals the solve left): Xout and J are evaluate_dev's
    bytes (the rollout and cost of the scoring core), every other output within its derived bound of the yardstick on the
    device's own Xout; the inputs reach every branch of the definition"""
    r = scored(name)
    cs = r.cs
    y = AR.al(cs, r.full.Xout, r.U, r.lam, r.mu)
    print(name, "mu", r.mu, "branch counts", y.counts)
    assert same(r.full.Xout, r.ev[3]) and same(r.full.J, r.ev[0])
    assert AR.reaches_every_branch(cs, y.counts), y.counts
    w1 = check(name, cs, r.full, y, "candidates")
    Uh = r.Uheld[:, None]
    yh = AR.al(cs, r.held.Xout[:, None], Uh, r.lam0, r.mu)
    w2 = check(name, cs, part(r.held, (slice(None), None)), yh, "held")
    print(name, "LARGEST error / bound", max(w1, w2), "stationarity |gU|_inf after the solve", np.abs(r.held.gU).max())


@pytest.mark.parametrize("name", list(CASES))
def test_penalty_and_reported_cost(name, oracle):
    """get_penalty (host and device forms) equals the oracle's penalties exactly after the same solve; LA(U = NULL) equals the
    cost get_stats reports within the value bound"""
    r = scored(name)
    cs = r.cs
    assert same(r.mu, r.mu_dev)
    if not r.solved:
        assert (r.mu == 1.0).all()
        return
    for b in range(cs.B):
        s = ER.oracle_of(oracle, cs, b, bool(r.kw.get("per_knot_dyn")))
        s.set_opts(oracle.default_opts(iterations_outer=3))
        s.solve()
        pen = np.concatenate([s.penalties(i) for i in range(len(cs.cons))])
        assert (pen == r.mu[b]).all(), (b, r.mu[b], np.unique(pen))
    yh = AR.al(cs, r.held.Xout[:, None], r.Uheld[:, None], r.lam0, r.mu)
    err = np.abs(r.held.LA - r.stats_cost)
    print(name, "max |LA - stats.cost| / bound", (err / yh.LAb[:, 0]).max())
    assert (err <= yh.LAb[:, 0]).all()


@pytest.mark.parametrize("name", list(CASES))
def test_restarted_handle_is_the_merit_at_rho_one(name):
    """zero duals and penalty 1 (a handle that has not solved): LA and gU agree with evaluate_grad_dev's J + P and gU at rho = 1
    within the two yardsticks' bounds"""
    make, kw = CASES[name]
    cs = make()
    U = GR.candidates_with_polar(cs, 101)
    sv = solver_of(cs, kw)
    try:
        assert (altro.penalty(sv) == 1.0).all()
        a = al(sv, U)
        J, P, gU, gx0 = (H(t) for t in altro.evaluate_grad(sv, T(U), rho=1.0))
    finally:
        sv.close()
    y = AR.al(cs, a.Xout, U, AR.zero_duals(cs), np.ones(cs.B))
    g = GR.merit_grad(cs, a.Xout, U, 1.0)
    assert same(a.J, J)
    assert (np.abs(a.LA - (J + P)) <= y.LAb + y.Jb + g.Pb + 2 * U_ * np.abs(a.LA)).all()
    assert (np.abs(a.gU - gU) <= 2 * y.gUb + 2 * g.gUb).all()
    assert (np.abs(a.gx0 - gx0) <= 2 * y.gx0b + 2 * g.gx0b).all()


# ---------------------------------------------------------------------------------------------- 2: invariances
@pytest.mark.parametrize("name", list(CASES))
def test_invariances_bit_for_bit(name):
    """a second identical call; the states in the workspace instead of Xout; every candidate alone (ncand = 1); the (B, N-1, m)
    shape; x0 = NULL against the held state passed explicitly; U = NULL against get_controls_dev's array passed explicitly;
    every subset of null outputs; the host twin"""
    r = scored(name)
    full = r.full
    same_outputs(full, r.again, "again")
    same_outputs(full, r.ws, "workspace")
    for c, a in enumerate(r.alone):
        same_outputs(part(full, (slice(None), slice(c, c + 1))), a, ("alone", c))
    assert r.one.LA.shape == (r.cs.B,) and r.one.gx0.shape == (r.cs.B, r.cs.n)
    same_outputs(part(full, (slice(None), 1)), r.one, "one")
    same_outputs(full, r.x0, "x0")
    same_outputs(r.held, r.held_explicit, "U = NULL")
    assert r.bad_subsets == []
    same_outputs(full, r.host, "host")
    same_outputs(full, r.hostp, "host, gx0 and gzmax only")
    same_outputs(r.held_drawn, r.host_held, "host, U = NULL")


@pytest.mark.parametrize("name", ["16-box(12,4)", "16-soc(6,3)", "wide-cone(7,3)", "wide-ltv(12,12)"])
def test_instance_alone_on_a_batch_one_handle(name):
    """instance b on a batch-1 handle holding its rows of data, after the same solve (the same penalty) and with its rows of the
    drawn duals: the bytes it gets inside the batch"""
    r = scored(name)
    for b in range(r.cs.B):
        sub = ER.sub_case(r.cs, b)
        sv = solver_of(sub, {k: v for k, v in r.kw.items() if k == "per_knot_dyn"})
        try:
            altro.solve(sv)
            assert same(altro.penalty(sv), r.mu[b:b + 1])
            install(sv, [l[b:b + 1] for l in r.lam])
            got = al(sv, r.U[b:b + 1])
        finally:
            sv.close()
        same_outputs(part(r.full, slice(b, b + 1)), got, ("batch-1", b))


# ---------------------------------------------------------------------------------------------- 3: the handle
@pytest.mark.parametrize("name", ["16-soc(6,3)", "wide-ltv(12,12)"])
def test_handle_unchanged(name):
    """a solve after the calls (device, host twin, U = NULL) is bit-identical to one on a handle that never made them"""
    make, kw = CASES[name]
    cs = make()
    U = ER.candidates(cs, 9)
    a, b = solver_of(cs, kw), solver_of(cs, kw)
    try:
        for rnd in range(2):
            al(b, U)
            al(b, U, x0=cs.x0 + 0.1, want=("LA", "gzmin"))
            al(b)
            altro.evaluate_al(b, U)
            altro.penalty(b)
            altro.solve(a), altro.solve(b)
            ea, eb = TE.everything(a, cs.x0), TE.everything(b, cs.x0)
            for k in ea:
                assert np.array_equal(ea[k], eb[k], equal_nan=True), (rnd, k)
            assert same(altro.penalty(a), altro.penalty(b))
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("name", ["16-box(12,4)", "wide-cone(7,3)"])
def test_sees_bounds_set_on_the_device(name):
    """set_bounds_dev with per-instance rows, then the call, nothing synchronised in between: every output is that of the
    yardstick on the new bounds"""
    r = scored(name)
    make, kw = CASES[name]
    cs = make()
    rng = np.random.default_rng(21)
    sv = solver_of(cs, kw)
    try:
        altro.solve(sv)
        install(sv, r.lam)
        ten = []
        for i, c in enumerate(cs.cons):
            if c.kind == "box":
                ub = 0.3 + 0.4 * rng.random((cs.B, cs.m))
                c.zmin[:, cs.n:], c.zmax[:, cs.n:] = -ub, ub
                ten.append((i, T(c.zmin), T(c.zmax)))
        for i, lo, hi in ten:
            altro.set_bounds(sv, i, lo, hi)
        g = al(sv, r.U)
        assert altro.dev_refusals(sv) == 0
    finally:
        sv.close()
    y = AR.al(cs, g.Xout, r.U, r.lam, r.mu)
    check(name, cs, g, y, "new bounds")
    assert (np.abs(g.LA - r.full.LA)[:, 1:] > 100 * y.LAb[:, 1:]).any()       # (the new bounds are not the old)


@pytest.mark.parametrize("force_wide", [False, True])
def test_staggered_clocks_see_their_own_window(monkeypatch, force_wide):
    """three MPC steps under a clock with starts 0, 1, 2, 0, 1: each instance's outputs are those of the window it holds, with
    the duals and the penalty the loop left"""
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
        lam, mu = [altro.get_duals(mp.solver, 0)], altro.penalty(mp.solver)
        g = al(mp.solver, U)
    finally:
        mp.solver.close()
    y = AR.al(cs, g.Xout, U, lam, mu)
    check("clock", cs, g, y, "force_wide %s" % force_wide)
    other = AR.al(ER.case_of_batch(pb, [3] * 5, cs.x0), g.Xout, U, lam, mu)
    assert (np.abs(g.gx0 - other.gx0)[[1, 2, 4]].max(axis=(1, 2)) > 1e6 * y.gx0b[[1, 2, 4]].max(axis=(1, 2))).all()


# ---------------------------------------------------------------------------------------------- 4: refusals
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
        L, B, n, nc = sv._L, sv.B, sv.n, 3
        Un = ER.candidates(ER.case_of_batch(pb, [0] * 5, prob.x0), 3)
        U = T(Un)
        SENT = -12345.5
        sh = shapes_of(sv, (B, nc))
        t = {k: torch.full(s, SENT, dtype=torch.float64, device=dev()) for k, s in sh.items()}
        host = np.zeros(sh["Xout"])
        hp = host.ctypes.data
        rt = C.CDLL(altro._lib.hip_runtimes()[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        base, size = C.c_void_p(), C.c_size_t()
        assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), C.c_void_p(t["gx0"].data_ptr())) == 0
        short = base.value + size.value - (B * nc * n * 8 - 8)           # the last B * ncand * n - 1 doubles of gx0's allocation
        st = lambda **kw: C.byref(altro._lib.ALOut(**{k: kw.get(k, t[k].data_ptr()) for k in FIELDS}))
        gp = lambda x: C.c_void_p(x.data_ptr())
        E = L.altro_batch_evaluate_al_dev
        none = {k: None for k in FIELDS if k != "Xout"}
        calls = [lambda: E(sv.h, nc, gp(U), None, None),                  # NULL out
                 lambda: E(sv.h, 0, gp(U), None, st()),                   # ncand < 1
                 lambda: E(sv.h, -2, gp(U), None, st()),
                 lambda: E(sv.h, nc, None, None, st()),                   # U NULL with ncand != 1
                 lambda: E(sv.h, nc, gp(U), None, st(**none)),            # no output but Xout
                 lambda: E(sv.h, nc, C.c_void_p(hp), None, st()),         # host pointers
                 lambda: E(sv.h, nc, gp(U), C.c_void_p(hp), st()),
                 lambda: E(sv.h, nc, gp(U), None, st(gXref=hp)),
                 lambda: E(sv.h, nc, gp(U), None, st(Xout=hp)),
                 lambda: E(sv.h, nc, gp(U), None, st(gx0=short))]         # one element short
        for i, call in enumerate(calls):
            rc = call()
            msg = (L.altro_last_error(sv.h) or b"").decode()
            assert rc == INV and msg, (i, rc, msg)
        assert "shorter" in msg
        assert E(None, nc, gp(U), None, st()) == INV and (L.altro_last_error(None) or b"").decode()
        assert L.altro_batch_get_penalty_dev(sv.h, None) == INV and L.altro_batch_get_penalty_dev(sv.h, C.c_void_p(hp)) == INV
        assert L.altro_batch_get_penalty(sv.h, None) == INV and L.altro_batch_get_penalty(None, None) == INV
        dp = C.POINTER(C.c_double)
        Eh = L.altro_batch_evaluate_al
        hj = np.full((B, nc), SENT)
        hs = lambda **kw: C.byref(altro._lib.ALOut(**kw))
        assert Eh(None, nc, Un.ctypes.data_as(dp), None, hs(LA=hj.ctypes.data)) == INV
        assert Eh(sv.h, nc, None, None, hs(LA=hj.ctypes.data)) == INV
        assert Eh(sv.h, 0, Un.ctypes.data_as(dp), None, hs(LA=hj.ctypes.data)) == INV
        assert Eh(sv.h, nc, Un.ctypes.data_as(dp), None, hs(Xout=host.ctypes.data)) == INV
        assert Eh(sv.h, nc, Un.ctypes.data_as(dp), None, None) == INV
        torch.cuda.synchronize()
        altro.synchronize(sv)
        for k in FIELDS:
            assert (t[k] == SENT).all(), k
        assert (hj == SENT).all() and (host == 0).all()
        same_outputs(al(sv, Un), al(tw, Un), "after the refusals")
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
        LA = torch.full((B, 1), 7.0, dtype=torch.float64, device=dev())
        assert L.altro_batch_evaluate_al_dev(h, 1, C.c_void_p(U.data_ptr()), None, C.byref(altro._lib.ALOut(LA=LA.data_ptr()))) == STATE
        assert (L.altro_last_error(h) or b"").decode()
        Jh = np.full((B, 1), 7.0)
        dp = C.POINTER(C.c_double)
        assert L.altro_batch_evaluate_al(h, 1, np.zeros((B, 1, N - 1, m)).ctypes.data_as(dp), None, C.byref(altro._lib.ALOut(J=Jh.ctypes.data))) == STATE
        torch.cuda.synchronize()
        assert (LA == 7.0).all() and (Jh == 7.0).all()
    finally:
        L.altro_batch_destroy(h)


# ---------------------------------------------------------------------------------------------- 5: envelope, autograd
TIGHT = AR.TIGHT


@pytest.mark.parametrize("name", ["16-box(12,4)", "wide-rows(20,5)"])
def test_envelope_on_the_device(name, oracle):
    """gx0 . d at U = NULL after a tight fixed-dual solve against central differences of the device's own tight fixed-dual
    re-solves at x0 +- h d, held INSTANCE BY INSTANCE to 16 times the error the oracle's identical procedure shows for the same
    instance, direction and step (the factor covers the device's other summation orders under the same stopping tolerances).
    The step of every instance comes from the oracle alone (AR.envelope_step): the first of a ladder at which the oracle's error
    is at least 1000 units in the last place of L_A over 2h.  Below that step the optimal cost is quadratic between the two
    points, both errors are a few such units and their ratio is chance (measured at h = 1e-4: 0.05 .. 77).  The check keeps its
    teeth: 16 times the oracle's error stays below 1e-6 of |gx0 . d|."""
    make, kw = CASES[name]
    cs = make()
    rng = np.random.default_rng(3)
    D = rng.standard_normal((cs.B, cs.n))
    steps = [AR.envelope_step(oracle, cs, b, bool(kw.get("per_knot_dyn")), D[b]) for b in range(cs.B)]
    h, ref = np.array([s[0] for s in steps]), np.array([s[1].err for s in steps])
    sv = solver_of(cs, kw)
    try:
        altro.solve(sv)
        lam = duals_of(sv, cs)
        api.set_options(sv, **TIGHT)
        altro.solve(sv)
        install(sv, lam)
        base = al(sv, want=("LA", "gx0", "gU"))
        U0 = altro.controls(sv)
        vals = []
        for sgn in (1.0, -1.0):
            altro.set_initial_state(sv, cs.x0 + sgn * h[:, None] * D)
            altro.initial_controls(sv, U0)
            install(sv, lam)
            altro.solve(sv)
            install(sv, lam)
            vals.append(al(sv, want=("LA",)).LA)
    finally:
        sv.close()
    fd = (vals[0] - vals[1]) / (2 * h)
    got = (base.gx0 * D).sum(axis=-1)
    err = np.abs(fd - got)
    print(name, "h", h, "device |fd - gx0.d|", err, "oracle", ref, "ratio", err / ref, "16 oracle / |gx0.d|", 16 * ref / np.abs(got),
          "oracle error in ulps of the quotient", ref / np.array([s[1].ulp for s in steps]), "stationarity", np.abs(base.gU).max())
    assert (err <= 16 * ref).all()
    assert (16 * ref <= 1e-6 * np.abs(got)).all()


@pytest.mark.parametrize("name", ["16-box(12,4)", "wide-cone(7,3)"])
def test_optimal_cost_autograd(name):
    """altro.optimal_cost: forward is LA of evaluate_al(U = NULL) after the solve, backward hands back w * gx0, w * gXref and
    w * gUref byte for byte; ExternalMPC.sensitivity is the same call"""
    make, kw = CASES[name]
    cs = make()
    sv = solver_of(cs, kw)
    try:
        x0, Xr, Ur = T(cs.x0).requires_grad_(), T(cs.Xref).requires_grad_(), T(cs.Uref).requires_grad_()
        w = T(np.random.default_rng(4).standard_normal(cs.B))
        V = altro.optimal_cost(sv, x0, Xr, Ur)
        assert V.grad_fn is not None and tuple(V.shape) == (cs.B,)
        V.backward(w)
        torch.cuda.synchronize()
        a = al(sv)
        s = altro.ExternalMPC(sv).sensitivity(out=("LA", "gx0"))
        assert same(H(V.detach()), a.LA) and same(s["LA"], a.LA) and same(s["gx0"], a.gx0)
        assert same(H(x0.grad), H(w[:, None] * T(a.gx0)))
        assert same(H(Xr.grad), H(w[:, None, None] * T(a.gXref)))
        assert same(H(Ur.grad), H(w[:, None, None] * T(a.gUref)))
        assert np.abs(a.gx0).max() > 0
    finally:
        sv.close()
