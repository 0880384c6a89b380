"""Warm start from the best of several candidates, chosen and installed on the device (altro_batch_warm_start_dev /
altro_batch_warm_start) on both backends.  Nothing here is a measured tolerance: every assertion is a byte equality or the
exact selection rule (tests/warm_start_ref.py).

Shapes: the cases of tests/test_evaluate_gpu.py (batch 5, N = 9; (64, 32) at batch 2, N = 4).  The handle's controls are the
reference controls; six candidates per instance -- the three of ER.candidates, a copy of candidate 0, a copy of the handle's
controls, one holding a NaN -- and the incumbent: 35 rows, a partial wave, instances straddling waves and 16-row blocks.  On
16-box also ncand = 1 and ncand = 17 (more rows per instance than a 256-thread block holds), and the (12, 4) case on both
backends.  The yardstick of every plane is the composition a caller had to write before: evaluate_dev with Xout, a gather by
`chosen`, set_initial_trajectory_dev -- on a twin handle.

The row tables, LDS sizes and shapes these cases do not reach are in tests/scoring_matrix.py."""
import ctypes as C
import functools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc, problems

import evaluate_ref as ER
import warm_start_ref as WR

pytestmark = pytest.mark.gpu
INV, STATE = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_STATE
OPTS = dict(mpc.REF_OPTS, iterations=60)
RUNS = [(name, False) for name in WR.CASES] + [("16-box(12,4)", True)]
IDS = [name + ("-forced-wide" if fw else "") for name, fw in RUNS]


def dev():
    return torch.device("cuda", 0)


def T(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev())


def H(t):
    return None if t is None else t.cpu().numpy()


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


class forced_wide:
    """ALTRO_FORCE_WIDE while solvers are created (read at creation)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("ALTRO_FORCE_WIDE")
        if self.on:
            os.environ["ALTRO_FORCE_WIDE"] = "1"

    def __exit__(self, *exc):
        if self.on:
            if self.old is None:
                del os.environ["ALTRO_FORCE_WIDE"]
            else:
                os.environ["ALTRO_FORCE_WIDE"] = self.old
        return False


def set_traj(sv, X, U):
    """host altro_batch_set_initial_trajectory with states"""
    X, U = api._c(X), api._c(U)
    sv._chk(sv._L.altro_batch_set_initial_trajectory(sv.h, api._p(X), api._p(U)))


def plane(sv):
    """(states, controls) through the device getters"""
    X = altro.states(sv, out=torch.empty((sv.B, sv.N, sv.n), dtype=torch.float64, device=dev()))
    U = altro.controls(sv, out=torch.empty((sv.B, sv.N - 1, sv.m), dtype=torch.float64, device=dev()))
    torch.cuda.synchronize()
    return H(X), H(U)


def ws(sv, U, rho=0.0, inc=True, host=False):
    """warm start on numpy inputs with sentinels in the outputs: (chosen, J, c_max) as numpy; host: the host twin"""
    nc1 = U.shape[1] + (1 if inc else 0)
    if host:
        out = (np.full(sv.B, -77, dtype=np.int32), np.full((sv.B, nc1), -5.5), np.full((sv.B, nc1), -5.5))
        return altro.warm_start(sv, U, rho=rho, include_current=inc, out=out)
    out = (torch.full((sv.B,), -77, dtype=torch.int32, device=dev()),) + tuple(
        torch.full((sv.B, nc1), -5.5, dtype=torch.float64, device=dev()) for _ in range(2))
    altro.warm_start(sv, T(U), rho=rho, include_current=inc, out=out)
    torch.cuda.synchronize()
    return tuple(H(o) for o in out)


def scores(tw, U, inc=True):
    """what the parent's calls give on a twin: (J, c_max (B, ncand + inc), X (B, ncand + inc, N, n), controls (same, N-1, m)) from
    evaluate_dev's rollout form with Xout on U; the last column from a second call on get_controls_dev's output"""
    parts = [T(U)]
    if inc:
        parts.append(altro.controls(tw, out=torch.empty((tw.B, tw.N - 1, tw.m), dtype=torch.float64, device=dev()))[:, None].contiguous())
    got = []
    for Up in parts:
        nc = Up.shape[1]
        J, c = (torch.empty((tw.B, nc), dtype=torch.float64, device=dev()) for _ in range(2))
        Xo = torch.empty((tw.B, nc, tw.N, tw.n), dtype=torch.float64, device=dev())
        altro.evaluate(tw, Up, out=(J, c, None), Xout=Xo)
        got.append((J, c, Xo, Up))
    torch.cuda.synchronize()
    return tuple(torch.cat([g[k] for g in got], dim=1).contiguous() for k in range(4))


def compose(tw, U, chosen, inc=True):
    """the composition on a twin: evaluate_dev with Xout, gather by `chosen` (the incumbent is column ncand; an instance with
    chosen < 0 keeps what it holds), set_initial_trajectory_dev.  Returns the scores."""
    J, c, Xo, Ut = scores(tw, U, inc)
    Xh = altro.states(tw, out=torch.empty((tw.B, tw.N, tw.n), dtype=torch.float64, device=dev()))
    Uh = altro.controls(tw, out=torch.empty((tw.B, tw.N - 1, tw.m), dtype=torch.float64, device=dev()))
    idx = torch.from_numpy(np.maximum(chosen, 0).astype(np.int64)).to(dev())
    keep = torch.from_numpy(chosen < 0).to(dev())
    ar = torch.arange(tw.B, device=dev())
    Xw = torch.where(keep[:, None, None], Xh, Xo[ar, idx]).contiguous()
    Uw = torch.where(keep[:, None, None], Uh, Ut[ar, idx]).contiguous()
    with api._bracket(tw):
        api._initial_trajectory_dev(tw, Xw, Uw)
    torch.cuda.synchronize()
    return H(J), H(c)


def everything(sv, x, ncons=1):
    """all the library owns that a caller can read"""
    st = altro.stats(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), it=st.iterations, ito=st.iterations_outer, status=st.status, cost=st.cost,
               cmax=st.c_max, Jt=st.cost_trace, ct=st.cmax_trace, alpha=altro.alpha_trace(sv))
    for i in range(ncons):
        out["dual%d" % i] = altro.get_duals(sv, i)
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


def assert_twins(a, b, x, ncons, what):
    ea, eb = everything(a, x, ncons), everything(b, x, ncons)
    for k in ea:
        assert np.array_equal(ea[k], eb[k], equal_nan=True), (what, k)


def solve_both(sv, tw, x, ncons, what, solvable=True):
    """the following solve on both handles, then everything a caller can read compared.  (64, 32) is scored and installed but
    not solved: the library's solve kernel refuses that size (ALTRO_ERR_UNSUPPORTED, the LDS of one CU) -- there both handles
    must refuse alike, and what they hold is compared as it stands"""
    for s in (sv, tw):
        if solvable:
            altro.solve(s)
        else:
            with pytest.raises(altro.AltroError) as e:
                altro.solve(s)
            assert e.value.code == altro._lib.ERR_UNSUPPORTED
    if solvable:
        assert_twins(sv, tw, x, ncons, what)
    else:
        (Xa, Ua), (Xb, Ub) = plane(sv), plane(tw)
        assert same(Xa, Xb) and same(Ua, Ub), what


def pair(cs, kw, fw=False):
    with forced_wide(fw):
        return tuple(altro.ALTROSolver(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**OPTS)) for _ in range(2))


@functools.lru_cache(maxsize=None)
def ran(name, fw):
    """every device call a case's tests look at, made once: a handle `sv` that gets the warm start and a twin `tw` that gets the
    composition, both reset to (zero states, reference controls) before every step"""
    make, kw = WR.CASES[name]
    cs = make()
    U = WR.six_candidates(cs, cs.Uref)
    B = cs.B
    r = NS(cs=cs, U=U, rho={})
    X0 = np.zeros((B, cs.N, cs.n))
    ncons = len(cs.cons)
    solvable = name != "wide-limits(64,32)"
    sv, tw = pair(cs, kw, fw)
    try:
        def reset():
            for s in (sv, tw):
                set_traj(s, X0, cs.Uref)
        reset()
        r.before = plane(sv)
        Je, ce, Xe, Ue = scores(tw, U)
        r.Je, r.ce, r.Xe = H(Je), H(ce), H(Xe)
        # the mask first (nothing has been solved yet: every step below starts from the same plane)
        r.mask = np.array([1, 0, 1, 1, 0][:B], dtype=np.int32)
        api.set_active(sv, r.mask)
        r.masked = ws(sv, U, 0.0)
        r.masked_plane = plane(sv)
        api.set_active(sv, None)
        reset()
        # no candidate with a finite merit, no incumbent
        r.none = ws(sv, np.full_like(U, np.nan), 0.0, inc=False)
        r.none_plane, r.none_twin = plane(sv), plane(tw)
        solve_both(sv, tw, cs.x0, ncons, "after chosen = -1", solvable)
        for rho in WR.RHOS:
            reset()
            q = NS()
            q.chosen, q.J, q.c = ws(sv, U, rho)
            q.Jt, q.ct = compose(tw, U, q.chosen)
            q.plane, q.twin = plane(sv), plane(tw)
            solve_both(sv, tw, cs.x0, ncons, ("after the solve", rho), solvable)
            r.rho[rho] = q
        # the host twin against the device form
        reset()
        r.host = ws(sv, U, 1e3, host=True)
        r.devc = ws(tw, U, 1e3)
        r.host_plane, r.dev_plane = plane(sv), plane(tw)
        # outputs left out: the merits go to the library's workspace
        reset()
        altro.warm_start(sv, T(U), rho=1e3, out=(None, None, None))
        r.null_plane = plane(sv)
    finally:
        sv.close(), tw.close()
    return r


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_scores_are_the_bytes_of_evaluate(name, fw):
    """1: J[:, :ncand], c_max[:, :ncand] are evaluate_dev's rollout-form bytes, the last column those of evaluate_dev on
    get_controls_dev's output; the NaN candidate's scores are NaN; the same for every rho"""
    r = ran(name, fw)
    for rho, q in r.rho.items():
        assert same(q.J, r.Je) and same(q.c, r.ce), rho
        assert same(q.J, q.Jt) and same(q.c, q.ct), rho
        assert np.isnan(q.J[:, 5]).all() and np.isnan(q.c[:, 5]).all()
        assert np.isfinite(q.J[:, [0, 1, 2, 3, 4, 6]]).all() and np.isfinite(q.c[:, [0, 1, 2, 3, 4, 6]]).all()
        assert same(q.J[:, 3], q.J[:, 0]) and same(q.J[:, 4], q.J[:, 6]) and same(q.c[:, 4], q.c[:, 6])


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_chosen_follows_the_rule_and_the_yardstick(name, fw):
    """2: chosen equals the rule on the device's own bytes and the numpy yardstick's winner (decidable:
    test_warm_start_api.py); duplicates never beat their originals, the NaN candidate is never chosen"""
    r = ran(name, fw)
    for rho, q in r.rho.items():
        assert q.chosen.dtype == np.int32 and list(q.chosen) == list(WR.select(q.J, q.c, rho, True)), rho
        win3 = WR.decided(r.cs, ER.candidates(r.cs, 5), r.cs.Uref, rho)[0]
        print(name, rho, list(q.chosen))
        assert list(q.chosen) == list(WR.expected_of_six(win3)), rho
        assert not np.isin(q.chosen, [3, 4, 5]).any()
    if name == "16-soc(6,3)":
        assert list(r.rho[0.0].chosen) != list(r.rho[1e3].chosen)


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_plane_is_the_composition(name, fw):
    """3: states and controls are byte-equal to those the composition leaves on a twin (the solves that follow are compared
    inside ran(): states, controls, duals, statistics, gains, counters); an incumbent that wins has its states re-rolled"""
    r = ran(name, fw)
    for rho, q in r.rho.items():
        assert same(q.plane[0], q.twin[0]) and same(q.plane[1], q.twin[1]), rho
        for b, w in enumerate(q.chosen):
            assert same(q.plane[0][b], r.Xe[b, w]) and same(q.plane[1][b], r.U[b, w] if w < 6 else r.cs.Uref[b]), (rho, b)
        assert not same(q.plane[0], r.before[0])
    assert same(r.null_plane[0], r.rho[1e3].plane[0]) and same(r.null_plane[1], r.rho[1e3].plane[1])


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_nothing_finite_installs_nothing(name, fw):
    """4: all candidates NaN, no incumbent: chosen = -1, the plane is that of an untouched twin (the next solve is compared
    inside ran())"""
    r = ran(name, fw)
    ch, J, c = r.none
    assert (ch == -1).all() and J.shape == (r.cs.B, 6) and np.isnan(J).all() and np.isnan(c).all()
    assert same(r.none_plane[0], r.none_twin[0]) and same(r.none_plane[1], r.none_twin[1])
    assert same(r.none_plane[0], r.before[0]) and same(r.none_plane[1], r.before[1])


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_mask(name, fw):
    """5: inactive instances get -2 and keep their bytes, active ones are as in the unmasked run; scoring is not masked"""
    r = ran(name, fw)
    ch, J, c = r.masked
    q = r.rho[0.0]
    on = r.mask != 0
    assert list(ch) == list(np.where(on, q.chosen, -2)) and list(ch) == list(WR.select(J, c, 0.0, True, active=r.mask))
    assert same(J, q.J) and same(c, q.c)
    for k in (0, 1):
        assert same(r.masked_plane[k][on], q.plane[k][on]) and same(r.masked_plane[k][~on], r.before[k][~on])
    assert (~on).any() and not same(q.plane[0][~on], r.before[0][~on])


@pytest.mark.parametrize("name,fw", RUNS, ids=IDS)
def test_host_twin_writes_the_same_bytes(name, fw):
    """7"""
    r = ran(name, fw)
    for a, b in zip(r.host, r.devc):
        assert a.dtype == b.dtype and same(a, b)
    assert same(r.host[0], r.rho[1e3].chosen) and same(r.host[1], r.rho[1e3].J)
    assert same(r.host_plane[0], r.dev_plane[0]) and same(r.host_plane[1], r.dev_plane[1])
    assert same(r.host_plane[0], r.rho[1e3].plane[0])


@pytest.mark.parametrize("ncand", [1, 17])
def test_one_candidate_and_more_rows_than_a_block(ncand):
    """16-box with ncand = 1 and ncand = 17 (18 rows per instance with the incumbent: more than the 16 of a 256-thread block):
    scores, rule and plane as above, with and without the incumbent"""
    cs = ER.case_16_box()
    U3 = ER.candidates(cs, 5)
    U = np.ascontiguousarray(np.stack([U3[:, j % 3] * (1.0 - 0.02 * (j // 3)) for j in range(ncand)], axis=1))
    X0 = np.zeros((cs.B, cs.N, cs.n))
    sv, tw = pair(cs, {})
    try:
        for inc in (True, False):
            for s in (sv, tw):
                set_traj(s, X0, cs.Uref)
            ch, J, c = ws(sv, U, 10.0, inc=inc)
            Jt, ct = compose(tw, U, ch, inc=inc)
            assert J.shape == (cs.B, ncand + inc) and same(J, Jt) and same(c, ct)
            assert list(ch) == list(WR.select(J, c, 10.0, inc))
            (Xa, Ua), (Xb, Ub) = plane(sv), plane(tw)
            assert same(Xa, Xb) and same(Ua, Ub)
            print(ncand, inc, list(ch))
        if ncand == 17:
            assert len(set(ch)) > 1
    finally:
        sv.close(), tw.close()


# ---------------------------------------------------------------------------------------------- seen as the next solve sees it
@pytest.mark.parametrize("name", ["16-box(12,4)", "16-soc(6,3)", "wide-cone(7,3)"])
def test_sees_device_setters_earlier_on_the_stream(name):
    """6: set_initial_state_dev, set_reference_dev, set_bounds_dev (per-instance rows) and update_constraint_data_dev, then the
    warm start, nothing synchronised in between: scores, choice and plane are those of a twin that synchronised after the same
    setters and was given the composition"""
    make, kw = WR.CASES[name]
    cs = make()
    U = WR.six_candidates(cs, cs.Uref)
    rng = np.random.default_rng(21)
    sv, tw = pair(cs, kw)
    try:
        X0 = np.zeros((cs.B, cs.N, cs.n))
        for s in (sv, tw):
            set_traj(s, X0, cs.Uref)
        before = scores(tw, U)
        x0 = cs.x0 + 0.3 * rng.standard_normal(cs.x0.shape)
        Xref = cs.Xref + 0.5 * rng.standard_normal(cs.Xref.shape)
        Uref = cs.Uref + 0.2 * rng.standard_normal(cs.Uref.shape)
        ten = [T(x0), T(Xref), T(Uref)]
        for i, c in enumerate(cs.cons):
            if c.kind == "box":
                ub = 0.3 + 0.4 * rng.random((cs.B, cs.m))
                zmin, zmax = c.zmin.copy(), c.zmax.copy()
                zmin[:, cs.n:], zmax[:, cs.n:] = -ub, ub
                ten += [T(zmin), T(zmax)]
            else:
                A, b = c.A * (0.6 + rng.random(c.A.shape)), c.b * (0.6 + 0.8 * rng.random(c.b.shape))
                sh = i in kw.get("shared", ())
                ten += [T(A[0, 0] if sh else A), T(b[0, 0] if sh else b)]
        Ut = T(U)
        out = (torch.full((cs.B,), -77, dtype=torch.int32, device=dev()),) + tuple(torch.empty((cs.B, 7), dtype=torch.float64, device=dev()) for _ in range(2))

        def setters(s):
            it = iter(ten)
            altro.set_initial_state(s, next(it))
            altro.update_trajectory(s, next(it), next(it))
            for i, c in enumerate(cs.cons):
                if c.kind == "box":
                    altro.set_bounds(s, i, next(it), next(it))
                else:
                    altro.update_constraint_data(s, i, next(it), next(it))
        setters(sv)
        altro.warm_start(sv, Ut, rho=1e3, out=out)
        torch.cuda.synchronize()
        ch, J, c_ = (H(o) for o in out)
        setters(tw)
        torch.cuda.synchronize()
        altro.synchronize(tw)
        Jt, ct = compose(tw, U, ch)
        assert same(J, Jt) and same(c_, ct) and list(ch) == list(WR.select(J, c_, 1e3, True))
        (Xa, Ua), (Xb, Ub) = plane(sv), plane(tw)
        assert same(Xa, Xb) and same(Ua, Ub) and same(Xa[:, 0], x0)
        assert altro.dev_refusals(sv) == 0
        assert (J[:, :5] != H(before[0])[:, :5]).all() and (c_ != H(before[1])).any()     # (the new data is not the old)
        altro.solve(sv), altro.solve(tw)
        assert_twins(sv, tw, x0, len(cs.cons), "after the solve")
    finally:
        sv.close(), tw.close()


@pytest.mark.parametrize("force_wide", [False, True])
def test_staggered_clocks_score_against_their_own_window(monkeypatch, force_wide):
    """6: three MPC steps under a clock with starts 0, 1, 2, 0, 1: each instance is scored against the window it holds"""
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
        win = api.get_clock(a.solver)[2]
        assert list(win) == [3, 2, 1, 3, 2]
        cs = ER.case_of_batch(pb, win, a.x0())
        U = ER.candidates(cs, 7)
        ch, J, c = ws(a.solver, U, 1e3)
        Jt, ct = compose(b.solver, U, ch)
        assert same(J, Jt) and same(c, ct) and list(ch) == list(WR.select(J, c, 1e3, True))
        (Xa, Ua), (Xb, Ub) = plane(a.solver), plane(b.solver)
        assert same(Xa, Xb) and same(Ua, Ub)
        other = ER.case_of_batch(pb, [3] * 5, a.x0())
        Xc = np.ascontiguousarray(H(scores(b.solver, U, inc=False)[2]))
        Jn, Jb = ER.cost(cs, Xc, U)
        assert (np.abs(Jn - ER.cost(other, Xc, U)[0])[[1, 2, 4]] > 100 * Jb[[1, 2, 4]]).all()   # (the windows differ)
        assert list(api.get_clock(a.solver)[2]) == [3, 2, 1, 3, 2]
        for mp in (a, b):
            mp.run_async(1, first=3)
            mp.synchronize()
        assert_twins(a.solver, b.solver, cs.x0, 1, "after the next step")
    finally:
        a.solver.close(), b.solver.close()


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("force_wide", [False, True])
def test_refusals_launch_nothing(monkeypatch, force_wide):
    """8: every ALTRO_ERR_INVALID_ARG case of the contract, a host pointer and a buffer one element short: error 1 with a
    message, the sentinel in every output untouched, and the next solve equals a twin's"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    pb = problems.gen_random_linear_batch(5, n=12, m=4, N=9, steps=8, seed=37, u_bnd=3.0)
    prob = mpc.gen_tracking_problem(pb)
    sv, tw = (altro.ALTROSolver(prob, altro.SolverOptions(**mpc.REF_OPTS)) for _ in range(2))
    try:
        L, B, nc = sv._L, sv.B, 3
        gp = lambda t: C.c_void_p(t.data_ptr())
        U = T(ER.candidates(ER.case_of_batch(pb, [0] * 5, prob.x0), 3))
        SENT = -12345.5
        J, c = (torch.full((B, nc + 1), SENT, dtype=torch.float64, device=dev()) for _ in range(2))
        ch = torch.full((B,), -77, dtype=torch.int32, device=dev())
        host = np.zeros((B, nc, sv.N, sv.n))
        hp = C.c_void_p(host.ctypes.data)
        paths = altro._lib.hip_runtimes()
        assert len(paths) == 1, paths
        rt = C.CDLL(paths[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        base, size = C.c_void_p(), C.c_size_t()
        assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(J)) == 0
        short = C.c_void_p(base.value + size.value - (B * (nc + 1) * 8 - 8))      # the last B * (ncand + 1) - 1 doubles of J's allocation
        W = L.altro_batch_warm_start_dev
        before = plane(sv)
        calls = [lambda: W(sv.h, nc, None, 0.0, 1, gp(ch), gp(J), gp(c)),                   # no U
                 lambda: W(sv.h, 0, gp(U), 0.0, 1, gp(ch), gp(J), gp(c)),                   # ncand < 1
                 lambda: W(sv.h, -2, gp(U), 0.0, 1, gp(ch), gp(J), gp(c)),
                 lambda: W(sv.h, nc, gp(U), -1.0, 1, gp(ch), gp(J), gp(c)),                 # rho
                 lambda: W(sv.h, nc, gp(U), float("nan"), 1, gp(ch), gp(J), gp(c)),
                 lambda: W(sv.h, nc, gp(U), float("inf"), 1, gp(ch), gp(J), gp(c)),
                 lambda: W(sv.h, nc, gp(U), 0.0, 2, gp(ch), gp(J), gp(c)),                  # include_current
                 lambda: W(sv.h, nc, gp(U), 0.0, -1, gp(ch), gp(J), gp(c)),
                 lambda: W(sv.h, nc, hp, 0.0, 1, gp(ch), gp(J), gp(c)),                     # host pointers
                 lambda: W(sv.h, nc, gp(U), 0.0, 1, hp, gp(J), gp(c)),
                 lambda: W(sv.h, nc, gp(U), 0.0, 1, gp(ch), hp, gp(c)),
                 lambda: W(sv.h, nc, gp(U), 0.0, 1, gp(ch), gp(J), hp),
                 lambda: W(sv.h, nc, gp(U), 0.0, 1, gp(ch), short, gp(c))]                  # one element short
        msgs = []
        for i, call in enumerate(calls):
            rc = call()
            msg = (L.altro_last_error(sv.h) or b"").decode()
            assert rc == INV and msg, (i, rc, msg)
            msgs.append(msg)
        assert "shorter" in msgs[12]
        assert W(None, nc, gp(U), 0.0, 1, gp(ch), gp(J), gp(c)) == INV and (L.altro_last_error(None) or b"").decode()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        Uh = np.zeros((B, nc, sv.N - 1, sv.m))
        assert L.altro_batch_warm_start(None, nc, Uh.ctypes.data_as(dp), 0.0, 1, None, None, None) == INV
        assert L.altro_batch_warm_start(sv.h, nc, None, 0.0, 1, None, None, None) == INV
        assert L.altro_batch_warm_start(sv.h, 0, Uh.ctypes.data_as(dp), 0.0, 1, None, None, None) == INV
        assert L.altro_batch_warm_start(sv.h, nc, Uh.ctypes.data_as(dp), -3.0, 1, None, None, None) == INV
        assert L.altro_batch_warm_start(sv.h, nc, Uh.ctypes.data_as(dp), 0.0, 7, None, None, None) == INV
        torch.cuda.synchronize()
        altro.synchronize(sv)
        assert (J == SENT).all() and (c == SENT).all() and (ch == -77).all()
        after = plane(sv)
        assert same(before[0], after[0]) and same(before[1], after[1])
        altro.solve(sv), altro.solve(tw)
        assert_twins(sv, tw, prob.x0, 1, "after the refusals")
        assert W(sv.h, nc, gp(U), 0.0, 0, gp(ch), None, None) == 0                           # chosen alone is fine
        torch.cuda.synchronize()
        assert ((H(ch) >= 0) & (H(ch) < nc)).all() and (J == SENT).all()
    finally:
        sv.close(), tw.close()


@pytest.mark.parametrize("n,m", [(12, 4), (7, 3)])
def test_state_error_before_set_dynamics(n, m):
    """8: a handle on which nothing but create has happened: ALTRO_ERR_STATE from both forms, nothing written"""
    L = altro._lib.lib()
    B, N = 3, 6
    h = C.c_void_p()
    dims = altro._lib.Dims(B, n, m, N)
    assert L.altro_batch_create(C.byref(dims), None, 0, C.byref(h)) == 0
    try:
        U = torch.zeros((B, 1, N - 1, m), dtype=torch.float64, device=dev())
        J = torch.full((B, 2), 7.0, dtype=torch.float64, device=dev())
        ch = torch.full((B,), -77, dtype=torch.int32, device=dev())
        gp = lambda t: C.c_void_p(t.data_ptr())
        assert L.altro_batch_warm_start_dev(h, 1, gp(U), 0.0, 1, gp(ch), gp(J), None) == STATE
        assert (L.altro_last_error(h) or b"").decode()
        Jh, chh = np.full((B, 2), 7.0), np.full(B, -77, dtype=np.int32)
        dp = C.POINTER(C.c_double)
        assert L.altro_batch_warm_start(h, 1, np.zeros((B, 1, N - 1, m)).ctypes.data_as(dp), 0.0, 1, chh.ctypes.data_as(C.POINTER(C.c_int32)),
                                        Jh.ctypes.data_as(dp), None) == STATE
        torch.cuda.synchronize()
        assert (J == 7.0).all() and (ch == -77).all() and (Jh == 7.0).all() and (chh == -77).all()
    finally:
        L.altro_batch_destroy(h)


# ---------------------------------------------------------------------------------------------- the closed loop
@pytest.mark.parametrize("force_wide", [False, True])
def test_tick_with_candidates_is_the_hand_written_sequence(monkeypatch, force_wide):
    """9: ExternalMPC.tick(candidates=...) over three ticks against a twin given, per tick, the setters and the shift, the
    composition (evaluate_dev with Xout, gather by the winner under the rule, set_initial_trajectory_dev), the solve and the
    read-out"""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B, n, m, N, ticks, rho = 5, 12, 4, 9, 3, 50.0
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=ticks + 1, seed=61, u_bnd=1.0)
    Xt, Ut = T(pb.Xtrack), T(pb.Utrack)
    a, b = (altro.ALTROSolver(mpc.gen_tracking_problem(pb), altro.SolverOptions(**mpc.REF_OPTS)) for _ in range(2))
    try:
        altro.solve(a), altro.solve(b)
        loop = altro.ExternalMPC(a)
        rng = np.random.default_rng(15)
        bad = 5.0 * rng.standard_normal((B, N - 1, m))        # the first tick's incumbent is far outside the bounds: a candidate wins
        altro.initial_controls(a, bad), altro.initial_controls(b, bad)
        picked = []
        for i in range(ticks):
            x = T(pb.Xtrack[:, i + 1] + 0.3 * rng.standard_normal((B, n)))
            Xr, Ur = Xt[:, i + 1:i + 1 + N].contiguous(), Ut[:, i + 1:i + N].contiguous()
            cand = torch.stack([Ur, torch.zeros_like(Ur), T(0.5 * rng.standard_normal((B, N - 1, m)))], dim=1).contiguous()
            ra = loop.tick(x, Xr, Ur, candidates=cand, candidate_rho=rho)
            with api._bracket(b):
                api._set_initial_state_dev(b, x)
                api._update_trajectory_dev(b, Xr, Ur)
                api.shift_fill(b, True, True)
            J, c, _, _ = scores(b, H(cand))
            ch = WR.select(H(J), H(c), rho, True)
            picked.append(list(ch))
            compose(b, H(cand), ch)
            with api._bracket(b):
                api.solve_async(b)
                rb = api._first_knot_dev(b, None)
            torch.cuda.synchronize()
            for ta, tb in zip(ra, rb):
                assert same(H(ta), H(tb)), i
            assert_twins(a, b, H(x), 1, ("tick", i))
        print(picked)
        assert all(w != 3 for w in picked[0]) and all(w >= 0 for p in picked for w in p)
    finally:
        a.close(), b.close()
