"""Sensitivity of the solution through the stored gains (altro_batch_solution_vjp(_dev), altro_batch_solution_jvp(_dev),
altro_batch_get_gain_factors_dev, api.solution) on both backends, against tests/solution_ref.py run in np.longdouble.

Shapes: the cases and solved handles of tests/test_covariance_gpu.py (build, make_solver), the smallest at which each path can go
wrong, N = 5 .. 8, one solve each -- 16-lane backend: (12, 4) at batch 9, (6, 3) with a cone, (6, 6), (8, 4); one-wave-per-instance
backend: (12, 12) per-knot at window 1, (17, 5), (64, 16), (30, 25) -- each "shared" and "pi", nseed = 3 (neither 1 nor a whole
wave of rows).  (30, 25) keeps no factors of Quu: its x0-only paths are checked, the others must answer UNSUPPORTED.

The accuracy bound of an output array, per instance: err = max |out - ref| / max |ref| against the long-double yardstick must
not exceed 16 x max(err of the float64 yardstick against the same ref, 2^-52).  The bound is computed here from the two numpy
runs; nothing of the device enters it."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc

import covariance_ref as CR
import evaluate_ref as ER
import solution_ref as SR
from test_covariance_gpu import IDS, OPTS, RUNS, build, make_solver
from test_warm_start_gpu import H, T, dev, everything, plane, same

pytestmark = pytest.mark.gpu
UNSUP = altro._lib.ERR_UNSUPPORTED
LD = np.longdouble
EPS = 2.0 ** -52
SENT = -12345.5
S = 3
VJP_OUT = ("gx0", "gXref", "gUref")
JVP_OUT = ("dX", "dU")
NOFAC = "wide(30,25)"


def shapes(sv, ns):
    lead = (sv.B,) if ns is None else (sv.B, ns)
    sx, su, s0 = lead + (sv.N, sv.n), lead + (sv.N - 1, sv.m), lead + (sv.n,)
    return dict(gx0=s0, gXref=sx, gUref=su, dX=sx, dU=su, gX=sx, gU=su, vx0=s0, vXref=sx, vUref=su)


def call(sv, op, ins, names, host=False, ns=S):
    """solution_vjp / solution_jvp on numpy inputs with sentinels in every output asked for: dict of numpy arrays, 'fb' too"""
    shp = shapes(sv, ns)
    fn = altro.solution_vjp if op == "vjp" else altro.solution_jvp
    if host:
        out = {k: np.full(shp[k], SENT) for k in names}
        out["fb"] = np.full(sv.B, -77, dtype=np.int32)
        got = fn(sv, **{k: (None if a is None else np.ascontiguousarray(a)) for k, a in ins.items()}, out=out)
        return {k: v for k, v in got.items()}
    out = {k: torch.full(shp[k], SENT, dtype=torch.float64, device=dev()) for k in names}
    out["fb"] = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
    got = fn(sv, **{k: (None if a is None else T(a)) for k, a in ins.items()}, out=out)
    torch.cuda.synchronize()
    return {k: H(v) for k, v in got.items()}


def seeds(cs, seed, ns=S):
    rng = np.random.default_rng(seed)
    B, N, n, m = cs.B, cs.N, cs.n, cs.m
    return NS(gX=rng.standard_normal((B, ns, N, n)), gU=rng.standard_normal((B, ns, N - 1, m)), vx0=rng.standard_normal((B, ns, n)),
              vXref=rng.standard_normal((B, ns, N, n)), vUref=rng.standard_normal((B, ns, N - 1, m)))


def policy_fb(sv, x):
    fbp = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
    altro.eval_policy(sv, T(x), fb=fbp)
    return H(fbp)


def within(got, ref, r64, valid, what):
    """check 1's rule for one array; instances without valid gains must be all NaN.  Returns the largest err / bound."""
    assert got.shape == ref.shape and not (got == SENT).any(), what
    for b in np.nonzero(valid == 0)[0]:
        assert np.isnan(got[b]).all(), (what, b, "an instance without valid gains is all NaN")
    ok = valid != 0
    assert np.isfinite(got[ok]).all(), what
    err, e64 = CR.rel_err(got[ok], ref[ok]), CR.rel_err(r64[ok], ref[ok])
    bound = 16 * np.maximum(e64, EPS)
    ratio = float((err / bound).max()) if ok.any() else 0.0
    print("%-36s err %.2e  float64 yardstick %.2e  bound %.2e  err/bound %.3f" % (what, err.max(initial=0), e64.max(initial=0), bound.min(initial=1), ratio))
    assert (err <= bound).all(), (what, err, bound)
    return ratio


@functools.lru_cache(maxsize=None)
def ran(name, pi):
    """every device call a case's tests look at, made once on one solved handle"""
    cs0, kw, _, _ = build(name, pi)
    sv, cs = make_solver(name, pi, cs0, kw)
    r = NS(cs=cs, kw=kw, pi=pi, nofac=name == NOFAC)
    try:
        r.before = everything(sv, cs.x0, len(cs.cons))
        r.Xbar, r.Ubar = plane(sv)
        r.K = altro.gains(sv)[0]
        r.valid = policy_fb(sv, r.Xbar[:, 0])
        r.sd = sd = seeds(cs, 61)
        r.e = np.ascontiguousarray(np.broadcast_to(np.eye(cs.n), (cs.B, cs.n, cs.n)))
        if r.nofac:
            r.F = None
            with pytest.raises(altro.AltroError) as e:
                api.get_gain_factors_dev(sv)
            r.fac_code = e.value.code
            r.vjp = call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), ("gx0",))
            r.vjp_host = call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), ("gx0",), host=True)
            r.jvp = call(sv, "jvp", dict(vx0=sd.vx0), JVP_OUT)
            r.jvp_host = call(sv, "jvp", dict(vx0=sd.vx0), JVP_OUT, host=True)
            r.refused = []
            for op, ins, names in (("vjp", dict(gX=sd.gX, gU=sd.gU), VJP_OUT), ("vjp", dict(gX=sd.gX), ("gXref",)), ("vjp", dict(gU=sd.gU), ("gUref",)),
                                   ("jvp", dict(vx0=sd.vx0, vXref=sd.vXref), JVP_OUT), ("jvp", dict(vUref=sd.vUref), ("dU",))):
                for host in (False, True):
                    with pytest.raises(altro.AltroError) as e:
                        call(sv, op, ins, names, host=host)
                    r.refused.append(e.value.code)
        else:
            r.F = H(api.get_gain_factors_dev(sv))
            r.vjp = call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), VJP_OUT)
            r.vjp_host = call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), VJP_OUT, host=True)
            r.jvp = call(sv, "jvp", dict(vx0=sd.vx0, vXref=sd.vXref, vUref=sd.vUref), JVP_OUT)
            r.jvp_host = call(sv, "jvp", dict(vx0=sd.vx0, vXref=sd.vXref, vUref=sd.vUref), JVP_OUT, host=True)
            # one output at a time, one seed at a time, one input at a time
            r.vjp_one = {k: call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), (k,)) for k in VJP_OUT}
            r.jvp_one = {k: call(sv, "jvp", dict(vx0=sd.vx0, vXref=sd.vXref, vUref=sd.vUref), (k,)) for k in JVP_OUT}
            r.vjp_s1 = call(sv, "vjp", dict(gX=sd.gX[:, 1], gU=sd.gU[:, 1]), VJP_OUT, ns=None)
            r.jvp_s1 = call(sv, "jvp", dict(vx0=sd.vx0[:, 1], vXref=sd.vXref[:, 1], vUref=sd.vUref[:, 1]), JVP_OUT, ns=None)
            r.vjp_gx = call(sv, "vjp", dict(gX=sd.gX), VJP_OUT)
            r.jvp_u = call(sv, "jvp", dict(vUref=sd.vUref), JVP_OUT)
        r.jvp_e = call(sv, "jvp", dict(vx0=r.e), ("dU",), ns=cs.n)
        r.after = everything(sv, cs.x0, len(cs.cons))
        if name.startswith("16"):
            r.F_host = altro.gain_factors(sv)
        # a setter that drops the stored gains
        altro.set_options(sv)
        r.dropped = call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), ("gx0",))
        r.dropped_j = call(sv, "jvp", dict(vx0=sd.vx0), JVP_OUT)
    finally:
        sv.close()
    return r


def refs(r, dtype):
    cs, sd, v = r.cs, r.sd, r.valid
    if r.nofac:
        return NS(vjp=dict(zip(VJP_OUT, SR.vjp(cs, r.K, None, v, sd.gX, sd.gU, dtype))), jvp=dict(zip(JVP_OUT, SR.jvp(cs, r.K, None, v, sd.vx0, dtype=dtype))))
    return NS(vjp=dict(zip(VJP_OUT, SR.vjp(cs, r.K, r.F, v, sd.gX, sd.gU, dtype))),
              jvp=dict(zip(JVP_OUT, SR.jvp(cs, r.K, r.F, v, sd.vx0, sd.vXref, sd.vUref, dtype))),
              vjp_gx=dict(zip(VJP_OUT, SR.vjp(cs, r.K, r.F, v, sd.gX, None, dtype))),
              jvp_u=dict(zip(JVP_OUT, SR.jvp(cs, r.K, r.F, v, None, None, sd.vUref, dtype))))


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_against_the_stored_model_yardstick(name, pi):
    """1: VJP and JVP outputs within 16 x max(float64 yardstick's error, 2^-52) of the long-double yardstick built from K, F, A,
    B and the weights; fb equals eval_policy's; instances with fb = 0 are all NaN.  (30, 25): the x0-only paths; the others
    answer UNSUPPORTED on both forms, and so does get_gain_factors_dev."""
    r = ran(name, pi)
    assert np.finfo(LD).nmant >= 63
    ref, r64 = refs(r, LD), refs(r, np.float64)
    assert (r.valid == 1).any(), r.valid
    w = []
    groups = [("vjp", r.vjp), ("jvp", r.jvp)] + ([] if r.nofac else [("vjp_gx", r.vjp_gx), ("jvp_u", r.jvp_u)])
    for g, got in groups:
        assert got["fb"].dtype == np.int32 and same(got["fb"], r.valid), (g, got["fb"], r.valid)
        for k in got:
            if k != "fb":
                w.append(within(got[k], getattr(ref, g)[k], getattr(r64, g)[k], r.valid, "%s %s %s" % (name, g, k)))
    print(name, "pi" if pi else "shared", "largest err / bound", max(w))
    if r.nofac:
        assert r.fac_code == UNSUP and r.refused == [UNSUP] * 10, (r.fac_code, r.refused)


def test_against_the_stored_model_yardstick_at_128_knots():
    """1 at the longest horizon the exact active set holds, (12, 4) at N = 128 with control and state sides in the set in every
    ASet word (tests/lane16_horizons.py stored_set_case): the (N - 1) m nseed workspace of the sweeps at its largest, 127 * 4 * 3
    doubles an instance; the same rule"""
    import lane16_horizons as lh
    name = lh.stored_set_name((12, 4), 128)
    sv, cs = make_solver(name, True, lh.stored_set_case(name), dict(shared=()))
    try:
        assert sv.N == 128 and altro.wave_cycles(sv).size != 0
        Xbar, _ = plane(sv)
        r = NS(cs=cs, kw=None, pi=True, nofac=False, K=altro.gains(sv)[0], valid=policy_fb(sv, Xbar[:, 0]), sd=seeds(cs, 62), F=H(api.get_gain_factors_dev(sv)))
        sd = r.sd
        got = dict(vjp=call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), VJP_OUT), jvp=call(sv, "jvp", dict(vx0=sd.vx0, vXref=sd.vXref, vUref=sd.vUref), JVP_OUT),
                   vjp_gx=call(sv, "vjp", dict(gX=sd.gX), VJP_OUT), jvp_u=call(sv, "jvp", dict(vUref=sd.vUref), JVP_OUT))
    finally:
        sv.close()
    assert (r.valid == 1).all(), r.valid
    ref, r64 = refs(r, LD), refs(r, np.float64)
    w = []
    for g, out in got.items():
        assert same(out["fb"], r.valid), g
        for k in out:
            if k != "fb":
                w.append(within(out[k], getattr(ref, g)[k], getattr(r64, g)[k], r.valid, "%s %s %s" % (name, g, k)))
    print(name, "largest err / bound", max(w))


@pytest.mark.parametrize("name,pi", [q for q in RUNS if q[0] != NOFAC], ids=[i for q, i in zip(RUNS, IDS) if q[0] != NOFAC])
def test_adjoint_identity(name, pi):
    """2: <gX, dX> + <gU, dU> against <gx0, vx0> + <gXref, vXref> + <gUref, vUref> per (instance, seed); the gap relative to the
    sum of the absolute terms within 16 x max(the same gap of the float64 numpy yardstick, 2^-52)"""
    r = ran(name, pi)
    sd, ok = r.sd, r.valid != 0

    def gap(vj, jv):
        t = lambda a: np.asarray(a, dtype=LD).reshape(r.cs.B, S, -1)
        lhs = [t(sd.gX) * t(jv["dX"]), t(sd.gU) * t(jv["dU"])]
        rhs = [t(vj["gx0"]) * t(sd.vx0), t(vj["gXref"]) * t(sd.vXref), t(vj["gUref"]) * t(sd.vUref)]
        diff = sum(a.sum(axis=2) for a in lhs) - sum(a.sum(axis=2) for a in rhs)
        return (np.abs(diff) / sum(np.abs(a).sum(axis=2) for a in lhs + rhs)).astype(np.float64)

    r64 = refs(r, np.float64)
    g, g64 = gap(r.vjp, r.jvp)[ok], gap(r64.vjp, r64.jvp)[ok]
    bound = 16 * np.maximum(g64, EPS)
    print(name, "adjoint gap", g.max(), "float64 yardstick", g64.max(), "gap / bound", (g / bound).max())
    assert (g <= bound).all(), (g, bound)


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_the_gain_is_the_first_knot_sensitivity(name, pi):
    """3: the JVP with vx0 = e_j and nothing else gives dU[:, j, 0, :] == K_0[:, :, j] exactly"""
    r = ran(name, pi)
    ok = r.valid != 0
    dU = r.jvp_e["dU"]                                       # (B, n, N-1, m)
    assert np.array_equal(dU[ok][:, :, 0, :], np.swapaxes(r.K[ok][:, 0], -1, -2))
    assert np.isnan(dU[~ok]).all()


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_twins_rows_and_null_outputs(name, pi):
    """5: host and _dev forms write the same bytes; row (b, s) equals the nseed = 1 call; an output does not depend on which
    others are NULL; get_gain_factors_dev equals gain_factors byte for byte on the 16-lane cases"""
    r = ran(name, pi)
    for a, b in ((r.vjp, r.vjp_host), (r.jvp, r.jvp_host)):
        assert set(a) == set(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and same(a[k], b[k]), k
    if not r.nofac:
        for k in VJP_OUT:
            assert same(r.vjp_one[k][k], r.vjp[k]) and same(r.vjp_s1[k], r.vjp[k][:, 1]), k
        for k in JVP_OUT:
            assert same(r.jvp_one[k][k], r.jvp[k]) and same(r.jvp_s1[k], r.jvp[k][:, 1]), k
    if name.startswith("16"):
        assert same(r.F, r.F_host)
    elif not r.nofac:     # the convention of the host getter: nothing above the diagonal, positive reciprocals on it
        iu = np.triu_indices(r.cs.m, 1)
        assert (r.F[..., iu[0], iu[1]] == 0).all() and (np.einsum("bkaa->bka", r.F)[r.valid != 0] > 0).all()


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_nothing_the_library_owns_changes(name, pi):
    """5: everything a caller can read is byte-identical before and after the calls (the refused ones included); after
    altro_batch_set_options (gains dropped) fb = 0 and the rows are NaN"""
    r = ran(name, pi)
    for k in r.before:
        assert np.array_equal(r.before[k], r.after[k], equal_nan=True), k
    for got in (r.dropped, r.dropped_j):
        assert (got["fb"] == 0).all()
        for k in got:
            assert k == "fb" or np.isnan(got[k]).all(), k


@pytest.mark.parametrize("name,pi", [("16-box(12,4)", True), ("16-soc(6,3)", True), ("wide(17,5)", True), ("wide-ltv(12,12)", False)])
def test_batch_one_handle_and_the_next_solve(name, pi):
    """5: instance b on a solved batch-1 handle holding its rows of data (same trajectory, same gains: checked first) gets the
    bytes it gets inside the batch; the next solve of a handle that made the calls is bit-identical to that of a handle that
    never did"""
    r = ran(name, pi)
    cs, sd = r.cs, r.sd
    if not name.startswith("wide-ltv"):
        for b in range(cs.B):
            sub = ER.sub_case(cs, b)
            sv, _ = make_solver(name, pi, sub, {})
            try:
                Xb, Ub = plane(sv)
                assert same(Xb, r.Xbar[b:b + 1]) and same(Ub, r.Ubar[b:b + 1]) and same(altro.gains(sv)[0], r.K[b:b + 1]), ("the solves differ", b)
                v = call(sv, "vjp", dict(gX=sd.gX[b:b + 1], gU=sd.gU[b:b + 1]), VJP_OUT)
                j = call(sv, "jvp", dict(vx0=sd.vx0[b:b + 1], vXref=sd.vXref[b:b + 1], vUref=sd.vUref[b:b + 1]), JVP_OUT)
            finally:
                sv.close()
            for got, full in ((v, r.vjp), (j, r.jvp)):
                for k in got:
                    assert same(got[k], full[k][b:b + 1]), (b, k)
    cs0, kw, _, _ = build(name, pi)
    a, csa = make_solver(name, pi, cs0, kw)
    cs1, kw1, _, _ = build(name, pi)
    t, _ = make_solver(name, pi, cs1, kw1)
    try:
        call(a, "vjp", dict(gX=sd.gX, gU=sd.gU), VJP_OUT)
        call(a, "jvp", dict(vx0=sd.vx0, vXref=sd.vXref, vUref=sd.vUref), JVP_OUT)
        x1 = csa.x0 + 0.05
        for s in (a, t):
            altro.set_initial_state(s, x1)
            altro.solve(s)
        ea, et = everything(a, x1, len(csa.cons)), everything(t, x1, len(csa.cons))
        for k in ea:
            assert np.array_equal(ea[k], et[k], equal_nan=True), k
    finally:
        a.close()
        t.close()


# ------------------------------------------------------------------ the true solution map where it is unambiguous
WIDE_OPEN = 1e6


def open_case(name):
    """(12, 4) on the 16-lane backend and (17, 5) on the one-wave-per-instance backend with the BOX opened so wide that no side
    is ever active (it stays, so the code path is the same) and no rows: the solution is affine in (x0, Xref, Uref)"""
    if name == "16-box(12,4)":
        return ER.add_box(ER.make_case(9, 12, 4, 6, 11), WIDE_OPEN)
    return ER.add_box(ER.make_case(3, 17, 5, 5, 25), WIDE_OPEN)


@functools.lru_cache(maxsize=None)
def ran_open(name):
    cs = open_case(name)
    sv = altro.ALTROSolver(ER.to_problem(altro, cs, shared=("cost", "box")), altro.SolverOptions(**OPTS))
    r = NS(cs=cs, sd=seeds(cs, 71))
    try:
        altro.solve(sv)
        sd = r.sd
        r.vjp = call(sv, "vjp", dict(gX=sd.gX, gU=sd.gU), VJP_OUT)
        r.jvp = call(sv, "jvp", dict(vx0=sd.vx0, vXref=sd.vXref, vUref=sd.vUref), JVP_OUT)
        # api.solution: the gradient of a random linear functional of (X, U)
        x0, Xr, Ur = (T(a).requires_grad_() for a in (cs.x0, cs.Xref, cs.Uref))
        X, U = altro.solution(sv, x0, Xr, Ur)
        r.cX, r.cU = sd.gX[:, 0], sd.gU[:, 0]
        loss = (T(r.cX) * X).sum() + (T(r.cU) * U).sum()
        r.grads = [H(g) for g in torch.autograd.grad(loss, (x0, Xr, Ur))]
        r.XU = (H(X.detach()), H(U.detach()))
        r.plane = plane(sv)
    finally:
        sv.close()
    r.J = SR.dense_jacobian(cs, LD)
    K64, F64 = SR.riccati(cs, np.float64)
    one = np.ones(cs.B, dtype=np.int32)
    r.v64 = dict(zip(VJP_OUT, SR.vjp(cs, K64, F64, one, r.sd.gX, r.sd.gU)))
    r.j64 = dict(zip(JVP_OUT, SR.jvp(cs, K64, F64, one, r.sd.vx0, r.sd.vXref, r.sd.vUref)))
    return r


@pytest.mark.parametrize("name", ["16-box(12,4)", "wide(17,5)"])
def test_the_true_solution_map(name):
    """4: device JVP and VJP against the exact Jacobian action of the affine solution map, from a dense KKT solve in
    np.longdouble built from A, B and the weights alone; the float64 yardstick of the 16 x rule is a float64 Riccati recursion
    on the same data.  This pins the signs and the -W scalings to the problem, not to the implementation."""
    r = ran_open(name)
    cs, sd = r.cs, r.sd
    one = np.ones(cs.B, dtype=np.int32)
    assert same(r.vjp["fb"], one) and same(r.jvp["fb"], one)
    dv = dict(zip(VJP_OUT, SR.dense_vjp(r.J, cs, sd.gX, sd.gU)))
    dj = dict(zip(JVP_OUT, SR.dense_jvp(r.J, cs, sd.vx0, sd.vXref, sd.vUref)))
    for k in VJP_OUT:
        within(r.vjp[k], dv[k], r.v64[k], one, "%s dense vjp %s" % (name, k))
    for k in JVP_OUT:
        within(r.jvp[k], dj[k], r.j64[k], one, "%s dense jvp %s" % (name, k))


@pytest.mark.parametrize("name", ["16-box(12,4)", "wide(17,5)"])
def test_api_solution_gradients(name):
    """6: torch.autograd.grad of a random linear functional of api.solution's (X, U) equals the dense reference of check 4 under
    the same rule; the forward returns the trajectory the solver holds"""
    r = ran_open(name)
    cs = r.cs
    assert same(r.XU[0], r.plane[0]) and same(r.XU[1], r.plane[1])
    one = np.ones(cs.B, dtype=np.int32)
    dv = SR.dense_vjp(r.J, cs, r.cX[:, None], r.cU[:, None])
    for k, g, d in zip(VJP_OUT, r.grads, dv):
        within(g[:, None], d, r.v64[k][:, :1], one, "%s api.solution %s" % (name, k))


@pytest.mark.parametrize("name", ["16-box(12,4)", "wide(17,5)"])
def test_c_abi_refuses_before_anything_is_enqueued(name):
    """the argument rules of the header at the C-ABI itself (the Python wrappers stop most of them earlier): INVALID_ARG with the
    handle unchanged and usable; a handle without a reference answers STATE as altro_batch_evaluate_dev does"""
    import ctypes as C
    INV, STATE = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_STATE
    cs = open_case(name)
    prob = ER.to_problem(altro, cs, shared=("cost", "box"))
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**OPTS))
    try:
        altro.solve(sv)
        L, h, B, N, n, m = sv._L, sv.h, sv.B, sv.N, sv.n, sv.m
        before = everything(sv, cs.x0, len(cs.cons))
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev())
        gX, gU, v0 = z(B, 1, N, n), z(B, 1, N - 1, m), z(B, 1, n)
        p = lambda t: None if t is None else t.data_ptr()
        out = lambda **kw: C.byref(altro._lib.SensOut(**{k: p(kw.get(k)) for k in VJP_OUT}))
        hx = np.zeros((B, 1, N, n))
        calls = [
            (L.altro_batch_solution_vjp_dev, (None, 1, p(gX), p(gU), out(gx0=v0), None)),
            (L.altro_batch_solution_vjp_dev, (h, 0, p(gX), p(gU), out(gx0=v0), None)),
            (L.altro_batch_solution_vjp_dev, (h, 1, None, None, out(gx0=v0), None)),
            (L.altro_batch_solution_vjp_dev, (h, 1, p(gX), p(gU), None, None)),
            (L.altro_batch_solution_vjp_dev, (h, 1, p(gX), p(gU), out(), None)),
            (L.altro_batch_solution_vjp_dev, (h, 1, hx.ctypes.data, p(gU), out(gx0=v0), None)),          # a host pointer
            (L.altro_batch_solution_jvp_dev, (None, 1, p(v0), None, None, p(gX), None, None)),
            (L.altro_batch_solution_jvp_dev, (h, -1, p(v0), None, None, p(gX), None, None)),
            (L.altro_batch_solution_jvp_dev, (h, 1, None, None, None, p(gX), p(gU), None)),
            (L.altro_batch_solution_jvp_dev, (h, 1, p(v0), p(gX), p(gU), None, None, None)),
            (L.altro_batch_solution_jvp_dev, (h, 1, p(v0), None, None, hx.ctypes.data, None, None)),
            (L.altro_batch_get_gain_factors_dev, (None, p(gU))),
            (L.altro_batch_get_gain_factors_dev, (h, None)),
            (L.altro_batch_solution_vjp, (h, 1, None, None, out(gx0=v0), None)),
            (L.altro_batch_solution_jvp, (h, 0, None, None, None, None, None, None)),
        ]
        for fn, args in calls:
            assert fn(*args) == INV, (fn.__name__, args[1:2])
        after = everything(sv, cs.x0, len(cs.cons))
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
        torch.cuda.synchronize()
        assert L.altro_batch_solution_vjp_dev(h, 1, p(gX), p(gU), out(gx0=v0), None) == 0      # still usable
    finally:
        sv.close()
    # no reference yet: STATE, as altro_batch_evaluate_dev
    d = altro._lib.Dims(cs.B, cs.n, cs.m, cs.N)
    o = altro.SolverOptions(**OPTS)
    h2 = C.c_void_p()
    Lb = altro._lib.lib()
    assert Lb.altro_batch_create(C.byref(d), C.byref(o), 0, C.byref(h2)) == 0
    try:
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev())
        gX, v0 = z(cs.B, 1, cs.N, cs.n), z(cs.B, 1, cs.n)
        st = altro._lib.SensOut(gx0=v0.data_ptr())
        assert Lb.altro_batch_solution_vjp_dev(h2, 1, gX.data_ptr(), None, C.byref(st), None) == STATE
        assert Lb.altro_batch_evaluate_dev(h2, 1, None, None, None, v0.data_ptr(), None, None, None) == STATE
        assert Lb.altro_batch_solution_jvp_dev(h2, 1, v0.data_ptr(), None, None, gX.data_ptr(), None, None) == STATE
    finally:
        Lb.altro_batch_destroy(h2)


@pytest.mark.parametrize("force_wide", [False, True])
def test_an_output_one_double_short_is_refused(monkeypatch, force_wide):
    """both `_dev` forms with one output one double short of its extent (gXref of the VJP, dU of the JVP; the last doubles of the
    tensor's own allocation, hipMemGetAddressRange): INVALID_ARG with "shorter" in the message, the sentinel in every output
    untouched, and the next solve equals a twin handle's.  (n, m) = (6, 3) at batch 5, N = 9: the smallest shape of
    tests/test_evaluate_gpu.py, on the backend it picks and on the one-wave-per-instance backend"""
    import ctypes as C
    import test_evaluate_gpu as TE
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    INV = altro._lib.ERR_INVALID_ARG
    prob = mpc.gen_tracking_problem(TE.random_linear(5, 6, 3, 41))
    sv, tw = (altro.ALTROSolver(prob, altro.SolverOptions(**mpc.REF_OPTS)) for _ in range(2))
    try:
        altro.solve(sv), altro.solve(tw)
        L, h, B, N, n, m = sv._L, sv.h, sv.B, sv.N, sv.n, sv.m
        full = lambda *s: torch.full(s, SENT, dtype=torch.float64, device=dev())
        gX, gU, v0 = T(np.ones((B, 1, N, n))), T(np.ones((B, 1, N - 1, m))), T(np.ones((B, 1, n)))
        o0, oX, oU = full(B, 1, n), full(B, 1, N, n), full(B, 1, N - 1, m)
        fb = torch.full((B,), -77, dtype=torch.int32, device=dev())
        paths = altro._lib.hip_runtimes()
        assert len(paths) == 1, paths
        rt = C.CDLL(paths[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]

        def short(t):
            base, size = C.c_void_p(), C.c_size_t()
            assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), C.c_void_p(t.data_ptr())) == 0
            return base.value + size.value - (t.numel() * 8 - 8)             # the last numel - 1 doubles of t's allocation

        p = lambda t: t.data_ptr()
        out = altro._lib.SensOut(gx0=p(o0), gXref=short(oX), gUref=p(oU))
        calls = [lambda: L.altro_batch_solution_vjp_dev(h, 1, p(gX), p(gU), C.byref(out), p(fb)),
                 lambda: L.altro_batch_solution_jvp_dev(h, 1, p(v0), p(gX), p(gU), p(oX), short(oU), p(fb))]
        for i, call_ in enumerate(calls):
            rc = call_()
            msg = (L.altro_last_error(h) or b"").decode()
            assert rc == INV and "shorter" in msg, (i, rc, msg)
        torch.cuda.synchronize()
        altro.synchronize(sv)
        for t in (o0, oX, oU):
            assert (t == SENT).all()
        assert (fb == -77).all()
        assert L.altro_batch_solution_jvp_dev(h, 1, p(v0), p(gX), p(gU), p(oX), p(oU), p(fb)) == 0     # the whole dU is fine
        altro.solve(sv), altro.solve(tw)
        ea, eb = TE.everything(sv, prob.x0), TE.everything(tw, prob.x0)
        for k in ea:
            assert np.array_equal(ea[k], eb[k], equal_nan=True), k
        assert (oU != SENT).any()
    finally:
        sv.close(), tw.close()


def test_api_solution_with_an_invalid_instance():
    """6: with instances whose stored pass was regularised (one iteration with bp_reg_initial > 0 on the one-wave-per-instance
    backend: the regularisation has not decayed to zero yet when the solve stops) the forward raises; with invalid="zero" their
    gradient rows are zero"""
    cs = open_case("wide(17,5)")
    opts = dict(OPTS, bp_reg_initial=1e-3, iterations=1, iterations_inner=1, iterations_outer=1)
    sv = altro.ALTROSolver(ER.to_problem(altro, cs, shared=("cost", "box")), altro.SolverOptions(**opts))
    try:
        x0, Xr, Ur = (T(a).requires_grad_() for a in (cs.x0, cs.Xref, cs.Uref))
        with pytest.raises(altro.AltroError):
            altro.solution(sv, x0, Xr, Ur)
        X, U = altro.solution(sv, x0, Xr, Ur, invalid="zero")
        fb = altro.solution_jvp(sv, vx0=T(cs.x0), out=("dU",))["fb"]
        assert (H(fb) == 0).all()
        grads = torch.autograd.grad(X.sum() + U.sum(), (x0, Xr, Ur))
        for g in grads:
            assert same(H(g), np.zeros(tuple(g.shape)))
    finally:
        sv.close()
