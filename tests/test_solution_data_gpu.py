"""Sensitivity of the solution with respect to cost weights, box bounds and dynamics (altro_batch_solution_vjp_data(_dev),
altro_batch_get_gain_active_set(_dev), api.mpc_layer) on both backends, against tests/solution_data_ref.py run in
np.longdouble from the device's own gains, factors, active set, trajectory and duals.

Shapes: the box-only cases and solved handles of tests/test_covariance_gpu.py (build, make_solver) -- 16-lane backend (12, 4) at
batch 9, (6, 6), (8, 4); one-wave-per-instance backend (64, 16) -- each "shared" and "pi", nseed = 3; a box-only (12, 4) with
per-knot dynamics through TrackMPC at window 1 (one-wave-per-instance backend, time-varying blocks); and "tight" variants of
(12, 4) and (64, 16) whose state bounds reach the terminal knot and bind, instance 0 of each with bounds it never reaches (an empty
set); every box case once more with the box opened to 1e6; and the stored set beyond its first word: "tight" (12, 4) and (6, 6)
at N = 17, 33 and 128 (tests/lane16_horizons.py stored_set_case: k_sens_data16 and the getter kernel read ASet word k >> 4, and at
N <= 16 word 0 is the only one there is), control and state sides in the set at knots >= 16 and, at N = 128, at knots >= 112.
Every run but those at N = 128 meets the dense adjoint (check 4).  The refusals are checked on (6, 3) with a cone, (17, 5)
with LINEAR rows, (30, 25) and a 16-lane (12, 4) at N = 130.

The accuracy bound of an output array, per instance: err = max |out - ref| / max |ref| against the long-double yardstick must
not exceed 16 x max(err of the float64 yardstick against the same ref, 2^-52).  The bound is computed here from the two numpy
runs; nothing of the device enters it."""
import ctypes as C
import functools
import math
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api

import covariance_ref as CR
import lane16_horizons as lh
import evaluate_ref as ER
import solution_data_ref as DR
import solution_ref as SR
from test_covariance_gpu import OPTS, build, make_solver
from test_solution_sens_gpu import seeds
from test_warm_start_gpu import H, T, dev, everything, plane, same

pytestmark = pytest.mark.gpu
INV, UNSUP = altro._lib.ERR_INVALID_ARG, altro._lib.ERR_UNSUPPORTED
LD = np.longdouble
EPS = 2.0 ** -52
SENT = -12345.5
S = 3
OUTS = DR.OUTS
WEIGHTS = ("gQ", "gQf", "gR")
TIGHT = ["16-box(12,4)-tight", "wide(64,16)-tight"]
LTV = "wide-ltv-box(12,4)"
BOX = ["16-box(12,4)", "16(6,6)", "16(8,4)", "wide(64,16)"]
OPEN = [s + "-open" for s in BOX]      # the same cases with the box opened to 1e6: it stays, no side is ever in the set
LONG = list(lh.STORED_SET_CASES)       # the stored set beyond ASet word 0: N = 17, 33, 128
RUNS = [(s, pi) for s in BOX for pi in (False, True)] + [(s, True) for s in TIGHT] + [(LTV, True)] + [(s, True) for s in OPEN] + [(s, True) for s in LONG]
IDS = [s + ("-pi" if pi else "-shared") for s, pi in RUNS]
TIES = [("16-box(12,4)-tight", True), ("16(6,6)", True), ("wide(64,16)-tight", True), (LTV, True)]      # both backends, sides of every kind, per-knot dynamics


def build_data(name, pi):
    """(Case, to_problem keywords)"""
    if name == "16-box(12,4)-tight":
        cs = ER.make_case(9, 12, 4, 6, 11, per_instance_cost=True)
        ub = np.concatenate([np.full((1, 4), 50.0), 0.2 + 0.05 * np.arange(8)[:, None] * np.ones((8, 4))])   # instance 0: never reached
        cs = ER.add_box(cs, ub, x_bnd=0.9, k0=0, k1=5)
        cs.cons[0].zmin[0, :12][np.isfinite(cs.cons[0].zmin[0, :12])] = -50.0
        cs.cons[0].zmax[0, :12][np.isfinite(cs.cons[0].zmax[0, :12])] = 50.0
        return cs, dict(shared=())
    if name == "wide(64,16)-tight":
        cs = ER.make_case(4, 64, 16, 5, 28, per_instance_cost=True)
        ub = np.concatenate([np.full((1, 16), 50.0), 0.3 + 0.1 * np.arange(3)[:, None] * np.ones((3, 16))])   # instance 0: never reached
        cs = ER.add_box(cs, ub, x_bnd=1.2, k0=0, k1=4)
        cs.cons[0].zmin[0, :64][np.isfinite(cs.cons[0].zmin[0, :64])] = -50.0
        cs.cons[0].zmax[0, :64][np.isfinite(cs.cons[0].zmax[0, :64])] = 50.0
        return cs, dict(shared=())
    if name == LTV:
        cs = ER.add_box(ER.make_case(3, 12, 4, 6, 33, per_knot_dyn=True, per_instance_cost=True), 0.5 + np.random.default_rng(34).random((3, 4)))
        return cs, dict(per_knot_dyn=True, shared=())
    if name in LONG:
        return lh.stored_set_case(name), dict(shared=())
    if name in OPEN:
        cs, kw, _, _ = build(name[:-len("-open")], pi)
        box = cs.cons[0]
        box.zmin[np.isfinite(box.zmin)], box.zmax[np.isfinite(box.zmax)] = -1e6, 1e6
        return cs, kw
    cs, kw, _, _ = build(name, pi)
    return cs, kw


def shapes(sv, ns, per_knot):
    lead = (sv.B,) if ns is None else (sv.B, ns)
    n, m, kn = sv.n, sv.m, ((sv.N - 1,) if per_knot else ())
    return dict(gQ=lead + (n,), gQf=lead + (n,), gR=lead + (m,), gzmin=lead + (n + m,), gzmax=lead + (n + m,), gA=lead + kn + (n, n),
                gB=lead + kn + (n, m), gf=lead + kn + (n,))


def call(sv, gX, gU, names=OUTS, per_knot=False, host=False, ns=S):
    """solution_vjp_data on numpy inputs with sentinels in every output asked for: dict of numpy arrays, 'fb' too"""
    shp = shapes(sv, ns, per_knot)
    cm = lambda k, a: a.swapaxes(-1, -2) if k in ("gA", "gB") else a      # column-major blocks
    ins = [None if a is None else np.ascontiguousarray(a) for a in (gX, gU)]
    if host:
        out = {k: cm(k, np.full(shp[k][:-2] + shp[k][:-3:-1] if k in ("gA", "gB") else shp[k], SENT)) for k in names}
        out["fb"] = np.full(sv.B, -77, dtype=np.int32)
        got = altro.solution_vjp_data(sv, ins[0], ins[1], per_knot=per_knot, out=out)
        return {k: np.ascontiguousarray(v) for k, v in got.items()}
    full = lambda s: torch.full(s, SENT, dtype=torch.float64, device=dev())
    out = {k: cm(k, full(shp[k][:-2] + shp[k][:-3:-1] if k in ("gA", "gB") else shp[k])) for k in names}
    out["fb"] = torch.full((sv.B,), -77, dtype=torch.int32, device=dev())
    got = altro.solution_vjp_data(sv, *(None if a is None else T(a) for a in ins), per_knot=per_knot, out=out)
    torch.cuda.synchronize()
    return {k: np.ascontiguousarray(H(v)) for k, v in got.items()}


def getter(sv, host=False):
    if host:
        return altro.gain_active_set(sv, "numpy")
    g = altro.gain_active_set(sv)
    torch.cuda.synchronize()
    return {k: H(v) for k, v in g.items()}


def within(got, ref, r64, valid, what):
    """the 16x rule for one array; instances without valid gains must be all NaN.  Returns the largest err / bound."""
    assert got.shape == ref.shape and not (got == SENT).any(), what
    for b in np.nonzero(valid == 0)[0]:
        assert np.isnan(got[b]).all(), (what, b, "an instance without valid gains is all NaN")
    ok = valid != 0
    assert np.isfinite(got[ok]).all(), what
    err, e64 = CR.rel_err(got[ok], ref[ok]), CR.rel_err(r64[ok], ref[ok])
    bound = 16 * np.maximum(e64, EPS)
    ratio = float((err / bound).max()) if ok.any() else 0.0
    print("%-40s err %.2e  float64 yardstick %.2e  err/bound %.3f" % (what, err.max(initial=0), e64.max(initial=0), ratio))
    assert (err <= bound).all(), (what, err, bound)
    return ratio


def tie_calls(sv, cs):
    """solution_jvp on tangents of the reference alone and solution_vjp_data on the seed that JVP forms from them, g = -(w v) with
    the product rounded (sensitivity.h's sens_negw): both calls then run the same two sweeps on the same numbers"""
    sd = seeds(cs, 94)
    wx, wu = SR.weights(cs, np.float64)
    gX, gU = -(wx[:, None] * sd.vXref), -(wu[:, None, None] * sd.vUref)
    jv = altro.solution_jvp(sv, vXref=T(sd.vXref), vUref=T(sd.vUref))
    torch.cuda.synchronize()
    return NS(jvp={k: H(v) for k, v in jv.items()}, data=call(sv, gX, gU, OUTS[:5]))


@functools.lru_cache(maxsize=None)
def ran(name, pi):
    """every device call a case's tests look at, made once on one solved handle"""
    cs0, kw = build_data(name, pi)
    sv, cs = make_solver(name, pi, cs0, kw)
    r = NS(cs=cs, kw=kw, pi=pi)
    try:
        r.before = everything(sv, cs.x0, len(cs.cons))
        r.X, r.U = plane(sv)
        r.K = altro.gains(sv)[0]
        r.F = H(api.get_gain_factors_dev(sv))
        r.duals, r.mu = altro.get_duals(sv, 0), altro.penalty(sv)
        r.sd = sd = seeds(cs, 91)
        r.vjp = {k: H(v) for k, v in altro.solution_vjp(sv, T(sd.gX), T(sd.gU)).items()}
        r.g, r.g_host = getter(sv), getter(sv, host=True)
        r.all0, r.all1 = call(sv, sd.gX, sd.gU), call(sv, sd.gX, sd.gU, per_knot=True)
        r.host0, r.host1 = call(sv, sd.gX, sd.gU, host=True), call(sv, sd.gX, sd.gU, per_knot=True, host=True)
        r.one = {k: call(sv, sd.gX, sd.gU, (k,), per_knot=True) for k in OUTS}
        r.w = call(sv, sd.gX, sd.gU, WEIGHTS)
        r.s1 = call(sv, sd.gX[:, 1], sd.gU[:, 1], ns=None)
        r.gx = call(sv, sd.gX, None)
        if (name, pi) in TIES:
            r.tie = tie_calls(sv, cs)
        r.after = everything(sv, cs.x0, len(cs.cons))
        altro.set_options(sv)      # a setter that drops the stored gains
        r.dropped, r.g_dropped = call(sv, sd.gX, sd.gU), getter(sv)
    finally:
        sv.close()
    return r


def refs(r, dtype, per_knot, gU=True):
    cs, sd = r.cs, r.sd
    lam = DR.costate(cs, r.X, r.U, r.duals, r.mu, dtype)
    return DR.sweep(cs, r.K, r.F, r.g["codes"], r.g["mu_pass"], r.g["fb"], r.X, r.U, lam, sd.gX, sd.gU if gU else None, per_knot, dtype)


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_getter(name, pi):
    """1: K and Quu recomputed from codes and mu_pass by a Riccati recursion in long double equal get_gains and the stored factors;
    mu_pass equals the penalty held; the host and _dev forms give the same bytes; the tight cases reach every kind of side"""
    r = ran(name, pi)
    cs, g = r.cs, r.g
    n, cd = cs.n, g["codes"]
    assert np.finfo(LD).nmant >= 63
    assert g["fb"].dtype == np.int32 and (g["fb"] == 1).all() and same(g["fb"], r.vjp["fb"]), g["fb"]
    assert same(g["mu_pass"], r.mu) and cd.dtype == np.uint8 and (cd <= 3).all() and (cd[:, -1, n:] == 0).all()
    for k in g:
        assert g[k].dtype == r.g_host[k].dtype and same(g[k], r.g_host[k]), k
    K, Quu = DR.riccati_codes(cs, cd, g["mu_pass"], LD)
    K64, Quu64 = DR.riccati_codes(cs, cd, g["mu_pass"], np.float64)
    w = [within(r.K, K, K64, g["fb"], name + " K from codes"), within(DR.quu_of_factors(r.F, np.float64), Quu, Quu64, g["fb"], name + " Quu from codes")]
    print(name, "getter: largest err / bound", max(w), "sides in the set", int((cd != 0).sum()))
    if name in TIGHT:
        assert (cd[:, :-1, n:] & 1).any() and (cd[:, :-1, n:] & 2).any(), "an upper and a lower control side"
        assert (cd[:, 1:-1, :n] != 0).any() and (cd[:, -1, :n] != 0).any(), "a state side at an interior knot and at knot N-1"
        assert (cd[0] == 0).all() and (cd[1:] != 0).any(), "one instance with an empty set"
    if name in LONG:
        lh.assert_late_sides(cd, n, cs.N)      # sides of every kind in the words the kernels reach with k >> 4 > 0
    if name in OPEN:
        assert (cd == 0).all()
    assert (r.g_dropped["fb"] == 0).all() and (r.g_dropped["codes"] == 0).all() and np.isnan(r.g_dropped["mu_pass"]).all()


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_against_the_yardstick(name, pi):
    """2: every output, summed and per knot, within the rule of the long-double sweeps built from the device's own K, F, codes,
    trajectory and duals; the per-knot blocks sum to the summed output within the rule"""
    r = ran(name, pi)
    w = []
    for pk, got in ((False, r.all0), (True, r.all1)):
        ref, r64 = refs(r, LD, pk), refs(r, np.float64, pk)
        assert same(got["fb"], r.g["fb"])
        for k in OUTS:
            w.append(within(got[k], ref[k], r64[k], r.g["fb"], "%s %s per_knot=%d" % (name, k, pk)))
    ref, r64 = refs(r, LD, False), refs(r, np.float64, False)
    for k in ("gA", "gB", "gf"):
        w.append(within(r.all1[k].astype(LD).sum(axis=2).astype(np.float64), ref[k], r64[k], r.g["fb"], name + " sum of the per-knot " + k))
    ref, r64 = refs(r, LD, False, gU=False), refs(r, np.float64, False, gU=False)
    for k in OUTS:
        w.append(within(r.gx[k], ref[k], r64[k], r.g["fb"], name + " gU = NULL " + k))
    print(name, "pi" if pi else "shared", "largest err / bound", max(w))


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_consistency_with_solution_vjp(name, pi):
    """3: dlam_0 is observable: gf at per_knot = 1, knot 0, is dlam_1 and gx0 of solution_vjp is s_0 = dlam_0, so
    gX_0 + hz_0 xi_0 + A_0' gf_0 = gx0 (xi_0 = 0); and the u-stationarity gU_k + hz_u nu_k + B_k' gf_k = 0 with nu = -gUref / (dt R).
    The gaps relative to the sum of the absolute terms, within 16 x max(the same gap of the float64 yardstick, 2^-52)"""
    r = ran(name, pi)
    cs, sd, ok = r.cs, r.sd, r.g["fb"] != 0
    _, hu = DR.hz_of(DR.theta_of(cs), cs, r.g["codes"], r.g["mu_pass"], LD)
    wu = LD(cs.dt) * cs.R.astype(LD)
    t = lambda a: np.asarray(a, dtype=LD)

    def gaps(gf, gx0, nu):
        Af = np.einsum("bij,bsi->bsj", t(cs.A[:, 0]), gf[:, :, 0])
        g0 = np.abs(t(sd.gX[:, :, 0]) + Af - gx0).max(axis=2) / (np.abs(t(sd.gX[:, :, 0])) + np.abs(Af) + np.abs(gx0)).max(axis=2)
        Bf = np.einsum("bkia,bski->bska", t(cs.Bm), gf)
        hn = hu[:, None] * nu
        gu = np.abs(t(sd.gU) + hn + Bf).max(axis=(2, 3)) / (np.abs(t(sd.gU)) + np.abs(hn) + np.abs(Bf)).max(axis=(2, 3))
        return g0.astype(np.float64)[ok], gu.astype(np.float64)[ok]

    y = refs(r, np.float64, True)
    got = gaps(t(r.all1["gf"]), t(r.vjp["gx0"]), -t(r.vjp["gUref"]) / wu[:, None, None])
    y64 = gaps(t(y["dlam"][:, :, 1:]), t(y["s0"]), t(y["nu"]))
    for g, g6, what in zip(got, y64, ("dlam_0", "u-stationarity")):
        bound = 16 * np.maximum(g6, EPS)
        print(name, what, "gap", g.max(), "float64 yardstick", g6.max(), "gap / bound", (g / bound).max())
        assert (g <= bound).all(), (what, g, bound)


DENSE = [(q, i) for q, i in zip(RUNS, IDS) if not (q[0] in LONG and lh.STORED_SET_CASES[q[0]][1] == 128)]


@pytest.mark.parametrize("name,pi", [q for q, _ in DENSE], ids=[i for _, i in DENSE])
def test_the_dense_adjoint_at_the_held_trajectory(name, pi):
    """4: every output of every run -- the box cases as they are and with the box opened to 1e6, the tight cases, the per-knot
    case, the long horizons N = 17 and 33 -- against the dense adjoint (one KKT solve in long double, no sweep, no gain of the
    device) at the trajectory, costate, set and penalty the handle holds; the float64 yardstick of the rule is the sweeps in
    float64 on a float64 Riccati recursion from the same codes.
    N = 128 is left out: the KKT matrix has 127 (2 n + m) rows, 3556 at (12, 4), and Gaussian elimination in long double
    (numpy's LAPACK has none) takes minutes; 448 rows (N = 17) take 1 s and 896 (N = 33) 8 s for the batch of two, so at the
    long horizons ONE solve serves both forms: the summed gA, gB, gf are the per-knot blocks added in long double."""
    r = ran(name, pi)
    cs, sd, g = r.cs, r.sd, r.g
    lam = DR.costate(cs, r.X, r.U, r.duals, r.mu, LD)
    K64, Quu64 = DR.riccati_codes(cs, g["codes"], g["mu_pass"], np.float64)
    w = []
    knots = None
    for pk, got in ((True, r.all1), (False, r.all0)):
        if name in LONG and not pk:
            ref = {k: (knots[k].sum(axis=2) if k in ("gA", "gB", "gf") else knots[k]) for k in OUTS}
        else:
            ref = knots = DR.dense_adjoint(cs, g["codes"], g["mu_pass"], g["fb"], r.X, r.U, lam, sd.gX, sd.gU, pk, LD)
        r64 = DR.sweep(cs, K64, DR.factors(Quu64), g["codes"], g["mu_pass"], g["fb"], r.X, r.U, lam.astype(np.float64), sd.gX, sd.gU, pk, np.float64)
        for k in OUTS:
            w.append(within(got[k], ref[k], r64[k], g["fb"], "%s dense %s per_knot=%d" % (name, k, pk)))
    print(name, "dense adjoint: largest err / bound", max(w))


@pytest.mark.parametrize("name,pi", RUNS, ids=IDS)
def test_bytes_and_nothing_changes(name, pi):
    """5: the host twin, one output at a time, the weights alone (no third sweep, no active set read) and a seed alone give the
    same bytes; everything a caller can read is identical before and after; after altro_batch_set_options fb = 0 and the rows
    are NaN"""
    r = ran(name, pi)
    for a, b in ((r.all0, r.host0), (r.all1, r.host1)):
        assert set(a) == set(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and same(a[k], b[k]), k
    for k in OUTS:
        assert same(r.one[k][k], r.all1[k]) and same(r.one[k]["fb"], r.all1["fb"]), k
        assert same(r.s1[k], r.all0[k][:, 1]), k
    for k in WEIGHTS:
        assert same(r.w[k], r.all0[k]), k
    for k in r.before:
        assert np.array_equal(r.before[k], r.after[k], equal_nan=True), k
    assert (r.dropped["fb"] == 0).all()
    for k in OUTS:
        assert np.isnan(r.dropped[k]).all(), k


fma = getattr(math, "fma", None) or (lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c)))      # correctly rounded


def fma_chain(dz, e):
    """acc = fma(dz_k, e_k, acc) over axis 2 (the knots) in turn from +0, per element, exactly as one fused operation each"""
    acc = np.zeros(dz.shape[:2] + dz.shape[3:])
    for i in np.ndindex(*acc.shape):
        a = 0.0
        for k in range(dz.shape[2]):
            a = fma(float(dz[i[:2] + (k,) + i[2:]]), float(e[i[:2] + (k,) + i[2:]]), a)
        acc[i] = a
    return acc


@pytest.mark.parametrize("name,pi", TIES, ids=[s + "-pi" for s, _ in TIES])
def test_the_two_kernels_run_the_same_sweeps(name, pi):
    """7: solution_jvp(vXref, vUref) returns the xi, nu that solution_vjp_data(-(w vXref), -(wu vUref)) runs on, so the lane-local
    sums of the data kernel are functions of the JVP's outputs, the trajectory, the reference and the getter's codes alone, in
    the orders sensitivity_data.h states.  Compared as bytes, no tolerance: a rounding of difference between the sweeps of the
    two kernels, the two halves of one autograd layer, fails here"""
    r = ran(name, pi)
    cs, g, t = r.cs, r.g, r.tie
    n, N = cs.n, cs.N
    assert (g["fb"] == 1).all() and same(t.jvp["fb"], g["fb"]) and same(t.data["fb"], g["fb"])
    dX, dU = t.jvp["dX"], t.jvp["dU"]                                   # (B, S, N, n), (B, S, N-1, m)
    ex, eu = (r.X - cs.Xref)[:, None], (r.U - cs.Uref)[:, None]           # e = z - zref, rounded first
    dt = np.float64(cs.dt)
    want = dict(gQf=dX[:, :, -1] * ex[:, :, -1], gQ=dt * fma_chain(dX[:, :, :-1], np.broadcast_to(ex[:, :, :-1], dX[:, :, :-1].shape)),
                gR=dt * fma_chain(dU, np.broadcast_to(eu, dU.shape)))
    dz = np.concatenate([dX, np.concatenate([dU, np.zeros_like(dU[:, :, :1])], axis=2)], axis=3)      # (B, S, N, n + m)
    for key, bit in (("gzmax", 1), ("gzmin", 2)):
        acc = np.zeros(dz.shape[:2] + dz.shape[3:])
        for k in range(N):                                               # plain adds, k ascending, only the knots in the set
            on = ((g["codes"][:, k] & bit) != 0)[:, None]
            acc = np.where(on, acc + dz[:, :, k], acc)
        want[key] = 0.0 - g["mu_pass"][:, None, None] * acc
    bad = {k: int((np.ascontiguousarray(t.data[k]).view(np.uint64) != np.ascontiguousarray(v).view(np.uint64)).sum()) for k, v in want.items()}
    print(name, "elements that differ in a bit:", bad, "of", {k: v.size for k, v in want.items()}, "sides in the set", int((g["codes"] != 0).sum()))
    for k, v in want.items():
        assert t.data[k].shape == v.shape and same(t.data[k], v), (k, bad[k])


@pytest.mark.parametrize("name", ["16-box(12,4)-tight", "wide(64,16)-tight"])
def test_batch_one_handle_and_the_next_solve(name):
    """5: instance b on a solved batch-1 handle holding its rows of data (same trajectory, same gains: checked first) gets the
    bytes it gets inside the batch; the next solve of a handle that made the calls is that of a handle that never did"""
    r = ran(name, True)
    cs, sd = r.cs, r.sd
    for b in (0, cs.B - 1):      # the instance with the empty set and one with sides of every kind
        sv, _ = make_solver(name, True, ER.sub_case(cs, b), r.kw)
        try:
            Xb, Ub = plane(sv)
            assert same(Xb, r.X[b:b + 1]) and same(Ub, r.U[b:b + 1]) and same(altro.gains(sv)[0], r.K[b:b + 1]), ("the solves differ", b)
            one = call(sv, sd.gX[b:b + 1], sd.gU[b:b + 1], per_knot=True)
            g1 = getter(sv)
        finally:
            sv.close()
        for k in OUTS:
            assert same(one[k], r.all1[k][b:b + 1]), (b, k)
        assert same(g1["codes"], r.g["codes"][b:b + 1]) and same(g1["mu_pass"], r.g["mu_pass"][b:b + 1])
    a, csa = make_solver(name, True, *build_data(name, True))
    t, _ = make_solver(name, True, *build_data(name, True))
    try:
        call(a, sd.gX, sd.gU), call(a, sd.gX, sd.gU, per_knot=True), getter(a)
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


def raw(sv, names, per_knot=0, short=None, nseed=1):
    """the C-ABI itself: (return code, {name: tensor}) of altro_batch_solution_vjp_data_dev with sentinel outputs"""
    shp = shapes(sv, nseed, per_knot)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev())
    gX, gU = z(sv.B, nseed, sv.N, sv.n), z(sv.B, nseed, sv.N - 1, sv.m)
    out = {k: torch.full(shp[k], SENT, dtype=torch.float64, device=dev()) for k in names}
    st = altro._lib.SensDataOut(**{k: (short(t) if short is not None else t.data_ptr()) for k, t in out.items()})
    rc = sv._L.altro_batch_solution_vjp_data_dev(sv.h, nseed, gX.data_ptr(), gU.data_ptr(), per_knot, C.byref(st), None)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", ["16-soc(6,3)", "wide(17,5)", "wide(30,25)"])
def test_refusals_of_the_classes_not_covered(name):
    """5: with a LINEAR or SOC constraint the active-set outputs and the getter answer UNSUPPORTED on both forms while gQ, gQf, gR
    run and pass check 2; (30, 25) keeps no factors: UNSUPPORTED for everything; the handle stays as it was"""
    cs0, kw, _, _ = build(name, True)
    sv, cs = make_solver(name, True, cs0, kw)
    try:
        before = everything(sv, cs.x0, len(cs.cons))
        codes = torch.zeros((sv.B, sv.N, sv.n + sv.m), dtype=torch.uint8, device=dev())
        hc = np.zeros((sv.B, sv.N, sv.n + sv.m), dtype=np.uint8)
        for k in OUTS[3:]:
            assert raw(sv, (k,))[0] == UNSUP, k
        assert raw(sv, OUTS)[0] == UNSUP
        if name == "wide(30,25)":
            assert raw(sv, WEIGHTS)[0] == UNSUP
        else:
            assert sv._L.altro_batch_get_gain_active_set_dev(sv.h, codes.data_ptr(), None, None) == UNSUP
            assert sv._L.altro_batch_get_gain_active_set(sv.h, hc.ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == UNSUP
            sd = seeds(cs, 92)
            got, host = call(sv, sd.gX, sd.gU, WEIGHTS), call(sv, sd.gX, sd.gU, WEIGHTS, host=True)
            K, F = altro.gains(sv)[0], H(api.get_gain_factors_dev(sv))
            X, U = plane(sv)
            valid = H(altro.solution_vjp(sv, T(sd.gX), T(sd.gU), out=("gx0",))["fb"])
            assert same(got["fb"], valid) and (valid == 1).any()
            zc, zl = np.zeros((cs.B, cs.N, cs.n + cs.m), dtype=np.uint8), np.zeros((cs.B, cs.N, cs.n))
            y = {dt: DR.sweep(cs, K, F, zc, np.ones(cs.B), valid, X, U, zl, sd.gX, sd.gU, False, dt) for dt in (LD, np.float64)}
            for k in WEIGHTS:
                within(got[k], y[LD][k], y[np.float64][k], valid, name + " " + k)
                assert same(got[k], host[k]), k
        after = everything(sv, cs.x0, len(cs.cons))
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
    finally:
        sv.close()


def test_refusals_at_the_c_abi():
    """5: the argument rules of the header at the C-ABI itself: INVALID_ARG with the handle unchanged and usable; an output one
    double short is refused with the sentinels untouched; a 16-lane handle with N = 130 answers UNSUPPORTED for what needs the set"""
    cs = ER.add_box(ER.make_case(2, 12, 4, 6, 11), 0.9)
    sv = altro.ALTROSolver(ER.to_problem(altro, cs, shared=("cost", "box")), altro.SolverOptions(**OPTS))
    try:
        altro.solve(sv)
        L, h, B, N, n, m = sv._L, sv.h, sv.B, sv.N, sv.n, sv.m
        before = everything(sv, cs.x0, 1)
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev())
        gX, gU, q = z(B, 1, N, n), z(B, 1, N - 1, m), z(B, 1, n)
        p = lambda t: None if t is None else t.data_ptr()
        out = lambda **kw: C.byref(altro._lib.SensDataOut(**{k: p(v) for k, v in kw.items()}))
        hx = np.zeros((B, 1, N, n))
        fn, gt = L.altro_batch_solution_vjp_data_dev, L.altro_batch_get_gain_active_set_dev
        for args in ((None, 1, p(gX), p(gU), 0, out(gQ=q), None), (h, 0, p(gX), p(gU), 0, out(gQ=q), None), (h, 1, None, None, 0, out(gQ=q), None),
                     (h, 1, p(gX), p(gU), 0, None, None), (h, 1, p(gX), p(gU), 0, out(), None), (h, 1, p(gX), p(gU), 2, out(gQ=q), None),
                     (h, 1, p(gX), p(gU), -1, out(gQ=q), None), (h, 1, hx.ctypes.data, p(gU), 0, out(gQ=q), None)):
            assert fn(*args) == INV, args[1:5]
        assert L.altro_batch_solution_vjp_data(h, 1, None, None, 0, out(gQ=q), None) == INV
        assert gt(None, p(q), p(q), None) == INV and gt(h, None, None, None) == INV
        assert L.altro_batch_get_gain_active_set(h, None, None, None) == INV
        # one double short (the last doubles of the tensor's own allocation)
        paths = altro._lib.hip_runtimes()
        assert len(paths) == 1, paths
        rt = C.CDLL(paths[0])
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]

        def short(t):
            base, size = C.c_void_p(), C.c_size_t()
            assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), C.c_void_p(t.data_ptr())) == 0
            return base.value + size.value - (t.numel() * 8 - 8)

        for k in ("gA", "gzmin"):
            rc, o = raw(sv, (k,), 1, short)
            assert rc == INV and "shorter" in (L.altro_last_error(h) or b"").decode() and (o[k] == SENT).all(), k
        after = everything(sv, cs.x0, 1)
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
        rc, o = raw(sv, OUTS, 1)
        assert rc == 0 and all((t != SENT).all() for t in o.values())      # still usable
    finally:
        sv.close()
    cl = ER.add_box(ER.make_case(1, 12, 4, 130, 12), 0.9)
    sv = altro.ALTROSolver(ER.to_problem(altro, cl, shared=("cost", "box")), altro.SolverOptions(**OPTS))
    try:
        altro.solve(sv)
        for k in OUTS[3:]:
            assert raw(sv, (k,))[0] == UNSUP, k
        assert sv._L.altro_batch_get_gain_active_set_dev(sv.h, None, torch.zeros(1, dtype=torch.float64, device=dev()).data_ptr(), None) == UNSUP
        rc, o = raw(sv, WEIGHTS)
        assert rc == 0 and all((t != SENT).all() for t in o.values())      # (NaN where the long horizon kept no valid gains)
    finally:
        sv.close()


def test_mpc_layer_gradients():
    """6: torch.autograd.grad of a random linear functional of api.mpc_layer's (X, U) with respect to A, B, f, Q, R, Qf, the bounds,
    x0 and the reference equals the dense reference at what the solver then holds, under the rule"""
    cs, kw = build_data("16-box(12,4)-tight", True)
    sv = altro.ALTROSolver(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**OPTS))
    try:
        cm = lambda a: T(np.swapaxes(a, -1, -2)).transpose(-1, -2)       # column-major blocks
        box = cs.cons[0]
        leaf = lambda t: t.requires_grad_()
        x0, Xr, Ur = (leaf(T(a)) for a in (cs.x0, cs.Xref, cs.Uref))
        A, Bm, f = leaf(cm(cs.A[:, 0])), leaf(cm(cs.Bm[:, 0])), leaf(T(cs.f[:, 0]))
        Q, R, Qf, zmin, zmax = (leaf(T(a)) for a in (cs.Q, cs.R, cs.Qf, box.zmin, box.zmax))
        X, U = altro.mpc_layer(sv, x0, Xr, Ur, A=A, B=Bm, f=f, Q=Q, R=R, Qf=Qf, zmin=zmin, zmax=zmax)
        sd = seeds(cs, 93, ns=1)
        loss = (T(sd.gX[:, 0]) * X).sum() + (T(sd.gU[:, 0]) * U).sum()
        grads = dict(zip(OUTS, (H(g) for g in torch.autograd.grad(loss, (Q, Qf, R, zmin, zmax, A, Bm, f)))))
        Xh, Uh = plane(sv)
        assert same(H(X.detach()), Xh) and same(H(U.detach()), Uh)
        g = getter(sv)
        duals, mu = altro.get_duals(sv, 0), altro.penalty(sv)
    finally:
        sv.close()
    assert (g["fb"] == 1).all()
    lam = DR.costate(cs, Xh, Uh, duals, mu, LD)
    ref = DR.dense_adjoint(cs, g["codes"], g["mu_pass"], g["fb"], Xh, Uh, lam, sd.gX, sd.gU, False, LD)
    K64, Quu64 = DR.riccati_codes(cs, g["codes"], g["mu_pass"], np.float64)
    r64 = DR.sweep(cs, K64, DR.factors(Quu64), g["codes"], g["mu_pass"], g["fb"], Xh, Uh, lam.astype(np.float64), sd.gX, sd.gU, False, np.float64)
    for k in OUTS:
        within(np.ascontiguousarray(grads[k])[:, None], ref[k], r64[k], g["fb"], "mpc_layer " + k)


def test_mpc_layer_with_an_invalid_instance():
    """6: with instances whose stored pass was regularised the forward raises; with invalid="zero" their gradient rows are zero"""
    cs = ER.add_box(ER.make_case(3, 17, 5, 5, 25), 1e6)
    opts = dict(OPTS, bp_reg_initial=1e-3, iterations=1, iterations_inner=1, iterations_outer=1)
    sv = altro.ALTROSolver(ER.to_problem(altro, cs, shared=("cost", "box")), altro.SolverOptions(**opts))
    try:
        x0, Xr, Ur, Q, R, Qf = (T(a).requires_grad_() for a in (cs.x0, cs.Xref, cs.Uref, cs.Q, cs.R, cs.Qf))
        with pytest.raises(altro.AltroError):
            altro.mpc_layer(sv, x0, Xr, Ur, Q=Q, R=R, Qf=Qf)
        X, U = altro.mpc_layer(sv, x0, Xr, Ur, Q=Q, R=R, Qf=Qf, invalid="zero")
        assert (getter(sv)["fb"] == 0).all()
        for gr in torch.autograd.grad(X.sum() + U.sum(), (x0, Xr, Q, R, Qf)):
            assert same(H(gr), np.zeros(tuple(gr.shape)))
    finally:
        sv.close()
