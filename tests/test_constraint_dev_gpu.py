"""Constraint data and box bounds from device pointers on the GPU (altro_batch_update_constraint_data_dev,
altro_batch_set_bounds_dev, altro_batch_get_dev_refusals): a handle driven by the `_dev` calls equals, exactly, a twin handle
driven by the host calls of the same name -- states, controls, the duals of every constraint, statistics and traces -- on both
backends, with shared and per-instance tables, with host and device calls mixed, and with rows the device-side check of the
bounds refuses.  Memory is allocated through torch."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc, problems
from altro_mpc_icra2021_amd.benchmarks import GRASP_MPC_OPTS, ROCKET_COLD_OPTS, run_grasp

pytestmark = pytest.mark.gpu
REF_OPTS = mpc.REF_OPTS
INV = altro._lib.ERR_INVALID_ARG


def dev():
    return torch.device("cuda", 0)


def T(a):
    """numpy -> GPU tensor, same bytes"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev())


def snapshot(sv):
    st = altro.stats(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), it=st.iterations, ito=st.iterations_outer, status=st.status,
               cost=st.cost, cmax=st.c_max, Jt=st.cost_trace, ct=st.cmax_trace, alpha=altro.alpha_trace(sv))
    for c in range(len(sv.con_ids)):
        out["dual%d" % c] = altro.get_duals(sv, c)
    return out


def assert_equal(a, b, what="", rows=None, other_rows=None):
    assert a.keys() == b.keys()
    for k in a:
        x = a[k] if rows is None else a[k][rows]
        y = b[k] if other_rows is None else b[k][other_rows]
        assert np.array_equal(x, y, equal_nan=True), (what, k)


# ---- grasp-style problems: (6, 6), per-knot torque balance (3 equality rows), normal-force limits (2 inequality rows) and
# two friction cones, written in the tangent basis of each contact so that a cone has dimension 3
def grasp_tables(nk):
    """[(soc, equality, A (nk, p, 12), b (nk, p))] over a long horizon of nk knots; a window is a slice of it"""
    gp = problems.gen_grasp_problem(N=nk + 1, tf=0.1 * nk)
    n = 6
    tabs = [(False, True, gp.constraints[1].A, gp.constraints[1].b), (False, False, gp.constraints[2].A, gp.constraints[2].b)]
    t1 = np.array([1.0, 0.0, 0.0])
    for i in range(2):
        A4 = gp.constraints[3 + i].A
        A3 = np.zeros((nk, 3, 12))
        for k in range(nk):
            v = gp.v[i][k]
            A3[k, 0, n + 3 * i:n + 3 * i + 3] = t1
            A3[k, 1, n + 3 * i:n + 3 * i + 3] = np.cross(v, t1)
            A3[k, 2] = A4[k, 3]
        tabs.append((True, False, A3, np.zeros((nk, 3))))
    return gp, tabs


def window(tab, i, N, B=None, b0=0):
    """data of one constraint for the window starting at knot i: shared (N-1, p, nz), or one window per instance, instance b
    (counted from b0) reading the long table from knot i + b"""
    _, _, A, b = tab
    if B is None:
        return A[i:i + N - 1].copy(), b[i:i + N - 1].copy()
    return (np.stack([A[i + b0 + k:i + b0 + k + N - 1] for k in range(B)]), np.stack([b[i + b0 + k:i + b0 + k + N - 1] for k in range(B)]))


def grasp_problem(gp, tabs, x0, N, per_instance=(False, False, False, False), b0=0):
    B = x0.shape[0]
    model = altro.LinearModel(gp.A, gp.Bm, gp.f, dt=gp.dt)
    Xr, Ur = np.tile(gp.x0, (B, N, 1)), np.tile(gp.U0[:N - 1], (B, 1, 1))
    obj = altro.TrackingObjective(np.full(6, 1e3), np.full(6, 1.0), np.full(6, 10.0), Xr, Ur)
    cons = altro.ConstraintList(6, 6, N)
    for tab, pi in zip(tabs, per_instance):
        A, b = window(tab, 0, N, B if pi else None, b0)
        con = altro.NormConstraint(A, b, per_instance=pi) if tab[0] else altro.LinearConstraint(A, b, equality=tab[1], per_instance=pi)
        cons.add_constraint(con, (1, N - 1))
    return altro.Problem(model, obj, cons, x0=x0, N=N, U0=Ur.copy())


def grasp_x0(gp, B, ticks, seed=3):
    rng = np.random.default_rng(seed)
    return [np.tile(gp.x0, (B, 1)) + 0.02 * rng.standard_normal((B, 6)) for _ in range(ticks + 1)]


def grasp_tick(sv, x0, data, device):
    """{set x0, primal shift, update every constraint, dual shift, solve}: the order of the reference's grasp loop"""
    altro.set_initial_state(sv, x0)
    altro.shift_fill(sv, True, False)
    for ci, (A, b) in enumerate(data):
        if device:
            altro.update_constraint_data(sv, ci, T(A), T(b))
        else:
            altro.update_constraint_data(sv, ci, A, b)
    altro.shift_fill(sv, False, True)
    altro.solve(sv)


def twins(prob, opts, k=2):
    return [altro.ALTROSolver(prob, altro.SolverOptions(**opts)) for _ in range(k)]


def close(*svs):
    for sv in svs:
        sv.close()


@pytest.mark.parametrize("switches", [(), ("ALTRO_NO_LONE", "ALTRO_NO_SHADOW", "ALTRO_NO_GROUP"), ("ALTRO_FORCE_WIDE",)])
def test_grasp_loop_shared_tables(monkeypatch, switches):
    """(6, 6), N = 8, B = 6 (two padded slots on the 16-lane backend): three ticks that rewrite all four per-knot, shared
    constraints; also with the lone, shadow and group scheduling off, and on the one-wave-per-instance backend."""
    for s in switches:
        monkeypatch.setenv(s, "1")
    B, N, S = 6, 8, 3
    gp, tabs = grasp_tables(N + S)
    xs = grasp_x0(gp, B, S)
    hs, ds = twins(grasp_problem(gp, tabs, xs[0], N), GRASP_MPC_OPTS)
    try:
        altro.solve(hs), altro.solve(ds)
        for i in range(1, S + 1):
            data = [window(t, i, N) for t in tabs]
            grasp_tick(hs, xs[i], data, False), grasp_tick(ds, xs[i], data, True)
            a = snapshot(hs)
            assert_equal(a, snapshot(ds), ("tick", i, switches))
            assert a["it"].min() >= 1
        assert altro.dev_refusals(ds) == 0
    finally:
        close(hs, ds)


def test_grasp_loop_per_instance_tables():
    """per_knot = 3 on every constraint, B = 5, distinct data per instance: the `_dev` handle equals the host handle after
    every tick, and instance i equals a batch-1 handle given instance i's data."""
    B, N, S = 5, 8, 3
    gp, tabs = grasp_tables(N + S + B)
    xs = grasp_x0(gp, B, S)
    pi = (True,) * 4
    hs, ds = twins(grasp_problem(gp, tabs, xs[0], N, pi), GRASP_MPC_OPTS)
    ones = [altro.ALTROSolver(grasp_problem(gp, tabs, xs[0][b:b + 1], N, pi, b0=b), altro.SolverOptions(**GRASP_MPC_OPTS)) for b in range(B)]
    try:
        for sv in [hs, ds] + ones:
            altro.solve(sv)
        for i in range(1, S + 1):
            data = [window(t, i, N, B) for t in tabs]
            grasp_tick(hs, xs[i], data, False), grasp_tick(ds, xs[i], data, True)
            d = snapshot(ds)
            assert_equal(snapshot(hs), d, ("tick", i))
            for b, sv in enumerate(ones):
                grasp_tick(sv, xs[i][b:b + 1], [window(t, i, N, 1, b0=b) for t in tabs], True)
                assert_equal(snapshot(sv), d, ("instance", b, "tick", i), other_rows=slice(b, b + 1))
        assert not np.array_equal(d["U"][0], d["U"][B - 1])       # the instances do differ
    finally:
        close(hs, ds, *ones)


def test_time_invariant_tables_update_b_then_A():
    """(6, 3) rocket: one-block cones and a one-block linear row, the time-invariant fast path of the sweeps.  Only b of the
    thrust cone, then only A of the thrust-angle cone."""
    rp = problems.gen_rocket_problem(N=31, tf=3.0)
    B = 5
    x0 = np.tile(rp.x0, (B, 1)) + 0.3 * np.random.default_rng(3).standard_normal((B, 6))
    hs, ds = twins(mpc.constrained_problem(rp, x0), ROCKET_COLD_OPTS)
    try:
        altro.solve(hs), altro.solve(ds)
        assert_equal(snapshot(hs), snapshot(ds), "before")
        b1 = rp.constraints[1].b * np.array([1.0, 1.0, 1.0, 0.8])
        A2 = rp.constraints[2].A * np.array([[1.0], [1.0], [1.3]])
        for step, (ci, A, b) in enumerate([(1, None, b1), (2, A2, None)]):
            altro.update_constraint_data(hs, ci, A, b)
            altro.update_constraint_data(ds, ci, None if A is None else T(A), None if b is None else T(b))
            altro.set_initial_state(hs, x0 * 0.98), altro.set_initial_state(ds, x0 * 0.98)
            altro.solve(hs), altro.solve(ds)
            a = snapshot(hs)
            assert_equal(a, snapshot(ds), ("update", step))
            assert a["it"].min() >= 1
    finally:
        close(hs, ds)


@pytest.mark.parametrize("force_wide", [False, True])
def test_shared_constraint_on_a_per_instance_table_fans_out(monkeypatch, force_wide):
    """constraint 0 shared per-knot, constraint 1 per-instance: the table is per-instance, and a `_dev` update of the shared
    constraint reaches every slot of it."""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B, N = 6, 8
    gp, tabs = grasp_tables(N + 2 + B)
    xs = grasp_x0(gp, B, 1)
    pi = (False, True, False, False)
    hs, ds = twins(grasp_problem(gp, tabs, xs[0], N, pi), GRASP_MPC_OPTS)
    try:
        altro.solve(hs), altro.solve(ds)
        A, b = window(tabs[0], 2, N)
        altro.update_constraint_data(hs, 0, A, b), altro.update_constraint_data(ds, 0, T(A), T(b))
        altro.set_initial_state(hs, xs[1]), altro.set_initial_state(ds, xs[1])
        altro.solve(hs), altro.solve(ds)
        assert_equal(snapshot(hs), snapshot(ds), ("fan-out", force_wide))
    finally:
        close(hs, ds)


@pytest.mark.parametrize("force_wide", [False, True])
def test_per_knot_rows_that_are_equal_at_every_knot(monkeypatch, force_wide):
    """Every per-knot constraint is given the same row at every knot.  The host call then finds the tables time-invariant and
    lets the sweeps load each lane's row once; the `_dev` call cannot look at the rows and keeps the per-knot loads.  Equal
    values from either place: the results do not differ."""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B, N = 6, 8
    gp, tabs = grasp_tables(N + 2)
    xs = grasp_x0(gp, B, 2)
    hs, ds = twins(grasp_problem(gp, tabs, xs[0], N), GRASP_MPC_OPTS)
    try:
        altro.solve(hs), altro.solve(ds)
        for i in (1, 2):
            data = [tuple(np.repeat(v[i:i + 1], N - 1, axis=0) for v in window(t, 0, N)) for t in tabs]
            grasp_tick(hs, xs[i], data, False), grasp_tick(ds, xs[i], data, True)
            a = snapshot(hs)
            assert_equal(a, snapshot(ds), ("equal rows", i, force_wide))
            assert a["it"].min() >= 1
    finally:
        close(hs, ds)


def add_late(sv, con, first, last, per_instance):
    """altro_batch_add_constraint of a per-knot cone on a solver that exists already (before its first solve)"""
    A, b = api._c(con[0]), api._c(con[1])
    cid = C.c_int32(-1)
    sv._chk(sv._L.altro_batch_add_constraint(sv.h, altro._lib.CON_SOC, altro._lib.SENSE_INEQ, first - 1, last - 1, A.shape[-2],
                                             api._p(A), api._p(b), None, None, 3 if per_instance else 1, C.byref(cid)))
    sv.con_ids.append(cid.value)


@pytest.mark.parametrize("force_wide", [False, True])
@pytest.mark.parametrize("late_per_instance", [False, True])
def test_device_update_then_add_constraint_then_solve(monkeypatch, force_wide, late_per_instance):
    """Before the first solve: `_dev` updates of two constraints, then altro_batch_add_constraint of a fourth -- which changes
    the row count of the wide backend's tables, and with per-instance data the shape of both backends' -- then the solve.  The
    rows the `_dev` calls wrote must survive the repack."""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B, N = 5, 8
    gp, tabs = grasp_tables(N + 3 + B)
    xs = grasp_x0(gp, B, 1)
    prob = grasp_problem(gp, tabs[:3], xs[0], N)
    hs, ds = twins(prob, GRASP_MPC_OPTS)
    try:
        d0, d1 = window(tabs[0], 2, N), window(tabs[1], 2, N)
        altro.update_constraint_data(hs, 0, *d0), altro.update_constraint_data(hs, 1, d1[0], None)
        altro.update_constraint_data(ds, 0, T(d0[0]), T(d0[1])), altro.update_constraint_data(ds, 1, T(d1[0]), None)
        late = window(tabs[3], 2, N, B if late_per_instance else None)
        add_late(hs, late, 1, N - 1, late_per_instance), add_late(ds, late, 1, N - 1, late_per_instance)
        prob.constraints.add_constraint(altro.NormConstraint(*late, per_instance=late_per_instance), (1, N - 1))   # (for get_duals)
        altro.solve(hs), altro.solve(ds)
        a = snapshot(hs)
        assert_equal(a, snapshot(ds), ("add after _dev", force_wide, late_per_instance))
        assert a["it"].min() >= 1 and "dual3" in a
        data = [window(t, 3, N) for t in tabs[:3]] + [window(tabs[3], 3, N, B if late_per_instance else None)]
        grasp_tick(hs, xs[1], data, False), grasp_tick(ds, xs[1], data, True)
        assert_equal(snapshot(hs), snapshot(ds), ("tick after the late constraint", force_wide, late_per_instance))
    finally:
        close(hs, ds)


def wide_problem(B=3, n=7, m=3, N=6, seed=17):
    """(7, 3) on the one-wave-per-instance backend: the box of the random-linear problem, two per-knot per-instance inequality
    rows on the controls, and a one-block cone of dimension 3"""
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=2, seed=seed)
    prob = mpc.gen_tracking_problem(pb)
    rng = np.random.default_rng(seed + 1)
    A = np.zeros((B, N - 1, 2, n + m))
    A[..., n:] = rng.standard_normal((B, N - 1, 2, m))
    b = -0.5 - rng.random((B, N - 1, 2))
    prob.constraints.add_constraint(altro.LinearConstraint(A, b, per_instance=True), (1, N - 1))
    Ac = np.zeros((3, n + m))
    Ac[0, n], Ac[1, n + 1], Ac[2, n + 2] = 1.0, 1.0, 0.5
    prob.constraints.add_constraint(altro.NormConstraint(Ac, np.array([0.0, 0.0, 2.0])), (1, N - 1))
    return prob, (A, b, Ac)


def test_wide_backend_per_instance_rows_and_a_cone():
    """(7, 3), N = 6, B = 3.  The first `_dev` update is issued before the first solve (the tables are then packed on the host
    once), the following ones between solves."""
    prob, (A, b, Ac) = wide_problem()
    hs, ds = twins(prob, REF_OPTS)
    try:
        for step, (sa, sb, sc) in enumerate([(1.1, 0.9, 1.2), (0.8, 1.2, 0.7), (1.3, 1.0, 1.0)]):
            altro.update_constraint_data(hs, 1, A * sa, b * sb), altro.update_constraint_data(ds, 1, T(A * sa), T(b * sb))
            altro.update_constraint_data(hs, 2, Ac * sc, None), altro.update_constraint_data(ds, 2, T(Ac * sc), None)
            altro.solve(hs), altro.solve(ds)
            a = snapshot(hs)
            assert_equal(a, snapshot(ds), ("wide", step))
            assert a["it"].min() >= 1
    finally:
        close(hs, ds)


@pytest.mark.parametrize("force_wide", [False, True])
def test_mixing_host_and_device_constraint_updates(monkeypatch, force_wide):
    """`_dev` update of constraint 0, then a host update of constraint 1 (which rebuilds the tables from the host copies of
    EVERY constraint: the copy of constraint 0 must come back from the device first), then the other way round."""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B, N = 6, 8
    gp, tabs = grasp_tables(N + 4)
    xs = grasp_x0(gp, B, 2)
    hs, ds = twins(grasp_problem(gp, tabs, xs[0], N), GRASP_MPC_OPTS)
    try:
        altro.solve(hs), altro.solve(ds)
        for i, dev_first in ((1, True), (2, False)):
            d0, d1 = window(tabs[0], 2 * i, N), window(tabs[1], 2 * i, N)
            altro.update_constraint_data(hs, 0, *d0), altro.update_constraint_data(hs, 1, *d1)
            if dev_first:
                altro.update_constraint_data(ds, 0, T(d0[0]), T(d0[1])), altro.update_constraint_data(ds, 1, *d1)
            else:
                altro.update_constraint_data(ds, 0, *d0), altro.update_constraint_data(ds, 1, T(d1[0]), T(d1[1]))
            altro.set_initial_state(hs, xs[i]), altro.set_initial_state(ds, xs[i])
            altro.solve(hs), altro.solve(ds)
            assert_equal(snapshot(hs), snapshot(ds), ("mixed", i, force_wide))
    finally:
        close(hs, ds)


def box_problem(n, m, N, B, seed=29):
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=2, seed=seed)
    prob = mpc.gen_tracking_problem(pb)
    prob.x0 = prob.x0 + 0.5 * np.random.default_rng(seed).standard_normal(prob.x0.shape)   # the bounds get active
    return pb, prob


def bound_rows(pb, scale):
    """(zmin, zmax) with the control bounds scaled; scale a scalar (one shared row) or (B,) (one row per instance)"""
    n, m = pb.n, pb.m
    s = np.atleast_1d(np.asarray(scale, dtype=float))[:, None]
    zmax = np.concatenate([np.full((len(s), n), np.inf), pb.u_bnd * s * np.ones((1, m))], axis=1)
    return (-zmax[0], zmax[0]) if np.ndim(scale) == 0 else (-zmax, zmax)


@pytest.mark.parametrize("n,m,N", [(12, 4, 10), (7, 3, 10)])
def test_mixing_device_bounds_with_a_host_cost_call(n, m, N):
    """`_dev` bounds, then a host set_tracking_cost per instance, which uploads every table again from the host copies: the
    copy of the bounds must come back from the device first."""
    B = 6
    pb, prob = box_problem(n, m, N, B)
    hs, ds = twins(prob, REF_OPTS)
    try:
        altro.solve(hs), altro.solve(ds)
        rng = np.random.default_rng(5)
        lo, hi = bound_rows(pb, 0.5 + 0.3 * rng.random(B))
        altro.set_bounds(hs, 0, lo, hi), altro.set_bounds(ds, 0, T(lo), T(hi))
        Q = 5.0 + 10.0 * rng.random((B, n))
        for sv in (hs, ds):
            altro.set_tracking_cost(sv, Q, np.full(m, 0.1), Q)
            altro.solve(sv)
        assert_equal(snapshot(hs), snapshot(ds), ("bounds then cost", n, m))
        lo, hi = bound_rows(pb, 0.6)                                  # and a shared row on top of the per-instance tables
        altro.set_bounds(hs, 0, lo, hi), altro.set_bounds(ds, 0, T(lo), T(hi))
        altro.solve(hs), altro.solve(ds)
        assert_equal(snapshot(hs), snapshot(ds), ("shared row on per-instance tables", n, m))
        assert altro.dev_refusals(ds) == 0
    finally:
        close(hs, ds)


@pytest.mark.parametrize("n,m,N", [(12, 4, 10), (7, 3, 10)])
def test_bounds_from_device_rows_and_refused_rows(n, m, N):
    """shared row -> new shared row -> per-instance rows, a solve after each; then rows the device refuses: row 1 holds a NaN,
    row 3 has zmin > zmax, row 4 makes an infinite side finite -- those instances keep their old rows, the others take the new
    ones, the counter reads 3; a refused shared row changes nothing and adds 1."""
    B = 6
    pb, prob = box_problem(n, m, N, B)
    hs, ds = twins(prob, REF_OPTS)
    try:
        altro.solve(hs), altro.solve(ds)
        rng = np.random.default_rng(7)
        old = bound_rows(pb, 0.5 + 0.4 * rng.random(B))
        for step, rows in enumerate([bound_rows(pb, 0.7), bound_rows(pb, 0.55), old]):
            altro.set_bounds(hs, 0, *rows), altro.set_bounds(ds, 0, T(rows[0]), T(rows[1]))
            altro.solve(hs), altro.solve(ds)
            a = snapshot(hs)
            assert_equal(a, snapshot(ds), ("bounds", step, n, m))
        assert altro.dev_refusals(ds) == 0
        new = bound_rows(pb, 0.4 + 0.3 * rng.random(B))
        lo, hi = new[0].copy(), new[1].copy()
        lo[1, n] = np.nan
        lo[3, n + 1], hi[3, n + 1] = hi[3, n + 1], lo[3, n + 1]
        hi[4, 0] = 100.0
        kept = [np.where(np.isin(np.arange(B), (1, 3, 4))[:, None], o, w) for o, w in zip(old, new)]
        altro.set_bounds(hs, 0, *kept), altro.set_bounds(ds, 0, T(lo), T(hi))
        altro.solve(hs), altro.solve(ds)
        assert_equal(snapshot(hs), snapshot(ds), ("refused rows", n, m))
        assert altro.dev_refusals(ds) == 3
        lo1, hi1 = bound_rows(pb, 0.3)
        lo1 = lo1.copy()
        lo1[n] = np.nan
        altro.set_bounds(ds, 0, T(lo1), T(hi1))
        altro.set_bounds(hs, 0, *kept)                               # the twin keeps its rows (and drops its stored gains too)
        altro.set_initial_state(hs, prob.x0 * 0.9), altro.set_initial_state(ds, prob.x0 * 0.9)
        altro.solve(hs), altro.solve(ds)
        assert_equal(snapshot(hs), snapshot(ds), ("refused shared row", n, m))
        assert altro.dev_refusals(ds) == 4
        assert (snapshot(ds)["it"] >= 1).all()
    finally:
        close(hs, ds)


def hip_runtime():
    paths = altro._lib.hip_runtimes()
    assert len(paths) == 1, paths
    return C.CDLL(paths[0])


@pytest.mark.parametrize("force_wide", [False, True])
def test_refusals_before_anything_is_enqueued(monkeypatch, force_wide):
    """A host pointer, a tensor one element short, NULL for both A and b, a BOX id for constraint data, a LINEAR id for the
    bounds, a NULL handle: ALTRO_ERR_INVALID_ARG with a message, and the handle then solves like an untouched twin."""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B, n, m, N = 3, 6, 3, 6
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=2, seed=19)
    prob = mpc.gen_tracking_problem(pb)                              # constraint 0: the BOX
    A = np.zeros((N - 1, 2, n + m))
    A[..., n:] = np.random.default_rng(2).standard_normal((N - 1, 2, m))
    b = np.full((N - 1, 2), -1.0)
    prob.constraints.add_constraint(altro.LinearConstraint(A, b), (1, N - 1))
    a, u = twins(prob, REF_OPTS)
    L = a._L
    try:
        altro.solve(a), altro.solve(u)
        gp = lambda t: C.c_void_p(t.data_ptr())
        box, lin = a.con_ids
        refused = []

        def refuse(rc, h=a):
            msg = (L.altro_last_error(h.h if h is not None else None) or b"").decode()
            assert rc == INV and msg, (rc, msg)
            refused.append(msg)

        At, bt = T(A * 2.0), T(b * 2.0)
        lo, hi = (T(v) for v in bound_rows(pb, np.full(B, 0.5)))
        host = np.zeros(A.size)
        hp = C.c_void_p(host.ctypes.data)
        refuse(L.altro_batch_update_constraint_data_dev(a.h, lin, hp, gp(bt)))
        refuse(L.altro_batch_update_constraint_data_dev(a.h, lin, gp(At), hp))
        refuse(L.altro_batch_set_bounds_dev(a.h, box, hp, gp(hi), 1))
        refuse(L.altro_batch_update_constraint_data_dev(a.h, lin, None, None))
        refuse(L.altro_batch_update_constraint_data_dev(a.h, box, gp(At), gp(bt)))
        refuse(L.altro_batch_update_constraint_data_dev(a.h, 99, gp(At), gp(bt)))
        refuse(L.altro_batch_set_bounds_dev(a.h, lin, gp(lo), gp(hi), 1))
        refuse(L.altro_batch_set_bounds_dev(a.h, box, None, gp(hi), 1))
        # one element short: the last A.size - 1 doubles of the allocation that holds the tensor
        rt = hip_runtime()
        rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        base, size = C.c_void_p(), C.c_size_t()
        assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(At)) == 0
        end = base.value + size.value
        refuse(L.altro_batch_update_constraint_data_dev(a.h, lin, C.c_void_p(end - (A.size - 1) * 8), None))
        refuse(L.altro_batch_set_bounds_dev(a.h, box, gp(lo), C.c_void_p(end - (B * (n + m) - 1) * 8), 1))
        assert all("shorter" in r for r in refused[-2:])
        assert L.altro_batch_update_constraint_data_dev(None, lin, gp(At), gp(bt)) == INV
        assert (L.altro_last_error(None) or b"").decode()
        assert L.altro_batch_set_bounds_dev(None, box, gp(lo), gp(hi), 1) == INV
        assert L.altro_batch_get_dev_refusals(None, C.byref(C.c_int64(0))) == INV
        refuse(L.altro_batch_get_dev_refusals(a.h, None))
        for sv in (a, u):
            altro.set_initial_state(sv, prob.x0 * 0.95)
            altro.solve(sv)
        assert_equal(snapshot(a), snapshot(u), ("after the refusals", force_wide))
        assert altro.dev_refusals(a) == 0
    finally:
        close(a, u)


def test_tick_takes_constraint_data_in_stream_order():
    """A and b are produced by torch kernels on torch's current stream, behind a long-running op; ExternalMPC.tick brackets
    the updates between wait_stream and signal_stream.  No synchronisation in the test before the final read."""
    B, N = 6, 8
    gp, tabs = grasp_tables(N + 2)
    xs = grasp_x0(gp, B, 1)
    hs, ds = twins(grasp_problem(gp, tabs, xs[0], N), GRASP_MPC_OPTS)
    try:
        altro.solve(hs), altro.solve(ds)
        data = [window(t, 1, N) for t in tabs]
        grasp_tick(hs, xs[1], data, False)
        want = snapshot(hs)
        half = [(T(A * 0.5), T(b * 0.5)) for A, b in data]
        x1 = T(xs[1])
        big = torch.randn(2048, 2048, device=dev())
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream(dev())
        with torch.cuda.stream(s1):
            for _ in range(20):                                  # work ahead of the producer
                big = big @ big * 1e-3
            made = {ci: (A + A, b + b) for ci, (A, b) in enumerate(half)}   # x + x is exact
            u0, _, st, it = altro.ExternalMPC(ds).tick(x1, constraint_data=made)
        got = snapshot(ds)                                       # (the getters wait for the solver's stream)
        assert_equal(want, got, "tick")
        assert np.array_equal(u0.cpu().numpy(), want["U"][:, 0]) and np.array_equal(it.cpu().numpy(), want["it"])
    finally:
        close(hs, ds)


def test_grasp_benchmark_loop_on_the_device_equals_the_host_loop():
    a = run_grasp(batch=4, N_mpc=11, steps=3, N_cold=41, device_io=False)
    b = run_grasp(batch=4, N_mpc=11, steps=3, N_cold=41, device_io=True)
    assert np.array_equal(np.asarray(a["iter"]), np.asarray(b["iter"]))
    assert np.array_equal(np.asarray(a["solve_succeeded"]), np.asarray(b["solve_succeeded"]))
