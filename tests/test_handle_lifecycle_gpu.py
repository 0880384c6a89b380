"""What a handle owns over its life, through the C-ABI on both backends: every device array that an entry point frees and
allocates again, the move of a 16-lane handle to the one-wave-per-instance kernel, create / destroy cycles, and the
diagnostic switches of altro_debug_set.  Everything here pins behaviour: results are compared bit for bit (np.array_equal)
between a handle that went through the reallocations and a fresh one that only ever saw the final data.

Sizes: batch 5 (not a multiple of the 4 instances of a wave: the 16-lane backend pads to 8), N = 8, (n, m) = (12, 4) on the
16-lane backend and (3, 2) on the other, one plain solve and two fused MPC steps.  Nothing asserts on free device memory."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest

from altro_mpc_icra2021_amd import _lib, problems
from helpers import D, I, Handle   # (Handle: batch 5, N = 8 unless told otherwise -- B and N below)

pytestmark = pytest.mark.gpu
OK, INV, UNSUP, STATE = _lib.OK, _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_STATE
B, N, STEPS = 5, 8, 2
DIMS = {"16-lane": (12, 4), "wide": (3, 2)}


@pytest.fixture(autouse=True)
def switches_of_the_environment():
    """the handles here are created through the C-ABI: every test starts from the switches api.ALTROSolver would forward
    (whatever an earlier test left in altro_debug_set(NULL, ..)), and leaves them so"""
    _lib.sync_debug_env()
    yield
    _lib.sync_debug_env()


@functools.lru_cache(maxsize=None)
def data(n, m, seed=7, steps=11):
    """a random-linear tracking problem with a track of N + steps + 1 knots, per-instance weights and control bounds, one
    shared and one per-instance LINEAR inequality row on the controls"""
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=steps, seed=seed)
    rng = np.random.default_rng([seed, n, m])
    z = n + m
    d = NS(n=n, m=m, dt=pb.dt, Nt=pb.Nt, Xt=pb.Xtrack, Ut=pb.Utrack, noise=pb.noise)
    d.A, d.Bm = np.transpose(pb.A, (0, 2, 1)), np.transpose(pb.Bm, (0, 2, 1))        # column-major blocks
    d.Q, d.R, d.Qf = 10 * (0.5 + rng.random((B, n))), 0.1 * (0.5 + rng.random((B, m))), 10 * (0.5 + rng.random((B, n)))
    ub = 3.0 * (1 + 0.1 * np.arange(B))
    d.lo = np.concatenate([np.full((B, n), -np.inf), -ub[:, None] * np.ones((B, m))], axis=1)
    d.hi = -d.lo
    d.A0, d.b0 = np.zeros((1, z)), np.array([-0.6 * m * 3.0])                        # sum(u) <= 0.6 m u_bnd
    d.A0[0, n:] = 1.0
    d.A1, d.b1 = np.zeros((B, 1, z)), -(1.0 + 0.2 * np.arange(B)).reshape(B, 1)      # u_0 - u_1 <= 1 + 0.2 b
    d.A1[:, 0, n], d.A1[:, 0, n + 1] = 1.0, -1.0
    return d


def add_constraints(h, d, linear=True):
    """BOX on the controls of knots 0 .. N-2, then (linear) the shared row, then the per-instance row; -> their ids"""
    ids = [C.c_int32(-1) for _ in range(3)]
    h.add_constraint(_lib.CON_BOX, 0, 0, N - 2, 0, None, None, D(d.lo[0]), D(d.hi[0]), 0, C.byref(ids[0]))
    if not linear:
        return [ids[0].value]
    h.add_constraint(_lib.CON_LINEAR, _lib.SENSE_INEQ, 0, N - 2, 1, D(d.A0), D(d.b0), None, None, 0, C.byref(ids[1]))
    lam = np.zeros((B, N - 1, 1))
    h.get_duals(ids[1], D(lam))     # (packs the tables while they hold shared rows only: the next block changes their shape)
    h.add_constraint(_lib.CON_LINEAR, _lib.SENSE_INEQ, 0, N - 2, 1, D(d.A1), D(d.b1), None, None, 2, C.byref(ids[2]))
    return [i.value for i in ids]


def final_data(h, d, ids=None, linear=True, steps=STEPS):
    """everything a solve reads, in one order for every handle; ids: the constraints exist already and take new data"""
    h.set_dynamics(D(d.A), D(d.Bm), None, 0, 1)
    h.set_tracking_cost_per_instance(D(d.Q), D(d.R), D(d.Qf), d.dt)
    if ids is None:
        ids = add_constraints(h, d, linear)
    else:
        h.update_constraint_data(ids[1], D(d.A0), D(d.b0))
        h.update_constraint_data(ids[2], D(d.A1), D(d.b1))
    h.set_bounds(ids[0], D(d.lo), D(d.hi), 1)
    h.set_track(D(d.Xt), D(d.Ut), d.Nt)
    h.set_noise(D(d.noise[:steps]), steps)
    h.set_log(steps)
    return ids


def run(h, ids, steps=STEPS):
    """one plain solve, `steps` fused MPC steps; -> everything the handle reports"""
    n, m = h.n, h.m
    h.solve()
    if steps:
        h.run_async(0, steps)
    h.synchronize()
    r = dict(X=np.zeros((B, N, n)), U=np.zeros((B, N - 1, m)), x0=np.zeros((B, n)), box=np.zeros((B, N - 1, 2, n + m)),
             cost=np.zeros(B), cmax=np.zeros(B))
    for k in ("iters", "outer", "status"):
        r[k] = np.zeros(B, dtype=np.int32)
    h.get_states(D(r["X"])), h.get_controls(D(r["U"])), h.get_initial_state(D(r["x0"]))
    h.get_stats(I(r["iters"]), I(r["outer"]), I(r["status"]), D(r["cost"]), D(r["cmax"]), None, None)
    if ids:
        h.get_duals(ids[0], D(r["box"]))
        for i in ids[1:]:
            r["lin%d" % i] = np.zeros((B, N - 1, 1))
            h.get_duals(i, D(r["lin%d" % i]))
    if steps:
        r.update(log_x0=np.zeros((steps, B, n)), log_u0=np.zeros((steps, B, m)), log_it=np.zeros((steps, B), dtype=np.int32))
        h.get_log(0, steps, D(r["log_x0"]), D(r["log_u0"]), I(r["log_it"]), None, None, None, None)
    r["reused"] = np.zeros(B, dtype=np.int64)
    h.get_reuse_counter(r["reused"].ctypes.data_as(C.POINTER(C.c_int64)))
    assert np.isfinite(r["X"]).all() and np.isfinite(r["U"]).all()
    return r


def same(a, b, skip=("reused",)):
    assert a.keys() == b.keys()
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


@functools.lru_cache(maxsize=None)
def fresh_run(backend):
    """a handle that receives the final data and nothing else: the reference of every comparison, computed once"""
    h = Handle(*DIMS[backend])
    try:
        r = run(h, final_data(h, data(*DIMS[backend])))
        factors = np.zeros((B, N - 1, h.m, h.m))      # (only the 16-lane backend keeps them: the handle runs where it should)
        assert h.rc("get_gain_factors", D(factors)) == (OK if backend == "16-lane" else UNSUP)
        assert (r["status"] != 0).all() and (r["log_it"] >= 0).all()     # every instance was solved, every step logged
        return r
    finally:
        assert h.destroy() == OK


@pytest.mark.parametrize("backend", list(DIMS))
def test_reallocation_sites_leave_no_trace(backend):
    """Handle A goes through every reallocation the API reaches, on another problem's data: tracks of 20, 30 and 20 knots,
    two log capacities, shared then per-instance weights and bounds, a per-instance constraint block behind a shared one, two
    noise lengths, altro_batch_evaluate with 1 and 4 candidates, one solve with the polish.  Then it is restarted and takes the
    final data: it computes what the fresh handle computes, bit for bit."""
    n, m = DIMS[backend]
    d, j, j30 = data(n, m), data(n, m, seed=8), data(n, m, seed=9, steps=21)
    assert (d.Nt, j.Nt, j30.Nt) == (20, 20, 30)
    h = Handle(n, m)
    try:
        h.set_dynamics(D(j.A), D(j.Bm), None, 0, 1)
        h.set_tracking_cost(D(j.Q[0]), D(j.R[0]), D(j.Qf[0]), j.dt)
        h.set_tracking_cost_per_instance(D(j.Q), D(j.R), D(j.Qf), j.dt)
        ids = add_constraints(h, j)
        h.set_bounds(ids[0], D(j.lo[1]), D(j.hi[1]), 0)
        h.set_bounds(ids[0], D(j.lo), D(j.hi), 1)
        for t in (j, j30, j):
            h.set_track(D(t.Xt), D(t.Ut), t.Nt)
        h.set_log(4), h.set_log(STEPS)
        h.set_noise(D(j30.noise[:3]), 3), h.set_noise(D(j.noise[:STEPS]), STEPS)
        for ncand in (1, 4):
            J = np.full((B, ncand), np.nan)
            h.evaluate(ncand, D(0.1 * np.ones((B, ncand, N - 1, m))), None, None, D(J), None, None, None)
            assert np.isfinite(J).all()
        h.polish(True)
        h.solve()
        h.polish(False)
        h.restart_instances(I(np.ones(B)), None, D(np.zeros((B, N - 1, m))))
        same(run(h, final_data(h, d, ids)), fresh_run(backend))
    finally:
        assert h.destroy() == OK


def test_move_to_the_wide_kernel_carries_the_handle_over():
    """x0, an active mask and a log capacity set on a (12, 4) handle before altro_batch_set_dynamics(per_knot = 1) moves it:
    it then holds them, solves, and matches a handle created on the one-wave-per-instance kernel and given the same data.
    (An episode clock cannot precede the move: it needs a track, and a handle with a track is not moved.)"""
    n, m = DIMS["16-lane"]
    d = data(n, m)
    Ak = np.stack([d.A[0] * (1.0 - 0.01 * k) for k in range(N - 1)])
    Bk = np.stack([d.Bm[0]] * (N - 1))
    x0, mask = d.Xt[:, 3].copy(), np.array([1, 1, 0, 1, 1], dtype=np.int32)
    ha = Handle(n, m)
    _lib.debug_set("force_wide", 1)
    try:
        hb = Handle(n, m)
    finally:
        _lib.debug_set("force_wide", 0)
    try:
        ha.set_initial_state(D(x0)), ha.set_active(I(mask)), ha.set_log(3)
        assert ha.rc("set_clock", I(np.zeros(B)), None) == STATE
        ha.set_dynamics(D(Ak), D(Bk), None, 1, 0)
        assert ha.rc("get_gain_factors", D(np.zeros((B, N - 1, m, m)))) == UNSUP      # (the wide backend answers)
        hb.set_dynamics(D(Ak), D(Bk), None, 1, 0)
        hb.set_initial_state(D(x0)), hb.set_active(I(mask)), hb.set_log(3)
        out = []
        for h in (ha, hb):
            gx, ga = np.zeros((B, n)), np.zeros(B, dtype=np.int32)
            h.get_initial_state(D(gx)), h.get_active(I(ga))
            assert np.array_equal(gx, x0) and np.array_equal(ga, mask)
            h.set_tracking_cost(D(d.Q[0]), D(d.R[0]), D(d.Qf[0]), d.dt)
            h.set_reference(D(d.Xt[:, :N]), D(d.Ut[:, :N - 1]))
            h.set_initial_trajectory(None, D(d.Ut[:, :N - 1]))
            r = run(h, None, steps=0)
            r["log_x0"], r["log_it"] = np.zeros((3, B, n)), np.zeros((3, B), dtype=np.int32)
            h.get_log(0, 3, D(r["log_x0"]), None, I(r["log_it"]), None, None, None, None)
            assert np.isnan(r["log_x0"]).all() and (r["log_it"] == -1).all()          # plain solves write no record
            out.append(r)
        same(out[0], out[1], skip=())
        assert np.array_equal(out[0]["U"][2], d.Ut[2, :N - 1]) and out[0]["status"][2] == 0      # the masked instance sat out
    finally:
        assert ha.destroy() == OK and hb.destroy() == OK


@pytest.mark.parametrize("backend", list(DIMS))
def test_create_destroy_cycles(backend):
    """20 handles created and destroyed in one process; the last one solves what the fresh handle solved"""
    n, m = DIMS[backend]
    for cycle in range(20):
        h = Handle(n, m)
        try:
            if cycle == 19:
                same(run(h, final_data(h, data(n, m))), fresh_run(backend), skip=())
        finally:
            assert h.destroy() == OK


SWITCHES = [(key, default) for _, key, default in _lib.DEBUG_ENV] + [("group_mode", 1), ("dev_via_stage", 0)]
CREATE_TIME = ("force_wide", "wide_compact", "wide_coop", "wide_static_mask")


def expected_rc(key, live):
    if key in CREATE_TIME:
        return STATE if live else OK
    if key == "dev_via_stage":
        return OK if live else STATE
    return OK


def test_switch_table():
    """altro_debug_set with a null handle (defaults of the handles created afterwards), a live 16-lane handle and a live wide
    one: create-time keys are refused on a handle, dev_via_stage needs one, group_mode is 0..4, keep_gains != 0 needs a debug
    build, scheduling keys are accepted everywhere and an unknown key is ALTRO_ERR_INVALID_ARG.  Every value set is the
    default, so nothing changes for the tests that follow."""
    L = _lib.lib()
    handles = {name: Handle(*nm) for name, nm in DIMS.items()}
    try:
        for who, h in [("null", None)] + [(k, v.h) for k, v in handles.items()]:
            for key, default in SWITCHES:
                assert L.altro_debug_set(h, key.encode(), default) == expected_rc(key, h is not None), (who, key)
            for key, value, rc in (("group_mode", 5, INV), ("group_mode", -1, INV), ("keep_gains", 1, UNSUP), ("no_such_switch", 0, INV)):
                assert L.altro_debug_set(h, key.encode(), value) == rc, (who, key, value)
                assert (L.altro_last_error(h) or b"").decode()
        assert L.altro_debug_set(None, None, 0) == INV
    finally:
        for h in handles.values():
            assert h.destroy() == OK


def test_no_reuse_on_a_live_handle_is_no_reuse_at_create():
    """"no_reuse" set on a live 16-lane handle gives the bits of a handle created under it, and neither reuses a gain; a
    default handle does (BOX only, six steps: the kernels with constraint rows reuse none)"""
    n, m = DIMS["16-lane"]
    hs = [Handle(n, m), Handle(n, m)]
    _lib.debug_set("no_reuse", 1)
    try:
        hs.append(Handle(n, m))
    finally:
        _lib.debug_set("no_reuse", 0)
    try:
        assert _lib.lib().altro_debug_set(hs[1].h, b"no_reuse", 1) == OK
        r0, ra, rb = (run(h, final_data(h, data(n, m), linear=False, steps=6), steps=6) for h in hs)
        print("gain reuses: default", r0["reused"].sum(), "no_reuse", ra["reused"].sum(), rb["reused"].sum())
        same(ra, rb, skip=())
        assert ra["reused"].sum() == 0 and r0["reused"].sum() > 0
    finally:
        for h in hs:
            assert h.destroy() == OK
