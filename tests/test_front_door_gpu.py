"""The front door of the host library on both backends: what the shared entry points refuse, and what they read back.

Every case runs on a 16-lane handle at (n, m) = (6, 3) and on a handle of the same dimensions on the one-wave-per-instance
backend (force_wide), through the raw C-ABI.  Batch 5 (the 16-lane backend pads it to 8 slots, the other holds 5), N = 5.

Refusal table: one row per entry point and bad argument.  A row's call returns before the library makes any HIP call; both
backends must give the same code and the same altro_last_error text, and the handle must go on to solve (one plain solve,
three fused MPC steps) exactly what a fresh handle given the same calls minus the refused one solves.  Rows whose id ends
in "parent" are refused in host code by the wide backend of the commit before the front door was shared, too; the others
were accepted there, or reached the HIP runtime with a null pointer.

Shared reads: exact equalities only (counts, an identity of integer counters, guard values, bytes of the log)."""
import ctypes as C
import functools

import numpy as np
import pytest

from altro_mpc_icra2021_amd import _lib, problems
from helpers import D, I, Handle

pytestmark = pytest.mark.gpu
OK, INV, STATE = _lib.OK, _lib.ERR_INVALID_ARG, _lib.ERR_STATE
B, N, NM, S = 5, 5, (6, 3), 4          # S: steps of uploaded noise; the log holds LOGCAP of them
LOGCAP = 3
BACKENDS = ("16-lane", "wide")
i64 = C.POINTER(C.c_int64)


@pytest.fixture(autouse=True)
def switches_of_the_environment():
    _lib.sync_debug_env()
    yield
    _lib.sync_debug_env()


def make(backend):
    _lib.debug_set("force_wide", 1 if backend == "wide" else 0)
    try:
        return Handle(*NM, batch=B, N=N)
    finally:
        _lib.debug_set("force_wide", 0)


@functools.lru_cache(maxsize=None)
def data():
    n, m = NM
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=11)
    assert pb.Nt == N + S + 1
    z = np.full(n + m, np.inf)
    z[n:] = 3.0
    # (noise for every step the track has room for: the rows "past the track" must get past the noise rule first)
    long_noise = np.random.default_rng(5).standard_normal((pb.Nt - N + 1, B, n))
    return pb, np.transpose(pb.A, (0, 2, 1)).copy(), np.transpose(pb.Bm, (0, 2, 1)).copy(), -z, z, long_noise


def setup(h, ctx=None):
    """everything a solve and a fused MPC launch read; ctx: what a row needs the handle to hold before its call"""
    pb, A, Bm, lo, hi, long_noise = data()
    n, m = NM
    h.box = C.c_int32(-1)
    h.set_dynamics(D(A), D(Bm), None, 0, 1)
    h.set_tracking_cost(D(np.full(n, 10.0)), D(np.full(m, 0.1)), D(np.full(n, 10.0)), pb.dt)
    h.add_constraint(_lib.CON_BOX, 0, 0, N - 2, 0, None, None, D(lo), D(hi), 0, C.byref(h.box))
    h.set_track(D(pb.Xtrack), D(pb.Utrack), pb.Nt)
    if ctx == "long noise":
        h.set_noise(D(long_noise), len(long_noise))
    else:
        h.set_noise(D(pb.noise), S)
    if ctx != "no log":
        h.set_log(LOGCAP)
    if ctx == "mask":
        h.set_active(I([1, 0, 1, 1, 0]))
    if ctx == "clock":
        h.set_clock(I(np.zeros(B)), None)


def undo(h, ctx):
    """the handle back to whole batches on one window, so that every context ends in the same solve"""
    if ctx == "mask":
        h.set_active(None)
    if ctx == "clock":
        h.set_clock(None, None)
    if ctx == "no log":
        h.set_log(LOGCAP)


def solve_and_read(h):
    """one plain solve, three fused MPC steps; -> everything the handle reports"""
    n, m = NM
    h.solve()
    h.run_async(0, LOGCAP)
    h.synchronize()
    r = dict(X=np.zeros((B, N, n)), U=np.zeros((B, N - 1, m)), x0=np.zeros((B, n)), cost=np.zeros(B), cmax=np.zeros(B),
             log_x0=np.zeros((LOGCAP, B, n)), log_u0=np.zeros((LOGCAP, B, m)), log_J=np.zeros((LOGCAP, B)))
    for k in ("iters", "outer", "status"):
        r[k] = np.zeros(B, dtype=np.int32)
    r["log_it"] = np.zeros((LOGCAP, B), dtype=np.int32)
    h.get_states(D(r["X"])), h.get_controls(D(r["U"])), h.get_initial_state(D(r["x0"]))
    h.get_stats(I(r["iters"]), I(r["outer"]), I(r["status"]), D(r["cost"]), D(r["cmax"]), None, None)
    h.get_log(0, LOGCAP, D(r["log_x0"]), D(r["log_u0"]), I(r["log_it"]), None, None, D(r["log_J"]), None)
    assert np.isfinite(r["X"]).all() and (r["status"] != 0).all() and (r["log_it"] >= 1).all()
    return r


@functools.lru_cache(maxsize=None)
def fresh(backend, ctx):
    """the same calls minus the refused one, on a handle of its own; computed once per backend and context"""
    h = make(backend)
    try:
        setup(h, ctx)
        undo(h, ctx)
        return solve_and_read(h)
    finally:
        assert h.destroy() == OK


def _f32():
    return C.byref(C.c_float())


def _w():
    return D(np.full(NM[0], 0.01))


# (id, context, the call, the code both backends answer, the parent's wide backend refuses it in host code too)
ROWS = [
    ("get_alpha_trace-null", None, lambda h: h.rc("get_alpha_trace", None), INV, False),
    ("get_states-null", None, lambda h: h.rc("get_states", None), INV, False),
    ("get_controls-null", None, lambda h: h.rc("get_controls", None), INV, False),
    ("get_duals-null", None, lambda h: h.rc("get_duals", h.box, None), INV, False),
    ("set_duals-null", None, lambda h: h.rc("set_duals", h.box, None), INV, False),
    ("last_solve_ms-null", None, lambda h: h.rc("last_solve_ms", None), INV, False),
    ("last_solve_ms-before_any_solve", None, lambda h: h.rc("last_solve_ms", _f32()), STATE, True),
    ("get_reuse_counter-null", None, lambda h: h.rc("get_reuse_counter", None), INV, True),
    ("get_confirm_counter-null", None, lambda h: h.rc("get_confirm_counter", None), INV, True),
    ("get_dev_refusals-null", None, lambda h: h.rc("get_dev_refusals", None), INV, True),
    ("set_initial_state-null", None, lambda h: h.rc("set_initial_state", None), INV, True),
    ("get_initial_state-null", None, lambda h: h.rc("get_initial_state", None), INV, True),
    ("set_reference-null", None, lambda h: h.rc("set_reference", None, None), INV, True),
    ("set_track-null", None, lambda h: h.rc("set_track", None, None, 12), INV, True),
    ("set_track-shorter_than_the_horizon", None, lambda h: h.rc("set_track", D(data()[0].Xtrack), D(data()[0].Utrack), N - 1), INV, True),
    ("set_bounds-not_the_box", None, lambda h: h.rc("set_bounds", h.box.value + 1, D(data()[3]), D(data()[4]), 0), INV, True),
    ("set_noise-null", None, lambda h: h.rc("set_noise", None, S), INV, True),
    ("set_noise-no_steps", None, lambda h: h.rc("set_noise", D(data()[0].noise), 0), INV, True),
    ("set_noise_model-null_weights", None, lambda h: h.rc("set_noise_model", 0, None, None), INV, True),
    ("set_noise_model-mode_3", None, lambda h: h.rc("set_noise_model", 3, _w(), None), INV, True),
    ("set_noise_model-group_2", None, lambda h: h.rc("set_noise_model", 1, _w(), I([0, 0, 0, 1, 1, 2])), INV, False),
    ("set_log-negative", None, lambda h: h.rc("set_log", -1), INV, True),
    ("get_log-before_set_log", "no log", lambda h: h.rc("get_log", 0, 1, None, None, None, None, None, None, None), STATE, True),
    ("get_log-negative_step", None, lambda h: h.rc("get_log", -1, 1, None, None, None, None, None, None, None), INV, True),
    ("get_log-past_the_capacity", None, lambda h: h.rc("get_log", 1, LOGCAP, None, None, None, None, None, None, None), INV, True),
    ("run_async-negative_step", None, lambda h: h.rc("run_async", -1, 1), INV, True),
    ("run_async-no_steps", None, lambda h: h.rc("run_async", 0, 0), INV, True),
    ("run_async-past_the_noise", None, lambda h: h.rc("run_async", 0, S + 1), INV, True),
    ("run_async-past_the_log", None, lambda h: h.rc("run_async", 0, LOGCAP + 1), INV, True),
    ("run_async-past_the_track", "long noise", lambda h: h.rc("run_async", S + 1, 1), INV, True),
    ("prepare_async-negative_step", None, lambda h: h.rc("prepare_async", -1), INV, True),
    ("prepare_async-past_the_noise", None, lambda h: h.rc("prepare_async", S), INV, True),
    ("prepare_async-past_the_track", "long noise", lambda h: h.rc("prepare_async", S + 1), INV, True),
    ("benchmark_solve-no_samples", None, lambda h: h.rc("benchmark_solve", 0, 1, None), INV, True),
    ("benchmark_solve-no_evals", None, lambda h: h.rc("benchmark_solve", 1, 0, None), INV, True),
    ("benchmark_solve-under_a_mask", "mask", lambda h: h.rc("benchmark_solve", 1, 1, None), STATE, True),
    ("benchmark_solve-under_a_clock", "clock", lambda h: h.rc("benchmark_solve", 1, 1, None), STATE, True),
]


@pytest.mark.parametrize("ctx,call,code", [pytest.param(c, f, rc, id=name + ("-parent" if parent else "")) for name, c, f, rc, parent in ROWS])
def test_refusal(ctx, call, code):
    answers = []
    for backend in BACKENDS:
        h = make(backend)
        try:
            setup(h, ctx)
            rc = call(h)
            answers.append((rc, h.error()))
            print(backend, answers[-1])
            undo(h, ctx)
            r, f = solve_and_read(h), fresh(backend, ctx)
            for k in f:
                assert np.array_equal(r[k], f[k]), (backend, k)
        finally:
            assert h.destroy() == OK
    assert answers[0][0] == code and answers[0] == answers[1], answers


GUARD_I, GUARD_D, PAD = -77, -7.5, 8


def guarded(dtype, *shape):
    """an array with PAD guard entries behind the first axis, everything set to the guard value"""
    return np.full((shape[0] + PAD,) + shape[1:], GUARD_I if np.issubdtype(dtype, np.integer) else GUARD_D, dtype=dtype)


def exactly_batch(a, written=True):
    guard = GUARD_I if np.issubdtype(a.dtype, np.integer) else GUARD_D
    assert (a[B:] == guard).all()     # nothing behind `batch` entries
    if written:
        assert (a[:B] != guard).all()
    return a[:B]


def counters(h, written=True):
    """every work counter of the handle; written=False: zero is an expected value, only the guards are checked"""
    c = {k: guarded(np.int64, B) for k in ("solves", "iters", "ok", "backward", "rollouts", "trials", "reused", "confirmed")}
    p = {k: v.ctypes.data_as(i64) for k, v in c.items()}
    h.get_solve_counters(p["solves"], p["iters"], p["ok"])
    h.get_work_counters(p["backward"], p["rollouts"], p["trials"])
    h.get_reuse_counter(p["reused"]), h.get_confirm_counter(p["confirmed"])
    return {k: exactly_batch(v, written) for k, v in c.items()}


@pytest.mark.parametrize("backend", BACKENDS)
def test_shared_reads(backend):
    n, m = NM
    h, twin = make(backend), make(backend)
    try:
        setup(h), setup(twin)
        h.solve()
        h.run_async(0, LOGCAP)       # one fused launch of three steps, logged, under the uploaded noise
        h.synchronize()
        # the launches are counted, and the reset takes the count and every counter back to zero
        count, ms = C.c_int32(-1), (C.c_float * 4)()
        h.timing_get(ms, 4, C.byref(count))
        assert count.value == 2 and ms[0] > 0 and ms[1] > 0
        h.last_solve_ms(_f32())
        c = counters(h)
        assert (c["solves"] == 1 + LOGCAP).all() and (c["iters"] >= c["solves"]).all()
        assert np.array_equal(c["iters"], c["backward"] + c["reused"] + c["confirmed"])
        # get_stats and get_alpha_trace fill `batch` entries
        st = dict(it=guarded(np.int32, B), ito=guarded(np.int32, B), status=guarded(np.int32, B), J=guarded(np.float64, B),
                  c=guarded(np.float64, B), Jt=guarded(np.float64, B, _lib.TRACE_LEN), ct=guarded(np.float64, B, _lib.TRACE_LEN))
        h.get_stats(I(st["it"]), I(st["ito"]), I(st["status"]), D(st["J"]), D(st["c"]), D(st["Jt"]), D(st["ct"]))
        for k in ("it", "ito", "status", "J", "c"):
            exactly_batch(st[k])
        exactly_batch(st["Jt"], written=False), exactly_batch(st["ct"], written=False)
        assert (st["Jt"][:B, 0] != GUARD_D).all() and (st["ct"][:B, 0] != GUARD_D).all()
        at = guarded(np.float64, B, _lib.TRACE_LEN)
        h.get_alpha_trace(D(at))
        exactly_batch(at, written=False)
        assert (at[:B] != GUARD_D).all()
        # the polish getters: zeros while the option is off
        ran, failed, dfail = guarded(np.int32, B), guarded(np.int32, B), guarded(np.int32, B)
        res, before, after = guarded(np.float64, B), guarded(np.float64, B), guarded(np.float64, B)
        h.get_polish_stats(I(ran), I(failed), D(res))
        h.get_polish_dual_residuals(D(before), D(after), I(dfail))
        for a in (ran, failed, dfail, res, before, after):
            assert (exactly_batch(a) == 0).all()
        # the log of the fused launch == what three single-step launches on the twin leave, byte for byte
        lg = dict(x0=np.zeros((LOGCAP, B, n)), u0=np.zeros((LOGCAP, B, m)), J=np.zeros((LOGCAP, B)), c=np.zeros((LOGCAP, B)))
        lgi = {k: np.zeros((LOGCAP, B), dtype=np.int32) for k in ("it", "ito", "status")}
        h.get_log(0, LOGCAP, D(lg["x0"]), D(lg["u0"]), I(lgi["it"]), I(lgi["ito"]), I(lgi["status"]), D(lg["J"]), D(lg["c"]))
        twin.solve()
        for s in range(LOGCAP):
            twin.step_async(s)
            twin.synchronize()
            x0, U = np.zeros((B, n)), np.zeros((B, N - 1, m))
            t = dict(J=np.zeros(B), c=np.zeros(B))
            ti = {k: np.zeros(B, dtype=np.int32) for k in ("it", "ito", "status")}
            twin.get_initial_state(D(x0)), twin.get_controls(D(U))
            twin.get_stats(I(ti["it"]), I(ti["ito"]), I(ti["status"]), D(t["J"]), D(t["c"]), None, None)
            assert lg["x0"][s].tobytes() == x0.tobytes() and lg["u0"][s].tobytes() == np.ascontiguousarray(U[:, 0]).tobytes(), s
            for k in t:
                assert lg[k][s].tobytes() == t[k].tobytes(), (s, k)
            for k in ti:
                assert np.array_equal(lgi[k][s], ti[k]), (s, k)
        # reset: no launches on record, every counter zero
        h.timing_reset()
        h.timing_get(ms, 4, C.byref(count))
        assert count.value == 0
        assert all((v == 0).all() for v in counters(h, written=False).values())
    finally:
        assert h.destroy() == OK and twin.destroy() == OK
