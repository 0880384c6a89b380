"""GPU tests of the per-step MPC log (altro_mpc_set_log / altro_mpc_get_log).

The yardstick is the project's own invariant that a fused launch equals single steps bit for bit
(test_fused_multi_step_launch_is_bit_identical_to_single_steps): the record a step of a fused launch leaves must equal,
field for field and bit for bit, what the accessors return after the same step run on its own.  No tolerance is involved
except in the two checks against host FP64 arithmetic / the oracle, which use the 1e-12 bound test_mpc_loop_matches_oracle
uses for the same quantity."""
import ctypes as C

import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import problems as P
from helpers import REF_OPTS, ROCKET_COLD_OPTS, ROCKET_MPC_OPTS, make_oracle, mpc_update, quadruped_gpu_problem, rocket_gpu_problem

pytestmark = pytest.mark.gpu

FIELDS = ("x0", "u0", "iterations", "iterations_outer", "status", "cost", "c_max")


def single_step_chain(mp, S):
    """step(i) for i < S, reading after each step what the log is specified to hold"""
    rec = {f: [] for f in FIELDS}
    for i in range(S):
        mp.step(i)
        st = altro.stats(mp.solver)
        rec["x0"].append(mp.x0())
        rec["u0"].append(altro.controls(mp.solver)[:, 0].copy())
        for f in FIELDS[2:]:
            rec[f].append(getattr(st, f).copy())
    return {f: np.stack(v) for f, v in rec.items()}


def assert_log_equals(lg, rec, what=""):
    for f in FIELDS:
        a, b = getattr(lg, f), rec[f]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, f, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert np.array_equal(a, b), (what, f, bad[:4].tolist())


def fused_with_log(make, S, split=4):
    mp = make()
    mp.initial_solve()
    xs = mp.x0()
    mp.enable_log(S)
    mp.run_async(split, first=0)
    mp.run_async(S - split)
    mp.synchronize()
    return mp, xs


def chain_vs_log(make, S):
    a = make()
    a.initial_solve()
    rec = single_step_chain(a, S)
    b, xs = fused_with_log(make, S)
    lg = b.log()
    assert lg.steps == S
    assert_log_equals(lg, rec)
    # the handles themselves end in the same state, and X_traj is the start state followed by every step's x0
    assert np.array_equal(altro.states(a.solver), altro.states(b.solver)) and np.array_equal(a.x0(), b.x0())
    X = b.closed_loop_trajectory()
    assert X.shape == (S + 1,) + xs.shape and np.array_equal(X[0], xs) and np.array_equal(X[1:], rec["x0"])
    assert np.all(lg.iterations >= 1) and np.all(np.isfinite(lg.cost))
    return lg


# (12, 4, 50): 16-lane box kernel, B = 37 leaves three padded slots; (16, 4, 50) and (24, 4, 30): both gain-reuse classes of
# the wide kernel; (48, 4, 21): cooperative four-wave blocks
@pytest.mark.parametrize("n,m,N", [(12, 4, 50), (16, 4, 50), (24, 4, 30), (48, 4, 21)])
def test_log_equals_single_step_chain_random_linear(n, m, N):
    B, S = 37, 9
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=13)
    chain_vs_log(lambda: altro.mpc.BatchMPC(pb), S)


def _rocket_tracking(B, Nm, S, seed=1):
    """the set-up of test_gpu_parity._rocket_track_mpc without its oracles: cold solve N = 301, conic tracking problem"""
    Nt, dt = 301, 0.05
    rp = P.gen_rocket_problem(N=Nt, tf=(Nt - 1) * dt, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
    rng = np.random.default_rng(seed)
    x0 = np.tile(rp.x0, (B, 1)) + rng.standard_normal((B, 6)) * np.array([1, 1, 1, .3, .3, .3]) * 0.5
    cold = altro.ALTROSolver(rocket_gpu_problem(altro, rp, x0), altro.SolverOptions(**ROCKET_COLD_OPTS))
    altro.solve(cold)
    assert np.all(altro.stats(cold).status == 1)
    Xt, Ut = altro.states(cold), altro.controls(cold)
    cold.close()
    tp = P.gen_rocket_problem(N=Nm, tf=dt * (Nm - 1), include_goal=False, theta_thrust_max=5.0, theta_glideslope=45.0)
    tp.Q, tp.R, tp.Qf = np.full(6, 10.0), np.full(3, 0.1), np.full(6, 10.0)
    noise = rng.standard_normal((S, B, 6))
    wts, grp = np.array([1e-3] * 3 + [1e-2] * 3), np.array([0, 0, 0, 1, 1, 1])     # simple_rocket.jl:65-71

    def make():
        prob = rocket_gpu_problem(altro, tp, Xt[:, 0].copy(), Xt[:, :Nm].copy(), Ut[:, :Nm - 1].copy(), U0=Ut[:, :Nm - 1].copy())
        return altro.mpc.TrackMPC(prob, altro.SolverOptions(**ROCKET_MPC_OPTS), Xt, Ut, noise, (wts, grp))
    return make


def test_log_equals_single_step_chain_rocket_cones():
    """(6, 3, 21) with second-order cones through TrackMPC: the conic instantiation, two-group noise model"""
    S = 9
    chain_vs_log(_rocket_tracking(9, 21, S), S)


def test_log_equals_single_step_chain_quadruped_ltv():
    """the device-resident LTV loop of test_quadruped_ltv_mpc_runs_device_resident (altro_mpc_set_dynamics_track, N = 15): a
    16-lane size that has moved to the wide kernel"""
    B, S, N = 6, 5, 15
    qp = P.gen_quadruped_problem(N=N)
    rng = np.random.default_rng(7)
    t0 = rng.uniform(0.0, 0.8, B)
    x0 = qp.x_des + rng.standard_normal((B, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
    long = P.gen_quadruped_problem(N=S + N + 1)
    D = [long.dynamics(t) for t in t0]
    A, Bm, d = (np.stack([q[i] for q in D]) for i in range(3))
    noise = rng.standard_normal((S, B, 12))
    Nt = S + N + 1

    def make():
        prob = quadruped_gpu_problem(altro, qp, x0, A[:, :N - 1], Bm[:, :N - 1], d[:, :N - 1])
        mp = altro.mpc.TrackMPC(prob, altro.SolverOptions(**P.QUADRUPED_OPTS), np.tile(qp.x_des, (B, Nt, 1)), np.zeros((B, Nt - 1, 12)),
                                noise, (np.full(12, 1e-3),))
        altro.set_dynamics_track(mp.solver, A, Bm, d, step_stride=1)
        altro.initial_controls(mp.solver, np.tile(qp.u_hover, (B, N - 1, 1)))
        return mp

    a = make()
    a.initial_solve()
    rec = single_step_chain(a, S)
    b = make()
    b.initial_solve()
    b.enable_log(S)
    b.run_async(4, first=0)
    b.run_async(S - 4)
    b.synchronize()
    assert_log_equals(b.log(), rec)


def test_log_setting_survives_the_move_to_the_wide_kernel():
    """altro_mpc_set_log on a fresh handle of a 16-lane size, BEFORE altro_mpc_set_dynamics_track moves it to the
    one-wave-per-instance kernel: the handle keeps its log setting, capacity included, with every slot empty."""
    B, N, nb = 4, 15, 20
    L = altro._lib.lib()
    ip = C.POINTER(C.c_int32)
    h = C.c_void_p()
    dims = altro._lib.Dims(B, 12, 4, N)
    assert L.altro_batch_create(C.byref(dims), None, 0, C.byref(h)) == 0
    try:
        assert L.altro_mpc_set_log(h, 5) == 0
        rng = np.random.default_rng(3)
        Ak, Bk = 0.1 * rng.standard_normal((B, nb, 12, 12)), 0.1 * rng.standard_normal((B, nb, 4, 12))
        assert L.altro_mpc_set_dynamics_track(h, altro.api._p(Ak), altro.api._p(Bk), None, nb, 1, 1) == 0
        it = np.zeros((5, B), dtype=np.int32)
        x = np.zeros((5, B, 12))
        assert L.altro_mpc_get_log(h, 0, 5, altro.api._p(x), None, it.ctypes.data_as(ip), None, None, None, None) == 0
        assert np.all(it == -1) and np.all(np.isnan(x))
        assert L.altro_mpc_get_log(h, 0, 6, None, None, None, None, None, None, None) == altro._lib.ERR_INVALID_ARG
        assert L.altro_mpc_set_log(h, 0) == 0
        assert L.altro_mpc_get_log(h, 0, 1, None, None, None, None, None, None, None) == altro._lib.ERR_STATE
    finally:
        L.altro_batch_destroy(h)


def test_scheduling_cannot_touch_the_log(monkeypatch):
    """grouping permutes wave slots (nsteps >= 4), lone / shadow phases make lanes work for other rows, resync changes when
    a row works: records are keyed by the caller's instance index, so the logs are identical"""
    B, S = 150, 14
    pb = altro.problems.gen_random_linear_batch(B, steps=S, seed=31)

    def run():
        mp = altro.mpc.BatchMPC(pb)
        mp.initial_solve()
        mp.enable_log(S)
        mp.run_async(S, first=0)
        mp.synchronize()
        return mp.log()

    a = run()
    assert np.all(a.status == altro.SOLVE_SUCCEEDED)
    for var in ("ALTRO_NO_GROUP", "ALTRO_NO_LONE", "ALTRO_NO_SHADOW", "ALTRO_NO_RESYNC"):
        monkeypatch.setenv(var, "1")
        b = run()
        monkeypatch.delenv(var)
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), (var, f)
    # and they are the single-step chain's (no grouping there: one step per launch)
    c = altro.mpc.BatchMPC(pb)
    c.initial_solve()
    assert_log_equals(a, single_step_chain(c, S), "grouped launch")


@pytest.mark.parametrize("n,m,N", [(12, 4, 50), (24, 4, 30)])
def test_log_on_equals_log_off(n, m, N):
    B, S = 70, 9
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=13)
    out = []
    for on in (False, True):
        mp = altro.mpc.BatchMPC(pb)
        mp.initial_solve()
        altro.timing_reset(mp.solver)
        if on:
            mp.enable_log(S)
        mp.run_async(4, first=0)
        mp.run_async(S - 4)
        mp.synchronize()
        st = altro.stats(mp.solver)
        out.append([altro.states(mp.solver), altro.controls(mp.solver), altro.get_duals(mp.solver), mp.x0(), st.iterations,
                    st.iterations_outer, st.status, st.cost, st.c_max, st.cost_trace, st.cmax_trace,
                    *altro.solve_counters(mp.solver), *altro.work_counters(mp.solver), altro.confirm_counter(mp.solver),
                    altro.reuse_counter(mp.solver)])
    for k, (x, y) in enumerate(zip(*out)):
        assert np.array_equal(x, y), k


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (20, 4, 21)])
def test_log_in_the_polish_loop(n, m, N):
    """projected_newton = 1 (the two cases of test_projected_newton_polish_inside_the_mpc_loop): the logged u0 is the POLISHED
    first control, the statistics are those altro_batch_get_stats reports after each single step"""
    B, S = 5, 6
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=87)
    pb.u_bnd = 1.0
    opts = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    a = altro.mpc.BatchMPC(pb, altro.SolverOptions(**opts))
    a.initial_solve()
    rec = {f: [] for f in FIELDS}
    nran = 0
    for i in range(S):
        a.step(i)
        st = altro.stats(a.solver)
        nran += int(altro.polish_stats(a.solver)[0].sum())
        rec["x0"].append(a.x0()); rec["u0"].append(altro.controls(a.solver)[:, 0].copy())
        for f in FIELDS[2:]:
            rec[f].append(getattr(st, f).copy())
    rec = {f: np.stack(v) for f, v in rec.items()}
    assert nran >= B * S - 2                                         # the polish really ran
    b = altro.mpc.BatchMPC(pb, altro.SolverOptions(**opts))
    b.initial_solve()
    b.enable_log(S)
    b.run_async(4, first=0)
    b.run_async(S - 4)
    b.synchronize()
    assert_log_equals(b.log(), rec)


def test_closed_loop_is_consistent_and_matches_the_oracle(oracle):
    """(12, 4, 50), B = 10, S = 8, seed 11, as test_mpc_loop_matches_oracle.  (a) on the host in FP64,
    x0[s+1] == A x0[s] + B u0[s] + noise[s+1] ||.||_inf / 100: the logged u0 is the control the plant step applied;
    (b) iterations and status of every step equal the oracle loop's, x0 within 1e-12."""
    B, S = 10, 8
    pb = altro.problems.gen_random_linear_batch(B, n=12, m=4, N=50, steps=S, seed=11)
    mp = altro.mpc.BatchMPC(pb)
    mp.initial_solve()
    mp.enable_log(S)
    mp.run_async(S, first=0)
    mp.synchronize()
    lg = mp.log()
    worst = 0.0
    for s in range(S - 1):
        xn = np.einsum("bij,bj->bi", pb.A, lg.x0[s]) + np.einsum("bij,bj->bi", pb.Bm, lg.u0[s])
        xn = xn + pb.noise[s + 1] * np.abs(xn).max(axis=1, keepdims=True) / 100.0
        r = np.abs(lg.x0[s + 1] - xn).max(axis=1) / np.maximum(1.0, np.abs(xn).max(axis=1))
        worst = max(worst, r.max())
        assert np.all(r <= 1e-12), (s, r.max())
    print("closed-loop residual of the logged (x0, u0): %.2e" % worst)
    orcs = [make_oracle(oracle, pb, b) for b in range(B)]
    for o in orcs:
        o.solve()
    for i in range(S):
        for b, o in enumerate(orcs):
            x0 = mpc_update(o, pb, b, i)
            so = o.solve()
            assert np.abs(x0 - lg.x0[i, b]).max() <= 1e-12 * max(1.0, np.abs(x0).max()), (i, b)
            assert int(lg.iterations[i, b]) == so.iterations and int(lg.status[i, b]) == so.status, (i, b)
            assert int(lg.iterations_outer[i, b]) == so.iterations_outer, (i, b)


@pytest.mark.parametrize("n,m,N", [(12, 4, 50), (20, 4, 21)])
def test_log_edges(n, m, N):
    B, S = 6, 8
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=5)
    mp = altro.mpc.BatchMPC(pb)
    s = mp.solver
    L = s._L
    with pytest.raises(altro.AltroError) as e:       # no log set
        mp.log(0, 1)
    assert e.value.code == altro._lib.ERR_STATE
    assert L.altro_mpc_set_log(s.h, -1) == altro._lib.ERR_INVALID_ARG
    mp.initial_solve()
    mp.enable_log(5)
    lg = mp.log(0, 5)                                 # a plain solve wrote nothing: every slot empty
    assert np.all(lg.iterations == -1) and np.all(lg.iterations_outer == -1) and np.all(lg.status == -1)
    for a in (lg.x0, lg.u0, lg.cost, lg.c_max):
        assert np.all(np.isnan(a))
    for first, ns in ((0, 6), (5, 1), (-1, 1), (3, 3)):
        with pytest.raises(altro.AltroError) as e:
            mp.log(first, ns)
        assert e.value.code == altro._lib.ERR_INVALID_ARG
    # prepare_async and benchmark_solve leave the log untouched
    other = altro.mpc.BatchMPC(pb)
    other.initial_solve()
    other.enable_log(5)
    other.step_benchmark(0, samples=1, evals=1)
    assert np.all(other.log(0, 5).iterations == -1) and np.all(np.isnan(other.log(0, 5).x0))
    # steps 0..2 written, 3..4 still empty
    mp.run_async(3, first=0)
    mp.synchronize()
    lg = mp.log(0, 5)
    assert np.all(lg.iterations[:3] >= 1) and np.all(lg.status[:3] == 1) and np.all(np.isfinite(lg.x0[:3]))
    assert np.all(lg.iterations[3:] == -1) and np.all(np.isnan(lg.x0[3:])) and np.all(np.isnan(lg.cost[3:]))
    assert mp.log().steps == 3                        # default range: up to the step the loop has reached
    # past the capacity: refused, nothing enqueued
    before = [c.copy() for c in altro.solve_counters(s)] + [mp.x0()]
    for first, ns in ((3, 3), (5, 1)):
        assert L.altro_mpc_run_async(s.h, first, ns) == altro._lib.ERR_INVALID_ARG
    assert L.altro_mpc_step_async(s.h, 5) == altro._lib.ERR_INVALID_ARG
    after = [c.copy() for c in altro.solve_counters(s)] + [mp.x0()]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    lg2 = mp.log(0, 5)
    assert all(np.array_equal(getattr(lg2, f)[:3], getattr(lg, f)[:3]) for f in FIELDS)
    # running a step again overwrites its slot: step 2 from the state after step 2 is another solve
    mp.run_async(1, first=2)
    mp.synchronize()
    lg3 = mp.log(0, 5)
    assert all(np.array_equal(getattr(lg3, f)[:2], getattr(lg, f)[:2]) for f in FIELDS)
    assert not np.array_equal(lg3.x0[2], lg.x0[2]) and np.array_equal(lg3.x0[2], mp.x0())
    assert np.array_equal(lg3.u0[2], altro.controls(s)[:, 0])
    # log off again: run_async works as before, beyond the old capacity too, and get_log is a state error
    mp.enable_log(0)
    mp.run_async(3, first=3)
    mp.synchronize()
    assert np.all(altro.stats(s).status == 1)
    with pytest.raises(altro.AltroError) as e:
        mp.log(0, 1)
    assert e.value.code == altro._lib.ERR_STATE


def test_benchmark_functions_with_fused_launches():
    from altro_mpc_icra2021_amd import benchmarks as Bm
    a = Bm.run_random_linear(batch=64, steps=12, launch_steps=1)
    b = Bm.run_random_linear(batch=64, steps=12, launch_steps=4)
    assert np.array_equal(a["iter"], b["iter"]) and np.array_equal(a["solve_succeeded"], b["solve_succeeded"])
    assert b["launch_steps"] == 4 and "launch_steps" not in a and len(b["time"]) == 3 and len(a["time"]) == 12
    assert np.all(np.asarray(b["time"]) > 0)
    kw = dict(batch=8, N_mpc=21, steps=6, N_cold=61, dt=0.25)
    a = Bm.run_rocket(**kw)
    b = Bm.run_rocket(launch_steps=4, **kw)
    assert np.array_equal(a["iter"], b["iter"]) and np.array_equal(a["solve_succeeded"], b["solve_succeeded"])
    assert b["launch_steps"] == 4 and len(b["time"]) == 2
    assert Bm.summarise(b)["launch_steps"] == 4
