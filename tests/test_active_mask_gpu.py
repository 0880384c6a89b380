"""Per-instance active mask and cold restart (altro_batch_set_active, altro_batch_restart_instances and their _dev twins) on
the GPU.  Everything is compared with np.array_equal: an active instance under a mask equals the same library's unmasked
path on the same batch bit for bit, an inactive instance equals its own state before the call, a restarted instance equals
a freshly created handle.  B = 18 pads to five waves of the 16-lane kernels: instances 0-3, 4-7, 8-11, 12-15 and 16-17 plus
two padded slots."""
import ctypes as C

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc
from altro_mpc_icra2021_amd import problems as P
from helpers import REF_OPTS, ROCKET_COLD_OPTS, ROCKET_MPC_OPTS, rocket_gpu_problem

pytestmark = pytest.mark.gpu

B, S = 18, 8
BOX16 = [(12, 4, 21), (6, 6, 21), (8, 4, 21)]
WIDE = [(16, 4, 21), (12, 6, 21), (24, 4, 21), (30, 15, 21), (48, 4, 21)]
SWITCHES = ("ALTRO_NO_LONE", "ALTRO_NO_SHADOW", "ALTRO_NO_GROUP")


def mask(kind, nb=B):
    a = np.ones(nb, dtype=np.int32)
    off = {"a": [0, 2, 3],          # exactly one active row in a wave: the lone paths
           "b": [5],                # one inactive row among three active: the shadow paths
           "c": [8, 9, 10, 11],     # a wave with all four rows inactive
           "d": [16, 17],           # the last, partly padded wave with its only real rows inactive
           "abcd": [0, 2, 3, 5, 8, 9, 10, 11, 16, 17],
           "e": list(range(nb)), "f": []}[kind]
    a[off] = 0
    return a


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def snapshot(sv, factors=False):
    """every per-instance output of a handle, instance-major"""
    st = altro.stats(sv)
    K, d = altro.gains(sv)
    out = dict(X=altro.states(sv), U=altro.controls(sv), x0=altro.initial_state(sv), active=api.get_active(sv),
               it=st.iterations, ito=st.iterations_outer, status=st.status,
               cost=st.cost, cmax=st.c_max, Jt=st.cost_trace, ct=st.cmax_trace, alpha=altro.alpha_trace(sv), K=K, d=d,
               reuse=altro.reuse_counter(sv), confirm=altro.confirm_counter(sv))
    for i, a in enumerate(altro.work_counters(sv)):
        out["work%d" % i] = a
    for i, a in enumerate(altro.solve_counters(sv)):
        out["solves%d" % i] = a
    for c in range(len(sv.con_ids)):
        out["dual%d" % c] = altro.get_duals(sv, c)
    for i, a in enumerate(altro.polish_stats(sv)):
        out["polish%d" % i] = a
    for i, a in enumerate(altro.polish_dual_residuals(sv)):
        out["pdual%d" % i] = a
    if factors:
        out["F"] = altro.gain_factors(sv)
    return out


COUNTERS = ("work0", "work1", "work2", "solves0", "solves1", "solves2", "reuse", "confirm")


def assert_same(a, b, rows=None, what="", skip=("active",)):
    assert a.keys() == b.keys()
    for k in a:
        if k in skip:
            continue
        x, y = a[k], b[k]
        if rows is not None:
            x, y = x[rows], y[rows]
        assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (what, k)


def log_fields(lg):
    return dict(x0=lg.x0, u0=lg.u0, it=lg.iterations, ito=lg.iterations_outer, status=lg.status, cost=lg.cost, cmax=lg.c_max)


def assert_log(msk_log, ref_log, active, what=""):
    """active instances: every step's record equals the unmasked run's; inactive ones: every slot never written"""
    on, off = np.nonzero(active)[0], np.nonzero(active == 0)[0]
    a, r = log_fields(msk_log), log_fields(ref_log)
    for k in a:
        assert np.array_equal(a[k][:, on], r[k][:, on]), (what, "log", k)
        if a[k].dtype.kind == "f":
            assert np.all(np.isnan(a[k][:, off])), (what, "log slot written", k)
        else:
            assert np.all(a[k][:, off] == -1), (what, "log slot written", k)


_ref_cache = {}


def linear_batch(n, m, N, seed=21):
    return P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=seed)


def started(pb, opts=None, log=S):
    mp = mpc.BatchMPC(pb, opts=altro.SolverOptions(**(opts or REF_OPTS)))
    mp.initial_solve()
    if log:
        mp.enable_log(log)
    return mp


def reference(n, m, N):
    """the unmasked fused run of a shape, computed once and shared (never modified)"""
    key = (n, m, N)
    if key not in _ref_cache:
        mp = started(linear_batch(n, m, N))
        mp.run_async(S, first=0)
        mp.synchronize()
        _ref_cache[key] = (snapshot(mp.solver, (n, m, N) in BOX16), mp.log(0, S))
        mp.solver.close()
    return _ref_cache[key]


def check_masked(mp, pre, ref_snap, ref_log, active, factors, what):
    on, off = np.nonzero(active)[0], np.nonzero(active == 0)[0]
    post = snapshot(mp.solver, factors)
    assert np.array_equal(post["active"], active)
    assert_same(post, ref_snap, rows=on, what=(what, "active rows"))
    assert_same(post, pre, rows=off, what=(what, "inactive rows"))
    if ref_log is not None:
        assert_log(mp.log(0, S), ref_log, active, what)


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
@pytest.mark.parametrize("n,m,N,switch", [(n, m, N, None) for (n, m, N) in BOX16 + WIDE] + [(n, m, N, sw) for (n, m, N) in BOX16 for sw in SWITCHES])
def test_fused_mpc_under_a_mask(monkeypatch, n, m, N, switch, kind):
    ref_snap, ref_log = reference(n, m, N)
    if switch is not None:
        monkeypatch.setenv(switch, "1")
    factors = (n, m, N) in BOX16
    active = mask(kind)
    msk = started(linear_batch(n, m, N))
    msk.set_active(active)
    pre = snapshot(msk.solver, factors)
    msk.run_async(S, first=0)
    msk.synchronize()
    check_masked(msk, pre, ref_snap, ref_log, active, factors, (n, m, switch, kind))
    msk.solver.close()


@pytest.mark.parametrize("n,m,N", BOX16 + WIDE)
def test_single_steps_and_plain_calls_under_a_mask(n, m, N):
    """S calls of altro_mpc_step_async under a mask equal the unmasked fused run (hence the masked fused run too), and the
    fine-grained sequence prepare + shift_fill + solve equals the same sequence on an unmasked handle."""
    ref_snap, ref_log = reference(n, m, N)
    factors = (n, m, N) in BOX16
    active = mask("abcd")
    on, off = np.nonzero(active)[0], np.nonzero(active == 0)[0]
    pb = linear_batch(n, m, N)
    one = started(pb)
    one.set_active(active)
    pre = snapshot(one.solver, factors)
    for i in range(S):
        one.step_async(i)
    one.synchronize()
    check_masked(one, pre, ref_snap, ref_log, active, factors, (n, m, "single steps"))
    fused = started(pb)
    fused.set_active(active)
    fused.run_async(S, first=0)
    fused.synchronize()
    assert_same(snapshot(fused.solver, factors), snapshot(one.solver, factors), what="fused == single steps under a mask")
    assert_same(log_fields(fused.log(0, S)), log_fields(one.log(0, S)), what="logs, fused == single steps")
    one.solver.close(), fused.solver.close()
    plain, pref = started(pb, log=0), started(pb, log=0)
    plain.set_active(active)
    pre = snapshot(plain.solver, factors)
    for mp in (plain, pref):
        s = mp.solver
        for i in range(3):
            s._chk(s._L.altro_mpc_prepare_async(s.h, i))
            api.shift_fill(s, True, True)
            api.solve(s)
    post, want = snapshot(plain.solver, factors), snapshot(pref.solver, factors)
    assert_same(post, want, rows=on, what=(n, m, "plain calls, active rows"))
    assert_same(post, pre, rows=off, what=(n, m, "plain calls, inactive rows"))
    plain.solver.close(), pref.solver.close()


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (24, 4, 21)])
def test_all_inactive_all_active_and_clearing_the_mask(n, m, N):
    ref_snap, ref_log = reference(n, m, N)
    factors = (n, m, N) in BOX16
    pb = linear_batch(n, m, N)
    # (e) nothing is active: nothing changes; the launch is still a launch and takes its slot of the timing ring
    mp = started(pb)
    mp.set_active(mask("e"))
    pre = snapshot(mp.solver, factors)
    altro.timing_reset(mp.solver)
    pre = snapshot(mp.solver, factors)
    mp.run_async(S, first=0)
    mp.synchronize()
    assert len(altro.timing_get(mp.solver)) == 1
    check_masked(mp, pre, ref_snap, ref_log, mask("e"), factors, (n, m, "e"))
    mp.solver.close()
    # (f) an explicit mask of ones: the unmasked run everywhere
    mp = started(pb)
    mp.set_active(mask("f"))
    mp.run_async(S, first=0)
    mp.synchronize()
    assert_same(snapshot(mp.solver, factors), ref_snap, what=(n, m, "f"))
    assert_log(mp.log(0, S), ref_log, mask("f"), "f")
    mp.solver.close()
    # clearing the mask restores the default: rows active throughout stay equal to an unmasked handle over further steps
    pb2 = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S + 4, seed=21)
    a, r = started(pb2, log=0), started(pb2, log=0)
    active = mask("abcd")
    a.set_active(active)
    a.run_async(4, first=0), r.run_async(4, first=0)
    a.set_active(None)
    assert np.array_equal(api.get_active(a.solver), np.ones(B, dtype=np.int32))
    a.run_async(4, first=4), r.run_async(4, first=4)
    a.synchronize(), r.synchronize()
    assert_same(snapshot(a.solver, factors), snapshot(r.solver, factors), rows=np.nonzero(active)[0], what=(n, m, "cleared"))
    off = np.nonzero(active == 0)[0]
    assert np.all(altro.solve_counters(a.solver)[0][off] == 5)   # initial solve + the four steps after the mask went
    a.solver.close(), r.solver.close()


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (24, 4, 21)])
def test_polish_under_a_mask(n, m, N):
    opts = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    factors = (n, m, N) in BOX16
    pb = linear_batch(n, m, N)
    active = mask("b")
    ref, msk = started(pb, opts, log=3), started(pb, opts, log=3)
    msk.set_active(active)
    pre = snapshot(msk.solver, factors)
    for mp in (ref, msk):
        mp.run_async(3, first=0)
        mp.synchronize()
    rs = snapshot(ref.solver, factors)
    print("polish ran on", int(rs["polish0"].sum()), "of", B, "instances in the last step")
    on, off = np.nonzero(active)[0], np.nonzero(active == 0)[0]
    post = snapshot(msk.solver, factors)
    assert_same(post, rs, rows=on, what=(n, m, "polish, active rows"))
    assert_same(post, pre, rows=off, what=(n, m, "polish, inactive rows"))
    a, r = log_fields(msk.log(0, 3)), log_fields(ref.log(0, 3))
    for k in a:
        assert np.array_equal(a[k][:, on], r[k][:, on]), ("polish log", k)
        assert np.all(np.isnan(a[k][:, off])) if a[k].dtype.kind == "f" else np.all(a[k][:, off] == -1), ("polish log slot", k)
    ref.solver.close(), msk.solver.close()


def rocket_cold(nb=6):
    rp = P.gen_rocket_problem(N=41, tf=10.0, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
    x0 = np.tile(rp.x0, (nb, 1)) + 0.1 * np.random.default_rng(2).standard_normal((nb, rp.n))
    return rocket_gpu_problem(altro, rp, x0), altro.SolverOptions(**ROCKET_COLD_OPTS)


def test_conic_kernel_under_a_mask():
    prob, opts = rocket_cold()
    active = np.array([1, 0, 1, 1, 0, 1], dtype=np.int32)
    ref, msk = altro.ALTROSolver(prob, opts), altro.ALTROSolver(prob, opts)
    api.set_active(msk, active)
    pre = snapshot(msk, True)
    altro.solve(ref), altro.solve(msk)
    post, want = snapshot(msk, True), snapshot(ref, True)
    print("rocket: status", want["status"], "iterations", want["it"])
    assert np.all(want["it"] > 1)          # a real cold solve, not one that ends at its first rollout
    assert_same(post, want, rows=np.nonzero(active)[0], what="rocket, active rows")
    assert_same(post, pre, rows=np.nonzero(active == 0)[0], what="rocket, inactive rows")
    ref.close(), msk.close()


def diff_counters(after, before):
    out = dict(after)
    for k in COUNTERS:
        out[k] = after[k] - before[k]
    return out


RESTART_SEED = 12   # of seeds 1..24 one of those where, on both shapes, an instance of {0, 5, B-1} holds a nonzero box dual and has
                    # reused gains after the four steps (seed 21 of the other tests: none of the three on (12, 4, 21))


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (24, 4, 21)])
def test_restart_equals_a_fresh_handle(n, m, N):
    """initial solve + 4 MPC steps, then instances {0, 5, B-1} restart from their reference controls and a new x0: their next
    solve is that of a new handle given the same data (work counters as the difference across the solve), and the others
    equal a handle that ran the same sequence without the restart.  The batch is chosen so that a restarted instance holds
    nonzero box duals and has reused gains before the restart: with duals kept or gains not dropped the solves differ."""
    factors = (n, m, N) in BOX16
    pb = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=RESTART_SEED)
    sel = np.array([0, 5, B - 1])
    which = np.zeros(B, dtype=np.int32)
    which[sel] = 1
    a, c = started(pb, log=0), started(pb, log=0)
    for mp in (a, c):
        mp.run_async(4, first=0)
        mp.synchronize()
    before = snapshot(a.solver, factors)
    print("before the restart: max |box dual|", np.abs(before["dual0"][sel]).max(axis=(1, 2, 3)), "reuse", before["reuse"][sel])
    assert np.any((np.abs(before["dual0"][sel]).max(axis=(1, 2, 3)) > 0) & (before["reuse"][sel] > 0))
    Xr, Ur = pb.window(4)
    x0 = a.x0()
    x0[sel] = Xr[sel, 0] + 0.05 * np.random.default_rng(9).standard_normal((3, n))
    api.restart_instances(a.solver, which, Ur)
    after_restart = snapshot(a.solver, factors)
    others = np.nonzero(which == 0)[0]
    assert_same(after_restart, before, rows=others, what="the restart touched an instance it was not asked to")
    assert np.all(after_restart["status"][sel] == 0) and np.all(after_restart["it"][sel] == 0)
    assert not np.any(after_restart["dual0"][sel]) and np.array_equal(after_restart["U"][sel], Ur[sel])
    for k in COUNTERS:
        assert np.array_equal(after_restart[k], before[k]), ("the restart reset an accumulating counter", k)
    for mp in (a, c):
        api.set_initial_state(mp.solver, x0)
        api.solve(mp.solver)
    fresh = altro.ALTROSolver(mpc.gen_tracking_problem(pb), altro.SolverOptions(**REF_OPTS))
    api.update_trajectory(fresh, Xr, Ur)
    api.set_initial_state(fresh, x0)
    api.initial_controls(fresh, Ur)
    f0 = snapshot(fresh, factors)
    api.solve(fresh)
    got = diff_counters(snapshot(a.solver, factors), after_restart)
    assert_same(got, diff_counters(snapshot(fresh, factors), f0), rows=sel, what=(n, m, "restarted rows == fresh handle"))
    assert_same(snapshot(a.solver, factors), snapshot(c.solver, factors), rows=others, what=(n, m, "rows not restarted"))
    a.solver.close(), c.solver.close(), fresh.close()


def test_restart_on_the_conic_kernel():
    """The same on the rocket's tracking MPC (second-order cones, 16-lane conic kernel): instances {0, B-1} restart.  The conic
    kernels take no gains from memory, so what a restart must clear here are the duals: checked nonzero before it."""
    nb, Nm, Nt, dt = 6, 41, 301, 0.05
    rp = P.gen_rocket_problem(N=Nt, tf=(Nt - 1) * dt, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
    rng = np.random.default_rng(1)
    x0c = np.tile(rp.x0, (nb, 1)) + rng.standard_normal((nb, 6)) * np.array([1, 1, 1, .3, .3, .3]) * 0.5
    cold = altro.ALTROSolver(rocket_gpu_problem(altro, rp, x0c), altro.SolverOptions(**ROCKET_COLD_OPTS))
    altro.solve(cold)
    Xt, Ut = altro.states(cold), altro.controls(cold)
    cold.close()
    tp = P.gen_rocket_problem(N=Nm, tf=dt * (Nm - 1), include_goal=False, theta_thrust_max=5.0, theta_glideslope=45.0)
    tp.Q, tp.R, tp.Qf = np.full(6, 10.0), np.full(3, 0.1), np.full(6, 10.0)
    noise = rng.standard_normal((4, nb, 6))
    wts, grp = np.array([1e-3] * 3 + [1e-2] * 3), np.array([0, 0, 0, 1, 1, 1])
    opts = altro.SolverOptions(**ROCKET_MPC_OPTS)

    def problem(k, x0):
        return rocket_gpu_problem(altro, tp, x0, Xt[:, k:k + Nm].copy(), Ut[:, k:k + Nm - 1].copy(), U0=Ut[:, k:k + Nm - 1].copy())

    def make():
        mp = mpc.TrackMPC(problem(0, Xt[:, 0].copy()), opts, Xt, Ut, noise, (wts, grp))
        mp.initial_solve()
        mp.run_async(4, first=0)
        mp.synchronize()
        return mp
    a, c = make(), make()
    sel = np.array([0, nb - 1])
    which = np.zeros(nb, dtype=np.int32)
    which[sel] = 1
    others = np.nonzero(which == 0)[0]
    before = snapshot(a.solver, True)
    ncon = len(a.solver.con_ids)
    assert any(np.abs(before["dual%d" % q][sel]).max() > 0 for q in range(ncon))
    x0 = a.x0()
    x0[sel] = Xt[sel, 4] + 0.05 * rng.standard_normal((len(sel), 6))
    api.restart_instances(a.solver, which, Ut[:, 4:4 + Nm - 1].copy())
    after_restart = snapshot(a.solver, True)
    assert_same(after_restart, before, rows=others, what="rocket: the restart touched another instance")
    for mp in (a, c):
        api.set_initial_state(mp.solver, x0)
        api.solve(mp.solver)
    fresh = altro.ALTROSolver(problem(4, x0), opts)
    f0 = snapshot(fresh, True)
    api.solve(fresh)
    got = diff_counters(snapshot(a.solver, True), after_restart)
    assert_same(got, diff_counters(snapshot(fresh, True), f0), rows=sel, what="rocket: restarted rows == fresh handle")
    assert_same(snapshot(a.solver, True), snapshot(c.solver, True), rows=others, what="rocket: rows not restarted")
    a.solver.close(), c.solver.close(), fresh.close()


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (24, 4, 21)])
def test_device_twins_leave_the_same_state(n, m, N):
    factors = (n, m, N) in BOX16
    pb = linear_batch(n, m, N)
    active = mask("abcd")
    which = np.zeros(B, dtype=np.int32)
    which[[0, 4, 17]] = 1
    Xr, Ur = pb.window(3)
    hst, dvc = started(pb, log=0), started(pb, log=0)
    for mp in (hst, dvc):
        mp.run_async(3, first=0)
    api.set_active(hst.solver, active)
    api.set_active(dvc.solver, T(active))
    api.restart_instances(hst.solver, which, Ur, X=Xr)
    api.restart_instances(dvc.solver, T(which), T(Ur), X=T(Xr))
    assert_same(snapshot(hst.solver, factors), snapshot(dvc.solver, factors), skip=(), what="after the setters")
    for mp in (hst, dvc):
        mp.run_async(2, first=3)
        mp.synchronize()
    assert_same(snapshot(hst.solver, factors), snapshot(dvc.solver, factors), skip=(), what="after two masked steps")
    hst.solver.close(), dvc.solver.close()


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (24, 4, 21)])
def test_external_mpc_tick_with_changing_masks_equals_the_host_loop(n, m, N):
    """Six ticks whose `active` and `restart` tensors change from tick to tick, against a host loop of the same calls:
    setters, restart, shift under active & ~restart, solve under active."""
    factors = (n, m, N) in BOX16
    ticks = 6
    pb = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=ticks + 1, seed=33)
    rng = np.random.default_rng(4)
    act = (rng.random((ticks, B)) > 0.3).astype(np.int32)
    act[2] = mask("abcd")
    rst = (rng.random((ticks, B)) > 0.85).astype(np.int32)
    rst[3] = 0
    x0s = pb.Xtrack[:, 1:ticks + 1].transpose(1, 0, 2) + 0.02 * rng.standard_normal((ticks, B, n))
    opts = altro.SolverOptions(**REF_OPTS)
    hst, dvc = altro.ALTROSolver(mpc.gen_tracking_problem(pb), opts), altro.ALTROSolver(mpc.gen_tracking_problem(pb), opts)
    api.solve(hst), api.solve(dvc)
    ext = mpc.ExternalMPC(dvc)
    for i in range(ticks):
        Xr, Ur = (np.ascontiguousarray(v) for v in pb.window(i + 1))
        u0, x1, st, it = ext.tick(T(x0s[i]), T(Xr), T(Ur), active=T(act[i]), restart=T(rst[i]) if i != 3 else None)
        api.set_initial_state(hst, x0s[i])
        api.update_trajectory(hst, Xr, Ur)
        if i != 3:
            api.restart_instances(hst, rst[i], Ur)
        api.set_active(hst, act[i] & (1 - rst[i]))
        api.shift_fill(hst, True, True)
        api.set_active(hst, act[i])
        api.solve(hst)
        torch.cuda.synchronize()
        assert np.array_equal(u0.cpu().numpy(), altro.controls(hst)[:, 0]), ("u0 of tick", i)
        assert np.array_equal(st.cpu().numpy(), altro.stats(hst).status), ("status of tick", i)
    assert_same(snapshot(hst, factors), snapshot(dvc, factors), skip=(), what="after six ticks")
    hst.close(), dvc.close()


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (24, 4, 21)])
def test_refusals_change_nothing(n, m, N):
    """A host pointer, a device buffer one element too short, NULL which / U, a NULL handle: ALTRO_ERR_INVALID_ARG with a
    message, and the snapshot is the one before."""
    factors = (n, m, N) in BOX16
    pb = linear_batch(n, m, N)
    mp = started(pb, log=0)
    s = mp.solver
    L, INV = s._L, altro._lib.ERR_INVALID_ARG
    pre = snapshot(s, factors)
    gp = lambda t: C.c_void_p(t.data_ptr())
    host_i = np.ones(B, dtype=np.int32)
    host_U = np.zeros((B, N - 1, m))
    g_which, g_U = T(host_i), T(host_U)
    # the last bytes of the allocations that hold the tensors, one element short of what the calls read
    paths = altro._lib.hip_runtimes()
    assert len(paths) == 1, paths
    rt = C.CDLL(paths[0])
    rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]

    def short(t, nbytes, elem):
        base, size = C.c_void_p(), C.c_size_t()
        assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(t)) == 0 and size.value >= nbytes
        return C.c_void_p(base.value + size.value - (nbytes - elem))
    short_i, short_U = short(g_which, B * 4, 4), short(g_U, B * (N - 1) * m * 8, 8)

    def refused(rc, h=s):
        msg = (L.altro_last_error(h.h if h is not None else None) or b"").decode()
        assert rc == INV and msg, (rc, msg)
    refused(L.altro_batch_set_active_dev(s.h, C.c_void_p(host_i.ctypes.data)))
    refused(L.altro_batch_set_active_dev(s.h, short_i))
    refused(L.altro_batch_restart_instances_dev(s.h, C.c_void_p(host_i.ctypes.data), None, gp(g_U)))
    refused(L.altro_batch_restart_instances_dev(s.h, gp(g_which), None, C.c_void_p(host_U.ctypes.data)))
    refused(L.altro_batch_restart_instances_dev(s.h, short_i, None, gp(g_U)))
    refused(L.altro_batch_restart_instances_dev(s.h, gp(g_which), None, short_U))
    refused(L.altro_batch_restart_instances_dev(s.h, gp(g_which), short_U, gp(g_U)))     # X: far too short for [B][N][n]
    refused(L.altro_batch_restart_instances_dev(s.h, gp(g_which), None, None))
    refused(L.altro_batch_restart_instances_dev(s.h, None, None, gp(g_U)))
    ip = C.POINTER(C.c_int32)
    refused(L.altro_batch_restart_instances(s.h, host_i.ctypes.data_as(ip), None, None))
    refused(L.altro_batch_restart_instances(s.h, None, None, api._p(host_U)))
    refused(L.altro_batch_get_active(s.h, None))
    assert L.altro_batch_set_active_dev(None, gp(g_which)) == INV and L.altro_batch_restart_instances_dev(None, None, None, None) == INV
    assert_same(snapshot(s, factors), pre, skip=(), what="after the refusals")
    s.close()


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (24, 4, 21)])
def test_benchmark_solve_under_a_mask_is_a_state_error(n, m, N):
    mp = started(linear_batch(n, m, N), log=0)
    mp.set_active(mask("b"))
    with pytest.raises(altro.AltroError) as e:
        api.benchmark_solve(mp.solver, 1, 1)
    assert e.value.code == altro._lib.ERR_STATE
    mp.set_active(None)
    assert api.benchmark_solve(mp.solver, 1, 1).shape == (1,)
    mp.solver.close()
