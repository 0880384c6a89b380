"""Per-instance episode clock (altro_mpc_set_clock, its _dev twin, altro_mpc_get_clock, BatchMPC.respawn) on the GPU.

The yardstick is always the same library's path WITHOUT a clock: a second handle runs initial_solve and then steps 0, 1, ...
one at a time, with the noise table re-indexed per instance (row l of instance b = the absolute row the clocked instance
meets at its local step l).  A clocked instance at absolute step i must equal the yardstick's step i - start[b] bit for bit
-- the log record of every step, and after the last step the full snapshot() of test_active_mask_gpu.py (X, U, x0, duals,
statistics, traces, gains, counters) against the yardstick's snapshot after as many steps as the instance ticked.  An
instance that never ticks equals its own snapshot before the launch, and every slot of a step it is idle at is never written.
Every comparison is np.array_equal.  B = 6 pads to two waves of the 16-lane kernels: four real rows, then two real rows and
two padded slots."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import api, mpc
from altro_mpc_icra2021_amd import problems as P
from helpers import REF_OPTS, ROCKET_COLD_OPTS, ROCKET_MPC_OPTS, quadruped_gpu_problem, rocket_gpu_problem
from test_active_mask_gpu import COUNTERS, assert_same, log_fields, snapshot

pytestmark = pytest.mark.gpu

B, N, S = 6, 11, 8
START = [0, 2, 0, 3, 1, 0]      # wave 0: rows falling out of step with each other; wave 1: one late row beside padded slots
LENGTH = [8, 3, 8, 1, 0, 5]
BOX16 = [(12, 4), (6, 6)]
WIDE = [(16, 4), (24, 4), (48, 4)]
PN_OPTS = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


# ---- the makers: noise (steps, B, n) -> a loop object with initial_solve / step / run_async / log
class Case:
    """make(noise) builds a fresh loop on the case's data; n: state dimension; Nt: knots of its track; dyn: (nblocks, stride)
    of its dynamics track or None; factors: snapshot() may read the gain factors (16-lane box kernels)"""

    def __init__(self, make, n, Nt, noise, dyn=None, factors=False, horizon=N):
        self.make, self.n, self.Nt, self.noise, self.dyn, self.factors, self.N = make, n, Nt, noise, dyn, factors, horizon
        self.yard = {}


_cases = {}


def linear_case(n, m, opts=None, Nt=None, extra=0):
    key = ("lin", n, m, tuple(sorted((opts or {}).items())), Nt, extra)
    if key not in _cases:
        pb = P.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S + extra, seed=21)
        if Nt is not None:
            pb = dataclasses.replace(pb, Xtrack=pb.Xtrack[:, :Nt].copy(), Utrack=pb.Utrack[:, :Nt - 1].copy())
        o = opts or REF_OPTS
        _cases[key] = Case(lambda nz: mpc.BatchMPC(dataclasses.replace(pb, noise=nz), opts=altro.SolverOptions(**o)), n, pb.Nt,
                           pb.noise, factors=(n, m) in BOX16)
    return _cases[key]


def rocket_case():
    """(6, 3) with second-order cones through TrackMPC: the conic 16-lane instantiation, two-group noise model"""
    if "rocket" not in _cases:
        Nt, dt = 301, 0.05
        rp = P.gen_rocket_problem(N=Nt, tf=(Nt - 1) * dt, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
        rng = np.random.default_rng(1)
        x0 = np.tile(rp.x0, (B, 1)) + rng.standard_normal((B, 6)) * np.array([1, 1, 1, .3, .3, .3]) * 0.5
        cold = altro.ALTROSolver(rocket_gpu_problem(altro, rp, x0), altro.SolverOptions(**ROCKET_COLD_OPTS))
        altro.solve(cold)
        Xt, Ut = altro.states(cold), altro.controls(cold)
        cold.close()
        tp = P.gen_rocket_problem(N=N, tf=dt * (N - 1), include_goal=False, theta_thrust_max=5.0, theta_glideslope=45.0)
        tp.Q, tp.R, tp.Qf = np.full(6, 10.0), np.full(3, 0.1), np.full(6, 10.0)
        noise = rng.standard_normal((S, B, 6))
        wts, grp = np.array([1e-3] * 3 + [1e-2] * 3), np.array([0, 0, 0, 1, 1, 1])

        def make(nz):
            prob = rocket_gpu_problem(altro, tp, Xt[:, 0].copy(), Xt[:, :N].copy(), Ut[:, :N - 1].copy(), U0=Ut[:, :N - 1].copy())
            return mpc.TrackMPC(prob, altro.SolverOptions(**ROCKET_MPC_OPTS), Xt, Ut, nz, (wts, grp))
        _cases["rocket"] = Case(make, 6, Nt, noise)
    return _cases["rocket"]


def ltv_case(nd=None):
    """the quadruped over altro_mpc_set_dynamics_track at step_stride = 1: every block of the track differs, so only the block
    index r = l + 1 of the instance's LOCAL step reproduces the yardstick.  nd: blocks of the dynamics track (default: as many
    as the reference track has knots, so the reference track ends first; fewer: the dynamics track does)"""
    if "ltv-data" not in _cases:
        qp = P.gen_quadruped_problem(N=N)
        rng = np.random.default_rng(7)
        t0 = rng.uniform(0.0, 0.8, B)
        x0 = qp.x_des + rng.standard_normal((B, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
        nb = S + N + 1
        D = [P.gen_quadruped_problem(N=nb).dynamics(t) for t in t0]
        A, Bm, d = (np.stack([q[i] for q in D]) for i in range(3))
        _cases["ltv-data"] = (qp, x0, nb, A, Bm, d, rng.standard_normal((S, B, 12)))
    qp, x0, nb, A, Bm, d, noise = _cases["ltv-data"]
    nd = A.shape[1] if nd is None else nd
    if ("ltv", nd) not in _cases:
        def make(nz):
            prob = quadruped_gpu_problem(altro, qp, x0, A[:, :N - 1], Bm[:, :N - 1], d[:, :N - 1])
            mp = mpc.TrackMPC(prob, altro.SolverOptions(**P.QUADRUPED_OPTS), np.tile(qp.x_des, (B, nb, 1)), np.zeros((B, nb - 1, 12)),
                              nz, (np.full(12, 1e-3),))
            altro.set_dynamics_track(mp.solver, A[:, :nd].copy(), Bm[:, :nd].copy(), d[:, :nd].copy(), step_stride=1)
            altro.initial_controls(mp.solver, np.tile(qp.u_hover, (B, N - 1, 1)))
            return mp
        _cases[("ltv", nd)] = Case(make, 12, nb, noise, dyn=(nd, 1))
    return _cases[("ltv", nd)]


# ---- the tick rule, restated independently of the library (include/altro_batch.h, altro_mpc_set_clock)
def ticks(case, start, length, i):
    """(B,) bool: the instances that tick at absolute step i"""
    out = np.zeros(B, dtype=bool)
    for b in range(B):
        l = i - start[b]
        ok = l >= 0 and (length is None or l < length[b]) and l + 1 + case.N <= case.Nt
        if ok and case.dyn is not None:
            ok = (l + 1) * case.dyn[1] + case.N - 2 < case.dyn[0]
        out[b] = ok
    return out


def noise_rows(start, nl):
    """rows[b][l]: the absolute noise row instance b meets at local step l"""
    return [[start[b] + l for l in range(nl)] for b in range(B)]


def yardstick(case, rows, nl):
    """the unclocked handle: initial_solve, then nl single steps; (snapshots after 0 .. nl steps, log of the nl steps).
    Its noise row l of instance b is the case's row rows[b][l] (zero where the clocked run never gets there).  Computed once
    per (case, rows) and never modified."""
    key = (tuple(map(tuple, rows)), nl)
    if key not in case.yard:
        nz = np.zeros((nl, B, case.n))
        for b in range(B):
            for l in range(nl):
                if 0 <= rows[b][l] < case.noise.shape[0]:
                    nz[l, b] = case.noise[rows[b][l], b]
        y = case.make(nz)
        y.initial_solve()
        y.enable_log(nl)
        snaps = [snapshot(y.solver, case.factors)]
        for l in range(nl):
            y.step(l)
            snaps.append(snapshot(y.solver, case.factors))
        case.yard[key] = (snaps, log_fields(y.log(0, nl)))
        y.solver.close()
    return case.yard[key]


def clocked(case, start, length=None, dev=False, log=S):
    c = case.make(case.noise)
    c.initial_solve()
    c.enable_log(log)
    if dev:
        c.set_clock(T(np.asarray(start, dtype=np.int32)), None if length is None else T(np.asarray(length, dtype=np.int32)))
    else:
        c.set_clock(np.asarray(start), None if length is None else np.asarray(length))
    return c


def never_written(rec, i, b):
    for k, a in rec.items():
        v = a[i, b]
        if not (np.all(np.isnan(v)) if a.dtype.kind == "f" else np.all(v == -1)):
            return False
    return True


def yard_for(case, start, length, nsteps=S):
    """(ticks (steps, B), yardstick snapshots, yardstick log): the yardstick runs as many steps as the busiest instance ticks"""
    tk = np.array([ticks(case, start, length, i) for i in range(nsteps)])
    nl = max(int(tk.sum(0).max()), 1)
    return (tk,) + yardstick(case, noise_rows(start, nl), nl)


def check(case, c, pre, start, length, nsteps=S, what="", skip=("active",)):
    """the clocked handle c after absolute steps 0 .. nsteps-1 from its initial solve, against the yardstick"""
    tk, snaps, ylog = yard_for(case, start, length, nsteps)
    post, rec = snapshot(c.solver, case.factors), log_fields(c.log(0, nsteps))
    print(what, "ticks per instance", tk.sum(0).tolist())
    for b in range(B):
        nt = int(tk[:, b].sum())
        assert_same(post, snaps[nt] if nt else pre, rows=[b], what=(what, "state", b, nt), skip=skip)
        for i in range(nsteps):
            if tk[i, b]:
                for k in rec:
                    assert np.array_equal(rec[k][i, b], ylog[k][i - start[b], b]), (what, "log", k, "step", i, "instance", b)
            else:
                assert never_written(rec, i, b), (what, "slot written", i, b)
    st, ln, win = api.get_clock(c.solver)
    assert np.array_equal(st, start) and np.array_equal(ln, np.full(B, -1) if length is None else np.maximum(length, 0))
    for b in range(B):   # the window is that of the last tick, or the one the instance held
        last = [i for i in range(nsteps) if tk[i, b]]
        assert win[b] == (last[-1] - start[b] + 1 if last else 0), (what, "window", b)


def run_fused_and_chain(case, start, length=None, what="", dev=False):
    f, s1 = clocked(case, start, length, dev), clocked(case, start, length, dev)
    pre = snapshot(f.solver, case.factors)
    f.run_async(S, first=0)
    f.synchronize()
    for i in range(S):
        s1.step_async(i)
    s1.synchronize()
    check(case, f, pre, start, length, what=(what, "fused"))
    check(case, s1, pre, start, length, what=(what, "single steps"))
    assert_same(snapshot(f.solver, case.factors), snapshot(s1.solver, case.factors), what=(what, "fused == chain"))
    return f, s1


ALL_CASES = [("lin", 12, 4), ("lin", 6, 6), ("rocket", 6, 3), ("lin", 16, 4), ("lin", 24, 4), ("lin", 48, 4), ("ltv", 12, 12)]


def get_case(kind, n, m):
    return linear_case(n, m) if kind == "lin" else rocket_case() if kind == "rocket" else ltv_case()


@pytest.mark.parametrize("kind,n,m", ALL_CASES)
def test_staggered_starts(kind, n, m):
    """1. start = [0, 2, 0, 3, 1, 0]: one fused launch and S single steps are equal, and each equals the yardstick per
    instance; slots i < start[b] are never written (check()).  Clearing the clock is refused while the windows differ."""
    case = get_case(kind, n, m)
    f, s1 = run_fused_and_chain(case, START, what=(kind, n, m))
    L = f.solver._L
    assert L.altro_mpc_set_clock(f.solver.h, None, None) == altro._lib.ERR_STATE
    assert (L.altro_last_error(f.solver.h) or b"").decode()
    assert np.array_equal(api.get_clock(f.solver)[0], START)       # still set
    assert L.altro_batch_benchmark_solve(f.solver.h, 1, 1, None) == altro._lib.ERR_STATE
    f.solver.close(), s1.solver.close()


@pytest.mark.parametrize("kind,n,m", ALL_CASES)
def test_ragged_ends_by_length(kind, n, m):
    """2a. length = [8, 3, 8, 1, 0, 5]: after an instance's last tick every later slot is never written and its state is
    frozen; the instance with length 0 is untouched for the whole launch, counters included."""
    case = get_case(kind, n, m)
    f, s1 = run_fused_and_chain(case, START, LENGTH, what=(kind, n, m, "length"))
    f.solver.close(), s1.solver.close()


@pytest.mark.parametrize("n,m", [(12, 4), (16, 4), (48, 4)])
def test_ragged_ends_by_the_track(n, m):
    """2b. no length, a track of N + 5 knots: local steps 0 .. 4 fit, so the instances that started early run off its end
    in mid-launch -- which ends their episode and is no error, while the same launch on a handle without a clock is refused"""
    case = linear_case(n, m, Nt=N + 5, extra=3)
    f, s1 = run_fused_and_chain(case, START, what=(n, m, "track end"))
    assert int(np.sum([ticks(case, START, None, S - 1)])) < B
    plain = case.make(case.noise)
    plain.initial_solve()
    with pytest.raises(altro._lib.AltroError):
        plain.run_async(S, first=0)
    for mp in (f, s1, plain):
        mp.solver.close()


def test_ragged_ends_by_the_dynamics_track():
    """2c. a dynamics track of N + 4 blocks under a reference track of S + N + 1 knots: window l + 1 needs blocks up to
    l + N - 1, so local steps 0 .. 4 tick and the DYNAMICS track, not the reference track, ends the episodes of the instances
    that started early, in mid-launch"""
    case = ltv_case(nd=N + 4)
    at_end = ticks(case, START, None, S - 1)
    case.dyn, keep = None, case.dyn
    by_ref_track = ticks(case, START, None, S - 1)
    case.dyn = keep
    assert by_ref_track.all() and at_end.sum() == 1, (by_ref_track, at_end)      # the block bound alone decides
    f, s1 = run_fused_and_chain(case, START, what=("ltv", "dynamics track end"))
    assert api.get_clock(f.solver)[2].max() == 5
    f.solver.close(), s1.solver.close()


@pytest.mark.parametrize("kind,n,m", [("lin", 12, 4), ("lin", 6, 6), ("lin", 24, 4)])
def test_a_whole_wave_idle_and_a_lone_ticking_row(kind, n, m):
    """3. rows 0-3 idle for the entire launch, exactly one row of the second wave ticking"""
    case = get_case(kind, n, m)
    start = [100, 100, 100, 100, 1, 100]
    f, s1 = run_fused_and_chain(case, start, what=(n, m, "lone"))
    f.solver.close(), s1.solver.close()


@pytest.mark.parametrize("switch", ["ALTRO_NO_GROUP", "ALTRO_NO_LONE", "ALTRO_NO_SHADOW", "ALTRO_NO_RESYNC", "ALTRO_NO_PAIR"])
def test_scheduling_switches_change_nothing(monkeypatch, switch):
    """4. case 1 with one scheduling feature of the 16-lane kernels off: the yardstick (computed with all of them on) holds"""
    case = linear_case(12, 4)
    yard_for(case, START, LENGTH)      # (with the defaults, before the switch goes into the environment)
    monkeypatch.setenv(switch, "1")
    f, s1 = run_fused_and_chain(case, START, LENGTH, what=switch)
    f.solver.close(), s1.solver.close()


@pytest.mark.parametrize("n,m", [(12, 4), (24, 4)])
def test_clock_and_mask_together(n, m):
    """5. instance 2 is masked out for the 3-step launch 2 .. 4 in mid-episode: its slots of those steps are never written and
    get_clock shows the window it held; unmasked, with its start moved by the three steps it sat out, it resumes at that
    window -- it equals the yardstick whose noise rows for it are 0, 1, 5, 6, 7."""
    case = linear_case(n, m)
    start = np.array(START)
    c = clocked(case, start)
    c.run_async(2, first=0)
    held = api.get_clock(c.solver)[2]
    assert held[2] == 2
    m_ = np.ones(B, dtype=np.int32)
    m_[2] = 0
    c.set_active(m_)
    c.synchronize()
    pre2 = snapshot(c.solver, case.factors)
    c.run_async(3, first=2)
    c.synchronize()
    assert_same(snapshot(c.solver, case.factors), pre2, rows=[2], what="masked, mid-episode")
    win = api.get_clock(c.solver)[2]
    assert win[2] == 2 and np.array_equal(np.delete(win, 2), np.delete(np.maximum(5 - start, 0), 2)), win
    c.set_active(None)
    start2 = start.copy()
    start2[2] += 3
    c.set_clock(start2)
    c.run_async(3, first=5)
    c.synchronize()
    rows = noise_rows(START, S)
    rows[2] = [0, 1, 5, 6, 7, 8, 9, 10]
    snaps, ylog = yardstick(case, rows, S)
    post, rec = snapshot(c.solver, case.factors), log_fields(c.log(0, S))
    for b in range(B):
        nt = 5 if b == 2 else S - START[b]
        assert_same(post, snaps[nt], rows=[b], what=("mask + clock", b))
        for i in range(S):
            l = rows[b].index(i) if i in rows[b][:nt] else None
            if l is None:
                assert never_written(rec, i, b), ("slot written", i, b)
            else:
                for k in rec:
                    assert np.array_equal(rec[k][i, b], ylog[k][l, b]), ("log", k, i, b)
    assert np.array_equal(api.get_clock(c.solver)[2], [8, 6, 5, 5, 7, 8])
    c.solver.close()


@pytest.mark.parametrize("n,m", [(12, 4), (24, 4)])
def test_polish_in_the_loop(n, m):
    """6. projected_newton = 1 (one solve kernel and one polish per step): equal to the yardstick, and at every step the
    instances idle AT THAT STEP keep everything, polish statistics included"""
    case = linear_case(n, m, opts=PN_OPTS)
    c = clocked(case, START, LENGTH)
    pre = prev = snapshot(c.solver, case.factors)
    for i in range(S):
        c.step(i)
        now = snapshot(c.solver, case.factors)
        idle = np.nonzero(~ticks(case, START, LENGTH, i))[0]
        assert_same(now, prev, rows=idle, what=("polish: idle at step", i))
        prev = now
    print("polish ran on", int(prev["polish0"].sum()), "instances in their last step")
    check(case, c, pre, START, LENGTH, what=(n, m, "polish chain"))
    f = clocked(case, START, LENGTH)
    f.run_async(S, first=0)
    f.synchronize()
    check(case, f, pre, START, LENGTH, what=(n, m, "polish fused"))
    c.solver.close(), f.solver.close()


@pytest.mark.parametrize("n,m", [(12, 4), (24, 4)])
def test_respawn_recipe(n, m):
    """7. four steps, respawn(which = [1, 4], x0 = new, at_step = 4), four more: the respawned instances' records of steps
    4 .. 7 are those of a FRESH handle's initial solve and steps 0 .. 3 on the same data with noise rows 4 .. 7 (the restart
    contract, carried through the clock); the others equal an undisturbed run."""
    case = linear_case(n, m)
    which = [1, 4]
    rng = np.random.default_rng(5)
    c = case.make(case.noise)
    c.initial_solve()
    c.enable_log(S)
    c.set_clock(np.zeros(B, dtype=np.int32))
    c.run_async(4, first=0)
    c.synchronize()
    xnew = c.x0()[which] + 0.05 * rng.standard_normal((2, case.n))
    c.respawn(which, xnew, at_step=4)
    st, ln, win = api.get_clock(c.solver)
    assert np.array_equal(st, [0, 4, 0, 0, 4, 0]) and np.array_equal(win, [4, 0, 4, 4, 0, 4]) and np.all(ln == -1)
    assert np.all(api.get_active(c.solver) == 1)
    c.run_async(4, first=4)
    c.synchronize()
    post, rec = snapshot(c.solver, case.factors), log_fields(c.log(0, S))
    # the fresh handle
    nz = np.zeros((4, B, case.n))
    nz[:, which] = case.noise[4:8][:, which]
    fr = case.make(nz)
    x0 = fr.x0()
    x0[which] = xnew
    api.set_initial_state(fr.solver, x0)
    fr.initial_solve()
    fr.enable_log(4)
    fr.run_async(4, first=0)
    fr.synchronize()
    frec = log_fields(fr.log(0, 4))
    for k in rec:
        assert np.array_equal(rec[k][4:8][:, which], frec[k][:, which]), ("respawned log", k)
    assert_same(post, snapshot(fr.solver, case.factors), rows=which, what="respawned state", skip=("active",) + COUNTERS)
    # the others: an undisturbed run of eight steps
    _, snaps, ylog = yard_for(case, [0] * B, None)
    others = [b for b in range(B) if b not in which]
    assert_same(post, snaps[S], rows=others, what="undisturbed state")
    for k in rec:
        assert np.array_equal(rec[k][:, others], ylog[k][:, others]), ("undisturbed log", k)
        assert np.array_equal(rec[k][:4][:, which], ylog[k][:4][:, which]), ("first life", k)
    c.solver.close(), fr.solver.close()


@pytest.mark.parametrize("n,m", [(12, 4), (24, 4)])
def test_device_twin(n, m):
    """8. set_clock from int32 torch tensors leaves the results of case 1 (with lengths); a host pointer, a buffer one element
    short and (where there is one) memory of another device are refused, nothing changes and the handle stays usable"""
    case = linear_case(n, m)
    f, s1 = run_fused_and_chain(case, START, LENGTH, what=(n, m, "dev"), dev=True)
    f.solver.close(), s1.solver.close()
    c = clocked(case, START, LENGTH, dev=True)
    s = c.solver
    L, INV = s._L, altro._lib.ERR_INVALID_ARG
    pre, clk = snapshot(s, case.factors), api.get_clock(s)
    host = np.ones(B, dtype=np.int32)
    g = T(host)
    gp = lambda t: C.c_void_p(t.data_ptr())
    paths = altro._lib.hip_runtimes()
    assert len(paths) == 1, paths
    rt = C.CDLL(paths[0])
    rt.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    base, size = C.c_void_p(), C.c_size_t()
    assert rt.hipMemGetAddressRange(C.byref(base), C.byref(size), gp(g)) == 0 and size.value >= B * 4
    short = C.c_void_p(base.value + size.value - (B * 4 - 4))      # the allocation ends one element before the array would
    bad = [(C.c_void_p(host.ctypes.data), None), (gp(g), C.c_void_p(host.ctypes.data)), (short, None), (gp(g), short)]
    if torch.cuda.device_count() > 1:
        other = torch.ones(B, dtype=torch.int32, device=torch.device("cuda", 1))
        bad += [(gp(other), None), (gp(g), gp(other))]
    for a, b in bad:
        assert L.altro_mpc_set_clock_dev(s.h, a, b) == INV
        assert (L.altro_last_error(s.h) or b"").decode()
    assert L.altro_mpc_get_clock(s.h, None, None, None) == INV
    assert_same(snapshot(s, case.factors), pre, what="after the refusals")
    for x, y in zip(api.get_clock(s), clk):
        assert np.array_equal(x, y)
    c.run_async(S, first=0)
    c.synchronize()
    check(case, c, pre, START, LENGTH, what=(n, m, "usable after the refusals"))
    s.close()


@pytest.mark.parametrize("n,m", [(12, 4), (24, 4)])
def test_device_twin_without_lengths(n, m):
    """8. case 1 itself in device form: set_clock(start, None) from a torch tensor (the null-length path of the device twin)
    equals the yardstick, and get_clock reports every length as unbounded (check())"""
    case = linear_case(n, m)
    c = clocked(case, START, None, dev=True)
    pre = snapshot(c.solver, case.factors)
    c.run_async(S, first=0)
    c.synchronize()
    check(case, c, pre, START, None, what=(n, m, "dev, no lengths"))
    c.solver.close()


@pytest.mark.parametrize("n,m", [(12, 4), (6, 6), (24, 4), (48, 4)])
def test_default_path(n, m):
    """9. an explicit all-zero clock with no lengths equals a handle with no clock bit for bit over a fused launch; get_clock
    on the handle without one reports start 0, length -1 and the handle's window; clearing the clock is accepted here."""
    case = linear_case(n, m)
    a, b = case.make(case.noise), case.make(case.noise)
    for mp in (a, b):
        mp.initial_solve()
        mp.enable_log(S)
    b.set_clock(np.zeros(B, dtype=np.int32))
    for mp in (a, b):
        mp.run_async(S, first=0)
        mp.synchronize()
    assert_same(snapshot(a.solver, case.factors), snapshot(b.solver, case.factors), what="zero clock == no clock")
    ra, rb = log_fields(a.log(0, S)), log_fields(b.log(0, S))
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), ("log", k)
    st, ln, win = api.get_clock(a.solver)
    assert np.all(st == 0) and np.all(ln == -1) and np.all(win == S)
    assert np.all(api.get_clock(b.solver)[2] == S)
    b.set_clock(None)      # every window is S: accepted, and the handle goes on from it
    st, ln, win = api.get_clock(b.solver)
    assert np.all(st == 0) and np.all(ln == -1) and np.all(win == S)
    a.solver.close(), b.solver.close()


def test_dynamics_track_must_cover_the_windows_held():
    """under a clock a plain solve reads the dynamics blocks of the window each instance holds: a new dynamics track that ends
    before one of them is refused (ALTRO_ERR_STATE), one that covers them is accepted"""
    case = ltv_case()
    c = clocked(case, START)
    c.run_async(S, first=0)
    c.synchronize()
    win = api.get_clock(c.solver)[2]
    assert win.max() == S
    rng = np.random.default_rng(3)
    s = c.solver

    def track(nb):
        A, Bm = 0.1 * rng.standard_normal((B, nb, 12, 12)), 0.1 * rng.standard_normal((B, nb, 12, 12))
        return s._L.altro_mpc_set_dynamics_track(s.h, api._p(A), api._p(Bm), None, nb, 1, 1)
    assert track(S + N - 2) == altro._lib.ERR_STATE        # window S needs blocks S .. S + N - 2
    assert (s._L.altro_last_error(s.h) or b"").decode()
    assert track(S + N - 1) == 0
    s.close()


def test_needs_a_track():
    """altro_mpc_set_clock on a handle that holds no track: ALTRO_ERR_STATE; clearing a clock that is not set is accepted"""
    L = altro._lib.lib()
    h = C.c_void_p()
    dims = altro._lib.Dims(B, 12, 4, N)
    assert L.altro_batch_create(C.byref(dims), None, 0, C.byref(h)) == 0
    try:
        z = np.zeros(B, dtype=np.int32)
        assert L.altro_mpc_set_clock(h, z.ctypes.data_as(C.POINTER(C.c_int32)), None) == altro._lib.ERR_STATE
        assert (L.altro_last_error(h) or b"").decode()
        assert L.altro_mpc_set_clock(h, None, None) == 0
    finally:
        L.altro_batch_destroy(h)
