"""GPU parity tests (run by the driver with -m gpu on a real MI355X): the HIP path, reached
through the C-ABI, against the CPU oracle on the same seeded inputs.

Tolerances: the brief (BASELINE.json north_star) asks for cost / constraint-violation
trajectories within 1e-6 relative; RTOL below is that number.  Integer outputs (iteration
counts, status) must be equal.  At BASELINE's full batch (8192) the oracle cannot run every
instance in seconds, so a strided sample is compared and the whole batch is checked through
size-independent properties (bounds respected, dynamics feasibility, x_1 == x0 exactly, every
status SOLVE_SUCCEEDED, instance i identical whatever the batch around it).
"""
import numpy as np
import pytest

import altro_mpc_icra2021_amd as altro
from altro_mpc_icra2021_amd import problems as P
from helpers import (REF_OPTS, ROCKET_COLD_OPTS, ROCKET_MPC_OPTS, make_oracle, mpc_update, quadruped_gpu_problem,
                     quadruped_oracle, rocket_gpu_problem, rocket_oracle)

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def rel_err(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def check_against_oracle(st, X, U, b, orc, so, utol=RTOL, ttol=RTOL, jtol=RTOL):
    assert int(st.status[b]) == so.status
    assert int(st.iterations[b]) == so.iterations
    assert int(st.iterations_outer[b]) == so.iterations_outer
    assert abs(st.cost[b] - so.cost) <= jtol * max(1.0, abs(so.cost))
    assert abs(st.c_max[b] - so.c_max) <= RTOL * max(1.0, abs(so.c_max))
    k = min(so.iterations, altro._lib.TRACE_LEN)
    Jo = np.array(so.J[:k])
    co = np.array(so.cmax_it[:k])
    assert np.all(np.abs(st.cost_trace[b, :k] - Jo) <= ttol * np.maximum(1.0, np.abs(Jo)))
    assert np.all(np.abs(st.cmax_trace[b, :k] - co) <= ttol * np.maximum(1.0, np.abs(co)))
    assert rel_err(X[b], orc.states()) <= RTOL
    assert rel_err(U[b], orc.controls()) <= utol


@pytest.mark.parametrize("n,m,N", [(16, 4, 50), (12, 6, 31), (20, 4, 21)])
def test_wide_kernel_strict_option_and_default_shortcuts(oracle, n, m, N):
    """The one-wave-per-instance kernel takes the default-mode shortcuts of the 16-lane kernels (confirmation
    iterations when every feedforward term is at rounding level, the line-search early-outs: solve_wide.h ilqr());
    altro_opts.strict = 1 runs every iteration in full.  (16,4), (12,6): the n, m <= 16 instantiation (products chained
    in registers, DPP row rollouts); (20,4): the generic one.
    (a) strict against the oracle, accepted steps included wherever the iteration moved;
    (b) default against strict over a closed loop: same statuses, iteration counts equal in all but a sliver of
        solves, closed-loop states and controls within 1e-6 -- and fewer rollouts (the point of the shortcuts)."""
    B, S = 5, 4
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=31)
    mp = altro.mpc.BatchMPC(pb, altro.SolverOptions(strict=1, **REF_OPTS))
    assert altro.wave_cycles(mp.solver).size == 0        # wide path
    mp.initial_solve()
    orcs = [make_oracle(oracle, pb, b) for b in range(B)]
    for o in orcs:
        o.solve()
    for i in range(S):
        mp.step(i)
        st, X, U, at = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), altro.alpha_trace(mp.solver)
        for b, o in enumerate(orcs):
            mpc_update(o, pb, b, i)
            so = o.solve()
            check_against_oracle(st, X, U, b, o, so)
            k = min(so.iterations, at.shape[1])
            Jt = np.array(so.J[:k])
            moved = np.r_[True, np.abs(np.diff(Jt)) > 1e-9 * np.maximum(1.0, np.abs(Jt[1:]))]
            assert np.array_equal(at[b, :k][moved], np.array(so.alpha[:k])[moved]), (i, b, at[b, :k], list(so.alpha[:k]))
    B, S = 128, 30
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=32)
    runs = []
    for strict in (0, 1):
        mp = altro.mpc.BatchMPC(pb, altro.SolverOptions(strict=strict, **REF_OPTS))
        mp.initial_solve()
        altro.timing_reset(mp.solver)
        x0s, u1s, its, sts = [], [], [], []
        for i in range(S):
            mp.step(i)
            st = altro.stats(mp.solver)
            x0s.append(mp.x0()); u1s.append(altro.controls(mp.solver)[:, 0].copy()); its.append(st.iterations.copy()); sts.append(st.status.copy())
        nb, nr, ntr = altro.work_counters(mp.solver)
        ngc = altro.confirm_counter(mp.solver)
        # confirmation iterations are settled by the costate sweep (no backward pass) in the default mode
        nfo = altro.reuse_counter(mp.solver)
        assert (ngc.sum() + nfo.sum() > 0.3 * B * S and nb.sum() + ngc.sum() + nfo.sum() == np.array(its).sum()) if strict == 0 else ngc.sum() + nfo.sum() == 0
        runs.append((np.array(x0s), np.array(u1s), np.array(its), np.array(sts), float((nr + ntr).sum())))
    (xa, ua, ia, sa, ra), (xb, ub, ib, sb, rb) = runs
    assert np.array_equal(sa, sb) and np.all(sa == altro.SOLVE_SUCCEEDED)
    # observed: no count differs, closed loops equal to 1e-14 (the shortcuts only skip work whose result is known)
    assert np.array_equal(ia, ib), (ia != ib).mean()
    assert rel_err(xa, xb) <= 1e-12 and rel_err(ua, ub) <= 1e-12, (rel_err(xa, xb), rel_err(ua, ub))
    assert ra < 0.8 * rb, (ra, rb)
    print("wide kernel (%d,%d), strict vs default over %d x %d solves: iteration counts differ in %.3f %%, x0 %.1e, u1 %.1e; rollouts %.0f vs %.0f" % (
        n, m, B, S, 100 * (ia != ib).mean(), rel_err(xa, xb), rel_err(ua, ub), rb, ra))


def test_wide_kernel_quadruped_strict_equals_default():
    """Per-knot dynamics and friction pyramids (the DPP row rollouts with parked blocks): five device-resident ticks at
    strict = 1 and in the default mode end in the same statuses and iteration counts and within 1e-6 of each other."""
    B, S, N = 64, 5, 15
    qp = P.gen_quadruped_problem(N=N)
    rng = np.random.default_rng(27)
    t0 = rng.uniform(0.0, 0.8, B)
    x0 = qp.x_des + rng.standard_normal((B, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
    A, Bm, d = _quadruped_track(qp, t0, S + N)
    noise = rng.standard_normal((S, B, 12))
    out = []
    for strict in (0, 1):
        mp = _quadruped_device_loop(qp, x0, A, Bm, d, noise, S, strict=strict)
        mp.initial_solve()
        its = [altro.stats(mp.solver).iterations.copy()]
        for i in range(S):
            mp.step(i)
            its.append(altro.stats(mp.solver).iterations.copy())
        out.append((np.array(its), altro.stats(mp.solver).status.copy(), altro.states(mp.solver), altro.controls(mp.solver), mp.x0()))
    (ia, sa, Xa, Ua, xa), (ib, sb, Xb, Ub, xb) = out
    assert np.array_equal(sa, sb)
    print("quadruped strict vs default: iteration counts differ in %.3f %%, X %.1e, U %.1e, x0 %.1e" % (100 * (ia != ib).mean(), rel_err(Xa, Xb), rel_err(Ua, Ub), rel_err(xa, xb)))
    assert np.array_equal(ia, ib), (ia != ib).mean()
    assert rel_err(Xa, Xb) <= 1e-9 and rel_err(Ua, Ub) <= 1e-9 and rel_err(xa, xb) <= 1e-9


@pytest.mark.parametrize("n,m,N", [(12, 4, 50), (6, 3, 21), (6, 6, 31), (8, 4, 11), (8, 4, 50)])
def test_mpc_loop_matches_oracle(oracle, n, m, N):
    """Warm-started MPC loop (reference run_MPC order) for every built kernel size."""
    B, S = 10, 8   # B not a multiple of 4: exercises the padded instance slots
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=11)
    mp = altro.mpc.BatchMPC(pb)
    mp.initial_solve()
    orcs = [make_oracle(oracle, pb, b) for b in range(B)]
    sos = [o.solve() for o in orcs]
    st = altro.stats(mp.solver)
    X, U = altro.states(mp.solver), altro.controls(mp.solver)
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], sos[b])
    for i in range(S):
        mp.step(i)
        st = altro.stats(mp.solver)
        X, U = altro.states(mp.solver), altro.controls(mp.solver)
        x0g = mp.x0()
        for b in range(B):
            x0 = mpc_update(orcs[b], pb, b, i)
            assert np.abs(x0 - x0g[b]).max() <= 1e-12 * max(1.0, np.abs(x0).max())
            so = orcs[b].solve()
            check_against_oracle(st, X, U, b, orcs[b], so)
            assert np.array_equal(X[b, 0], x0g[b])  # :err_x0 of the reference is identically 0


@pytest.mark.parametrize("n,m,N", [(12, 6, 31), (2, 2, 21), (15, 2, 21), (35, 2, 21), (55, 2, 21), (30, 10, 21), (30, 25, 21),
                                   (16, 4, 50), (32, 4, 50), (48, 4, 50), (64, 4, 50),
                                   (17, 16, 12), (33, 5, 15), (48, 16, 12)])   # edges of the compact LDS carve-up (n = 17..48, m <= 16)
def test_mpc_loop_wide_kernel_sizes_match_oracle(oracle, n, m, N):
    """Sizes outside the 16-lane kernel set run on the one-wave-per-instance MFMA kernel
    (solve_wide.h): the horizon sweep's (12, 6), points of the state- and control-dimension
    sweeps (run_random_linear.jl:110-153: n in {2..55} with m = 2, m in {2..25} with n = 30), and
    BASELINE configs[3]'s own shape (n in {16, 32, 48, 64}, m = 4, N = 50: every LDS size class of
    the kernel up to its largest, n = 64)."""
    B, S = (5, 4) if N < 50 else (4, 3)
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=21)
    mp = altro.mpc.BatchMPC(pb)
    assert altro.wave_cycles(mp.solver).size == 0        # the 16-lane kernel's diagnostic is absent: wide path
    mp.initial_solve()
    orcs = [make_oracle(oracle, pb, b) for b in range(B)]
    sos = [o.solve() for o in orcs]
    st = altro.stats(mp.solver)
    X, U = altro.states(mp.solver), altro.controls(mp.solver)
    Kg, dg = altro.gains(mp.solver)
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], sos[b])
        Ko, do = orcs[b].gains()
        assert rel_err(Kg[b], Ko) <= RTOL and rel_err(dg[b], do) <= RTOL
    for i in range(S):
        mp.step(i)
        st = altro.stats(mp.solver)
        X, U = altro.states(mp.solver), altro.controls(mp.solver)
        x0g = mp.x0()
        for b in range(B):
            x0 = mpc_update(orcs[b], pb, b, i)
            assert np.abs(x0 - x0g[b]).max() <= 1e-12 * max(1.0, np.abs(x0).max())
            check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())


@pytest.mark.parametrize("N,lin", [(15, True), (40, True), (15, False)])
def test_quadruped_contact_switching_mpc_matches_oracle(oracle, N, lin):
    """Quadruped MPC (BASELINE configs[4]; Woofer/MPCControl/altro_solver.jl:40-88): n = m = 12,
    per-knot affine dynamics re-linearised before every solve with the trot's contact mask
    (update_dynamics_matrices!), friction pyramids + f_z box, then set_initial_state!, primal and
    dual shift_fill!, solve!.  Every instance starts at its own gait phase and state error.
    N = 15 is the reference's horizon (MPC.yaml:21), N = 40 BASELINE's; lin = False swaps the
    pyramids for the second-order friction cones of FrictionConstraint.jl."""
    B, S = 6, 5
    qp = P.gen_quadruped_problem(N=N, linearized_friction=lin)
    rng = np.random.default_rng(7)
    t0 = rng.uniform(0.0, 0.8, B)
    x0 = qp.x_des + rng.standard_normal((B, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])

    def dyn(i):
        D = [qp.dynamics(t0[b] + i * qp.dt) for b in range(B)]
        return np.stack([a for a, _, _ in D]), np.stack([bm for _, bm, _ in D]), np.stack([dd for _, _, dd in D])

    A, Bm, d = dyn(0)
    sv = altro.ALTROSolver(quadruped_gpu_problem(altro, qp, x0, A, Bm, d), altro.SolverOptions(**P.QUADRUPED_OPTS))
    assert altro.wave_cycles(sv).size == 0            # n + m = 24: the wide kernel
    altro.solve(sv)
    orcs = [quadruped_oracle(oracle, qp, x0[b], A[b], Bm[b], d[b], P.QUADRUPED_OPTS) for b in range(B)]
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    nact = 0
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())
    for i in range(1, S + 1):
        xn = np.zeros((B, 12))
        for b in range(B):
            xn[b] = orcs[b].plant_step() + 1e-3 * rng.standard_normal(12)
        A, Bm, d = dyn(i)
        altro.set_dynamics(sv, altro.LinearModel(A, Bm, d, dt=qp.dt, per_knot=True))
        altro.set_initial_state(sv, xn)
        altro.shift_fill(sv, True, True)
        altro.solve(sv)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        for b in range(B):
            o = orcs[b]
            o.set_dynamics(A[b], Bm[b], d[b])
            o.set_initial_state(xn[b])
            o.shift_fill(True, True)
            so = o.solve()
            check_against_oracle(st, X, U, b, o, so)
            for c in range(5):
                lam = altro.get_duals(sv, c)[b]
                assert np.abs(lam.reshape(-1) - o.duals(o.con_ids[c])).max() <= RTOL * max(1.0, np.abs(o.duals(o.con_ids[c])).max())
            fz = U[b][:, 2::3]
            nact += int((fz < 1e-3).sum())
    assert nact > 20      # swing legs sit on the f_z >= 0 bound: the contact switches are exercised


def _quadruped_track(qp, t0, nblocks):
    """(A, B, d) of absolute knots 0 .. nblocks-1 for every instance: the trot's contact mask at t0[b] + t dt,
    linearised about x_des (update_dynamics_matrices!, altro_solver.jl:5-37)"""
    long = P.gen_quadruped_problem(N=nblocks + 1)
    D = [long.dynamics(t) for t in t0]
    return np.stack([a for a, _, _ in D]), np.stack([bm for _, bm, _ in D]), np.stack([dd for _, _, dd in D])


def _quadruped_device_loop(qp, x0, A, Bm, d, noise, steps, **more_opts):
    """TrackMPC over the quadruped problem with the dynamics of every tick resident on the device"""
    B, N = x0.shape[0], qp.N
    Nt = steps + N + 1
    prob = quadruped_gpu_problem(altro, qp, x0, A[:, :N - 1], Bm[:, :N - 1], d[:, :N - 1])
    mp = altro.mpc.TrackMPC(prob, altro.SolverOptions(**dict(P.QUADRUPED_OPTS, **more_opts)), np.tile(qp.x_des, (B, Nt, 1)), np.zeros((B, Nt - 1, 12)),
                            noise, (np.full(12, 1e-3),))
    altro.set_dynamics_track(mp.solver, A, Bm, d, step_stride=1)
    altro.initial_controls(mp.solver, np.tile(qp.u_hover, (B, N - 1, 1)))      # set_track installed the track's zeros
    return mp


@pytest.mark.parametrize("N", [15, 40])
def test_quadruped_ltv_mpc_runs_device_resident(oracle, N):
    """The reference re-linearises the model before every tick (altro_solver.jl:5-37, then :44-88).  With the blocks
    of every tick uploaded once (altro_mpc_set_dynamics_track) the whole loop -- plant step with the current
    knot-0 model, new x0, window <- tick + 1, shift_fill, solve -- runs on the device: K ticks in one launch are
    bit-identical to K single-tick launches, and every tick matches the oracle driven through the reference's
    sequence with its model rewritten per tick."""
    B, S = 6, 5
    qp = P.gen_quadruped_problem(N=N)
    rng = np.random.default_rng(7)
    t0 = rng.uniform(0.0, 0.8, B)
    x0 = qp.x_des + rng.standard_normal((B, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
    A, Bm, d = _quadruped_track(qp, t0, S + N)
    noise = rng.standard_normal((S, B, 12))
    one, fused = (_quadruped_device_loop(qp, x0, A, Bm, d, noise, S) for _ in range(2))
    assert altro.wave_cycles(one.solver).size == 0
    orcs = [quadruped_oracle(oracle, qp, x0[b], A[b, :N - 1], Bm[b, :N - 1], d[b, :N - 1], P.QUADRUPED_OPTS) for b in range(B)]
    one.initial_solve()
    fused.initial_solve()
    st, X, U = altro.stats(one.solver), altro.states(one.solver), altro.controls(one.solver)
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())
    for i in range(S):
        one.step(i)
        st, X, U, x0g = altro.stats(one.solver), altro.states(one.solver), altro.controls(one.solver), one.x0()
        for b, o in enumerate(orcs):
            xn = o.plant_step() + 1e-3 * noise[i, b]                           # the model of the tick that just ended
            assert np.abs(xn - x0g[b]).max() <= 1e-12 * max(1.0, np.abs(xn).max())
            o.set_dynamics(A[b, i + 1:i + N], Bm[b, i + 1:i + N], d[b, i + 1:i + N])
            o.set_initial_state(xn)
            o.shift_fill(True, True)
            check_against_oracle(st, X, U, b, o, o.solve())
    fused.run_async(S, first=0)
    fused.synchronize()
    sf = altro.stats(fused.solver)
    assert np.array_equal(altro.states(fused.solver), X) and np.array_equal(altro.controls(fused.solver), U)
    assert np.array_equal(sf.iterations, st.iterations) and np.array_equal(sf.cost, st.cost) and np.array_equal(sf.status, st.status)
    assert np.array_equal(fused.x0(), x0g)


@pytest.mark.parametrize("lin", [True, False])
def test_quadruped_full_batch_properties_and_sampled_parity(oracle, lin):
    """BASELINE configs[4] at its per-GPU size: quadruped contact-switching MPC, N = 40, batch 2048 (16384 over 8
    GPUs), three ticks device-resident, with either friction form ALTROParams.jl:67-72 can build (lin: linearised
    pyramids, C8; otherwise second-order cones, C4).  The oracle follows a strided sample; the whole batch is checked through
    size-independent properties: every status SOLVE_SUCCEEDED, 0 <= f_z <= 133 and the friction pyramids to the
    constraint tolerance, the per-knot affine dynamics satisfied, x_1 == x0 exactly, instance results independent of
    the batch around them."""
    B, S, N = 2048, 3, 40
    qp = P.gen_quadruped_problem(N=N, linearized_friction=lin)
    rng = np.random.default_rng(17)
    t0 = rng.uniform(0.0, 0.8, B)
    x0 = qp.x_des + rng.standard_normal((B, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
    # the gait has four phases: linearise once per distinct contact pattern and index it by (instance, knot)
    A, Bm, d = np.zeros((B, S + N, 12, 12)), np.zeros((B, S + N, 12, 12)), np.zeros((B, S + N, 12))
    cache = {}
    for b in range(B):
        for t in range(S + N):
            c = tuple(P.trot_contacts(t0[b] + t * qp.dt))
            if c not in cache:
                cache[c] = P.quadruped_linearize(qp.x_des, np.zeros(12), qp.feet, np.array(c), qp.inertia, qp.mass, qp.dt)
            A[b, t], Bm[b, t], d[b, t] = cache[c]
    noise = rng.standard_normal((S, B, 12))
    mp = _quadruped_device_loop(qp, x0, A, Bm, d, noise, S)
    mp.initial_solve()
    sample = list(range(0, B, 511)) + [B - 1]
    orcs = {b: quadruped_oracle(oracle, qp, x0[b], A[b, :N - 1], Bm[b, :N - 1], d[b, :N - 1], P.QUADRUPED_OPTS) for b in sample}
    for o in orcs.values():
        o.solve()
    tol = P.QUADRUPED_OPTS["constraint_tolerance"]
    for i in range(S):
        mp.step(i)
        st, X, U, x0g = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), mp.x0()
        ok = st.status == altro.SOLVE_SUCCEEDED
        # (second-order friction cones: up to 1 % of the 2048 solves per tick end at the cost or outer-iteration limit, in the
        #  oracle as on the GPU, same iteration counts: tools/debug/gpu_quad_soc_fail.py; the sample below is compared status
        #  for status)
        assert np.all(ok) if lin else ok.mean() >= 0.985, np.bincount(st.status)
        assert np.array_equal(X[:, 0], x0g)
        X, U, okX = X, U, ok
        fx, fy, fz = U[:, :, 0::3], U[:, :, 1::3], U[:, :, 2::3]
        fx, fy, fz = fx[ok], fy[ok], fz[ok]
        assert fz.min() >= -tol and fz.max() <= qp.fz_max + tol
        if lin:
            assert (np.abs(fx) - qp.mu * fz).max() <= tol and (np.abs(fy) - qp.mu * fz).max() <= tol
        else:
            assert (np.hypot(fx, fy) - qp.mu * fz).max() <= 2 * tol
        Aw, Bw, dw = A[:, i + 1:i + N], Bm[:, i + 1:i + N], d[:, i + 1:i + N]
        Xn = np.einsum("bkij,bkj->bki", Aw, X[:, :-1]) + np.einsum("bkij,bkj->bki", Bw, U) + dw
        assert np.abs(Xn - X[:, 1:]).max() <= 1e-11 * max(1.0, np.abs(X).max())
        for b, o in orcs.items():
            xn = o.plant_step() + 1e-3 * noise[i, b]
            o.set_dynamics(A[b, i + 1:i + N], Bm[b, i + 1:i + N], d[b, i + 1:i + N])
            o.set_initial_state(xn)
            o.shift_fill(True, True)
            so = o.solve()
            if lin:
                check_against_oracle(st, X, U, b, o, so)
            else:
                # A swing leg's force sits at the APEX of its friction cone (f = 0 to rounding), where the three branches
                # of the projection meet: which one a knot takes -- and with it the first step of the solve -- is decided
                # by the last bit (tools/debug/gpu_quad_soc_trace.py: identical traces for ticks on end, then one solve
                # whose first iterate differs by 3e-6 and which ends at the same optimum).  Compared here: the status and,
                # for solves that succeed on both sides, the optimum they reach.
                assert int(st.status[b]) == so.status
                if so.status == 1:
                    assert abs(st.cost[b] - so.cost) <= RTOL * max(1.0, abs(so.cost))
                    assert rel_err(X[b], o.states()) <= 1e-5 and rel_err(U[b], o.controls()) <= 1e-4
    sub = np.array([5, 1000, B - 1])
    mp2 = _quadruped_device_loop(qp, x0[sub], A[sub], Bm[sub], d[sub], noise[:, sub], S)
    mp2.initial_solve()
    mp2.run_async(S, first=0)
    mp2.synchronize()
    assert np.array_equal(altro.states(mp2.solver), X[sub]) and np.array_equal(altro.controls(mp2.solver), U[sub])


def test_grasp_cold_solve_at_the_reference_horizon(oracle):
    """The cold grasp solve at the size the benchmark script runs it (grasp_benchmark.jl:72: GraspProblem(o, 251),
    tf = 6 s) through the C-ABI against the oracle: a batch of perturbed initial states; per-knot equality,
    inequality and second-order-cone rows plus the goal at knot 251."""
    gp = P.gen_grasp_problem(N=251, tf=6.0)
    opts = dict(cost_tolerance=1e-6, cost_tolerance_intermediate=1e-4, constraint_tolerance=1e-6,
                iterations=5000, iterations_outer=60, iterations_inner=300)
    B = 6
    rng = np.random.default_rng(11)
    x0 = np.tile(gp.x0, (B, 1))
    x0[1:, 1:3] += 0.1 * rng.standard_normal((B - 1, 2))      # instance 0 is the reference's problem
    sv = altro.ALTROSolver(rocket_gpu_problem(altro, gp, x0), altro.SolverOptions(**opts))
    altro.solve(sv)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    assert np.all(st.status == altro.SOLVE_SUCCEEDED)
    for b in range(B):
        o = rocket_oracle(oracle, gp, x0[b], opts)
        so = o.solve()
        assert so.status == 1
        check_against_oracle(st, X, U, b, o, so, utol=1e-5, ttol=1e-5)


@pytest.mark.parametrize("n,B", [(16, 8192), (32, 8192), (48, 8192), (64, 8192)])
def test_state_dim_sweep_full_batch_properties(oracle, n, B):
    """BASELINE configs[3] at its per-GPU size (65536 instances over 8 GPUs = 8192 each): random_linear_mpc with m = 4,
    N = 50 and n = 16, 32, 48, 64 (n = 64: the cooperative four-wave blocks), four fused MPC steps.  Whole-batch properties after the
    launch: every solve SOLVE_SUCCEEDED, |u| <= 3 to the constraint tolerance, the dynamics satisfied to rounding,
    x_1 == x0 bit for bit, the reported c_max equal to the bound violation evaluated on the host; a strided sample
    follows the oracle; instances are independent of the batch around them (a sub-batch reproduces them bit for bit)."""
    m, N, S = 4, 50, 4
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=71)
    mp = altro.mpc.BatchMPC(pb)
    mp.initial_solve()
    sample = [0, B // 2 + 1, B - 1]
    orcs = {b: make_oracle(oracle, pb, b) for b in sample}
    for o in orcs.values():
        o.solve()
    for i in range(S - 1):
        mp.step(i)
        for b, o in orcs.items():
            mpc_update(o, pb, b, i)
            o.solve()
    mp.step(S - 1)
    st, X, U, x0g = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), mp.x0()
    for b, o in orcs.items():
        mpc_update(o, pb, b, S - 1)
        check_against_oracle(st, X, U, b, o, o.solve())
    assert np.all(st.status == altro.SOLVE_SUCCEEDED)
    assert np.array_equal(X[:, 0], x0g)
    Xn = np.einsum("bij,bkj->bki", pb.A, X[:, :-1]) + np.einsum("bij,bkj->bki", pb.Bm, U)
    assert np.abs(Xn - X[:, 1:]).max() <= 1e-11 * max(1.0, np.abs(X).max())
    viol = np.maximum(np.abs(U) - pb.u_bnd, 0.0).reshape(B, -1).max(1)
    assert viol.max() < REF_OPTS["constraint_tolerance"]
    assert np.abs(viol - st.c_max).max() <= 1e-12
    sub = np.array([1, B // 3, B - 2])
    import copy
    pb2 = copy.copy(pb)
    pb2.A, pb2.Bm, pb2.Xtrack, pb2.Utrack, pb2.noise = pb.A[sub], pb.Bm[sub], pb.Xtrack[sub], pb.Utrack[sub], pb.noise[:, sub]
    mp2 = altro.mpc.BatchMPC(pb2)
    mp2.initial_solve()
    mp2.run_async(S, first=0)
    mp2.synchronize()
    assert np.array_equal(altro.states(mp2.solver), X[sub]) and np.array_equal(altro.controls(mp2.solver), U[sub])


def test_rocket_full_batch_properties(oracle):
    """BASELINE configs[2] at its own size: rocket landing with the three second-order cones, N_mpc = 100, batch 4096,
    fused device loop.  Whole-batch properties after every launch: thrust-magnitude, thrust-angle and glideslope
    cones to the reported violation, affine dynamics satisfied, x_1 == x0, at least 99 % of the solves SOLVE_SUCCEEDED
    (Altro's default kickout_max_penalty = false: a solve that reaches the penalty cap goes on updating duals there),
    reported c_max consistent with the cones evaluated on the host, instances independent of the batch."""
    B, Nm, S = 4096, 100, 4
    Nt, dt = 301, 0.05
    rp = P.gen_rocket_problem(N=Nt, tf=(Nt - 1) * dt, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
    rng = np.random.default_rng(23)
    x0 = np.tile(rp.x0, (B, 1)) + rng.standard_normal((B, 6)) * np.array([1, 1, 1, .3, .3, .3]) * 0.5
    cold = altro.ALTROSolver(rocket_gpu_problem(altro, rp, x0), altro.SolverOptions(**ROCKET_COLD_OPTS))
    altro.solve(cold)
    assert np.all(altro.stats(cold).status == 1)
    Xt, Ut = altro.states(cold), altro.controls(cold)
    cold.close()
    tp = P.gen_rocket_problem(N=Nm, tf=dt * (Nm - 1), include_goal=False, theta_thrust_max=5.0, theta_glideslope=45.0)
    tp.Q, tp.R, tp.Qf = np.full(6, 10.0), np.full(3, 0.1), np.full(6, 10.0)
    noise = rng.standard_normal((S, B, 6))
    wts, grp = np.array([1e-3] * 3 + [1e-2] * 3), np.array([0, 0, 0, 1, 1, 1])

    def loop(idx):
        prob = rocket_gpu_problem(altro, tp, Xt[idx, 0].copy(), Xt[idx, :Nm].copy(), Ut[idx, :Nm - 1].copy(), U0=Ut[idx, :Nm - 1].copy())
        mp = altro.mpc.TrackMPC(prob, altro.SolverOptions(**ROCKET_MPC_OPTS), Xt[idx], Ut[idx], noise[:, idx], (wts, grp))
        mp.initial_solve()
        return mp

    mp = loop(np.arange(B))
    u_bnd, tan_th, tan_gl = 2.0 * 10.0 * 9.81, np.tan(np.deg2rad(5.0)), np.tan(np.deg2rad(45.0))
    for i in range(S):
        mp.step(i)
        st, X, U, x0g = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), mp.x0()
        ok = st.status == altro.SOLVE_SUCCEEDED
        assert ok.mean() >= 0.99, ok.mean()     # (with kickout_max_penalty = 1 it is 0.89-0.99: solves that reach the cap stop there)
        assert np.all(st.c_max[ok] < ROCKET_MPC_OPTS["constraint_tolerance"])
        assert np.array_equal(X[:, 0], x0g)
        Xn = X[:, :-1] @ tp.A.T + U @ tp.Bm.T + tp.f
        assert np.abs(Xn - X[:, 1:]).max() <= 1e-11 * max(1.0, np.abs(X).max())
        # cone violations on the host: projection distance <= the |v| - t excess
        ex = np.maximum(np.linalg.norm(U, axis=2) - u_bnd, 0.0).max(1)
        ex = np.maximum(ex, np.maximum(np.linalg.norm(U[:, :, :2], axis=2) - tan_th * U[:, :, 2], 0.0).max(1))
        ex = np.maximum(ex, np.maximum(np.linalg.norm(X[:, 7:Nm - 1, :2], axis=2) - tan_gl * X[:, 7:Nm - 1, 2], 0.0).max(1))
        assert np.all(ex <= 2.0 * st.c_max + 1e-9), (ex - 2.0 * st.c_max).max()
    sub = np.array([3, 2000, B - 1])
    mp2 = loop(sub)
    mp2.run_async(S, first=0)
    mp2.synchronize()
    assert np.array_equal(altro.states(mp2.solver), X[sub]) and np.array_equal(altro.controls(mp2.solver), U[sub])


def test_strict_option_matches_oracle_and_bounds_the_default_shortcuts(oracle):
    """altro_opts.strict = 1 runs Altro.jl's exact sequence on the 16-lane kernels (no line-search early-out,
    S <- (S + S')/2 after every knot); the default takes both shortcuts (include/altro_batch.h).
    (a) strict against the oracle: everything check_against_oracle compares plus the accepted steps;
    (b) default against strict over a 100-step closed loop: same statuses, iteration counts equal in all but a
        sliver of solves, closed-loop states and applied controls within 1e-6."""
    B, S = 8, 8
    pb = altro.problems.gen_random_linear_batch(B, steps=S, seed=12)
    mp = altro.mpc.BatchMPC(pb, altro.SolverOptions(strict=1, **REF_OPTS))
    mp.initial_solve()
    orcs = [make_oracle(oracle, pb, b) for b in range(B)]
    for o in orcs:
        o.solve()
    for i in range(S):
        mp.step(i)
        st, X, U, at = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), altro.alpha_trace(mp.solver)
        for b, o in enumerate(orcs):
            mpc_update(o, pb, b, i)
            so = o.solve()
            check_against_oracle(st, X, U, b, o, so)
            # accepted steps wherever the iteration made progress (at a converged iterate J(alpha) - J is pure
            # rounding and the two sides may accept different steps for the same trajectory)
            k = min(so.iterations, at.shape[1])
            Jt = np.array(so.J[:k])
            moved = np.r_[True, np.abs(np.diff(Jt)) > 1e-9 * np.maximum(1.0, np.abs(Jt[1:]))]
            assert np.array_equal(at[b, :k][moved], np.array(so.alpha[:k])[moved]), (i, b, at[b, :k], list(so.alpha[:k]))
    B, S = 256, 100
    pb = altro.problems.gen_random_linear_batch(B, steps=S, seed=13)
    runs = []
    for strict in (0, 1):
        mp = altro.mpc.BatchMPC(pb, altro.SolverOptions(strict=strict, **REF_OPTS))
        mp.initial_solve()
        x0s, u1s, its, sts = [], [], [], []
        for i in range(S):
            mp.step(i)
            st = altro.stats(mp.solver)
            x0s.append(mp.x0()); u1s.append(altro.controls(mp.solver)[:, 0].copy()); its.append(st.iterations.copy()); sts.append(st.status.copy())
        runs.append((np.array(x0s), np.array(u1s), np.array(its), np.array(sts), altro.timing_get(mp.solver).sum()))
    (xa, ua, ia, sa, ta), (xb, ub, ib, sb, tb) = runs
    assert np.array_equal(sa, sb) and np.all(sa == altro.SOLVE_SUCCEEDED)
    # observed: no count differs, closed loops equal to 1e-14 (the shortcuts only skip work whose result is known)
    assert np.array_equal(ia, ib), (ia != ib).mean()
    assert rel_err(xa, xb) <= 1e-12 and rel_err(ua, ub) <= 1e-12, (rel_err(xa, xb), rel_err(ua, ub))
    print("strict vs default over %d x %d solves: iteration counts differ in %.3f %%, closed-loop x0 %.1e, u1 %.1e; kernel time %.1f vs %.1f ms" % (
        B, S, 100 * (ia != ib).mean(), rel_err(xa, xb), rel_err(ua, ub), tb, ta))


def test_benchmark_solve_protocol_matches_oracle(oracle):
    """benchmark_solve!(altro, samples=5, evals=5) inside the MPC loop (random_linear_problem.jl:121-173):
    altro_mpc_prepare_async + altro_batch_shift_fill + altro_batch_benchmark_solve against the oracle
    driven through the same sequence (restore the primal trajectory only, 26 repeated solves)."""
    B, S = 6, 6
    pb = altro.problems.gen_random_linear_batch(B, steps=S, seed=4)
    mp = altro.mpc.BatchMPC(pb)
    mp.initial_solve()
    orcs = [make_oracle(oracle, pb, b) for b in range(B)]
    for o in orcs:
        o.solve()
    for i in range(S):
        ms = mp.step_benchmark(i, samples=5, evals=5)
        assert ms.shape == (5,) and np.all(ms > 0)
        st = altro.stats(mp.solver)
        X, U = altro.states(mp.solver), altro.controls(mp.solver)
        for b, o in enumerate(orcs):
            mpc_update(o, pb, b, i)
            so = o.benchmark_solve(samples=5, evals=5)
            check_against_oracle(st, X, U, b, o, so)
            lam_o = o.duals(0).reshape(pb.N - 1, 2, pb.n + pb.m)
            assert rel_err(altro.get_duals(mp.solver)[b], lam_o) <= RTOL
    # the generic form on a cold problem with reset_duals = true: every repetition is the same solve
    prob = altro.mpc.gen_tracking_problem(pb)
    prob.x0 = prob.x0 + 0.5
    cold = altro.ALTROSolver(prob, altro.SolverOptions(cost_tolerance=1e-4, constraint_tolerance=1e-4, penalty_initial=1000.0, penalty_scaling=100.0))
    altro.solve(cold)
    it1, J1, U1 = altro.iterations(cold).copy(), altro.cost(cold).copy(), altro.controls(cold)
    altro.initial_controls(cold, prob.U0)
    altro.benchmark_solve(cold, samples=2, evals=2)
    # (same iterate path; not bit for bit: a repetition may take gains from memory where the first solve ran the pass)
    assert np.array_equal(altro.iterations(cold), it1) and np.abs(altro.cost(cold) - J1).max() <= 1e-9 * np.abs(J1).max()
    assert rel_err(altro.controls(cold), U1) <= 1e-9


def test_reference_sweeps_reproduce_the_stored_iteration_statistics_point_by_point():
    """run_random_linear.jl:108-153 end to end on the GPU, in the reference's own protocol: the horizon
    sweep (n = 12, m = 6, N in 11..101), the state-dimension sweep (n in 2..55, m = 2, N = 21) and the
    control-dimension sweep (m in 2..25, n = 30, N = 21), 100 MPC steps each, every step ending in
    benchmark_solve!(altro, samples=5, evals=5) and iterations(altro) read afterwards
    (random_linear_problem.jl:161,171) -- the numbers stored in horizon_comp.jld2, state_dim_comp.jld2,
    control_dim_comp.jld2 (tests/golden/ref_iteration_stats.json) are the counts of the LAST of the 26
    repeated solves, which start from the multipliers the earlier ones converged (reset_duals=false and
    benchmark_solve! restores only the primal trajectory).  Each stored point is compared with the same
    point here (8 random problems instead of the reference's one).  tests/test_oracle.py holds the same
    comparison for the oracle and the note on the one stored outlier (n = 15)."""
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_iteration_stats.json")))["stats"]
    B, S = 8, 100
    points = ([("horizon_comp.jld2", i, (12, 6, N), 1) for i, N in enumerate((11, 31, 51, 71, 101))] +
              [("state_dim_comp.jld2", i, (n, 2, 21), 10) for i, n in enumerate((2, 15, 25, 35, 45, 55))] +
              [("control_dim_comp.jld2", i, (30, m, 21), 15) for i, m in enumerate((2, 6, 10, 15, 20, 25))])
    for key, idx, (n, m, N), seed in points:
        g = gold[key][idx]
        pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=seed)
        mp = altro.mpc.BatchMPC(pb)
        mp.initial_solve()
        its = np.zeros((S, B), dtype=int)
        for i in range(S):
            mp.step_benchmark(i, samples=5, evals=5)
            st = altro.stats(mp.solver)
            its[i] = st.iterations
            assert np.all(st.status == altro.SOLVE_SUCCEEDED), (n, m, N, i)
        print("sweep point n=%d m=%d N=%d: reference mean %.2f max %d | here mean %.2f median %.0f max %d, per-problem means %.2f..%.2f" % (
            n, m, N, g["altro_mean"], g["altro_max"], its.mean(), np.median(its), its.max(), its.mean(0).min(), its.mean(0).max()))
        assert its.min() == 2 and np.median(its) == 2, (n, m, N)
        if (n, m, N) == (15, 2, 21):   # the stored outlier: all of its 100 solves took 3-4 iterations (tests/test_oracle.py)
            assert g["altro_min"] == 3 and its.mean() < g["altro_mean"]
            continue
        assert abs(its.mean() - g["altro_mean"]) <= 0.2, (n, m, N, its.mean(), g["altro_mean"])
        # 800 solves here against the reference's 100: the maximum is a tail statistic, so bound the tail's weight
        assert (its > g["altro_max"] + 1).mean() <= 0.01 and its.max() <= g["altro_max"] + 6, (n, m, N, its.max(), g["altro_max"])
        # the reference's single problem must sit inside the spread of the 8 problems here
        assert its.mean(0).min() - 0.1 <= g["altro_mean"] <= its.mean(0).max() + 0.15, (n, m, N, its.mean(0), g["altro_mean"])


def test_cold_solve_far_from_reference_matches_oracle(oracle):
    """Cold solves from a perturbed initial state: many active bounds, several AL outer
    iterations, line-search activity."""
    B = 12
    pb = altro.problems.gen_random_linear_batch(B, steps=1, seed=21)
    prob = altro.mpc.gen_tracking_problem(pb)
    rng = np.random.default_rng(0)
    prob.x0 = prob.x0 + rng.standard_normal(prob.x0.shape) * np.linspace(0.5, 8.0, B)[:, None]
    opts = dict(REF_OPTS, reset_duals=1, constraint_tolerance=1e-6, cost_tolerance=1e-6,
                cost_tolerance_intermediate=1e-6, penalty_scaling=10.0)
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**opts))
    altro.solve(sv)
    st = altro.stats(sv)
    X, U = altro.states(sv), altro.controls(sv)
    Kg, dg = altro.gains(sv)
    at = altro.alpha_trace(sv)
    nout = 0
    for b in range(B):
        o = make_oracle(oracle, pb, b, opts=opts)
        o.set_initial_state(prob.x0[b])
        so = o.solve()
        nout = max(nout, so.iterations_outer)
        check_against_oracle(st, X, U, b, o, so)
        # gains of the last backward pass and the accepted line-search steps
        Ko, do = o.gains()
        assert rel_err(Kg[b], Ko) <= RTOL and np.abs(dg[b] - do).max() <= RTOL * max(1.0, np.abs(do).max())
        # (only where the iteration made progress: at a converged iterate J(alpha) - J is pure
        # rounding and the two sides may accept different steps for the same trajectory)
        k = min(so.iterations, altro._lib.TRACE_LEN)
        Jt = np.array(so.J[:k])
        moved = np.r_[True, np.abs(np.diff(Jt)) > 1e-9 * np.maximum(1.0, np.abs(Jt[1:]))]
        assert np.array_equal(at[b, :k][moved], np.array(so.alpha[:k])[moved])
        # duals
        lam = altro.get_duals(sv)[b]           # (nk, 2, nz)
        assert np.abs(lam.reshape(-1) - o.duals(0)).max() <= RTOL * max(1.0, np.abs(o.duals(0)).max())
    assert nout >= 2, "test must exercise the AL outer loop"


def test_unconstrained_problem(oracle):
    B = 4
    pb = altro.problems.gen_random_linear_batch(B, n=8, m=4, N=15, steps=1, seed=4)
    prob = altro.mpc.gen_tracking_problem(pb)
    prob.constraints.items.clear()
    prob.x0 = prob.x0 + 1.0
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**REF_OPTS))
    altro.solve(sv)
    st = altro.stats(sv)
    X, U = altro.states(sv), altro.controls(sv)
    for b in range(B):
        o = make_oracle(oracle, pb, b, bounded=False)
        o.set_initial_state(prob.x0[b])
        so = o.solve()
        check_against_oracle(st, X, U, b, o, so)


def test_full_batch_properties_and_sampled_parity(oracle):
    """BASELINE config 2: n=12, m=4, N=50, batch 8192."""
    B, S = 8192, 3
    pb = altro.problems.gen_random_linear_batch(B, steps=S, seed=1)
    mp = altro.mpc.BatchMPC(pb)
    mp.initial_solve()
    sample = list(range(0, B, 683)) + [B - 1]
    orcs = {b: make_oracle(oracle, pb, b) for b in sample}
    for o in orcs.values():
        o.solve()
    for i in range(S):
        mp.step(i)
        st = altro.stats(mp.solver)
        X, U = altro.states(mp.solver), altro.controls(mp.solver)
        x0 = mp.x0()
        assert np.all(st.status == altro.SOLVE_SUCCEEDED)
        assert np.median(st.iterations) == 2
        assert np.abs(U).max() <= pb.u_bnd + 1e-4          # constraint_tolerance of the run
        assert np.array_equal(X[:, 0], x0)
        Xn = np.einsum("bij,bkj->bki", pb.A, X[:, :-1]) + np.einsum("bij,bkj->bki", pb.Bm, U)
        assert np.abs(Xn - X[:, 1:]).max() <= 1e-11 * max(1.0, np.abs(X).max())
        for b, o in orcs.items():
            mpc_update(o, pb, b, i)
            so = o.solve()
            check_against_oracle(st, X, U, b, o, so)


def test_instance_results_do_not_depend_on_batch(oracle):
    """Instances are independent: instance i gives bit-identical results alone or in a batch."""
    pb = altro.problems.gen_random_linear_batch(9, steps=2, seed=8)
    mp = altro.mpc.BatchMPC(pb)
    mp.initial_solve()
    mp.step(0)
    Xall = altro.states(mp.solver)
    pb1 = altro.problems.gen_random_linear_batch(1, steps=2, seed=8, first_instance=5)
    mp1 = altro.mpc.BatchMPC(pb1)
    mp1.initial_solve()
    mp1.step(0)
    assert np.array_equal(altro.states(mp1.solver)[0], Xall[5])


@pytest.mark.parametrize("n,m,N", [(12, 4, 50), (16, 4, 50), (24, 4, 30)])
def test_fused_multi_step_launch_is_bit_identical_to_single_steps(n, m, N):
    """altro_mpc_run_async(first, n) == n calls of altro_mpc_step_async, bit for bit -- on the 16-lane kernel and on both
    gain-reuse classes of the one-wave-per-instance kernel ((16, 4): single tile, (24, 4): generic), whose stored gains, exact
    active sets and the roles of their planes have to survive the end of a launch exactly as they stood."""
    B, S = 37, 9
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=13)
    a = altro.mpc.BatchMPC(pb)
    b = altro.mpc.BatchMPC(pb)
    a.initial_solve()
    b.initial_solve()
    for i in range(S):
        a.step(i)
    b.run_async(4, first=0)
    b.run_async(S - 4)
    b.synchronize()
    assert np.array_equal(altro.states(a.solver), altro.states(b.solver))
    assert np.array_equal(altro.controls(a.solver), altro.controls(b.solver))
    assert np.array_equal(altro.get_duals(a.solver), altro.get_duals(b.solver))
    assert np.array_equal(a.x0(), b.x0())
    sa, sb = altro.stats(a.solver), altro.stats(b.solver)
    assert np.array_equal(sa.iterations, sb.iterations) and np.array_equal(sa.status, sb.status)
    assert np.array_equal(sa.cost, sb.cost)
    ns, ni, nok = altro.solve_counters(b.solver)
    assert np.all(ns == S + 1) and np.all(nok == S + 1)


@pytest.mark.parametrize("n,m,N,strict", [(12, 4, 50, 0), (12, 4, 50, 1), (8, 4, 21, 0), (6, 3, 21, 0), (6, 6, 31, 0), (12, 3, 31, 1)])
def test_lone_row_backward_pass_is_bit_identical_to_the_four_row_pass(monkeypatch, n, m, N, strict):
    """A backward pass that only one row of a wave needs runs with the instance spread over the wave's four DPP rows
    (solve_dpp16.h backward_split<4>).  ALTRO_NO_LONE=1 (read at create time) keeps the four-row pass: every output of a
    desynchronised multi-step launch must be the same bit for bit, and the lone form must actually have run."""
    B, S = 23, 12
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=29)
    opts = dict(REF_OPTS, strict=strict)

    def run():
        mp = altro.mpc.BatchMPC(pb, opts=altro.SolverOptions(**opts))
        mp.initial_solve()
        mp.run_async(S, first=0)
        mp.synchronize()
        return mp

    a = run()
    lone_passes = int(altro.wave_cycles(a.solver)[:, 7].sum())
    monkeypatch.setenv("ALTRO_NO_LONE", "1")
    b = run()
    assert int(altro.wave_cycles(b.solver)[:, 7].sum()) == 0
    assert lone_passes > 0 or n < 12
    assert np.array_equal(altro.states(a.solver), altro.states(b.solver))
    assert np.array_equal(altro.controls(a.solver), altro.controls(b.solver))
    assert np.array_equal(altro.get_duals(a.solver), altro.get_duals(b.solver))
    assert np.array_equal(a.x0(), b.x0())
    sa, sb = altro.stats(a.solver), altro.stats(b.solver)
    assert np.array_equal(sa.iterations, sb.iterations) and np.array_equal(sa.status, sb.status)
    assert np.array_equal(sa.cost, sb.cost) and np.array_equal(sa.cost_trace, sb.cost_trace)
    Ka, da = altro.gains(a.solver)
    Kb, db = altro.gains(b.solver)
    assert np.array_equal(Ka, Kb) and np.array_equal(da, db)


def test_separate_shift_fill_call_equals_fused_shift(oracle):
    """The reference's explicit call sequence (set_initial_state!, update_trajectory!,
    RD.shift_fill!, Altro.shift_fill!, solve!) through the fine-grained C-ABI calls gives the
    same result as the device-resident MPC step."""
    B, S = 6, 3
    pb = altro.problems.gen_random_linear_batch(B, steps=S, seed=17)
    mp = altro.mpc.BatchMPC(pb)
    mp.initial_solve()
    sv = altro.ALTROSolver(altro.mpc.gen_tracking_problem(pb), altro.SolverOptions(**REF_OPTS))
    altro.solve(sv)
    for i in range(S):
        mp.step(i)
        x0 = mp.x0()                       # plant step + noise, as computed on device
        altro.set_initial_state(sv, x0)
        Xr, Ur = pb.window(i + 1)
        altro.update_trajectory(sv, Xr, Ur)
        altro.shift_fill(sv, True, True)
        altro.solve(sv)
        assert np.array_equal(altro.states(sv), altro.states(mp.solver))
        assert np.array_equal(altro.controls(sv), altro.controls(mp.solver))
        assert np.array_equal(altro.get_duals(sv), altro.get_duals(mp.solver))


def test_shift_fill_and_accessors_roundtrip():
    B = 5
    pb = altro.problems.gen_random_linear_batch(B, n=6, m=3, N=9, steps=1, seed=2)
    sv = altro.ALTROSolver(altro.mpc.gen_tracking_problem(pb), altro.SolverOptions(**REF_OPTS))
    rng = np.random.default_rng(1)
    U = rng.standard_normal((B, 8, 3))
    altro.initial_controls(sv, U)
    assert np.array_equal(altro.controls(sv), U)
    lam = rng.random((B, 8, 2, 9))
    lam[..., :6] = 0.0   # only bounded elements (the controls) carry duals, as in BoundConstraint
    altro.set_duals(sv, lam)
    assert np.array_equal(altro.get_duals(sv), lam)
    altro.shift_fill(sv, True, True)
    Us = altro.controls(sv)
    assert np.array_equal(Us[:, :-1], U[:, 1:]) and np.array_equal(Us[:, -1], U[:, -1])
    ls = altro.get_duals(sv)
    assert np.array_equal(ls[:, :-1], lam[:, 1:]) and np.array_equal(ls[:, -1], lam[:, -1])


def test_rocket_cold_solve_with_cones_matches_oracle(oracle):
    """Rocket landing cold solve (goal equality + max-thrust, thrust-angle and glideslope second-order
    cones; rocket_landing_problem.jl:96-167 with the options of run_simple_rocket.jl:39-50)."""
    B = 6
    rp = P.gen_rocket_problem(N=61, tf=15.0, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
    rng = np.random.default_rng(0)
    x0 = np.tile(rp.x0, (B, 1)) + rng.standard_normal((B, 6)) * np.array([1, 1, 1, .3, .3, .3]) * np.linspace(0, 1, B)[:, None]
    sv = altro.ALTROSolver(rocket_gpu_problem(altro, rp, x0), altro.SolverOptions(**ROCKET_COLD_OPTS))
    altro.solve(sv)
    st = altro.stats(sv)
    X, U = altro.states(sv), altro.controls(sv)
    for b in range(B):
        o = rocket_oracle(oracle, rp, x0[b], ROCKET_COLD_OPTS)
        so = o.solve()
        assert so.status == 1 and so.iterations_outer >= 3
        check_against_oracle(st, X, U, b, o, so)
        for ci in range(len(rp.constraints)):
            lam_o = o.duals(o.con_ids[ci])
            lam_g = altro.get_duals(sv, ci)[b].reshape(-1)
            assert np.abs(lam_g - lam_o).max() <= RTOL * max(1.0, np.abs(lam_o).max())
    ang = np.degrees(np.arctan2(np.linalg.norm(U[..., :2], axis=-1), U[..., 2]))
    assert ang.max() <= 5.0 + 1e-3


def test_rocket_mpc_steps_with_cones_match_oracle(oracle):
    """Warm-started conic MPC through the fine-grained calls in the reference's order
    (simple_rocket.jl:59-82: plant step + noise, set_initial_state!, update_trajectory!,
    RD.shift_fill!, Altro.shift_fill!, then solve!); tracking problem per mpc.jl:11-47 (goal
    dropped, constraint ranges clipped to the horizon)."""
    B, Nm, S = 5, 21, 4
    rp = P.gen_rocket_problem(N=61, tf=15.0, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
    cold = rocket_oracle(oracle, rp, rp.x0, ROCKET_COLD_OPTS)
    assert cold.solve().status == 1
    Xt, Ut = cold.states(), cold.controls()          # Z_track
    tp = P.gen_rocket_problem(N=Nm, tf=rp.dt * (Nm - 1), include_goal=False, theta_thrust_max=5.0, theta_glideslope=45.0)
    tp.Q, tp.R, tp.Qf = np.full(6, 10.0), np.full(3, 0.1), np.full(6, 10.0)      # gen_tracking_problem
    rng = np.random.default_rng(3)
    x0 = np.tile(Xt[0], (B, 1))
    Xr = np.tile(Xt[:Nm], (B, 1, 1))
    Ur = np.tile(Ut[:Nm - 1], (B, 1, 1))
    sv = altro.ALTROSolver(rocket_gpu_problem(altro, tp, x0, Xr, Ur, U0=Ur.copy()), altro.SolverOptions(**ROCKET_MPC_OPTS))
    altro.solve(sv)
    orcs = [rocket_oracle(oracle, tp, x0[b], ROCKET_MPC_OPTS, Xr[b], Ur[b], U0=Ur[b]) for b in range(B)]
    sos = [o.solve() for o in orcs]
    st = altro.stats(sv)
    X, U = altro.states(sv), altro.controls(sv)
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], sos[b])
    for i in range(S):
        x0n = np.zeros((B, 6))
        for b in range(B):
            xn = orcs[b].plant_step()
            noise = np.r_[rng.standard_normal(3) * np.linalg.norm(xn[:3]) / 1000.0,
                          rng.standard_normal(3) * np.linalg.norm(xn[3:]) / 100.0]   # simple_rocket.jl:65-71
            x0n[b] = xn + noise
            orcs[b].set_initial_state(x0n[b])
            orcs[b].set_reference(Xt[i + 1:i + 1 + Nm], Ut[i + 1:i + Nm])
            orcs[b].shift_fill(True, True)
        altro.set_initial_state(sv, x0n)
        altro.update_trajectory(sv, np.tile(Xt[i + 1:i + 1 + Nm], (B, 1, 1)), np.tile(Ut[i + 1:i + Nm], (B, 1, 1)))
        altro.shift_fill(sv, True, True)
        altro.solve(sv)
        st = altro.stats(sv)
        X, U = altro.states(sv), altro.controls(sv)
        for b in range(B):
            so = orcs[b].solve()
            assert so.status == 1
            check_against_oracle(st, X, U, b, orcs[b], so)


def check_stiff(st, X, U, b, orc, so):
    """check_against_oracle for the horizon-100 conic solves.  Status, iteration counts, the
    violation and the states are held to RTOL as everywhere.  The AL cost J = l(Z) + sum of
    mu/2 c^2 terms is ill-conditioned by construction once mu grows: dJ = mu c dc, so with
    mu = 1e8 (the cap, reached after 6 outer iterations from 1e3 x 10) and c = 1e-4 a 1e-10
    difference in a constraint value is 1e-6 in J.  Hence: iterates of the first 16 iterations and
    the controls 2e-5; final J 1e-6 while mu <= 1e5 (outer <= 3), 5e-3 for solves that ran on to
    the penalty cap."""
    check_against_oracle(st, X, U, b, orc, so, utol=2e-5, ttol=2e-5, jtol=RTOL if so.iterations_outer <= 3 else 5e-3)
    # Bookkeeping of the two conditioning classes, so that a regression of the well-conditioned one cannot hide behind the
    # loose control tolerance: "well" = the solve ended with mu <= 1e5 (at most three outer iterations from 1e3 x 10);
    # "meets" = final J, X and U ALL within the suite's 1e-6.
    well = so.iterations_outer <= 3
    meets = (abs(st.cost[b] - so.cost) <= RTOL * max(1.0, abs(so.cost)) and rel_err(X[b], orc.states()) <= RTOL and
             rel_err(U[b], orc.controls()) <= RTOL)
    return well, meets


class StiffTally:
    """fraction of the compared horizon-100 solves that meet 1e-6 on J, X and U, per conditioning class"""

    def __init__(self):
        self.n = {True: 0, False: 0}
        self.ok = {True: 0, False: 0}

    def add(self, res):
        well, meets = res
        self.n[well] += 1
        self.ok[well] += int(meets)

    def frac(self, well):
        return self.ok[well] / max(1, self.n[well])

    def report(self, name):
        print("%s: well-conditioned solves (mu <= 1e5) %d, of which %d meet 1e-6 on J, X, U (%.1f %%); solves that ran to larger penalties %d, of which %d (%.1f %%)" % (
            name, self.n[True], self.ok[True], 100 * self.frac(True), self.n[False], self.ok[False], 100 * self.frac(False)))


def _rocket_track_mpc(oracle, theta_mpc, B, Nm, seed):
    """BASELINE configs[2] set-up (benchmarks/rocket_landing/simple_rocket.jl:20-82, mpc.jl:11-47):
    cold solve N = 301 (GPU, itself checked against the oracle above), tracking problem of horizon
    Nm on the device-resident TrackMPC loop, one oracle per instance fed the same noise."""
    Nt, dt = 301, 0.05
    rp = P.gen_rocket_problem(N=Nt, tf=(Nt - 1) * dt, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
    rng = np.random.default_rng(seed)
    x0 = np.tile(rp.x0, (B, 1)) + rng.standard_normal((B, 6)) * np.array([1, 1, 1, .3, .3, .3]) * 0.5
    cold = altro.ALTROSolver(rocket_gpu_problem(altro, rp, x0), altro.SolverOptions(**ROCKET_COLD_OPTS))
    altro.solve(cold)
    assert np.all(altro.stats(cold).status == 1)
    Xt, Ut = altro.states(cold), altro.controls(cold)
    tp = P.gen_rocket_problem(N=Nm, tf=dt * (Nm - 1), include_goal=False, theta_thrust_max=theta_mpc, theta_glideslope=45.0)
    tp.Q, tp.R, tp.Qf = np.full(6, 10.0), np.full(3, 0.1), np.full(6, 10.0)
    noise = rng.standard_normal((64, B, 6))
    wts, grp = np.array([1e-3] * 3 + [1e-2] * 3), np.array([0, 0, 0, 1, 1, 1])     # simple_rocket.jl:65-71
    prob = rocket_gpu_problem(altro, tp, Xt[:, 0].copy(), Xt[:, :Nm].copy(), Ut[:, :Nm - 1].copy(), U0=Ut[:, :Nm - 1].copy())
    mp = altro.mpc.TrackMPC(prob, altro.SolverOptions(**ROCKET_MPC_OPTS), Xt, Ut, noise, (wts, grp))
    mp.initial_solve()
    orcs = [rocket_oracle(oracle, tp, Xt[b, 0], ROCKET_MPC_OPTS, Xt[b, :Nm], Ut[b, :Nm - 1], U0=Ut[b, :Nm - 1]) for b in range(B)]
    st, X, U = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver)
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())

    def oracle_step(b, i):
        o = orcs[b]
        xn = o.plant_step()
        nz = noise[i, b] * np.r_[np.full(3, np.linalg.norm(xn[:3]) * 1e-3), np.full(3, np.linalg.norm(xn[3:]) * 1e-2)]
        o.set_initial_state(xn + nz)
        o.set_reference(Xt[b, i + 1:i + 1 + Nm], Ut[b, i + 1:i + Nm])
        o.shift_fill(True, True)
        return xn + nz
    return tp, mp, orcs, oracle_step, Xt, Ut


def ran_to_penalty_cap(so):
    """A solve that did not reach the constraint tolerance before mu hit penalty_max (1e8) leaves
    duals lambda = Pi(lambda - mu c) that carry the 1e-8 state agreement amplified by mu; the next
    warm start (reset_duals = false) inherits them, so that instance stops being a parity case."""
    return so.status != 1 or so.iterations_outer >= 5


def test_rocket_mpc_horizon_100_matches_oracle(oracle):
    """Horizon-100 conic MPC (BASELINE configs[2] shape: n=6, m=3, N_mpc=100, three second-order
    cones per knot) through the fused device loop, strict parity at every step.  The tracking
    problem's thrust-angle cone is opened by 0.02 % relative to the cold problem's: on the
    reference's exact configuration the tracked trajectory rides that cone to the last bit with
    zero duals, so whether a knot's cone counts as violated is decided by 1-ulp rounding of
    A z + b (next test); with the tie removed every iterate matches."""
    B, Nm, S = 6, 100, 8
    tp, mp, orcs, oracle_step, _, _ = _rocket_track_mpc(oracle, 5.001, B, Nm, seed=1)
    live, checked, tally = set(range(B)), 0, StiffTally()
    for i in range(S):
        mp.step(i)
        st, X, U, x0g = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), mp.x0()
        for b in sorted(live):
            x0o = oracle_step(b, i)
            assert np.abs(x0g[b] - x0o).max() <= 1e-9 * max(1.0, np.abs(x0o).max())
            so = orcs[b].solve()
            tally.add(check_stiff(st, X, U, b, orcs[b], so))
            checked += 1
            if ran_to_penalty_cap(so):
                live.discard(b)
    tally.report("horizon 100, tie removed")
    assert checked >= 30 and len(live) >= B - 3
    # the well-conditioned class IS a 1e-6 parity case (J, X and U): every one of its solves, not most of them
    assert tally.n[True] >= 20 and tally.frac(True) == 1.0


def test_rocket_mpc_horizon_100_reference_config(oracle):
    """The reference's exact configuration (same cones in the cold and the tracking problem).
    Instances whose line-search path equals the oracle's must match as above.  Where the path
    differs, the test proves the cause is an exact active-set tie: the warm start of that solve has
    a cone with | ||v̄|| - t | below 1e-13 of its scale, so the cone's Hessian block is switched on
    or off by the rounding of A z + b.  The two runs are then two valid executions of the same
    algorithm; what is still required is that the GPU's solve is no worse an MPC step (constraint
    violation within tolerance class, tracking cost not above the oracle's by more than half)."""
    B, Nm, S = 8, 100, 6
    tp, mp, orcs, oracle_step, Xt, Ut = _rocket_track_mpc(oracle, 5.0, B, Nm, seed=1)
    tol = ROCKET_MPC_OPTS["constraint_tolerance"]
    live, strict, ties, tally = set(range(B)), 0, 0, StiffTally()
    for i in range(S):
        mp.step(i)
        st, X, U = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver)
        for b in sorted(live):
            o = orcs[b]
            x0o = oracle_step(b, i)
            Uw = o.controls()
            so = o.solve()
            k = min(so.iterations, altro._lib.TRACE_LEN)
            # same path: equal iteration count and iterate costs.  (The accepted step sizes are not
            # compared: at a converged iterate d ~ 0, J(alpha) - J is pure rounding and either side
            # may accept a different alpha for a bit-identical trajectory.)  A flipped cone changes
            # the gains, hence the very first iterate's cost.
            Jo = np.array(so.J[:k])
            same = int(st.iterations[b]) == so.iterations and bool(
                np.all(np.abs(st.cost_trace[b, :k] - Jo) <= 2e-5 * np.maximum(1.0, np.abs(Jo))))
            if same:
                tally.add(check_stiff(st, X, U, b, o, so))
                strict += 1
                if ran_to_penalty_cap(so):
                    live.discard(b)
                continue
            # diverged: tie evidence on the warm start of this solve
            Xw = np.zeros((Nm, 6))
            Xw[0] = x0o
            for kk in range(Nm - 1):
                Xw[kk + 1] = tp.A @ Xw[kk] + tp.Bm @ Uw[kk] + tp.f
            margin = np.inf
            for c in tp.constraints:
                if c.kind != P.SOC:
                    continue
                for kk in range(c.k_first, c.k_last + 1):
                    v = c.A @ np.r_[Xw[kk], Uw[min(kk, Nm - 2)]] + c.b
                    margin = min(margin, abs(np.linalg.norm(v[:-1]) - v[-1]) / max(1.0, abs(v[-1])))
            assert margin < 1e-13, (i, b, margin)
            ties += 1

            def plain(Xa, Ua):       # the tracking objective without AL terms
                ex, eu = Xa - Xt[b, i + 1:i + 1 + Nm], Ua - Ut[b, i + 1:i + Nm]
                return 0.5 * tp.dt * (np.sum(tp.Q * ex[:-1] ** 2) + np.sum(tp.R * eu ** 2)) + 0.5 * np.sum(tp.Qf * ex[-1] ** 2)
            assert st.c_max[b] <= max(10 * tol, 2 * so.c_max)
            assert plain(X[b], U[b]) <= 1.5 * plain(o.states(), o.controls()) + 1e-3
            live.discard(b)
    tally.report("horizon 100, reference configuration")
    assert strict >= B and ties >= 1     # both kinds of case were exercised
    assert tally.n[True] >= 8 and tally.frac(True) == 1.0   # same-path solves of the well-conditioned class: 1e-6 on J, X, U


def test_flexible_satellite_mpc_matches_oracle(oracle):
    """Flexible spacecraft LQ MPC (flexible_sat_mpc.jl:133-296; n = 12, m = 3, N = 80, |u| <= 0.01):
    cold solve, then the reference's loop on the device: x0 <- A x0 + B u_1 + 0.0002 randn, solve
    again from the unshifted previous solution with the duals reset (:259-277)."""
    B, S = 6, 6
    pb, x0 = P.gen_flexsat_batch(B, steps=S)
    prob = altro.mpc.gen_tracking_problem(pb)
    prob.x0 = x0.copy()
    mp = altro.mpc.TrackMPC(prob, altro.SolverOptions(**P.FLEXSAT_OPTS), pb.Xtrack, pb.Utrack, pb.noise,
                            noise_model=(np.full(12, 2e-4),), shift=False)
    mp.initial_solve()
    orcs = []
    st, X, U = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver)
    for b in range(B):
        o = make_oracle(oracle, pb, b, opts=P.FLEXSAT_OPTS)
        o.set_initial_state(x0[b])
        check_against_oracle(st, X, U, b, o, o.solve())
        orcs.append(o)
    sat = 0
    for i in range(S):
        mp.step(i)
        st, X, U, x0g = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), mp.x0()
        for b in range(B):
            xn = orcs[b].plant_step() + 2e-4 * pb.noise[i, b]
            assert np.abs(x0g[b] - xn).max() <= 1e-12
            orcs[b].set_initial_state(xn)
            so = orcs[b].solve()
            assert so.status == 1
            check_against_oracle(st, X, U, b, orcs[b], so)
            sat += int((np.abs(U[b]) > pb.u_bnd - 1e-4).sum())
    assert sat > 100            # the torque bound is active throughout


def test_grasp_cold_solve_matches_oracle_and_reference_fixture(oracle):
    """Grasp optimisation (grasp_problem.jl:1-107): per-knot-varying torque-balance equality,
    normal-force inequality and two friction second-order cones, plus the goal at the last knot
    (which shares constraint-row lanes with the stage constraints).  Checked against the oracle
    AND directly against the trajectory the reference stored (grasp_ref_traj.jld2)."""
    from test_oracle_cones import load_grasp_fixture
    y, z, F1, F2, theta, p1 = load_grasp_fixture()
    gp = P.gen_grasp_problem(N=31, tf=3.0)
    opts = dict(cost_tolerance=1e-8, cost_tolerance_intermediate=1e-7, constraint_tolerance=1e-7, penalty_initial=1.0,
                penalty_scaling=10.0, iterations=5000, iterations_outer=60, iterations_inner=300,
                gradient_tolerance=1e-5, gradient_tolerance_intermediate=1e-5)
    B = 5
    rng = np.random.default_rng(5)
    x0 = np.tile(gp.x0, (B, 1))
    x0[1:, 1:3] += 0.2 * rng.standard_normal((B - 1, 2))      # instance 0 is the reference's problem
    sv = altro.ALTROSolver(rocket_gpu_problem(altro, gp, x0), altro.SolverOptions(**opts))
    altro.solve(sv)
    st = altro.stats(sv)
    X, U = altro.states(sv), altro.controls(sv)
    for b in range(B):
        o = rocket_oracle(oracle, gp, x0[b], opts)
        so = o.solve()
        assert so.status == 1
        check_against_oracle(st, X, U, b, o, so)
        for ci in range(len(gp.constraints)):
            lam_o = o.duals(o.con_ids[ci])
            lam_g = altro.get_duals(sv, ci)[b].reshape(-1)
            assert np.abs(lam_g - lam_o).max() <= RTOL * max(1.0, np.abs(lam_o).max())
    # the reference's stored solver output
    assert np.abs(X[0, :, 1] - y).max() < 1e-6 and np.abs(X[0, :, 2] - z).max() < 1e-6
    assert np.abs(U[0, :, 1:3] - F1).max() < 1e-6 and np.abs(U[0, :, 4:6] - F2).max() < 1e-6
    # ... and the reference's OWN solve, iterate path included: with the options that solve effectively ran with
    # (old/altro_cold_solve.jl:79-86: the AL stage at the polish tolerance 1e-5, the polish itself skipped; see
    # tests/test_oracle_cones.py) the kernels reproduce the stored trajectory to rounding after the same 17 iterations
    ref_opts = dict(cost_tolerance_intermediate=1e-5, constraint_tolerance=1e-5, penalty_initial=1.0, penalty_scaling=10.0)
    sv2 = altro.ALTROSolver(rocket_gpu_problem(altro, gp, x0[:1]), altro.SolverOptions(**ref_opts))
    altro.solve(sv2)
    s2, X2, U2 = altro.stats(sv2), altro.states(sv2), altro.controls(sv2)
    assert int(s2.status[0]) == 1 and int(s2.iterations[0]) == 17 and int(s2.iterations_outer[0]) == 5
    assert np.abs(X2[0, :, 1] - y).max() < 1e-10 and np.abs(X2[0, :, 2] - z).max() < 1e-10
    assert np.abs(U2[0, :, 1:3] - F1).max() < 1e-10 and np.abs(U2[0, :, 4:6] - F2).max() < 1e-10


def test_grasp_mpc_loop_with_per_step_constraint_updates_matches_oracle(oracle):
    """run_grasp_mpc (grasp_mpc.jl:8-104) with mpc_update! (grasp_mpc_helpers.jl:1-55): every MPC
    step takes x0 from the plant with 1 % noise, retargets the tracking cost, shifts the primal
    trajectory, REWRITES the per-knot data of all four stage constraints (torque balance, normal
    force, both friction cones) for the shifted window, shifts the duals and solves.  Options of
    grasp_benchmark.jl:26-34 (reset_duals stays true), tracking weights :79-80."""
    B, Nc, Nm, S = 4, 61, 21, 6
    gp = P.gen_grasp_problem(N=Nc, tf=6.0)
    cold_opts = dict(cost_tolerance=1e-6, cost_tolerance_intermediate=1e-4, constraint_tolerance=1e-6,
                     iterations=5000, iterations_outer=60, iterations_inner=300)           # grasp_benchmark.jl:19-25
    cold = rocket_oracle(oracle, gp, gp.x0, cold_opts)
    assert cold.solve().status == 1
    Xt, Ut = cold.states(), cold.controls()                                                  # Z_track
    mpc_opts = dict(cost_tolerance=1e-4, cost_tolerance_intermediate=1e-3, constraint_tolerance=1e-4,
                    penalty_initial=10000.0, penalty_scaling=100.0)

    def window(k0):
        """stage constraints of knots k0 .. k0+Nm-1 of the long problem; the goal is dropped (mpc.jl:33-40)"""
        out = []
        for c in gp.constraints[1:]:
            out.append(P.ConstraintSpec(c.kind, c.sense, 0, Nm - 2, A=c.A[k0:k0 + Nm - 1].copy(), b=c.b[k0:k0 + Nm - 1].copy()))
        return out

    import copy
    tp = copy.copy(gp)
    tp.N, tp.Q, tp.R, tp.Qf = Nm, np.full(6, 1e3), np.full(6, 1.0), np.full(6, 10.0)
    tp.constraints = window(0)
    x0 = np.tile(Xt[0], (B, 1))
    Xr, Ur = np.tile(Xt[:Nm], (B, 1, 1)), np.tile(Ut[:Nm - 1], (B, 1, 1))
    sv = altro.ALTROSolver(rocket_gpu_problem(altro, tp, x0, Xr, Ur, U0=Ur.copy()), altro.SolverOptions(**mpc_opts))
    altro.solve(sv)
    orcs = [rocket_oracle(oracle, tp, x0[b], mpc_opts, Xr[b], Ur[b], U0=Ur[b]) for b in range(B)]
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())
    rng = np.random.default_rng(9)
    for i in range(1, S + 1):
        cons = window(i)
        x0n = np.zeros((B, 6))
        for b in range(B):
            xn = orcs[b].plant_step()
            x0n[b] = xn + rng.standard_normal(6) * np.abs(xn).max() / 100.0
            orcs[b].set_initial_state(x0n[b])
            orcs[b].set_reference(Xt[i:i + Nm], Ut[i:i + Nm - 1])
            orcs[b].shift_fill(True, False)
            for ci, c in enumerate(cons):
                orcs[b].update_constraint_data(orcs[b].con_ids[ci], c.A, c.b)
            orcs[b].shift_fill(False, True)
        altro.set_initial_state(sv, x0n)
        altro.update_trajectory(sv, np.tile(Xt[i:i + Nm], (B, 1, 1)), np.tile(Ut[i:i + Nm - 1], (B, 1, 1)))
        altro.shift_fill(sv, True, False)
        for ci, c in enumerate(cons):
            altro.update_constraint_data(sv, ci, c.A, c.b)
        altro.shift_fill(sv, False, True)
        altro.solve(sv)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        for b in range(B):
            so = orcs[b].solve()
            assert so.status == 1
            check_against_oracle(st, X, U, b, orcs[b], so)


@pytest.mark.parametrize("force_wide", [False, True])
def test_per_instance_constraint_data_grasp_batch_at_different_mpc_phases(oracle, monkeypatch, force_wide):
    """Every problem of the reference owns its constraint tables and mpc_update! rewrites them in place
    (grasp_mpc_helpers.jl:46-55), so a batch may hold problems at DIFFERENT phases of the grasp trajectory.
    Constraints added with per-instance data (per_knot bits 0 and 1): instance b tracks the window that starts
    at knot 3 b + i at MPC step i, with its own torque-balance, normal-force and friction-cone tables; each
    instance against its own oracle, on the 16-lane kernel and on the one-wave-per-instance kernel."""
    if force_wide:
        monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    B, Nc, Nm, S = 5, 61, 21, 3
    gp = P.gen_grasp_problem(N=Nc, tf=6.0)
    cold = rocket_oracle(oracle, gp, gp.x0, dict(cost_tolerance=1e-6, cost_tolerance_intermediate=1e-4, constraint_tolerance=1e-6,
                                                 iterations=5000, iterations_outer=60, iterations_inner=300))
    assert cold.solve().status == 1
    Xt, Ut = cold.states(), cold.controls()
    mpc_opts = dict(cost_tolerance=1e-4, cost_tolerance_intermediate=1e-3, constraint_tolerance=1e-4,
                    penalty_initial=10000.0, penalty_scaling=100.0)
    off = 3 * np.arange(B)                                      # phase of each instance along the cold trajectory

    def window(k0):
        return [P.ConstraintSpec(c.kind, c.sense, 0, Nm - 2, A=c.A[k0:k0 + Nm - 1].copy(), b=c.b[k0:k0 + Nm - 1].copy())
                for c in gp.constraints[1:]]

    def batch_tables(i):                                        # per constraint: A (B, Nm-1, p, nz), b (B, Nm-1, p)
        ws = [window(off[b] + i) for b in range(B)]
        return [(np.stack([w[ci].A for w in ws]), np.stack([w[ci].b for w in ws])) for ci in range(4)]

    import copy
    tp = copy.copy(gp)
    tp.N, tp.Q, tp.R, tp.Qf = Nm, np.full(6, 1e3), np.full(6, 1.0), np.full(6, 10.0)
    x0 = np.stack([Xt[off[b]] for b in range(B)])
    Xr = np.stack([Xt[off[b]:off[b] + Nm] for b in range(B)])
    Ur = np.stack([Ut[off[b]:off[b] + Nm - 1] for b in range(B)])
    cons = altro.ConstraintList(6, 6, Nm)
    specs = window(0)
    for ci, (A, b) in enumerate(batch_tables(0)):
        c = specs[ci]
        con = altro.NormConstraint(A, b, per_instance=True) if c.kind == P.SOC else altro.LinearConstraint(A, b, equality=(c.sense == P.EQ), per_instance=True)
        cons.add_constraint(con, (1, Nm - 1))
    prob = altro.Problem(altro.LinearModel(tp.A, tp.Bm, tp.f, dt=tp.dt), altro.TrackingObjective(tp.Q, tp.R, tp.Qf, Xr, Ur), cons,
                         x0=x0, N=Nm, U0=Ur.copy())
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**mpc_opts))
    assert (altro.wave_cycles(sv).size == 0) == force_wide
    altro.solve(sv)
    orcs = []
    for b in range(B):
        tb = copy.copy(tp)
        tb.constraints = window(off[b])
        orcs.append(rocket_oracle(oracle, tb, x0[b], mpc_opts, Xr[b], Ur[b], U0=Ur[b]))
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    for b in range(B):
        check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())
    assert len({tuple(np.round(U[b, 0], 6)) for b in range(B)}) == B      # the instances really solve different problems
    rng = np.random.default_rng(31)
    for i in range(1, S + 1):
        x0n = np.zeros((B, 6))
        for b in range(B):
            xn = orcs[b].plant_step()
            x0n[b] = xn + rng.standard_normal(6) * np.abs(xn).max() / 100.0
            orcs[b].set_initial_state(x0n[b])
            orcs[b].set_reference(Xt[off[b] + i:off[b] + i + Nm], Ut[off[b] + i:off[b] + i + Nm - 1])
            orcs[b].shift_fill(True, False)
            for ci, c in enumerate(window(off[b] + i)):
                orcs[b].update_constraint_data(orcs[b].con_ids[ci], c.A, c.b)
            orcs[b].shift_fill(False, True)
        altro.set_initial_state(sv, x0n)
        altro.update_trajectory(sv, np.stack([Xt[off[b] + i:off[b] + i + Nm] for b in range(B)]),
                                np.stack([Ut[off[b] + i:off[b] + i + Nm - 1] for b in range(B)]))
        altro.shift_fill(sv, True, False)
        for ci, (A, bb) in enumerate(batch_tables(i)):
            altro.update_constraint_data(sv, ci, A, bb)
        altro.shift_fill(sv, False, True)
        altro.solve(sv)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        for b in range(B):
            so = orcs[b].solve()
            assert so.status == 1
            check_against_oracle(st, X, U, b, orcs[b], so)


def test_update_constraint_data_is_seen_by_the_next_solve(oracle):
    """grasp_mpc_helpers.jl:46-55 mutates the per-knot constraint matrices in place between
    solves; altro_batch_update_constraint_data is that mutation."""
    gp = P.gen_grasp_problem(N=21, tf=2.0)
    gp2 = P.gen_grasp_problem(N=21, tf=2.0, mu=0.3, f_max=2.5)
    opts = dict(cost_tolerance_intermediate=1e-5, constraint_tolerance=1e-5, penalty_initial=1.0, penalty_scaling=10.0)
    x0 = np.tile(gp.x0, (3, 1))
    sv = altro.ALTROSolver(rocket_gpu_problem(altro, gp, x0), altro.SolverOptions(**opts))
    altro.solve(sv)
    for ci, c in enumerate(gp2.constraints):
        altro.update_constraint_data(sv, ci, c.A, c.b)
    altro.initial_controls(sv, np.tile(gp.U0, (3, 1, 1)))
    altro.set_options(sv, reset_duals=1)
    altro.solve(sv)
    o = rocket_oracle(oracle, gp2, gp.x0, opts)
    so = o.solve()
    st = altro.stats(sv)
    check_against_oracle(st, altro.states(sv), altro.controls(sv), 1, o, so)


def test_wide_kernel_passes_the_16_lane_kernels_conic_and_lq_tests(oracle, monkeypatch):
    """ALTRO_FORCE_WIDE=1 makes altro_batch_create pick the one-wave-per-instance kernel for every
    size: the rocket (goal + three cones, cold and warm), grasp (per-knot cones and equalities, the
    reference's stored trajectory), update_constraint_data and flexible-satellite tests above must
    pass unchanged on it, i.e. the two kernels agree with the oracle and with each other."""
    monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    test_rocket_cold_solve_with_cones_matches_oracle(oracle)
    test_rocket_mpc_steps_with_cones_match_oracle(oracle)
    test_grasp_cold_solve_matches_oracle_and_reference_fixture(oracle)
    test_update_constraint_data_is_seen_by_the_next_solve(oracle)
    test_flexible_satellite_mpc_matches_oracle(oracle)
    test_cold_solve_far_from_reference_matches_oracle(oracle)


def test_per_knot_dynamics_on_a_16_lane_size_move_to_the_wide_kernel(oracle):
    """RD.LinearModel with `times` (per-knot A_k, B_k, d_k; ALTROParams.jl:61) at (n, m) = (12, 4): the
    16-lane kernels hold time-invariant dynamics only, so altro_batch_set_dynamics moves the fresh
    handle to the one-wave-per-instance kernel."""
    B, n, m, N = 5, 12, 4, 25
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=33)
    rng = np.random.default_rng(33)
    scale = 1.0 + 0.1 * rng.standard_normal((N - 1, 1, 1))
    A = pb.A[:, None] * scale[None]                                   # (B, N-1, n, n): per instance and per knot
    Bm = pb.Bm[:, None] * (1.0 + 0.1 * rng.standard_normal((N - 1, 1, 1)))[None]
    d = 0.05 * rng.standard_normal((B, N - 1, n))
    prob = altro.mpc.gen_tracking_problem(pb)
    prob.model = altro.LinearModel(A, Bm, d, dt=pb.dt, per_knot=True)
    prob.x0 = prob.x0 + rng.standard_normal(prob.x0.shape)
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**REF_OPTS))
    assert altro.wave_cycles(sv).size == 0
    altro.solve(sv)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    for b in range(B):
        o = make_oracle(oracle, pb, b)
        o.set_dynamics(A[b], Bm[b], d[b])
        o.set_initial_state(prob.x0[b])
        check_against_oracle(st, X, U, b, o, o.solve())


@pytest.mark.parametrize("n,m,N", [(24, 4, 30), (16, 4, 30), (12, 4, 30), (8, 4, 21)])
def test_gain_reuse_is_dropped_by_every_setter_the_gains_depend_on(oracle, n, m, N):
    """Box-only, time-invariant problems (the wide kernel's generic instantiation for n > 16, its single-tile one at (16, 4), the 16-lane kernels otherwise): in the default mode
    iterations whose active set and penalty match the stored backward pass take their gains from memory, also across
    solves and launches.  Everything the gains depend on must drop them -- a new model (set_dynamics), new options
    (another penalty), new cost weights -- and everything the ACTIVE SET depends on must be seen by the hash that guards
    them: new duals, a new initial trajectory, a new reference, a new initial state.  After each change the solve still
    follows the oracle driven through the same calls; with stale gains the iterate path (cost trace, iteration counts)
    differs: the test fails under ALTRO_DEBUG_KEEP_GAINS=1, the diagnostic switch that keeps them."""
    B = 4
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=81)
    prob = altro.mpc.gen_tracking_problem(pb)
    rng = np.random.default_rng(82)
    prob.x0 = prob.x0 + 0.3 * rng.standard_normal(prob.x0.shape)
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**REF_OPTS))
    orcs = [make_oracle(oracle, pb, b) for b in range(B)]
    for b, o in enumerate(orcs):
        o.set_initial_state(prob.x0[b])

    def both(tag):
        altro.timing_reset(sv)
        altro.solve(sv)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        for b, o in enumerate(orcs):
            check_against_oracle(st, X, U, b, o, o.solve())
        return int(altro.reuse_counter(sv).sum())

    both("cold")
    x1 = prob.x0 + 0.02 * rng.standard_normal(prob.x0.shape)
    altro.set_initial_state(sv, x1)
    for b, o in enumerate(orcs):
        o.set_initial_state(x1[b])
    reused = both("warm")                       # same model: iterations without a backward pass
    assert reused > 0
    A2 = pb.A * 0.97
    altro.set_dynamics(sv, altro.LinearModel(A2, pb.Bm, None, dt=pb.dt))
    for b, o in enumerate(orcs):
        o.set_dynamics(A2[b], pb.Bm[b])
    both("new model")
    opts2 = dict(REF_OPTS, penalty_initial=50.0)
    altro.set_options(sv, **opts2)
    for o in orcs:
        o.set_opts(oracle.default_opts(**opts2))
    both("new penalty")
    Q2, R2, Qf2 = np.full(n, 3.0 * pb.Qk), np.full(m, 0.5 * pb.Rk), np.full(n, 2.0 * pb.Qfk)
    altro.set_tracking_cost(sv, Q2, R2, Qf2)
    for o in orcs:
        o.set_cost(Q2, R2, Qf2)
    both("new weights")
    lam = altro.get_duals(sv)
    lam[:, ::3, 0, n:] += 0.5                   # duals > 0 make rows active that were not: another active set, same gains?
    altro.set_duals(sv, lam)
    for b, o in enumerate(orcs):
        o.set_duals(0, lam[b])
    both("new duals")
    U2 = np.clip(altro.controls(sv) + 0.8 * rng.standard_normal((B, N - 1, m)), -4.0, 4.0)   # beyond the bounds in places
    altro.initial_controls(sv, U2)
    for b, o in enumerate(orcs):
        o.set_controls(U2[b])
    both("new initial trajectory")
    Xr, Ur = pb.window(0)
    Xr2, Ur2 = Xr + 0.1 * rng.standard_normal(Xr.shape), 1.6 * Ur      # a reference that saturates the controls
    altro.update_trajectory(sv, Xr2, Ur2)
    for b, o in enumerate(orcs):
        o.set_reference(Xr2[b], Ur2[b])
    both("new reference")
    both("same again")


def test_scheduling_switches_do_not_change_results(monkeypatch):
    """Grouping the instances of a fused launch by their expected backward passes (ALTRO_NO_GROUP), keeping the rows of a
    wave in step (ALTRO_NO_RESYNC), the lone-row pass (ALTRO_NO_LONE), idle rows shadowing a busy one (ALTRO_NO_SHADOW) and the backward
    pass reading its cost / box expansion back from the plane the rollout left (ALTRO_NO_QZ_PASS), issue priority for the wave of a
    SIMD that has more work left (ALTRO_NO_MATE_RANK) decide
    WHEN, in WHICH wave, on whose operands and from which copy of the same numbers a row works, never what it computes: every output is the same bit for bit.  Gain reuse (ALTRO_NO_REUSE) changes the arithmetic of an
    iteration (first-order recursion with the stored gains instead of a backward pass): same statuses and iteration
    counts, trajectories equal to 1e-12."""
    B, S = 150, 14
    pb = altro.problems.gen_random_linear_batch(B, steps=S, seed=31)

    def run():
        mp = altro.mpc.BatchMPC(pb)
        mp.initial_solve()
        altro.timing_reset(mp.solver)
        mp.run_async(S, first=0)
        mp.synchronize()
        return mp

    a = run()
    assert int(altro.reuse_counter(a.solver).sum()) > 0
    Xa, Ua, La, sa = altro.states(a.solver), altro.controls(a.solver), altro.get_duals(a.solver), altro.stats(a.solver)
    for var in ("ALTRO_NO_GROUP", "ALTRO_NO_RESYNC", "ALTRO_NO_LONE", "ALTRO_NO_SHADOW", "ALTRO_NO_QZ_PASS", "ALTRO_NO_MATE_RANK"):
        monkeypatch.setenv(var, "1")
        b = run()
        monkeypatch.delenv(var)
        sb = altro.stats(b.solver)
        assert np.array_equal(Xa, altro.states(b.solver)) and np.array_equal(Ua, altro.controls(b.solver)), var
        assert np.array_equal(La, altro.get_duals(b.solver)) and np.array_equal(a.x0(), b.x0()), var
        assert np.array_equal(sa.iterations, sb.iterations) and np.array_equal(sa.cost, sb.cost), var
    monkeypatch.setenv("ALTRO_NO_REUSE", "1")
    b = run()
    monkeypatch.delenv("ALTRO_NO_REUSE")
    assert int(altro.reuse_counter(b.solver).sum()) == 0
    sb = altro.stats(b.solver)
    assert np.array_equal(sa.iterations, sb.iterations) and np.array_equal(sa.status, sb.status)
    ex, eu = rel_err(Xa, altro.states(b.solver)), rel_err(Ua, altro.controls(b.solver))
    print("gain reuse on / off over %d steps of %d instances: X %.1e, U %.1e" % (S, B, ex, eu))
    assert ex <= 1e-12 and eu <= 1e-12    # (the stored gains are guarded by the exact active set: a reused K IS the K a pass would compute)
    assert np.abs(sa.cost - sb.cost).max() <= 1e-12 * max(1.0, np.abs(sb.cost).max())
    ia, ib = altro.solve_counters(a.solver)[1], altro.solve_counters(b.solver)[1]
    assert np.array_equal(ia, ib)               # iteration counts over all 14 steps, instance by instance


@pytest.mark.parametrize("n", [32, 48])
def test_wide_kernel_compact_lds_layout_does_not_change_results(monkeypatch, n):
    """n = 17..48, m <= 16, time-invariant dynamics: [Qux | Qu] and K live inside the buffer of W = S [A B] (solve_wide.h
    lds_layout, `compact`), which takes the carve-up from three one-wave blocks per CU to four (n <= 32) and from a
    cooperative block to two one-wave blocks (n <= 48).  ALTRO_WIDE_COMPACT=0 is the separate-buffer layout: same bits."""
    B, S = 24, 6
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=4, N=50, steps=S, seed=17)

    def run():
        mp = altro.mpc.BatchMPC(pb)
        mp.initial_solve()
        mp.run_async(S, first=0)
        mp.synchronize()
        return mp

    a = run()
    monkeypatch.setenv("ALTRO_WIDE_COMPACT", "0")
    b = run()
    monkeypatch.delenv("ALTRO_WIDE_COMPACT")
    sa, sb = altro.stats(a.solver), altro.stats(b.solver)
    assert (sa.status == 1).all()
    assert np.array_equal(altro.states(a.solver), altro.states(b.solver)) and np.array_equal(altro.controls(a.solver), altro.controls(b.solver))
    assert np.array_equal(altro.get_duals(a.solver), altro.get_duals(b.solver)) and np.array_equal(a.x0(), b.x0())
    assert np.array_equal(sa.iterations, sb.iterations) and np.array_equal(sa.cost, sb.cost)
    Ka, da = altro.gains(a.solver)
    Kb, db = altro.gains(b.solver)
    assert np.array_equal(Ka, Kb) and np.array_equal(da, db)


@pytest.mark.parametrize("n", [48, 20])
def test_wide_kernel_generic_rows_on_large_states(oracle, n):
    """Linear inequality rows, an equality at the terminal knot, a second-order cone and a control box on a random
    linear model with n = 48 (the cooperative four-wave blocks: the constraint products A_c' D A_c go through the
    helper waves too) and n = 20 (one wave per block, same code): cold solve and two warm solves against the oracle."""
    m, N, B, dt = 4, 15, 3, 0.1
    pbr = altro.problems.gen_random_linear_batch(1, n=n, m=m, N=N, steps=1, seed=61)
    rng = np.random.default_rng(62 + n)
    nz = n + m
    cons = []
    Al = np.zeros((3, nz)); Al[:, :n] = 0.3 * rng.standard_normal((3, n)); Al[:, n:] = rng.standard_normal((3, m))
    cons.append(P.ConstraintSpec(P.LINEAR, P.INEQ, 0, N - 2, A=Al, b=-1.5 * np.ones(3)))          # A z - 1.5 <= 0
    Ae = np.zeros((2, nz)); Ae[:, :n] = rng.standard_normal((2, n))
    cons.append(P.ConstraintSpec(P.LINEAR, P.EQ, N - 1, N - 1, A=Ae, b=np.zeros(2)))              # terminal equality
    As = np.zeros((3, nz)); As[0, n] = 1.0; As[1, n + 1] = 1.0; As[2, n + 2] = 0.0
    cons.append(P.ConstraintSpec(P.SOC, P.INEQ, 0, N - 2, A=As, b=np.array([0.0, 0.0, 2.0])))       # |u_0, u_1| <= 2
    zmin = np.r_[np.full(n, -np.inf), np.full(m, -2.5)]; zmax = np.r_[np.full(n, np.inf), np.full(m, 2.5)]
    cons.append(P.ConstraintSpec(P.BOX, P.INEQ, 0, N - 2, zmin=zmin, zmax=zmax))
    rp = P.RocketProblemData(n=n, m=m, N=N, dt=dt, A=pbr.A[0], Bm=pbr.Bm[0], f=np.zeros(n), Q=np.full(n, 10.0), R=np.full(m, 0.1),
                             Qf=np.full(n, 10.0), xf=np.zeros(n), x0=np.zeros(n), U0=np.zeros((N - 1, m)), constraints=cons)
    x0 = rng.standard_normal((B, n)) * 0.4
    opts = dict(REF_OPTS, penalty_initial=10.0, penalty_scaling=10.0, iterations_outer=40)
    sv = altro.ALTROSolver(altro.mpc.constrained_problem(rp, x0), altro.SolverOptions(**opts))
    assert altro.wave_cycles(sv).size == 0
    orcs = [rocket_oracle(oracle, rp, x0[b], opts) for b in range(B)]
    for rep in range(3):
        if rep:
            x0 = x0 + 0.05 * rng.standard_normal(x0.shape)
            altro.set_initial_state(sv, x0)
        altro.solve(sv)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        for b in range(B):
            if rep:
                orcs[b].set_initial_state(x0[b])
            check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())
        assert np.all(st.status == altro.SOLVE_SUCCEEDED) and (rep > 0 or st.iterations_outer.max() >= 2)   # feasible, and the rows were active


@pytest.mark.parametrize("N", [3, 4, 5, 6])
def test_wide_kernel_shortest_horizons(oracle, monkeypatch, N):
    """Horizons of 3..6 knots (3 is the ABI's minimum) on the one-wave-per-instance kernel, time-invariant and per-knot dynamics: the row
    rollouts request their operands up to three knots ahead and the dynamics / gain blocks two knots ahead, so every
    clamp at the end of the horizon is exercised (sizes (3,2), (12,4) via ALTRO_FORCE_WIDE, and (16,4)).
    The horizon axis of this kernel as a table -- every knot loop with its period and lookahead, N = 3 to 33, one class per
    rollout and sweep, with guards that bounds bind and that the sweeps ran -- is tests/wide_horizons.py, run by
    tests/test_wide_horizons.py and tests/test_wide_horizons_gpu.py."""
    monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    for n, m in ((3, 2), (12, 4), (16, 4)):
        B, S = 4, 3
        pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=40 + N)
        mp = altro.mpc.BatchMPC(pb)
        assert altro.wave_cycles(mp.solver).size == 0
        mp.initial_solve()
        orcs = [make_oracle(oracle, pb, b) for b in range(B)]
        sos = [o.solve() for o in orcs]
        st, X, U = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver)
        for b in range(B):
            check_against_oracle(st, X, U, b, orcs[b], sos[b])
        for i in range(S):
            mp.step(i)
            st, X, U = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver)
            for b in range(B):
                mpc_update(orcs[b], pb, b, i)
                check_against_oracle(st, X, U, b, orcs[b], orcs[b].solve())
        # per-knot dynamics on the same sizes
        rng = np.random.default_rng(50 + N)
        A = pb.A[:, None] * (1.0 + 0.1 * rng.standard_normal((N - 1, 1, 1)))[None]
        Bm = pb.Bm[:, None] * (1.0 + 0.1 * rng.standard_normal((N - 1, 1, 1)))[None]
        d = 0.05 * rng.standard_normal((B, N - 1, n))
        prob = altro.mpc.gen_tracking_problem(pb)
        prob.model = altro.LinearModel(A, Bm, d, dt=pb.dt, per_knot=True)
        prob.x0 = prob.x0 + rng.standard_normal(prob.x0.shape)
        sv = altro.ALTROSolver(prob, altro.SolverOptions(**REF_OPTS))
        altro.solve(sv)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        for b in range(B):
            o = make_oracle(oracle, pb, b)
            o.set_dynamics(A[b], Bm[b], d[b])
            o.set_initial_state(prob.x0[b])
            check_against_oracle(st, X, U, b, o, o.solve())


@pytest.mark.parametrize("n,m", [(12, 4), (12, 3), (8, 4), (6, 6), (6, 3), (12, 6), (20, 9), (16, 4), (10, 10), (9, 14)])
def test_option_fuzz_matches_oracle(oracle, n, m):
    """Random solver options on random problems, cold starts far from the reference: iteration caps that end
    solves in MAX_ITERATIONS / MAX_ITERATIONS_OUTER, short line searches (failed searches and the
    regularisation bumps that follow), dual and penalty caps, reset_duals on and off -- every status,
    count and trace must equal the oracle's, on every 16-lane instantiation and on the wide kernel
    ((12,6), (16,4), (10,10), (9,14): the n, m <= 16 instantiations of the m <= 8 / 4 / 12 / 16 classes, with their
    row rollouts and costate sweeps; (20,9): the generic m <= 12 class)."""
    rng = np.random.default_rng(100 + m)
    rng_k = np.random.default_rng(300 + n)       # its own stream: the draws above keep the sequence that reaches every status
    B, N = 6, 20
    statuses = set()
    for trial in range(10):
        pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1000 + trial)
        prob = altro.mpc.gen_tracking_problem(pb)
        prob.x0 = prob.x0 + rng.standard_normal(prob.x0.shape) * rng.uniform(0.5, 10.0)
        opts = dict(cost_tolerance=10.0 ** rng.uniform(-8, -3), constraint_tolerance=10.0 ** rng.uniform(-8, -3),
                    penalty_initial=10.0 ** rng.uniform(-1, 4), penalty_scaling=float(rng.choice([2.0, 10.0, 100.0])),
                    penalty_max=10.0 ** rng.uniform(4, 8), dual_max=10.0 ** rng.uniform(0, 8),
                    iterations=int(rng.choice([3, 8, 40, 1000])), iterations_inner=int(rng.choice([2, 5, 300])),
                    iterations_outer=int(rng.choice([1, 2, 4, 30])), iterations_linesearch=int(rng.choice([0, 2, 20])),
                    reset_duals=int(rng.integers(0, 2)), kickout_max_penalty=int(rng_k.integers(0, 2)))
        opts["cost_tolerance_intermediate"] = opts["cost_tolerance"] * float(rng.choice([1.0, 10.0]))
        sv = altro.ALTROSolver(prob, altro.SolverOptions(**opts))
        altro.solve(sv)
        altro.solve(sv)                      # a second solve from the first one's result (warm duals when reset_duals = 0)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        for b in range(B):
            o = make_oracle(oracle, pb, b, opts=opts)
            o.set_initial_state(prob.x0[b])
            o.solve()
            so = o.solve()
            statuses.add(so.status)
            if so.status == 3 and so.iterations_outer >= 10:
                # a solve that sat at the penalty cap through ten or more outer iterations without meeting the constraint
                # tolerance (kickout_max_penalty = 0): every one of those inner solves ends on a dJ-vs-tolerance comparison
                # of rounding-level numbers, so the inner iteration COUNT may differ by one or two between two correct
                # implementations; everything else is still held together
                assert int(st.status[b]) == so.status and int(st.iterations_outer[b]) == so.iterations_outer
                assert abs(int(st.iterations[b]) - so.iterations) <= 2
                assert rel_err(X[b], o.states()) <= 1e-4 and rel_err(U[b], o.controls()) <= 1e-4
                continue
            check_against_oracle(st, X, U, b, o, so)
    # the fuzz reached several termination statuses (three or four of them on five of the seven shapes; the m = 6 draw
    # sequence ends every capped solve on the outer-iteration cap)
    assert len(statuses) >= (2 if m in (6, 10, 14) else 3), statuses


def test_conic_option_fuzz_matches_oracle(oracle):
    """Random solver options on short rocket landings (goal equality + three second-order cones): both
    cone treatments (soc_second_order on / off), iteration caps, short line searches, penalty schedules.
    Penalties stay below 1e6 so that no iterate sits exactly on a cone boundary (see the horizon-100 test
    for what happens there)."""
    rng = np.random.default_rng(77)
    B = 4
    statuses = set()
    for trial in range(6):
        N = int(rng.choice([11, 21, 31]))
        rp = P.gen_rocket_problem(N=N, tf=0.25 * (N - 1), Qfk=1e3, Rk=1.0, theta_thrust_max=float(rng.choice([5.0, 10.0])),
                                  theta_glideslope=45.0)
        x0 = np.tile(rp.x0, (B, 1)) + rng.standard_normal((B, 6)) * np.array([1, 1, 1, .3, .3, .3]) * 0.5
        opts = dict(ROCKET_COLD_OPTS)
        opts.update(cost_tolerance=10.0 ** rng.uniform(-6, -3), constraint_tolerance=10.0 ** rng.uniform(-6, -3),
                    penalty_initial=10.0 ** rng.uniform(-1, 2), penalty_scaling=float(rng.choice([5.0, 10.0, 50.0])),
                    penalty_max=10.0 ** rng.uniform(4, 6), iterations=int(rng.choice([15, 60, 400])),
                    iterations_inner=int(rng.choice([4, 30, 300])), iterations_outer=int(rng.choice([2, 5, 30])),
                    iterations_linesearch=int(rng.choice([3, 20])), soc_second_order=int(rng.integers(0, 2)))
        opts["cost_tolerance_intermediate"] = opts["cost_tolerance"] * 10.0
        sv = altro.ALTROSolver(rocket_gpu_problem(altro, rp, x0), altro.SolverOptions(**opts))
        altro.solve(sv)
        st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
        for b in range(B):
            o = rocket_oracle(oracle, rp, x0[b], opts)
            so = o.solve()
            statuses.add(so.status)
            check_against_oracle(st, X, U, b, o, so)
            for ci in range(len(rp.constraints)):
                lam_o = o.duals(o.con_ids[ci])
                lam_g = altro.get_duals(sv, ci)[b].reshape(-1)
                assert np.abs(lam_g - lam_o).max() <= RTOL * max(1.0, np.abs(lam_o).max())
    assert len(statuses) >= 2, statuses


def test_benchmark_script_functions_run():
    """benchmarks.py restates the reference's four benchmark scripts as functions; small batches here."""
    from altro_mpc_icra2021_amd import benchmarks as Bm
    r = Bm.summarise(Bm.run_random_linear(batch=16, steps=5))
    assert r["iterations_median"] == 2.0 and r["solve_succeeded_frac"] == 1.0
    r = Bm.summarise(Bm.run_rocket(batch=8, N_mpc=21, steps=4, N_cold=61, dt=0.25))
    assert r["solve_succeeded_frac"] >= 0.9
    r = Bm.summarise(Bm.run_grasp(batch=4, N_mpc=11, steps=3, N_cold=41, tf=4.0))
    assert r["solve_succeeded_frac"] == 1.0 and r["iterations_median"] <= 4.0      # the reference's grasp MPC median is 3
    for lin in (True, False):
        r = Bm.summarise(Bm.run_quadruped(batch=8, N=15, steps=3, linearized_friction=lin))
        assert r["solve_succeeded_frac"] == 1.0


def test_error_paths():
    # n > 64 is outside both kernels
    pb = altro.problems.gen_random_linear_batch(2, n=70, m=2, N=9, steps=1)
    with pytest.raises(altro.AltroError) as e:
        altro.ALTROSolver(altro.mpc.gen_tracking_problem(pb))
    assert e.value.code == altro._lib.ERR_UNSUPPORTED
    # n = 64 with m = 20: the padded knot matrices exceed the 160 KB of LDS of a CU
    pb = altro.problems.gen_random_linear_batch(1, n=64, m=20, N=5, steps=1)
    sv = altro.ALTROSolver(altro.mpc.gen_tracking_problem(pb))
    with pytest.raises(altro.AltroError) as e:
        altro.solve(sv)
    assert e.value.code == altro._lib.ERR_UNSUPPORTED
    # cones of dimension 5 fit neither kernel
    pb = altro.problems.gen_random_linear_batch(2, n=12, m=6, N=9, steps=1)
    prob = altro.mpc.gen_tracking_problem(pb)
    prob.constraints.add_constraint(altro.NormConstraint(np.ones((5, 18)), np.zeros(5)), (1, 8))
    with pytest.raises(altro.AltroError) as e:
        altro.ALTROSolver(prob)
    assert e.value.code == altro._lib.ERR_UNSUPPORTED
    # a second-order cone of dimension 5 does not fit a quad
    pb = altro.problems.gen_random_linear_batch(2, n=6, m=3, N=9, steps=1)
    prob = altro.mpc.gen_tracking_problem(pb)
    prob.constraints.add_constraint(altro.NormConstraint(np.ones((5, 9)), np.zeros(5)), (1, 8))
    with pytest.raises(altro.AltroError) as e:
        altro.ALTROSolver(prob)
    assert e.value.code == altro._lib.ERR_UNSUPPORTED


def test_projected_newton_polish_matches_oracle(oracle):
    """SURVEY 8 f4 (parity with Altro.jl unpinned; see tests/test_oracle_cones.py): altro_opts.projected_newton = 1 --
    the AL kernel stops at projected_newton_tolerance, then csrc/pn_core.h (view: csrc/pn_polish.h) projects the trajectory onto the active
    constraints and the dynamics.  Against the oracle's polish on (a) a box-constrained LQ batch with saturating
    controls and (b) the grasp problem (cones, per-knot equalities and inequalities, goal): same AL stage, same
    decision to polish, the polished trajectories within 1e-6, constraints and dynamics to the polish tolerance."""
    B = 5
    pb = altro.problems.gen_random_linear_batch(B, steps=1, seed=81)
    prob = altro.mpc.gen_tracking_problem(pb)
    rng = np.random.default_rng(3)
    prob.x0 = prob.x0 + np.array([25.0, 25.0, 0.1, 12.0, 25.0])[:, None] + rng.standard_normal(prob.x0.shape)
    opts = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**opts))
    altro.solve(sv)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    ran, failed, res = altro.polish_stats(sv)
    d0, d1, dfail = altro.polish_dual_residuals(sv)
    assert ran.sum() >= 3 and not failed.any()
    for b in range(B):
        o = make_oracle(oracle, pb, b, opts=opts)
        o.set_initial_state(prob.x0[b])
        so = o.solve()
        assert int(st.status[b]) == so.status == 1 and int(st.iterations[b]) == so.iterations and int(ran[b]) == so.pn_ran
        assert abs(st.cost[b] - so.cost) <= RTOL * max(1.0, abs(so.cost)) and st.c_max[b] < 1e-8
        assert rel_err(X[b], o.states()) <= RTOL and rel_err(U[b], o.controls()) <= RTOL
        if ran[b]:
            assert np.abs(X[b, :-1] @ pb.A[b].T + U[b] @ pb.Bm[b].T - X[b, 1:]).max() < 1e-8 and np.abs(U[b]).max() <= pb.u_bnd + 1e-8
        # the dual half (Altro's multiplier projection): stationarity residual with the AL duals and with the projected multipliers
        assert int(dfail[b]) == so.pn_dual_failed == 0
        assert abs(d0[b] - so.pn_dual_residual0) <= 1e-6 * max(1.0, so.pn_dual_residual0) and abs(d1[b] - so.pn_dual_residual) <= 1e-6 * max(1.0, so.pn_dual_residual0)
        if ran[b]:
            assert d1[b] < 1e-5 * d0[b]       # a polished optimum: the KKT conditions hold with the projected multipliers
    # the grasp problem: AL stage to a loose 1e-2, polish to 1e-6
    gp = P.gen_grasp_problem(N=31, tf=3.0)
    gopts = dict(cost_tolerance_intermediate=1e-5, penalty_initial=1.0, penalty_scaling=10.0, constraint_tolerance=1e-6,
                 projected_newton=1, projected_newton_tolerance=1e-2)
    x0 = np.tile(gp.x0, (3, 1))
    x0[1:, 1:3] += 0.1 * rng.standard_normal((2, 2))
    sg = altro.ALTROSolver(rocket_gpu_problem(altro, gp, x0), altro.SolverOptions(**gopts))
    altro.solve(sg)
    st, X, U = altro.stats(sg), altro.states(sg), altro.controls(sg)
    ran, failed, res = altro.polish_stats(sg)
    d0, d1, dfail = altro.polish_dual_residuals(sg)
    assert ran.all() and not failed.any() and res.max() < 1e-6
    for b in range(3):
        o = rocket_oracle(oracle, gp, x0[b], gopts)
        so = o.solve()
        assert so.pn_ran == 1 and int(st.status[b]) == so.status == 1 and int(st.iterations[b]) == so.iterations
        assert st.c_max[b] < 1e-6 and abs(st.cost[b] - so.cost) <= 1e-5 * max(1.0, abs(so.cost))
        assert rel_err(X[b], o.states()) <= 1e-5 and rel_err(U[b], o.controls()) <= 1e-5
        assert int(dfail[b]) == so.pn_dual_failed
        assert abs(d0[b] - so.pn_dual_residual0) <= 1e-4 * max(1.0, so.pn_dual_residual0) and abs(d1[b] - so.pn_dual_residual) <= 1e-4 * max(1.0, so.pn_dual_residual0)


@pytest.mark.parametrize("n,m,N", [(12, 4, 21), (20, 4, 21)])
def test_projected_newton_polish_inside_the_mpc_loop(oracle, n, m, N):
    """solve!(::ALTROSolver) ends with the polish (Altro's default), so an MPC loop with projected_newton = 1 shifts the
    POLISHED trajectory and the PROJECTED multipliers into the next step.  Both backends ((12, 4): 16-lane, (20, 4): one wave
    per instance) run the steps of a fused launch as pairs of (one-step solve kernel, polish kernel); against the oracle's loop
    step by step, and the fused launch against single steps bit for bit."""
    B, S = 5, 6
    pb = altro.problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=S, seed=87)
    pb.u_bnd = 1.0                                   # the track was generated with |u| <= 3: controls saturate in every solve, the AL stage ends above 1e-8
    opts = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    mp = altro.mpc.BatchMPC(pb, altro.SolverOptions(**opts))
    mp.initial_solve()
    orcs = [make_oracle(oracle, pb, b, opts=opts) for b in range(B)]
    for o in orcs:
        o.solve()
    nran = 0
    for i in range(S):
        mp.step(i)
        st, X, U, L = altro.stats(mp.solver), altro.states(mp.solver), altro.controls(mp.solver), altro.get_duals(mp.solver)
        ran, failed, res = altro.polish_stats(mp.solver)
        x0g = mp.x0()
        assert not failed.any()
        for b in range(B):
            x0 = mpc_update(orcs[b], pb, b, i)
            assert np.abs(x0 - x0g[b]).max() <= 1e-9 * max(1.0, np.abs(x0).max())
            so = orcs[b].solve()
            assert int(st.status[b]) == so.status == 1 and int(st.iterations[b]) == so.iterations and int(ran[b]) == so.pn_ran, (i, b)
            assert rel_err(X[b], orcs[b].states()) <= RTOL and rel_err(U[b], orcs[b].controls()) <= RTOL, (i, b)
            assert st.c_max[b] < 1e-8
            lo = orcs[b].duals(0).reshape(N - 1, 2, n + m)
            assert np.abs(L[b][:N - 1] - lo).max() <= 1e-6 * max(1.0, np.abs(lo).max()), (i, b)
            nran += so.pn_ran
    assert nran >= B * S - 2    # the polish ran in (nearly) every solve of the loop
    # K fused steps = K single steps
    mf = altro.mpc.BatchMPC(pb, altro.SolverOptions(**opts))
    mf.initial_solve()
    mf.run_async(S, first=0)
    mf.synchronize()
    assert np.array_equal(altro.states(mf.solver), X) and np.array_equal(altro.controls(mf.solver), U)
    assert np.array_equal(altro.get_duals(mf.solver), L) and np.array_equal(mf.x0(), x0g)


def test_projected_newton_polish_on_the_one_wave_per_instance_backend(oracle, monkeypatch):
    """SURVEY 8 f4 on the second backend (csrc/pn_core.h through the view csrc/pn_wide.h; parity with Altro.jl unpinned as above): projected_newton = 1 on
    sizes outside the 16-lane set -- (a) box-constrained LQ at (20, 4) with saturating controls, (b) the quadruped tick
    (n = m = 12, per-knot dynamics, friction rows + f_z box), (c) the grasp problem forced onto this backend (cones,
    per-knot equalities and inequalities, goal) -- against the oracle's polish: same AL stage, same decision to polish,
    polished trajectories, objective and both residuals of the multiplier projection."""
    B = 4
    pb = altro.problems.gen_random_linear_batch(B, n=20, m=4, N=21, steps=1, seed=85)
    prob = altro.mpc.gen_tracking_problem(pb)
    prob.x0 = prob.x0 + np.array([20.0, 15.0, 0.1, 25.0])[:, None]
    opts = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**opts))
    assert altro.wave_cycles(sv).size == 0        # wide path
    altro.solve(sv)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    ran, failed, res = altro.polish_stats(sv)
    d0, d1, dfail = altro.polish_dual_residuals(sv)
    assert ran.sum() >= 2 and not failed.any()
    for b in range(B):
        o = make_oracle(oracle, pb, b, opts=opts)
        o.set_initial_state(prob.x0[b])
        so = o.solve()
        assert int(st.status[b]) == so.status == 1 and int(st.iterations[b]) == so.iterations and int(ran[b]) == so.pn_ran
        assert abs(st.cost[b] - so.cost) <= RTOL * max(1.0, abs(so.cost)) and st.c_max[b] < 1e-8
        assert rel_err(X[b], o.states()) <= RTOL and rel_err(U[b], o.controls()) <= RTOL
        assert int(dfail[b]) == so.pn_dual_failed == 0
        assert abs(d0[b] - so.pn_dual_residual0) <= 1e-6 * max(1.0, so.pn_dual_residual0) and abs(d1[b] - so.pn_dual_residual) <= 1e-6 * max(1.0, so.pn_dual_residual0)
        if ran[b]:
            assert np.abs(X[b, :-1] @ pb.A[b].T + U[b] @ pb.Bm[b].T - X[b, 1:]).max() < 1e-8 and np.abs(U[b]).max() <= pb.u_bnd + 1e-8
            assert d1[b] < 1e-5 * d0[b]
    # (b) one quadruped tick: per-knot dynamics, linearised friction pyramids, f_z box
    N = 10
    qb = P.gen_quadruped_batch(3, N=N, steps=1, seed=19)
    qopts = dict(P.QUADRUPED_OPTS, constraint_tolerance=1e-7, projected_newton=1, projected_newton_tolerance=1e-2)
    sq = altro.ALTROSolver(quadruped_gpu_problem(altro, qb.qp, qb.x0, qb.A[:, :N - 1], qb.Bm[:, :N - 1], qb.d[:, :N - 1]), altro.SolverOptions(**qopts))
    altro.solve(sq)
    st, X, U = altro.stats(sq), altro.states(sq), altro.controls(sq)
    ran, failed, res = altro.polish_stats(sq)
    d0, d1, dfail = altro.polish_dual_residuals(sq)
    assert not failed.any()
    for b in range(3):
        o = quadruped_oracle(oracle, qb.qp, qb.x0[b], qb.A[b, :N - 1], qb.Bm[b, :N - 1], qb.d[b, :N - 1], qopts)
        so = o.solve()
        assert int(st.status[b]) == so.status and int(st.iterations[b]) == so.iterations and int(ran[b]) == so.pn_ran
        assert abs(st.cost[b] - so.cost) <= 1e-5 * max(1.0, abs(so.cost)) and abs(st.c_max[b] - so.c_max) <= 1e-7
        assert rel_err(X[b], o.states()) <= 1e-5 and rel_err(U[b], o.controls()) <= 1e-5
        assert abs(d0[b] - so.pn_dual_residual0) <= 1e-4 * max(1.0, so.pn_dual_residual0) and abs(d1[b] - so.pn_dual_residual) <= 1e-4 * max(1.0, so.pn_dual_residual0)
    assert ran.sum() >= 1
    # (c) the grasp problem on this backend
    monkeypatch.setenv("ALTRO_FORCE_WIDE", "1")
    rng = np.random.default_rng(3)
    gp = P.gen_grasp_problem(N=31, tf=3.0)
    gopts = dict(cost_tolerance_intermediate=1e-5, penalty_initial=1.0, penalty_scaling=10.0, constraint_tolerance=1e-6,
                 projected_newton=1, projected_newton_tolerance=1e-2)
    x0 = np.tile(gp.x0, (2, 1))
    x0[1:, 1:3] += 0.1 * rng.standard_normal((1, 2))
    sg = altro.ALTROSolver(rocket_gpu_problem(altro, gp, x0), altro.SolverOptions(**gopts))
    assert altro.wave_cycles(sg).size == 0
    altro.solve(sg)
    st, X, U = altro.stats(sg), altro.states(sg), altro.controls(sg)
    ran, failed, res = altro.polish_stats(sg)
    assert ran.all() and not failed.any() and res.max() < 1e-6
    for b in range(2):
        o = rocket_oracle(oracle, gp, x0[b], gopts)
        so = o.solve()
        assert so.pn_ran == 1 and int(st.status[b]) == so.status == 1 and int(st.iterations[b]) == so.iterations
        assert st.c_max[b] < 1e-6 and abs(st.cost[b] - so.cost) <= 1e-5 * max(1.0, abs(so.cost))
        assert rel_err(X[b], o.states()) <= 1e-5 and rel_err(U[b], o.controls()) <= 1e-5


def test_projected_newton_polish_walks_its_workspace_slots():
    """The one-wave-per-instance polish (csrc/pn_core.h through csrc/pn_wide.h) runs min(B, 64) blocks; block s polishes the instances s, s + 64, ...
    in the workspace of slot s.  Batch 66 at (20, 4, 21), recipe of case (a) above, with instances 64 and 65 exact copies
    of 0 and 1 (dynamics, reference, x0; the bounds are common): what the second visit of slots 0 and 1 leaves must equal
    the first visit's byte for byte -- it would not if a slot's workspace were read where the instance's is meant, or the
    other way round.  Instance 2 differs from instance 0, so the comparison cannot pass on a constant."""
    B = 66
    pb = altro.problems.gen_random_linear_batch(B, n=20, m=4, N=21, steps=1, seed=85)
    for a in (pb.A, pb.Bm, pb.Xtrack, pb.Utrack):
        a[64:66] = a[0:2]
    prob = altro.mpc.gen_tracking_problem(pb)
    prob.x0 = prob.x0 + np.resize(np.array([20.0, 15.0, 0.1, 25.0]), B)[:, None]
    prob.x0[64:66] = prob.x0[0:2]
    opts = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    sv = altro.ALTROSolver(prob, altro.SolverOptions(**opts))
    assert altro.wave_cycles(sv).size == 0        # wide path
    altro.solve(sv)
    st, X, U = altro.stats(sv), altro.states(sv), altro.controls(sv)
    ran, failed, res = altro.polish_stats(sv)
    d0, d1, dfail = altro.polish_dual_residuals(sv)
    sv.close()
    assert ran[0] + ran[1] >= 1
    outs = dict(states=X, controls=U, cost=st.cost, c_max=st.c_max, status=st.status, iterations=st.iterations,
                ran=ran, failed=failed, residual=res, dual_before=d0, dual_after=d1, dual_failed=dfail)
    for name, a in outs.items():
        a = np.asarray(a)
        for i in (0, 1):
            assert a[i].tobytes() == a[64 + i].tobytes(), (name, i)
    assert not np.array_equal(X[2], X[0]) and not np.array_equal(U[2], U[0]) and st.cost[2] != st.cost[0]


def test_initial_state_uploaded_before_per_knot_dynamics_survives_the_move_to_the_wide_kernel():
    """altro_batch_set_initial_state before altro_batch_set_dynamics(per_knot = 1) on a 16-lane size: the handle moves to
    the one-wave-per-instance backend and carries x0 over (it used to be dropped silently)."""
    import ctypes as C
    L = altro._lib.lib()
    B, n, m, N = 3, 12, 4, 9
    dims = altro._lib.Dims(B, n, m, N)
    opts = altro.SolverOptions(**REF_OPTS)
    h = C.c_void_p()
    assert L.altro_batch_create(C.byref(dims), C.byref(opts), 0, C.byref(h)) == 0
    try:
        rng = np.random.default_rng(5)
        x0 = np.ascontiguousarray(rng.standard_normal((B, n)))
        dp = C.POINTER(C.c_double)
        assert L.altro_batch_set_initial_state(h, x0.ctypes.data_as(dp)) == 0
        A = np.ascontiguousarray(np.tile(np.eye(n) * 0.9, (N - 1, 1, 1)))
        Bm = np.ascontiguousarray(rng.standard_normal((N - 1, m, n)))       # column-major n x m blocks
        assert L.altro_batch_set_dynamics(h, A.ctypes.data_as(dp), Bm.ctypes.data_as(dp), None, 1, 0) == 0
        out = np.zeros((B, n))
        assert L.altro_batch_get_initial_state(h, out.ctypes.data_as(dp)) == 0
        assert np.array_equal(out, x0)
    finally:
        L.altro_batch_destroy(h)
