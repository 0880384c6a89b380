"""The reference's benchmark scripts, batched: each function runs one of them on the GPU for a
batch of independent problems and returns the result Dict of the reference (`:time`, `:iter`;
random_linear_problem.jl:188) as a Python dict of arrays, one column per instance.

  random_linear_mpc/run_random_linear.jl:110-153   -> run_random_linear, horizon / state / control sweeps
  rocket_landing/run_simple_rocket.jl:31-135        -> run_rocket
  grasp_optimization/grasp_benchmark.jl:60-85       -> run_grasp
  quadruped/Woofer/MPCControl/altro_solver.jl:40-88 -> run_quadruped

The OSQP / ECOS / COSMO twins of the reference are not part of this library (tests/ compare
against an offline oracle instead), so there is no `:err_traj` column.  Times are the kernel's
device time per MPC step for the whole batch (HIP events on the handle's stream)."""
import numpy as np

from . import api, mpc, problems

ROCKET_COLD_OPTS = dict(cost_tolerance_intermediate=1e-4, penalty_scaling=500.0, penalty_initial=1e-2,
                        constraint_tolerance=1e-5, iterations=5000, iterations_inner=100,
                        iterations_linesearch=100, iterations_outer=60)
"""run_simple_rocket.jl:39-50"""
ROCKET_MPC_OPTS = dict(cost_tolerance=1e-4, cost_tolerance_intermediate=1e-4, constraint_tolerance=1e-4,
                       reset_duals=0, penalty_initial=1000.0, penalty_scaling=10.0)
"""run_simple_rocket.jl:121-129"""
GRASP_COLD_OPTS = dict(cost_tolerance=1e-6, cost_tolerance_intermediate=1e-4, constraint_tolerance=1e-6,
                       iterations=5000, iterations_outer=60, iterations_inner=300)
"""grasp_benchmark.jl:19-25"""
GRASP_MPC_OPTS = dict(cost_tolerance=1e-4, cost_tolerance_intermediate=1e-3, constraint_tolerance=1e-4,
                      penalty_initial=10000.0, penalty_scaling=100.0)
"""grasp_benchmark.jl:26-34"""


def _result(times_ms, iters, ok, B):
    times_ms = np.asarray(times_ms)
    return {"time": times_ms, "time_us_per_solve": 1e3 * times_ms / B, "iter": np.asarray(iters),
            "solve_succeeded": np.asarray(ok), "batch": B}


def _result_from_log(launch_ms, log, B, launch_steps):
    """The same Dict from the per-step log of fused launches: `iter` / `solve_succeeded` hold one row per STEP as before,
    `time` one entry per LAUNCH of `launch_steps` steps (a fused launch has no per-step device times)."""
    res = _result(launch_ms, log.iterations.copy(), log.solve_succeeded, B)
    in_launch = np.array([min(launch_steps, log.steps - f) for f in range(0, log.steps, launch_steps)])
    res["time_us_per_solve"] = 1e3 * res["time"] / (B * in_launch)
    res["launch_steps"] = int(launch_steps)
    return res


def _run_fused(mp, steps, launch_steps, B):
    """`steps` MPC steps in launches of `launch_steps` (the last one shorter), statistics of every step from the device log."""
    mp.enable_log(steps)
    t = []
    for first in range(0, steps, launch_steps):
        mp.run_async(min(launch_steps, steps - first), first)
        mp.synchronize()
        t.append(api.stats(mp.solver).tsolve_ms)
    return _result_from_log(t, mp.log(0, steps), B, launch_steps)


def run_random_linear(n=12, m=4, N=50, batch=1024, steps=100, seed=1, launch_steps=1):
    """run_MPC(prob_mpc, opts, Z_track, 100) (random_linear_problem.jl:85-189).  launch_steps = K > 1: the steps run K to a
    launch (altro_mpc_run_async) and `iter` / `solve_succeeded` come from the per-step log; `time` is then per launch."""
    pb = problems.gen_random_linear_batch(batch, n=n, m=m, N=N, steps=steps, seed=seed)
    mp = mpc.BatchMPC(pb)
    mp.initial_solve()
    if launch_steps > 1:
        return _run_fused(mp, steps, launch_steps, batch)
    t, it, ok = [], [], []
    for i in range(steps):
        mp.step(i)
        st = api.stats(mp.solver)
        t.append(st.tsolve_ms); it.append(st.iterations.copy()); ok.append(st.status == api.SOLVE_SUCCEEDED)
    return _result(t, it, ok, batch)


def run_sweeps(batch=256, steps=100):
    """The three sweeps of run_random_linear.jl:110-153 (seeds 1, 10, 15 there)."""
    out = {"horizon": {}, "state_dim": {}, "control_dim": {}}
    for N in (11, 31, 51, 71, 101):
        out["horizon"][N] = run_random_linear(12, 6, N, batch, steps, seed=1)
    for n in (2, 15, 25, 35, 45, 55):
        out["state_dim"][n] = run_random_linear(n, 2, 21, batch, steps, seed=10)
    for m in (2, 6, 10, 15, 20, 25):
        out["control_dim"][m] = run_random_linear(30, m, 21, batch, steps, seed=15)
    return out


def run_rocket(batch=256, N_mpc=21, steps=100, N_cold=301, dt=0.05, seed=1, launch_steps=1):
    """Cold solve of the landing problem, then conic tracking MPC along it (run_simple_rocket.jl:31-135,
    simple_rocket.jl:59-82).  Instances differ in their initial state.  launch_steps: as in run_random_linear."""
    rp = problems.gen_rocket_problem(N=N_cold, tf=(N_cold - 1) * dt, Qfk=1e4, Rk=1.0, theta_thrust_max=5.0, theta_glideslope=45.0)
    rng = np.random.default_rng(seed)
    x0 = np.tile(rp.x0, (batch, 1)) + rng.standard_normal((batch, 6)) * np.array([1, 1, 1, .3, .3, .3]) * 0.5
    cold = api.ALTROSolver(mpc.constrained_problem(rp, x0), api.SolverOptions(**ROCKET_COLD_OPTS))
    api.solve(cold)
    cst = api.stats(cold)
    Xt, Ut = api.states(cold), api.controls(cold)
    cold.close()
    steps = min(steps, N_cold - N_mpc - 1)
    tp = problems.gen_rocket_problem(N=N_mpc, tf=dt * (N_mpc - 1), include_goal=False, theta_thrust_max=5.0, theta_glideslope=45.0)
    tp.Q, tp.R, tp.Qf = np.full(6, 10.0), np.full(3, 0.1), np.full(6, 10.0)            # gen_tracking_problem (mpc.jl:12-14)
    noise = rng.standard_normal((steps, batch, 6))
    prob = mpc.constrained_problem(tp, Xt[:, 0].copy(), Xt[:, :N_mpc].copy(), Ut[:, :N_mpc - 1].copy(), U0=Ut[:, :N_mpc - 1].copy())
    mp = mpc.TrackMPC(prob, api.SolverOptions(**ROCKET_MPC_OPTS), Xt, Ut, noise,
                      (np.array([1e-3] * 3 + [1e-2] * 3), np.array([0, 0, 0, 1, 1, 1])))
    mp.initial_solve()
    if launch_steps > 1:
        res = _run_fused(mp, steps, launch_steps, batch)
    else:
        t, it, ok = [], [], []
        for i in range(steps):
            mp.step(i)
            st = api.stats(mp.solver)
            t.append(st.tsolve_ms); it.append(st.iterations.copy()); ok.append(st.status == api.SOLVE_SUCCEEDED)
        res = _result(t, it, ok, batch)
    res["cold"] = {"time": cst.tsolve_ms, "iter": cst.iterations, "solve_succeeded": cst.status == api.SOLVE_SUCCEEDED}
    return res


def _run_grasp_device(sv, gp, Xt, Ut, batch, N_mpc, steps, rng):
    """The loop of run_grasp with every per-tick array in GPU memory (mpc.ExternalMPC): the cold solve's trajectory and its
    per-knot constraint tables are uploaded once and every window is a slice of them on the device, the plant is torch
    arithmetic, the noise is the host generator's, uploaded once."""
    import torch
    dev = torch.device("cuda", sv.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    Xt_d, Ut_d = up(Xt), up(Ut)
    tabs = [(up(c.A), up(c.b)) for c in gp.constraints[1:]]
    A_d, B_d, f_d = up(gp.A.T), up(gp.Bm.T), up(gp.f)
    noise = up(np.stack([rng.standard_normal((batch, 6)) for _ in range(steps)]))
    loop = mpc.ExternalMPC(sv)
    x = up(np.tile(Xt[0], (batch, 1)))
    u0, _, _, _ = api.first_knot(sv)
    its, sts = [], []
    for i in range(1, steps + 1):
        xn = x @ A_d + u0 @ B_d + f_d
        xn = xn + noise[i - 1] * xn.abs().max(dim=1, keepdim=True).values / 100.0
        Xr = Xt_d[i:i + N_mpc].expand(batch, -1, -1).contiguous()
        Ur = Ut_d[i:i + N_mpc - 1].expand(batch, -1, -1).contiguous()
        data = {ci: (A[i:i + N_mpc - 1], b[i:i + N_mpc - 1]) for ci, (A, b) in enumerate(tabs)}
        u0, _, st, it = loop.tick(xn, Xr, Ur, constraint_data=data)
        x = xn
        its.append(it); sts.append(st)
    torch.cuda.synchronize(dev)
    it = torch.stack(its).cpu().numpy()
    ok = torch.stack(sts).cpu().numpy() == api.SOLVE_SUCCEEDED
    return _result(np.full(steps, np.nan), it, ok, batch)   # (no per-tick device times: nothing waits for a tick here)


def run_grasp(batch=256, N_mpc=21, steps=30, N_cold=251, tf=25.0, seed=1, device_io=False):
    """Cold grasp solve, then run_grasp_mpc (grasp_mpc.jl:8-104): every step rewrites the per-knot
    constraint data of the shifted window (grasp_mpc_helpers.jl:1-55).
    device_io=True: the same loop with every per-tick array in GPU memory (no PCIe copy, no host synchronisation inside the
    loop; `time` is then NaN)."""
    import copy
    gp = problems.gen_grasp_problem(N=N_cold, tf=tf)
    x0c = np.tile(gp.x0, (batch, 1))
    cold = api.ALTROSolver(mpc.constrained_problem(gp, x0c), api.SolverOptions(**GRASP_COLD_OPTS))
    api.solve(cold)
    cst = api.stats(cold)
    Xt, Ut = api.states(cold)[0], api.controls(cold)[0]
    cold.close()
    steps = min(steps, N_cold - N_mpc - 1)

    def window(k0):
        return [problems.ConstraintSpec(c.kind, c.sense, 0, N_mpc - 2, A=c.A[k0:k0 + N_mpc - 1].copy(), b=c.b[k0:k0 + N_mpc - 1].copy())
                for c in gp.constraints[1:]]                                          # the goal is dropped (mpc.jl:33-40)
    tp = copy.copy(gp)
    tp.N, tp.Q, tp.R, tp.Qf = N_mpc, np.full(6, 1e3), np.full(6, 1.0), np.full(6, 10.0)   # grasp_benchmark.jl:79-80
    tp.constraints = window(0)
    Xr, Ur = np.tile(Xt[:N_mpc], (batch, 1, 1)), np.tile(Ut[:N_mpc - 1], (batch, 1, 1))
    sv = api.ALTROSolver(mpc.constrained_problem(tp, np.tile(Xt[0], (batch, 1)), Xr, Ur, U0=Ur.copy()), api.SolverOptions(**GRASP_MPC_OPTS))
    api.solve(sv)
    rng = np.random.default_rng(seed)
    cold_res = {"time": cst.tsolve_ms, "iter": cst.iterations[:1], "solve_succeeded": cst.status[:1] == api.SOLVE_SUCCEEDED}
    if device_io:
        res = _run_grasp_device(sv, gp, Xt, Ut, batch, N_mpc, steps, rng)
        sv.close()
        res["cold"] = cold_res
        return res
    t, it, ok = [], [], []
    for i in range(1, steps + 1):
        X, U = api.states(sv), api.controls(sv)
        xn = X[:, 0] @ gp.A.T + U[:, 0] @ gp.Bm.T + gp.f
        xn = xn + rng.standard_normal((batch, 6)) * np.abs(xn).max(axis=1, keepdims=True) / 100.0
        api.set_initial_state(sv, xn)
        api.update_trajectory(sv, np.tile(Xt[i:i + N_mpc], (batch, 1, 1)), np.tile(Ut[i:i + N_mpc - 1], (batch, 1, 1)))
        api.shift_fill(sv, True, False)
        for ci, c in enumerate(window(i)):
            api.update_constraint_data(sv, ci, c.A, c.b)
        api.shift_fill(sv, False, True)
        api.solve(sv)
        st = api.stats(sv)
        t.append(st.tsolve_ms); it.append(st.iterations.copy()); ok.append(st.status == api.SOLVE_SUCCEEDED)
    res = _result(t, it, ok, batch)
    res["cold"] = cold_res
    return res


def _run_quadruped_device(qp, phases, batch, steps, x0, rng):
    """The loop of run_quadruped with every per-tick array in GPU memory (mpc.ExternalMPC): the linearisation tables of the
    16 gait phases for every tick are uploaded once and indexed on the device, the plant is torch arithmetic on the
    predicted state, the noise is the host generator's, uploaded once.  Same numbers as the host loop, bit for bit."""
    import torch
    dev = torch.device("cuda", 0)
    tabs = [[qp.dynamics(ph + i * qp.dt) for ph in phases] for i in range(steps + 1)]      # [tick][phase] -> (A, B, d)
    # column-major blocks, as the C-ABI reads them: the tensors hold the transposed matrices
    At = torch.from_numpy(np.ascontiguousarray(np.swapaxes(np.array([[t[0] for t in row] for row in tabs]), -1, -2))).to(dev)
    Bt = torch.from_numpy(np.ascontiguousarray(np.swapaxes(np.array([[t[1] for t in row] for row in tabs]), -1, -2))).to(dev)
    dt_ = torch.from_numpy(np.ascontiguousarray(np.array([[t[2] for t in row] for row in tabs]))).to(dev)
    idx = torch.arange(batch, device=dev) % 16
    noise = torch.from_numpy(np.stack([rng.standard_normal((batch, 12)) for _ in range(steps)])).to(dev)
    dyn = lambda i: api.LinearModel(At[i].index_select(0, idx).transpose(-1, -2), Bt[i].index_select(0, idx).transpose(-1, -2),
                                    dt_[i].index_select(0, idx), dt=qp.dt, per_knot=True)
    A0 = dyn(0)
    host = lambda t: t.cpu().numpy()
    sv = api.ALTROSolver(mpc.quadruped_problem(qp, x0, host(A0.A), host(A0.B), host(A0.d)), api.SolverOptions(**problems.QUADRUPED_OPTS))
    api.solve(sv)
    loop = mpc.ExternalMPC(sv)
    _, x1, _, _ = api.first_knot(sv)
    its, sts, evs = [], [], []
    for i in range(1, steps + 1):
        xn = x1 + noise[i - 1] * 1e-3
        _, x1, st, it = loop.tick(xn, dynamics=dyn(i))
        its.append(it); sts.append(st)
    torch.cuda.synchronize(dev)
    it = torch.stack(its).cpu().numpy()
    ok = torch.stack(sts).cpu().numpy() == api.SOLVE_SUCCEEDED
    res = _result(np.full(steps, np.nan), it, ok, batch)   # (no per-tick device times: nothing waits for a tick here)
    res["solver"] = sv
    return res


def run_quadruped(batch=256, N=15, steps=30, linearized_friction=True, seed=7, device_io=False, keep_solver=False):
    """foot_forces! (altro_solver.jl:40-88) in a loop: re-linearise the per-knot dynamics for the
    advancing trot schedule, set x0, shift primal and dual, solve.  The plant here is the linear
    model's own first knot plus 1e-3 noise (the reference steps MuJoCo).
    device_io=True: the same loop with every per-tick array in GPU memory (torch tensors; no PCIe copy, no host
    synchronisation inside the loop; `time` is then NaN).  keep_solver=True: the result carries the solver ("solver")."""
    if device_io:
        qp = problems.gen_quadruped_problem(N=N, linearized_friction=linearized_friction)
        rng = np.random.default_rng(seed)
        phases = rng.uniform(0.0, 0.8, 16)
        x0 = qp.x_des + rng.standard_normal((batch, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
        res = _run_quadruped_device(qp, phases, batch, steps, x0, rng)
        if not keep_solver:
            res.pop("solver").close()
        return res
    qp = problems.gen_quadruped_problem(N=N, linearized_friction=linearized_friction)
    rng = np.random.default_rng(seed)
    phases = rng.uniform(0.0, 0.8, 16)
    idx = np.arange(batch) % 16
    dyn = lambda i: tuple(np.stack(a)[idx] for a in zip(*[qp.dynamics(ph + i * qp.dt) for ph in phases]))
    x0 = qp.x_des + rng.standard_normal((batch, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
    A, Bm, d = dyn(0)
    sv = api.ALTROSolver(mpc.quadruped_problem(qp, x0, A, Bm, d), api.SolverOptions(**problems.QUADRUPED_OPTS))
    api.solve(sv)
    t, it, ok = [], [], []
    for i in range(1, steps + 1):
        X = api.states(sv)
        xn = X[:, 1] + 1e-3 * rng.standard_normal((batch, 12))
        A, Bm, d = dyn(i)
        api.set_dynamics(sv, api.LinearModel(A, Bm, d, dt=qp.dt, per_knot=True))
        api.set_initial_state(sv, xn)
        api.shift_fill(sv, True, True)
        api.solve(sv)
        st = api.stats(sv)
        t.append(st.tsolve_ms); it.append(st.iterations.copy()); ok.append(st.status == api.SOLVE_SUCCEEDED)
    res = _result(t, it, ok, batch)
    if keep_solver:
        res["solver"] = sv
    return res


def summarise(res):
    it = np.asarray(res["iter"])
    out = {"batch": int(res["batch"]), "steps": int(it.shape[0]), "iterations_median": float(np.median(it)),
           "iterations_mean": float(it.mean()), "iterations_max": int(it.max()),
           "solve_succeeded_frac": float(np.mean(res["solve_succeeded"])),
           "ms_per_step_median": float(np.median(res["time"])), "us_per_solve_median": float(np.median(res["time_us_per_solve"]))}
    if "launch_steps" in res:   # fused launches: `time` holds one entry per launch, a step's figure is its share of it
        out["launch_steps"] = int(res["launch_steps"])
        out["ms_per_step_median"] = out["us_per_solve_median"] * out["batch"] / 1e3
    return out
