"""MPC harness for batches: restates benchmarks/mpc.jl::gen_tracking_problem (:11-47) and the
loop of benchmarks/random_linear_mpc/random_linear_problem.jl::run_MPC (:85-189) on top of the
batched solver.  The OSQP twin of the reference is replaced by the offline oracle in tests/.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, api

REF_OPTS = dict(cost_tolerance=1e-4, cost_tolerance_intermediate=1e-4, constraint_tolerance=1e-4,
                penalty_initial=1000.0, penalty_scaling=100.0, reset_duals=0)
"""SolverOptions of run_random_linear.jl:41-49 (projected_newton=false is the only built mode)."""


def gen_tracking_problem(pb, N=None):
    """gen_tracking_problem(prob, N): tracking cost Q=10 I, R=0.1 I, Qf=10 I about the first N
    knots of the long trajectory, same bound constraint on knots 1..N-1 (mpc.jl:11-47)."""
    N = pb.N if N is None else N
    n, m = pb.n, pb.m
    Xr, Ur = pb.Xtrack[:, :N], pb.Utrack[:, :N - 1]
    model = api.LinearModel(pb.A, pb.Bm, dt=pb.dt)
    def w(v, k):   # scalar weight -> (k,); per-instance (B, k) as given
        return np.full(k, v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
    obj = api.TrackingObjective(w(pb.Qk, n), w(pb.Rk, m), w(pb.Qfk, n), Xr, Ur)
    cons = api.ConstraintList(n, m, N)
    ub = pb.u_bnd if np.ndim(pb.u_bnd) == 0 else np.repeat(np.asarray(pb.u_bnd, dtype=np.float64)[:, None], m, axis=1)
    cons.add_constraint(api.BoundConstraint(n, m, u_min=-ub, u_max=ub), (1, N - 1))
    return api.Problem(model, obj, cons, x0=Xr[:, 0].copy(), N=N, U0=Ur.copy())


@dataclass
class MPCLog:
    """Per-step records of a device-resident MPC run (altro_mpc_get_log), step-major: what the reference's loops keep of
    every step (simple_rocket.jl:137-205: X_traj[i+1] = prob_mpc.x0, iters[i], status[i], costs[i])."""
    first: int                      # absolute index of the first step held
    x0: np.ndarray                  # (S, B, n) initial state each step's solve started from
    u0: np.ndarray                  # (S, B, m) first control of the trajectory the step left: what the next plant step applies
    iterations: np.ndarray          # (S, B) int32
    iterations_outer: np.ndarray    # (S, B) int32
    status: np.ndarray              # (S, B) int32
    cost: np.ndarray                # (S, B)
    c_max: np.ndarray               # (S, B)

    @property
    def steps(self):
        return self.x0.shape[0]

    @property
    def solve_succeeded(self):
        return self.status == _lib.SOLVE_SUCCEEDED

    def x_traj(self, x_start):
        """The closed-loop trajectory the reference calls X_traj, (S + 1, B, n): `x_start` (B, n), the initial state the
        handle held before step `first`, then x0 of every step (simple_rocket.jl:137,164)."""
        return x_traj(x_start, self)


def x_traj(x_start, log):
    x_start = np.asarray(x_start, dtype=np.float64)
    if x_start.shape != log.x0.shape[1:]:
        raise ValueError(f"x_start is {x_start.shape}, the log holds states {log.x0.shape[1:]}")
    return np.concatenate([x_start[None], log.x0], axis=0)


class BatchMPC:
    """Device-resident MPC loop over a RandomLinearBatch (reference run_MPC).

    The long reference trajectory and the per-step noise samples are uploaded once; every
    `step(i)` then runs entirely on the GPU in the reference's order:
    plant step + 1 % noise -> x0; retarget tracking cost to window i+1; primal shift_fill;
    dual shift_fill; solve  (random_linear_problem.jl:125-139,161).
    """

    def __init__(self, pb, opts=None, device=0):
        self.pb = pb
        self.solver = api.ALTROSolver(gen_tracking_problem(pb), opts or api.SolverOptions(**REF_OPTS), device)
        s = self.solver
        Xt, Ut = api._c(pb.Xtrack), api._c(pb.Utrack)
        s._chk(s._L.altro_mpc_set_track(s.h, api._p(Xt), api._p(Ut), pb.Nt))
        nz = api._c(pb.noise)
        s._chk(s._L.altro_mpc_set_noise(s.h, api._p(nz), nz.shape[0]))
        self._U0 = Ut[:, :s.N - 1]   # controls of the track's first window: what a respawned instance starts from
        self.i = 0

    def initial_solve(self):
        """solve!(altro) before the loop (random_linear_problem.jl:113)."""
        api.solve(self.solver)

    def step_async(self, i=None):
        i = self.i if i is None else i
        s = self.solver
        s._chk(s._L.altro_mpc_step_async(s.h, i))
        self.i = i + 1

    def run_async(self, nsteps, first=None):
        """nsteps consecutive MPC steps in one launch (altro_mpc_run_async)."""
        first = self.i if first is None else first
        s = self.solver
        s._chk(s._L.altro_mpc_run_async(s.h, first, nsteps))
        self.i = first + nsteps

    def synchronize(self):
        s = self.solver
        s._chk(s._L.altro_batch_synchronize(s.h))

    def step(self, i=None):
        self.step_async(i)
        self.synchronize()

    def step_benchmark(self, i=None, samples=5, evals=5):
        """One MPC step exactly as the reference's loop body runs it (random_linear_problem.jl:121-161):
        plant step + noise -> x0; update_trajectory!; RD.shift_fill!(Z); Altro.shift_fill!(conSet);
        benchmark_solve!(altro, samples=5, evals=5).  The statistics read afterwards are those of the
        last of the 1 + samples*evals repeated solves, as in the reference's result Dict.  Returns the
        per-sample times (ms, whole batch)."""
        i = self.i if i is None else i
        s = self.solver
        s._chk(s._L.altro_mpc_prepare_async(s.h, i))
        api.shift_fill(s, True, True)
        ms = api.benchmark_solve(s, samples, evals)
        self.i = i + 1
        return ms

    def x0(self):
        s = self.solver
        out = np.empty((s.B, s.n))
        s._chk(s._L.altro_batch_get_initial_state(s.h, api._p(out)))
        return out

    def set_active(self, active):
        """Per-instance active mask of the loop (api.set_active; None clears it): inactive instances take no plant step, are
        not shifted or solved, and their slots of log() stay never written (iterations = status = -1, NaN)."""
        api.set_active(self.solver, active)

    def set_clock(self, start, length=None):
        """Per-instance episode clock of the loop (api.set_clock; start None clears it): instance b takes absolute step i as
        its local step i - start[b], with that step's window, and is idle outside 0 <= local step < length[b]."""
        api.set_clock(self.solver, start, length)

    def respawn(self, which, x0, at_step, U=None):
        """Start the instances `which` (indices) over between two launches: from `at_step` on they run a new episode from
        x0 (len(which), n), as a new solver given that x0 would run its steps 0, 1, ... -- with the noise rows of the
        absolute steps.  The recipe: cold restart from the controls U (len(which), N-1, m; default the track's first window),
        which under the clock rewinds their window to 0; set their x0; a plain solve under a mask of just those instances
        (the solve before the loop); the previous mask back; start[which] = at_step.  Sets an all-zero clock first when none
        is set.  Synchronises."""
        s = self.solver
        which = np.atleast_1d(np.asarray(which, dtype=np.int64))
        sel = np.zeros(s.B, dtype=np.int32)
        sel[which] = 1
        x0 = np.asarray(x0, dtype=np.float64).reshape(len(which), s.n)
        start, length, _ = api.get_clock(s)
        api.set_clock(s, start, None if (length < 0).all() else length)   # (a clock must be in force for the rewind)
        Ufull = np.ascontiguousarray(self._U0)
        if U is not None:
            Ufull = Ufull.copy()
            Ufull[which] = np.asarray(U, dtype=np.float64).reshape(len(which), s.N - 1, s.m)
        api.restart_instances(s, sel, Ufull)
        xall = self.x0()
        xall[which] = x0
        api.set_initial_state(s, xall)
        mask = api.get_active(s)
        api.set_active(s, sel)
        api.solve(s)
        api.set_active(s, None if mask.all() else mask)
        start[which] = int(at_step)
        api.set_clock(s, start, None if (length < 0).all() else length)

    def enable_log(self, steps):
        """Keep one record per MPC step on the device for steps 0 .. steps-1 (altro_mpc_set_log); 0 switches it off.
        Remembers the initial state the handle holds now: the first row of closed_loop_trajectory()."""
        s = self.solver
        s._chk(s._L.altro_mpc_set_log(s.h, int(steps)))
        self.log_steps = int(steps)
        self.log_first, self.log_x_start = self.i, (self.x0() if steps else None)

    def log(self, first=0, nsteps=None):
        """MPCLog of steps first .. first+nsteps-1 (default: up to the step the loop has reached)."""
        s = self.solver
        nsteps = max(self.i - first, 0) if nsteps is None else nsteps
        ip = C.POINTER(C.c_int32)
        x0, u0 = np.empty((nsteps, s.B, s.n)), np.empty((nsteps, s.B, s.m))
        it, ito, st = (np.empty((nsteps, s.B), dtype=np.int32) for _ in range(3))
        cost, cm = np.empty((nsteps, s.B)), np.empty((nsteps, s.B))
        s._chk(s._L.altro_mpc_get_log(s.h, int(first), int(nsteps), api._p(x0), api._p(u0), it.ctypes.data_as(ip),
                                      ito.ctypes.data_as(ip), st.ctypes.data_as(ip), api._p(cost), api._p(cm)))
        return MPCLog(int(first), x0, u0, it, ito, st, cost, cm)

    def closed_loop_trajectory(self):
        """X_traj of the steps run since enable_log: (S + 1, B, n)."""
        return self.log(self.log_first).x_traj(self.log_x_start)


class TrackMPC:
    """Device-resident MPC loop for any tracking problem: the solver is built on the first window
    of (Xtrack, Utrack); `noise` are unit normals (steps, B, n).  noise_model: None for the
    random-linear model (1 % of ||x0||_inf), (weights, groups) for the two-group 2-norm model of
    the rocket benchmark (simple_rocket.jl:65-71), or (weights,) for absolute noise
    (flexible_sat_mpc.jl:266).  shift=False keeps the previous solution and duals as the warm
    start instead of shifting them (flexible_sat_mpc.jl:275-276)."""

    def __init__(self, prob, opts, Xtrack, Utrack, noise, noise_model=None, device=0, shift=True):
        self.solver = api.ALTROSolver(prob, opts, device)
        s = self.solver
        Xt, Ut = api._c(Xtrack), api._c(Utrack)
        s._chk(s._L.altro_mpc_set_track(s.h, api._p(Xt), api._p(Ut), Xt.shape[1]))
        api.set_initial_state(s, prob.x0)        # set_track starts from the track's first knot; the problem's x0 wins
        nz = api._c(noise)
        s._chk(s._L.altro_mpc_set_noise(s.h, api._p(nz), nz.shape[0]))
        if noise_model is not None:
            w = api._c(noise_model[0])
            if len(noise_model) > 1:
                g = np.ascontiguousarray(noise_model[1], dtype=np.int32)
                s._chk(s._L.altro_mpc_set_noise_model(s.h, 1, api._p(w), g.ctypes.data_as(C.POINTER(C.c_int32))))
            else:
                s._chk(s._L.altro_mpc_set_noise_model(s.h, 2, api._p(w), None))
        if not shift:
            s._chk(s._L.altro_mpc_set_shift(s.h, 0))
        self._U0 = Ut[:, :s.N - 1]
        self.i = 0

    initial_solve = BatchMPC.initial_solve
    step_async = BatchMPC.step_async
    run_async = BatchMPC.run_async
    synchronize = BatchMPC.synchronize
    step = BatchMPC.step
    step_benchmark = BatchMPC.step_benchmark
    x0 = BatchMPC.x0
    set_active = BatchMPC.set_active
    set_clock = BatchMPC.set_clock
    respawn = BatchMPC.respawn
    enable_log = BatchMPC.enable_log
    log = BatchMPC.log
    closed_loop_trajectory = BatchMPC.closed_loop_trajectory


class ExternalMPC:
    """MPC loop for a plant the CALLER owns (a simulator, a learned model, a re-linearisation: the reference's foot_forces!,
    altro_solver.jl:40-88, where MuJoCo is the plant), with every array in GPU memory: one `tick` is
    set x0 [, new reference window] [, new dynamics]; primal + dual shift_fill; solve; read the first knot -- enqueued on
    the solver's stream between one wait_stream and one signal_stream against torch's current stream, with no host
    synchronisation and no copy over PCIe.  The tensors returned are ready in torch's stream order.  The solver must hold
    a solution to shift (api.solve once before the loop), as in the reference.

    Two rates: the solver ticks slowly, and between two ticks the plant is driven by the feedback policy the last solve
    holds, u = u_k + K_k (x - x_k) saturated at the BOX (`policy`, altro_batch_eval_policy_dev), also without the host:

        loop = ExternalMPC(solver)
        for i in range(ticks):
            u, *_ = loop.tick(x, Xref[i], Uref[i])                 # 50-100 Hz
            for s in range(S):                                     # 1 kHz: S plant substeps per tick
                x = plant(x, u)
                u = loop.policy(x, out=u)                          # knot 0: the tick period is one knot

    (A loop whose ticks are several knots apart passes the knot each instance is at as an int32 tensor, `knot=`.)"""

    def __init__(self, solver, shift=True):
        self.solver = solver
        self.shift = bool(shift)
        self.i = 0

    def tick(self, x0, Xref=None, Uref=None, dynamics=None, out=None, active=None, restart=None, U_restart=None,
             constraint_data=None, bounds=None, candidates=None, candidate_rho=0.0):
        """x0 (B, n); Xref (B, N, n) and Uref (B, N-1, m): the new reference window (both or neither); dynamics: an
        api.LinearModel of column-major-stored tensors (api module docstring) -- all GPU tensors on the solver's device.
        active (B,) int32: the instances this tick shifts and solves; it stays set as the solver's mask (api.set_active).
        restart (B,) int32: instances that start cold this tick (api.restart_instances) from the controls U_restart
        (B, N-1, m; default Uref) -- they are not shifted, and are solved if active.  With neither, a mask the solver holds
        stays in force; restart without active means every instance is active, and leaves no mask set.  For an inactive
        instance the tensors returned hold its last values.
        constraint_data {con: (A, b)}: new data of LINEAR / SOC constraints (index into the problem's constraint list; A or b
        may be None), bounds (zmin, zmax): new rows of the BOX -- GPU tensors (api.update_constraint_data / api.set_bounds),
        applied after the primal shift and before the dual shift, the order of the reference's grasp loop
        (grasp_mpc.jl:60-75).
        candidates (B, ncand, N-1, m) or (B, N-1, m): control sequences that compete with the shifted solution for this tick's
        warm start under merit = J + candidate_rho * c_max (api.warm_start with the incumbent included, so a tick never starts
        worse than the shifted solution under that merit) -- after this tick's setters, shift, constraint data and final
        mask, immediately before the solve.
        Returns (u0, x1, status, iterations) as api.first_knot does (out: tensors to write into)."""
        s = self.solver
        if not api._on_gpu(x0):
            raise ValueError("ExternalMPC.tick takes GPU tensors; the numpy loop is api.set_initial_state / shift_fill / solve")
        if (Xref is None) != (Uref is None):
            raise ValueError("tick: give Xref and Uref together")
        if candidates is not None:   # refused before anything of this tick is enqueued
            api.check_device_tensor(candidates, api._warm_start_args(s, candidates, candidate_rho, True)[1], s.device, "candidates")
        shift_mask = None
        if restart is not None:
            if U_restart is None:
                U_restart = Uref
            if U_restart is None:
                raise ValueError("tick: restart needs U_restart (or the Uref of the same tick)")
            if self.shift:   # mask arithmetic on the caller's stream, before the bracket: a restarted instance is not shifted
                import torch
                on = active if active is not None else torch.ones_like(restart)
                shift_mask = ((on != 0) & (restart == 0)).to(torch.int32)
        _lib.check_single_runtime()
        api.wait_stream(s)
        try:
            api._set_initial_state_dev(s, x0)
            if Xref is not None:
                api._update_trajectory_dev(s, Xref, Uref)
            if dynamics is not None:
                api._set_dynamics_dev(s, dynamics)
            if restart is not None:
                api._restart_instances_dev(s, restart, U_restart)
            if self.shift:
                if shift_mask is not None:
                    api._set_active_dev(s, shift_mask)
                elif active is not None:
                    api._set_active_dev(s, active)
                if constraint_data or bounds is not None:
                    api.shift_fill(s, True, False)
                    self._constraints_dev(constraint_data, bounds)
                    api.shift_fill(s, False, True)
                else:
                    api.shift_fill(s, True, True)
            else:
                self._constraints_dev(constraint_data, bounds)
            if active is not None:
                api._set_active_dev(s, active)
            elif shift_mask is not None:     # no mask given: the shift's was this tick's own
                api.set_active(s, None)
            if candidates is not None:
                api._warm_start_dev(s, candidates, candidate_rho, True, (None, None, None))
            api.solve_async(s)
            res = api._first_knot_dev(s, out)
        finally:
            api.signal_stream(s)
        self.i += 1
        return res

    def policy(self, x, knot=None, clamp=True, out=None):
        """u (B, m) = u_k + K_k (x - x_k) of the trajectory and gains the solver holds once its stream reaches this point,
        saturated at the BOX when clamp (api.eval_policy, device form): x (B, n) float64 and knot (B,) int32 GPU tensors
        (knot None: knot 0), out: a tensor to write into.  Ordered against torch's current stream like tick; no host
        synchronisation."""
        if not api._on_gpu(x):
            raise ValueError("ExternalMPC.policy takes GPU tensors; the numpy form is api.eval_policy")
        return api.eval_policy(self.solver, x, knot=knot, clamp=clamp, out=out)

    def evaluate(self, U=None, X=None, x0=None, out=None, Xout=None):
        """(J, c_max, defect) of candidate trajectories against the problem the next tick's solve would see once the solver's
        stream reaches this point (api.evaluate): a pass-through, GPU tensors or numpy."""
        return api.evaluate(self.solver, U, X=X, x0=x0, out=out, Xout=Xout)

    def merit(self, U, x0=None, rho=0.0):
        """M = J + rho P of candidate control sequences against the problem the next tick's solve would see, as a tensor torch
        differentiates once with respect to U and x0 (api.merit): a pass-through, GPU tensors."""
        return api.merit(self.solver, U, x0=x0, rho=rho)

    def sensitivity(self, **kw):
        """the solver's augmented Lagrangian of the controls it holds (or of U=...), its stationarity residual gU and the
        derivatives of the optimal cost with respect to x0, the reference, the cost weights and the box bounds, against the
        problem the next tick's solve would see (api.evaluate_al): a pass-through, GPU tensors or numpy."""
        return api.evaluate_al(self.solver, **kw)

    def solution_vjp(self, gX=None, gU=None, out=None):
        """the gradients of a loss on the solution the solver holds with respect to x0 and the reference, through the stored
        gains (api.solution_vjp): a pass-through, GPU tensors or numpy."""
        return api.solution_vjp(self.solver, gX=gX, gU=gU, out=out)

    def solution_vjp_data(self, gX=None, gU=None, per_knot=False, out=None):
        """the gradients of a loss on the solution the solver holds with respect to the cost weights, the box bounds and the
        dynamics, through the stored gains and the active set of their pass (api.solution_vjp_data): a pass-through, GPU
        tensors or numpy."""
        return api.solution_vjp_data(self.solver, gX=gX, gU=gU, per_knot=per_knot, out=out)

    def solution_jvp(self, vx0=None, vXref=None, vUref=None, out=None):
        """the directional derivatives of the solution the solver holds along tangents of x0 and the reference, through the
        stored gains (api.solution_jvp): a pass-through, GPU tensors or numpy."""
        return api.solution_jvp(self.solver, vx0=vx0, vXref=vXref, vUref=vUref, out=out)

    def warm_start(self, U, rho=0.0, include_current=True, out=None):
        """(chosen, J, c_max) of api.warm_start: the best of the candidates U (and the trajectory held, when include_current)
        becomes the initial trajectory of the next tick's solve once the solver's stream reaches this point: a pass-through,
        GPU tensors or numpy."""
        return api.warm_start(self.solver, U, rho=rho, include_current=include_current, out=out)

    def simulate(self, x0=None, w=None, nsamp=None, clamp=True, out=None, fb=None, Xout=None, Uout=None):
        """(J, c_max, dx_max) of api.simulate_policy: the policy the solver holds once its stream reaches this point, run in
        closed loop on the model from the start states x0 (B, nsamp, n) under the disturbances w (B, nsamp, N-1, n) -- what the
        last solve is worth if the state estimate is off or the plant is pushed: a pass-through, GPU tensors or numpy."""
        return api.simulate_policy(self.solver, x0=x0, w=w, nsamp=nsamp, clamp=clamp, out=out, fb=fb, Xout=Xout, Uout=Uout)

    def covariance(self, Sigma0=None, W=None, con_id=None, kappa=None, out=None):
        """The dict of api.propagate_covariance: the covariance of the closed loop under the policy the solver holds once its
        stream reaches this point, from the covariance Sigma0 of the state estimate and W of the disturbance per step -- the
        standard deviations of states, controls and constraint rows, the expected cost increase and, with kappa, a box pulled
        in by kappa deviations that set_bounds takes as it is: a pass-through, GPU tensors or numpy."""
        return api.propagate_covariance(self.solver, Sigma0=Sigma0, W=W, con_id=con_id, kappa=kappa, out=out)

    def cost_to_go(self, penalty=False, out=None):
        """The dict of api.cost_to_go: the quadratic cost-to-go (P, p, v) of the policy the solver holds once its stream reaches
        this point, around the trajectory it holds -- the second order of the optimal cost in x0, the expected cost increase
        for every (Sigma0, W) at once: a pass-through, GPU tensors or numpy."""
        return api.cost_to_go(self.solver, penalty=penalty, out=out)

    def _constraints_dev(self, constraint_data, bounds):
        s = self.solver
        for con, (A, b) in (constraint_data or {}).items():
            api._update_constraint_data_dev(s, con, A, b)
        if bounds is not None:
            box = [k for k, (c, _, _) in enumerate(s.prob.constraints.items) if isinstance(c, api.BoundConstraint)]
            if not box:
                raise ValueError("tick: bounds given, but the problem has no BoundConstraint")
            api._set_bounds_dev(s, box[0], *bounds)


def _add_specs(cons, specs, n, m):
    from . import problems as P
    for c in specs:
        if c.kind == P.BOX:
            cons.add_constraint(api.BoundConstraint(n, m, u_min=c.zmin[n:], u_max=c.zmax[n:]), (c.k_first + 1, c.k_last + 1))
        else:
            con = api.NormConstraint(c.A, c.b) if c.kind == P.SOC else api.LinearConstraint(c.A, c.b, equality=(c.sense == P.EQ))
            cons.add_constraint(con, (c.k_first + 1, c.k_last + 1))


def constrained_problem(data, x0, Xref=None, Uref=None, U0=None, constraints=None):
    """Problem(model, objective, ...; constraints) for the rocket / grasp data of problems.py
    (rocket_landing_problem.jl:66-186, grasp_problem.jl:1-107): x0 is (B, n); the reference
    defaults to the goal state, the initial controls to the data's guess."""
    B = x0.shape[0]
    model = api.LinearModel(data.A, data.Bm, data.f, dt=data.dt)
    Xr = np.tile(data.xf, (B, data.N, 1)) if Xref is None else Xref
    Ur = np.zeros((B, data.N - 1, data.m)) if Uref is None else Uref
    obj = api.TrackingObjective(data.Q, data.R, data.Qf, Xr, Ur)
    cons = api.ConstraintList(data.n, data.m, data.N)
    _add_specs(cons, data.constraints if constraints is None else constraints, data.n, data.m)
    return api.Problem(model, obj, cons, x0=x0, N=data.N, U0=np.tile(data.U0, (B, 1, 1)) if U0 is None else U0)


def quadruped_problem(qp, x0, A, Bm, d):
    """AltroParams (Structs/ALTROParams.jl:32-108) for a batch: x0 (B, 12); A, Bm, d per instance
    and per knot, (B, N-1, 12, 12) and (B, N-1, 12)."""
    B = x0.shape[0]
    model = api.LinearModel(A, Bm, d, dt=qp.dt, per_knot=True)
    obj = api.TrackingObjective(qp.Q, qp.R, qp.Q, np.tile(qp.x_des, (B, qp.N, 1)), np.zeros((B, qp.N - 1, qp.m)))
    cons = api.ConstraintList(qp.n, qp.m, qp.N)
    _add_specs(cons, qp.constraints, qp.n, qp.m)
    return api.Problem(model, obj, cons, x0=x0.copy(), N=qp.N, U0=np.tile(qp.u_hover, (B, qp.N - 1, 1)))
