"""What a tick that rewrites constraint data or box bounds costs on the host path and on the device path:
wall-clock and HIP-event time per tick, everything the host does included, in alternating windows, every configuration in a
process of its own.  Raw times go to the JSON file.
  grasp_host_shared / grasp_dev_shared   the grasp tick (batch 4096, (6, 6), N = 21): x0, primal shift, all four per-knot
                                         constraints rewritten, dual shift, solve, status out; tables shared by the batch
  grasp_host_pi / grasp_dev_pi           the same with one table per instance (per_knot = 3)
  bounds_host / bounds_dev               (12, 4, 50) x 8192: x0, one row of bounds per instance, shift, solve, status out
  headline                               the 20-step fused launch of the headline workload (8192 x (12, 4, 50)): device time of
                                         the launch, to show that it does not move between two builds
The host modes and `headline` run on any build, e.g. one of the parent commit.
Usage: gpu_constraint_dev.py out.json tag=lib.so:mode [tag=lib.so:mode ...]"""
import json, os, statistics, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
W, K = 6, 50          # windows per run, ticks per window


def child(mode):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc, problems
    from altro_mpc_icra2021_amd.benchmarks import GRASP_MPC_OPTS
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {"ms_per_tick": [], "event_ms_per_tick": [], "solve_ms": []}
    on_dev = "_dev" in mode

    def windows(tick):
        """one untimed tick of the timed shape (code objects, and the one-time change of the bounds tables to one row per
        instance, stay out of the windows); then W windows of K ticks: wall clock and a pair of events on torch's current
        stream around each"""
        tick(1)
        for w in range(W):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for k in range(K):
                tick(w * K + k + 2)
            e1.record()
            torch.cuda.synchronize()
            out["ms_per_tick"].append(1e3 * (time.perf_counter() - t0) / K)
            out["event_ms_per_tick"].append(e0.elapsed_time(e1) / K)
            out["solve_ms"].append(api.stats(sv).tsolve_ms)

    if mode.startswith("grasp"):
        B, N, spread = 4096, 21, 16
        pi = mode.endswith("_pi")
        nk = W * K + 2 + spread + N
        gp = problems.gen_grasp_problem(N=nk + 1, tf=0.1 * nk)
        tabs = [(c.kind == problems.SOC, c.sense == problems.EQ, c.A, c.b) for c in gp.constraints[1:]]
        rng = np.random.default_rng(3)
        xs = np.tile(gp.x0, (W * K + 2, B, 1)) + 0.02 * rng.standard_normal((W * K + 2, B, 6))
        idx = (np.arange(B) % spread)[:, None] + np.arange(N - 1)[None, :] if pi else np.arange(N - 1)   # knots of window 0
        Xr, Ur = np.tile(gp.x0, (B, N, 1)), np.tile(gp.U0[:N - 1], (B, 1, 1))
        cons = altro.ConstraintList(6, 6, N)
        for soc, eq, A, b in tabs:
            con = altro.NormConstraint(A[idx], b[idx], per_instance=pi) if soc else altro.LinearConstraint(A[idx], b[idx], equality=eq, per_instance=pi)
            cons.add_constraint(con, (1, N - 1))
        prob = altro.Problem(altro.LinearModel(gp.A, gp.Bm, gp.f, dt=gp.dt), altro.TrackingObjective(np.full(6, 1e3), np.full(6, 1.0), np.full(6, 10.0), Xr, Ur),
                             cons, x0=xs[0], N=N, U0=Ur.copy())
        sv = api.ALTROSolver(prob, api.SolverOptions(**GRASP_MPC_OPTS))
        api.solve(sv)
        if on_dev:
            tabs_d, xs_d, idx_d = [(T(A), T(b)) for _, _, A, b in tabs], T(xs), T(idx)
            loop = mpc.ExternalMPC(sv)

            def tick(i):
                data = {ci: (A[idx_d + i], b[idx_d + i]) for ci, (A, b) in enumerate(tabs_d)}    # the windows, gathered on the device
                loop.tick(xs_d[i], constraint_data=data)
        else:
            def tick(i):
                api.set_initial_state(sv, xs[i])
                api.shift_fill(sv, True, False)
                for ci, (_, _, A, b) in enumerate(tabs):
                    api.update_constraint_data(sv, ci, A[idx + i], b[idx + i])
                api.shift_fill(sv, False, True)
                api.solve(sv)
                api.stats(sv).status
        windows(tick)
    elif mode.startswith("bounds"):
        B, n, m, N = 8192, 12, 4, 50
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        rng = np.random.default_rng(5)
        P = 64                                                           # distinct (x0, bounds) inputs, taken in turn
        xs = pb.Xtrack[None, :, 0] + 0.05 * rng.standard_normal((P, B, n))
        hi = np.concatenate([np.full((P, B, n), np.inf), pb.u_bnd * (0.8 + 0.2 * rng.random((P, B, 1))) * np.ones((1, 1, m))], axis=2)
        if on_dev:
            xs_d, hi_d = T(xs), T(hi)
            lo_d = -hi_d
            loop = mpc.ExternalMPC(sv)
            tick = lambda i: loop.tick(xs_d[i % P], bounds=(lo_d[i % P], hi_d[i % P]))
        else:
            def tick(i):
                api.set_initial_state(sv, xs[i % P])
                api.set_bounds(sv, 0, -hi[i % P], hi[i % P])
                api.shift_fill(sv, True, True)
                api.solve(sv)
                api.stats(sv).status
        windows(tick)
    else:   # headline: device time of the 20-step fused launch
        S = 20
        pb = problems.gen_random_linear_batch(8192, n=12, m=4, N=50, steps=S * (W + 1), seed=1)
        mp = mpc.BatchMPC(pb)
        mp.initial_solve()
        out = {"launch_ms": []}
        for w in range(W + 1):
            mp.run_async(S, w * S)
            mp.synchronize()
            if w:                                                        # the first launch is the warm-up
                out["launch_ms"].append(api.stats(mp.solver).tsolve_ms)
    print(json.dumps(out), flush=True)


if len(sys.argv) == 3 and sys.argv[1] == "--child":
    child(sys.argv[2])
else:
    path, cfgs = sys.argv[1], sys.argv[2:]
    res = {"windows_per_run": W, "ticks_per_window": K,
           "unit": "ms per tick (mean of a window): wall clock, and HIP events around the window; solve_ms: device time of the window's last solve; "
                   "launch_ms: device time of one 20-step launch", "runs": []}
    for rep in range(2):
        for a in cfgs:
            tag, rest = a.split("=", 1)
            lib, mode = rest.rsplit(":", 1)
            e = dict(os.environ); e["ALTRO_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=e, stdout=subprocess.PIPE, text=True, timeout=500)
            if p.returncode != 0:
                sys.exit("run %s failed with status %d" % (tag, p.returncode))     # nothing more is started on the device
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res["runs"].append({"tag": tag, "mode": mode, "rep": rep, **r})
            print("%-18s" % tag, {k: [round(x, 3) for x in v] for k, v in r.items()}, flush=True)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
    for tag in dict.fromkeys(r["tag"] for r in res["runs"]):
        keys = [k for k in res["runs"][[r["tag"] for r in res["runs"]].index(tag)] if k not in ("tag", "mode", "rep")]
        for k in keys:
            v = [x for r in res["runs"] if r["tag"] == tag for x in r[k]]
            print("%-18s %-20s median %.3f  min %.3f  max %.3f  (%d)" % (tag, k, statistics.median(v), min(v), max(v), len(v)))
