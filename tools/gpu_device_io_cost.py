"""What a closed-loop tick costs with host I/O and with device-pointer I/O: wall-clock per tick, everything the
host does included, in alternating windows, every configuration in a process of its own.  Raw times go to the JSON file.
  quad_host / quad_dev   the quadruped tick (batch 2048, N = 40, per-instance per-knot dynamics): host setters / getters, or
                         mpc.ExternalMPC.tick with tensors
  ext_host / ext_dev     a one-step external tick on the headline shape (batch 8192, (12, 4, 50)): x0 and reference window in,
                         first control and status out; beside both the device time of the solve alone
  pack                   16-lane backend: the _dev setters of x0 and of a reference window, packing from the caller's pointer
                         or after a copy into the staging buffer ("dev_via_stage")
Usage: gpu_device_io_cost.py out.json tag=lib.so:mode [tag=lib.so:mode ...]     (mode: one of the names above; the host modes
run on any build, e.g. one of the parent commit)"""
import json, os, statistics, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
W, K = 6, 10          # windows per run, ticks per window


def child(mode):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {"ms_per_tick": [], "solve_ms": []}
    if mode.startswith("quad"):
        B, N = 2048, 40
        qp = problems.gen_quadruped_problem(N=N)
        rng = np.random.default_rng(7)
        phases = rng.uniform(0.0, 0.8, 16)
        idx = np.arange(B) % 16
        tabs = [[np.stack(a) for a in zip(*[qp.dynamics(ph + i * qp.dt) for ph in phases])] for i in range(W * K + 1)]
        x0 = qp.x_des + rng.standard_normal((B, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
        noise = rng.standard_normal((W * K, B, 12))
        sv = api.ALTROSolver(mpc.quadruped_problem(qp, x0, *[a[idx] for a in tabs[0]]), api.SolverOptions(**problems.QUADRUPED_OPTS))
        api.solve(sv)
        if mode == "quad_dev":
            At = T(np.swapaxes(np.array([t[0] for t in tabs]), -1, -2)); Bt = T(np.swapaxes(np.array([t[1] for t in tabs]), -1, -2))
            dt_, nz, ix = T(np.array([t[2] for t in tabs])), T(noise), T(idx)
            loop = mpc.ExternalMPC(sv)
            x1 = api.first_knot(sv)[1]
        for w in range(W):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(K):
                i = w * K + k + 1
                if mode == "quad_dev":
                    mdl = api.LinearModel(At[i].index_select(0, ix).transpose(-1, -2), Bt[i].index_select(0, ix).transpose(-1, -2),
                                          dt_[i].index_select(0, ix), dt=qp.dt, per_knot=True)
                    _, x1, st, it = loop.tick(x1 + nz[i - 1] * 1e-3, dynamics=mdl)
                else:
                    xn = api.states(sv)[:, 1] + 1e-3 * noise[i - 1]
                    api.set_dynamics(sv, api.LinearModel(*[a[idx] for a in tabs[i]], dt=qp.dt, per_knot=True))
                    api.set_initial_state(sv, xn)
                    api.shift_fill(sv, True, True)
                    api.solve(sv)
                    st = api.stats(sv).status
            torch.cuda.synchronize()
            out["ms_per_tick"].append(1e3 * (time.perf_counter() - t0) / K)
            out["solve_ms"].append(api.stats(sv).tsolve_ms)
    elif mode.startswith("ext"):
        B, n, m, N = 8192, 12, 4, 50
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=W * K + 1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        A, Bm, nz, Xt, Ut = T(pb.A), T(pb.Bm), T(pb.noise), T(pb.Xtrack), T(pb.Utrack)
        x = T(pb.Xtrack[:, 0]); xh = pb.Xtrack[:, 0].copy()
        loop = mpc.ExternalMPC(sv)
        u0 = api.first_knot(sv)[0] if mode == "ext_dev" else None
        for w in range(W):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(K):
                i = w * K + k
                if mode == "ext_dev":
                    x = torch.bmm(A, x.unsqueeze(-1)).squeeze(-1) + torch.bmm(Bm, u0.unsqueeze(-1)).squeeze(-1)
                    x = x + nz[i] * (0.01 * x.abs().amax(dim=1, keepdim=True))
                    u0, _, st, it = loop.tick(x, Xt[:, i + 1:i + 1 + N].contiguous(), Ut[:, i + 1:i + N].contiguous())
                else:
                    u0h = api.controls(sv)[:, 0]
                    xh = np.einsum("bij,bj->bi", pb.A, xh) + np.einsum("bij,bj->bi", pb.Bm, u0h)
                    xh = xh + pb.noise[i] * 0.01 * np.abs(xh).max(axis=1, keepdims=True)
                    api.set_initial_state(sv, xh)
                    api.update_trajectory(sv, *pb.window(i + 1))
                    api.shift_fill(sv, True, True)
                    api.solve(sv)
                    st = api.stats(sv).status
            torch.cuda.synchronize()
            out["ms_per_tick"].append(1e3 * (time.perf_counter() - t0) / K)
            out["solve_ms"].append(api.stats(sv).tsolve_ms)
    else:   # pack
        B, n, m, N, reps = 8192, 12, 4, 50, 200
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        x0, Xr, Ur = T(pb.Xtrack[:, 0]), T(pb.Xtrack[:, :N]), T(pb.Utrack[:, :N - 1])
        out = {}
        for w in range(W):
            for via in (0, 1):
                altro.debug_set("dev_via_stage", via, sv.h)
                for name, fn in (("x0", lambda: api._set_initial_state_dev(sv, x0)), ("ref", lambda: api._update_trajectory_dev(sv, Xr, Ur))):
                    fn(); api.synchronize(sv)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    api.wait_stream(sv); e0.record(); api.wait_stream(sv)
                    for _ in range(reps):
                        fn()
                    api.signal_stream(sv); e1.record(); torch.cuda.synchronize()
                    out.setdefault("%s_%s_us" % (name, "via_stage" if via else "direct"), []).append(1e3 * e0.elapsed_time(e1) / reps)
    print(json.dumps(out), flush=True)


if len(sys.argv) == 3 and sys.argv[1] == "--child":
    child(sys.argv[2])
else:
    path, cfgs = sys.argv[1], sys.argv[2:]
    res = {"windows_per_run": W, "ticks_per_window": K, "unit": "wall-clock ms per tick (mean of a window); solve_ms: device time of the window's last solve", "runs": []}
    for rep in range(2):
        for a in cfgs:
            tag, rest = a.split("=", 1)
            lib, mode = rest.rsplit(":", 1)
            e = dict(os.environ); e["ALTRO_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=e, stdout=subprocess.PIPE, text=True, timeout=400)
            if p.returncode != 0:
                sys.exit("run %s failed with status %d" % (tag, p.returncode))     # nothing more is started on the device
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res["runs"].append({"tag": tag, "mode": mode, "rep": rep, **r})
            print("%-14s" % tag, {k: [round(x, 3) for x in v] for k, v in r.items()}, flush=True)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
    for tag in dict.fromkeys(r["tag"] for r in res["runs"]):
        keys = [k for k in res["runs"][[r["tag"] for r in res["runs"]].index(tag)] if k not in ("tag", "mode", "rep")]
        for k in keys:
            v = [x for r in res["runs"] if r["tag"] == tag for x in r[k]]
            print("%-14s %-20s median %.3f  min %.3f  max %.3f  (%d)" % (tag, k, statistics.median(v), min(v), max(v), len(v)))
