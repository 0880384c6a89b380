"""What one altro_batch_simulate_policy_dev call costs, beside the same study written with the calls a caller had
before it, on the same tensors in the same run: per sample and knot one altro_batch_eval_policy_dev and a torch plant step
(x <- A x + B u + w, two bmm and two additions on a (batch, n) state), then one altro_batch_evaluate_dev (given form) on the
trajectories collected.  batch 8192, nsamp 8, the 16-lane backend at (12, 4, N = 50) and the one-wave-per-instance backend at
(32, 16, N = 21), box-constrained random-linear problems solved once, disturbed starts and disturbances of relative size 1e-2.
HIP events on torch's stream around a window of back-to-back calls, each call ordered against torch's stream by its own
wait_stream / signal_stream (the public wrappers), device time per call = window / calls; two warm-up windows, then the median,
minimum and maximum over the windows, the variants alternating window by window.  The composition is (N - 1) * nsamp launch
pairs per call and is timed with fewer, shorter windows.
bytes_moved: what the fused call cannot avoid -- x0, w, the gains, the nominal trajectory, the reference window, the dynamics,
cost and bounds tables, J, c_max, dx_max, fb; state_bytes: the states and controls the composition moves on top (x read and
written at every knot by the policy and the plant step, X and U written and read again by the scoring).
bench: `bench.py --gpus 1 --steps 20 --warmup 5`, three runs of this build and, when a build of the parent commit is given,
three of it, alternating -- separate processes, before this one touches the GPU.
Usage: gpu_simulate_timing.py out.json [batch] [parent libaltro_hip.so]"""
import json, os, statistics, subprocess, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
WINDOWS, WARM, REPS, NSAMP = 20, 2, 10, 8
C_WINDOWS, C_REPS = 5, 1


def main(path, B, parent):
    bench_rows = bench(parent)     # first: child processes are started before this one opens the GPU
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    res = {"batch": B, "nsamp": NSAMP, "windows": WINDOWS, "calls_per_window": REPS, "composition_windows": C_WINDOWS,
           "composition_calls_per_window": C_REPS,
           "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)", "shapes": []}
    for n, m, N in ((12, 4, 50), (32, 16, 21)):
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        wide = (n, m) != (12, 4)
        rng = np.random.default_rng(2)
        Xbar = api.states(sv)
        x0 = T(Xbar[:, None, 0] + 1e-2 * (1.0 + np.abs(Xbar[:, None, 0])) * rng.standard_normal((B, NSAMP, n)))
        w = T(1e-2 * (1.0 + np.abs(Xbar[:, None, 1:])) * rng.standard_normal((B, NSAMP, N - 1, n)))
        A, Bm = T(pb.A), T(pb.Bm)
        J, c, dx = (torch.empty((B, NSAMP), dtype=torch.float64, device=dev) for _ in range(3))
        Jc, cc = (torch.empty((B, NSAMP), dtype=torch.float64, device=dev) for _ in range(2))
        fb = torch.empty((B,), dtype=torch.int32, device=dev)
        Xo, Uo = torch.empty((B, NSAMP, N, n), dtype=torch.float64, device=dev), torch.empty((B, NSAMP, N - 1, m), dtype=torch.float64, device=dev)
        Xc, Uc = torch.empty_like(Xo), torch.empty_like(Uo)
        knots = [torch.full((B,), k, dtype=torch.int32, device=dev) for k in range(N - 1)]
        u = torch.empty((B, m), dtype=torch.float64, device=dev)

        def fused():
            api.simulate_policy(sv, x0, w, out=(J, c, dx), fb=fb)

        def fused_traj():
            api.simulate_policy(sv, x0, w, out=(J, c, dx), fb=fb, Xout=Xo, Uout=Uo)

        def composition():
            for s in range(NSAMP):
                x = x0[:, s].contiguous()
                for k in range(N - 1):
                    Xc[:, s, k] = x
                    api.eval_policy(sv, x, knot=knots[k], clamp=True, out=u)
                    Uc[:, s, k] = u
                    x = torch.bmm(A, x.unsqueeze(-1)).squeeze(-1) + torch.bmm(Bm, u.unsqueeze(-1)).squeeze(-1) + w[:, s, k]
                Xc[:, s, N - 1] = x
            api.evaluate(sv, Uc, X=Xc, out=(Jc, cc, None))

        # the two are the same study: the composition's torch plant step sums in another order, so the states agree to rounding
        fused_traj()
        composition()
        torch.cuda.synchronize()
        agree = float((Xo - Xc).abs().max() / Xo.abs().max())
        print("(%d, %d, %d): fb %s, max |X fused - X composition| / max |X| = %.2e, max |J diff| / J = %.2e"
              % (n, m, N, sorted(set(fb.tolist())), agree, float(((J - Jc).abs() / J).max())), flush=True)
        calls = {"simulate_policy_dev": (fused, WINDOWS, REPS), "simulate_policy_dev + Xout, Uout": (fused_traj, WINDOWS, REPS),
                 "composition": (composition, C_WINDOWS, C_REPS)}
        times = {k: [] for k in calls}
        for wdw in range(WINDOWS + WARM):
            for name, (fn, nw, reps) in calls.items():       # the variants alternate window by window
                if wdw >= nw + WARM:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                api.synchronize(sv)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if wdw >= WARM:
                    times[name].append(1e3 * e0.elapsed_time(e1) / reps)
        Rr = B * NSAMP
        tables = B * (n * (n + m) + n) + B * N * (n + m) + 4 * (n + m)          # dynamics, reference window, weights and bounds
        gains = B * (N - 1) * m * (16 if not wide else n) + B * N * (16 if not wide else n + m)   # gain rows and the nominal trajectory
        base = (Rr * n + Rr * (N - 1) * n + tables + gains + 3 * Rr) * 8 + B * 4
        traj = (Rr * N * n + Rr * (N - 1) * m) * 8
        row = {"n": n, "m": m, "N": N, "backend": "one-wave-per-instance" if wide else "16-lane", "relative_state_difference": agree, "calls": {}}
        for name, v in times.items():
            med = statistics.median(v)
            row["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v, "bytes_moved": base + (traj if "Xout" in name else 0),
                                  "state_bytes": (2 * traj + 3 * Rr * (N - 1) * n * 8) if name == "composition" else 0}
            print("(%d, %d, %d) %-34s median %11.1f us  min %11.1f  max %11.1f" % (n, m, N, name, med, min(v), max(v)), flush=True)
        co, fu = row["calls"]["composition"], row["calls"]["simulate_policy_dev"]
        row["composition_over_fused"] = co["median_us"] / fu["median_us"]
        row["faster_than_composition"] = bool(fu["max_us"] < co["min_us"])
        print("   composition / fused: %.1f" % row["composition_over_fused"], flush=True)
        res["shapes"].append(row)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        sv.close()
    res["bench"] = bench_rows
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def bench(parent, runs=3):
    """the bench line of this build and of the parent's, `runs` processes each, alternating"""
    out = {"command": "bench.py --gpus 1 --steps 20 --warmup 5", "this": [], "parent": []}
    for _ in range(runs):
        for name, lib in (("this", None), ("parent", parent)):
            if name == "parent" and not lib:
                continue
            e = dict(os.environ)
            if lib:
                e["ALTRO_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.join(R, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], env=e,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                raise RuntimeError("bench.py failed (%s): %s" % (name, p.stdout[-2000:]))
            out[name].append(json.loads(lines[-1]))
            print("bench", name, lines[-1][:300], flush=True)
    return out


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8192, sys.argv[3] if len(sys.argv) > 3 else None)
