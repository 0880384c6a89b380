"""What one altro_batch_cost_to_go_dev call costs, with P0, p0, v0 only and with the full tracks P, p, v, beside
altro_batch_propagate_covariance_dev on the same handle -- its transpose (S' = M S M' + W against P = H + K'Hu K + M'P M) and so
the natural yardstick.  Batch 8192, box-constrained random-linear problems solved once: (12, 4, N = 50) on the 16-lane backend,
(32, 4, 50) and (64, 4, 50) on the one-wave-per-instance backend; mode 0 (mode 1 adds two loads and a few selects per knot and
lane to the same products).
HIP events on torch's stream around a window of back-to-back calls, each call ordered against torch's stream by its own
wait_stream / signal_stream (the public wrappers), device time per call = window / calls; two warm-up windows, then the median,
minimum and maximum over the windows, the calls alternating window by window.
flops: the two n x n x n products per knot at the unpadded size, 4 n^3 (N - 1) per instance (M, K'Hu K and p are left out), so
the rate printed is a lower bound of what the units did.
Usage: gpu_cost_to_go_timing.py out.json [batch]"""
import json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
WINDOWS, WARM, REPS = 10, 2, 5


def main(path, B):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    E = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    res = {"batch": B, "windows": WINDOWS, "calls_per_window": REPS,
           "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)", "shapes": []}
    for n, m, N in ((12, 4, 50), (32, 4, 50), (64, 4, 50)):
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=10)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        rng = np.random.default_rng(2)
        L0 = 0.05 / np.sqrt(n) * rng.standard_normal((n, n))
        S0, W = T(L0 @ L0.T), T(0.01 * L0 @ L0.T)
        fb = torch.empty((B,), dtype=torch.int32, device=dev)
        head = {"P0": E(B, n, n), "p0": E(B, n), "v0": E(B), "fb": fb}
        full = dict(head, P=E(B, N, n, n), p=E(B, N, n), v=E(B, N))
        cov = {"sx": E(B, N, n), "su": E(B, N - 1, m), "dJ": E(B), "fb": torch.empty((B,), dtype=torch.int32, device=dev)}
        calls = {"cost_to_go_dev P0 p0 v0": lambda: api.cost_to_go(sv, out=head),
                 "cost_to_go_dev full tracks": lambda: api.cost_to_go(sv, out=full),
                 "propagate_covariance_dev": lambda: api.propagate_covariance(sv, S0, W, out=cov)}
        times = {k: [] for k in calls}
        for wdw in range(WINDOWS + WARM):
            for name, fn in calls.items():       # the calls alternate window by window
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                api.synchronize(sv)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(REPS):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if wdw >= WARM:
                    times[name].append(1e3 * e0.elapsed_time(e1) / REPS)
        flops = 4.0 * n ** 3 * (N - 1) * B
        row = {"n": n, "m": m, "N": N, "backend": "16-lane" if n <= 16 else "one-wave-per-instance", "fb": sorted(set(fb.tolist())),
               "flops_per_call": flops, "calls": {}}
        for name, v in times.items():
            med = statistics.median(v)
            row["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v}
            print("(%d, %d, %d) %-28s median %11.1f us  min %11.1f  max %11.1f" % (n, m, N, name, med, min(v), max(v)), flush=True)
        row["fp64_tflops"] = flops / row["calls"]["cost_to_go_dev P0 p0 v0"]["median_us"] * 1e-6
        print("   cost to go: %.2f TFLOP/s FP64 (products only, unpadded)" % row["fp64_tflops"], flush=True)
        res["shapes"].append(row)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        del head, full, cov
        sv.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8192)
