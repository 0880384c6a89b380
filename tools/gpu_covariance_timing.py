"""What one altro_batch_propagate_covariance_dev call costs, beside the cheapest earlier way to the same matrices
when W = 0: altro_batch_simulate_policy_dev with nsamp = n unit starts (x0 = xbar_0 + e_j), w = NULL, clamp = 0 and Xout, whose
deviations are the columns of the state-transition products.  Batch 8192, box-constrained random-linear problems solved once:
(12, 4, N = 50) on the 16-lane backend, (32, 4, 50) and (64, 4, 50) on the one-wave-per-instance backend.
HIP events on torch's stream around a window of back-to-back calls, each call ordered against torch's stream by its own
wait_stream / signal_stream (the public wrappers), device time per call = window / calls; two warm-up windows, then the median,
minimum and maximum over the windows, the two calls alternating window by window.
flops: the two n x n x n products per knot at the unpadded size, 4 n^3 (N - 1) per instance (M, the diagonals and the rows are
left out), so the rate printed is a lower bound of what the units did.
Usage: gpu_covariance_timing.py out.json [batch]"""
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
    res = {"batch": B, "windows": WINDOWS, "calls_per_window": REPS,
           "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)", "shapes": []}
    for n, m, N in ((12, 4, 50), (32, 4, 50), (64, 4, 50)):
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=10)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        rng = np.random.default_rng(2)
        L0 = 0.05 / np.sqrt(n) * rng.standard_normal((n, n))
        S0, W = T(L0 @ L0.T), T(0.01 * L0 @ L0.T)
        out = {"sx": torch.empty((B, N, n), dtype=torch.float64, device=dev), "su": torch.empty((B, N - 1, m), dtype=torch.float64, device=dev),
               "dJ": torch.empty((B,), dtype=torch.float64, device=dev), "fb": torch.empty((B,), dtype=torch.int32, device=dev),
               "zmin_t": torch.empty((B, n + m), dtype=torch.float64, device=dev), "zmax_t": torch.empty((B, n + m), dtype=torch.float64, device=dev)}
        Xbar = api.states(sv)
        x0 = T(Xbar[:, None, 0] + np.eye(n)[None])
        Xo = torch.empty((B, n, N, n), dtype=torch.float64, device=dev)

        def covariance():
            api.propagate_covariance(sv, S0, W, kappa=2.0, out=out)

        def simulate():
            api.simulate_policy(sv, x0, None, clamp=False, out=(None, None, None), Xout=Xo)

        calls = {"propagate_covariance_dev": covariance, "simulate_policy_dev nsamp = n": simulate}
        times = {k: [] for k in calls}
        for wdw in range(WINDOWS + WARM):
            for name, fn in calls.items():       # the two alternate window by window
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
        row = {"n": n, "m": m, "N": N, "backend": "16-lane" if n <= 16 else "one-wave-per-instance", "fb": sorted(set(out["fb"].tolist())),
               "flops_per_call": flops, "calls": {}}
        for name, v in times.items():
            med = statistics.median(v)
            row["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v}
            print("(%d, %d, %d) %-32s median %11.1f us  min %11.1f  max %11.1f" % (n, m, N, name, med, min(v), max(v)), flush=True)
        row["fp64_tflops"] = flops / row["calls"]["propagate_covariance_dev"]["median_us"] * 1e-6
        print("   covariance: %.2f TFLOP/s FP64 (products only, unpadded)" % row["fp64_tflops"], flush=True)
        res["shapes"].append(row)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        sv.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8192)
