"""What one altro_batch_eval_policy_dev launch costs, beside altro_batch_get_first_knot_dev on the same handle in
the same run: HIP events on torch's stream around a window of back-to-back launches on the solver's stream (wait_stream before
the first, signal_stream after the last), device time per launch = window / launches; warm-up first, then the median over the
windows.  knot = NULL and a random knot array; the 16-lane backend at (12, 4, N = 50) and the one-wave-per-instance backend at
(32, 16, N = 21).  Also the bytes the call must move over the time.
Usage: gpu_policy_eval.py out.json [batch]"""
import json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
WINDOWS, LAUNCHES = 20, 50


def main(path, B):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    res = {"batch": B, "windows": WINDOWS, "launches_per_window": LAUNCHES,
           "unit": "device microseconds per launch (HIP events around a window of back-to-back launches / launches)", "shapes": []}
    for n, m, N in ((12, 4, 50), (32, 16, 21)):
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        rng = np.random.default_rng(2)
        x = T(api.states(sv)[:, 0] + 1e-2 * rng.standard_normal((B, n)))
        knot = T(rng.integers(0, N - 1, B).astype(np.int32))
        u = torch.empty((B, m), dtype=torch.float64, device=dev)
        fb = torch.empty((B,), dtype=torch.int32, device=dev)
        fk = api._first_knot_dev(sv)
        calls = {"eval_policy_dev knot=NULL": lambda: api._eval_policy_dev(sv, x, None, True, u, fb),
                 "eval_policy_dev random knot": lambda: api._eval_policy_dev(sv, x, knot, True, u, fb),
                 "get_first_knot_dev": lambda: api._first_knot_dev(sv, fk)}
        times = {k: [] for k in calls}
        for w in range(WINDOWS + 2):                       # two warm-up windows
            for name, fn in calls.items():                 # the calls alternate window by window
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                api.synchronize(sv)
                e0.record()
                api.wait_stream(sv)
                for _ in range(LAUNCHES):
                    fn()
                api.signal_stream(sv)
                e1.record()
                torch.cuda.synchronize()
                if w >= 2:
                    times[name].append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
        assert int((fb.cpu() == 1).sum()) == B
        wide = not ((n, m) == (12, 4))
        nbytes = B * ((n + m * 16 + n + m) if not wide else (n + m * n + n + m + m)) * 8
        row = {"n": n, "m": m, "N": N, "backend": "one-wave-per-instance" if wide else "16-lane", "bytes_moved": nbytes, "calls": {}}
        for name, v in times.items():
            med = statistics.median(v)
            row["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v}
            if name.startswith("eval"):
                row["calls"][name]["GB_per_s"] = nbytes / (med * 1e-6) / 1e9
            print("(%d, %d, %d) %-30s median %.2f us  min %.2f  max %.2f" % (n, m, N, name, med, min(v), max(v)), flush=True)
        res["shapes"].append(row)
        sv.close()
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8192)
