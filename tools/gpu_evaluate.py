"""What one altro_batch_evaluate_dev launch costs, beside a torch implementation of the same rollout and scores
on the same tensors in the same run -- what a caller does today: a loop of N-1 batched FP64 matmuls for the states, then the
tracking cost and the box violation as a handful of vectorised operations.
HIP events on torch's stream around a window of back-to-back calls (the library's on the solver's stream between wait_stream
and signal_stream), device time per call = window / calls; two warm-up windows, then the median, minimum and maximum over 20
windows, the variants alternating window by window.  The 16-lane backend at (12, 4, N = 50) and the one-wave-per-instance
backend at (32, 16, N = 21), batch 8192, ncand 1 and 8; rollout form with and without Xout, and the given form.
bytes_moved: what the call cannot avoid -- U, x0, the reference window, the dynamics, cost and bounds tables, the outputs; the
states once when Xout is written or X is read (the rollout form without Xout still writes and re-reads them in its workspace:
that traffic is the call's own choice and is not counted).
Usage: gpu_evaluate.py out.json [batch]"""
import json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
WINDOWS, WARM = 20, 2


def main(path, B):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    res = {"batch": B, "windows": WINDOWS, "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)",
           "cases": []}
    for n, m, N in ((12, 4, 50), (32, 16, 21)):
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        wide = (n, m) != (12, 4)
        At, Bt = T(np.swapaxes(pb.A, -1, -2)), T(np.swapaxes(pb.Bm, -1, -2))          # x_{k+1} = x_k A' + u_k B'
        Xr, Ur, x0 = T(pb.Xtrack[:, :N])[:, None], T(pb.Utrack[:, :N - 1])[:, None], T(pb.Xtrack[:, 0])
        Q, Rw, Qf, dt, ub = pb.Qk, pb.Rk, pb.Qfk, pb.dt, pb.u_bnd
        for nc in (1, 8):
            rng = np.random.default_rng(2)
            U = T(pb.Utrack[:, None, :N - 1] + 0.5 * rng.standard_normal((B, nc, N - 1, m)))
            J, c, d = (torch.empty((B, nc), dtype=torch.float64, device=dev) for _ in range(3))
            Xo = torch.empty((B, nc, N, n), dtype=torch.float64, device=dev)
            Xt = torch.empty((B, nc, N, n), dtype=torch.float64, device=dev)

            def t_scores(X):
                ex, eu = X - Xr, U - Ur
                Jt = 0.5 * dt * (Q * (ex[:, :, :-1] ** 2).sum((2, 3)) + Rw * (eu ** 2).sum((2, 3))) + 0.5 * Qf * (ex[:, :, -1] ** 2).sum(-1)
                ct = torch.clamp(torch.maximum(U - ub, -ub - U), min=0.0).amax((2, 3))
                return Jt, ct

            def t_rollout():
                Xt[:, :, 0] = x0[:, None]
                for k in range(N - 1):
                    Xt[:, :, k + 1] = torch.baddbmm(torch.bmm(Xt[:, :, k], At), U[:, :, k], Bt)
                return t_scores(Xt)

            def t_given():
                Jt, ct = t_scores(Xo)
                pred = torch.matmul(Xo[:, :, :-1], At[:, None]) + torch.matmul(U, Bt[:, None])
                return Jt, ct, (pred - Xo[:, :, 1:]).abs().amax((2, 3))

            api._evaluate_dev(sv, U, None, None, (J, c, d), Xo)
            torch.cuda.synchronize()
            Jt, ct = t_rollout()
            assert torch.allclose(Jt, J, rtol=1e-6, atol=0.0) and torch.allclose(ct, c, rtol=0.0, atol=1e-12) and torch.allclose(Xt, Xo, rtol=1e-6, atol=1e-6)
            calls = {"evaluate_dev rollout + Xout": (lambda: api._evaluate_dev(sv, U, None, None, (J, c, d), Xo), 20, True),
                     "evaluate_dev rollout": (lambda: api._evaluate_dev(sv, U, None, None, (J, c, d), None), 20, True),
                     "evaluate_dev given": (lambda: api._evaluate_dev(sv, U, Xo, None, (J, c, d), None), 20, True),
                     "torch rollout + scores": (t_rollout, 2, False),
                     "torch given scores": (t_given, 4, False)}
            times = {k: [] for k in calls}
            for w in range(WINDOWS + WARM):
                for name, (fn, reps, lib) in calls.items():       # the variants alternate window by window
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    api.synchronize(sv)
                    torch.cuda.synchronize()
                    e0.record()
                    if lib:
                        api.wait_stream(sv)
                    for _ in range(reps):
                        fn()
                    if lib:
                        api.signal_stream(sv)
                    e1.record()
                    torch.cuda.synchronize()
                    if w >= WARM:
                        times[name].append(1e3 * e0.elapsed_time(e1) / reps)
            Rr = B * nc
            tables = B * (n * (n + m) + n) + B * N * (n + m) + 4 * (n + m)          # dynamics, reference window, weights and bounds
            base = (Rr * (N - 1) * m + B * n + tables + 3 * Rr) * 8
            states = Rr * N * n * 8
            nbytes = {"evaluate_dev rollout + Xout": base + states, "evaluate_dev rollout": base, "evaluate_dev given": base + states}
            row = {"n": n, "m": m, "N": N, "ncand": nc, "backend": "one-wave-per-instance" if wide else "16-lane", "calls": {}}
            for name, v in times.items():
                med = statistics.median(v)
                row["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v}
                if name in nbytes:
                    row["calls"][name].update(bytes_moved=nbytes[name], GB_per_s=nbytes[name] / (med * 1e-6) / 1e9)
                print("(%d, %d, %d) ncand %d %-30s median %9.1f us  min %9.1f  max %9.1f" % (n, m, N, nc, name, med, min(v), max(v)), flush=True)
            mu = lambda k: row["calls"][k]["median_us"]
            row["torch_over_library"] = {"rollout": mu("torch rollout + scores") / mu("evaluate_dev rollout"),
                                         "rollout + Xout": mu("torch rollout + scores") / mu("evaluate_dev rollout + Xout"),
                                         "given": mu("torch given scores") / mu("evaluate_dev given")}
            print("   torch / library:", row["torch_over_library"], flush=True)
            res["cases"].append(row)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
        sv.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8192)
