"""What one altro_batch_warm_start_dev call costs, beside the composition a caller writes without it, on the
same tensors in the same run: altro_batch_evaluate_dev with Xout, then torch for the merit, the argmin and the gather of the
winner's states and controls, then altro_batch_set_initial_trajectory_dev.
HIP events on torch's stream around a window of back-to-back calls, each call ordered against torch's stream by its own
wait_stream / signal_stream (the public wrappers), device time per call = window / calls; two warm-up windows, then the median,
minimum and maximum over 20 windows, the variants alternating window by window.  The 16-lane backend at (12, 4, N = 50) and the
one-wave-per-instance backend at (32, 16, N = 21), batch 8192, box-constrained random-linear problems, ncand 1 and 8, without
the incumbent (the composition has none) and, for the fused call only, with it.
bytes_moved: what a call cannot avoid -- U, x0, the reference window, the dynamics, cost and bounds tables, J, c_max, chosen, the
winner's plane; state_bytes: the candidate states the composition moves on top (written by the rollout, read by the scoring
kernel, the winner's read by the gather and written and read again on its way into the plane) -- the fused call moves none.
Closed loop: mean iLQR iterations per solve over 20 ExternalMPC ticks of the headline workload (12, 4, N = 50) without
candidates and with the candidates {reference controls, zero controls} and the incumbent.
Usage: gpu_warm_start.py out.json [batch]"""
import json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
WINDOWS, WARM, REPS, RHO = 20, 2, 10, 1e3


def main(path, B):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    res = {"batch": B, "windows": WINDOWS, "calls_per_window": REPS, "rho": RHO,
           "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)", "cases": []}
    for n, m, N in ((12, 4, 50), (32, 16, 21)):
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        wide = (n, m) != (12, 4)
        ar = torch.arange(B, device=dev)
        for nc in (1, 8):
            rng = np.random.default_rng(2)
            U = T(pb.Utrack[:, None, :N - 1] + 0.5 * rng.standard_normal((B, nc, N - 1, m)))
            J, c = (torch.empty((B, nc), dtype=torch.float64, device=dev) for _ in range(2))
            J1, c1 = (torch.empty((B, nc + 1), dtype=torch.float64, device=dev) for _ in range(2))
            ch = torch.empty((B,), dtype=torch.int32, device=dev)
            Xo = torch.empty((B, nc, N, n), dtype=torch.float64, device=dev)
            Xg, Ug = torch.empty((B, N, n), dtype=torch.float64, device=dev), torch.empty((B, N - 1, m), dtype=torch.float64, device=dev)

            def fused():
                api.warm_start(sv, U, rho=RHO, include_current=False, out=(ch, J, c))

            def fused_inc():
                api.warm_start(sv, U, rho=RHO, include_current=True, out=(ch, J1, c1))

            def composition():
                api.evaluate(sv, U, out=(J, c, None), Xout=Xo)
                w = torch.argmin(J + RHO * c, dim=1)
                Xw, Uw = Xo[ar, w].contiguous(), U[ar, w].contiguous()
                with api._bracket(sv):
                    api._initial_trajectory_dev(sv, Xw, Uw)
                return w

            # the two give the same plane (the choice is decidable on these inputs: no ties, nothing infinite)
            w = composition()
            api.states(sv, out=Xg), api.controls(sv, out=Ug)
            torch.cuda.synchronize()
            Xc, Uc = Xg.clone(), Ug.clone()
            fused()
            api.states(sv, out=Xg), api.controls(sv, out=Ug)
            torch.cuda.synchronize()
            agree = bool(torch.equal(ch.long(), w) and torch.equal(Xg, Xc) and torch.equal(Ug, Uc))
            print("(%d, %d, %d) ncand %d: fused call and composition leave the same plane: %s" % (n, m, N, nc, agree), flush=True)
            calls = {"warm_start_dev": fused, "warm_start_dev + incumbent": fused_inc, "composition": composition}
            times = {k: [] for k in calls}
            for wdw in range(WINDOWS + WARM):
                for name, fn in calls.items():       # the variants alternate window by window
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
            Rr = B * nc
            tables = B * (n * (n + m) + n) + B * N * (n + m) + 4 * (n + m)          # dynamics, reference window, weights and bounds
            pl = B * (N * (16 if not wide else n) + (0 if not wide else (N - 1) * m))   # the plane written
            base = (Rr * (N - 1) * m + B * n + tables + 2 * Rr + B * (N - 1) * m + pl) * 8 + B * 4
            states = (2 * Rr * N * n + 3 * B * N * n) * 8
            row = {"n": n, "m": m, "N": N, "ncand": nc, "backend": "one-wave-per-instance" if wide else "16-lane", "same_plane_as_composition": agree,
                   "calls": {}}
            for name, v in times.items():
                med = statistics.median(v)
                row["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v, "bytes_moved": base,
                                      "state_bytes": states if name == "composition" else 0}
                print("(%d, %d, %d) ncand %d %-28s median %9.1f us  min %9.1f  max %9.1f" % (n, m, N, nc, name, med, min(v), max(v)), flush=True)
            co, fu = row["calls"]["composition"], row["calls"]["warm_start_dev"]
            row["saving_us"] = co["median_us"] - fu["median_us"]
            row["composition_spread_us"] = co["max_us"] - co["min_us"]
            row["saving_exceeds_spread"] = bool(row["saving_us"] > row["composition_spread_us"])
            print("   composition - fused: %.1f us; composition max - min: %.1f us" % (row["saving_us"], row["composition_spread_us"]), flush=True)
            res["cases"].append(row)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
        sv.close()
    res["closed_loop"] = closed_loop(min(B, 8192))
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def closed_loop(B, ticks=20, n=12, m=4, N=50):
    """mean iLQR iterations per solve over `ticks` ExternalMPC ticks, the plant x+ = A x + B u0 + noise on the device"""
    import numpy as np
    import torch
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=ticks, seed=1)
    A, Bm, noise, Xt, Ut = T(pb.A), T(pb.Bm), T(pb.noise), T(pb.Xtrack), T(pb.Utrack)
    out = {"batch": B, "ticks": ticks, "n": n, "m": m, "N": N, "candidates": ["reference controls", "zero controls"], "rho": RHO}
    for name, use in (("no candidates", False), ("candidates + incumbent", True)):
        sv = altro.ALTROSolver(mpc.gen_tracking_problem(pb), altro.SolverOptions(**mpc.REF_OPTS))
        altro.solve(sv)
        loop = altro.ExternalMPC(sv)
        x, u0 = T(pb.Xtrack[:, 0]), altro.first_knot(sv)[0]
        its = torch.zeros((), dtype=torch.float64, device=dev)
        ok = torch.zeros((), dtype=torch.float64, device=dev)
        for i in range(ticks):
            xn = torch.bmm(A, x.unsqueeze(-1)).squeeze(-1) + torch.bmm(Bm, u0.unsqueeze(-1)).squeeze(-1)
            x = xn + noise[i] * (0.01 * xn.abs().amax(dim=1, keepdim=True))
            Xr, Ur = Xt[:, i + 1:i + 1 + N].contiguous(), Ut[:, i + 1:i + N].contiguous()
            cand = torch.stack([Ur, torch.zeros_like(Ur)], dim=1).contiguous() if use else None
            u0, _, st, it = loop.tick(x, Xr, Ur, candidates=cand, candidate_rho=RHO)
            its += it.double().mean()
            ok += (st == altro.SOLVE_SUCCEEDED).double().mean()
        torch.cuda.synchronize()
        out[name] = {"mean_iterations_per_solve": float(its) / ticks, "solve_succeeded_frac": float(ok) / ticks}
        print("closed loop, %-24s mean iterations per solve %.4f, succeeded %.4f" % (name, float(its) / ticks, float(ok) / ticks), flush=True)
        sv.close()
    return out


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8192)
