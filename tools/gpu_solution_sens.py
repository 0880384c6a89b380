"""What one altro_batch_solution_vjp_dev / altro_batch_solution_jvp_dev call costs, beside the same recursion
composed of batched torch operations on the same GPU (bmm / einsum per knot, the triangular solves as two bmm with the explicit
inverse of Quu, which is cheaper than what the kernel does): the only yardstick there is, no earlier commit has the call.
Handles: box-constrained random-linear problems (12, 4, N = 50) at batch 8192 on the 16-lane backend, nseed 1 and 4; the
quadruped MPC loop (12, 12, N = 40) at batch 2048 on the one-wave-per-instance backend after one step (window 1, per-knot
dynamics), nseed 1 and 4.
HIP events on torch's stream around a window of back-to-back calls, each call ordered against torch's stream by its own
wait_stream / signal_stream (the public wrappers), device time per call = window / calls; two warm-up windows, then the median,
minimum and maximum over the windows, the calls alternating window by window.  Nothing is asserted; the largest difference
between the kernel's and the torch composition's outputs is recorded as a sanity figure.
Usage: gpu_solution_sens.py out.json [batch] [quadruped batch]"""
import json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
WINDOWS, WARM, REPS = 10, 2, 5


def main(path, B0, B1):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)

    def random_linear(B):
        n, m, N = 12, 4, 50
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=10)
        prob = mpc.gen_tracking_problem(pb)
        sv = api.ALTROSolver(prob, api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        A = np.broadcast_to(prob.model.A, (B, n, n))[:, None]      # one block for every knot: expanded on the device
        Bm = np.broadcast_to(prob.model.B, (B, n, m))[:, None]
        return sv, None, A, Bm, prob

    def quadruped(B):
        N, S = 40, 1
        qp = problems.gen_quadruped_problem(N=N)
        rng = np.random.default_rng(17)
        t0 = rng.uniform(0.0, 0.8, B)
        x0 = qp.x_des + rng.standard_normal((B, 12)) * np.array([.02, .02, .02, .05, .05, .05, .3, .3, .1, .3, .3, .3])
        Tn = 1 + S + N
        A, Bm, d = np.zeros((B, Tn, 12, 12)), np.zeros((B, Tn, 12, 12)), np.zeros((B, Tn, 12))
        cache = {}
        for b in range(B):
            for t in range(Tn):
                c = tuple(problems.trot_contacts(t0[b] + t * qp.dt))
                if c not in cache:
                    cache[c] = problems.quadruped_linearize(qp.x_des, np.zeros(12), qp.feet, np.array(c), qp.inertia, qp.mass, qp.dt)
                A[b, t], Bm[b, t], d[b, t] = cache[c]
        Nt = Tn + 1
        prob = mpc.quadruped_problem(qp, x0, A[:, :N - 1], Bm[:, :N - 1], d[:, :N - 1])
        mp = mpc.TrackMPC(prob, api.SolverOptions(**problems.QUADRUPED_OPTS), np.tile(qp.x_des, (B, Nt, 1)), np.zeros((B, Nt - 1, 12)),
                          rng.standard_normal((1 + S, B, 12)), (np.full(12, 1e-3),))
        api.set_dynamics_track(mp.solver, A, Bm, d, step_stride=1)
        api.initial_controls(mp.solver, np.tile(qp.u_hover, (B, N - 1, 1)))
        mp.initial_solve()
        mp.step(0)
        return mp.solver, mp, A[:, 1:N], Bm[:, 1:N], prob

    res = {"windows": WINDOWS, "calls_per_window": REPS,
           "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)", "handles": []}
    for label, make, B in (("random-linear (12, 4, 50), 16-lane backend", random_linear, B0),
                           ("quadruped (12, 12, 40), one-wave-per-instance backend, window 1", quadruped, B1)):
        sv, keep, A, Bm, prob = make(B)
        n, m, N = sv.n, sv.m, sv.N
        dt = prob.model.dt
        bc = lambda a, k: np.broadcast_to(np.asarray(a, dtype=np.float64), (B, k))
        wx = np.repeat((dt * bc(prob.obj.Q, n))[:, None], N, axis=1)
        wx[:, -1] = bc(prob.obj.Qf, n)
        wx, wu = T(wx), T(dt * bc(prob.obj.R, m))
        At, Bt = T(A).expand(B, N - 1, n, n), T(Bm).expand(B, N - 1, n, m)
        K, _ = api.get_gains_dev(sv)
        K = K.contiguous()
        F = api.get_gain_factors_dev(sv).cpu().numpy()
        # Quu^-1 = L^-T D^-1 L^-1 once, on the host, outside the timed window (the torch side gets it for nothing)
        Li = np.linalg.inv(np.tril(F, -1) + np.eye(m))
        Qi = T(np.swapaxes(Li, -1, -2) @ (np.einsum("bkaa->bka", F)[..., None] * Li))
        row = {"handle": label, "batch": B, "n": n, "m": m, "N": N, "runs": []}
        for ns in (1, 4):
            g = torch.Generator(device="cpu").manual_seed(5)
            rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g).to(dev)
            gX, gU, vx0, vX, vU = rnd(B, ns, N, n), rnd(B, ns, N - 1, m), rnd(B, ns, n), rnd(B, ns, N, n), rnd(B, ns, N - 1, m)
            vo = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in (("gx0", (B, ns, n)), ("gXref", (B, ns, N, n)), ("gUref", (B, ns, N - 1, m)))}
            jo = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in (("dX", (B, ns, N, n)), ("dU", (B, ns, N - 1, m)))}
            vo["fb"] = jo["fb"] = torch.empty((B,), dtype=torch.int32, device=dev)

            def lin(gx, gu, xi0):
                s = gx[:, :, N - 1]
                d = [None] * (N - 1)
                for k in range(N - 2, -1, -1):
                    qx = gx[:, :, k] + s @ At[:, k]
                    qu = gu[:, :, k] + s @ Bt[:, k]
                    d[k] = -(qu @ Qi[:, k])
                    s = qx + qu @ K[:, k]
                xi, nu = [xi0], []
                for k in range(N - 1):
                    nu.append(xi[k] @ K[:, k].transpose(-1, -2) + d[k])
                    xi.append(xi[k] @ At[:, k].transpose(-1, -2) + nu[k] @ Bt[:, k].transpose(-1, -2))
                return s, torch.stack(xi, dim=2), torch.stack(nu, dim=2)

            def t_vjp():
                s0, xi, nu = lin(gX, gU, torch.zeros_like(vx0))
                return s0, -(wx[:, None] * xi), -(wu[:, None, None] * nu)

            def t_jvp():
                _, xi, nu = lin(-(wx[:, None] * vX), -(wu[:, None, None] * vU), vx0)
                return xi, nu

            calls = {"solution_vjp_dev": lambda: api.solution_vjp(sv, gX, gU, out=vo), "torch vjp": t_vjp,
                     "solution_jvp_dev": lambda: api.solution_jvp(sv, vx0, vX, vU, out=jo), "torch jvp": t_jvp}
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
            tv, tj = t_vjp(), t_jvp()
            ok = (vo["fb"] != 0)
            diff = max(float((a[ok] - b[ok]).abs().max() / b[ok].abs().max()) for a, b in
                       ((vo["gx0"], tv[0]), (vo["gXref"], tv[1]), (vo["gUref"], tv[2]), (jo["dX"], tj[0]), (jo["dU"], tj[1])))
            run = {"nseed": ns, "valid_instances": int(ok.sum()), "largest_relative_difference_kernel_vs_torch": diff, "calls": {}}
            for name, v in times.items():
                med = statistics.median(v)
                run["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v}
                print("%-28s nseed %d %-18s median %11.1f us  min %11.1f  max %11.1f" % (label[:28], ns, name, med, min(v), max(v)), flush=True)
            for op in ("vjp", "jvp"):
                run["torch_over_kernel_" + op] = run["calls"]["torch " + op]["median_us"] / run["calls"]["solution_%s_dev" % op]["median_us"]
            print("   torch / kernel: vjp %.1f  jvp %.1f   valid %d of %d   kernel vs torch %.2e" % (
                run["torch_over_kernel_vjp"], run["torch_over_kernel_jvp"], run["valid_instances"], B, diff), flush=True)
            row["runs"].append(run)
            with open(path, "w") as f:
                json.dump(dict(res, handles=res["handles"] + [row]), f, indent=1)
        res["handles"].append(row)
        sv.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8192, int(sys.argv[3]) if len(sys.argv) > 3 else 2048)
