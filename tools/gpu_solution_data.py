"""What one altro_batch_solution_vjp_data_dev call costs, beside altro_batch_solution_vjp_dev on the same handle in
the same process: with every output (the blocks summed over the knots, and per knot) and with gQ, gQf, gR alone (two sweeps, the
active set and the duals never read).
Handles: box-constrained random-linear problems (12, 4, N = 50) at batch 8192 on the 16-lane backend; a quadruped-shaped box-only
problem (12, 12, N = 40) with per-knot dynamics at batch 2048 on the one-wave-per-instance backend after one MPC step (window 1);
nseed 1 and 4.
HIP events on torch's stream around a window of back-to-back calls, each call ordered against torch's stream by its own
wait_stream / signal_stream (the public wrappers), device time per call = window / calls; two warm-up windows, then the median,
minimum and maximum over the windows, the calls alternating window by window.  Beside them the same recursion -- the three sweeps,
the sums and the rank-two blocks -- composed of batched torch operations on the same GPU (matmul / einsum per knot, the triangular
solves as one product with the explicit inverse of Quu, which is cheaper than what the kernel does; the masks of the finite sides
and of the set are made outside the timed window).  Nothing is asserted; the largest difference between the kernel's and the torch
composition's outputs is recorded as a sanity figure.
Usage: gpu_solution_data.py out.json [batch] [per-knot batch]"""
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

    def random_linear(B):
        pb = problems.gen_random_linear_batch(B, n=12, m=4, N=50, steps=1, seed=10)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        prob = sv.prob
        A = np.broadcast_to(prob.model.A, (B, 12, 12))[:, None]      # one block for every knot: expanded on the device
        Bm = np.broadcast_to(prob.model.B, (B, 12, 4))[:, None]
        return sv, None, A, Bm, np.asarray(prob.obj.Xref), np.asarray(prob.obj.Uref)

    def per_knot(B):
        n, m, N = 12, 12, 40
        rng = np.random.default_rng(41)
        nb = N + 3
        A = np.eye(n) + 0.3 * rng.standard_normal((B, nb, n, n)) / np.sqrt(n)
        Bm = 0.5 * rng.standard_normal((B, nb, n, m))
        f = 0.05 * rng.standard_normal((B, nb, n))
        Xt, Ut = rng.standard_normal((B, nb, n)), 0.3 * rng.standard_normal((B, nb - 1, m))
        model = api.LinearModel(A[:, :N - 1], Bm[:, :N - 1], f[:, :N - 1], dt=0.1, per_knot=True)
        obj = api.TrackingObjective(1.0 + 9.0 * rng.random(n), 0.1 + rng.random(m), 39.0 * np.ones(n), Xt[:, :N], Ut[:, :N - 1])
        cons = api.ConstraintList(n, m, N)
        cons.add_constraint(api.BoundConstraint(n, m, u_min=-0.8 * np.ones(m), u_max=0.8 * np.ones(m)), (1, N - 1))
        prob = api.Problem(model, obj, cons, x0=Xt[:, 0].copy(), N=N, U0=Ut[:, :N - 1].copy())
        mp = mpc.TrackMPC(prob, api.SolverOptions(**dict(mpc.REF_OPTS, iterations=60)), Xt, Ut, rng.standard_normal((2, B, n)), (np.full(n, 1e-3),))
        api.set_dynamics_track(mp.solver, A, Bm, f, step_stride=1)
        mp.initial_solve()
        mp.step_async(0)
        mp.synchronize()
        return mp.solver, mp, A[:, 1:N], Bm[:, 1:N], Xt[:, 1:N + 1], Ut[:, 1:N]

    res = {"windows": WINDOWS, "calls_per_window": REPS,
           "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)", "handles": []}
    for label, make, B in (("random-linear (12, 4, 50), 16-lane backend", random_linear, B0),
                           ("box-only per-knot (12, 12, 40), one-wave-per-instance backend, window 1", per_knot, B1)):
        sv, keep, A, Bm, Xr, Ur = make(B)
        n, m, N = sv.n, sv.m, sv.N
        nz = n + m
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        prob = sv.prob
        dt = prob.model.dt
        bc = lambda a, k: np.broadcast_to(np.asarray(a, dtype=np.float64), (B, k))
        wx = np.repeat((dt * bc(prob.obj.Q, n))[:, None], N, axis=1)
        wx[:, -1] = bc(prob.obj.Qf, n)
        wx, wu = T(wx), T(dt * bc(prob.obj.R, m))
        At, Bt = T(A).expand(B, N - 1, n, n), T(Bm).expand(B, N - 1, n, m)
        Xr, Ur = T(np.broadcast_to(Xr, (B, N, n))), T(np.broadcast_to(Ur, (B, N - 1, m)))
        K = api.get_gains_dev(sv)[0].contiguous()
        F = api.get_gain_factors_dev(sv).cpu().numpy()
        Li = np.linalg.inv(np.tril(F, -1) + np.eye(m))
        Qi = T(np.swapaxes(Li, -1, -2) @ (np.einsum("bkaa->bka", F)[..., None] * Li))     # Quu^-1, outside the timed window
        Xh = api.states(sv, out=torch.empty((B, N, n), dtype=torch.float64, device=dev))
        Uh = api.controls(sv, out=torch.empty((B, N - 1, m), dtype=torch.float64, device=dev))
        Zh = torch.zeros((B, N, nz), dtype=torch.float64, device=dev)
        Zh[..., :n], Zh[:, :-1, n:] = Xh, Uh
        ga = api.gain_active_set(sv)
        up, lo_ = (ga["codes"] & 1).to(torch.float64)[:, None], ((ga["codes"] >> 1) & 1).to(torch.float64)[:, None]
        mup, mu = ga["mu_pass"], api.penalty(sv, out=torch.empty((B,), dtype=torch.float64, device=dev))
        ci, (con, first, last) = next((i, it) for i, it in enumerate(prob.constraints.items) if isinstance(it[0], api.BoundConstraint))
        zmin, zmax = (np.broadcast_to(a, (B, nz)) for a in con.zbounds(B))
        hi, lo = np.zeros((B, N, nz)), np.zeros((B, N, nz))
        hi[:, first - 1:last], lo[:, first - 1:last] = np.isfinite(zmax)[:, None], np.isfinite(zmin)[:, None]
        hi[:, N - 1, n:] = lo[:, N - 1, n:] = 0
        lhi, llo = np.zeros((B, N, nz)), np.zeros((B, N, nz))
        du = api.get_duals(sv, ci)
        lhi[:, first - 1:last], llo[:, first - 1:last] = du[:, :, 0], du[:, :, 1]
        hi, lo, lhi, llo = T(hi), T(lo), T(lhi), T(llo)
        zmax0, zmin0 = T(np.where(np.isfinite(zmax), zmax, 0.0))[:, None], T(np.where(np.isfinite(zmin), zmin, 0.0))[:, None]
        row = {"handle": label, "batch": B, "n": n, "m": m, "N": N, "runs": []}
        for ns in (1, 4):
            g = torch.Generator(device="cpu").manual_seed(5)
            rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g).to(dev)
            E = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
            cm = lambda *s: E(*s[:-2], s[-1], s[-2]).transpose(-1, -2)
            gX, gU = rnd(B, ns, N, n), rnd(B, ns, N - 1, m)
            fb = torch.empty((B,), dtype=torch.int32, device=dev)
            vo = dict(gx0=E(B, ns, n), gXref=E(B, ns, N, n), gUref=E(B, ns, N - 1, m), fb=fb)
            w = dict(gQ=E(B, ns, n), gQf=E(B, ns, n), gR=E(B, ns, m), fb=fb)
            sm = dict(w, gzmin=E(B, ns, n + m), gzmax=E(B, ns, n + m), gA=cm(B, ns, n, n), gB=cm(B, ns, n, m), gf=E(B, ns, n))
            pk = dict(w, gzmin=E(B, ns, n + m), gzmax=E(B, ns, n + m), gA=cm(B, ns, N - 1, n, n), gB=cm(B, ns, N - 1, n, m), gf=E(B, ns, N - 1, n))

            def lin():
                s = gX[:, :, N - 1]
                d = [None] * (N - 1)
                for k in range(N - 2, -1, -1):
                    qx = gX[:, :, k] + s @ At[:, k]
                    qu = gU[:, :, k] + s @ Bt[:, k]
                    d[k] = -(qu @ Qi[:, k])
                    s = qx + qu @ K[:, k]
                xi, nu = [torch.zeros_like(s)], []
                for k in range(N - 1):
                    nu.append(xi[k] @ K[:, k].transpose(-1, -2) + d[k])
                    xi.append(xi[k] @ At[:, k].transpose(-1, -2) + nu[k] @ Bt[:, k].transpose(-1, -2))
                return torch.stack(xi, dim=2), torch.stack(nu, dim=2)

            def t_weights():
                xi, nu = lin()
                ex, eu = (Xh - Xr)[:, None], (Uh - Ur)[:, None]
                return xi, nu, ex, dt * (xi[:, :, :-1] * ex[:, :, :-1]).sum(dim=2), xi[:, :, -1] * ex[:, :, -1], dt * (nu * eu).sum(dim=2)

            def t_all(per_knot):
                xi, nu, ex, gQ, gQf, gR = t_weights()
                dz = torch.cat([xi, torch.nn.functional.pad(nu, (0, 0, 0, 1))], dim=-1)
                m3 = mup[:, None, None]
                gzmax, gzmin = -(m3 * (dz * up).sum(dim=2)), -(m3 * (dz * lo_).sum(dim=2))
                chi, clo = Zh - zmax0, zmin0 - Zh
                mm = mu[:, None, None]
                ghi = hi * (lhi + torch.where((chi >= 0) | (lhi > 0), mm * chi, torch.zeros_like(chi)))
                glo = lo * (llo + torch.where((clo >= 0) | (llo > 0), mm * clo, torch.zeros_like(clo)))
                l = wx * ex[:, 0] + (ghi - glo)[..., :n]
                hx = wx + m3 * (up[:, 0, :, :n] + lo_[:, 0, :, :n])
                dl = gX + hx[:, None] * xi
                lam, dlam = [None] * N, [None] * N
                lam[N - 1], dlam[N - 1] = l[:, N - 1], dl[:, :, N - 1]
                for k in range(N - 2, -1, -1):
                    lam[k] = l[:, k] + (lam[k + 1][:, None] @ At[:, k])[:, 0]
                    dlam[k] = dl[:, :, k] + dlam[k + 1] @ At[:, k]
                lam1, dlam1 = torch.stack(lam[1:], dim=1), torch.stack(dlam[1:], dim=2)
                if per_knot:
                    gA = torch.einsum("bki,bskj->bskij", lam1, xi[:, :, :-1]) + torch.einsum("bski,bkj->bskij", dlam1, Xh[:, :-1])
                    gB = torch.einsum("bki,bskj->bskij", lam1, nu) + torch.einsum("bski,bkj->bskij", dlam1, Uh)
                    gf = dlam1
                else:
                    gA = torch.einsum("bki,bskj->bsij", lam1, xi[:, :, :-1]) + torch.einsum("bski,bkj->bsij", dlam1, Xh[:, :-1])
                    gB = torch.einsum("bki,bskj->bsij", lam1, nu) + torch.einsum("bski,bkj->bsij", dlam1, Uh)
                    gf = dlam1.sum(dim=2)
                return dict(gQ=gQ, gQf=gQf, gR=gR, gzmin=gzmin, gzmax=gzmax, gA=gA, gB=gB, gf=gf)

            calls = {"solution_vjp_dev": lambda: api.solution_vjp(sv, gX, gU, out=vo),
                     "vjp_data_dev gQ gQf gR": lambda: api.solution_vjp_data(sv, gX, gU, out=w),
                     "vjp_data_dev all, summed": lambda: api.solution_vjp_data(sv, gX, gU, out=sm),
                     "vjp_data_dev all, per knot": lambda: api.solution_vjp_data(sv, gX, gU, per_knot=True, out=pk),
                     "torch gQ gQf gR": t_weights, "torch all, summed": lambda: t_all(False), "torch all, per knot": lambda: t_all(True)}
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
            ok = fb != 0
            diff = max(float((kn[k][ok] - tv[k][ok]).abs().max() / tv[k][ok].abs().max().clamp_min(1e-300))
                       for kn, tv in ((sm, t_all(False)), (pk, t_all(True))) for k in tv)
            run = {"nseed": ns, "valid_instances": int(ok.sum()), "largest_relative_difference_kernel_vs_torch": diff, "calls": {}}
            for name, v in times.items():
                med = statistics.median(v)
                run["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v}
                print("%-28s nseed %d %-28s median %11.1f us  min %11.1f  max %11.1f" % (label[:28], ns, name, med, min(v), max(v)), flush=True)
            for a, b in (("gQ gQf gR", "gQ gQf gR"), ("all, summed", "all, summed"), ("all, per knot", "all, per knot")):
                run["torch_over_kernel " + a] = run["calls"]["torch " + b]["median_us"] / run["calls"]["vjp_data_dev " + a]["median_us"]
            print("   torch / kernel:", {k: round(v, 1) for k, v in run.items() if k.startswith("torch_over")}, "kernel vs torch %.2e" % diff, flush=True)
            row["runs"].append(run)
        res["handles"].append(row)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        sv.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8192, int(sys.argv[3]) if len(sys.argv) > 3 else 2048)
