"""Do two builds of the library polish to the same bytes?  For each of the two libraries -- the parent's first,
then this build's -- one fresh child process (ALTRO_HIP_LIB selects the library, as in the other A/B tools) runs, with
projected_newton = 1,
  the box-constrained LQ batch of the oracle parity test at (12, 4), the same forced onto the one-wave-per-instance backend,
  and the batch of the wide-backend test at (20, 4);
  the grasp problem at N = 31 on both backends; the quadruped tick at N = 10;
  the six-step MPC loop at (12, 4) and (20, 4), plain, with three of its steps under an active mask, and under an episode clock
and records SHA-256 of the raw bytes of states, controls, cost, c_max, status, iterations, the three polish statistics, the
three outputs of the multiplier projection and get_duals of constraint 0.
The parent's child ends before the other starts; each has its own time limit; a child that ends abnormally ends the tool and
nothing more is started.  The result is the table of digests and whether every one is equal; exit status 1 when one differs.
Usage: gpu_pn_bytes_ab.py out.json <parent libaltro_hip.so>"""
import hashlib, json, os, subprocess, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "tests")):
    sys.path.insert(0, p)
CHILD_LIMIT_S = 240


def child(path):
    import numpy as np
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import mpc, problems as P
    from helpers import REF_OPTS, quadruped_gpu_problem, rocket_gpu_problem
    out = {}
    nran = {}

    def rec(case, sv):
        st = altro.stats(sv)
        ran, failed, res = altro.polish_stats(sv)
        d0, d1, dfail = altro.polish_dual_residuals(sv)
        arrays = dict(states=altro.states(sv), controls=altro.controls(sv), cost=st.cost, c_max=st.c_max, status=st.status,
                      iterations=st.iterations, polish_ran=ran, polish_failed=failed, polish_residual=res, dual_before=d0,
                      dual_after=d1, dual_failed=dfail, duals=altro.get_duals(sv, 0))
        for k, a in arrays.items():
            out["%s | %s" % (case, k)] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
        nran[case] = int(ran.sum())

    def solved(case, prob, opts, wide=False):
        if wide:
            os.environ["ALTRO_FORCE_WIDE"] = "1"
        sv = altro.ALTROSolver(prob, altro.SolverOptions(**opts))
        os.environ.pop("ALTRO_FORCE_WIDE", None)
        assert not wide or altro.wave_cycles(sv).size == 0, case
        altro.solve(sv)
        rec(case, sv)
        sv.close()

    pn = dict(REF_OPTS, constraint_tolerance=1e-8, projected_newton=1)
    # the LQ batches of test_projected_newton_polish_matches_oracle and of the wide-backend test, case (a)
    pb = P.gen_random_linear_batch(5, steps=1, seed=81)
    prob = mpc.gen_tracking_problem(pb)
    prob.x0 = prob.x0 + np.array([25.0, 25.0, 0.1, 12.0, 25.0])[:, None] + np.random.default_rng(3).standard_normal(prob.x0.shape)
    solved("LQ (12, 4)", prob, pn)
    solved("LQ (12, 4) forced wide", prob, pn, wide=True)
    pb = P.gen_random_linear_batch(4, n=20, m=4, N=21, steps=1, seed=85)
    prob = mpc.gen_tracking_problem(pb)
    prob.x0 = prob.x0 + np.array([20.0, 15.0, 0.1, 25.0])[:, None]
    solved("LQ (20, 4)", prob, pn)
    # the grasp problem: AL stage to a loose 1e-2, polish to 1e-6
    gp = P.gen_grasp_problem(N=31, tf=3.0)
    gopts = dict(cost_tolerance_intermediate=1e-5, penalty_initial=1.0, penalty_scaling=10.0, constraint_tolerance=1e-6,
                 projected_newton=1, projected_newton_tolerance=1e-2)
    x0 = np.tile(gp.x0, (3, 1))
    x0[1:, 1:3] += 0.1 * np.random.default_rng(3).standard_normal((2, 2))
    solved("grasp N = 31", rocket_gpu_problem(altro, gp, x0), gopts)
    solved("grasp N = 31 forced wide", rocket_gpu_problem(altro, gp, x0), gopts, wide=True)
    # one quadruped tick: per-knot dynamics, linearised friction pyramids, f_z box
    N = 10
    qb = P.gen_quadruped_batch(3, N=N, steps=1, seed=19)
    qopts = dict(P.QUADRUPED_OPTS, constraint_tolerance=1e-7, projected_newton=1, projected_newton_tolerance=1e-2)
    solved("quadruped tick N = 10", quadruped_gpu_problem(altro, qb.qp, qb.x0, qb.A[:, :N - 1], qb.Bm[:, :N - 1], qb.d[:, :N - 1]), qopts)
    # the MPC loop of test_projected_newton_polish_inside_the_mpc_loop, six steps in one fused launch
    B, S = 5, 6
    for n, m in ((12, 4), (20, 4)):
        pb = P.gen_random_linear_batch(B, n=n, m=m, N=21, steps=S, seed=87)
        pb.u_bnd = 1.0     # the track was generated with |u| <= 3: controls saturate in every solve
        for kind in ("plain", "mask", "clock"):
            mp = mpc.BatchMPC(pb, altro.SolverOptions(**pn))
            mp.initial_solve()
            if kind == "clock":     # instances out of step with each other; one ends early, one never starts
                mp.set_clock(np.array([0, 2, 0, 3, 1]), np.array([6, 3, 6, 1, 0]))
            mp.run_async(3, first=0)
            if kind == "mask":
                mp.set_active(np.array([1, 0, 1, 1, 0], dtype=np.int32))
            mp.run_async(3, first=3)
            mp.synchronize()
            rec("MPC loop (%d, %d) %s" % (n, m, kind), mp.solver)
            mp.solver.close()
    with open(path, "w") as f:
        json.dump({"digests": out, "polished": nran}, f, indent=1)


def main(path, parent):
    parent = os.path.abspath(parent)
    got = {}
    for name, lib in (("parent", parent), ("this", None)):
        e = dict(os.environ)
        e.pop("ALTRO_HIP_LIB", None)
        if lib:
            e["ALTRO_HIP_LIB"] = lib
        tmp = path + "." + name
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=e, timeout=CHILD_LIMIT_S)
        if p.returncode != 0:
            sys.exit("the child of the %s build ended with status %d: nothing more is started" % (name, p.returncode))
        with open(tmp) as f:
            got[name] = json.load(f)
        os.remove(tmp)
    a, b = got["parent"]["digests"], got["this"]["digests"]
    keys = sorted(a)
    differ = [k for k in keys if a[k] != b.get(k)] + sorted(set(b) - set(keys))
    res = {"what": "SHA-256 of the raw bytes of each output, the parent's library against this build's", "outputs": len(keys),
           "all_equal": not differ, "differ": differ, "instances_polished_in_the_last_solve": got["parent"]["polished"],
           "digests": {k: {"parent": a[k], "this": b.get(k)} for k in keys}}
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("%d outputs, %d differ%s" % (len(keys), len(differ), "".join("\n  " + k for k in differ)))
    print("polished in the last solve:", got["parent"]["polished"])
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main(sys.argv[1], sys.argv[2])
