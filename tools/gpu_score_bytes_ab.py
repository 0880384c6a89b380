"""Do two builds of the library score, differentiate, warm-start, simulate, evaluate the policy and differentiate the solution to
the same bytes?
For each of the two libraries -- the parent's first, then this build's -- one fresh child process (ALTRO_HIP_LIB selects the
library, as in the other A/B tools) builds the seven cases of tests/evaluate_ref.py plus (12, 4) forced onto the
one-wave-per-instance backend, solves each once and records SHA-256 of the raw bytes of
  evaluate_dev          given form: J, c_max, defect; rollout form: J, c_max, defect, Xout
  evaluate_grad_dev     rho 0 and 10, the candidates of evaluate_grad_ref.candidates_with_polar (on the cone case all three
                        branches of the cone): J, P, gU, gx0, Xout
  warm_start_dev        six candidates + incumbent, rho 0 and 1e3: chosen, J, c_max, the installed states and controls
  simulate_policy_dev   nsamp 3, with and without w, clamp 0 and 1: J, c_max, dx_max, fb, Xout, Uout
  eval_policy_dev       at every knot: u, fb
  propagate_covariance_dev   W = 0.01 I: sx, su, dJ, fb and, where the case has a box, zmin_t, zmax_t at kappa = 1
  solution_vjp / _jvp   nseed 3, the seeds of tests/test_solution_sens_gpu.py: all outputs and fb, gx0 alone; vx0 alone, all inputs
  get_gain_factors_dev, gain_active_set, solution_vjp_data summed, per knot, the weights alone and with gU = None
                        (7w; where the library refuses a call -- cone rows, m > 16, the unsolved case -- its status code)
The parent's child ends before the other starts; each has its own time limit; a child that ends abnormally ends the tool and
nothing more is started.  The result is the table of digests and whether every one is equal; exit status 1 when one differs.
Usage: gpu_score_bytes_ab.py out.json <parent libaltro_hip.so>"""
import hashlib, json, os, subprocess, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "tests")):
    sys.path.insert(0, p)
CHILD_LIMIT_S = 300
S = 3


def child(path):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc
    import evaluate_ref as ER
    import evaluate_grad_ref as GR
    import simulate_ref as SR
    import test_solution_sens_gpu as SS
    import warm_start_ref as WR
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    E = lambda *shape, dtype=torch.float64: torch.full(shape, -12345.5 if dtype == torch.float64 else -77, dtype=dtype, device=dev)
    out = {}

    def rec(case, call, **arrays):
        torch.cuda.synchronize()
        for k, t in arrays.items():
            out["%s | %s | %s" % (case, call, k)] = hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()

    for name, fw in [(k, False) for k in WR.CASES] + [("16-box(12,4)", True)]:
        make, kw = WR.CASES[name]
        cs = make()
        B, N, n, m = cs.B, cs.N, cs.n, cs.m
        case = name + (" forced wide" if fw else "")
        if fw:
            os.environ["ALTRO_FORCE_WIDE"] = "1"
        sv = altro.ALTROSolver(ER.to_problem(altro, cs, **kw), altro.SolverOptions(**dict(mpc.REF_OPTS, iterations=60)))
        os.environ.pop("ALTRO_FORCE_WIDE", None)
        if name != "wide-limits(64,32)":      # (the solve kernel refuses that size: its gains stay invalid, its loop is open)
            altro.solve(sv)
        Xbar, Ubar = altro.states(sv), altro.controls(sv)
        # evaluate_dev, both forms
        U3 = T(ER.candidates(cs, 5))
        J, c, d, Xo = E(B, 3), E(B, 3), E(B, 3), E(B, 3, N, n)
        altro.evaluate(sv, U3, out=(J, c, d), Xout=Xo)
        rec(case, "evaluate rollout", J=J, c_max=c, defect=d, Xout=Xo)
        J, c, d = E(B, 3), E(B, 3), E(B, 3)
        altro.evaluate(sv, U3, X=Xo, out=(J, c, d))
        rec(case, "evaluate given", J=J, c_max=c, defect=d)
        # evaluate_grad_dev, without and with the pullback of the rows
        Ug = T(GR.candidates_with_polar(cs, 5))
        nc = Ug.shape[1]
        for rho in (0.0, 10.0):
            J, P, gU, g0, Xo = E(B, nc), E(B, nc), E(B, nc, N - 1, m), E(B, nc, n), E(B, nc, N, n)
            altro.evaluate_grad(sv, Ug, rho=rho, out=(J, P, gU, g0), Xout=Xo)
            rec(case, "evaluate_grad rho %g" % rho, J=J, P=P, gU=gU, gx0=g0, Xout=Xo)
        # simulate_policy_dev
        x0 = SR.disturbed_starts(Xbar[:, 0], S, 71)
        x0[:, -1] = SR.disturbed_starts(Xbar[:, 0], 1, 72, rel=3.0)[:, 0]
        w = SR.disturbances(Xbar, S, 73)
        for clamp in (0, 1):
            for wname, wt in (("w", T(w)), ("no w", None)):
                J, c, dx, fb = E(B, S), E(B, S), E(B, S), E(B, dtype=torch.int32)
                Xs, Us = E(B, S, N, n), E(B, S, N - 1, m)
                altro.simulate_policy(sv, T(x0), wt, None, clamp, (J, c, dx), fb, Xs, Us)
                rec(case, "simulate %s clamp %d" % (wname, clamp), J=J, c_max=c, dx_max=dx, fb=fb, Xout=Xs, Uout=Us)
        # eval_policy_dev at every knot, from the far sample's start
        for k in range(N - 1):
            u, fb = E(B, m), E(B, dtype=torch.int32)
            altro.eval_policy(sv, T(Xbar[:, k] + (x0[:, -1] - Xbar[:, 0])), knot=torch.full((B,), k, dtype=torch.int32, device=dev), clamp=True, out=u, fb=fb)
            rec(case, "eval_policy knot %d" % k, u=u, fb=fb)
        # propagate_covariance_dev: W = 0.01 I, Sigma0 = 0; the box tightened by one deviation where the case has a box
        Wc = T(0.01 * np.eye(n))
        cov = altro.propagate_covariance(sv, None, Wc, None, 1.0 if any(c.kind == "box" for c in cs.cons) else None)
        rec(case, "propagate_covariance", **cov)
        # the sensitivity of the solution, nseed 3; a call the library refuses records its status code
        def sens(call, fn):
            try:
                got = fn()
            except altro.AltroError as e:
                out["%s | %s | status" % (case, call)] = "status %d" % e.code
                return
            rec(case, call, **(got if isinstance(got, dict) else dict(F=got)))

        sd = SS.seeds(cs, 81, ns=S)
        gX, gU, v0, vX, vU = (T(a) for a in (sd.gX, sd.gU, sd.vx0, sd.vXref, sd.vUref))
        sens("solution_vjp", lambda: altro.solution_vjp(sv, gX, gU))
        sens("solution_vjp gx0 alone", lambda: altro.solution_vjp(sv, gX, gU, out=("gx0",)))
        sens("solution_jvp vx0 alone", lambda: altro.solution_jvp(sv, vx0=v0))
        sens("solution_jvp", lambda: altro.solution_jvp(sv, v0, vX, vU))
        sens("get_gain_factors_dev", lambda: api.get_gain_factors_dev(sv))
        sens("gain_active_set", lambda: altro.gain_active_set(sv))
        sens("solution_vjp_data summed", lambda: altro.solution_vjp_data(sv, gX, gU))
        sens("solution_vjp_data per knot", lambda: altro.solution_vjp_data(sv, gX, gU, per_knot=True))
        sens("solution_vjp_data weights alone", lambda: altro.solution_vjp_data(sv, gX, gU, out=("gQ", "gQf", "gR")))
        sens("solution_vjp_data gU = None", lambda: altro.solution_vjp_data(sv, gX, None))
        # warm_start_dev (last: it rewrites the plane)
        U6 = T(WR.six_candidates(cs, Ubar))
        for rho in (0.0, 1e3):
            ch, J, c = E(B, dtype=torch.int32), E(B, 7), E(B, 7)
            altro.warm_start(sv, U6, rho=rho, include_current=True, out=(ch, J, c))
            rec(case, "warm_start rho %g" % rho, chosen=ch, J=J, c_max=c, states=altro.states(sv, out=E(B, N, n)), controls=altro.controls(sv, out=E(B, N - 1, m)))
        sv.close()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


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
    keys = sorted(got["parent"])
    differ = [k for k in keys if got["parent"][k] != got["this"].get(k)] + sorted(set(got["this"]) - set(keys))
    res = {"what": "SHA-256 of the raw bytes of each output, the parent's library against this build's", "outputs": len(keys),
           "all_equal": not differ, "differ": differ, "digests": {k: {"parent": got["parent"][k], "this": got["this"].get(k)} for k in keys}}
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("%d outputs, %d differ%s" % (len(keys), len(differ), "".join("\n  " + k for k in differ)))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main(sys.argv[1], sys.argv[2])
