"""What one altro_batch_evaluate_grad_dev launch costs, beside altro_batch_evaluate_dev on the same shapes timed
ON THE PARENT COMMIT'S LIBRARY as the yardstick: the rollout form without Xout, which rolls out, stores and re-reads the states
and evaluates every row once -- the work the gradient call does forwards.
Two fresh child processes, the parent's library first (ALTRO_HIP_LIB selects the library, as in the other A/B tools), then this
build's; each has its own time limit, and a child that ends abnormally ends the tool and nothing more is started.
HIP events on torch's stream around a window of back-to-back calls on the solver's stream between wait_stream and
signal_stream, device time per call = window / calls; two warm-up windows, then the median, minimum and maximum over 20
windows.  The 16-lane backend at (12, 4, N = 50) and the one-wave-per-instance backend at (32, 16, N = 21), batch 8192,
ncand 1 and 8; and, because those two are box-only problems, the two small problems of tests/evaluate_ref.py that have LINEAR
and SOC rows -- 16-soc(6,3) and wide-cone(7,3), N = 9, the candidates of evaluate_grad_ref.candidates_with_polar -- at the same
batch, where rho = 10 runs the row pullback and rho = 0 does not.  Each child times evaluate_dev and, where its
library has it, evaluate_grad_dev with all four outputs at rho = 10 and at rho = 0.
bytes_moved: what the call cannot avoid -- U, x0, the reference window, the weights and bounds, the outputs, the dynamics
tables TWICE (forwards and transposed), and the states written once and read once.
Usage: gpu_evaluate_grad.py out.json <parent libaltro_hip.so> [batch]"""
import json, os, statistics, subprocess, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (R, os.path.join(R, "tests")):
    sys.path.insert(0, p_)
WINDOWS, WARM, CHILD_LIMIT_S = 20, 2, 240
SHAPES = ((12, 4, 50), (32, 16, 21))
ROW_CASES = ("16-soc(6,3)", "wide-cone(7,3)")


def child(path, B, grad):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    grad = grad and hasattr(altro._lib.lib(), "altro_batch_evaluate_grad_dev")
    rows = []

    def timed(sv, U, label, with_bytes):
        n, m, N, nc = sv.n, sv.m, sv.N, U.shape[1]
        J, c, d, P = (torch.empty((B, nc), dtype=torch.float64, device=dev) for _ in range(4))
        gU, gx0 = torch.empty_like(U), torch.empty((B, nc, n), dtype=torch.float64, device=dev)
        calls = {"evaluate_dev rollout": lambda: api._evaluate_dev(sv, U, None, None, (J, c, d), None)}
        if grad:
            calls["evaluate_grad_dev rho 10"] = lambda: api._evaluate_grad_dev(sv, U, None, 10.0, (J, P, gU, gx0), None)
            calls["evaluate_grad_dev rho 0"] = lambda: api._evaluate_grad_dev(sv, U, None, 0.0, (J, P, gU, gx0), None)
        times = {k: [] for k in calls}
        reps = 20
        for w in range(WINDOWS + WARM):
            for name, fn in calls.items():       # the variants alternate window by window
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                api.synchronize(sv)
                torch.cuda.synchronize()
                e0.record()
                api.wait_stream(sv)
                for _ in range(reps):
                    fn()
                api.signal_stream(sv)
                e1.record()
                torch.cuda.synchronize()
                if w >= WARM:
                    times[name].append(1e3 * e0.elapsed_time(e1) / reps)
        if grad:
            assert torch.isfinite(gU).all() and torch.isfinite(gx0).all() and torch.isfinite(P).all()
        Rr = B * nc
        dyn = B * (n * (n + m) + n)
        tables = B * N * (n + m) + 4 * (n + m)                                    # reference window, weights and bounds
        states = Rr * N * n
        nbytes = {"evaluate_dev rollout": (Rr * (N - 1) * m + B * n + dyn + tables + 3 * Rr + 2 * states) * 8,
                  "evaluate_grad_dev rho 10": (2 * Rr * (N - 1) * m + B * n + Rr * n + 2 * dyn + tables + 2 * Rr + 2 * states) * 8}
        nbytes["evaluate_grad_dev rho 0"] = nbytes["evaluate_grad_dev rho 10"]
        row = {"n": n, "m": m, "N": N, "ncand": nc, "problem": label, "backend": "16-lane" if n + m <= 16 else "one-wave-per-instance", "calls": {}}
        for name, v in times.items():
            med = statistics.median(v)
            row["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v}
            if with_bytes:
                row["calls"][name].update(bytes_moved=nbytes[name], GB_per_s=nbytes[name] / (med * 1e-6) / 1e9)
            print("(%d, %d, %d) ncand %d %-26s median %9.1f us  min %9.1f  max %9.1f" % (n, m, N, nc, name, med, min(v), max(v)), flush=True)
        rows.append(row)

    for n, m, N in SHAPES:
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        for nc in (1, 8):
            rng = np.random.default_rng(2)
            timed(sv, T(pb.Utrack[:, None, :N - 1] + 0.5 * rng.standard_normal((B, nc, N - 1, m))), "box only", True)
        sv.close()
    import evaluate_ref as ER
    import evaluate_grad_ref as GR
    import warm_start_ref as WR
    for name in ROW_CASES:       # LINEAR and SOC rows: the row value and, at rho 10, its pullback
        make, kw = WR.CASES[name]
        cs = make(B=B)
        sv = api.ALTROSolver(ER.to_problem(altro, cs, **kw), api.SolverOptions(**mpc.REF_OPTS))
        timed(sv, T(GR.candidates_with_polar(cs, 5)), name, False)
        sv.close()
    with open(path, "w") as f:
        json.dump(rows, f)


def main(path, parent_lib, B):
    res = {"batch": B, "windows": WINDOWS, "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)",
           "yardstick": "evaluate_dev, rollout form without Xout, on the parent commit's library", "cases": []}
    parts = {}
    for tag, lib, grad in (("parent", parent_lib, 1), ("this", None, 1)):
        tmp = path + "." + tag + ".tmp"
        env = dict(os.environ)
        env.pop("ALTRO_HIP_LIB", None)
        if lib:
            env["ALTRO_HIP_LIB"] = os.path.abspath(lib)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp, str(B), str(grad)], env=env, timeout=CHILD_LIMIT_S).returncode
        if rc != 0:
            print("child '%s' ended with status %d: nothing more is started" % (tag, rc))
            return rc
        with open(tmp) as f:
            parts[tag] = json.load(f)
        os.remove(tmp)
    for rp, rt in zip(parts["parent"], parts["this"]):
        row = dict(rt)
        row["parent_calls"] = rp["calls"]
        base = rp["calls"]["evaluate_dev rollout"]
        row["ratio_to_parent_evaluate_dev"] = {k: v["median_us"] / base["median_us"] for k, v in rt["calls"].items()}
        if "bytes_moved" in base:
            row["predicted_ratio_from_bytes"] = rt["calls"]["evaluate_grad_dev rho 10"]["bytes_moved"] / base["bytes_moved"]
        print("(%d, %d, %d) ncand %d %s  time / parent's evaluate_dev:" % (row["n"], row["m"], row["N"], row["ncand"], row["problem"]),
              row["ratio_to_parent_evaluate_dev"], " bytes predict %.2f" % row.get("predicted_ratio_from_bytes", float("nan")), flush=True)
        for k, v in rt["calls"].items():       # every call the parent's library has too: this median - parent median against the parent's own spread
            if k in rp["calls"]:
                q = rp["calls"][k]
                print("    %-26s parent %9.1f (max - min %6.1f)  this %9.1f  diff %+7.1f  %s" % (
                    k, q["median_us"], q["max_us"] - q["min_us"], v["median_us"], v["median_us"] - q["median_us"],
                    "within" if v["median_us"] - q["median_us"] <= q["max_us"] - q["min_us"] else "NOT within"), flush=True)
        res["cases"].append(row)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        sys.exit(main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 8192))
