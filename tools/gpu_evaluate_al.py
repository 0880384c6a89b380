"""What one altro_batch_evaluate_al_dev launch costs, beside altro_batch_evaluate_grad_dev at rho = 10 on the same
shapes timed ON THE PARENT COMMIT'S LIBRARY, in its own process, as the yardstick: the same rollout, the same reverse sweep
with zero multipliers.
Two fresh child processes, the parent's library first (ALTRO_HIP_LIB selects the library, as in the other A/B tools), then this
build's; each has its own time limit, and a child that ends abnormally ends the tool and nothing more is started.
HIP events on torch's stream around a window of back-to-back calls on the solver's stream between wait_stream and
signal_stream, device time per call = window / calls; two warm-up windows, then the median, minimum and maximum over 20
windows.  The 16-lane backend at (12, 4, N = 50) and the one-wave-per-instance backend at (32, 16, N = 21), batch 8192,
ncand 1 and 8, after one solve (the duals and the penalty it left), once with all twelve outputs and once with LA + gU + gx0.
bytes_moved: what a call cannot avoid -- evaluate_grad_dev's bytes (tools/gpu_evaluate_grad.py) and, on top of them, the box
duals of every knot read once, the penalty, and the outputs written: for all outputs gXref, gUref, gQ, gQf, gR, gzmin, gzmax
and Xout (which replaces the workspace: no extra bytes).
Usage: gpu_evaluate_al.py out.json <parent libaltro_hip.so> [batch] [this-first]   (this-first: this build's child runs before
the parent's, to tell an effect of the order of the two processes from one of the build)"""
import json, os, statistics, subprocess, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (R, os.path.join(R, "tests")):
    sys.path.insert(0, p_)
WINDOWS, WARM, CHILD_LIMIT_S = 20, 2, 240
SHAPES = ((12, 4, 50), (32, 16, 21))


def child(path, B):
    import numpy as np
    import torch
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    from altro_mpc_icra2021_amd import api, mpc, problems
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    has_al = hasattr(altro._lib.lib(), "altro_batch_evaluate_al_dev")
    rows = []

    def timed(sv, U):
        n, m, N, nc = sv.n, sv.m, sv.N, U.shape[1]
        E = lambda *s: torch.empty((B, nc) + s, dtype=torch.float64, device=dev)
        J, P, gU, gx0 = E(), E(), torch.empty_like(U), E(n)
        calls = {"evaluate_grad_dev rho 10": lambda: api._evaluate_grad_dev(sv, U, None, 10.0, (J, P, gU, gx0), None)}
        if has_al:
            full = dict(LA=E(), J=J, gU=gU, gx0=gx0, gXref=E(N, n), gUref=E(N - 1, m), gQ=E(n), gQf=E(n), gR=E(m), gzmin=E(n + m), gzmax=E(n + m),
                        Xout=E(N, n))
            three = {k: full[k] for k in ("LA", "gU", "gx0")}
            st = {k: altro._lib.ALOut(**{f: t.data_ptr() for f, t in o.items()}) for k, o in (("all", full), ("three", three))}
            import ctypes as C
            E_ = sv._L.altro_batch_evaluate_al_dev
            calls["evaluate_al_dev all outputs"] = lambda: sv._chk(E_(sv.h, nc, C.c_void_p(U.data_ptr()), None, C.byref(st["all"])))
            calls["evaluate_al_dev LA gU gx0"] = lambda: sv._chk(E_(sv.h, nc, C.c_void_p(U.data_ptr()), None, C.byref(st["three"])))
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
        assert torch.isfinite(gU).all() and torch.isfinite(gx0).all()
        Rr = B * nc
        dyn = B * (n * (n + m) + n)
        tables = B * N * (n + m) + 4 * (n + m)                                    # reference window, weights and bounds
        states = Rr * N * n
        grad = 2 * Rr * (N - 1) * m + B * n + Rr * n + 2 * dyn + tables + 2 * Rr + 2 * states
        duals = B * N * 2 * m + B                                                 # the box bounds the controls: 2 m duals per knot
        nbytes = {"evaluate_grad_dev rho 10": grad * 8, "evaluate_al_dev LA gU gx0": (grad - Rr + duals) * 8,
                  "evaluate_al_dev all outputs": (grad + duals + states + Rr * (N - 1) * m + Rr * (2 * n + m + 2 * (n + m))) * 8}
        row = {"n": n, "m": m, "N": N, "ncand": nc, "backend": "16-lane" if n + m <= 16 else "one-wave-per-instance", "calls": {}}
        for name, v in times.items():
            med = statistics.median(v)
            row["calls"][name] = {"median_us": med, "min_us": min(v), "max_us": max(v), "windows_us": v, "bytes_moved": nbytes[name],
                                  "GB_per_s": nbytes[name] / (med * 1e-6) / 1e9}
            print("(%d, %d, %d) ncand %d %-28s median %9.1f us  min %9.1f  max %9.1f" % (n, m, N, nc, name, med, min(v), max(v)), flush=True)
        rows.append(row)

    for n, m, N in SHAPES:
        pb = problems.gen_random_linear_batch(B, n=n, m=m, N=N, steps=1, seed=1)
        sv = api.ALTROSolver(mpc.gen_tracking_problem(pb), api.SolverOptions(**mpc.REF_OPTS))
        api.solve(sv)
        for nc in (1, 8):
            rng = np.random.default_rng(2)
            timed(sv, T(pb.Utrack[:, None, :N - 1] + 0.5 * rng.standard_normal((B, nc, N - 1, m))))
        sv.close()
    with open(path, "w") as f:
        json.dump(rows, f)


def main(path, parent_lib, B, this_first=False):
    res = {"batch": B, "windows": WINDOWS, "unit": "device microseconds per call (HIP events around a window of back-to-back calls / calls)",
           "yardstick": "evaluate_grad_dev, rho = 10, all four outputs, on the parent commit's library in its own process", "cases": []}
    parts = {}
    order = (("parent", parent_lib), ("this", None))
    res["order"] = "this build's child first" if this_first else "the parent's child first"
    for tag, lib in (order[::-1] if this_first else order):
        tmp = path + "." + tag + ".tmp"
        env = dict(os.environ)
        env.pop("ALTRO_HIP_LIB", None)
        if lib:
            env["ALTRO_HIP_LIB"] = os.path.abspath(lib)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp, str(B)], env=env, timeout=CHILD_LIMIT_S).returncode
        if rc != 0:
            print("child '%s' ended with status %d: nothing more is started" % (tag, rc))
            return rc
        with open(tmp) as f:
            parts[tag] = json.load(f)
        os.remove(tmp)
    for rp, rt in zip(parts["parent"], parts["this"]):
        row = dict(rt)
        row["parent_calls"] = rp["calls"]
        base = rp["calls"]["evaluate_grad_dev rho 10"]
        row["ratio_to_parent_evaluate_grad_dev"] = {k: v["median_us"] / base["median_us"] for k, v in rt["calls"].items()}
        row["predicted_ratio_from_bytes"] = {k: v["bytes_moved"] / base["bytes_moved"] for k, v in rt["calls"].items()}
        print("(%d, %d, %d) ncand %d  time / parent's evaluate_grad_dev:" % (row["n"], row["m"], row["N"], row["ncand"]),
              {k: round(v, 3) for k, v in row["ratio_to_parent_evaluate_grad_dev"].items()}, " bytes predict",
              {k: round(v, 3) for k, v in row["predicted_ratio_from_bytes"].items()}, flush=True)
        res["cases"].append(row)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit(main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 8192, "this-first" in sys.argv[4:]))
