"""What the per-step MPC log costs on the headline workload: kernel time of twelve consecutive 20-step
windows of the closed loop, batch 8192, (12, 4, 50), for several builds of the library (ALTRO_HIP_LIB) with the log off or on.
Every configuration runs in a process of its own, each window right after 200 steps of a scratch copy of the batch (clocks
up), the configurations alternating, twice over.  Raw window times go to the JSON file.
Usage: gpu_mpc_log_cost.py out.json tag=lib.so[:log] [tag=lib.so[:log] ...]      (":log": altro_mpc_set_log before the windows)"""
import json, os, subprocess, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
B, S, W = 8192, 20, 12
if len(sys.argv) == 3 and sys.argv[1] == "--child":
    import altro_amd_loader  # noqa: F401
    import altro_mpc_icra2021_amd as altro
    log_on = sys.argv[2] == "1"
    pb = altro.problems.gen_random_linear_batch(B, n=12, m=4, N=50, steps=5 + S * W + 200, seed=1)
    mp, heat = altro.mpc.BatchMPC(pb), altro.mpc.BatchMPC(pb)
    for m_ in (mp, heat):
        m_.initial_solve()
        for i in range(5):
            m_.step(i)
    if log_on:
        mp.enable_log(5 + S * W)     # a window touches the records of its own 20 steps, as a log of capacity 25 would
    out = []
    for w in range(W):
        heat.run_async(100, first=5); heat.run_async(100, first=105); heat.synchronize()
        altro.timing_reset(mp.solver)
        mp.run_async(S, first=5 + w * S); mp.synchronize()
        out.append(float(altro.timing_get(mp.solver).sum()))
    if log_on:
        lg = mp.log(5, S * W)
        assert (lg.iterations >= 1).all() and (lg.status == 1).mean() > 0.99
    print(json.dumps(out), flush=True)
else:
    path, cfgs = sys.argv[1], sys.argv[2:]
    res = {"batch": B, "steps_per_window": S, "windows_per_run": W, "unit": "ms per window (sum of the launch's kernel times)", "runs": []}
    for rep in range(2):
        for a in cfgs:
            tag, lib = a.split("=", 1)
            log_on = lib.endswith(":log")
            lib = lib[:-4] if log_on else lib
            e = dict(os.environ); e["ALTRO_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "1" if log_on else "0"], env=e, stdout=subprocess.PIPE, text=True, timeout=400)
            if p.returncode != 0:
                sys.exit("run %s failed with status %d" % (tag, p.returncode))     # nothing more is started on the device
            ms = json.loads(p.stdout.strip().splitlines()[-1])
            res["runs"].append({"tag": tag, "log": log_on, "rep": rep, "ms": ms})
            print("%-12s" % tag, " ".join("%6.2f" % x for x in ms), flush=True)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
    import statistics
    for tag in dict.fromkeys(r["tag"] for r in res["runs"]):
        ms = [x for r in res["runs"] if r["tag"] == tag for x in r["ms"]]
        print("%-12s median %.3f  min %.3f  max %.3f  (%d windows)" % (tag, statistics.median(ms), min(ms), max(ms), len(ms)))
