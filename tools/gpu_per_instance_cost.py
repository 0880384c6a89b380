"""Cost of the per-instance mode: kernel time of 20 fused MPC steps of the headline closed loop (batch 8192, (12, 4, 50)) with
the cost weights and bounds given once for the batch and given per instance (every row the same: the results are identical,
only the tables differ).  The two handles alternate window by window, each window right after 200 steps of a scratch copy
(clocks up).  Prints one line per mode and the ratio of the means.
Usage: gpu_per_instance_cost.py [windows]"""
import sys, os, json
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import altro_amd_loader  # noqa: F401
import altro_mpc_icra2021_amd as altro

B, S = 8192, 20
W = int(sys.argv[1]) if len(sys.argv) > 1 else 8
pb = altro.problems.gen_random_linear_batch(B, n=12, m=4, N=50, steps=5 + S * W + 200, seed=1)
pi = altro.problems.gen_random_linear_batch(B, n=12, m=4, N=50, steps=5 + S * W + 200, seed=1)
pi.Qk, pi.Rk, pi.Qfk = np.full((B, pb.n), pb.Qk), np.full((B, pb.m), pb.Rk), np.full((B, pb.n), pb.Qfk)
pi.u_bnd = np.full(B, pb.u_bnd)
mps = {"shared": altro.mpc.BatchMPC(pb), "per_instance": altro.mpc.BatchMPC(pi)}
heat = altro.mpc.BatchMPC(pb)
for m_ in list(mps.values()) + [heat]:
    m_.initial_solve()
    for i in range(5):
        m_.step(i)
out = {k: [] for k in mps}
for w in range(W):
    for k, mp in mps.items():
        heat.run_async(100, first=5); heat.run_async(100, first=105); heat.synchronize()
        altro.timing_reset(mp.solver)
        mp.run_async(S, first=5 + w * S); mp.synchronize()
        out[k].append(float(altro.timing_get(mp.solver).sum()))
assert np.array_equal(altro.states(mps["shared"].solver), altro.states(mps["per_instance"].solver))
for k, v in out.items():
    print("%-13s" % k, " ".join("%6.2f" % x for x in v), " | mean %.3f ms" % np.mean(v), flush=True)
print(json.dumps({"B": B, "steps": S, "windows": W, "shared_ms": float(np.mean(out["shared"])),
                  "per_instance_ms": float(np.mean(out["per_instance"])),
                  "ratio": float(np.mean(out["per_instance"]) / np.mean(out["shared"]))}))
