"""What the active mask buys and costs on the headline closed loop ((12, 4, 50), batch 8192, 20-step fused windows): a
handful of instances are made hard -- control bounds so tight (altro_batch_set_bounds, per instance) that their solves run
into the iteration caps -- and a window is timed with them active and with them masked out; then the plain cost of an
explicit all-active mask against no mask on the unmodified batch.  Illustration only: prints one JSON line.
Usage: python tools/gpu_active_mask_cost.py [--batch 8192] [--hard 8] [--windows 6]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import altro_amd_loader  # noqa: E402,F401
import altro_mpc_icra2021_amd as altro  # noqa: E402
from altro_mpc_icra2021_amd import api  # noqa: E402


def windows(mp, first, S, W):
    out = []
    for w in range(W):
        altro.timing_reset(mp.solver)
        mp.run_async(S, first=first + w * S)
        mp.synchronize()
        out.append(float(altro.timing_get(mp.solver).sum()))
    return out


def started(pb, hard, tight):
    mp = altro.mpc.BatchMPC(pb)
    if len(hard):
        ub = np.full(pb.A.shape[0], float(pb.u_bnd))
        ub[hard] = tight
        lo = np.c_[np.full((len(ub), pb.n), -np.inf), -np.repeat(ub[:, None], pb.m, axis=1)]
        api.set_bounds(mp.solver, 0, lo, -lo)
    mp.initial_solve()
    for i in range(5):
        mp.step(i)
    return mp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--hard", type=int, default=8)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--tight", type=float, default=0.02)
    a = ap.parse_args()
    B, S, W = a.batch, 20, a.windows
    pb = altro.problems.gen_random_linear_batch(B, n=12, m=4, N=50, steps=5 + S * W, seed=1)
    hard = np.linspace(0, B - 1, a.hard).astype(int)
    res = dict(batch=B, steps_per_window=S, windows=W, hard_instances=int(a.hard), tight_bound=a.tight)
    for tag, mask in (("hard_active", None), ("hard_masked", True)):
        mp = started(pb, hard, a.tight)
        if mask:
            act = np.ones(B, dtype=np.int32)
            act[hard] = 0
            mp.set_active(act)
        ms = windows(mp, 5, S, W)
        it = altro.solve_counters(mp.solver)[1]
        res[tag + "_ms"] = [round(x, 3) for x in ms]
        res[tag + "_mean_ms"] = round(float(np.mean(ms)), 3)
        res[tag + "_max_iterations_per_window"] = int(it.max())
        mp.solver.close()
    for tag, mask in (("no_mask", False), ("explicit_all_active", True), ("no_mask_again", False)):
        mp = started(pb, [], a.tight)
        if mask:
            mp.set_active(np.ones(B, dtype=np.int32))
        ms = windows(mp, 5, S, W)
        res[tag + "_ms"] = [round(x, 3) for x in ms]
        res[tag + "_mean_ms"] = round(float(np.mean(ms)), 3)
        mp.solver.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
