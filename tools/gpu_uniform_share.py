"""Share of the four-row rollouts and first-order sweeps of the fused headline launch that run as the wave-uniform
variant (solve_dpp16.h uniform_phase), from the form counters of altro_batch_get_wave_passes:
python tools/gpu_uniform_share.py [steps] [batch].  With ALTRO_NO_SHADOW=1 none is uniform."""
import sys, os, json
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import altro_amd_loader
import altro_mpc_icra2021_amd as altro
S = int(sys.argv[1]) if len(sys.argv) > 1 else 100
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
pb = altro.problems.gen_random_linear_batch(B, steps=S + 5)
mp = altro.mpc.BatchMPC(pb)
mp.initial_solve()
for i in range(5): mp.step(i)
altro.timing_reset(mp.solver)
mp.run_async(S, first=5); mp.synchronize()
w = altro.wave_passes(mp.solver)[:, 1:4]
uni, gen = (w & 0xFFFF).sum(0), (w >> 16).sum(0)
nb, nr, ntr = altro.work_counters(mp.solver)
out = {"steps": S, "batch": B, "waves": int(w.shape[0])}
for i, name in enumerate(("open_rollout", "closed_rollout", "first_order_sweep")):
    tot = int(uni[i] + gen[i])
    out[name] = {"four_row_phases": tot, "uniform": int(uni[i]), "generic": int(gen[i]), "uniform_share": float(uni[i]) / max(1, tot)}
    print("%-18s four-row phases %8d  uniform %8d  generic %8d  share %.3f  (%.1f per wave)" % (name, tot, uni[i], gen[i], uni[i] / max(1, tot), tot / w.shape[0]))
tot = int(uni.sum() + gen.sum())
out["all"] = {"four_row_phases": tot, "uniform_share": float(uni.sum()) / max(1, tot)}
out["rollouts_per_instance"] = float(nr.sum()) / B
print("all                four-row phases %8d  share %.3f; rollouts per instance (every form) %.1f" % (tot, uni.sum() / max(1, tot), nr.sum() / B))
print(json.dumps(out))
