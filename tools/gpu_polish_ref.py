"""Largest error / bound of every check of tests/test_polish_gpu.py, per backend: the projected-Newton polish on the device
against the dense yardstick (tests/polish_ref.py) and against the oracle, on the cases of tests/polish_cases.py.
python tools/gpu_polish_ref.py [out.json]   (default: profiles/polish_ref.json)"""
import sys, os, json
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "oracle"), os.path.join(R, "tests")):
    sys.path.insert(0, p)
import numpy as np
import altro_amd_loader
import altro_mpc_icra2021_amd as altro
import polish_cases as PC

RTOL = 1e-6
worst = {"lane16": {}, "wide": {}}
cases = {}
for cid in PC.CASE_IDS:
    c = PC.case(cid)
    tw, po = PC.device_pair(altro, c)
    rec = {"backend": c.backend, "shape": [c.n, c.m, c.N], "reaches": list(c.reaches), "instances": []}
    for b in range(c.batch):
        _, opo = PC.oracle_pair(cid, b)
        ratios, ok, why = PC.judge_device(c, b, tw, po)
        ratios["oracle parity X"] = float(np.abs(po.X[b] - opo.X).max() / max(1.0, np.abs(opo.X).max()) / RTOL)
        ratios["oracle parity U"] = float(np.abs(po.U[b] - opo.U).max() / max(1.0, np.abs(opo.U).max()) / RTOL)
        rec["instances"].append({"admissible": ok, "why_not": why, "polish_residual": float(po.residual[b]), "ratios": ratios})
        for k, v in ratios.items():
            w = worst[c.backend].setdefault(k, {"ratio": -1.0, "case": None})
            if v > w["ratio"]:
                w["ratio"], w["case"] = float(v), "%s[%d]" % (cid, b)
    cases[cid] = rec
    print(cid, {k: "%.3g" % max(i["ratios"].get(k, 0.0) for i in rec["instances"]) for k in rec["instances"][0]["ratios"]}, flush=True)
out = {"what": "error / bound, largest over the cases of tests/polish_cases.py (3 instances each); a ratio above 1 fails tests/test_polish_gpu.py",
       "worst": worst, "cases": cases}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, "profiles", "polish_ref.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(worst))
