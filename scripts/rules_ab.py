#!/usr/bin/env python3
"""Speed of the Life-like rule kernels beside B3/S23, in one process and one
GPU visit: on SIZE^2 cells (bit layout, default window and T) every rule runs
advance(8192) untimed, then ROUNDS x advance(1000) timed, the rules taking
turns within each round, and finally VERIFY further generations of every rule
are checked against life_step_torch_roll(rule=).  Prints one JSON line per
rule: ms per 1000 generations (median, min, max) and the ratio of its median
to B3/S23's from the same call (docs/PERFORMANCE.md "Life-like rules").
DENSITY (default 0.5) is the initial density; 0 times every kernel on an empty
grid, which stays empty under any rule: the same instructions on all-zero
operands, which separates instruction issue from the clock the chip holds on
the data (a dense chaotic rule toggles far more bits than B3/S23's sparse ash).

    python scripts/rules_ab.py [SIZE] [ROUNDS] [VERIFY] [DENSITY]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import gol_amd  # noqa: E402
from gol_amd.ops.life_ops import life_step_torch_roll  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
verify = int(sys.argv[3]) if len(sys.argv) > 3 else 240
density = float(sys.argv[4]) if len(sys.argv) > 4 else 0.5

rules = gol_amd.native().hip_rules()  # B3/S23 first
assert rules and rules[0] == "B3/S23" and len(rules) > 1, rules
sims = {}
for rule in rules:
    s = gol_amd.Simulation(gol_amd.LifeConfig(S, S, gen_limit=10**9, check_similarity=False, layout="bits",
                                              rule=rule), engine="hip")
    s.init_random(1, density)
    s.advance(8192)
    sims[rule] = s
ms = {rule: [] for rule in rules}
for _ in range(rounds):
    for rule, s in sims.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.advance(1000)
        torch.cuda.synchronize()
        ms[rule].append((time.perf_counter() - t0) * 1e3)
base = statistics.median(ms[rules[0]])
ok = True
for rule, s in sims.items():
    d = s.describe()
    rec = {"rule": rule, "size": S, "density": density, "kernel": d["kernel"], "tmax": d["tmax"], "rounds": rounds,
           "ms_per_1000_median": round(statistics.median(ms[rule]), 4), "ms_per_1000_min": round(min(ms[rule]), 4),
           "ms_per_1000_max": round(max(ms[rule]), 4), "ratio_to_default": round(statistics.median(ms[rule]) / base, 4)}
    if verify > 0:
        before = s.tile()
        s.advance(verify)
        want = life_step_torch_roll(before, verify, device="cuda", rule=rule)
        rec["verified_generations"] = verify
        rec["verified"] = bool((s.tile() == want).all())
        rec["alive"] = int(want.sum())
        ok = ok and rec["verified"]
        del before, want
    print(json.dumps(rec), flush=True)
sys.exit(0 if ok else 1)
