#!/usr/bin/env python3
"""Speed of the bounded plane (boundary="dead") beside the torus, in one
process and one GPU visit: on SIZE^2 cells (bit layout) three engines take
turns within each round -

  torus        the torus with its defaults (adder window, row ring, wrapped
               columns, quiet-tile policy, lazy tail);
  torus_plain  the torus forced onto the plane's schedule: the DPP window, no
               row ring, no wrapped columns, no skipping, no lazy tail;
  plane        the bounded plane.

Every engine runs advance(8192) untimed, then ROUNDS x advance(1000) timed, and
finally VERIFY further generations of each are checked against
life_step_torch_roll with the matching boundary.  Prints one JSON line per
engine: ms per 1000 generations (median, min, max) and the ratio of its median
to torus_plain's, the plane's yardstick (the plane adds its mask ops to the same
level body; the torus's lead over both is the price of the torus-only fast
paths).  docs/PERFORMANCE.md "Bounded plane".

    python scripts/boundary_ab.py [SIZE] [ROUNDS] [VERIFY] [DENSITY]
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

PLAIN = {"xlane": "0", "row_ring": "0", "wrap": "0", "quiet_skip": "0", "lazy_tail": "0"}
ENGINES = {"torus": ("torus", {}), "torus_plain": ("torus", PLAIN), "plane": ("dead", {})}

sims = {}
for name, (boundary, tune) in ENGINES.items():
    s = gol_amd.Simulation(gol_amd.LifeConfig(S, S, gen_limit=10**9, check_similarity=False, layout="bits",
                                              boundary=boundary, tune=tune), engine="hip")
    s.init_random(1, density)
    s.advance(8192)
    sims[name] = s
ms = {name: [] for name in ENGINES}
for _ in range(rounds):
    for name, s in sims.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.advance(1000)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3)
base = statistics.median(ms["torus_plain"])
ok = True
for name, s in sims.items():
    d = s.describe()
    rec = {"engine": name, "boundary": d["boundary"], "size": S, "density": density, "kernel": d["kernel"],
           "tmax": d["tmax"], "epoch": d["epoch"], "row_ring": d["row_ring"], "drifting": d["drifting"],
           "quiet_mode": d["quiet_mode"], "launch_paths": d["launch_paths"], "tuning_changed": d["tuning_changed"],
           "rounds": rounds,
           "ms_per_1000_median": round(statistics.median(ms[name]), 4), "ms_per_1000_min": round(min(ms[name]), 4),
           "ms_per_1000_max": round(max(ms[name]), 4),
           "ratio_to_torus_plain": round(statistics.median(ms[name]) / base, 4)}
    if verify > 0:
        before = s.tile()
        s.advance(verify)
        want = life_step_torch_roll(before, verify, device="cuda", boundary=d["boundary"])
        rec["verified_generations"] = verify
        rec["verified"] = bool((s.tile() == want).all())
        rec["alive"] = int(want.sum())
        ok = ok and rec["verified"]
        del before, want
    print(json.dumps(rec), flush=True)
sys.exit(0 if ok else 1)
