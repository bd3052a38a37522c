#!/usr/bin/env python3
"""Speed of the population census (LifeConfig.census) in one process and one
GPU visit.

cost (default): on SIZE^2 cells (bit layout, a dense soup PREWARM generations
old) four engines take turns within each round -

  default       the torus with its defaults (adder window, linked launches,
                quiet-tile policy, lazy tail, folded strip);
  plain         the torus forced onto the census's schedule:
                xlane=0 link=0 quiet_skip=0 lazy_tail=0;
  plain_nofold  plain, and fold=0 chain=0 (what the census also turns off);
  census        plain with census on.

TMAX (default 0: the engine's choice) is the block size of the last three.
Every engine runs ROUNDS x advance(1000) timed (the default engine's rounds
are listed one by one: as the soup settles its skipping kernel takes over,
which none of the others has); then VERIFY further generations
of each are checked against life_step_torch_roll, and the census's series over
them against the oracle stepped one generation at a time.  One JSON line per
engine: ms per 1000 generations (median, min, max) and the ratio of its median
to plain's and to plain_nofold's.

loop: on SIZE^2 cells GENS generations, the census run (one advance(GENS)
with census on, engine otherwise default) against the loop that existed before
it, advance(1); alive_count() GENS times on the default engine, ROUNDS times
each, taking turns; the two series must be equal.  One JSON line.

    python scripts/census_ab.py cost [SIZE] [ROUNDS] [VERIFY] [PREWARM] [TMAX]
    python scripts/census_ab.py loop [SIZE] [GENS] [ROUNDS]

docs/PERFORMANCE.md "Population census".
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gol_amd  # noqa: E402
from gol_amd.ops.life_ops import life_step_torch_roll  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "cost"
arg = [int(v) for v in sys.argv[2:]]


def make(S, census, tune, tmax=0):
    return gol_amd.Simulation(gol_amd.LifeConfig(S, S, gen_limit=10**9, check_similarity=False, layout="bits",
                                                 census=census, tmax=tmax, tune=tune), engine="hip")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def describe(d):
    return {k: d[k] for k in ("kernel", "tmax", "epoch", "row_ring", "drifting", "quiet_mode", "launch_paths",
                              "tuning_changed")}


if mode == "cost":
    S, rounds, verify, prewarm, tmax = (arg + [32768, 20, 24, 100, 0][len(arg):])[:5]
    PLAIN = {"xlane": "0", "link": "0", "quiet_skip": "0", "lazy_tail": "0"}
    NOFOLD = dict(PLAIN, fold="0", chain="0")
    ENGINES = {"default": (False, {}), "plain": (False, PLAIN), "plain_nofold": (False, NOFOLD),
               "census": (True, PLAIN)}
    sims = {}
    for name, (census, tune) in ENGINES.items():
        s = make(S, census, tune, tmax if tune else 0)
        s.init_random(1, 0.5)
        s.advance(prewarm)
        sims[name] = s
    ms = {name: [] for name in ENGINES}
    for _ in range(rounds):
        for name, s in sims.items():
            ms[name].append(timed(lambda: s.advance(1000))[1])
    ok = True
    for name, s in sims.items():
        med = statistics.median(ms[name])
        rec = {"engine": name, "census": ENGINES[name][0], "size": S, "prewarm": prewarm, "rounds": rounds,
               **describe(s.describe()),
               "ms_per_1000_median": round(med, 4), "ms_per_1000_min": round(min(ms[name]), 4),
               "ms_per_1000_max": round(max(ms[name]), 4),
               "ms_per_1000_rounds": [round(v, 3) for v in ms[name]],
               "ratio_to_plain": round(med / statistics.median(ms["plain"]), 4),
               "ratio_to_plain_nofold": round(med / statistics.median(ms["plain_nofold"]), 4)}
        if verify > 0:
            x = s.tile()
            rep = s.advance(verify)
            pop = []
            for _ in range(verify if ENGINES[name][0] else 0):
                x = life_step_torch_roll(x, 1, device="cuda")
                pop.append(int(x.sum(dtype=np.int64)))
            if not ENGINES[name][0]:
                x = life_step_torch_roll(x, verify, device="cuda")
            rec["verified_generations"] = verify
            rec["verified"] = bool((s.tile() == x).all()) and rep.population.tolist() == pop
            rec["alive"] = int(x.sum(dtype=np.int64))
            ok = ok and rec["verified"]
            del x
        print(json.dumps(rec), flush=True)
    sys.exit(0 if ok else 1)

if mode == "loop":
    S, gens, rounds = (arg + [4096, 1000, 5][len(arg):])[:3]
    census, loop = make(S, True, {}), make(S, False, {})
    for s in (census, loop):
        s.init_random(1, 0.5)

    def run_loop():
        out = []
        for _ in range(gens):
            loop.advance(1)
            out.append(loop.alive_count())
        return out

    t_census, t_loop, same = [], [], True
    for _ in range(rounds):
        rep, t = timed(lambda: census.advance(gens))
        t_census.append(t)
        series, t = timed(run_loop)
        t_loop.append(t)
        same = same and rep.population.tolist() == series
    same = same and bool((census.tile() == loop.tile()).all())
    mc, ml = statistics.median(t_census), statistics.median(t_loop)
    print(json.dumps({"mode": "loop", "size": S, "generations": gens, "rounds": rounds,
                      "census_ms_median": round(mc, 3), "census_ms_min": round(min(t_census), 3),
                      "census_ms_max": round(max(t_census), 3), "loop_ms_median": round(ml, 3),
                      "loop_ms_min": round(min(t_loop), 3), "loop_ms_max": round(max(t_loop), 3),
                      "loop_over_census": round(ml / mc, 2), "series_equal": same,
                      "census_engine": describe(census.describe()), "loop_engine": describe(loop.describe())}),
          flush=True)
    sys.exit(0 if same else 1)

sys.exit(f"unknown mode {mode!r} (want cost or loop)")
