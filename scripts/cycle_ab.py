#!/usr/bin/env python3
"""Speed of the per-generation grid fingerprint (LifeConfig.fingerprint) and of
Simulation.find_cycle in one process and one GPU visit.

cost (default): on SIZE^2 cells (bit layout, a dense soup PREWARM generations
old) these engines take turns within each round -

  plain        the torus forced onto the fingerprint's schedule:
               xlane=0 link=0 quiet_skip=0 lazy_tail=0 (the like-for-like baseline);
  census       plain with the census on, at its default block size;
  fprint_t8, fprint_t12, fprint_t16
               plain with the fingerprint on, at T = 8, 12 and 16.

Every engine runs ROUNDS x advance(1000) timed; then VERIFY further
generations of each fingerprint engine are checked entry by entry against the
stand-alone fingerprint kernel on the plain engine stepped one generation at a
time.  One JSON line per engine: ms per 1000 generations (median, min, max) and
the ratio of its median to plain's and to the census's.

settle: a SIZE^2 soup (seed 1, density 0.5) is advanced to generation START on
a fingerprint engine, then find_cycle(START + MAXGENS, PERIOD) runs: how many
generations and how much time it needs.  One JSON line.

    python scripts/cycle_ab.py cost [SIZE] [ROUNDS] [VERIFY] [PREWARM]
    python scripts/cycle_ab.py settle [SIZE] [START] [MAXGENS] [PERIOD]

docs/PERFORMANCE.md "Cycle detection".
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import gol_amd  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "cost"
arg = [int(v) for v in sys.argv[2:]]
PLAIN = {"xlane": "0", "link": "0", "quiet_skip": "0", "lazy_tail": "0"}


def make(S, tune, tmax=0, **kw):
    return gol_amd.Simulation(gol_amd.LifeConfig(S, S, gen_limit=10**9, check_similarity=False, layout="bits",
                                                 tmax=tmax, tune=tune, **kw), engine="hip")


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
    S, rounds, verify, prewarm = (arg + [32768, 20, 8, 100][len(arg):])[:4]
    ENGINES = {"plain": (0, {}), "census": (0, {"census": True}),
               **{f"fprint_t{t}": (t, {"fingerprint": True}) for t in (8, 12, 16)}}
    sims = {}
    for name, (tmax, kw) in ENGINES.items():
        s = make(S, PLAIN, tmax, **kw)
        s.init_random(1, 0.5)
        s.advance(prewarm)
        sims[name] = s
    ms = {name: [] for name in ENGINES}
    for _ in range(rounds):
        for name, s in sims.items():
            ms[name].append(timed(lambda: s.advance(1000))[1])
    # The plain engine, one generation at a time, and the stand-alone kernel.
    want = []
    for _ in range(verify):
        sims["plain"].advance(1)
        want.append(sims["plain"].fingerprint())
    ok = True
    for name, s in sims.items():
        med = statistics.median(ms[name])
        rec = {"engine": name, "size": S, "prewarm": prewarm, "rounds": rounds, **describe(s.describe()),
               "ms_per_1000_median": round(med, 4), "ms_per_1000_min": round(min(ms[name]), 4),
               "ms_per_1000_max": round(max(ms[name]), 4), "ms_per_1000_rounds": [round(v, 3) for v in ms[name]],
               "ratio_to_plain": round(med / statistics.median(ms["plain"]), 4),
               "ratio_to_census": round(med / statistics.median(ms["census"]), 4)}
        if verify > 0 and name.startswith("fprint"):
            rep = s.advance(verify)
            rec["verified_generations"] = verify
            rec["verified"] = [int(v) for v in rep.fingerprint] == want and s.fingerprint() == want[-1]
            ok = ok and rec["verified"]
        print(json.dumps(rec), flush=True)
    sys.exit(0 if ok else 1)

if mode == "settle":
    S, start, maxgens, period = (arg + [32768, 10192, 200000, 64][len(arg):])[:4]
    s = make(S, {}, fingerprint=True)
    s.init_random(1, 0.5)
    _, t_start = timed(lambda: s.advance(start))
    alive0 = s.alive_count()
    r, t = timed(lambda: s.find_cycle(start + maxgens, period))
    rec = {k: v for k, v in r.as_dict().items() if k != "loop_ms"}
    print(json.dumps({"mode": "settle", "size": S, "start": start, "max_gens": maxgens, "max_period": period,
                      "advance_to_start_ms": round(t_start, 2), "alive_at_start": alive0,
                      "find_cycle_ms": round(t, 2), "generations_run": r.generation - start,
                      "ms_per_1000": round(t / max(1, r.generation - start) * 1000, 4), **rec,
                      "alive_at_end": s.alive_count(), "engine": describe(s.describe())}), flush=True)
    sys.exit(0)

sys.exit(f"unknown mode {mode!r} (want cost or settle)")
