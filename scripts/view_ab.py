#!/usr/bin/env python3
"""Speed of the density map, the window read and the pattern placement
(Simulation.density / window / place) in one process and one GPU visit.

reduce: on SIZE^2 cells (a soup of density 0.5) the synchronous calls

  alive_count   the one whole-grid reduction there was before (tile_ops.hip
                alive_k: 4-byte loads, a hipMallocAsync per call);
  density_32    density(32): one output block per word and 32 rows;
  density_1024  density(1024);
  density_33    density(33): every word cut at a block edge;
  u8_bits_32    density(32) of a byte engine whose state is its bit image
                (directly after advance(12); SIZE <= 32768 only, for memory)

run one after the other, each WARM untimed and then CALLS timed calls in a row,
host clock around the call; alive_count comes last (its stream-ordered
allocation is returned to the system at every call, which the calls after it
would pay for), and the byte engine is made after the bit engine is done.  One
JSON line per call: median / min / max ms, GB/s of bit words at the median,
ratio of the median to alive_count's and to density_32's; every map is checked
against alive_count (its sum) once.

window: on SIZE^2 cells, window(x, y, 256, 256), place(256 x 256) and
store_rows(y, 256) (the band read-out there was before), the same way, in
microseconds.

frames: the benchmark's workload, SIZE^2 cells for CHUNKS x advance(K), with
and without a density(BLOCK) map after every chunk, taking turns in ROUNDS
rounds; per chunk the time of the advance and of the map, the engine's mode
(quiet_mode, tail_replays, drift before the map) - so the cost of a frame while
the soup is dense and once the skipping kernel has taken over can be read off.

    python scripts/view_ab.py reduce [SIZE] [CALLS] [WARM]
    python scripts/view_ab.py window [SIZE] [CALLS] [WARM]
    python scripts/view_ab.py frames [SIZE] [CHUNKS] [K] [BLOCK] [ROUNDS]

docs/PERFORMANCE.md "Density maps and windows".
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

mode = sys.argv[1] if len(sys.argv) > 1 else "reduce"
arg = [int(v) for v in sys.argv[2:]]


def make(S, layout="bits", tune=None):
    return gol_amd.Simulation(gol_amd.LifeConfig(S, S, gen_limit=10**9, check_similarity=False, layout=layout,
                                                 tune=tune or {}), engine="hip")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def take_turns(calls, n, warm):
    """{name: [ms] * n}: `warm` untimed rounds, then n timed ones, the calls taking turns within a round."""
    ms = {k: [] for k in calls}
    for i in range(warm + n):
        for k, fn in calls.items():
            _, t = timed(fn)
            if i >= warm:
                ms[k].append(t)
    return ms


def in_a_row(fn, n, warm):
    """[ms] * n of n calls in a row after `warm` untimed ones."""
    return [timed(fn)[1] for _ in range(warm + n)][warm:]


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": len(v)}


if mode == "reduce":
    S, n, warm = (arg + [65536, 20, 3][len(arg):])[:3]
    sim = make(S)
    sim.init_random(1, 0.5)
    alive = sim.alive_count()
    calls = {"density_32": lambda: sim.density(32), "density_1024": lambda: sim.density(1024),
             "density_33": lambda: sim.density(33)}
    checks = {k: int(fn().sum()) == alive for k, fn in calls.items()}
    ms = {k: in_a_row(fn, n, warm) for k, fn in calls.items()}
    ms["alive_count"] = in_a_row(sim.alive_count, n, warm)
    if S <= 32768:
        del sim
        u8 = make(S, "u8")
        assert u8.describe()["u8_compute"] == "bits"
        u8.init_random(1, 0.5)
        u8.advance(12)  # the bit image is the state now
        ms["u8_bits_32"] = in_a_row(lambda: u8.density(32), n, warm)
        checks["u8_bits_32"] = int(u8.density(32).sum()) == u8.alive_count()
    word_bytes = S * S / 8
    for k, v in ms.items():
        rec = {"mode": "reduce", "call": k, "size": S, **stats(v)}
        rec["GB_per_s"] = word_bytes / (rec["median_ms"] * 1e-3) / 1e9
        rec["vs_alive_count"] = rec["median_ms"] / statistics.median(ms["alive_count"])
        rec["vs_density_32"] = rec["median_ms"] / statistics.median(ms["density_32"])
        if k in checks:
            rec["sum_equals_alive_count"] = checks[k]
        print(json.dumps(rec), flush=True)

elif mode == "window":
    S, n, warm = (arg + [65536, 20, 3][len(arg):])[:3]
    sim = make(S)
    sim.init_random(1, 0.5)
    x, y = S // 2 - 100, S // 2 - 100  # off the word grid
    stamp = np.asarray(sim.window(x, y, 256, 256))
    assert (sim.native_engine.store_rows(y, 256)[:, x:x + 256] == stamp).all()
    calls = {"window_256": lambda: sim.window(x, y, 256, 256), "place_256": lambda: sim.place(stamp, x, y),
             "store_rows_256": lambda: sim.native_engine.store_rows(y, 256)}
    for k, v in take_turns(calls, n, warm).items():
        rec = {"mode": "window", "call": k, "size": S, **stats(v)}
        rec.update({"median_us": rec.pop("median_ms") * 1e3, "min_us": rec.pop("min_ms") * 1e3,
                    "max_us": rec.pop("max_ms") * 1e3})
        print(json.dumps(rec), flush=True)

elif mode == "frames":
    S, chunks, K, block, rounds = (arg + [32768, 20, 1000, 32, 2][len(arg):])[:5]
    for rnd in range(rounds):
        for with_maps in (False, True):
            sim = make(S)
            sim.init_random(1, 0.5)
            per_chunk, total = [], 0.0
            for c in range(chunks):
                _, t_adv = timed(lambda: sim.advance(K))
                rec = {"advance_ms": t_adv}
                if with_maps:
                    d0 = sim.describe()
                    drift = sim.native_engine.drift
                    m, t_map = timed(lambda: sim.density(block))
                    d1 = sim.describe()
                    rec.update({"map_ms": t_map, "quiet_mode": d1["quiet_mode"], "drift_before": drift,
                                "replayed_tail": d1["tail_replays"] - d0["tail_replays"], "population": int(m.sum())})
                    total += t_map
                total += t_adv
                per_chunk.append(rec)
            print(json.dumps({"mode": "frames", "size": S, "chunks": chunks, "K": K, "block": block, "round": rnd,
                              "maps": with_maps, "total_ms": total, "per_chunk": per_chunk}), flush=True)
            del sim
else:
    raise SystemExit(__doc__)
