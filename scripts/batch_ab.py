#!/usr/bin/env python3
"""Batched universes against the loop they replace (docs/PERFORMANCE.md "Batched universes").

    python scripts/batch_ab.py batch [--out FILE]   # simulate_batch: 65536 soups of 64 x 64 per launch
    python scripts/batch_ab.py loop [--out FILE]    # the same soups, 256 of them, one Simulation.find_cycle each

`batch` reports kernel_ms of 5 warm calls (median), universes/s and
cell-updates/s (4096 x the sum of `generations` over the kernel time) for the
default vertical move and for ds_bpermute, the median for three smaller
shapes, and compares the first 2048 universes with the cpu engine.  `loop` needs nothing of this change: run it
on the parent commit's build for the comparison.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402

import gol_amd  # noqa: E402

SOUPS = dict(shape=(64, 64), random=(1, 0.5), max_gens=4096, max_period=64)


def batch() -> dict:
    out = {}
    for vm in ("auto", "bpermute"):
        kw = dict(batch=65536, engine="hip", tune={"batch_vmove": vm}, **SOUPS)
        r = gol_amd.simulate_batch(**kw)  # warm
        ms = []
        for _ in range(5):
            r = gol_amd.simulate_batch(**kw)
            ms.append(r.kernel_ms)
        med = statistics.median(ms)
        gens = int(r.generations.astype(np.int64).sum())
        out[vm] = dict(variant=r.variant, kernel_ms=ms, median_ms=med, universes_per_s=65536 / (med * 1e-3),
                       sum_generations=gens, cell_updates_per_s=gens * 4096 / (med * 1e-3), counts=r.counts(),
                       mean_generations=gens / 65536, max_generations=int(r.generations.max()))
    out["smaller"] = {}
    for W, H in ((32, 8), (32, 16), (64, 32)):  # density 0.4
        kw = dict(batch=65536, shape=(W, H), random=(1, 0.4), max_gens=4096, max_period=64, engine="hip")
        gol_amd.simulate_batch(**kw)
        runs = [gol_amd.simulate_batch(**kw) for _ in range(5)]
        out["smaller"][f"{W}x{H}"] = dict(variant=runs[-1].variant,
                                          median_ms=statistics.median(x.kernel_ms for x in runs),
                                          sum_generations=int(runs[-1].generations.astype(np.int64).sum()),
                                          counts=runs[-1].counts())
    cpu = gol_amd.simulate_batch(batch=2048, engine="cpu", **SOUPS)
    out["first_2048_equal_cpu_engine"] = bool(
        np.array_equal(cpu.generations, r.generations[:2048]) and np.array_equal(cpu.period, r.period[:2048])
        and np.array_equal(cpu.population, r.population[:2048]) and np.array_equal(cpu.stop, r.stop[:2048]))
    return out


def loop(n: int = 256) -> dict:
    from gol_amd import LifeConfig, Simulation  # noqa: PLC0415

    def run(count):
        find, res = 0.0, []
        t0 = time.perf_counter()
        for b in range(count):
            sim = Simulation(LifeConfig(64, 64, fingerprint=True), engine="hip")
            sim.init_random(1 + b, 0.5)
            t1 = time.perf_counter()
            c = sim.find_cycle(4096, max_period=64)
            find += time.perf_counter() - t1
            res.append((c.generation, c.period, c.stop_reason))
        return time.perf_counter() - t0, find, res

    run(8)  # warm: module load, code objects, allocator
    total, find, res = run(n)
    return dict(universes=n, total_s=total, find_cycle_s=find, universes_per_s_total=n / total,
                universes_per_s_find_cycle_only=n / find, first=res[:4], periods=sorted({r[1] for r in res}))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mode", choices=["batch", "loop"])
    ap.add_argument("--out", default=None, help="also write the record to this JSON file")
    a = ap.parse_args()
    rec = batch() if a.mode == "batch" else loop()
    print(json.dumps(rec))
    if a.out:
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
