#!/usr/bin/env python3
"""What a caller that reads the grid between chunks pays for the lazy tail
(tuning lazy_tail): the bench's soup (32768^2, seed 1, density 0.5) taken to
generation 10192, then 20 chunks of 1000 generations with run_until, once
untouched and once with store_rows(0, 1) after every chunk.  Prints the wall
time of the 20 chunks (reads included) and the engine's tail counters, for
comparing two trees.

    python scripts/lazy_tail_readers.py [TREE]    # TREE: a checkout holding gol_amd
"""
import os
import sys
import time

tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, tree)
import gol_amd  # noqa: E402

S, START, CHUNK, CHUNKS = 32768, 10192, 1000, 20
print(f"tree {tree}: module {gol_amd.native().__file__}", flush=True)
for reads in (False, True):
    sim = gol_amd.Simulation(gol_amd.LifeConfig(S, S, gen_limit=10**9, layout="bits", timing_barriers=False),
                             engine="hip")
    eng = sim.native_engine
    sim.init_random(1, 0.5)
    eng.run_until(START)
    sim.backend.synchronize()
    t0 = time.perf_counter()
    for _ in range(CHUNKS):
        eng.run_until(sim.generation + CHUNK)
        if reads:
            eng.store_rows(0, 1)
    sim.backend.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    d = sim.describe()
    print(f"{'store_rows(0, 1) after every chunk' if reads else 'no reads':36s} {ms:8.3f} ms for {CHUNKS} x {CHUNK} "
          f"generations ({ms / CHUNKS:.3f} per chunk)  overshoots {d.get('tail_overshoots', '-')} "
          f"replays {d.get('tail_replays', '-')}  launches {sum(d['launch_paths'].values())}", flush=True)
    del sim, eng
