#!/usr/bin/env python3
"""A 32768^2 grid of still lifes only (2 x 2 blocks on a 16-cell lattice) under quiet_skip=1: after the first two
blocks every tile skips, so a launch's duration is the cost of the groups that all skip."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

from gol_amd import LifeConfig, Simulation  # noqa: E402

N = 32768
g = np.zeros((N, N), np.uint8)
for dy in (0, 1):
    for dx in (0, 1):
        g[4 + dy::16, 4 + dx::16] = 1
tune = {"quiet_skip": "1"}
for kv in sys.argv[1:]:
    k, v = kv.split("=")
    tune[k] = v
sim = Simulation(LifeConfig(N, N, gen_limit=10**9, layout="bits", tune=tune), engine="hip")
sim.load(g)
eng = sim.native_engine
for i in range(1, 11):
    eng.run_until(i * 1200)  # 100 blocks each
d = sim.describe()
print({k: d[k] for k in d if k.startswith("quiet")}, d["launch_paths"], flush=True)
alive = int(sim.tile().sum())
print("alive", alive, "expected", 4 * (N // 16) ** 2)
assert alive == 4 * (N // 16) ** 2
