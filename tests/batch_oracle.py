"""The definition of a batch run in NumPy (a helper, not a test module).

It uses no project code: ``rng_cell`` is re-implemented on uint64, a
generation is a roll / pad neighbour count over ``(B, H, W)``, and the stop
test follows the snapshot schedule of ``simulate_batch``:

* with ``max_period = P`` the state is saved at generations 0, P, 2P, ...;
* after computing generation ``t >= 1`` it is compared with the snapshot of
  generation ``s = P * floor((t - 1) / P)`` (at ``t = s + P`` before the new
  snapshot is taken); on equality the universe stops with ``generations = t``,
  ``period = t - s``, ``stop`` = extinction (2) where the grid is empty, else
  cycle (1), and its grid is frozen;
* a universe still running after ``max_gens`` reports ``generations =
  max_gens``, ``period = 0``, ``stop`` = limit (0).
"""
from __future__ import annotations

import math

import numpy as np

LIMIT, CYCLE, EXTINCTION = 0, 1, 2
STOP_NAMES = ("limit", "cycle", "extinction")

RULES = {"life": "B3/S23", "highlife": "B36/S23", "daynight": "B3678/S34678", "seeds": "B2/S",
         "replicator": "B1357/S1357", "lwod": "B3/S012345678", "34life": "B34/S34"}


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def density_thresh(d: float) -> int:
    if d <= 0:
        return 0
    if d >= 1:
        return 1 << 24
    return int(d * float(1 << 24) + 0.5)


def random_soups(W: int, H: int, seed: int, density: float, B: int) -> np.ndarray:
    """(B, H, W): universe b is the grid of seed + b (cell = hash(seed, row, col) < density)."""
    with np.errstate(over="ignore"):
        seeds = (np.arange(B, dtype=np.uint64) + np.uint64(seed & (2**64 - 1)))[:, None, None]
        rows = (np.arange(H, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03))[None, :, None]
        cols = (np.arange(W, dtype=np.uint64) * np.uint64(0xABC98388FB8FAC03))[None, None, :]
        k = seeds ^ rows ^ cols
    return ((_splitmix64(k) >> np.uint64(40)) < np.uint64(density_thresh(density))).astype(np.uint8)


def parse_rule(rule: str) -> tuple[set[int], set[int]]:
    text = RULES.get(rule.lower(), rule).upper().replace("/", "")
    b, s = text[1:].split("S")
    return {int(ch) for ch in b}, {int(ch) for ch in s}


def step(g: np.ndarray, rule: str = "B3/S23", boundary: str = "torus") -> np.ndarray:
    """One generation of every universe of g (B, H, W)."""
    birth, survive = parse_rule(rule)
    g = g.astype(np.uint8)
    if boundary == "torus":
        n = sum(np.roll(np.roll(g, dy, 1), dx, 2) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    else:
        H, W = g.shape[1:]
        p = np.pad(g, ((0, 0), (1, 1), (1, 1)))
        n = sum(p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if (dy, dx) != (0, 0))
    born = np.isin(n, sorted(birth)) & (g == 0)
    stay = np.isin(n, sorted(survive)) & (g == 1)
    return (born | stay).astype(np.uint8)


def run(grids: np.ndarray, max_gens: int, max_period: int = 64, rule: str = "B3/S23", boundary: str = "torus"):
    """(generations, period, stop, population, final grids) of the batch."""
    g = np.array(grids, dtype=np.uint8)
    B = g.shape[0]
    gens = np.full(B, max_gens, dtype=np.int32)
    period = np.zeros(B, dtype=np.int32)
    active = np.ones(B, dtype=bool)
    snap, s = g.copy(), 0
    for t in range(1, max_gens + 1):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        g[idx] = step(g[idx], rule, boundary)
        same = (g[idx] == snap[idx]).all(axis=(1, 2))
        stopped = idx[same]
        gens[stopped] = t
        period[stopped] = t - s
        active[stopped] = False
        if t - s == max_period:
            snap, s = g.copy(), t
    pop = g.sum(axis=(1, 2)).astype(np.int32)
    stop = np.where(period == 0, LIMIT, np.where(pop == 0, EXTINCTION, CYCLE)).astype(np.uint8)
    return gens, period, stop, pop, g


def counts(stop: np.ndarray) -> dict[str, int]:
    return {name: int((np.asarray(stop) == code).sum()) for code, name in enumerate(STOP_NAMES)}


def place(W: int, H: int, rows: list[str], y: int, x: int) -> np.ndarray:
    """An H x W grid with the pattern's first cell at row y, column x (wrapping)."""
    g = np.zeros((H, W), dtype=np.uint8)
    for i, line in enumerate(rows):
        for j, ch in enumerate(line):
            if ch == "O":
                g[(y + i) % H, (x + j) % W] = 1
    return g


BLOCK = ["OO", "OO"]
BLINKER = ["OOO"]
GLIDER = [".O.", "..O", "OOO"]  # moves one cell down and right every 4 generations

SHAPES = [(W, H) for W in (32, 64) for H in (8, 16, 32, 64)]  # (W, H)


def glider_period(W: int, H: int) -> int:
    return 4 * math.lcm(W, H)


# The random batches every engine is compared on:
# (rule, W, H, boundary, B, density, max_gens, P) -> the stop counts and periods
# the oracle gives (seeds 1..B).
RANDOM_TABLE = [
    ("life", 32, 16, "torus", 64, 0.4, 1024, 64),
    ("life", 64, 8, "torus", 64, 0.4, 1024, 64),
    ("life", 32, 32, "dead", 32, 0.4, 2048, 16),
    ("daynight", 32, 32, "torus", 32, 0.4, 512, 64),
    ("highlife", 64, 16, "torus", 32, 0.4, 1024, 64),
    ("replicator", 32, 8, "torus", 32, 0.3, 512, 64),
]
