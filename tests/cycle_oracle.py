"""Oracles for the cycle-detection tests (a helper, not a test module).

* ``fingerprint``: the grid fingerprint, written in vectorised numpy from its
  definition and independent of the package's implementations:

      F = sum over y, j of word(y, j) * r(y) * A(j)   (mod 2^64)
      word(y, j): cells (y, 32j .. 32j + 31), cell 32j + b at bit b, 0 beyond W
      r(y) = fmix32(y) | 1, A(j) = splitmix64(j) | 1

* ``fingerprint_at``: the share of a word-aligned window at a global row and
  word, for grids that are known only as a few islands (tests/far_oracle.py).
* ``brute_cycle``: steps a grid with a caller-supplied step function, keeps
  every grid in a dict and returns (entry, period) of the first repeat.
* ``pattern_board``: the 96 x 48 torus of the tests: a T-tetromino (it becomes
  a traffic light, period 2), a pulsar (3), a pentadecathlon (15) and a block;
  it enters its cycle at generation 9 with period lcm(2, 3, 15) = 30.
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _row_keys(H: int, y0: int = 0) -> np.ndarray:
    """r(y) of rows y0 .. H - 1."""
    h = np.arange(y0, H, dtype=np.uint64)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h | np.uint64(1)


def _col_keys(n: int, j0: int = 0) -> np.ndarray:
    """A(j) of words j0 .. n - 1."""
    with np.errstate(over="ignore"):
        x = np.arange(j0, n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x | np.uint64(1)


def fingerprint(grid: np.ndarray) -> int:
    g = np.asarray(grid) != 0
    H, W = g.shape
    nw = (W + 31) // 32
    if W % 32:
        g = np.pad(g, ((0, 0), (0, nw * 32 - W)))
    # cell 32j + b at bit b of word j: little-endian bit order, then little-endian bytes
    words = np.packbits(g, axis=1, bitorder="little").view("<u4").astype(np.uint64)
    with np.errstate(over="ignore"):
        terms = words * _row_keys(H)[:, None] * _col_keys(nw)[None, :]
        return int(terms.sum(dtype=np.uint64))


def fingerprint_at(window: np.ndarray, y0: int, word0: int) -> int:
    """The share of a word-aligned window (its width a multiple of 32) whose
    first cell is global row y0, global word word0.  F is linear in the words,
    so a sparse grid's fingerprint is the sum of this over its islands."""
    g = np.asarray(window) != 0
    h, w = g.shape
    assert w % 32 == 0 and y0 >= 0 and word0 >= 0, (w, y0, word0)
    words = np.packbits(g, axis=1, bitorder="little").view("<u4").astype(np.uint64)
    with np.errstate(over="ignore"):
        terms = words * _row_keys(y0 + h, y0)[:, None] * _col_keys(word0 + w // 32, word0)[None, :]
        return int(terms.sum(dtype=np.uint64))


def series(grids) -> np.ndarray:
    return np.array([fingerprint(g) for g in grids], dtype=np.uint64)


def brute_cycle(grid: np.ndarray, step, limit: int):
    """(entry, period, grids) of the first repeat within `limit` generations, or
    (None, None, grids); grids[g] is generation g."""
    seen = {}
    grids = []
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    for t in range(limit + 1):
        key = g.tobytes()
        if key in seen:
            return seen[key], t - seen[key], grids
        seen[key] = t
        grids.append(g)
        g = step(g)
    return None, None, grids


PATTERNS = {
    "t_tetromino": ((5, 5), ["OOO", ".O."]),
    "pulsar": ((4, 30), ["..OOO...OOO..", ".............", "O....O.O....O", "O....O.O....O", "O....O.O....O",
                         "..OOO...OOO..", ".............", "..OOO...OOO..", "O....O.O....O", "O....O.O....O",
                         "O....O.O....O", ".............", "..OOO...OOO.."]),
    "pentadecathlon": ((28, 60), ["..O....O..", "OO.OOOO.OO", "..O....O.."]),
    "block": ((40, 10), ["OO", "OO"]),
}
BOARD_W, BOARD_H = 96, 48
BOARD_ENTRY, BOARD_PERIOD = 9, 30


def pattern_board(names=tuple(PATTERNS)) -> np.ndarray:
    g = np.zeros((BOARD_H, BOARD_W), dtype=np.uint8)
    for n in names:
        (r0, c0), rows = PATTERNS[n]
        for i, line in enumerate(rows):
            for j, ch in enumerate(line):
                g[r0 + i, c0 + j] = ch == "O"
    return g
