"""Oracles for tiles whose buffers pass 2 GiB and 4 GiB (a helper, not a test
module; tests/test_far_gpu.py on the GPU, tests/test_far.py on the CPU engine).

No host can hold such a grid, and a whole-grid tensor oracle does not fit a GPU
beside the engine, so every expectation here is computed in NumPy on windows
of a few hundred cells a side, from the step of tests/batch_oracle.py:

* ``far_height`` / ``far_rows``: the smallest geometry whose tile buffer passes
  2^32 bytes by 64 MiB, and the owned rows ``y31`` / ``y32`` whose padded byte
  range holds offset 2^31 / 2^32.
* Phase 1, ``run_islands``: about six 48 x 40 soups placed on an empty grid,
  further apart than their light cones reach in n generations, so the grid
  after n generations is the sum of the islands evolved alone on a zero-padded
  window (``Sparse``): its windows, live-cell count, density map, census series
  and - the fingerprint is linear - fingerprint series.  The rows 2^31 / pitch
  and 2^32 / pitch above every island are empty, so a row offset truncated to
  31 or 32 bits lands where the density map shows it.
* Phase 2, ``run_soup``: a dense soup from the device's RNG.  Windows read
  before the run are the RNG's definition at their global coordinates; the
  same windows after n generations are the NumPy evolution of the "before"
  windows, n cells in from their edges; and the whole-grid counts agree with
  each other and, at generation 0, with the RNG's density.

* ``run_cycle_confirmation``: find_cycle's snapshot copy and exact comparison
  of a grid whose only live cells lie beyond ``y32``.

Rectangles are (x0, y0, w, h) in unwrapped coordinates: on the torus they may
start below 0 or end beyond W or H, and are read and written in up to four
in-grid pieces; on the bounded plane they are clipped to the grid, whose edge
is dead in the NumPy step as well.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

import batch_oracle
import cycle_oracle

SOUP_W, SOUP_H = 48, 40
WIN_W, WIN_H = 160, 64
FAR_W = 65536
FAR_BYTES = 2**32 + 2**26  # the least a far tile buffer holds
STRIP = 62 * 32            # cells of a column strip of the symmetric-window kernels (63 * 32: the adder window's)


def far_height(native, layout: str, W: int = FAR_W) -> int:
    """The smallest multiple of 1024 rows whose halo-free tile passes FAR_BYTES
    (any engine's tile has at least these rows and this pitch)."""
    lay = native.Layout.Bits if layout == "bits" else native.Layout.U8
    pitch = native.TileGeom.make(lay, 1024, W, 0, 0).pitch
    H = (FAR_BYTES // (1024 * pitch) + 1) * 1024
    assert native.TileGeom.make(lay, H, W, 0, 0).bytes() > FAR_BYTES >= native.TileGeom.make(lay, H - 1024, W, 0, 0).bytes()
    return H


@dataclasses.dataclass(frozen=True)
class Far:
    W: int
    H: int
    y31: int  # owned row whose padded bytes hold offset 2^31
    y32: int  # ... 2^32
    shifts: tuple = ()  # rows that 2^31 and 2^32 bytes are


def far_rows(geom, W: int, H: int) -> Far:
    """``geom``: the engine's storage tile (Simulation.native_engine.geom)."""
    assert (geom.W, geom.H) == (W, H), (geom.W, geom.H)
    assert geom.bytes() > FAR_BYTES, f"a tile of {geom.bytes()} bytes is no far tile"
    y31, y32 = 2**31 // geom.pitch - geom.Dv, 2**32 // geom.pitch - geom.Dv
    assert (geom.Dv + y31) * geom.pitch <= 2**31 < (geom.Dv + y31 + 1) * geom.pitch
    assert (geom.Dv + y32) * geom.pitch <= 2**32 < (geom.Dv + y32 + 1) * geom.pitch
    assert 0 < y31 < y32 < H - 2 * SOUP_H, (y31, y32, H)
    return Far(W, H, y31, y32, (2**31 // geom.pitch, 2**32 // geom.pitch))


def small_rows(W: int, H: int) -> Far:
    """The same procedure on a grid a host can hold: the two special rows at a third and two thirds."""
    return Far(W, H, H // 3, 2 * H // 3)


# ---- rectangles ----------------------------------------------------------------------------------

def _split(a0: int, n: int, N: int):
    """[a0, a0 + n) cut where it wraps: (in-grid start, offset in the range, length)."""
    a = a0
    while a < a0 + n:
        g = a % N
        ln = min(N - g, a0 + n - a)
        yield g, a - a0, ln
        a += ln


def pieces(rect, far: Far, boundary: str):
    """The in-grid pieces of a rectangle: (gx, gy, w, h, ox, oy), piece cell (0, 0) being global (gx, gy) and
    cell (ox, oy) of the rectangle.  Torus: up to four; plane: the rectangle must lie inside the grid."""
    x0, y0, w, h = rect
    if boundary != "torus":
        assert 0 <= x0 and x0 + w <= far.W and 0 <= y0 and y0 + h <= far.H, rect
        return [(x0, y0, w, h, 0, 0)]
    assert w <= far.W and h <= far.H
    return [(gx, gy, pw, ph, ox, oy) for gy, oy, ph in _split(y0, h, far.H) for gx, ox, pw in _split(x0, w, far.W)]


def grow(rect, n: int, far: Far, boundary: str):
    """The rectangle with n cells of light cone on every side (the plane: clipped to the grid)."""
    x0, y0, w, h = rect
    x0, y0, x1, y1 = x0 - n, y0 - n, x0 + w + n, y0 + h + n
    if boundary != "torus":
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, far.W), min(y1, far.H)
    return x0, y0, x1 - x0, y1 - y0


def read_rect(sim, rect, far: Far, boundary: str) -> np.ndarray:
    out = np.zeros((rect[3], rect[2]), np.uint8)
    for gx, gy, w, h, ox, oy in pieces(rect, far, boundary):
        out[oy:oy + h, ox:ox + w] = sim.window(gx, gy, w, h)
    return out


def evolve(g: np.ndarray, n: int, rule: str) -> list:
    """Generations 0 .. n of a window whose outside is dead (a grid edge, or out of the light cone's reach)."""
    gens = [np.asarray(g, np.uint8)]
    for _ in range(n):
        gens.append(batch_oracle.step(gens[-1][None], rule, "dead")[0])
    return gens


# ---- phase 1: islands ------------------------------------------------------------------------------

@dataclasses.dataclass
class Island:
    name: str
    x: int  # first cell, unwrapped (the torus corner island starts below 0)
    y: int
    soup: np.ndarray
    mode: str

    @property
    def rect(self):
        return self.x, self.y, SOUP_W, SOUP_H


def spots(far: Far, boundary: str, w: int, h: int):
    """Where islands (w x h = the soup) and windows go: (name, x, y).  The x of the far ones is no multiple of
    32 and straddles a seam of column strips: 3 * 1984 = 6 * 992 (symmetric-window strips, the packed and the
    byte LDS tiles), 1984 and 2016 (the first seam of either window) and W / 2 (a 1024-cell LDS tile's)."""
    W, H = far.W, far.H
    if boundary == "torus":
        out = [("corner", -(w // 2), -(h // 2))]  # rows H-1 -> 0, columns W-1 -> 0
    else:
        out = [("corner00", 0, 0), ("cornerWH", W - w, H - h)]
    x31 = (3 * STRIP if W >= 4 * STRIP else STRIP // 2) - w // 2 + 13
    out += [("y31", x31, far.y31 - h // 2),
            ("y32", STRIP + 32 - w + 7, far.y32 - h // 2),
            ("last", 5 * W // 8 + 7, H - h - 5),  # in the last 50 rows (islands) or so
            ("row300", 3 * W // 4 + 11, 300 if H > 4096 else H // 6),
            ("mid", W // 2 - w // 2 + 3, (far.y31 + far.y32) // 2)]
    return out


def islands(far: Far, boundary: str, seed: int = 11) -> list:
    rng = np.random.default_rng(seed)
    out = []
    for i, (name, x, y) in enumerate(spots(far, boundary, SOUP_W, SOUP_H)):
        soup = (rng.random((SOUP_H, SOUP_W)) < 0.5).astype(np.uint8)
        out.append(Island(name, x, y, soup, "or" if i % 2 else "copy"))
    return out


def _apart(a, b, far: Far, boundary: str) -> int:
    """Chebyshev distance of two rectangles' first cells (around the torus)."""
    dx, dy = abs(a[0] - b[0]), abs(a[1] - b[1])
    if boundary == "torus":
        dx, dy = min(dx, far.W - dx), min(dy, far.H - dy)
    return max(dx, dy)


def check_plan(isles, far: Far, n: int, boundary: str) -> None:
    """Islands more than 2n + 48 cells apart (their cones never meet), one of them beyond y32, and the rows
    2^31 / pitch and 2^32 / pitch above every island out of every cone."""
    for i, a in enumerate(isles):
        assert a.x % 32 != 0 or a.name.startswith("corner"), a.name
        for b in isles[i + 1:]:
            assert _apart(a.rect, b.rect, far, boundary) > 2 * n + SOUP_W, (a.name, b.name, n)
    assert any(a.y > far.y32 for a in isles) and any(a.y < far.y32 < a.y + SOUP_H for a in isles)
    assert any(a.y < far.y31 < a.y + SOUP_H for a in isles)
    for a in isles:
        for s in far.shifts:
            ghost = (a.x, a.y - s, SOUP_W, SOUP_H)
            for b in isles:
                cx, cy, cw, ch = grow(b.rect, n, far, "torus")
                assert not (ghost[0] < cx + cw and cx < ghost[0] + SOUP_W and ghost[1] < cy + ch and cy < ghost[1] + SOUP_H), \
                    (a.name, s, b.name)


class Sparse:
    """What the grid of the islands is at generations 0 .. n, island by island."""

    def __init__(self, isles, far: Far, n: int, rule: str = "B3/S23", boundary: str = "torus"):
        self.far, self.n, self.boundary, self.isles = far, n, boundary, isles
        self.rects, self.gens = [], []
        for a in isles:
            rect = grow(a.rect, n, far, boundary)
            g = np.zeros((rect[3], rect[2]), np.uint8)
            g[a.y - rect[1]:a.y - rect[1] + SOUP_H, a.x - rect[0]:a.x - rect[0] + SOUP_W] = a.soup
            self.rects.append(rect)
            self.gens.append(evolve(g, n, rule))

    def population(self) -> np.ndarray:
        return np.array([sum(int(g[t].sum()) for g in self.gens) for t in range(self.n + 1)], np.int64)

    def density(self, t: int, by: int, bx: int) -> np.ndarray:
        out = np.zeros((-(-self.far.H // by), -(-self.far.W // bx)), np.int64)
        for (x0, y0, _, _), g in zip(self.rects, self.gens):
            ys, xs = np.nonzero(g[t])
            np.add.at(out, (((ys + y0) % self.far.H) // by, ((xs + x0) % self.far.W) // bx), 1)
        return out

    def fingerprints(self) -> np.ndarray:
        out = []
        for t in range(self.n + 1):
            f = 0
            for rect, g in zip(self.rects, self.gens):
                for gx, gy, w, h, ox, oy in pieces(rect, self.far, self.boundary):
                    left = gx % 32
                    a = np.zeros((h, -(-(left + w) // 32) * 32), np.uint8)  # the piece on the global word grid
                    a[:, left:left + w] = g[t][oy:oy + h, ox:ox + w]
                    f += cycle_oracle.fingerprint_at(a, gy, gx // 32)
            out.append(f % 2**64)
        return np.array(out, np.uint64)

    def grid(self, t: int) -> np.ndarray:
        """The whole grid (small geometries only)."""
        out = np.zeros((self.far.H, self.far.W), np.uint8)
        for rect, g in zip(self.rects, self.gens):
            for gx, gy, w, h, ox, oy in pieces(rect, self.far, self.boundary):
                out[gy:gy + h, gx:gx + w] |= g[t][oy:oy + h, ox:ox + w]
        return out


def density_block(far: Far) -> tuple:
    """(by, bx) of the map that watches the whole buffer: about 64 x 16 blocks."""
    return -(-far.H // 64), max(32, far.W // 16)


def run_islands(sim, far: Far, n: int, rule: str = "B3/S23", boundary: str = "torus", census: bool = False,
                fingerprint: bool = False) -> Sparse:
    """Phase 1 on `sim` (any engine of this geometry, rule and boundary); returns the expectations it met."""
    isles = islands(far, boundary)
    check_plan(isles, far, n, boundary)
    sp = Sparse(isles, far, n, rule, boundary)
    pop, fps = sp.population(), sp.fingerprints()
    sim.init_random(1, 0.0)
    assert sim.alive_count() == 0
    for a in isles:
        for gx, gy, w, h, ox, oy in pieces(a.rect, far, boundary):
            sim.place(a.soup[oy:oy + h, ox:ox + w], gx, gy, mode=a.mode)
    assert sim.alive_count() == pop[0], (sim.alive_count(), pop[0])
    rep = sim.advance(n)
    assert rep.executed == n
    for a, rect, g in zip(isles, sp.rects, sp.gens):
        got = read_rect(sim, rect, far, boundary)
        assert (got == g[n]).all(), (a.name, rect, int((got != g[n]).sum()))
    assert sim.alive_count() == pop[n], (sim.alive_count(), pop[n])
    by, bx = density_block(far)
    d, want = sim.density((by, bx)), sp.density(n, by, bx)
    assert d.dtype == np.int64 and d.shape == want.shape
    assert (d == want).all(), ("blocks (row, column) that differ", np.argwhere(d != want)[:8].tolist())
    assert sim.fingerprint() == int(fps[n])  # the stand-alone kernel, on every engine
    if census:
        assert rep.population.tolist() == pop[1:].tolist()
    if fingerprint:
        assert rep.fingerprint.tolist() == fps[1:].tolist()
    return sp


def run_cycle_confirmation(sim, far: Far) -> None:
    """find_cycle's snapshot copy and exact comparison where only rows beyond y32 are alive: a blinker there,
    on a fingerprint engine with cycle_match_bits=0 (every period is a candidate, so the cells decide).  The
    comparison after one generation must see the blinker's cells differ - else period 1 is confirmed - and
    after two the snapshot must hold them as they were - else period 2 never is."""
    x, y = STRIP - 1, far.y32 + (far.H - far.y32) // 2
    sim.init_random(1, 0.0)
    sim.place(np.ones((1, 3), np.uint8), x, y)
    g0 = sim.generation
    r = sim.find_cycle(g0 + 40, 2, 4)
    assert (r.period, r.stop_reason, r.confirmations, r.false_candidates) == (2, "cycle", 1, 0), r
    assert r.generation == sim.generation == g0 + 6 and r.repeats_from == g0
    want = np.zeros((3, 3), np.uint8)
    want[1, :] = 1  # an even generation: as placed
    assert (sim.window(x, y - 1, 3, 3) == want).all() and sim.alive_count() == 3


# ---- phase 2: a dense soup --------------------------------------------------------------------------

def rng_rect(seed: int, density: float, rect, far: Far) -> np.ndarray:
    """The cells init_random(seed, density) gives the rectangle (wrapped), from the RNG's definition."""
    x0, y0, w, h = rect
    with np.errstate(over="ignore"):
        rows = ((np.arange(y0, y0 + h) % far.H).astype(np.uint64) * np.uint64(0xD1B54A32D192ED03))[:, None]
        cols = ((np.arange(x0, x0 + w) % far.W).astype(np.uint64) * np.uint64(0xABC98388FB8FAC03))[None, :]
        k = np.uint64(seed) ^ rows ^ cols
    return ((batch_oracle._splitmix64(k) >> np.uint64(40)) < np.uint64(batch_oracle.density_thresh(density))).astype(np.uint8)


def count_bound(density: float, cells: int) -> tuple:
    """(expected live cells, 6 sigma) of a soup of the RNG's own density."""
    p = batch_oracle.density_thresh(density) / 2**24
    return p * cells, 6.0 * math.sqrt(cells * p * (1.0 - p))


def windows(far: Far, boundary: str) -> list:
    """About eight WIN_H x WIN_W interiors: the islands' kinds of places, one at the right edge and one
    further down beyond y32."""
    W, H = far.W, far.H
    out = spots(far, boundary, WIN_W, WIN_H)
    out += [("right", W - WIN_W, far.y32 + (H - far.y32) // 3), ("deep", W // 3 + 5, far.y32 + (H - far.y32) // 2)]
    return [(name, (x, y, WIN_W, WIN_H)) for name, x, y in out]


def run_soup(sim, far: Far, n: int, rule: str = "B3/S23", boundary: str = "torus", census: bool = False,
             fingerprint: bool = False, seed: int = 5, density: float = 0.4) -> tuple:
    """Phase 2 on `sim`; returns the live cells at generation 0 and n."""
    sim.init_random(seed, density)
    wins = windows(far, boundary)
    assert any(r[1] > far.y32 for _, r in wins) and any(r[1] < far.y32 < r[1] + WIN_H for _, r in wins)
    before = {}
    for name, rect in wins:
        big = grow(rect, n, far, boundary)
        before[name] = read_rect(sim, big, far, boundary)
        assert (before[name] == rng_rect(seed, density, big, far)).all(), (name, big)
    band = sim.native_engine.store_rows(far.y32 - 1, 3)
    assert band.shape == (3, far.W) and (band == rng_rect(seed, density, (0, far.y32 - 1, far.W, 3), far)).all()
    by, bx = density_block(far)
    c0, d0 = sim.alive_count(), int(sim.density((by, bx)).sum())
    mean, six_sigma = count_bound(density, far.W * far.H)
    assert c0 == d0 and abs(c0 - mean) <= six_sigma, (c0, d0, mean, six_sigma)
    rep = sim.advance(n)
    assert rep.executed == n
    for name, rect in wins:
        big = grow(rect, n, far, boundary)
        want = evolve(before[name], n, rule)[n][rect[1] - big[1]:rect[1] - big[1] + WIN_H, rect[0] - big[0]:rect[0] - big[0] + WIN_W]
        got = read_rect(sim, rect, far, boundary)
        assert (got == want).all(), (name, rect, int((got != want).sum()))
        if name == "y32":
            band = sim.native_engine.store_rows(far.y32 - 1, 3)
            r = far.y32 - 1 - rect[1]
            assert (band[:, rect[0]:rect[0] + WIN_W] == want[r:r + 3]).all()
    c, d = sim.alive_count(), int(sim.density((by, bx)).sum())
    assert c == d, (c, d)
    if census:
        assert int(rep.population[-1]) == c, (int(rep.population[-1]), c)
    if fingerprint:
        assert int(rep.fingerprint[-1]) == sim.fingerprint()  # the fused series against the stand-alone kernel
    return c0, c
