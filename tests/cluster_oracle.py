"""The definition of the cluster census in Python (a helper, not a test module).

It uses no project code.  All distances and coordinates follow the universe's
topology: the torus wraps on both axes, the bounded plane ("dead") does not.

1. Two live cells are linked when their Chebyshev distance is at most 2.
2. A cluster is a connected component of the live cells under that relation.
3. Clusters are ordered by their smallest cell in row-major order.
4. Per axis, with ``occ`` the occupied coordinates and ``n`` the size: on the
   plane the origin is ``min(occ)`` and the extent ``max - min + 1``; on the
   torus the origin is the occupied ``o`` with neither ``o - 1`` nor ``o - 2``
   (mod n) occupied and the extent ``1 + max((p - o) mod n)``; without such
   an ``o`` the cluster spans the axis, origin 0, extent n.
5. The signature is the grid fingerprint of the cluster translated to its
   origin: the sum over its cells ``(y, x)`` of ``2^(x % 32) * r(y) * A(x // 32)``
   modulo 2^64, ``r(y) = fmix32(y) | 1``, ``A(j) = splitmix64(j) | 1``.
6. A record is (universe, signature, cells, height, width, spanning), with
   spanning = 1 (the columns, x) | 2 (the rows, y).
"""
from __future__ import annotations

import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
SPANS_X, SPANS_Y = 1, 2

RECORD = np.dtype([("universe", np.int32), ("signature", np.uint64), ("cells", np.int32), ("height", np.int16),
                   ("width", np.int16), ("spanning", np.uint8)])


def row_key(y: int) -> int:
    h = y & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h | 1


def col_key(j: int) -> int:
    x = (j + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return (x ^ (x >> 31)) | 1


def fingerprint(cells) -> int:
    """Of an iterable of (y, x) live cells."""
    return sum((1 << (x % 32)) * row_key(y) * col_key(x // 32) for y, x in cells) & M64


def axis(occ: set, n: int, torus: bool) -> tuple[int, int, bool]:
    """(origin, extent, spans) of the occupied coordinates on an axis of n."""
    if not torus:
        return min(occ), max(occ) - min(occ) + 1, False
    starts = [o for o in sorted(occ) if (o - 1) % n not in occ and (o - 2) % n not in occ]
    assert len(starts) <= 1, (sorted(occ), n)
    if not starts:
        return 0, n, True
    o = starts[0]
    return o, 1 + max((p - o) % n for p in occ), False


def components(grid: np.ndarray, boundary: str) -> list[list[tuple[int, int]]]:
    """The clusters of one H x W grid, each a list of cells, in the order of item 3."""
    H, W = grid.shape
    torus = boundary == "torus"
    live = {(int(y), int(x)) for y, x in zip(*np.nonzero(grid))}
    out = []
    for start in sorted(live):
        if start not in live:
            continue
        live.discard(start)
        comp, todo = [start], [start]
        while todo:
            cy, cx = todo.pop()
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ny, nx = cy + dy, cx + dx
                    if torus:
                        ny, nx = ny % H, nx % W
                    if (ny, nx) in live:
                        live.discard((ny, nx))
                        comp.append((ny, nx))
                        todo.append((ny, nx))
        out.append(comp)
    return out


def describe(comp: list[tuple[int, int]], W: int, H: int, boundary: str) -> tuple[int, int, int, int, int]:
    """(signature, cells, height, width, spanning) of one cluster."""
    torus = boundary == "torus"
    y0, h, sy = axis({y for y, _ in comp}, H, torus)
    x0, w, sx = axis({x for _, x in comp}, W, torus)
    sig = fingerprint(((y - y0) % H, (x - x0) % W) for y, x in comp)
    return sig, len(comp), h, w, (SPANS_X if sx else 0) | (SPANS_Y if sy else 0)


def clusters(grid: np.ndarray, boundary: str = "torus") -> list[tuple[int, int, int, int, int]]:
    H, W = grid.shape
    return [describe(c, W, H, boundary) for c in components(np.asarray(grid), boundary)]


def records(grids: np.ndarray, boundary: str = "torus") -> tuple[np.ndarray, np.ndarray]:
    """(clusters per universe int32 (B,), records) of a (B, H, W) batch."""
    rows, counts = [], []
    for u, g in enumerate(np.asarray(grids)):
        cl = clusters(g, boundary)
        counts.append(len(cl))
        rows += [(u, *c) for c in cl]
    return np.array(counts, dtype=np.int32), np.array(rows, dtype=RECORD)


def signature(cells: np.ndarray) -> int:
    """Of a 2-D array holding exactly one cluster (plane semantics)."""
    cells = np.asarray(cells)
    cl = clusters(cells, "dead")
    assert len(cl) == 1, len(cl)
    return cl[0][0]


def table(recs: np.ndarray) -> list[tuple[int, int, int, int, int, int]]:
    """(signature, cells, height, width, spanning, count): count descending, then signature."""
    kinds: dict = {}
    for r in recs:
        k = (int(r["signature"]), int(r["cells"]), int(r["height"]), int(r["width"]), int(r["spanning"]))
        kinds[k] = kinds.get(k, 0) + 1
    return sorted(((*k, n) for k, n in kinds.items()), key=lambda t: (-t[5], t[0], t[1:5]))


def images(rows: list[str]) -> list[np.ndarray]:
    """The 8 symmetric images of a pattern given as lines of 'O' and '.'."""
    g = np.array([[ch == "O" for ch in line] for line in rows], dtype=np.uint8)
    out = []
    for t in (g, g.T):
        for fy in (t, t[::-1]):
            out += [fy, fy[:, ::-1]]
    return out


def life_phases(g: np.ndarray, period: int) -> list[np.ndarray]:
    """The pattern's `period` generations under B3/S23 on a plane with room around it."""
    g = np.pad(np.asarray(g, dtype=np.uint8), period + 2)
    out = []
    for _ in range(period):
        out.append(g)
        p = np.pad(g, 1)
        n = sum(p[1 + dy:1 + dy + g.shape[0], 1 + dx:1 + dx + g.shape[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if (dy, dx) != (0, 0))
        g = ((n == 3) | ((n == 2) & (g == 1))).astype(np.uint8)
    return out


NAMED = {  # name -> (period, pattern)
    "block": (1, ["OO", "OO"]),
    "beehive": (1, [".OO.", "O..O", ".OO."]),
    "loaf": (1, [".OO.", "O..O", ".O.O", "..O."]),
    "boat": (1, ["OO.", "O.O", ".O."]),
    "tub": (1, [".O.", "O.O", ".O."]),
    "ship": (1, ["OO.", "O.O", ".OO"]),
    "pond": (1, [".OO.", "O..O", "O..O", ".OO."]),
    "blinker": (2, ["OOO"]),
    "toad": (2, [".OOO", "OOO."]),
    "beacon": (2, ["OO..", "OO..", "..OO", "..OO"]),
    "glider": (4, [".O.", "..O", "OOO"]),
    "barge": (1, [".O..", "O.O.", ".O.O", "..O."]),
    "long boat": (1, ["OO..", "O.O.", ".O.O", "..O."]),
    "mango": (1, [".OO..", "O..O.", ".O..O", "..OO."]),
    "eater": (1, ["OO..", "O.O.", "..O.", "..OO"]),
    "traffic light": (2, ["..OOO..", ".......", "O.....O", "O.....O", "O.....O", ".......", "..OOO.."]),
}


def named_forms(name: str) -> list[np.ndarray]:
    """Every phase of every symmetric image of a named pattern."""
    period, rows = NAMED[name]
    return [ph for im in images(rows) for ph in life_phases(im, period)]


# ---- the grids every engine is compared on ------------------------------------
import functools  # noqa: E402

BLOCK = ["OO", "OO"]
BLINKER = ["OOO"]
GLIDER = [".O.", "..O", "OOO"]
PAIRS = [(0, 2), (0, 3), (2, 0), (3, 0), (2, 2), (3, 3), (2, -2), (3, -3)]  # (dy, dx): distance 2 links, 3 does not


def place(W: int, H: int, rows: list[str], y: int, x: int) -> np.ndarray:
    """An H x W grid with the pattern's first cell at row y, column x (wrapping)."""
    g = np.zeros((H, W), dtype=np.uint8)
    for i, line in enumerate(rows):
        for j, ch in enumerate(line):
            if ch == "O":
                g[(y + i) % H, (x + j) % W] = 1
    return g


def seam_positions(W: int, H: int) -> dict[str, tuple[int, int]]:
    """Where a pattern lies in the middle and across each seam: (y, x) of its first cell."""
    return {"middle": (H // 2 - 1, 10), "row seam": (H - 1, 10), "word seam": (H // 2 - 1, 31),
            "column seam": (H // 2 - 1, W - 1), "first column": (H // 2 - 1, 0), "corner": (H - 1, W - 1)}


def lattice(W: int, H: int, torus: bool) -> np.ndarray:
    """Single cells at pitch 3: floor(n / 3) a side where the axis wraps, ceil(n / 3) where it does not."""
    g = np.zeros((H, W), dtype=np.uint8)
    ny, nx = (H // 3, W // 3) if torus else (-(-H // 3), -(-W // 3))
    g[np.ix_(3 * np.arange(ny), 3 * np.arange(nx))] = 1
    return g


def serpentine(W: int, H: int) -> np.ndarray:
    """A one-cell-wide path: runs on rows 0, 3, 6, ... over columns 0 .. W - 4, joined at alternating ends."""
    g = np.zeros((H, W), dtype=np.uint8)
    runs = list(range(0, H - 3, 3))
    for k, y in enumerate(runs):
        g[y, :W - 3] = 1
        if k + 1 < len(runs):
            g[y:y + 3, W - 4 if k % 2 == 0 else 0] = 1
    return g


@functools.lru_cache(maxsize=None)
def case_grids(W: int, H: int) -> tuple[tuple[str, ...], np.ndarray]:
    """(labels, grids (n, H, W)): the cases of one shape, the same on both boundaries."""
    out: list[tuple[str, np.ndarray]] = []
    for name, rows in (("block", BLOCK), ("blinker", BLINKER), ("glider", GLIDER)):
        for where, (y, x) in seam_positions(W, H).items():
            out.append((f"{name} {where}", place(W, H, rows, y, x)))
    corners = np.zeros((H, W), dtype=np.uint8)
    corners[[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = 1
    out.append(("four corners", corners))
    for where, (y, x) in seam_positions(W, H).items():
        for dy, dx in PAIRS:
            g = np.zeros((H, W), dtype=np.uint8)
            g[y, x] = g[(y + dy) % H, (x + dx) % W] = 1
            out.append((f"pair {dy},{dx} {where}", g))
    for y in (0, 1):
        g = np.zeros((H, W), dtype=np.uint8)
        g[y, 5] = g[H - 1, 5] = 1
        out.append((f"rows {y} and last", g))
    full_row, full_col = np.zeros((H, W), dtype=np.uint8), np.zeros((H, W), dtype=np.uint8)
    full_row[2, :] = 1
    full_col[:, 3] = 1
    gap1, gap2 = full_row.copy(), full_row.copy()
    gap1[2, 7] = 0
    gap2[2, 7:9] = 0
    out += [("full row", full_row), ("full column", full_col), ("full grid", np.ones((H, W), dtype=np.uint8)),
            ("row gap 1", gap1), ("row gap 2", gap2), ("empty", np.zeros((H, W), dtype=np.uint8)),
            ("lattice torus", lattice(W, H, True)), ("lattice plane", lattice(W, H, False)),
            ("serpentine", serpentine(W, H))]
    return tuple(label for label, _ in out), np.stack([g for _, g in out])


@functools.lru_cache(maxsize=None)
def case_records(W: int, H: int, boundary: str) -> tuple[np.ndarray, np.ndarray]:
    """The oracle's (clusters, records) of case_grids(W, H); computed once, not to be modified."""
    counts, recs = records(case_grids(W, H)[1], boundary)
    counts.setflags(write=False)
    recs.setflags(write=False)
    return counts, recs


def of_case(W: int, H: int, boundary: str, label: str) -> np.ndarray:
    """The oracle's records of one case."""
    u = case_grids(W, H)[0].index(label)
    recs = case_records(W, H, boundary)[1]
    return recs[recs["universe"] == u]


@functools.lru_cache(maxsize=None)
def predication_batch(B: int) -> np.ndarray:
    """B universes of 32 x 8 whose neighbours in a wave differ: none, one and many clusters, full edge rows."""
    W, H = 32, 8
    rng = np.random.default_rng(12345 + B)
    edge = np.zeros((H, W), dtype=np.uint8)
    edge[[0, H - 1], :] = 1
    pool = [np.zeros((H, W), dtype=np.uint8), place(W, H, BLOCK, 3, 7), lattice(W, H, False), edge,
            np.ones((H, W), dtype=np.uint8), serpentine(W, H), place(W, H, GLIDER, H - 1, W - 1)]
    grids = []
    for b in range(B):
        k = b % (len(pool) + 2)
        grids.append(pool[k] if k < len(pool) else (rng.random((H, W)) < (0.1 if k == len(pool) else 0.35)).astype(np.uint8))
    return np.stack(grids)


@functools.lru_cache(maxsize=None)
def predication_records(B: int, boundary: str) -> tuple[np.ndarray, np.ndarray]:
    counts, recs = records(predication_batch(B), boundary)
    counts.setflags(write=False)
    recs.setflags(write=False)
    return counts, recs
