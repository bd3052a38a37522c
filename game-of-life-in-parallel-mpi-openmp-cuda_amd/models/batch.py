"""Batched small universes: many soups per call, each run until it repeats.

The engine behind ``Simulation`` streams one huge grid; ``simulate_batch``
runs ``B`` independent universes of one small shape (32 or 64 cells wide, 8,
16, 32 or 64 high), one boundary and one rule - or, with ``rules=``, a rule per
universe - and reports for each when it stopped and into what
(csrc/include/gol/batch.hpp has the semantics, the hip engine's kernel is
csrc/kernels/life_batch.hip).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .._native import native
from .life import DEFAULT_BOUNDARY, DEFAULT_RULE, make_tuning, parse_rule

# Names of the ``BatchResult.stop`` codes.
BATCH_STOP = ("limit", "cycle", "extinction")

# A cluster record (csrc/include/gol/batch.hpp): ``height`` and ``width`` are
# the extents in rows and columns, ``spanning`` is ``SPANS_X`` (the cluster
# goes round the torus' columns) | ``SPANS_Y`` (round its rows).
CLUSTER_RECORD = np.dtype([("universe", np.int32), ("signature", np.uint64), ("cells", np.int32),
                           ("height", np.int16), ("width", np.int16), ("spanning", np.uint8)])
SPANS_X, SPANS_Y = 1, 2


def _records(arrays) -> np.ndarray:
    universe, signature, cells, height, width, spanning = arrays
    out = np.empty(len(universe), dtype=CLUSTER_RECORD)
    for name, a in zip(CLUSTER_RECORD.names, (universe, signature, cells, height, width, spanning)):
        out[name] = a
    return out


def cluster_name(signature: int) -> str:
    """The name of a cluster signature - block, beehive, loaf, boat, tub, ship,
    pond, blinker, toad, beacon, glider, traffic light and a few more, in every
    phase and symmetric image - or its 16 hex digits."""
    return native().cluster_name(int(signature))


def cluster_signature(cells) -> int:
    """The signature of the one cluster a 2-D array of 0/1 holds (any size,
    plane semantics); ``RuntimeError`` when it holds none or several."""
    g = np.asarray(cells)
    if g.ndim != 2:
        raise ValueError(f"cluster_signature: cells must be a 2-D array, got {g.ndim} dimensions")
    if ((g != 0) & (g != 1)).any():
        raise RuntimeError("cluster_signature: the array holds 0 (dead) and 1 (live) only")
    return int(native().cluster_signature(np.ascontiguousarray(g.astype(np.uint8))))


def cluster_table(records: np.ndarray) -> list[tuple]:
    """Records aggregated to ``(signature, name, cells, height, width,
    spanning, count)``, sorted by count descending, then signature."""
    keys = ["signature", "cells", "height", "width", "spanning"]
    if len(records) == 0:
        return []
    kinds, counts = np.unique(records[keys], return_counts=True)
    order = np.lexsort((kinds["signature"], -counts))
    return [(int(k["signature"]), cluster_name(int(k["signature"])), int(k["cells"]), int(k["height"]),
             int(k["width"]), int(k["spanning"]), int(n)) for k, n in zip(kinds[order], counts[order])]


def find_clusters(grids, boundary: str = DEFAULT_BOUNDARY, engine: str = "auto", *, threads: int = 0, device: int = 0,
                  tune=None) -> tuple[np.ndarray, np.ndarray]:
    """The cluster census of arbitrary 0/1 grids ``(B, H, W)`` of a batch
    shape: ``(clusters, records)``, the number of clusters of every universe
    (int32) and the ``CLUSTER_RECORD`` array, sorted by universe, then by each
    cluster's smallest cell in row-major order.  The hip engine runs
    csrc/kernels/life_batch_clusters.hip, the cpu engine a flood fill."""
    C = native()
    if engine == "auto":
        engine = "hip" if C.hip_available() else "cpu"
    if engine not in ("hip", "cpu"):
        raise ValueError(f"unknown engine {engine!r} (want hip, cpu or auto)")
    g = np.asarray(grids)
    if g.ndim != 3:
        raise ValueError(f"find_clusters: grids must be a (B, H, W) array, got {g.ndim} dimensions")
    if g.dtype != np.uint8:
        if ((g != 0) & (g != 1)).any():
            raise RuntimeError("batch: the input holds 0 (dead) and 1 (live) only")
        g = g.astype(np.uint8)
    r = C.find_clusters(np.ascontiguousarray(g), boundary=str(boundary), engine=engine, threads=int(threads),
                        device=int(device), tune=make_tuning(tune))
    return r[0], _records(r[1:7])


@dataclasses.dataclass
class BatchResult:
    """Per-universe results (arrays of length B) of ``simulate_batch``.

    ``generations``: the generation the universe stopped at (``max_gens`` at
    the limit); ``period``: its minimal period where that is at most
    ``max_period`` (0 at the limit); ``stop``: a code into ``BATCH_STOP``;
    ``population``: live cells of the final grid; ``grids``: the final grids
    ``(B, H, W)``, each at its universe's own stop generation, or ``None``.
    ``kernel_ms``: the hip engine's one kernel (the cpu engine's loop).
    ``rules``: the canonical B/S strings of a ``rules=`` run (else ``None``);
    ``soups``: its ``soups=K`` (else ``None``).  With ``clusters=True``:
    ``clusters``, the number of clusters of each final grid (int32),
    ``cluster_records``, their ``CLUSTER_RECORD`` array sorted by universe, and
    ``clusters_ms``, the census' two kernels (the cpu engine's wall time); else
    ``None``."""
    generations: np.ndarray
    period: np.ndarray
    stop: np.ndarray
    population: np.ndarray
    grids: np.ndarray | None
    kernel_ms: float
    variant: str
    rules: list[str] | None = None
    soups: int | None = None
    clusters: np.ndarray | None = None
    cluster_records: np.ndarray | None = None
    clusters_ms: float | None = None

    def cluster_table(self, stop=None) -> list[tuple]:
        """The kinds of clusters: ``(signature, name, cells, height, width,
        spanning, count)``, count descending, then signature.  ``stop``: a stop
        reason or several (names or codes), to count only those universes."""
        if self.cluster_records is None:
            raise ValueError("cluster_table: the batch was not run with clusters=True")
        recs = self.cluster_records
        if stop is not None:
            wanted = [stop] if isinstance(stop, (str, int, np.integer)) else list(stop)
            codes = [BATCH_STOP.index(w) if isinstance(w, str) else int(w) for w in wanted]
            recs = recs[np.isin(self.stop[recs["universe"]], codes)]
        return cluster_table(recs)

    def stop_names(self) -> list[str]:
        return [BATCH_STOP[int(c)] for c in self.stop]

    def counts(self) -> dict[str, int]:
        """Universes per stop reason."""
        return {name: int((self.stop == code).sum()) for code, name in enumerate(BATCH_STOP)}

    def per_rule(self) -> dict[str, np.ndarray]:
        """Summaries over the R rules of a ``rules=`` run (row r: universes
        ``r*K .. r*K + K - 1``, K = ``soups`` or 1): ``counts`` (R, 3) int64 in
        ``BATCH_STOP`` order, ``mean_generations`` float64, ``max_generations``
        int32, ``max_period`` int32, ``mean_population`` float64."""
        if self.rules is None:
            raise ValueError("per_rule: the batch was not run with rules=")
        R, K = len(self.rules), self.soups or 1
        stop = self.stop.reshape(R, K)
        gens, per, pop = (a.reshape(R, K) for a in (self.generations, self.period, self.population))
        return {"counts": np.stack([(stop == code).sum(axis=1) for code in range(len(BATCH_STOP))], axis=1).astype(np.int64),
                "mean_generations": gens.sum(axis=1, dtype=np.int64) / K,
                "max_generations": gens.max(axis=1).astype(np.int32),
                "max_period": per.max(axis=1).astype(np.int32),
                "mean_population": pop.sum(axis=1, dtype=np.int64) / K}


def life_like_rules() -> list[str]:
    """The 131,072 Life-like rules without B0 as canonical B/S strings, in a
    fixed order: rule ``i`` has birth mask ``(i & 0xFF) << 1`` (bit n: born at
    n neighbours) and survive mask ``i >> 8``.  B1/S is index 1, B3/S23 is
    index ``(0b1100 << 8) | 0b100`` = 3076."""
    births = ["B" + "".join(str(n) for n in range(1, 9) if (i >> (n - 1)) & 1) for i in range(256)]
    survives = ["/S" + "".join(str(n) for n in range(9) if (i >> n) & 1) for i in range(512)]
    return [b + s for s in survives for b in births]


def simulate_batch(grids=None, *, batch=None, shape=None, random=None, max_gens: int = 1024, max_period: int = 64,
                   rule: str = DEFAULT_RULE, boundary: str = DEFAULT_BOUNDARY, engine: str = "auto",
                   return_grids: bool = False, threads: int = 0, device: int = 0, tune=None, rules=None,
                   soups=None, clusters: bool = False) -> BatchResult:
    """Run ``B`` universes until each repeats or reaches ``max_gens``.

    Input: ``grids``, a ``(B, H, W)`` array of 0/1, or ``random=(seed,
    density)`` with ``batch=B`` and ``shape=(W, H)`` (the order of ``LifeConfig`` and
    ``random_grid``): universe ``b`` is then
    ``random_grid(W, H, seed + b, density)``, drawn on the device by the hip
    engine.  The state is saved at generations 0, P, 2P, ... (``P =
    max_period``); generation ``t`` is compared with the newest snapshot older
    than it, and on equality the universe stops with ``generations = t`` and
    ``period = t - s``: the exact minimal period whenever it is at most ``P``.

    ``rules``, a sequence of names or B/S strings, gives every universe a rule
    of its own; on the hip engine the rules are then data (a table on the
    device), so any rule without B0 runs there.  Alone it pairs rule ``b``
    with universe ``b``: ``len(rules) == B``, input as above.  With
    ``soups=K`` it is the cross product, ``B = R * K``: universe ``r*K + j``
    runs rule ``r`` on soup ``j``, and the input is ``grids (K, H, W)`` or
    ``random`` with seeds ``seed .. seed + K - 1`` (``batch``, if given, must
    be ``R * K``).  ``ValueError``: ``rules`` with a non-default ``rule``,
    ``soups`` without ``rules``, lengths that do not agree.

    Refused, naming the limit: widths other than 32 and 64, heights other
    than 8, 16, 32 and 64, ``B`` outside 1..2^24, ``max_period`` outside
    1..65536, ``max_gens`` outside 1..2^24, B0 rules, cells other than 0/1,
    ``grids`` together with ``random``; on the hip engine a rule that is not
    compiled for it (``hip_rules()``; ``rules=[...]`` takes any).
    ``engine="auto"``: hip where a device is available, else cpu (any rule).

    ``clusters=True`` adds the cluster census of the final grids
    (``BatchResult.clusters``, ``cluster_records``, ``cluster_table()``): live
    cells at Chebyshev distance at most 2 belong to one cluster.  A call whose
    records would exceed 2^28 is refused."""
    C = native()
    if grids is not None and (random is not None or batch is not None):
        raise ValueError("simulate_batch: give either grids or random=(seed, density) with batch=B, not both")
    canon = K = None
    extra = {}
    if rules is not None:
        if parse_rule(rule) != DEFAULT_RULE:
            raise ValueError(f"simulate_batch: give either rule={rule!r} or rules=[...], not both")
        canon = []
        for i, r in enumerate(rules):
            try:
                canon.append(parse_rule(r))
            except RuntimeError as e:
                raise RuntimeError(f"batch: rule {i} of the list: {e}") from None
        if not canon:
            raise ValueError("simulate_batch: rules is empty")
        R = len(canon)
        if soups is not None:
            K = int(soups)
            if K < 1:
                raise ValueError(f"simulate_batch: soups={K}: must be at least 1")
        form = f"{R} rules" if K is None else f"{R} rules x soups={K}"
        if grids is not None and np.ndim(grids) == 3:
            given, want = int(np.shape(grids)[0]), R if K is None else K
            if given != want:
                raise ValueError(f"simulate_batch: {form} take grids ({want}, H, W), got {given} grids")
        elif batch is not None and int(batch) != R * (K or 1):
            raise ValueError(f"simulate_batch: {form} make batch={R * (K or 1)}, got batch={int(batch)}")
        batch = None if grids is not None else R * (K or 1)
        extra = dict(rules=canon, soups=K or 1, share_soups=K is not None)
    elif soups is not None:
        raise ValueError("simulate_batch: soups=K goes with rules=[...]")
    if engine == "auto":
        engine = "hip" if C.hip_available() else "cpu"
    if engine not in ("hip", "cpu"):
        raise ValueError(f"unknown engine {engine!r} (want hip, cpu or auto)")
    common = dict(max_gens=int(max_gens), max_period=int(max_period), rule=parse_rule(rule), boundary=str(boundary),
                  engine=engine, return_grids=bool(return_grids), threads=int(threads), device=int(device),
                  tune=make_tuning(tune))
    if clusters:
        common["clusters"] = True
    if grids is not None:
        g = np.asarray(grids)
        if g.ndim != 3:
            raise ValueError(f"simulate_batch: grids must be a (B, H, W) array, got {g.ndim} dimensions")
        if shape is not None and tuple(shape) != (g.shape[2], g.shape[1]):
            raise ValueError(f"simulate_batch: shape={tuple(shape)} (W, H) is not the grids' {(g.shape[2], g.shape[1])}")
        if g.dtype != np.uint8:
            if ((g != 0) & (g != 1)).any():
                raise RuntimeError("batch: the input holds 0 (dead) and 1 (live) only")
            g = g.astype(np.uint8)
        r = C.simulate_batch(np.ascontiguousarray(g), **common, **extra)
    else:
        if random is None or batch is None or shape is None:
            raise ValueError("simulate_batch: without grids, give batch=B, shape=(W, H) and random=(seed, density)")
        seed, density = random
        W, H = shape
        r = C.simulate_batch(None, batch=int(batch), W=int(W), H=int(H), seed=int(seed), density=float(density),
                             **common, **extra)
    census = {}
    if clusters:
        c = r[7]
        census = dict(clusters=c[0], cluster_records=_records(c[1:7]), clusters_ms=float(c[7]))
    return BatchResult(*r[:7], rules=canon, soups=K, **census)
