"""Batched small universes: many soups per call, each run until it repeats.

The engine behind ``Simulation`` streams one huge grid; ``simulate_batch``
runs ``B`` independent universes of one small shape (32 or 64 cells wide, 8,
16, 32 or 64 high), one rule and one boundary, and reports for each when it
stopped and into what (csrc/include/gol/batch.hpp has the semantics, the hip
engine's kernel is csrc/kernels/life_batch.hip).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .._native import native
from .life import DEFAULT_BOUNDARY, DEFAULT_RULE, make_tuning, parse_rule

# Names of the ``BatchResult.stop`` codes.
BATCH_STOP = ("limit", "cycle", "extinction")


@dataclasses.dataclass
class BatchResult:
    """Per-universe results (arrays of length B) of ``simulate_batch``.

    ``generations``: the generation the universe stopped at (``max_gens`` at
    the limit); ``period``: its minimal period where that is at most
    ``max_period`` (0 at the limit); ``stop``: a code into ``BATCH_STOP``;
    ``population``: live cells of the final grid; ``grids``: the final grids
    ``(B, H, W)``, each at its universe's own stop generation, or ``None``.
    ``kernel_ms``: the hip engine's one kernel (the cpu engine's loop)."""
    generations: np.ndarray
    period: np.ndarray
    stop: np.ndarray
    population: np.ndarray
    grids: np.ndarray | None
    kernel_ms: float
    variant: str

    def stop_names(self) -> list[str]:
        return [BATCH_STOP[int(c)] for c in self.stop]

    def counts(self) -> dict[str, int]:
        """Universes per stop reason."""
        return {name: int((self.stop == code).sum()) for code, name in enumerate(BATCH_STOP)}


def simulate_batch(grids=None, *, batch=None, shape=None, random=None, max_gens: int = 1024, max_period: int = 64,
                   rule: str = DEFAULT_RULE, boundary: str = DEFAULT_BOUNDARY, engine: str = "auto",
                   return_grids: bool = False, threads: int = 0, device: int = 0, tune=None) -> BatchResult:
    """Run ``B`` universes until each repeats or reaches ``max_gens``.

    Input: ``grids``, a ``(B, H, W)`` array of 0/1, or ``random=(seed,
    density)`` with ``batch=B`` and ``shape=(W, H)`` (the order of ``LifeConfig`` and
    ``random_grid``): universe ``b`` is then
    ``random_grid(W, H, seed + b, density)``, drawn on the device by the hip
    engine.  The state is saved at generations 0, P, 2P, ... (``P =
    max_period``); generation ``t`` is compared with the newest snapshot older
    than it, and on equality the universe stops with ``generations = t`` and
    ``period = t - s``: the exact minimal period whenever it is at most ``P``.

    Refused, naming the limit: widths other than 32 and 64, heights other
    than 8, 16, 32 and 64, ``B`` outside 1..2^24, ``max_period`` outside
    1..65536, ``max_gens`` outside 1..2^24, B0 rules, cells other than 0/1,
    ``grids`` together with ``random``; on the hip engine a rule that is not
    compiled for it (``hip_rules()``).  ``engine="auto"``: hip where a device
    is available, else cpu (any rule)."""
    C = native()
    if grids is not None and (random is not None or batch is not None):
        raise ValueError("simulate_batch: give either grids or random=(seed, density) with batch=B, not both")
    if engine == "auto":
        engine = "hip" if C.hip_available() else "cpu"
    if engine not in ("hip", "cpu"):
        raise ValueError(f"unknown engine {engine!r} (want hip, cpu or auto)")
    common = dict(max_gens=int(max_gens), max_period=int(max_period), rule=parse_rule(rule), boundary=str(boundary),
                  engine=engine, return_grids=bool(return_grids), threads=int(threads), device=int(device),
                  tune=make_tuning(tune))
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
        r = C.simulate_batch(np.ascontiguousarray(g), **common)
    else:
        if random is None or batch is None or shape is None:
            raise ValueError("simulate_batch: without grids, give batch=B, shape=(W, H) and random=(seed, density)")
        seed, density = random
        W, H = shape
        r = C.simulate_batch(None, batch=int(batch), W=int(W), H=int(H), seed=int(seed), density=float(density),
                             **common)
    return BatchResult(*r)
