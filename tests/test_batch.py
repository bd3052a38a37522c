"""Batched small universes (simulate_batch), CPU tier: the cpu engine and both
CLIs against the NumPy definition in tests/batch_oracle.py."""
from __future__ import annotations

import csv
import json
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import batch_oracle as bo
import gol_amd
from gol_amd import BATCH_STOP, random_grid, simulate_batch

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden" / "batch"
ENGINE = "cpu"


def check(res, want, what=""):
    """All four fields (and the grids, where returned) against the oracle's run() tuple."""
    gens, period, stop, pop, grids = want
    assert np.array_equal(res.generations, gens), (what, res.generations, gens)
    assert np.array_equal(res.period, period), (what, res.period, period)
    assert np.array_equal(res.stop, stop), (what, res.stop, stop)
    assert np.array_equal(res.population, pop), (what, res.population, pop)
    if res.grids is not None:
        assert res.grids.dtype == np.uint8 and np.array_equal(res.grids, grids), what
    for a in (res.generations, res.period, res.population):
        assert a.dtype == np.int32
    assert res.stop.dtype == np.uint8


def one(res):
    return int(res.generations[0]), int(res.period[0]), res.stop_names()[0], int(res.population[0])


_ORACLE = {}


def oracle_random(row):
    """The oracle's result of a RANDOM_TABLE row, computed once per session."""
    if row not in _ORACLE:
        rule, W, H, boundary, B, density, max_gens, P = row
        _ORACLE[row] = bo.run(bo.random_soups(W, H, 1, density, B), max_gens, P, rule, boundary)
    return _ORACLE[row]


# ---- seeding ----------------------------------------------------------------

def test_oracle_rng_is_random_grid():
    """The oracle's rng_cell against the package's: every count below rests on it."""
    for W, H in ((32, 8), (64, 64), (64, 16)):
        for seed, d in ((1, 0.5), (7, 0.3), (2**64 - 2, 0.4)):
            soups = bo.random_soups(W, H, seed, d, 3)
            for b in range(3):
                assert np.array_equal(soups[b], random_grid(W, H, (seed + b) % 2**64, d)), (W, H, seed, b)


def test_universe_b_is_random_grid_of_seed_plus_b():
    W, H, seed, d = 64, 16, 41, 0.37
    res = simulate_batch(batch=5, shape=(W, H), random=(seed, d), max_gens=1, max_period=1, engine=ENGINE,
                         return_grids=True)
    first = np.stack([random_grid(W, H, seed + b, d) for b in range(5)])
    # max_gens = 1: the final grid of a universe is generation 1 of its soup
    assert np.array_equal(res.grids, bo.step(first))
    given = simulate_batch(first, max_gens=300, engine=ENGINE, return_grids=True)
    drawn = simulate_batch(batch=5, shape=(W, H), random=(seed, d), max_gens=300, engine=ENGINE, return_grids=True)
    check(drawn, (given.generations, given.period, given.stop, given.population, given.grids))


# ---- known patterns ------------------------------------------------------------

@pytest.mark.parametrize("boundary", ["torus", "dead"])
@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_still_lifes_and_blinker(W, H, boundary):
    grids = np.stack([np.zeros((H, W), np.uint8), bo.place(W, H, bo.BLOCK, 2, 5), bo.place(W, H, bo.BLINKER, 3, 7),
                      bo.place(W, H, bo.BLOCK, H - 3, W - 3), bo.place(W, H, bo.BLINKER, H - 2, 29)])
    res = simulate_batch(grids, max_gens=50, boundary=boundary, engine=ENGINE, return_grids=True)
    assert [BATCH_STOP[c] for c in res.stop] == res.stop_names()
    got = list(zip(res.generations.tolist(), res.period.tolist(), res.stop_names(), res.population.tolist()))
    assert got == [(1, 1, "extinction", 0), (1, 1, "cycle", 4), (2, 2, "cycle", 3), (1, 1, "cycle", 4),
                   (2, 2, "cycle", 3)]
    check(res, bo.run(grids, 50, 64, "B3/S23", boundary))


@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_glider_round_trip_on_the_torus(W, H):
    """A glider returns to its place after 4 * lcm(W, H) generations: with
    max_period that large the snapshot of generation 0 recurs exactly then."""
    n = bo.glider_period(W, H)
    assert n == 4 * math.lcm(W, H) and {(64, 64): 256, (32, 8): 128}.get((W, H), n) == n
    g = bo.place(W, H, bo.GLIDER, 1, 1)[None]
    res = simulate_batch(g, max_gens=n + 10, max_period=n, engine=ENGINE, return_grids=True)
    assert one(res) == (n, n, "cycle", 5)
    assert np.array_equal(res.grids, g)


def crossing_glider():
    """64 x 64, a glider that starts at row 13 / column 29: in 300 generations
    it moves 75 cells down and right, across rows 15->16, 31->32, 63->0 and
    columns 31->32, 63->0."""
    return bo.place(64, 64, bo.GLIDER, 13, 29)[None]


def test_glider_crossing_every_seam_reaches_the_limit():
    g = crossing_glider()
    res = simulate_batch(g, max_gens=300, max_period=64, engine=ENGINE, return_grids=True)
    assert one(res) == (300, 0, "limit", 5)
    want = bo.run(g, 300, 64)
    live = np.argwhere(want[4][0])
    assert live[:, 0].min() < 32 and live[:, 1].min() < 48, live  # it has wrapped both ways
    check(res, want)
    full = simulate_batch(g, max_gens=300, max_period=256, engine=ENGINE)
    assert one(full) == (256, 256, "cycle", 5)


@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_glider_into_the_corner_of_the_plane_ends_as_a_block(W, H):
    g = bo.place(W, H, bo.GLIDER, H - 7, W - 7)[None]
    want = bo.run(g, 200, 64, "B3/S23", "dead")
    assert (int(want[1][0]), int(want[2][0]), int(want[3][0])) == (1, bo.CYCLE, 4)
    res = simulate_batch(g, max_gens=200, boundary="dead", engine=ENGINE, return_grids=True)
    assert one(res) == (int(want[0][0]), 1, "cycle", 4)
    check(res, want)


# ---- the stop test at the boundary of a snapshot window -------------------------

def test_stop_at_a_window_boundary():
    """A blinker with max_period = 2 stops at t = s + P = 2, where the compare
    comes before the new snapshot.  The T-tetromino becomes a traffic light
    (period 2) at generation 9; with P = 2 it first equals a snapshot at a
    multiple of P, and with P = 1 a period-2 oscillator never does."""
    W, H = 32, 16
    blinker = bo.place(W, H, bo.BLINKER, 4, 4)[None]
    assert one(simulate_batch(blinker, max_gens=20, max_period=2, engine=ENGINE)) == (2, 2, "cycle", 3)
    assert one(simulate_batch(blinker, max_gens=20, max_period=1, engine=ENGINE)) == (20, 0, "limit", 3)
    assert one(simulate_batch(blinker, max_gens=20, max_period=3, engine=ENGINE)) == (2, 2, "cycle", 3)
    t = bo.place(W, H, ["OOO", ".O."], 6, 12)[None]
    for P in (1, 2, 3, 4, 5, 64):
        want = bo.run(t, 100, P)
        res = simulate_batch(t, max_gens=100, max_period=P, engine=ENGINE, return_grids=True)
        check(res, want, f"P={P}")
        if P >= 2:
            assert int(res.period[0]) == 2 and int(res.stop[0]) == bo.CYCLE
    two = bo.run(t, 40, 2)
    assert int(two[0][0]) % 2 == 0  # it settles exactly at a multiple of P
    # max_gens on the very generation of the repeat: the repeat wins over the limit
    assert one(simulate_batch(blinker, max_gens=2, max_period=2, engine=ENGINE)) == (2, 2, "cycle", 3)
    assert one(simulate_batch(blinker, max_gens=1, max_period=2, engine=ENGINE)) == (1, 0, "limit", 3)


# ---- random batches --------------------------------------------------------------

# What the oracle gives for the rows of bo.RANDOM_TABLE (seeds 1..B): stop counts and periods.
RANDOM_EXPECT = [
    ({"limit": 1, "cycle": 61, "extinction": 2}, {0, 1, 2}),
    ({"limit": 0, "cycle": 64, "extinction": 0}, {1, 2, 6, 9}),
    ({"limit": 0, "cycle": 32, "extinction": 0}, {1, 2}),
    ({"limit": 10, "cycle": 16, "extinction": 6}, {0, 1, 2, 4, 16}),
    ({"limit": 1, "cycle": 31, "extinction": 0}, {0, 1, 2}),
    ({"limit": 0, "cycle": 0, "extinction": 32}, {1}),
]


@pytest.mark.parametrize("row,expect", list(zip(bo.RANDOM_TABLE, RANDOM_EXPECT)),
                         ids=[f"{r[0]}-{r[1]}x{r[2]}-{r[3]}" for r in bo.RANDOM_TABLE])
def test_random_batches(row, expect):
    rule, W, H, boundary, B, density, max_gens, P = row
    want = oracle_random(row)
    counts, periods = expect
    assert bo.counts(want[2]) == counts and set(want[1].tolist()) == periods
    if rule == "replicator":
        assert set(want[0].tolist()) == {65}
    if (rule, W, H) in (("life", 32, 16), ("daynight", 32, 32)):
        assert all(counts[k] > 0 for k in BATCH_STOP)  # every kind of stop is in the batch
    res = simulate_batch(batch=B, shape=(W, H), random=(1, density), max_gens=max_gens, max_period=P, rule=rule,
                         boundary=boundary, engine=ENGINE, return_grids=True)
    check(res, want)
    assert res.counts() == counts
    assert res.kernel_ms >= 0 and f"{W}x{H}" in res.variant


# ---- partial waves and freezing -----------------------------------------------------

@pytest.mark.parametrize("B", [1, 7, 9, 65])
def test_partial_waves_and_frozen_grids(B):
    """32 x 8: eight universes share a wave on the hip engine.  The final grid
    of each universe is the oracle's state at that universe's own stop
    generation, not at the batch's last generation."""
    W, H = 32, 8
    soups = bo.random_soups(W, H, 3, 0.35, B)
    want = bo.run(soups, 400, 16)
    res = simulate_batch(soups, max_gens=400, max_period=16, engine=ENGINE, return_grids=True)
    check(res, want)
    if B >= 7:
        assert len(set(want[0].tolist())) > 1  # they stop at different generations
    b = int(np.argmin(want[0]))
    g = soups[b:b + 1]
    for _ in range(int(want[0][b])):
        g = bo.step(g)
    assert np.array_equal(res.grids[b], g[0])
    quiet = simulate_batch(soups, max_gens=400, max_period=16, engine=ENGINE)
    assert quiet.grids is None
    check(quiet, want)


# ---- refusals --------------------------------------------------------------------------

@pytest.mark.parametrize("kw,names", [
    (dict(shape=(48, 16)), "width must be 32 or 64"),
    (dict(shape=(128, 16)), "width must be 32 or 64"),
    (dict(shape=(32, 12)), "height must be 8, 16, 32 or 64"),
    (dict(shape=(64, 128)), "height must be 8, 16, 32 or 64"),
    (dict(max_period=0), "2^16"),
    (dict(max_period=65537), "65536"),
    (dict(max_gens=0), "2^24"),
    (dict(max_gens=2**24 + 1), "16777216"),
    (dict(batch=0), "2^24"),
    (dict(batch=2**24 + 1), "16777216"),
    (dict(rule="B03/S23"), "B0"),
])
def test_refusals_name_the_limit(kw, names):
    args = dict(batch=2, shape=(32, 16), random=(1, 0.5), max_gens=10, max_period=4, engine=ENGINE)
    args.update(kw)
    with pytest.raises(RuntimeError, match=re.escape(names)):
        simulate_batch(**args)


def test_refused_inputs():
    g = np.zeros((2, 8, 32), np.uint8)
    g[1, 3, 4] = 2
    with pytest.raises(RuntimeError, match="0 .dead. and 1 .live. only"):
        simulate_batch(g, engine=ENGINE)
    with pytest.raises(RuntimeError, match="0 .dead. and 1 .live. only"):
        simulate_batch(g.astype(np.int64) * 128, engine=ENGINE)  # 256 would wrap to 0 as a byte
    ok = np.zeros((2, 8, 32), np.uint8)
    with pytest.raises(ValueError, match="either grids or random"):
        simulate_batch(ok, random=(1, 0.5), engine=ENGINE)
    with pytest.raises(ValueError, match="either grids or random"):
        simulate_batch(ok, batch=2, engine=ENGINE)
    with pytest.raises(ValueError, match="batch=B, shape=.W, H. and random"):
        simulate_batch(batch=2, random=(1, 0.5), engine=ENGINE)
    with pytest.raises(ValueError, match=r"\(B, H, W\)"):
        simulate_batch(ok[0], engine=ENGINE)
    with pytest.raises(RuntimeError, match="width must be 32 or 64"):
        simulate_batch(np.zeros((2, 32, 8), np.uint8), engine=ENGINE)  # (B, H, W), not (B, W, H)
    with pytest.raises(ValueError, match="engine"):
        simulate_batch(ok, engine="ref")
    assert gol_amd.BATCH_STOP == ("limit", "cycle", "extinction") == tuple(gol_amd.native().BATCH_STOP)


def test_the_cpu_engine_runs_any_rule():
    rule = "B35/S236"  # not in life_rules.def
    soups = bo.random_soups(32, 16, 5, 0.4, 6)
    check(simulate_batch(soups, max_gens=150, rule=rule, engine=ENGINE, return_grids=True), bo.run(soups, 150, 64, rule))


# ---- the CLIs ---------------------------------------------------------------------------

def cli(which):
    if which == "gol":
        return [str(REPO / "bin" / "gol")]
    return [sys.executable, "-m", "gol_amd"]


def run_cli(which, args, cwd):
    env = dict(os.environ, PYTHONPATH=str(REPO))
    return subprocess.run(cli(which) + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env,
                          cwd=cwd)


@pytest.mark.parametrize("which", ["gol", "python"])
def test_cli_batch(which, native, tmp_path):
    rule, W, H, boundary, B, density, max_gens, P = bo.RANDOM_TABLE[0]
    want = simulate_batch(batch=B, shape=(W, H), random=(1, density), max_gens=max_gens, max_period=P, engine=ENGINE)
    out, metrics = tmp_path / "b.csv", tmp_path / "m.json"
    r = run_cli(which, [W, H, "none", "--batch", B, "--random", f"1:{density}", "--gens", max_gens, "--max-period", P,
                        "--engine", ENGINE, "--batch-csv", out, "--metrics-json", metrics], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Batch: 64 universes: 1 limit, 61 cycle, 2 extinction; largest generations 1024\n"
    rows = list(csv.reader(out.read_text().splitlines()))
    assert rows[0] == ["universe", "seed", "generations", "stop", "period", "population"] and len(rows) == B + 1
    names = want.stop_names()
    for b, line in enumerate(rows[1:]):
        assert line == [str(b), str(1 + b), str(want.generations[b]), names[b], str(want.period[b]),
                        str(want.population[b])]
    rec = json.loads(metrics.read_text())
    assert rec["batch"] == B and rec["batch_variant"] == want.variant and rec["batch_kernel_ms"] >= 0
    assert (rec["limit"], rec["cycle"], rec["extinction"]) == (1, 61, 2)
    assert not list(tmp_path.glob("*.out"))  # no grid file


@pytest.mark.parametrize("which", ["gol", "python"])
def test_cli_batch_refusals(which, native, tmp_path):
    base = [32, 16, "none", "--batch", 4, "--random", "1", "--engine", ENGINE]
    for extra in (["--census", "c.csv"], ["--cycle", "8"], ["--output", "o.txt"], ["--density", "d.pgm"],
                  ["--window", "0,0,8,8:w.txt"], ["--place", "p.rle"], ["--checkpoint-every", "10"],
                  ["--decomp", "1x1"]):
        r = run_cli(which, base + extra, tmp_path)
        assert r.returncode != 0 and "--batch with " + extra[0] in r.stderr, (extra, r.stderr)
    r = run_cli(which, [32, 16, "--batch", 4, "--random", "1", "--engine", ENGINE], tmp_path)
    assert r.returncode != 0 and "input 'none'" in r.stderr
    r = run_cli(which, [32, 16, "none", "--batch", 4, "--engine", ENGINE], tmp_path)
    assert r.returncode != 0 and "--random" in r.stderr
    r = run_cli(which, [48, 16, "none", "--batch", 4, "--random", "1", "--engine", ENGINE], tmp_path)
    assert r.returncode != 0 and "width must be 32 or 64" in r.stderr
    r = run_cli(which, [32, 16, "--random", "1", "--engine", ENGINE, "--max-period", 8, "--output", "none"], tmp_path)
    assert r.returncode != 0 and "need --batch" in r.stderr
    if which == "gol":
        r = run_cli(which, base + ["--gpus", 2], tmp_path)
        assert r.returncode != 0 and "one device" in r.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("which", ["gol", "python"])
def test_cli_without_batch_prints_what_it_printed_before(which, native, tmp_path):
    """tests/golden/batch/stdout_<cli>.txt is the stdout of this run recorded
    before --batch existed, its one run-dependent field (the execution time in
    milliseconds) replaced by <ms>."""
    r = run_cli(which, [64, 48, "--random", "7:0.4", "--engine", "cpu", "--gens", 120, "--output", "none"], tmp_path)
    assert r.returncode == 0, r.stderr
    got = re.sub(r"(?<=Execution time:\t)[0-9.]+(?= msecs)", "<ms>", r.stdout)
    assert got.encode() == (GOLDEN / f"stdout_{which}.txt").read_bytes()
