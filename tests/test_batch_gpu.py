"""Batched small universes on the MI355X: the hip engine (life_batch.hip)
against the NumPy definition (tests/batch_oracle.py) and the cpu engine.
Every supported (W, H) runs on both boundaries: that reaches every vertical
move (wave rotate, row rotate, ds_bpermute) and both word counts."""
from __future__ import annotations

import csv
import subprocess

import numpy as np
import pytest

import batch_oracle as bo
from gol_amd import random_grid, simulate_batch
from test_batch import RANDOM_EXPECT, check, crossing_glider, one, oracle_random

pytestmark = pytest.mark.gpu

ENGINE = "hip"


def against_cpu(**kw):
    hip = simulate_batch(engine="hip", return_grids=True, **kw)
    cpu = simulate_batch(engine="cpu", return_grids=True, **kw)
    check(hip, (cpu.generations, cpu.period, cpu.stop, cpu.population, cpu.grids))
    return hip


@pytest.mark.parametrize("boundary", ["torus", "dead"])
@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_known_patterns(gpu, W, H, boundary):
    """Still lifes, blinkers and gliders of every shape in one batch; patterns
    sit on the first and last rows and columns, where a universe meets the
    next one of its wave (or wraps)."""
    n = bo.glider_period(W, H)
    grids = np.stack([np.zeros((H, W), np.uint8), bo.place(W, H, bo.BLOCK, 2, 5), bo.place(W, H, bo.BLINKER, 3, 7),
                      bo.place(W, H, bo.BLOCK, H - 1, W - 1), bo.place(W, H, bo.BLINKER, H - 1, 30),
                      bo.place(W, H, bo.BLINKER, 0, 3), bo.place(W, H, bo.GLIDER, 1, 1),
                      bo.place(W, H, bo.GLIDER, H - 7, W - 7), bo.place(W, H, bo.BLOCK, 0, 31)])
    want = bo.run(grids, n + 10, n, "B3/S23", boundary)
    res = simulate_batch(grids, max_gens=n + 10, max_period=n, boundary=boundary, engine=ENGINE, return_grids=True)
    check(res, want)
    got = list(zip(res.generations.tolist(), res.period.tolist(), res.stop_names(), res.population.tolist()))
    assert got[:3] == [(1, 1, "extinction", 0), (1, 1, "cycle", 4), (2, 2, "cycle", 3)]
    if boundary == "torus":
        assert got[3] == (1, 1, "cycle", 4) and got[4] == got[5] == (2, 2, "cycle", 3)
        assert got[6] == got[7] == (n, n, "cycle", 5)
    else:
        assert got[7][1:] == (1, "cycle", 4)  # the glider in the corner ends as a block


def test_glider_across_every_seam(gpu):
    """64 x 64: rows 63->0 (the wave rotate's wrap), 31->32, 15->16 and columns 31->32, 63->0."""
    g = crossing_glider()
    res = simulate_batch(g, max_gens=300, max_period=64, engine=ENGINE, return_grids=True)
    assert one(res) == (300, 0, "limit", 5)
    check(res, bo.run(g, 300, 64))
    assert one(simulate_batch(g, max_gens=300, max_period=256, engine=ENGINE)) == (256, 256, "cycle", 5)
    # the same through ds_bpermute
    check(simulate_batch(g, max_gens=300, max_period=64, engine=ENGINE, return_grids=True,
                         tune={"batch_vmove": "bpermute"}), bo.run(g, 300, 64))


def test_stop_at_a_window_boundary(gpu):
    W, H = 32, 16
    blinker = bo.place(W, H, bo.BLINKER, 4, 4)[None]
    assert one(simulate_batch(blinker, max_gens=20, max_period=2, engine=ENGINE)) == (2, 2, "cycle", 3)
    assert one(simulate_batch(blinker, max_gens=20, max_period=1, engine=ENGINE)) == (20, 0, "limit", 3)
    assert one(simulate_batch(blinker, max_gens=2, max_period=2, engine=ENGINE)) == (2, 2, "cycle", 3)
    assert one(simulate_batch(blinker, max_gens=1, max_period=2, engine=ENGINE)) == (1, 0, "limit", 3)
    t = bo.place(W, H, ["OOO", ".O."], 6, 12)[None]
    for P in (1, 2, 3, 4, 5, 64):
        check(simulate_batch(t, max_gens=100, max_period=P, engine=ENGINE, return_grids=True), bo.run(t, 100, P),
              f"P={P}")


@pytest.mark.parametrize("row,expect", list(zip(bo.RANDOM_TABLE, RANDOM_EXPECT)),
                         ids=[f"{r[0]}-{r[1]}x{r[2]}-{r[3]}" for r in bo.RANDOM_TABLE])
def test_random_batches(gpu, row, expect):
    rule, W, H, boundary, B, density, max_gens, P = row
    want = oracle_random(row)
    assert bo.counts(want[2]) == expect[0] and set(want[1].tolist()) == expect[1]
    res = simulate_batch(batch=B, shape=(W, H), random=(1, density), max_gens=max_gens, max_period=P, rule=rule,
                         boundary=boundary, engine=ENGINE, return_grids=True)
    check(res, want)
    assert res.counts() == expect[0]
    assert res.kernel_ms > 0 and f"{W}x{H}" in res.variant and f"{64 // H}/wave" in res.variant


@pytest.mark.parametrize("boundary,lo,hi", [("torus", 514, 3458), ("dead", 194, 1730)])
def test_soups_64x64(gpu, boundary, lo, hi):
    """32 soups of 64 x 64, one per wave, run to their period-2 ends."""
    res = against_cpu(batch=32, shape=(64, 64), random=(1, 0.5), max_gens=4096, max_period=64, boundary=boundary)
    assert res.counts() == {"limit": 0, "cycle": 32, "extinction": 0} and set(res.period.tolist()) == {2}
    assert (int(res.generations.min()), int(res.generations.max())) == (lo, hi)
    assert "dpp wave_ror/rol" in res.variant


def test_every_compiled_rule_and_a_refused_one(gpu):
    rules = list(gpu.hip_rules())
    assert len(rules) == 7 and rules[0] == "B3/S23"
    for rule in rules:
        for shape in ((32, 16), (64, 32)):
            res = against_cpu(batch=16, shape=shape, random=(1, 0.4), max_gens=300, max_period=64, rule=rule)
            assert rule in res.variant
    with pytest.raises(RuntimeError, match="not compiled for the HIP engine") as e:
        simulate_batch(batch=2, shape=(32, 16), random=(1, 0.4), rule="B35/S236", engine=ENGINE)
    for rule in rules:
        assert rule in str(e.value)


@pytest.mark.parametrize("B", [1, 7, 9, 1000])
def test_partial_waves(gpu, B):
    """32 x 8: eight universes per wave; B = 64/H - 1, 64/H + 1 and a
    thousand, with and without the grids."""
    soups = bo.random_soups(32, 8, 3, 0.35, B)
    cpu = simulate_batch(soups, max_gens=400, max_period=16, engine="cpu", return_grids=True)
    want = (cpu.generations, cpu.period, cpu.stop, cpu.population, cpu.grids)
    if B <= 9:
        check(cpu, bo.run(soups, 400, 16))
    res = simulate_batch(soups, max_gens=400, max_period=16, engine=ENGINE, return_grids=True)
    check(res, want)
    quiet = simulate_batch(soups, max_gens=400, max_period=16, engine=ENGINE)
    assert quiet.grids is None
    check(quiet, want)
    drawn = simulate_batch(batch=B, shape=(32, 8), random=(3, 0.35), max_gens=400, max_period=16, engine=ENGINE,
                           return_grids=True)
    check(drawn, want)


@pytest.mark.parametrize("W,H", [(32, 8), (64, 64), (64, 16), (32, 32)])
def test_device_rng_is_random_grid(gpu, W, H):
    """The soups the kernel draws in its lanes.  Under B/S012345678 (cpu engine
    only) no cell ever changes, so generation 1 is the soup itself; the hip
    engine compiles lwod (B3/S012345678), whose generation 1 of the same soups
    the oracle computes from random_grid."""
    for seed, d in ((1, 0.5), (2**64 - 2, 0.3)):
        res = simulate_batch(batch=5, shape=(W, H), random=(seed, d), max_gens=1, max_period=1, rule="B/S012345678",
                             engine="cpu", return_grids=True)
        soups = np.stack([random_grid(W, H, (seed + b) % 2**64, d) for b in range(5)])
        assert np.array_equal(res.grids, soups)
        hip = simulate_batch(batch=5, shape=(W, H), random=(seed, d), max_gens=1, max_period=1, rule="lwod",
                             engine=ENGINE, return_grids=True)
        assert np.array_equal(hip.grids, bo.step(soups, "lwod"))
        assert np.array_equal(hip.population, bo.step(soups, "lwod").sum(axis=(1, 2)))


def test_cli_hip(gpu, gol_bin, tmp_path):
    rule, W, H, boundary, B, density, max_gens, P = bo.RANDOM_TABLE[0]
    want = oracle_random(bo.RANDOM_TABLE[0])
    out = tmp_path / "b.csv"
    r = subprocess.run([str(gol_bin), str(W), str(H), "none", "--batch", str(B), "--random", f"1:{density}", "--gens",
                        str(max_gens), "--max-period", str(P), "--engine", "hip", "--batch-csv", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Batch: 64 universes: 1 limit, 61 cycle, 2 extinction; largest generations 1024\n"
    rows = list(csv.reader(out.read_text().splitlines()))[1:]
    assert [[int(x[0]), int(x[1]), int(x[2]), x[3], int(x[4]), int(x[5])] for x in rows] == [
        [b, 1 + b, int(want[0][b]), bo.STOP_NAMES[want[2][b]], int(want[1][b]), int(want[3][b])] for b in range(B)]
