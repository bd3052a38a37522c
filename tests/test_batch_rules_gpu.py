"""A rule per universe on the MI355X: the rule-table kernels of life_batch.hip
against the per-universe-rule NumPy oracle of tests/test_batch_rules.py, the
cpu engine and the compiled-rule kernels."""
from __future__ import annotations

import csv
import subprocess

import numpy as np
import pytest

import batch_oracle as bo
from gol_amd import life_like_rules, random_grid, simulate_batch
from test_batch import check
from test_batch_rules import (FILE_RULES, RULES23, RULES_FILE, all_masks, check_cli_files, masks, oracle_cross,
                              run_rules, step_rules)

pytestmark = pytest.mark.gpu

ENGINE = "hip"


def neighbours(g, boundary):
    if boundary == "torus":
        return sum(np.roll(np.roll(g, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    H, W = g.shape
    p = np.pad(g, 1)
    return sum(p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))


# ---- every rule, one generation -----------------------------------------------------

@pytest.mark.parametrize("W,H,seed,boundary", [(32, 16, 29, "torus"), (32, 16, 10, "dead"), (64, 64, 1, "torus"),
                                               (64, 64, 1, "dead")])
def test_every_rule_one_generation(gpu, W, H, seed, boundary):
    """The soup holds all 18 (centre, neighbour count) combinations, so the
    successors under the 131,072 rules are pairwise distinct: a wrong entry of
    any rule's table shows."""
    g = bo.random_soups(W, H, seed, 0.5, 1)
    n = neighbours(g[0], boundary)
    assert {(int(c), int(k)) for c, k in zip(g[0].ravel(), n.ravel())} == {(c, k) for c in (0, 1) for k in range(9)}
    rules = life_like_rules()
    b, s = all_masks()
    # The oracle's step as a lookup: entry (centre, count) of rule i's table at every cell.  At 64 x 64 that is
    # seconds instead of most of a minute; every 64th rule is checked against the step itself.
    table = np.concatenate([(b[:, None] >> np.arange(9)) & 1, (s[:, None] >> np.arange(9)) & 1], axis=1).astype(np.uint8)
    want = np.take(table, (9 * g[0].astype(np.int64) + n).ravel(), axis=1).reshape(len(rules), H, W)
    sub = np.arange(0, len(rules), 64)
    assert np.array_equal(want[sub], step_rules(np.broadcast_to(g, (len(sub), H, W)), b[sub], s[sub], boundary))
    keys = np.ascontiguousarray(np.packbits(want.reshape(len(rules), -1), axis=1))
    assert len(np.unique(keys.view(f"V{keys.shape[1]}"))) == len(rules)
    res = simulate_batch(g, rules=rules, soups=1, max_gens=1, max_period=1, boundary=boundary, engine=ENGINE,
                         return_grids=True)
    assert np.array_equal(res.grids, want)
    assert np.array_equal(res.population, want.sum(axis=(1, 2)))
    assert "rule table 131072 rules x 1" in res.variant


# ---- every rule, run to the stop ------------------------------------------------------

def test_every_rule_to_the_stop(gpu):
    """32 x 8: eight universes of eight different rules share each wave."""
    rules = life_like_rules()
    kw = dict(shape=(32, 8), random=(1, 0.5), rules=rules, soups=1, max_gens=64, max_period=8, return_grids=True)
    hip = simulate_batch(engine="hip", **kw)
    cpu = simulate_batch(engine="cpu", **kw)
    check(hip, (cpu.generations, cpu.period, cpu.stop, cpu.population, cpu.grids))
    # what the NumPy oracle gives for this input
    assert hip.counts() == {"limit": 98360, "cycle": 29782, "extinction": 2930}
    assert set(hip.period.tolist()) == set(range(9))
    sub = np.arange(0, len(rules), 256)
    b, s = all_masks()
    g = bo.random_soups(32, 8, 1, 0.5, 1)
    want = run_rules(np.tile(g, (len(sub), 1, 1)), b[sub], s[sub], 64, 8)
    for got, w in zip((hip.generations, hip.period, hip.stop, hip.population, hip.grids), want):
        assert np.array_equal(got[sub], w)


# ---- every shape, both boundaries -------------------------------------------------------

_ORACLE = {}


def oracle_shape(W, H, boundary):
    """The oracle's run of RULES23 x 3 soups, computed once per session."""
    key = (W, H, boundary)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_cross(RULES23, bo.random_soups(W, H, 1, 0.4, 3), 200, 16, boundary)
    return _ORACLE[key]


@pytest.mark.parametrize("boundary", ["torus", "dead"])
@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_every_shape(gpu, W, H, boundary):
    """23 rules x 3 soups = 69 universes: a partial last wave at every H < 64,
    rule boundaries inside the waves."""
    want = oracle_shape(W, H, boundary)
    kw = dict(shape=(W, H), random=(1, 0.4), rules=RULES23, soups=3, max_gens=200, max_period=16, boundary=boundary,
              engine=ENGINE, return_grids=True)
    res = simulate_batch(**kw)
    check(res, want)
    assert "rule table 23 rules x 3" in res.variant and f"{64 // H}/wave" in res.variant
    if (W, H) in ((64, 64), (32, 16)):
        assert "dpp" in res.variant
        permuted = simulate_batch(tune={"batch_vmove": "bpermute"}, **kw)
        assert "ds_bpermute" in permuted.variant
        check(permuted, want)


def test_every_shape_covers_the_rules_and_the_stops(gpu):
    b, s = masks(RULES23)
    for n in range(1, 9):
        assert ((b >> n) & 1).any() and not ((b >> n) & 1).all(), n
    for n in range(9):
        assert ((s >> n) & 1).any() and not ((s >> n) & 1).all(), n
    stops = set()
    for boundary in ("torus", "dead"):
        for W, H in bo.SHAPES:
            stops |= set(oracle_shape(W, H, boundary)[2].tolist())
    assert stops == {bo.LIMIT, bo.CYCLE, bo.EXTINCTION}


# ---- the table kernel against the compiled kernels ------------------------------------------

def test_table_kernel_against_compiled_kernels(gpu):
    rules = list(gpu.hip_rules())
    assert len(rules) == 7
    for rule in rules:
        for shape in ((32, 16), (64, 32)):
            kw = dict(shape=shape, random=(1, 0.4), max_gens=300, max_period=64, engine=ENGINE, return_grids=True)
            table = simulate_batch(rules=[rule], soups=16, **kw)
            compiled = simulate_batch(rule=rule, batch=16, **kw)
            check(table, (compiled.generations, compiled.period, compiled.stop, compiled.population, compiled.grids))
            assert "rule table" in table.variant and "rule table" not in compiled.variant


# ---- the pairing form, the soups the kernel draws ----------------------------------------------

def test_pairing(gpu):
    W, H, B = 32, 8, 9
    rules = RULES23[7:7 + B]
    soups = bo.random_soups(W, H, 11, 0.45, B)
    b, s = masks(rules)
    want = run_rules(soups, b, s, 80, 8)
    check(simulate_batch(soups, rules=rules, max_gens=80, max_period=8, engine=ENGINE, return_grids=True), want)
    check(simulate_batch(batch=B, shape=(W, H), random=(11, 0.45), rules=rules, max_gens=80, max_period=8,
                         engine=ENGINE, return_grids=True), want)


@pytest.mark.parametrize("W,H", [(32, 8), (64, 64), (64, 16), (32, 32)])
def test_device_rng_with_soups(gpu, W, H):
    """Universe r*K + j starts from random_grid(W, H, seed + j, d): under
    B/S012345678 nothing changes (cpu engine), and generation 1 under lwod is
    the oracle's (hip engine); a second rule checks that it shares the soups."""
    K = 3
    for seed, d in ((1, 0.5), (2**64 - 2, 0.3)):
        soups = np.stack([random_grid(W, H, (seed + j) % 2**64, d) for j in range(K)])
        kw = dict(shape=(W, H), random=(seed, d), soups=K, max_gens=1, max_period=1, return_grids=True)
        cpu = simulate_batch(rules=["B/S012345678", "B/S012345678"], engine="cpu", **kw)
        assert np.array_equal(cpu.grids, np.tile(soups, (2, 1, 1)))
        hip = simulate_batch(rules=["lwod", "B/S012345678", "seeds"], engine=ENGINE, **kw)
        want = np.concatenate([bo.step(soups, "lwod"), soups, bo.step(soups, "seeds")])
        assert np.array_equal(hip.grids, want)
        assert np.array_equal(hip.population, want.sum(axis=(1, 2)))


# ---- the CLI ------------------------------------------------------------------------------------

def test_cli_hip(gpu, gol_bin, tmp_path):
    assert "B35/S236" in FILE_RULES and "B35/S236" not in gpu.hip_rules()
    (tmp_path / "rules.txt").write_text(RULES_FILE)
    K, W, H = 4, 32, 16
    want = oracle_cross(FILE_RULES, bo.random_soups(W, H, 7, 0.4, K), 200, 16)
    c = bo.counts(want[2])
    out, per = tmp_path / "b.csv", tmp_path / "r.csv"
    r = subprocess.run([str(gol_bin), str(W), str(H), "none", "--batch-rules", "rules.txt", "--soups", str(K),
                        "--random", "7:0.4", "--gens", "200", "--max-period", "16", "--engine", "hip", "--batch-csv",
                        str(out), "--rules-csv", str(per)], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == (f"Batch: 20 universes: {c['limit']} limit, {c['cycle']} cycle, {c['extinction']} extinction; "
                        f"largest generations {want[0].max()}\nRules: 5 rules x 4 soups\n")
    check_cli_files(FILE_RULES, K, 7, want, out, per)
    assert list(csv.reader(per.read_text().splitlines()))[3][0] == "B35/S236"
