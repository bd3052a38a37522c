"""The cluster census on the hip engine (csrc/kernels/life_batch_clusters.hip)
against the oracle: all fields and the order, on every batch shape and both
boundaries (tests/cluster_oracle.py has the definition and the cases, whose
properties tests/test_clusters.py checks)."""
from __future__ import annotations

import csv
import subprocess

import numpy as np
import pytest

import batch_oracle as bo
import cluster_oracle as co
import gol_amd
from test_clusters import BLOCK_SIG, BOUNDARIES, assert_census

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_cases(gpu, W, H, boundary):
    """Seams, linking distance, spanning, the lattices, the serpentine: some 70 grids a shape."""
    grids = co.case_grids(W, H)[1]
    want = co.case_records(W, H, boundary)
    assert_census(gol_amd.find_clusters(grids, boundary, engine="hip"), want)
    if H in (16, 64):  # the heights with a DPP move: the permute computes the same
        assert_census(gol_amd.find_clusters(grids, boundary, engine="hip", tune={"batch_vmove": "bpermute"}), want)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("B", [1, 7, 9, 65])
def test_predication(gpu, B, boundary):
    """32 x 8: eight universes a wave with 0, 1 and many clusters, full edge rows next to each other,
    partial last waves."""
    grids = co.predication_batch(B)
    want = co.predication_records(B, boundary)
    assert_census(gol_amd.find_clusters(grids, boundary, engine="hip"), want)
    assert_census(gol_amd.find_clusters(grids, boundary, engine="hip", tune={"batch_vmove": "bpermute"}), want)


@pytest.mark.parametrize("row", bo.RANDOM_TABLE, ids=lambda r: f"{r[0]}-{r[1]}x{r[2]}-{r[3]}")
def test_end_to_end(gpu, row):
    rule, W, H, boundary, B, density, max_gens, P = row
    final = bo.run(bo.random_soups(W, H, 1, density, B), max_gens, P, bo.RULES[rule], boundary)[4]
    want = co.records(final, boundary)
    kw = dict(batch=B, shape=(W, H), random=(1, density), max_gens=max_gens, max_period=P, rule=rule,
              boundary=boundary, engine="hip")
    res = gol_amd.simulate_batch(clusters=True, **kw)
    assert_census((res.clusters, res.cluster_records), want)
    assert int(res.clusters.sum()) == len(res.cluster_records)
    assert res.clusters_ms > 0
    assert [(t[0], *t[2:]) for t in res.cluster_table()] == co.table(want[1])
    if rule == "life":
        names = {t[1]: t[6] for t in res.cluster_table()}
        assert names["block"] == int((want[1]["signature"] == BLOCK_SIG).sum()) > 0
        assert names["blinker"] > 0
    off = gol_amd.simulate_batch(return_grids=True, **kw)
    assert off.clusters is None and off.cluster_records is None
    assert np.array_equal(off.grids, final)
    for name in ("generations", "period", "stop", "population"):
        assert np.array_equal(getattr(res, name), getattr(off, name)), name
    assert res.variant == off.variant


def test_rules_with_soups(gpu):
    rules, K, W, H = ["B3/S23", "B36/S23", "B2/S", "B3678/S34678"], 5, 64, 16
    soups = bo.random_soups(W, H, 5, 0.35, K)
    res = gol_amd.simulate_batch(soups, rules=rules, soups=K, max_gens=300, max_period=16, engine="hip",
                                 return_grids=True, clusters=True)
    cpu = gol_amd.simulate_batch(soups, rules=rules, soups=K, max_gens=300, max_period=16, engine="cpu",
                                 return_grids=True, clusters=True)
    assert np.array_equal(res.grids, cpu.grids)
    assert_census((res.clusters, res.cluster_records), co.records(res.grids, "torus"))
    assert_census((res.clusters, res.cluster_records), (cpu.clusters, cpu.cluster_records))


def test_cli_hip(gpu, gol_bin, tmp_path):
    W, H, B, seed, density, gens = 64, 32, 40, 9, 0.4, 600
    final = bo.run(bo.random_soups(W, H, seed, density, B), gens, 64, "B3/S23", "dead")[4]
    want = co.table(co.records(final, "dead")[1])
    r = subprocess.run([str(gol_bin), str(W), str(H), "none", "--random", f"{seed}:{density}", "--gens", str(gens),
                        "--batch", str(B), "--boundary", "dead", "--engine", "hip", "--batch-census", "census.csv"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    total = sum(t[5] for t in want)
    assert r.stdout.splitlines()[-1] == (f"Clusters: {total} in {B} universes, {len(want)} kinds; most common "
                                         f"{gol_amd.cluster_name(want[0][0])} x{want[0][5]}")
    with open(tmp_path / "census.csv") as f:
        rows = list(csv.reader(f))
    assert rows[1:] == [[f"{t[0]:016x}", gol_amd.cluster_name(t[0]), *map(str, t[1:])] for t in want]
