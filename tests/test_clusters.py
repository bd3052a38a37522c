"""The cluster census of batched universes: the oracle's own properties, the
cpu engine against the oracle (all fields, and order), the host functions and
both command lines (tests/cluster_oracle.py has the definition and the cases;
tests/test_clusters_gpu.py runs the same cases on the hip engine)."""
from __future__ import annotations

import csv
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import batch_oracle as bo
import cluster_oracle as co
import gol_amd

REPO = Path(__file__).resolve().parent.parent
BOUNDARIES = ("torus", "dead")
BLOCK_SIG = co.signature(np.ones((2, 2), dtype=np.uint8))


def assert_census(got, want):
    counts, recs = got
    want_counts, want_recs = want
    assert counts.dtype == np.int32 and recs.dtype == co.RECORD
    assert np.array_equal(counts, want_counts)
    assert len(recs) == len(want_recs)
    for name in co.RECORD.names:
        bad = np.flatnonzero(recs[name] != want_recs[name])
        assert bad.size == 0, (name, recs[bad[:3]], want_recs[bad[:3]])


# ---- the definition itself (oracle only): what the issue states must hold ------

@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_oracle_seams_and_linking(W, H):
    for name, rows in (("block", co.BLOCK), ("blinker", co.BLINKER), ("glider", co.GLIDER)):
        middle = co.of_case(W, H, "torus", f"{name} middle")
        assert len(middle) == 1 and int(middle[0]["signature"]) == co.signature(co.images(rows)[0])
        assert gol_amd.cluster_name(int(middle[0]["signature"])) == name
        for where in co.seam_positions(W, H):
            r = co.of_case(W, H, "torus", f"{name} {where}")
            assert len(r) == 1 and r[0]["spanning"] == 0, (name, where)
            assert r[["signature", "cells", "height", "width"]] == middle[["signature", "cells", "height", "width"]]
    assert len(co.of_case(W, H, "dead", "four corners")) == 4
    for where in co.seam_positions(W, H):
        for dy, dx in co.PAIRS:
            assert len(co.of_case(W, H, "torus", f"pair {dy},{dx} {where}")) == (1 if max(abs(dy), abs(dx)) == 2 else 2)
    for dy, dx in co.PAIRS:
        assert len(co.of_case(W, H, "dead", f"pair {dy},{dx} middle")) == (1 if max(abs(dy), abs(dx)) == 2 else 2)
    for y in (0, 1):
        assert len(co.of_case(W, H, "dead", f"rows {y} and last")) == 2
        assert len(co.of_case(W, H, "torus", f"rows {y} and last")) == 1


@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_oracle_spanning_and_counts(W, H):
    span = {label: co.of_case(W, H, "torus", label) for label in
            ("full row", "full column", "full grid", "row gap 1", "row gap 2")}
    assert all(len(r) == 1 for r in span.values())
    assert [int(span[k][0]["spanning"]) for k in span] == [co.SPANS_X, co.SPANS_Y, co.SPANS_X | co.SPANS_Y,
                                                           co.SPANS_X, 0]
    assert (span["full row"][0]["height"], span["full row"][0]["width"]) == (1, W)
    assert (span["full column"][0]["height"], span["full column"][0]["width"]) == (H, 1)
    assert span["row gap 1"][0]["width"] == W and span["row gap 1"][0]["cells"] == W - 1
    # A gap of 2: the origin is the cell after the gap, so the cluster is a plain row of W - 2 cells.
    assert span["row gap 2"][0]["width"] == W - 2
    assert int(span["row gap 2"][0]["signature"]) == co.signature(np.ones((1, W - 2), dtype=np.uint8))
    assert len(co.of_case(W, H, "torus", "empty")) == 0 and len(co.of_case(W, H, "dead", "empty")) == 0
    assert len(co.of_case(W, H, "torus", "lattice torus")) == (H // 3) * (W // 3)
    assert len(co.of_case(W, H, "dead", "lattice plane")) == -(-H // 3) * -(-W // 3)
    if (W, H) == (64, 64):
        assert len(co.of_case(W, H, "torus", "lattice torus")) == 441
        assert len(co.of_case(W, H, "dead", "lattice plane")) == 484
    for bd in BOUNDARIES:
        s = co.of_case(W, H, bd, "serpentine")
        assert len(s) == 1 and s[0]["cells"] == co.serpentine(W, H).sum() and s[0]["spanning"] == 0


def test_oracle_known_signatures():
    assert BLOCK_SIG == 0x39AD81228FA38958
    assert co.signature(np.ones((1, 3), dtype=np.uint8)) == 0x2EE499925DD09FC9
    assert co.signature(np.ones((3, 1), dtype=np.uint8)) == 0x402127091C2A1A91
    assert len({co.signature(f) for f in co.named_forms("glider")}) == 16


# ---- the cpu engine -------------------------------------------------------------

@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("W,H", bo.SHAPES)
def test_cpu_cases(W, H, boundary):
    grids = co.case_grids(W, H)[1]
    assert_census(gol_amd.find_clusters(grids, boundary, engine="cpu"), co.case_records(W, H, boundary))


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("B", [1, 7, 9, 65])
def test_cpu_predication(B, boundary):
    got = gol_amd.find_clusters(co.predication_batch(B), boundary, engine="cpu", threads=3)
    assert_census(got, co.predication_records(B, boundary))


@pytest.mark.parametrize("row", bo.RANDOM_TABLE, ids=lambda r: f"{r[0]}-{r[1]}x{r[2]}-{r[3]}")
def test_cpu_end_to_end(row):
    rule, W, H, boundary, B, density, max_gens, P = row
    soups = bo.random_soups(W, H, 1, density, B)
    final = bo.run(soups, max_gens, P, bo.RULES[rule], boundary)[4]
    want = co.records(final, boundary)
    res = gol_amd.simulate_batch(batch=B, shape=(W, H), random=(1, density), max_gens=max_gens, max_period=P,
                                 rule=rule, boundary=boundary, engine="cpu", clusters=True)
    assert_census((res.clusters, res.cluster_records), want)
    assert int(res.clusters.sum()) == len(res.cluster_records)
    assert res.clusters_ms is not None and res.clusters_ms >= 0
    table = res.cluster_table()
    assert [(t[0], *t[2:]) for t in table] == co.table(want[1])
    if rule == "life":
        names = {t[1]: t[6] for t in table}
        assert names["block"] == int((want[1]["signature"] == BLOCK_SIG).sum()) > 0
        assert names["blinker"] > 0
        cyc = res.cluster_table(stop="cycle")
        assert sum(t[6] for t in cyc) == int(res.clusters[res.stop == bo.CYCLE].sum())


def test_cpu_rules_with_soups_and_option_off():
    rules, K, W, H = ["B3/S23", "B36/S23", "B2/S"], 4, 32, 16
    soups = bo.random_soups(W, H, 5, 0.35, K)
    kw = dict(max_gens=300, max_period=16, engine="cpu", return_grids=True)
    res = gol_amd.simulate_batch(soups, rules=rules, soups=K, clusters=True, **kw)
    off = gol_amd.simulate_batch(soups, rules=rules, soups=K, **kw)
    assert off.clusters is None and off.cluster_records is None and off.clusters_ms is None
    with pytest.raises(ValueError, match="clusters=True"):
        off.cluster_table()
    for name in ("generations", "period", "stop", "population", "grids"):
        assert np.array_equal(getattr(res, name), getattr(off, name)), name
    assert res.variant == off.variant
    assert_census((res.clusters, res.cluster_records), co.records(res.grids, "torus"))


# ---- host functions ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(co.NAMED))
def test_names(name):
    for form in co.named_forms(name):
        sig = gol_amd.cluster_signature(form)
        assert sig == co.signature(form)
        assert gol_amd.cluster_name(sig) == name


def test_signature_refusals_and_unknown_names():
    two = np.zeros((3, 9), dtype=np.uint8)
    two[1, 1] = two[1, 4] = 1  # distance 3
    with pytest.raises(RuntimeError, match="more than one cluster"):
        gol_amd.cluster_signature(two)
    two[1, 4], two[1, 3] = 0, 1  # distance 2
    assert gol_amd.cluster_signature(two) == co.signature(two)
    with pytest.raises(RuntimeError, match="no live cell"):
        gol_amd.cluster_signature(np.zeros((4, 4), dtype=np.uint8))
    wide = np.zeros((5, 200), dtype=np.uint8)  # any size: wider than a batch universe
    wide[2, 3:190:2] = 1
    assert gol_amd.cluster_signature(wide) == co.signature(wide)
    assert gol_amd.cluster_name(0x0123456789ABCDEF) == "0123456789abcdef"
    assert gol_amd.cluster_name(5) == "0000000000000005"


def test_record_limit():
    C = gol_amd.native()
    assert C.CLUSTER_RECORDS_MAX == 2**28
    total, offsets = C.cluster_offsets([3, 0, 2])
    assert total == 5 and list(offsets) == [0, 3, 3]
    counts = np.full(2**20, 256, dtype=np.int32)  # exactly 2^28: accepted
    assert C.cluster_offsets(counts)[0] == 2**28
    counts[-1] += 1
    with pytest.raises(RuntimeError, match=r"2\^28 = 268435456"):
        C.cluster_offsets(counts)


def test_find_clusters_refusals():
    with pytest.raises(RuntimeError, match="width must be 32 or 64"):
        gol_amd.find_clusters(np.zeros((1, 8, 48), dtype=np.uint8), engine="cpu")
    with pytest.raises(RuntimeError, match="0 .dead. and 1 .live. only"):
        gol_amd.find_clusters(np.full((1, 8, 32), 2, dtype=np.uint8), engine="cpu")
    with pytest.raises(ValueError, match="B, H, W"):
        gol_amd.find_clusters(np.zeros((8, 32), dtype=np.uint8), engine="cpu")


# ---- both command lines -------------------------------------------------------------

def run_cli(which, args, cwd):
    cmd = [str(REPO / "bin" / "gol")] if which == "gol" else [sys.executable, "-m", "gol_amd"]
    return subprocess.run(cmd + args, cwd=cwd, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=str(REPO)))


@pytest.mark.parametrize("which", ["gol", "python"])
def test_cli_census(which, native, tmp_path):
    W, H, B, seed, density, gens = 32, 16, 24, 3, 0.4, 400
    final = bo.run(bo.random_soups(W, H, seed, density, B), gens, 64, "B3/S23", "torus")[4]
    want = co.table(co.records(final, "torus")[1])
    base = [str(W), str(H), "none", "--random", f"{seed}:{density}", "--gens", str(gens), "--batch", str(B),
            "--engine", "cpu"]
    plain = run_cli(which, base + ["--metrics-json", "plain.json"], tmp_path)
    r = run_cli(which, base + ["--batch-census", "census.csv", "--metrics-json", "m.json"], tmp_path)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[:-1] == plain.stdout.splitlines()  # the existing lines, then one more
    total = sum(t[5] for t in want)
    assert lines[-1] == (f"Clusters: {total} in {B} universes, {len(want)} kinds; most common "
                         f"{gol_amd.cluster_name(want[0][0])} x{want[0][5]}")
    with open(tmp_path / "census.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["signature", "name", "cells", "height", "width", "spanning", "count"]
    assert rows[1:] == [[f"{t[0]:016x}", gol_amd.cluster_name(t[0]), *map(str, t[1:])] for t in want]
    m, p = json.loads((tmp_path / "m.json").read_text()), json.loads((tmp_path / "plain.json").read_text())
    assert m["batch_clusters"] == total and m["batch_cluster_kinds"] == len(want) and m["batch_clusters_ms"] >= 0
    assert set(m) - set(p) == {"batch_clusters", "batch_cluster_kinds", "batch_clusters_ms"}


@pytest.mark.parametrize("which", ["gol", "python"])
def test_cli_census_needs_a_batch(which, native, tmp_path):
    r = run_cli(which, ["32", "16", "none", "--random", "3", "--gens", "5", "--engine", "cpu", "--batch-census",
                        "census.csv"], tmp_path)
    assert r.returncode != 0
    assert "--batch-census needs --batch" in r.stderr + r.stdout
    assert not (tmp_path / "census.csv").exists()
