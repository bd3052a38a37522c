"""Cycle detection on the CPU tier: the per-generation grid fingerprint
(LifeConfig.fingerprint) of the cpu and ref engines against an independent
NumPy oracle (tests/cycle_oracle.py), over layouts, rules, boundaries, chunked
runs and decompositions; Simulation.find_cycle against a brute-force finder that
keeps whole grids, on a board of known oscillators and on soups; its bounds and
stops; the rejection path (tuning cycle_match_bits); the CLIs, the checkpoints
and the untouched default."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cycle_oracle as co
from gol_amd import (CycleReport, LifeConfig, Simulation, grid_fingerprint, life_step_numpy, parse_rule, random_grid,
                     reference_run)
from gol_amd.parallel import InProcessGroup
from gol_amd.utils import io
from gol_amd.utils.checkpoint import load_checkpoint, run_with_checkpoints, save_checkpoint

REPO = Path(__file__).resolve().parents[1]


def oracle_grids(g, gens, rule="B3/S23", boundary="torus"):
    """grids[t]: generation t, t = 0..gens, stepped with NumPy."""
    grids = [np.ascontiguousarray(g, dtype=np.uint8)]
    for _ in range(gens):
        grids.append(life_step_numpy(grids[-1], 1, rule=parse_rule(rule), boundary=boundary))
    return grids


def cpu_sim(g, layout="auto", tune=None, **kw):
    H, W = g.shape
    sim = Simulation(LifeConfig(W, H, gen_limit=10**6, check_similarity=False, layout=layout, fingerprint=True,
                                tune=tune or {}, **kw), engine="cpu")
    sim.load(g)
    return sim


# ---- 1. the series -----------------------------------------------------------------------------------
def test_host_formula_vs_oracle(native):
    """The package's host implementation and the oracle agree, on odd widths
    too, and the fingerprint sees where a cell is."""
    for W, H in ((96, 48), (33, 33), (257, 129), (1, 1), (32, 1)):
        g = random_grid(W, H, W + H, 0.4)
        assert grid_fingerprint(g) == co.fingerprint(g), (W, H)
    g = np.zeros((8, 70), dtype=np.uint8)
    one = []
    for y, x in ((0, 0), (0, 1), (1, 0), (0, 32), (7, 69)):
        g[:] = 0
        g[y, x] = 1
        one.append(grid_fingerprint(g))
    assert len(set(one)) == len(one) and grid_fingerprint(np.zeros((8, 70), dtype=np.uint8)) == 0


@pytest.mark.parametrize("boundary", ["torus", "dead"])
@pytest.mark.parametrize("rule", ["B3/S23", "highlife"])
@pytest.mark.parametrize("W,H,layout", [(96, 48, "bits"), (33, 33, "u8"), (257, 129, "u8")])
def test_series_vs_oracle(native, W, H, layout, rule, boundary):
    g = random_grid(W, H, 5, 0.4)
    gens = 40
    grids = oracle_grids(g, gens, rule, boundary)
    want = co.series(grids[1:])
    assert len(set(want.tolist())) == gens  # a soup: every generation differs
    # cpu engine: a deep-halo epoch, whose halo rows hold live cells that must not be weighed
    for tmax, epoch in ((8, 16), (16, 0)):
        sim = cpu_sim(g, layout, tmax=tmax, epoch=epoch, rule=rule, boundary=boundary)
        assert sim.fingerprint() == co.fingerprint(g)
        rep = sim.advance(gens)
        assert rep.fingerprint.dtype == np.uint64 and rep.fingerprint.tolist() == want.tolist(), (tmax, epoch)
        assert (sim.tile() == grids[-1]).all()
        assert int(rep.fingerprint[-1]) == sim.fingerprint() == grid_fingerprint(sim.tile())
        d = sim.describe()
        assert d["fingerprint"] is True and "fingerprint" in d["kernel"]
    # ref engine
    out, n, _, fp = reference_run(g, gens, False, rule=rule, boundary=boundary, fingerprint=True)
    assert n == gens and fp.dtype == np.uint64 and fp.tolist() == want.tolist() and (out == grids[-1]).all()
    # with the census too: (grid, gens, ms, population, fingerprint)
    r5 = reference_run(g, gens, False, rule=rule, boundary=boundary, census=True, fingerprint=True)
    assert len(r5) == 5 and r5[3].tolist() == [int(x.sum()) for x in grids[1:]] and r5[4].tolist() == want.tolist()


@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_series_with_census_drift_request_and_ring(native, layout):
    """The census and the fingerprint together; a backend asked to drift its
    frame does not (the fingerprint weighs columns); a row ring."""
    g = random_grid(96, 70, 8, 0.4)
    grids = oracle_grids(g, 30)
    sim = cpu_sim(g, layout, census=True, tune={"cpu_drift": "1", "cpu_ring": "1"})
    rep = sim.advance(30)
    assert rep.fingerprint.tolist() == co.series(grids[1:]).tolist()
    assert rep.population.tolist() == [int(x.sum()) for x in grids[1:]]
    assert sim.describe()["drifting"] is False


def test_chunked_runs_concatenate(native):
    g = random_grid(96, 48, 12, 0.4)
    want = co.series(oracle_grids(g, 100)[1:]).tolist()
    sim = cpu_sim(g)
    parts = [sim.advance(n).fingerprint.tolist() for n in (37, 5, 58)]
    assert [len(p) for p in parts] == [37, 5, 58] and sum(parts, []) == want
    assert cpu_sim(g).advance(100).fingerprint.tolist() == want


DECOMPS = [(spec, P, W, H, layout) for spec, P in (("1x1", 1), ("2x2", 4), ("1x3", 3))
           for W, H, layout in ((96, 48, "bits"), (33, 33, "u8"), (257, 129, "u8"), (200, 60, "u8"))
           if not (W == 33 and spec == "2x2")]  # the engine splits no columns into tiles narrower than 32 cells


@pytest.mark.parametrize("spec,P,W,H,layout", DECOMPS)
def test_decompositions_report_the_global_series(native, tune, spec, P, W, H, layout):
    """Byte grids of 257 and 200 columns split at columns 128 and 100: where
    that is no multiple of 32, the cpu engine weighs a tile's cells by the
    global word grid all the same."""
    g = random_grid(W, H, 77, 0.4)
    gens = 35
    grids = oracle_grids(g, gens)
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, decomp=spec, layout=layout, tmax=8, epoch=16,
                                    fingerprint=True, tune=tune), P, engine="cpu")
    grp.load(g)
    assert grp.fingerprint() == [co.fingerprint(g)] * P
    reps = grp.advance(gens)
    assert len(reps) == P
    for rep in reps:  # every rank: the sum over ranks, not its share
        assert rep.fingerprint.tolist() == co.series(grids[1:]).tolist()
    assert (grp.gather() == grids[-1]).all()
    assert grp.fingerprint() == [co.fingerprint(grids[-1])] * P


def test_gloo_callback_transport_sums(native, tmp_path):
    """Two rank processes over gloo: the series goes through the callback
    transport's torch.distributed SUM on int64 views, whose two's-complement
    addition is the sum modulo 2^64."""
    W, H, gens = 128, 96, 60
    g = random_grid(W, H, 31, 0.4)
    io.write_grid(str(tmp_path / "in.txt"), g)
    env = dict(os.environ, PYTHONPATH=str(REPO) + os.pathsep + os.environ.get("PYTHONPATH", ""),
               GOL_HOST_THREADS="2", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node=2", "--standalone",
           "--local-addr=127.0.0.1", "-m", "gol_amd", str(W), str(H), "in.txt", "--engine", "cpu", "--gens", str(gens),
           "--no-similarity", "--decomp", "1x2", "--comm", "torch", "--epoch", "9", "--fingerprint", "fp.csv",
           "--metrics-json", "m.json", "--output", "out.txt", "--style", "mpi"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    grids = oracle_grids(g, gens)
    want = co.series(grids[1:]).tolist()
    assert sum(v >= 2**63 for v in want) > 5  # sums that are negative as int64
    assert (tmp_path / "out.txt").read_text() == io.format_text(grids[-1])
    assert (tmp_path / "fp.csv").read_text().splitlines() == [f"{i + 1},{v:016x}" for i, v in enumerate(want)]
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["fingerprint"] is True and m["fingerprints"] == [f"{v:016x}" for v in want] and m["ranks"] == 2


# ---- 2. the pattern board ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def board():
    """(grid, grids of generations 0 .. 9 + 30 - 1 ... as found by brute force)."""
    b = co.pattern_board()
    entry, period, grids = co.brute_cycle(b, life_step_numpy, 400)
    # the brute-force result itself: the tests below cannot pass vacuously
    assert (entry, period) == (co.BOARD_ENTRY, co.BOARD_PERIOD) == (9, 30)
    return b, grids


def board_grid_at(grids, generation):
    return grids[9 + (generation - 9) % 30]


def check_board_cycle(sim, r: CycleReport, grids, chunk_len):
    assert isinstance(r, CycleReport)
    assert r.period == 30 and r.stop_reason == "cycle" and r.confirmations == 1
    assert r.generation == sim.generation
    assert 9 + 2 * 30 - 1 <= r.generation <= 9 + 2 * 30 - 1 + chunk_len + 30
    assert (sim.tile() == board_grid_at(grids, r.generation)).all()
    assert len(r.fingerprint) == r.generation
    assert int(r.fingerprint[-1]) == co.fingerprint(sim.tile())


@pytest.mark.parametrize("layout", ["bits", "u8"])
@pytest.mark.parametrize("chunk", [7, 64, 0])
def test_find_cycle_on_the_pattern_board(native, board, chunk, layout):
    b, grids = board
    sim = cpu_sim(b, layout)
    r = sim.find_cycle(400, 64, chunk)
    check_board_cycle(sim, r, grids, chunk or 256)
    assert r.repeats_from == 9 and r.false_candidates == 0


def test_find_cycle_over_ranks(native, board, tune):
    b, grids = board
    grp = InProcessGroup(LifeConfig(96, 48, decomp="2x2", tmax=4, epoch=8, fingerprint=True, tune=tune), 4,
                         engine="cpu")
    grp.load(b)
    rs = grp.find_cycle(400, 64, 16)
    assert len({(r.period, r.generation, r.repeats_from, r.false_candidates) for r in rs}) == 1
    assert rs[0].period == 30 and rs[0].repeats_from == 9
    assert (grp.gather() == board_grid_at(grids, rs[0].generation)).all()


# ---- 3. bounds and stops ---------------------------------------------------------------------------------
def test_max_period_below_the_period_runs_to_the_limit(native, board):
    b, grids = board
    sim = cpu_sim(b)
    r = sim.find_cycle(400, 29)
    assert r.period == 0 and r.stop_reason == "limit" and r.repeats_from == -1 and r.confirmations == 0
    assert sim.generation == 400 == r.generation and (sim.tile() == board_grid_at(grids, 400)).all()


def test_a_confirmation_that_would_pass_the_limit_is_skipped(native, board):
    b, _ = board
    sim = cpu_sim(b)
    r = sim.find_cycle(80, 64, 75)  # the first search is at 75; 75 + 30 > 80
    assert r.period == 0 and r.stop_reason == "limit" and sim.generation == 80 and r.false_candidates == 0


def test_a_lone_block_is_period_one(native):
    sim = cpu_sim(co.pattern_board(["block"]))
    r = sim.find_cycle(400, 64)
    assert r.period == 1 and r.stop_reason == "cycle" and r.repeats_from == 0 and r.generation == sim.generation
    assert (sim.tile() == co.pattern_board(["block"])).all()


def test_a_board_that_dies_out_is_an_extinction(native):
    g = np.zeros((48, 96), dtype=np.uint8)
    g[3, 3:5] = 1  # two cells: dead after one generation
    sim = cpu_sim(g)
    r = sim.find_cycle(400, 64)
    assert r.period == 1 and r.stop_reason == "extinction" and not sim.tile().any()


def test_find_cycle_needs_the_fingerprint(native):
    sim = Simulation(LifeConfig(96, 48), engine="cpu")
    with pytest.raises(RuntimeError, match="find_cycle needs fingerprint=1"):
        sim.find_cycle(100, 8)


# ---- 4. soups --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [2, 3, 4, 5])
def test_soups_settle_as_brute_force_says(native, seed):
    g = random_grid(64, 40, seed, 0.4)
    entry, period, grids = co.brute_cycle(g, life_step_numpy, 6000)
    assert entry is not None and period <= 300, "brute force found no cycle of period <= 300 within the limit"
    sim = cpu_sim(g)
    r = sim.find_cycle(6000, 300)
    assert (r.period, r.repeats_from, r.stop_reason) == (period, entry, "cycle")
    assert (sim.tile() == grids[entry + (r.generation - entry) % period]).all()


# ---- 5. the rejection path -------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 4])
def test_cycle_match_bits(native, board, bits):
    """With few or no bits compared, candidates are rejected on the cells and
    the result stays the same (chunk 7: the first search is in the transient)."""
    b, grids = board
    sim = cpu_sim(b, tune={"cycle_match_bits": bits})
    r = sim.find_cycle(400, 64, 7)
    assert r.period == 30 and r.stop_reason == "cycle" and r.false_candidates > 0
    assert r.generation == sim.generation and (sim.tile() == board_grid_at(grids, r.generation)).all()


# ---- 6. CLIs -----------------------------------------------------------------------------------------------
def _gol(gol_bin, args, cwd, ok=True):
    r = subprocess.run([str(gol_bin), *map(str, args)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _py(args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=str(REPO), GOL_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-m", "gol_amd", *map(str, args)], cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.mark.parametrize("front", ["gol", "py"])
def test_cli_fingerprint_and_cycle(native, gol_bin, tmp_path, front, board):
    run = (lambda a, ok=True: _gol(gol_bin, a, tmp_path, ok)) if front == "gol" else (
        lambda a, ok=True: _py(a, tmp_path, ok))
    help_text = run(["--help"]).stdout
    assert "--fingerprint" in help_text and "--cycle" in help_text
    g = random_grid(64, 64, 3, 0.3)
    io.write_grid(str(tmp_path / "in.txt"), g)
    want = [f"{i + 1},{v:016x}" for i, v in enumerate(co.series(oracle_grids(g, 40)[1:]).tolist())]
    for engine in ("cpu", "ref"):
        run([64, 64, "in.txt", "--engine", engine, "--gens", 40, "--no-similarity", "--fingerprint", f"{engine}.csv",
             "--output", "none", "--metrics-json", f"{engine}.json"])
        assert (tmp_path / f"{engine}.csv").read_text().splitlines() == want, engine
    m = json.loads((tmp_path / "cpu.json").read_text())
    assert m["fingerprint"] is True and m["fingerprints"] == [ln.split(",")[1] for ln in want] and "cycle" not in m
    # neither flag: the usual output, no series in the metrics
    plain = run([64, 64, "in.txt", "--engine", "cpu", "--gens", 40, "--output", "none", "--metrics-json", "off.json"])
    assert "Cycle" not in plain.stdout and "fingerprints" not in json.loads((tmp_path / "off.json").read_text())
    # --cycle: the usual lines, then one more
    b, grids = board
    io.write_grid(str(tmp_path / "board.txt"), b)
    r = run([96, 48, "board.txt", "--engine", "cpu", "--gens", 400, "--cycle", 64, "--output", "out.txt",
             "--fingerprint", "board.csv", "--metrics-json", "c.json"])
    usual = run([96, 48, "board.txt", "--engine", "cpu", "--gens", 400, "--output", "none"]).stdout.splitlines()
    lines = r.stdout.splitlines()
    c = json.loads((tmp_path / "c.json").read_text())["cycle"]
    assert lines[-1] == f"Cycle: period 30 at generation {c['generation']} (fingerprints repeat from 9)"
    assert len(lines) == len(usual) + 1
    assert [ln.split(":")[0] for ln in lines[:-1]] == [ln.split(":")[0] for ln in usual]
    assert (c["period"], c["repeats_from"], c["stop_reason"], c["false_candidates"]) == (30, 9, "cycle", 0)
    assert (tmp_path / "out.txt").read_text() == io.format_text(board_grid_at(grids, c["generation"]))
    assert len((tmp_path / "board.csv").read_text().splitlines()) == c["generation"]
    r = run([96, 48, "board.txt", "--engine", "cpu", "--gens", 400, "--cycle", 29, "--output", "none"])
    assert r.stdout.splitlines()[-1] == "Cycle: none within 400 generations"
    # what --cycle does not run with is refused by name
    assert "--cycle" in run([96, 48, "board.txt", "--engine", "ref", "--cycle", 8], ok=False).stderr
    assert "--cycle" in run([96, 48, "board.txt", "--engine", "cpu", "--cycle", 0], ok=False).stderr


# ---- 7. checkpoints ----------------------------------------------------------------------------------------
def test_checkpoint_api_carries_the_setting(native, tmp_path):
    g = random_grid(64, 64, 5, 0.3)
    want = co.series(oracle_grids(g, 80)[1:]).tolist()
    sim = Simulation(LifeConfig(64, 64, gen_limit=80, check_similarity=False, fingerprint=True), engine="cpu")
    sim.load(g)
    first = sim.native_engine.run_until(30)
    save_checkpoint(sim, str(tmp_path / "ck"))
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["fingerprint"] is True and "fingerprints" not in meta  # the setting, not the series
    cfg, grid = load_checkpoint(str(tmp_path / "ck"))
    assert cfg.fingerprint is True and cfg.start_gen == 30
    sim2 = Simulation(cfg, engine="cpu")
    sim2.load_text(str(grid))
    rep = run_with_checkpoints(sim2, 20, None)
    assert np.asarray(first.fingerprint).tolist() == want[:30] and rep.fingerprint.tolist() == want[30:]
    off = Simulation(LifeConfig(64, 64), engine="cpu")
    off.load(g)
    save_checkpoint(off, str(tmp_path / "ck0"))
    assert "fingerprint" not in json.loads((tmp_path / "ck0" / "meta.json").read_text())
    assert load_checkpoint(str(tmp_path / "ck0"))[0].fingerprint is False


@pytest.mark.parametrize("front", ["gol", "py"])
def test_checkpoint_cli_carries_the_setting(native, gol_bin, tmp_path, front):
    run = (lambda a: _gol(gol_bin, a, tmp_path)) if front == "gol" else (lambda a: _py(a, tmp_path))
    other = (lambda a: _py(a, tmp_path)) if front == "gol" else (lambda a: _gol(gol_bin, a, tmp_path))
    W, H = 96, 64
    g = random_grid(W, H, 3, 0.3)
    io.write_grid(str(tmp_path / "in.txt"), g)
    want = [f"{v:016x}" for v in co.series(oracle_grids(g, 50)[1:]).tolist()]
    run([W, H, "in.txt", "--engine", "cpu", "--no-similarity", "--fingerprint", "a.csv", "--gens", 20,
         "--checkpoint-every", 7, "--checkpoint-dir", "ck", "--output", "none"])
    assert (tmp_path / "a.csv").read_text().splitlines() == [f"{i + 1},{v}" for i, v in enumerate(want[:20])]
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["generation"] == 14 and meta["fingerprint"] is True
    # a resume takes the setting from the checkpoint; either front end
    other([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--output", "none", "--metrics-json", "r.json"])
    assert json.loads((tmp_path / "r.json").read_text())["fingerprints"] == want[14:]


# ---- 8. off by default -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_off_by_default(native, layout):
    g = random_grid(96, 48, 3, 0.4)
    assert LifeConfig(96, 48).fingerprint is False
    sim = Simulation(LifeConfig(96, 48, gen_limit=30, check_similarity=False, layout=layout), engine="cpu")
    sim.load(g)
    rep = sim.run()
    assert rep.fingerprint.dtype == np.uint64 and len(rep.fingerprint) == 0
    d = sim.describe()
    assert d["fingerprint"] is False and "fingerprint" not in d["kernel"]
    assert "fingerprint" not in rep.as_dict()
    assert sim.fingerprint() == co.fingerprint(sim.tile())  # the stand-alone value needs no setting
    assert len(reference_run(g, 30, False)) == 3


def test_refusals_that_need_no_gpu(native):
    with pytest.raises(RuntimeError, match="fingerprint=1 with self_exchange"):
        Simulation(LifeConfig(64, 64, fingerprint=True, self_exchange=True), engine="cpu")
    with pytest.raises(RuntimeError, match="fingerprint=1 with graphs=1"):
        Simulation(LifeConfig(64, 64, fingerprint=True, graphs="on"), engine="cpu")
    be = native.cpu_backend(1)
    assert be.supports_fingerprint(native.Layout.Bits, "B36/S23", "dead", True)
