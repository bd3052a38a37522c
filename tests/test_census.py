"""The per-generation population census (LifeConfig.census) on the CPU tier:
the serial oracle's series against a plain NumPy step-and-sum, the CPU engine
against the oracle (both layouts, every block size, deep-halo epochs whose
blocks compute halo rows that hold live cells, the drift emulation, odd byte
widths), decompositions, the callback transport's sum over gloo, other rules
and the bounded plane, termination, chunked runs, the CLIs, the checkpoints, and
the untouched default."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation, life_step_numpy, random_grid, reference_run, simulate
from gol_amd.parallel import InProcessGroup
from gol_amd.utils import io
from gol_amd.utils.checkpoint import load_checkpoint, run_with_checkpoints, save_checkpoint
from test_boundary import TERMINATION

REPO = Path(__file__).resolve().parents[1]
TMAX = [1, 2, 4, 8, 12, 16]


def oracle(g, gens, **kw):
    """(final grid, series) of the exact serial loop without the similarity
    stop.  The loop still ends on an empty grid, which stays empty: zeros from
    there."""
    out, n, _, pop = reference_run(g, gens, False, census=True, **kw)
    assert pop.dtype == np.int64 and len(pop) == n and (n == gens or not out.any())
    return out, np.concatenate([pop, np.zeros(gens - n, dtype=np.int64)])


# ---- 1. the oracle itself ---------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"rule": "B36/S23"}, {"boundary": "dead"}])
def test_reference_series_vs_numpy_step_and_sum(native, kw):
    g = random_grid(48, 40, 3, 0.4)
    out, pop = oracle(g, 30, **kw)
    x, want = g, []
    for _ in range(30):
        x = life_step_numpy(x, 1, **kw)
        want.append(int(x.sum()))
    assert pop.tolist() == want and (out == x).all()
    assert len(set(want)) > 10  # a curve, not a constant
    # without the flag the call returns what it always did
    assert len(reference_run(g, 30, False, **kw)) == 3


def test_reference_series_stops_with_the_loop(native):
    g = np.zeros((16, 16), dtype=np.uint8)
    g[3, 3:5] = 1  # two cells: dead after one generation
    out, gens, _, pop = reference_run(g, 100, census=True)
    assert gens == 1 and pop.tolist() == [0] and not out.any()


# ---- 2. the CPU engine against the oracle ---------------------------------------------------------
def run_cpu(g, gens, layout, tmax, epoch=0, tune=None, **kw):
    H, W = g.shape
    cfg = LifeConfig(W, H, gen_limit=10**6, check_similarity=False, layout=layout, tmax=tmax, epoch=epoch,
                     census=True, tune=tune or {}, **kw)
    sim = Simulation(cfg, engine="cpu")
    sim.load(g)
    rep = sim.advance(gens)
    return sim, rep


@pytest.mark.parametrize("drift", ["0", "1"])
@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("tmax", TMAX)
@pytest.mark.parametrize("W,layout", [(96, "bits"), (96, "u8")])
def test_cpu_engine_vs_oracle(native, W, layout, tmax, deep, drift):
    """epoch = 2 tmax: the first block of every epoch computes tmax halo rows
    above and below the tile, which hold live cells and are not counted."""
    g = random_grid(W, 70, 11 + tmax, 0.4)
    gens = 3 * tmax + 1
    sim, rep = run_cpu(g, gens, layout, tmax, 2 * tmax if deep else 0, {"cpu_drift": drift})
    want_out, want = oracle(g, gens)
    assert rep.population.dtype == np.int64
    assert rep.population.tolist() == want.tolist()
    assert (sim.tile() == want_out).all()
    assert sim.alive_count() == want[-1]
    d = sim.describe()
    assert d["census"] is True and "census" in d["kernel"]
    assert d["epoch"] == (2 * tmax if deep else d["epoch"])


@pytest.mark.parametrize("W", [33, 257, 1999])
def test_cpu_engine_odd_byte_widths(native, W):
    """The bits beyond W in the last word are not counted."""
    g = random_grid(W, 37, W, 0.4)
    for tmax, epoch in ((8, 16), (16, 0)):
        sim, rep = run_cpu(g, 3 * tmax + 1, "u8", tmax, epoch)
        want_out, want = oracle(g, 3 * tmax + 1)
        assert rep.population.tolist() == want.tolist(), (tmax, epoch)
        assert (sim.tile() == want_out).all()


def test_cpu_ring(native):
    g = random_grid(256, 128, 4, 0.4)
    sim, rep = run_cpu(g, 40, "bits", 8, tune={"cpu_ring": "1"})
    assert sim.describe()["row_ring"] is True
    assert rep.population.tolist() == oracle(g, 40)[1].tolist()


# ---- 3. ranks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,P,W,H,layout", [("2x2", 4, 128, 70, "bits"), ("1x3", 3, 96, 70, "u8"),
                                               ("3x1", 3, 96, 70, "u8")])
def test_cpu_decompositions_report_the_global_series(native, tune, spec, P, W, H, layout):
    g = random_grid(W, H, 77, 0.4)
    gens = 35
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, decomp=spec, layout=layout, tmax=8, epoch=16, census=True,
                                    tune=tune), P, engine="cpu")
    grp.load(g)
    reps = grp.advance(gens)
    want_out, want = oracle(g, gens)
    assert len(reps) == P
    for rep in reps:  # every rank: the sum over ranks, not its share
        assert rep.population.tolist() == want.tolist()
    assert (grp.gather() == want_out).all()


def test_gloo_callback_transport_sums(native, tmp_path):
    """Two rank processes over gloo: the series goes through the callback
    transport's torch.distributed SUM on int64."""
    W, H, gens = 128, 96, 60
    g = random_grid(W, H, 31, 0.4)
    io.write_grid(str(tmp_path / "in.txt"), g)
    env = dict(os.environ, PYTHONPATH=str(REPO) + os.pathsep + os.environ.get("PYTHONPATH", ""),
               GOL_HOST_THREADS="2", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node=2", "--standalone",
           "--local-addr=127.0.0.1", "-m", "gol_amd", str(W), str(H), "in.txt", "--engine", "cpu", "--gens", str(gens),
           "--no-similarity", "--decomp", "1x2", "--comm", "torch", "--epoch", "9", "--census", "pop.csv",
           "--metrics-json", "m.json", "--output", "out.txt", "--style", "mpi"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want_out, want = oracle(g, gens)
    assert (tmp_path / "out.txt").read_text() == io.format_text(want_out)
    lines = (tmp_path / "pop.csv").read_text().splitlines()
    assert lines == [f"{i + 1},{v}" for i, v in enumerate(want.tolist())]
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["census"] is True and m["population"] == want.tolist() and m["ranks"] == 2


# ---- 4. other rules and the bounded plane, on cpu and ref ------------------------------------------------
@pytest.mark.parametrize("layout", ["bits", "u8"])
@pytest.mark.parametrize("kw", [{"rule": "B36/S23"}, {"boundary": "dead"}, {"rule": "B3678/S34678", "boundary": "dead"}])
def test_cpu_other_rules_and_the_plane(native, layout, kw):
    g = random_grid(96, 70, 9, 0.4)
    for tmax, epoch in ((8, 16), (16, 0)):
        gens = 3 * tmax + 1
        sim, rep = run_cpu(g, gens, layout, tmax, epoch, **kw)
        want_out, want = oracle(g, gens, **kw)
        assert rep.population.tolist() == want.tolist(), (tmax, epoch)
        assert (sim.tile() == want_out).all()
        assert rep.population.tolist() != oracle(g, gens)[1].tolist()  # cannot pass as B3/S23 on the torus


# ---- 5. termination ------------------------------------------------------------------------------------
def two_cells():
    g = np.zeros((64, 64), dtype=np.uint8)
    g[5, 5:7] = 1
    return g


def soup_that_settles():
    return random_grid(64, 32, 11, 0.2)  # stops by similarity before generation 1000 on the torus


@pytest.mark.parametrize("boundary", ["torus", "dead"])
@pytest.mark.parametrize("grid", [t[0] for t in TERMINATION] + [two_cells, soup_that_settles])
def test_termination_series(native, grid, boundary):
    """Whatever stops the run: the series has generation() - g0 entries (the
    engine may have evaluated a few generations past the reported stop, and
    keeps them), it is the oracle's series of that many generations, its last
    entry is alive_count(), and an extinct grid ends it in 0."""
    g = grid()
    H, W = g.shape
    for layout, tmax, poll in (("bits", 0, 0), ("u8", 4, 7), ("bits", 16, 1000)):
        sim = Simulation(LifeConfig(W, H, gen_limit=1000, layout=layout, tmax=tmax, poll_gens=poll, census=True,
                                    boundary=boundary), engine="cpu")
        sim.load(g)
        rep = sim.run()
        n = sim.generation
        assert len(rep.population) == n and n >= rep.generations
        assert rep.population.tolist() == oracle(g, n, boundary=boundary)[1].tolist()
        assert rep.population[-1] == sim.alive_count()
        plain = simulate(g, 1000, engine="cpu", layout=layout, tmax=tmax, poll_gens=poll, boundary=boundary)[1]
        assert (rep.generations, rep.stop_reason) == (plain.generations, plain.stop_reason)
        if rep.stop_reason == "extinction":
            assert rep.population[-1] == 0
    if grid is two_cells:
        assert rep.stop_reason == "extinction"
    if grid is soup_that_settles and boundary == "torus":
        assert rep.stop_reason == "similarity"


def test_run_until_from_a_later_generation(native):
    g = random_grid(96, 64, 8, 0.4)
    sim = Simulation(LifeConfig(96, 64, gen_limit=500, check_similarity=False, census=True), engine="cpu")
    sim.load(g)
    sim.advance(13)
    r = sim.native_engine.run_until(50)
    assert sim.generation == 50 and len(r.population) == 37
    assert np.asarray(r.population).tolist() == oracle(g, 50)[1][13:].tolist()


# ---- 6. chunked runs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,tune", [("bits", {}), ("u8", {}), ("bits", {"cpu_ring": "1", "cpu_drift": "1"})])
def test_chunked_equals_whole(native, layout, tune):
    g = random_grid(128, 64, 21, 0.4)
    cfg = dict(gen_limit=10**6, check_similarity=False, layout=layout, census=True, tune=tune)
    whole = Simulation(LifeConfig(128, 64, **cfg), engine="cpu")
    whole.load(g)
    want = whole.advance(100).population
    parts = Simulation(LifeConfig(128, 64, **cfg), engine="cpu")
    parts.load(g)
    got = np.concatenate([parts.advance(n).population for n in (37, 5, 58)])
    assert got.tolist() == want.tolist() == oracle(g, 100)[1].tolist()
    assert (parts.tile() == whole.tile()).all()


def test_run_with_checkpoints_concatenates(native, tmp_path):
    g = random_grid(96, 64, 3, 0.3)
    sim = Simulation(LifeConfig(96, 64, gen_limit=50, check_similarity=False, census=True), engine="cpu")
    sim.load(g)
    rep = run_with_checkpoints(sim, 7, str(tmp_path / "ck"))
    assert rep.population.tolist() == oracle(g, 50)[1].tolist()


# ---- 7. census off ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_census_off_is_untouched(native, layout):
    assert LifeConfig(64, 64).census is False and native.EngineConfig().census is False
    g = random_grid(96, 64, 8, 0.3)
    off_out, off = simulate(g, 300, engine="cpu", layout=layout)
    on_out, on = simulate(g, 300, engine="cpu", layout=layout, census=True)
    assert off.population.dtype == np.int64 and len(off.population) == 0
    assert len(on.population) > 0
    assert (off_out == on_out).all()
    for f in ("generations", "executed", "stop_reason", "first_unchanged", "extinct", "exchanges", "polls",
              "kernel_launches"):
        assert getattr(off, f) == getattr(on, f), f
    assert "population" not in off.as_dict() and "population" not in on.as_dict()
    d = Simulation(LifeConfig(64, 64, layout=layout), engine="cpu").describe()
    assert d["census"] is False and "census" not in d["kernel"]


def test_refusals_that_need_no_gpu(native):
    with pytest.raises(RuntimeError, match="census=1 with self_exchange"):
        Simulation(LifeConfig(64, 64, census=True, self_exchange=True), engine="cpu")
    with pytest.raises(RuntimeError, match="census=1 with graphs=1"):
        Simulation(LifeConfig(64, 64, census=True, graphs="on"), engine="cpu")
    be = native.cpu_backend(1)
    assert be.supports_census(native.Layout.Bits, "B36/S23", "dead")


# ---- 8. CLIs and checkpoints -----------------------------------------------------------------------------
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
def test_cli_census_file_and_metrics(native, gol_bin, tmp_path, front):
    run = (lambda a: _gol(gol_bin, a, tmp_path)) if front == "gol" else (lambda a: _py(a, tmp_path))
    assert "--census" in run(["--help"]).stdout
    g = random_grid(64, 64, 3, 0.3)
    io.write_grid(str(tmp_path / "in.txt"), g)
    want = [f"{i + 1},{v}" for i, v in enumerate(oracle(g, 40)[1].tolist())]
    for engine in ("cpu", "ref"):
        run([64, 64, "in.txt", "--engine", engine, "--gens", 40, "--no-similarity", "--census", f"{engine}.csv",
             "--output", "none", "--metrics-json", f"{engine}.json"])
        assert (tmp_path / f"{engine}.csv").read_text().splitlines() == want, engine
    m = json.loads((tmp_path / "cpu.json").read_text())
    assert m["census"] is True and m["population"] == oracle(g, 40)[1].tolist()
    # without the flag the metrics carry no series
    run([64, 64, "in.txt", "--engine", "cpu", "--gens", 40, "--output", "none", "--metrics-json", "off.json"])
    assert "population" not in json.loads((tmp_path / "off.json").read_text())
    # a run that stops early writes the generations it advanced through
    io.write_grid(str(tmp_path / "two.txt"), two_cells())
    run([64, 64, "two.txt", "--engine", "cpu", "--census", "two.csv", "--output", "none"])
    lines = (tmp_path / "two.csv").read_text().splitlines()
    assert lines[0] == "1,0" and [ln.split(",")[0] for ln in lines] == [str(i + 1) for i in range(len(lines))]


@pytest.mark.parametrize("front", ["gol", "py"])
def test_checkpoint_carries_the_census(native, gol_bin, tmp_path, front):
    run = (lambda a: _gol(gol_bin, a, tmp_path)) if front == "gol" else (lambda a: _py(a, tmp_path))
    other = (lambda a: _py(a, tmp_path)) if front == "gol" else (lambda a: _gol(gol_bin, a, tmp_path))
    W, H = 96, 64
    g = random_grid(W, H, 3, 0.3)
    io.write_grid(str(tmp_path / "in.txt"), g)
    want = oracle(g, 50)[1].tolist()
    run([W, H, "in.txt", "--engine", "cpu", "--no-similarity", "--census", "a.csv", "--gens", 20,
         "--checkpoint-every", 7, "--checkpoint-dir", "ck", "--output", "none"])
    # chunked by the checkpoints, the file is the whole run's series
    assert (tmp_path / "a.csv").read_text().splitlines() == [f"{i + 1},{v}" for i, v in enumerate(want[:20])]
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["generation"] == 14 and meta["census"] is True
    # the default leaves meta.json as it always was
    run([W, H, "in.txt", "--engine", "cpu", "--no-similarity", "--gens", 20, "--checkpoint-every", 7,
         "--checkpoint-dir", "ck0", "--output", "none"])
    assert "census" not in json.loads((tmp_path / "ck0" / "meta.json").read_text())
    # a resume takes the setting from the checkpoint and counts from the checkpoint's generation; either front end
    for f, name in ((run, "b"), (other, "c")):
        f([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--census", f"{name}.csv", "--output", "none",
           "--metrics-json", f"{name}.json"])
        assert (tmp_path / f"{name}.csv").read_text().splitlines() == [f"{i + 1},{want[i]}" for i in range(14, 50)]
        f([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--output", "none", "--metrics-json", f"{name}.json"])
        assert json.loads((tmp_path / f"{name}.json").read_text())["population"] == want[14:]


def test_checkpoint_api_carries_the_census(native, tmp_path):
    g = random_grid(64, 64, 5, 0.3)
    sim = Simulation(LifeConfig(64, 64, gen_limit=80, check_similarity=False, census=True), engine="cpu")
    sim.load(g)
    first = sim.native_engine.run_until(30)
    save_checkpoint(sim, str(tmp_path / "ck"))
    cfg, grid = load_checkpoint(str(tmp_path / "ck"))
    assert cfg.census is True and cfg.start_gen == 30
    sim2 = Simulation(cfg, engine="cpu")
    sim2.load_text(str(grid))
    rep = sim2.run()
    want = oracle(g, 80)[1].tolist()
    assert np.asarray(first.population).tolist() == want[:30] and rep.population.tolist() == want[30:]
    # the series is not in the checkpoint
    assert "population" not in json.loads((tmp_path / "ck" / "meta.json").read_text())
    off = Simulation(LifeConfig(64, 64), engine="cpu")
    off.load(g)
    save_checkpoint(off, str(tmp_path / "ck0"))
    assert load_checkpoint(str(tmp_path / "ck0"))[0].census is False
