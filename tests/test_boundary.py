"""The bounded plane (boundary="dead") on the CPU tier: the oracles against
each other, the CPU backend against the NumPy oracle, decompositions, closed
forms that need no oracle code, termination against the serial loop, the CLIs,
the checkpoints, and the untouched default."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation, life_step, life_step_numpy, random_grid, reference_run, simulate
from gol_amd.ops.life_ops import life_step_torch, life_step_torch_roll
from gol_amd.parallel import InProcessGroup
from gol_amd.utils import io
from gol_amd.utils.checkpoint import load_checkpoint, save_checkpoint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the oracles agree with each other ------------------------------------------
@pytest.mark.parametrize("W,H,min_diff", [(70, 41, 75), (33, 33, 1)])
def test_oracles_agree_and_differ_from_the_torus(native, W, H, min_diff):
    """One generation changes only cells on the grid's edge (2 (W + H) - 4 of
    them).  On 70 x 41 at density 0.4 the plane and the torus differ in 75 or
    more cells (89 to 121 over twenty seeds).  A 33 x 33 grid has 128 edge cells
    and differs in 39 to 70, so there only "differs, and only on the edge" is
    asserted."""
    g = random_grid(W, H, 3, 0.4)
    one_dead, one_torus = life_step_numpy(g, 1, boundary="dead"), life_step_numpy(g, 1)
    diff = one_dead != one_torus
    print(f"{W}x{H}: plane and torus differ in {int(diff.sum())} cells after one generation")
    assert diff.sum() >= min_diff
    assert not diff[1:-1, 1:-1].any()
    want = life_step_numpy(g, 6, boundary="dead")
    got = {"torch": (life_step_torch(g, 6, boundary="dead"), life_step_torch(g, 6)),
           "torch_roll": (life_step_torch_roll(g, 6, boundary="dead"), life_step_torch_roll(g, 6)),
           "reference_run": (reference_run(g, 6, False, boundary="dead")[0], reference_run(g, 6, False)[0]),
           "numpy": (want, life_step_numpy(g, 6))}
    for name, (dead, torus) in got.items():
        assert (dead == want).all(), name
        assert (torus == got["numpy"][1]).all(), name
        assert (dead != torus).any(), name  # cannot pass on a torus
    with pytest.raises(ValueError):
        life_step_numpy(g, 1, boundary="moat")


def test_a_moat_is_not_a_plane(native):
    """Why the edge is enforced inside the generations: a torus padded with
    dead cells lets cells be born in the padding."""
    g = np.zeros((8, 8), dtype=np.uint8)
    g[0, 2:5] = 1  # a blinker on the edge row
    moat = life_step_numpy(np.pad(g, 4), 2)[4:-4, 4:-4]
    assert moat.any() and not life_step_numpy(g, 2, boundary="dead").any()


# ---- 2. the CPU backend against the NumPy oracle ----------------------------------------
SHAPES = [(64, 5, "bits"), (64, 5, "u8"), (96, 70, "bits"), (96, 70, "u8"), (33, 33, "u8"), (257, 129, "u8"),
          (32, 1, "bits"), (1, 1, "u8"), (2, 3, "u8")]


@pytest.mark.parametrize("tmax", [1, 8, 16])
@pytest.mark.parametrize("W,H,layout", SHAPES)
def test_cpu_backend_vs_numpy(native, W, H, layout, tmax):
    gens = 2 * tmax + 3
    g = random_grid(W, H, 5 + tmax, 0.4)
    out = life_step(g, gens, engine="cpu", layout=layout, tmax=tmax, boundary="dead")
    assert (out == life_step_numpy(g, gens, boundary="dead")).all()
    if W * H > 64:
        assert not (out == life_step_numpy(g, gens)).all()


@pytest.mark.parametrize("layout", ["bits", "u8"])
@pytest.mark.parametrize("rule", ["B3678/S34678", "B2/S"])
def test_cpu_backend_other_rules(native, rule, layout):
    g = random_grid(96, 70, 9, 0.4)
    for tmax in (1, 8, 16):
        gens = 2 * tmax + 3
        out = life_step(g, gens, engine="cpu", layout=layout, tmax=tmax, rule=rule, boundary="dead")
        assert (out == life_step_numpy(g, gens, rule=rule, boundary="dead")).all()


# ---- 3. decompositions -----------------------------------------------------------------------
@pytest.mark.parametrize("spec,P,W,H,layout", [("2x2", 4, 128, 70, "bits"), ("1x3", 3, 96, 70, "u8"),
                                               ("3x1", 3, 96, 70, "u8")])
def test_cpu_decompositions(native, tune, spec, P, W, H, layout):
    """Corner ranks, a rank with both neighbours real, and P == 2, where the
    torus's west and east (north and south) neighbour are one rank and the
    plane keeps one of the two."""
    g = random_grid(W, H, 77, 0.4)
    gens = 35
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, decomp=spec, layout=layout, tmax=8, boundary="dead",
                                    tune=tune), P, engine="cpu")
    grp.load(g)
    grp.advance(gens)
    assert (grp.gather() == life_step_numpy(g, gens, boundary="dead")).all()


def test_plane_neighbours(native):
    d = native.Decomposition.make(128, 70, 4, "2x2", 32)
    assert list(d.neighbors(0)) == list(d.neighbors(0, False))
    N, S, Wd, E = 0, 1, 2, 3
    nb = [list(d.neighbors(r, True)) for r in range(4)]
    assert (nb[0][N], nb[0][S], nb[0][Wd], nb[0][E]) == (-1, 2, -1, 1)
    assert (nb[3][N], nb[3][S], nb[3][Wd], nb[3][E]) == (1, -1, 2, -1)
    assert nb[0][4:] == [-1, -1, -1, 3] and nb[3][4:] == [0, -1, -1, -1]
    mid = list(native.Decomposition.make(96, 70, 3, "1x3", 32).neighbors(1, True))
    assert (mid[N], mid[S], mid[Wd], mid[E]) == (0, 2, -1, -1)


# ---- 4. closed forms, no oracle code --------------------------------------------------------------
def blinker_row0():
    g = np.zeros((64, 64), dtype=np.uint8)
    g[0, 10:13] = 1
    return g


def blinker_col0():
    g = np.zeros((64, 64), dtype=np.uint8)
    g[10:13, 0] = 1
    return g


def glider(H=64, W=64):
    g = np.zeros((H, W), dtype=np.uint8)
    for r, c in ((1, 2), (2, 3), (3, 1), (3, 2), (3, 3)):
        g[r, c] = 1
    return g


def block_at(H, W, r, c):
    g = np.zeros((H, W), dtype=np.uint8)
    g[r:r + 2, c:c + 2] = 1
    return g


@pytest.mark.parametrize("grid", [blinker_row0, blinker_col0])
@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_edge_blinker_dies(native, grid, layout):
    g = grid()
    for gens in (1, 2, 3):
        out = life_step(g, gens, engine="cpu", layout=layout, boundary="dead")
        assert out.any() == (gens < 2), gens  # empty from generation 2
    out, rep = simulate(g, 1000, engine="cpu", layout=layout, boundary="dead")
    assert rep.stop_reason == "extinction" and not out.any()
    out, rep = simulate(g, 1000, engine="cpu", layout=layout)
    assert rep.stop_reason == "limit" and out.sum() == 3


@pytest.mark.parametrize("H,block,first", [(64, (62, 62), 244), (32, (30, 30), 116)])
@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_glider_runs_into_the_corner(native, layout, H, block, first):
    g = glider(H, 64)
    out, rep = simulate(g, 1000, engine="cpu", layout=layout, boundary="dead")
    assert rep.stop_reason == "similarity" and rep.first_unchanged == first
    assert (out == block_at(H, 64, *block)).all()
    out, rep = simulate(g, 1000, engine="cpu", layout=layout)
    assert rep.stop_reason == "limit" and out.sum() == 5


def reference_outcome(g, limit=1000):
    ref, gens, _ = reference_run(g, limit, boundary="dead")
    if gens < limit:
        return ref, gens, "extinction" if not ref.any() else "similarity"
    return ref, gens, "fixed_point" if (life_step_numpy(ref, 1, boundary="dead") == ref).all() else "limit"


# (grid, the reason the serial loop itself must show)
TERMINATION = [(blinker_row0, "extinction"), (blinker_col0, "extinction"), (glider, "similarity")]


@pytest.mark.parametrize("grid,reason", TERMINATION)
def test_termination_vs_reference(native, grid, reason):
    g = grid()
    ref, rgens, rreason = reference_outcome(g)
    assert rreason == reason, (rreason, rgens)
    for layout, tmax, poll in (("bits", 0, 0), ("u8", 4, 7), ("bits", 16, 1000)):
        out, rep = simulate(g, 1000, engine="cpu", layout=layout, tmax=tmax, poll_gens=poll, boundary="dead")
        assert (rep.generations, rep.stop_reason) == (rgens, reason), (layout, tmax, poll)
        assert (out == ref).all()


# ---- 5. CLIs and checkpoints ---------------------------------------------------------------------
def _gol(gol_bin, args, cwd, ok=True):
    r = subprocess.run([str(gol_bin), *map(str, args)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _py(args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=REPO, GOL_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-m", "gol_amd", *map(str, args)], cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _gens(stdout):
    return int(next(ln for ln in stdout.splitlines() if ln.startswith("Generations")).split()[-1])


def test_cli_boundary_cpu_equals_ref(native, gol_bin, tmp_path):
    g = random_grid(64, 64, 3, 0.3)
    io.write_grid(str(tmp_path / "in.txt"), g)
    want = life_step_numpy(g, 40, boundary="dead")
    assert not (want == life_step_numpy(g, 40)).all()
    outs = {}
    for run, name in ((_gol, "gol"), (_py, "py")):
        for engine in ("cpu", "ref"):
            args = [64, 64, "in.txt", "--boundary", "dead", "--engine", engine, "--gens", 40, "--no-similarity",
                    "--output", f"{name}_{engine}.out"]
            r = run(gol_bin, args, tmp_path) if run is _gol else run(args, tmp_path)
            assert _gens(r.stdout) == 40
            outs[name, engine] = (tmp_path / f"{name}_{engine}.out").read_bytes()
    assert len(set(outs.values())) == 1
    assert (io.read_grid(str(tmp_path / "gol_cpu.out"), 64, 64) == want).all()


def test_cli_help_and_metrics_name_the_boundary(native, gol_bin, tmp_path):
    assert "--boundary" in _gol(gol_bin, ["--help"], tmp_path).stdout
    assert "--boundary" in _py(["--help"], tmp_path).stdout
    for run, name in ((_gol, "gol"), (_py, "py")):
        for flag, want in ((["--boundary", "dead"], "dead"), ([], "torus")):
            args = [64, 64, "--random", 5, *flag, "--engine", "cpu", "--gens", 5, "--output", "none",
                    "--metrics-json", f"{name}.json"]
            run(gol_bin, args, tmp_path) if run is _gol else run(args, tmp_path)
            assert json.loads((tmp_path / f"{name}.json").read_text())["boundary"] == want
    bad = _gol(gol_bin, [64, 64, "--random", 5, "--boundary", "moat", "--engine", "cpu"], tmp_path, ok=False)
    assert "moat" in bad.stderr
    _py([64, 64, "--random", 5, "--boundary", "moat", "--engine", "cpu"], tmp_path, ok=False)


@pytest.mark.parametrize("front", ["gol", "py"])
def test_checkpoint_carries_the_boundary(native, gol_bin, tmp_path, front):
    run = (lambda a, ok=True: _gol(gol_bin, a, tmp_path, ok)) if front == "gol" else (
        lambda a, ok=True: _py(a, tmp_path, ok))
    W, H = 96, 64
    g = random_grid(W, H, 3, 0.3)
    io.write_grid(str(tmp_path / "in.txt"), g)
    ref, rgens, _ = reference_run(g, 50, boundary="dead")
    assert rgens == 50 and not (ref == reference_run(g, 50)[0]).all()
    run([W, H, "in.txt", "--engine", "cpu", "--boundary", "dead", "--gens", 20, "--checkpoint-every", 7,
         "--checkpoint-dir", "ck", "--output", "a.out"])
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["generation"] == 14 and meta["boundary"] == "dead"
    # the default leaves meta.json as it always was, named or not
    run([W, H, "in.txt", "--engine", "cpu", "--gens", 20, "--checkpoint-every", 7, "--checkpoint-dir", "ck0",
         "--output", "a0.out"])
    assert "boundary" not in json.loads((tmp_path / "ck0" / "meta.json").read_text())
    run([W, H, "in.txt", "--engine", "cpu", "--boundary", "torus", "--gens", 20, "--checkpoint-every", 7,
         "--checkpoint-dir", "ck1", "--output", "a1.out"])
    assert (tmp_path / "ck1" / "meta.json").read_bytes() == (tmp_path / "ck0" / "meta.json").read_bytes()
    # a resume takes the boundary from the checkpoint, with or without the same flag
    for extra in ([], ["--boundary", "dead"]):
        out = run([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--output", "b.out", *extra]).stdout
        assert _gens(out) == rgens
        assert (io.read_grid(str(tmp_path / "b.out"), W, H) == ref).all()
    # ... and refuses the other one
    bad = run([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--output", "c.out", "--boundary", "torus"],
              ok=False)
    assert "--boundary dead" in bad.stderr
    # either front end resumes the other's checkpoint
    other = (lambda a: _py(a, tmp_path)) if front == "gol" else (lambda a: _gol(gol_bin, a, tmp_path))
    out = other([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--output", "d.out"]).stdout
    assert _gens(out) == rgens
    assert (io.read_grid(str(tmp_path / "d.out"), W, H) == ref).all()


def test_checkpoint_api_carries_the_boundary(native, tmp_path):
    g = glider()
    ref, rgens, reason = reference_outcome(g)
    assert reason == "similarity"
    sim = Simulation(LifeConfig(64, 64, boundary="dead"), engine="cpu")
    sim.load(g)
    sim.native_engine.run_until(100)
    save_checkpoint(sim, str(tmp_path / "ck"))
    cfg, grid = load_checkpoint(str(tmp_path / "ck"))
    assert cfg.boundary == "dead" and cfg.start_gen == 100
    sim2 = Simulation(cfg, engine="cpu")
    sim2.load_text(str(grid))
    rep = sim2.run()
    assert rep.generations == rgens
    assert (sim2.tile() == ref).all()


# ---- 6. what the plane switches off, and the refusals that need no GPU --------------------------------
def test_describe_on_the_plane(native):
    d = Simulation(LifeConfig(256, 128, boundary="dead", tune={"cpu_ring": "1", "cpu_drift": "1"}),
                   engine="cpu").describe()
    assert d["boundary"] == "dead" and "boundary dead" in d["kernel"]
    assert d["row_ring"] is False and d["drifting"] is False and d["quiet_mode"] == "off"
    assert d["halo_words"] > 0
    torus = Simulation(LifeConfig(256, 128, tune={"cpu_ring": "1", "cpu_drift": "1"}), engine="cpu").describe()
    assert torus["drifting"] is True  # the same tuning drifts on the torus: the plane turned it off


def test_cpu_ring_and_drift_are_off_on_the_plane(native):
    g = random_grid(256, 128, 4, 0.4)
    out = life_step(g, 40, engine="cpu")
    cfg = LifeConfig(256, 128, gen_limit=40, boundary="dead", tune={"cpu_ring": "1", "cpu_drift": "1"})
    sim = Simulation(cfg, engine="cpu")
    sim.load(g)
    sim.advance(40)
    assert (sim.tile() == life_step_numpy(g, 40, boundary="dead")).all()
    assert not (sim.tile() == out).all()


def test_refusals_name_the_combination(native):
    with pytest.raises(RuntimeError, match="boundary=dead with self_exchange"):
        Simulation(LifeConfig(64, 64, boundary="dead", self_exchange=True), engine="cpu")
    with pytest.raises(RuntimeError, match="boundary=dead with graphs=1"):
        Simulation(LifeConfig(64, 64, boundary="dead", graphs="on"), engine="cpu")
    with pytest.raises(RuntimeError, match="moat"):
        Simulation(LifeConfig(64, 64, boundary="moat"), engine="cpu")


# ---- 7. the default is untouched ------------------------------------------------------------------
def test_default_boundary_untouched(native):
    assert LifeConfig(64, 64).to_native().boundary == "torus"
    assert native.EngineConfig().boundary == "torus"
    g = random_grid(96, 64, 8, 0.3)
    plain_out, plain = simulate(g, 300, engine="cpu")
    out, rep = simulate(g, 300, engine="cpu", boundary="torus")
    assert (out == plain_out).all()
    assert (rep.generations, rep.stop_reason) == (plain.generations, plain.stop_reason)
    assert (life_step_numpy(g, 9, boundary="torus") == life_step_numpy(g, 9)).all()
    assert (reference_run(g, 300, boundary="torus")[0] == reference_run(g, 300)[0]).all()
    d = Simulation(LifeConfig(64, 64), engine="cpu").describe()
    assert d["boundary"] == "torus" and "boundary" not in d["kernel"] and "plane" not in d["kernel"]
