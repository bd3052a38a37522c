"""Quiet-tile skipping (csrc/include/gol/quiet.hpp, tuning quiet_skip): a
workgroup of the skipping kernel leaves its tile alone when the tile and its
light cone are what they were 12 generations ago.  Skipping is exact, so every
test compares cells, stop generations and reasons with the fp32 PyTorch
oracle, the CPU backend and a quiet_skip=0 run, and asserts that some waves
skipped and not all did (no test passes vacuously).

The reference has no counterpart (every generation rewrites every cell,
src/game_cuda.cu:128-148)."""
import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation
from gol_amd.ops.life_ops import life_step_torch_roll
from gol_amd.utils.checkpoint import load_checkpoint, save_checkpoint

pytestmark = pytest.mark.gpu

# 5120 cells = 160 words: two full 62-word strips and a narrow one; 768 rows in
# 4-wave groups of 96 rows: eight groups per strip.
W, H = 5120, 768
TUNE = {"quiet_skip": "1", "group": "4", "quiet_rows": "96"}
STRIP = 62 * 32  # cells per full column strip
GROUP = 96       # rows per group

BLOCK = ["11", "11"]
BLINKER = ["111"]
GLIDER_SE = [".1.", "..1", "111"]
GLIDER_NW = ["111", "1..", ".1."]
RPENT = [".11", "11.", ".1."]
PENTADECATHLON = ["..1....1..", "11.1111.11", "..1....1.."]
PULSAR = ["..111...111..", ".............", "1....1.1....1", "1....1.1....1", "1....1.1....1", "..111...111..",
          ".............", "..111...111..", "1....1.1....1", "1....1.1....1", "1....1.1....1", ".............",
          "..111...111.."]


def put(g, y, x, pat):
    for dy, row in enumerate(pat):
        for dx, c in enumerate(row):
            if c == "1":
                g[(y + dy) % g.shape[0], (x + dx) % g.shape[1]] = 1


def ash(still_only=False, seed=5):
    """Blocks and blinkers on a 16-cell lattice (about every third site)."""
    g = np.zeros((H, W), np.uint8)
    rng = np.random.default_rng(seed)
    for y in range(4, H - 8, 16):
        for x in range(4, W - 8, 16):
            r = rng.integers(0, 6)
            if r == 0:
                put(g, y, x, BLOCK)
            elif r == 1 and not still_only:
                put(g, y, x, BLINKER)
    return g


def clear(g, y0, y1, x0, x1):
    g[np.ix_(np.arange(y0, y1) % H, np.arange(x0, x1) % W)] = 0


@pytest.fixture(scope="module")
def field():
    g = ash()
    clear(g, 180, 230, 2500, 2550)
    put(g, 198, 2518, PULSAR)           # p3: settles (3 divides 12)
    clear(g, 400, 440, 700, 750)
    put(g, 418, 720, PENTADECATHLON)    # p15: never settles
    clear(g, 560, 620, 3300, 3360)
    put(g, 588, 3328, RPENT)
    # Gliders across a strip boundary, a group boundary, the row seam and the
    # column wrap, both ways.
    for y, x, pat in [(300, STRIP - 6, GLIDER_SE), (330, STRIP + 4, GLIDER_NW),
                      (2 * GROUP - 6, 1000, GLIDER_SE), (3 * GROUP + 4, 1100, GLIDER_NW),
                      (H - 6, 4000, GLIDER_SE), (3, 4100, GLIDER_NW),
                      (500, W - 6, GLIDER_SE), (530, 3, GLIDER_NW)]:
        clear(g, y - 12, y + 16, x - 12, x + 16)
        put(g, y, x, pat)
    return g


CHECK_GENS = (7, 100, 355, 600)  # none a multiple of 12


@pytest.fixture(scope="module")
def oracle(field):
    """The field at CHECK_GENS from the fp32 PyTorch oracle, computed once."""
    out, cur, at = {}, field, 0
    for g in CHECK_GENS:
        cur = life_step_torch_roll(cur, g - at, device="cuda")
        out[g], at = cur, g
    return out


def sim_of(tune, layout="bits", gen_limit=100000, **kw):
    return Simulation(LifeConfig(W, H, gen_limit=gen_limit, layout=layout, tune=dict(tune), **kw), engine="hip")


def skipped_some_not_all(sim):
    d = sim.describe()
    assert d["quiet_mode"] == "on" and d["quiet_blocks"]["skip"] > 0, d["quiet_mode"]
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"], (d["quiet_waves_skipped"], d["quiet_waves_launched"])
    return d


@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_skipping_is_exact_vs_torch_and_unskipped_run(gpu, field, oracle, layout):
    """Bit layout, and the byte layout on its bit image."""
    sim, plain = sim_of(TUNE, layout), sim_of({**TUNE, "quiet_skip": "0"}, layout)
    assert sim.describe()["row_ring"] and sim.describe()["tmax"] == 12
    sim.load(field)
    plain.load(field)
    for g in CHECK_GENS:
        sim.native_engine.run_until(g)
        plain.native_engine.run_until(g)
        got = sim.tile()
        assert np.array_equal(got, oracle[g]), g
        assert np.array_equal(got, plain.tile()), g
    d = skipped_some_not_all(sim)
    # Most of the field is ash: by the end most waves skip.
    assert d["quiet_waves_skipped"] > d["quiet_waves_launched"] // 4
    assert plain.describe()["quiet_mode"] == "off" and plain.describe()["quiet_waves_launched"] == 0


# A 24 x 24 soup of density 0.35 from numpy's default_rng(SOUP_SEED) on a
# background of blocks: found on the CPU backend, it freezes at generation
# SOUP_FIXED, long after the blocks around it went quiet.
SOUP_SEED, SOUP_FIXED = 57, 456


def soup_field():
    g = ash(still_only=True)
    clear(g, 330, 440, 2400, 2520)
    rng = np.random.default_rng(SOUP_SEED)
    g[372:396, 2448:2472] = rng.random((24, 24)) < 0.35
    return g


def test_stop_generation_and_reason_are_exact(gpu):
    g = soup_field()
    reps = {}
    for name, kw in (("cpu", dict(engine="cpu")), ("skip", dict(engine="hip")), ("plain", dict(engine="hip"))):
        tune = dict(TUNE, quiet_skip="0") if name == "plain" else dict(TUNE)
        sim = Simulation(LifeConfig(W, H, gen_limit=3000, tune={} if name == "cpu" else tune), **kw)
        sim.load(g)
        rep = sim.run()
        reps[name] = (rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct)
        if name == "skip":
            skipped_some_not_all(sim)
            out = sim.tile()
        elif name == "cpu":
            want = sim.tile()
    assert reps["cpu"][1] == "similarity" and reps["cpu"][2] == SOUP_FIXED
    assert reps["skip"] == reps["cpu"] == reps["plain"], reps
    assert np.array_equal(out, want)


@pytest.mark.parametrize("event", ["load", "store_rows", "checkpoint", "step_of_7", "step_of_1000"])
def test_everything_that_touches_the_grid_invalidates(gpu, field, oracle, event, tmp_path):
    sim = sim_of(TUNE)
    sim.load(field)
    eng = sim.native_engine
    if event == "load":
        # Settle on another field first: its clean tiles must not survive the load.
        sim.load(ash(seed=9))
        eng.run_until(240)
        sim.load(field)
        eng.generation = 0
        for g in CHECK_GENS:
            eng.run_until(g)
            assert np.array_equal(sim.tile(), oracle[g]), g
    elif event == "store_rows":
        for g in CHECK_GENS:
            eng.run_until(g - 3)
            band = eng.store_rows(GROUP - 5, 40)
            eng.run_until(g)
            assert np.array_equal(sim.tile(), oracle[g]), g
            if g == CHECK_GENS[0]:
                assert band.shape == (40, W)
    elif event == "checkpoint":
        eng.run_until(355)
        save_checkpoint(sim, str(tmp_path / "ck"))
        eng.run_until(600)
        assert np.array_equal(sim.tile(), oracle[600])
        cfg, grid = load_checkpoint(str(tmp_path / "ck"))
        assert cfg.start_gen == 355
        cfg.gen_limit, cfg.tune = 100000, dict(TUNE)
        sim2 = Simulation(cfg, engine="hip")
        sim2.load_text(str(grid))
        sim2.native_engine.run_until(600)
        assert np.array_equal(sim2.tile(), oracle[600])
        skipped_some_not_all(sim2)
    elif event == "step_of_7":
        eng.run_until(240)  # 20 blocks of 12: most tiles skip by now
        eng.run_until(247)  # blocks of 4, 2 and 1 generations
        for g in (355, 600):
            eng.run_until(g)
            assert np.array_equal(sim.tile(), oracle[g]), g
    else:
        # 1000 = 83 blocks of 12 and the 4-generation remainder block.
        eng.run_until(355)
        assert np.array_equal(sim.tile(), oracle[355])
        eng.run_until(1355)
        assert np.array_equal(sim.tile(), life_step_torch_roll(oracle[600], 1355 - 600, device="cuda"))
    skipped_some_not_all(sim)
