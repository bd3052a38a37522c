"""The candidate list of the skipping kernel on the GPU (tuning quiet_list,
quiet_grid; csrc/kernels/life_quiet_impl.hpp): a skipping block launches only
the tiles next to the last block's activity.  Results may not change, so every
test compares cells, stop generations and reasons with the fp32 PyTorch oracle,
the CPU backend, a quiet_list=0 run (one workgroup per tile) and a quiet_skip=0
run, and asserts that the list was short and not empty (no test passes
vacuously).  The field and the helpers are those of tests/test_quiet_skip.py:
5120 x 768 cells, 3 strips x 8 groups = 24 tiles.

The reference has no counterpart (every generation rewrites every cell,
src/game_cuda.cu:128-148)."""
import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation
from gol_amd.ops.life_ops import life_step_torch_roll
from gol_amd.utils.checkpoint import load_checkpoint, save_checkpoint

pytestmark = pytest.mark.gpu

W, H = 5120, 768
TILES = 24
TUNE = {"quiet_skip": "1", "group": "4", "quiet_rows": "96"}
LIST = {**TUNE, "quiet_list": "1"}
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


def listed_some_not_all(sim):
    """The list is on, it is short and not empty, and the waves read as before."""
    d = sim.describe()
    assert d["quiet_mode"] == "on" and d["quiet_list"] is True and d["quiet_blocks"]["skip"] > 0, d["quiet_mode"]
    assert 0 < d["quiet_candidates"] < TILES, d["quiet_candidates"]
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"], (d["quiet_waves_skipped"], d["quiet_waves_launched"])
    return d


@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_list_is_exact_vs_torch_unlisted_and_unskipped_runs(gpu, field, oracle, layout):
    sims = [sim_of(LIST, layout), sim_of({**TUNE, "quiet_list": "0"}, layout), sim_of({**TUNE, "quiet_skip": "0"}, layout)]
    for s in sims:
        s.load(field)
    for g in CHECK_GENS:
        tiles = []
        for s in sims:
            s.native_engine.run_until(g)
            tiles.append(s.tile())
        assert np.array_equal(tiles[0], oracle[g]), g
        assert np.array_equal(tiles[0], tiles[1]) and np.array_equal(tiles[0], tiles[2]), g
    d, d0 = listed_some_not_all(sims[0]), sims[1].describe()
    # Tiles that are not launched count as launched and skipped: the waves read as without the list.
    assert d0["quiet_list"] is False and d0["quiet_candidates"] == -1
    assert d["quiet_waves_launched"] == d0["quiet_waves_launched"]
    assert d["quiet_waves_skipped"] == d0["quiet_waves_skipped"]
    assert d["launch_paths"] == d0["launch_paths"]
    assert sims[2].describe()["quiet_list"] is False


def test_default_is_the_list_where_skipping_is_on(gpu):
    assert sim_of(TUNE).describe()["quiet_list"] is True
    assert sim_of({**TUNE, "quiet_skip": "0"}).describe()["quiet_list"] is False


def test_gliders_reenter_tiles_that_left_the_list(gpu):
    """Gliders start inside quiet regions of still lifes and cross a strip boundary, a group boundary, the row
    seam and the column wrap: 1200 generations move each 300 cells along both axes, across at least two tiles
    that were on no list when it arrived.  One runs into a block."""
    g = ash(still_only=True)
    # A glider travels (dx, dy) = +-(1, 1) per 4 generations; its lane of 330 cells is cleared of the ash.
    starts = [(300, STRIP - 40, GLIDER_SE), (430, STRIP + 40, GLIDER_NW), (2 * GROUP - 30, 900, GLIDER_SE),
              (3 * GROUP + 30, 1300, GLIDER_NW), (H - 40, 4000, GLIDER_SE), (40, 4500, GLIDER_NW),
              (500, W - 40, GLIDER_SE), (700, 40, GLIDER_NW)]
    for y, x, pat in starts:
        s = 1 if pat is GLIDER_SE else -1
        for t in range(0, 331, 8):
            clear(g, y + s * t - 10, y + s * t + 14, x + s * t - 10, x + s * t + 14)
        put(g, y, x, pat)
    put(g, 300 + 150, STRIP - 40 + 151, BLOCK)  # in the first glider's way
    sim, plain = sim_of(LIST), sim_of({**TUNE, "quiet_skip": "0"})
    sim.load(g)
    plain.load(g)
    for gen in (600, 1200):
        sim.native_engine.run_until(gen)
        plain.native_engine.run_until(gen)
        assert np.array_equal(sim.tile(), plain.tile()), gen
    assert np.array_equal(sim.tile(), life_step_torch_roll(g, 1200, device="cuda"))
    # Gliders in six of the eight groups: their neighbourhoods may well cover every tile at the end.
    d = sim.describe()
    assert d["quiet_list"] is True and 0 < d["quiet_candidates"] <= TILES
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]


SOUP_SEED, SOUP_FIXED = 57, 456


def soup_field():
    g = ash(still_only=True)
    clear(g, 330, 440, 2400, 2520)
    rng = np.random.default_rng(SOUP_SEED)
    g[372:396, 2448:2472] = rng.random((24, 24)) < 0.35
    return g


def run_report(g, engine, tune, gen_limit=3000):
    sim = Simulation(LifeConfig(W, H, gen_limit=gen_limit, tune=dict(tune)), engine=engine)
    sim.load(g)
    rep = sim.run()
    return (rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct), sim.tile(), sim


@pytest.mark.parametrize("case", ["soup", "soup_and_far_blinker", "empty"])
def test_termination_with_tiles_that_are_never_launched(gpu, case):
    """The change flags of tiles off the list reach the poll through the flag counts: (a) the soup stops at its
    fixed point; (b) a blinker in a far tile - quiet, and a candidate of no block after the second - keeps the
    run from stopping there; (c) an empty grid is extinct."""
    if case == "empty":
        g = np.zeros((H, W), np.uint8)
    else:
        g = soup_field()
        if case == "soup_and_far_blinker":
            clear(g, 90, 110, 4600, 4620)
            put(g, 100, 4608, BLINKER)
    cpu, want, _ = run_report(g, "cpu", {})
    got, out, sim = run_report(g, "hip", LIST)
    plain, _, _ = run_report(g, "hip", {**TUNE, "quiet_skip": "0"})
    assert got == cpu == plain, (got, cpu, plain)
    assert np.array_equal(out, want)
    if case == "soup":
        assert cpu[1] == "similarity" and cpu[2] == SOUP_FIXED
        d = sim.describe()  # frozen at the end: the last blocks listed nothing
        assert d["quiet_list"] is True and d["quiet_candidates"] == 0
        assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]
    elif case == "soup_and_far_blinker":
        assert cpu[0] == 3000 and cpu[1] != "similarity", cpu
        d = sim.describe()
        assert d["quiet_list"] is True and d["quiet_candidates"] == 0, d["quiet_candidates"]  # all is quiet or p2
    else:
        assert cpu[3], cpu


@pytest.mark.parametrize("grid", ["1", "3", "-1"])
def test_looping_kernel_gives_the_same(gpu, field, oracle, grid):
    """quiet_grid forces fewer groups than items (they loop over the list through the ticket); -1 sizes the
    grid from the reports."""
    sim = sim_of({**LIST, "quiet_grid": grid})
    sim.load(field)
    for g in CHECK_GENS:
        sim.native_engine.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
    d = listed_some_not_all(sim)
    ref = sim_of(LIST)
    ref.load(field)
    for g in CHECK_GENS:  # the same runs and reads: the same blocks
        ref.native_engine.run_until(g)
        assert np.array_equal(ref.tile(), oracle[g]), g
    d0 = ref.describe()
    assert (d["quiet_waves_launched"], d["quiet_waves_skipped"]) == (d0["quiet_waves_launched"], d0["quiet_waves_skipped"])
    got, out, _ = run_report(soup_field(), "hip", {**LIST, "quiet_grid": grid})
    want, ref_out, _ = run_report(soup_field(), "hip", {**TUNE, "quiet_list": "0"})
    assert got == want and got[2] == SOUP_FIXED
    assert np.array_equal(out, ref_out)


@pytest.mark.parametrize("chunks", ["12", "24", "5", "-5"])
def test_short_waves_give_the_same(gpu, field, oracle, chunks):
    """quiet_chunks forced: every item of every list launch as 12, 24 (4 rows each) or 5 (uneven: 19 and 20
    rows) one-wave workgroups; -5: only where five times the reported list fits the machine, so launches of
    both kernels alternate with the list's length."""
    tune = {**LIST, "quiet_chunks": chunks}
    sim, ref = sim_of(tune), sim_of({**LIST, "quiet_chunks": "1"})
    sim.load(field)
    ref.load(field)
    for g in CHECK_GENS:
        sim.native_engine.run_until(g)
        ref.native_engine.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
        assert np.array_equal(ref.tile(), oracle[g]), g
    d, d0 = listed_some_not_all(sim), ref.describe()
    assert (d["quiet_waves_launched"], d["quiet_waves_skipped"]) == (d0["quiet_waves_launched"], d0["quiet_waves_skipped"])
    assert d["launch_paths"] == d0["launch_paths"]
    got, out, _ = run_report(soup_field(), "hip", tune)
    want, ref_out, _ = run_report(soup_field(), "hip", {**TUNE, "quiet_list": "0"})
    assert got == want and got[2] == SOUP_FIXED
    assert np.array_equal(out, ref_out)


def test_short_waves_with_a_short_grid_and_remainder_rows(gpu, field, oracle):
    """Three items' worth of waves stride over the list; groups of 109 and 110 rows in 7 chunks."""
    sim = sim_of({**LIST, "quiet_chunks": "7", "quiet_grid": "3", "quiet_rows": "97"})
    sim.load(field)
    for g in CHECK_GENS:
        sim.native_engine.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
    d = sim.describe()
    assert d["quiet_list"] is True and 0 < d["quiet_candidates"] < 21
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]


def test_groups_with_remainder_rows(gpu, field, oracle):
    """quiet_rows=97: 768 rows in 7 groups of 109 and 110 rows."""
    sim = sim_of({**LIST, "quiet_rows": "97"})
    sim.load(field)
    for g in CHECK_GENS:
        sim.native_engine.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
    d = sim.describe()
    assert d["quiet_list"] is True and 0 < d["quiet_candidates"] < 21
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]


@pytest.mark.parametrize("event", ["load", "store_rows", "checkpoint", "step_of_7"])
def test_everything_that_touches_the_grid_invalidates_the_list(gpu, field, oracle, event, tmp_path):
    sim = sim_of(LIST)
    sim.load(field)
    eng = sim.native_engine
    if event == "load":
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
        cfg.gen_limit, cfg.tune = 100000, dict(LIST)
        sim2 = Simulation(cfg, engine="hip")
        sim2.load_text(str(grid))
        sim2.native_engine.run_until(600)
        assert np.array_equal(sim2.tile(), oracle[600])
        listed_some_not_all(sim2)
    else:
        eng.run_until(240)  # 20 blocks of 12: most tiles are off the list by now
        eng.run_until(247)  # blocks of 4, 2 and 1 generations
        for g in (355, 600):
            eng.run_until(g)
            assert np.array_equal(sim.tile(), oracle[g]), g
    listed_some_not_all(sim)
