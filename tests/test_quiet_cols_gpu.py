"""The column kernel of the skipping kernel on the GPU (tuning quiet_cols,
quiet_col_group, quiet_col_items; csrc/kernels/life_quiet_cols_impl.hpp): a
computing tile of a candidate-list launch recomputes only the groups of word
columns whose light cone changed in the last block.  Results may not change,
so every test compares cells, stop generations and reasons with the fp32
PyTorch oracle, the CPU backend, a quiet_cols=0 run and a quiet_skip=0 run,
and asserts that columns were computed and that they were fewer than the
columns of the tiles they lie in (no test passes vacuously).  The field and
the helpers are those of tests/test_quiet_list_gpu.py: 5120 x 768 cells, 3
strips x 8 groups = 24 tiles, the third strip 36 word columns wide.

The reference has no counterpart (every generation rewrites every cell,
src/game_cuda.cu:128-148)."""
import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation
from gol_amd.ops.life_ops import life_step_torch_roll
from gol_amd.utils.checkpoint import load_checkpoint, save_checkpoint

from test_quiet_list_gpu import (BLOCK, CHECK_GENS, GLIDER_NW, GLIDER_SE, GROUP, H, LIST, PENTADECATHLON, SOUP_FIXED,
                                 STRIP, TILES, TUNE, W, ash, clear, field, oracle, put, run_report, sim_of,
                                 soup_field)  # noqa: F401  (field, oracle: fixtures)

pytestmark = pytest.mark.gpu

COLS = {**LIST, "quiet_cols": "1"}
NOCOLS = {**LIST, "quiet_cols": "0"}


def narrow_not_empty(sim):
    """The column kernel ran: it computed columns, and fewer than its tiles own."""
    d = sim.describe()
    assert d["quiet_mode"] == "on" and d["quiet_list"] is True and d["quiet_cols"] is True
    assert 0 < d["quiet_cols_computed"] < d["quiet_cols_of_tiles"], (d["quiet_cols_computed"], d["quiet_cols_of_tiles"])
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]
    return d


def same_statistics(d, d0):
    assert (d["quiet_waves_launched"], d["quiet_waves_skipped"]) == (d0["quiet_waves_launched"], d0["quiet_waves_skipped"])
    assert d["launch_paths"] == d0["launch_paths"]
    assert d["quiet_blocks"] == d0["quiet_blocks"]


@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_columns_are_exact_vs_torch_whole_tile_and_unskipped_runs(gpu, field, oracle, layout):
    sims = [sim_of(COLS, layout), sim_of(NOCOLS, layout), sim_of({**TUNE, "quiet_skip": "0"}, layout)]
    for s in sims:
        s.load(field)
    cand = []
    for g in CHECK_GENS:
        tiles = []
        for s in sims:
            s.native_engine.run_until(g)
            tiles.append(s.tile())
        assert np.array_equal(tiles[0], oracle[g]), g
        assert np.array_equal(tiles[0], tiles[1]) and np.array_equal(tiles[0], tiles[2]), g
        cand.append((sims[0].describe()["quiet_candidates"], sims[1].describe()["quiet_candidates"]))
    d, d0 = narrow_not_empty(sims[0]), sims[1].describe()
    assert d0["quiet_cols"] is False and d0["quiet_cols_computed"] == 0
    same_statistics(d, d0)
    assert all(a == b for a, b in cand), cand  # tile words decide as before: the same lists
    assert 0 < d["quiet_candidates"] < TILES
    assert sims[2].describe()["quiet_cols"] is False


def test_default_is_off_and_auto_follows_the_list_length(gpu, field, oracle):
    d = sim_of(TUNE).describe()
    assert d["quiet_cols"] is False and d["tuning"]["quiet_cols"] == "0"
    assert sim_of({**COLS, "quiet_list": "0"}).describe()["quiet_cols"] is False
    assert sim_of({**COLS, "quiet_skip": "0"}).describe()["quiet_cols"] is False
    sim = sim_of({**LIST, "quiet_cols": "-1"})  # auto: every list of this field is shorter than quiet_col_items
    sim.load(field)
    sim.native_engine.run_until(355)
    assert np.array_equal(sim.tile(), oracle[355])
    narrow_not_empty(sim)


@pytest.mark.parametrize("case", ["soup", "soup_and_far_blinker", "empty"])
def test_termination_with_tiles_and_columns_that_are_never_recomputed(gpu, case):
    if case == "empty":
        g = np.zeros((H, W), np.uint8)
    else:
        g = soup_field()
        if case == "soup_and_far_blinker":
            clear(g, 90, 110, 4600, 4620)
            put(g, 100, 4608, ["111"])
    cpu, want, _ = run_report(g, "cpu", {})
    got, out, sim = run_report(g, "hip", COLS)
    assert got == cpu, (got, cpu)
    assert np.array_equal(out, want)
    d = sim.describe()
    if case == "soup":
        assert cpu[1] == "similarity" and cpu[2] == SOUP_FIXED
        assert d["quiet_candidates"] == 0
        narrow_not_empty(sim)
    elif case == "soup_and_far_blinker":
        assert cpu[0] == 3000 and cpu[1] != "similarity", cpu
        assert d["quiet_candidates"] == 0
        narrow_not_empty(sim)
    else:
        assert cpu[3], cpu


def test_gliders_cross_strips_groups_the_seam_and_the_wrap(gpu):
    """The gliders of the list test, from still-life ash: each crosses tiles and columns that were in no
    window when it arrived; one runs into a block."""
    g = ash(still_only=True)
    starts = [(300, STRIP - 40, GLIDER_SE), (430, STRIP + 40, GLIDER_NW), (2 * GROUP - 30, 900, GLIDER_SE),
              (3 * GROUP + 30, 1300, GLIDER_NW), (H - 40, 4000, GLIDER_SE), (40, 4500, GLIDER_NW),
              (500, W - 40, GLIDER_SE), (700, 40, GLIDER_NW)]
    for y, x, pat in starts:
        s = 1 if pat is GLIDER_SE else -1
        for t in range(0, 331, 8):
            clear(g, y + s * t - 10, y + s * t + 14, x + s * t - 10, x + s * t + 14)
        put(g, y, x, pat)
    put(g, 300 + 150, STRIP - 40 + 151, BLOCK)
    sim, ref = sim_of(COLS), sim_of(NOCOLS)
    sim.load(g)
    ref.load(g)
    for gen in (600, 1200):
        sim.native_engine.run_until(gen)
        ref.native_engine.run_until(gen)
        assert np.array_equal(sim.tile(), ref.tile()), gen
    assert np.array_equal(sim.tile(), life_step_torch_roll(g, 1200, device="cuda"))
    same_statistics(narrow_not_empty(sim), ref.describe())


def test_pentadecathlon_keeps_a_narrow_constant_window(gpu):
    """p15 never settles: its tile computes in every block, the same one group of columns."""
    g = ash(still_only=True)
    clear(g, 400, 440, 700, 750)
    put(g, 418, 720, PENTADECATHLON)  # words 22 and 23 of strip 0: lane columns 23, 24 - one group of four
    sim = sim_of(COLS)
    sim.load(g)
    eng = sim.native_engine
    eng.run_until(240)
    c0 = sim.describe()
    eng.run_until(480)
    c1 = sim.describe()
    eng.run_until(720)
    c2 = sim.describe()
    assert np.array_equal(sim.tile(), life_step_torch_roll(g, 720, device="cuda"))
    per20 = c1["quiet_cols_computed"] - c0["quiet_cols_computed"]
    assert per20 == c2["quiet_cols_computed"] - c1["quiet_cols_computed"] == 20 * 4, per20
    assert c2["quiet_cols_of_tiles"] - c1["quiet_cols_of_tiles"] == 20 * 62
    assert 1 <= c2["quiet_candidates"] <= 9


@pytest.mark.parametrize("group", ["2", "4", "8"])
def test_wide_spot_and_soup_across_two_strips(gpu, group):
    """A 300-cell row of blinker fuel (wider than a group of 2, 4 or 8 words) and a 24 x 24 soup straddling
    the boundary of strips 0 and 1."""
    g = ash(still_only=True)
    clear(g, 180, 260, 900, 1400)
    g[220, 1000:1300] = 1
    clear(g, 440, 540, STRIP - 60, STRIP + 60)
    rng = np.random.default_rng(3)
    g[480:504, STRIP - 12:STRIP + 12] = rng.random((24, 24)) < 0.4
    sim = sim_of({**COLS, "quiet_col_group": group})
    sim.load(g)
    want, at = g, 0
    for gen in (100, 355):
        sim.native_engine.run_until(gen)
        want, at = life_step_torch_roll(want, gen - at, device="cuda"), gen
        assert np.array_equal(sim.tile(), want), gen
    narrow_not_empty(sim)


def test_groups_with_remainder_rows(gpu, field, oracle):
    """quiet_rows=97: groups of 109 and 110 rows, three bands of 40, 40 and 29 or 30 rows."""
    sim, ref = sim_of({**COLS, "quiet_rows": "97"}), sim_of({**NOCOLS, "quiet_rows": "97"})
    sim.load(field)
    ref.load(field)
    for g in CHECK_GENS:
        sim.native_engine.run_until(g)
        ref.native_engine.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
        assert np.array_equal(ref.tile(), oracle[g]), g  # (both grids are read: the same lazy tails)
    same_statistics(narrow_not_empty(sim), ref.describe())


@pytest.mark.parametrize("extra", [{"quiet_cols": "-1", "quiet_col_items": "9"},
                                  {"quiet_cols": "1", "quiet_chunks": "7", "quiet_grid": "3"},
                                  {"quiet_cols": "1", "quiet_chunks": "1", "quiet_grid": "-1"}],
                         ids=["auto_bound_9", "forced_chunks_and_grid", "sized_grid"])
def test_alternating_and_forced_kernels_give_the_same(gpu, field, oracle, extra):
    """quiet_col_items=9: the lists of this field are longer at first and shorter later, so whole-tile and
    column launches alternate (records of unknown validity in between).  Forced chunks and a forced grid
    with quiet_cols=1: three items' worth of waves stride over the units."""
    sim, ref = sim_of({**LIST, **extra}), sim_of(NOCOLS)
    sim.load(field)
    ref.load(field)
    for g in CHECK_GENS:
        sim.native_engine.run_until(g)
        ref.native_engine.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
        assert np.array_equal(ref.tile(), oracle[g]), g  # (both grids are read: the same lazy tails)
    d, d0 = narrow_not_empty(sim), ref.describe()
    assert (d["quiet_waves_launched"], d["quiet_waves_skipped"]) == (d0["quiet_waves_launched"], d0["quiet_waves_skipped"])
    assert d["launch_paths"] == d0["launch_paths"]
    got, out, _ = run_report(soup_field(), "hip", {**LIST, **extra})
    want, ref_out, _ = run_report(soup_field(), "hip", {**TUNE, "quiet_list": "0"})
    assert got == want and got[2] == SOUP_FIXED
    assert np.array_equal(out, ref_out)


@pytest.mark.parametrize("event", ["load", "store_rows", "checkpoint", "step_of_7"])
def test_everything_that_touches_the_grid_invalidates_the_records(gpu, field, oracle, event, tmp_path):
    sim = sim_of(COLS)
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
            eng.store_rows(GROUP - 5, 40)
            eng.run_until(g)
            assert np.array_equal(sim.tile(), oracle[g]), g
    elif event == "checkpoint":
        eng.run_until(355)
        save_checkpoint(sim, str(tmp_path / "ck"))
        eng.run_until(600)
        assert np.array_equal(sim.tile(), oracle[600])
        cfg, grid = load_checkpoint(str(tmp_path / "ck"))
        cfg.gen_limit, cfg.tune = 100000, dict(COLS)
        sim2 = Simulation(cfg, engine="hip")
        sim2.load_text(str(grid))
        sim2.native_engine.run_until(600)
        assert np.array_equal(sim2.tile(), oracle[600])
        narrow_not_empty(sim2)
    else:
        eng.run_until(240)
        eng.run_until(247)  # blocks of 4, 2 and 1 generations
        for g in (355, 600):
            eng.run_until(g)
            assert np.array_equal(sim.tile(), oracle[g]), g
    narrow_not_empty(sim)
