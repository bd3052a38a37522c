"""The auto policy of quiet-tile skipping on the GPU (tuning quiet_skip=-1, the
default; quiet::Policy in csrc/include/gol/quiet.hpp, Engine::launch and
Engine::tail_wanted in csrc/src/engine.cpp): dense blocks, every
quiet_scout-th one a detecting scout, the skipping kernel once quiet_on percent
of the tiles are clean, dense blocks again below quiet_off.  The other GPU
tests of the skipping kernel run quiet_skip=1, where every block is the
skipping kernel's; here scouts stand between dense blocks, dense blocks hand
over to skipping blocks and back, skipping blocks run on a frame the adder
window has drifted, stops are found in poll windows that hold the flags of
both kinds of block, and the lazy tail follows the policy's state.

Every test runs against two dense kernels at T = 12: the DPP window (tmax=12,
no drift) and the adder window (xlane=3, drifting frame).  The field, the
helpers and CHECK_GENS are those of tests/test_quiet_list_gpu.py: 5120 x 768
cells, 3 strips x 8 groups = 24 tiles.  Every comparison is exact: cells
against the fp32 PyTorch oracle, stop reports against the CPU engine and a
quiet_skip=0 run.

The policy reads reports that lag the launches, so no test asserts at which
block a transition happened: only which kinds of block ran, and the mode after
a read of the grid (a read synchronises; mode() then polls the newest report
as the next launch would).  The thresholds come from the oracle: quiet_on and
quiet_off lie at least 20 points below the field's share of clean tiles, and
quiet_off at least 20 points above the soup's.

The reference has no counterpart (every generation rewrites every cell,
src/game_cuda.cu:128-148)."""
import functools

import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation
from gol_amd.ops.life_ops import life_step_torch_roll

from test_quiet_list_gpu import (BLINKER, CHECK_GENS, GROUP, H, SOUP_FIXED, STRIP, TILES, W, clear, field, oracle, put,
                                 run_report, soup_field)  # noqa: F401  (field, oracle: fixtures)

pytestmark = pytest.mark.gpu

T = 12
ON, OFF = 35, 25
BASE = {"quiet_skip": "-1", "quiet_scout": "2", "group": "4", "quiet_rows": "96"}
AUTO = {**BASE, "quiet_on": str(ON), "quiet_off": str(OFF)}
SCOUTS_ONLY = {**BASE, "quiet_on": "101"}  # not clamped, and no share exceeds 100: scouts for ever

# The dense kernel of the blocks the policy leaves dense: tuning, LifeConfig arguments, whether the frame drifts.
DENSE = {"dpp": ({}, {"tmax": T}, False), "adder": ({"xlane": "3"}, {}, True)}
dense_kernels = pytest.mark.parametrize("dense", ["dpp", "adder"])


def sim_of(dense, tune, gen_limit=100000, **kw):
    """A simulation whose gate is open: a test that never reached the policy fails here."""
    extra, cfg, drifts = DENSE[dense]
    tune = {**tune, **extra}
    sim = Simulation(LifeConfig(W, H, gen_limit=gen_limit, layout="bits", tune=tune, **cfg, **kw), engine="hip")
    d = sim.describe()
    skip = int(tune.get("quiet_skip", "-1"))
    assert d["row_ring"] and d["tmax"] == T, (d["row_ring"], d["tmax"])
    assert d["quiet_mode"] == {-1: "auto:dense", 0: "off", 1: "on"}[skip], d["quiet_mode"]
    # quiet_skip=1 takes the skipping kernel's window for every block: no drift.
    assert sim.native_engine.drifting is (drifts and skip != 1), (dense, skip)
    return sim


def mode(sim):
    """The policy's mode on the newest report.  After a read of the grid or the end of a run (both
    synchronise) that is the report of the last block launched."""
    sim.native_engine.quiet_waves_skipped  # polls, as the next launch would
    return sim.native_engine.quiet_mode()


def clean_shares(g, blocks):
    """Percent of the 24 tiles (GROUP rows of a strip of STRIP cells) whose cells at generation 12 (k + 1)
    equal those at 12 k, k = 0 .. blocks - 1, from the oracle."""
    out, cur = [], g
    for _ in range(blocks):
        nxt = life_step_torch_roll(cur, T, device="cuda")
        same = [np.array_equal(cur[y:y + GROUP, x:x + STRIP], nxt[y:y + GROUP, x:x + STRIP])
                for x in range(0, W, STRIP) for y in range(0, H, GROUP)]
        out.append(100 * sum(same) // len(same))
        cur = nxt
    return out


def busy_soup():
    return (np.random.default_rng(11).random((H, W)) < 0.5).astype(np.uint8)


@pytest.fixture(scope="module")
def thresholds(field):
    """The thresholds against the oracle's shares; returns the field's and the soup's."""
    quiet, busy = clean_shares(field, 9), clean_shares(busy_soup(), 3)
    assert OFF <= ON <= min(quiet) - 20, quiet
    assert OFF >= max(busy) + 20, busy
    return quiet, busy


@pytest.fixture(scope="module")
def oracle_3355(oracle):
    return life_step_torch_roll(oracle[600], 3355 - 600, device="cuda")


def ran_all_three(sim):
    d = sim.describe()
    b = d["quiet_blocks"]
    assert b["dense"] > 0 and b["scout"] > 0 and b["skip"] > 0, b
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"], (d["quiet_waves_skipped"], d["quiet_waves_launched"])
    return d


@dense_kernels
def test_dense_scout_skipping_is_exact(gpu, field, oracle, thresholds, dense):
    sims = [sim_of(dense, AUTO), sim_of(dense, {**AUTO, "quiet_skip": "0"}), sim_of(dense, {**AUTO, "quiet_skip": "1"})]
    for s in sims:
        s.load(field)
    for g in CHECK_GENS:
        tiles = []
        for s in sims:
            s.native_engine.run_until(g)
            tiles.append(s.tile())
        assert np.array_equal(tiles[0], oracle[g]), g
        assert np.array_equal(tiles[0], tiles[1]) and np.array_equal(tiles[0], tiles[2]), g
    assert mode(sims[0]) == "auto:skipping"
    d = ran_all_three(sims[0])
    print(f"quiet_blocks[{dense}] dense/scout/skipping: {d['quiet_blocks']}")
    assert sims[1].describe()["quiet_blocks"] == {"dense": 0, "scout": 0, "skip": 0}
    assert sims[2].describe()["quiet_blocks"]["dense"] == 0
    if dense == "adder":
        # Skipping blocks on a drifted frame: two runs with no read in between (a read rotates the frame
        # back).  The first ends on dense blocks and synchronises, so the second starts on its reports.
        sim = sim_of(dense, AUTO)
        sim.load(field)
        eng = sim.native_engine
        eng.run_until(100)
        assert eng.drift != 0 and eng.quiet_blocks_dense > 0
        eng.run_until(355)
        assert eng.drift != 0 and eng.quiet_blocks_skip > 0, (eng.drift, eng.quiet_blocks_skip)
        assert np.array_equal(sim.tile(), oracle[355])
        assert mode(sim) == "auto:skipping"
        ran_all_three(sim)


@dense_kernels
def test_scouts_only(gpu, field, oracle, dense):
    """quiet_on=101: dense blocks and scouts alternate for the whole run; every scout follows a dense block,
    which leaves it no words: it may skip nothing."""
    sim = sim_of(dense, SCOUTS_ONLY)
    sim.load(field)
    for g in CHECK_GENS:
        sim.native_engine.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
        assert mode(sim) == "auto:dense", g
    d = sim.describe()
    print(f"quiet_blocks[{dense}] dense/scout/skipping: {d['quiet_blocks']}")
    b = d["quiet_blocks"]
    assert b["skip"] == 0 and b["scout"] > 0 and abs(b["dense"] - b["scout"]) <= 1, b
    assert d["quiet_waves_skipped"] == 0 and d["quiet_waves_launched"] == 4 * TILES * b["scout"]


@dense_kernels
def test_fall_back_and_return(gpu, field, oracle, thresholds, dense):
    sim = sim_of(dense, AUTO)
    eng = sim.native_engine
    sim.load(field)
    for g in CHECK_GENS:
        eng.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
    assert mode(sim) == "auto:skipping"
    before = sim.describe()["quiet_blocks"]
    # A soup no tile of which is ever clean: the skipping blocks report it, the policy goes back.
    soup = busy_soup()
    sim.load(soup)
    eng.generation = 0
    want = soup
    for g in (10 * T, 20 * T):
        eng.run_until(g)
        want = life_step_torch_roll(want, 10 * T, device="cuda")
        assert np.array_equal(sim.tile(), want), g
    assert mode(sim) == "auto:dense"
    busy = sim.describe()["quiet_blocks"]
    assert busy["dense"] > before["dense"] and busy["scout"] > before["scout"], (before, busy)
    # The field again: scouts find it quiet within three chunks of four blocks.
    sim.load(field)
    eng.generation = 0
    want, at = field, 0
    for chunk in range(3):
        eng.run_until(at + 4 * T)
        want, at = life_step_torch_roll(want, 4 * T, device="cuda"), at + 4 * T
        assert np.array_equal(sim.tile(), want), at
        if mode(sim) == "auto:skipping":
            break
    assert mode(sim) == "auto:skipping"
    for g in (g for g in CHECK_GENS if g > at):
        eng.run_until(g)
        assert np.array_equal(sim.tile(), oracle[g]), g
    assert mode(sim) == "auto:skipping"
    d = ran_all_three(sim)
    assert d["quiet_blocks"]["skip"] > busy["skip"]
    print(f"quiet_blocks[{dense}] dense/scout/skipping: {before} -> {busy} -> {d['quiet_blocks']}")


def stop_field(case):
    if case == "empty":
        return np.zeros((H, W), np.uint8)
    g = soup_field()
    if case == "soup_and_far_blinker":
        clear(g, 90, 110, 4600, 4620)
        put(g, 100, 4608, BLINKER)
    return g


@functools.lru_cache(maxsize=None)
def cpu_stop(case):
    """The CPU engine's report and cells, once per case."""
    rep, cells, _ = run_report(stop_field(case), "cpu", {})
    return rep, cells


def hip_stop(g, dense, tune, gen_limit=3000, **kw):
    sim = sim_of(dense, tune, gen_limit=gen_limit, **kw)
    sim.load(g)
    rep = sim.run()
    return (rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct), sim.tile(), sim


@dense_kernels
@pytest.mark.parametrize("poll", [0, 16], ids=["poll_default", "poll_16"])
@pytest.mark.parametrize("case", ["soup", "soup_and_far_blinker", "empty"])
def test_stops_are_exact_across_transitions(gpu, thresholds, case, poll, dense):
    """run() to completion: the poll windows hold flags of dense blocks, scouts and skipping blocks (the
    default window is 21 blocks; poll_gens=16 polls after every block)."""
    g = stop_field(case)
    cpu, want = cpu_stop(case)
    got, out, sim = hip_stop(g, dense, AUTO, poll_gens=poll)
    plain, plain_out, _ = hip_stop(g, dense, {**AUTO, "quiet_skip": "0"}, poll_gens=poll)
    assert got == cpu == plain, (got, cpu, plain)
    assert np.array_equal(out, want) and np.array_equal(plain_out, want)
    d = sim.describe()
    print(f"quiet_blocks[{case}, {dense}, poll {poll}] dense/scout/skipping: {d['quiet_blocks']}")
    b = d["quiet_blocks"]
    assert b["dense"] > 0, b  # (an empty grid may stop before the first scout)
    if case == "soup":
        assert cpu[1] == "similarity" and cpu[2] == SOUP_FIXED
        assert b["skip"] > 0, b  # the stop was found while skipping
        assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]
    elif case == "soup_and_far_blinker":
        assert cpu[0] == 3000 and cpu[1] != "similarity", cpu
        assert b["skip"] > 0 and mode(sim) == "auto:skipping", b
    else:
        assert cpu[3], cpu


def fields(rep):
    return rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct


def tail(sim):
    d = sim.describe()
    return d["spine_generation"], d["tail_overshoots"], d["tail_replays"]


@dense_kernels
def test_lazy_tail_follows_the_policy(gpu, field, oracle_3355, thresholds, dense):
    """Chunked runs with no read in between (tests/test_lazy_tail_gpu.py): in auto, a run ends on a full
    block where the policy is skipping when it ends - never while it is dense."""
    limits = (355, 1355, 2355, 3355)
    lazy, plain = sim_of(dense, AUTO), sim_of(dense, {**AUTO, "lazy_tail": "0"})
    scouts = sim_of(dense, SCOUTS_ONLY)
    reps = {}
    for name, sim in (("lazy", lazy), ("plain", plain), ("scouts", scouts)):
        sim.load(field)
        eng, reps[name] = sim.native_engine, []
        for limit in limits:
            spine0, over0, _ = tail(sim)
            reps[name].append(eng.run_until(limit))
            # The state tail_wanted() saw at this run's last epoch (it polls; nothing has polled since).
            skipping = eng.quiet_mode() == "auto:skipping"
            spine, over, replays = tail(sim)
            assert sim.generation == limit <= spine < limit + T and replays == 0, (name, limit, spine)
            if name == "lazy" and skipping and (limit - spine0) % T != 0:
                assert over == over0 + 1 and spine > limit and (spine - spine0) % T == 0, (limit, spine0, spine, over)
            if name != "lazy" or not skipping:
                assert over == over0 and spine == limit, (name, limit, spine, over)
    assert mode(lazy) == mode(plain) == "auto:skipping" and mode(scouts) == "auto:dense"
    assert tail(lazy)[1] > 0 and tail(plain)[1] == 0 and tail(scouts)[1] == 0
    assert [fields(r) for r in reps["lazy"]] == [fields(r) for r in reps["plain"]] == [fields(r) for r in reps["scouts"]]
    assert [r.executed for r in reps["lazy"]] == [355, 1000, 1000, 1000]
    # Fewer launches than with the remainder blocks of every chunk.
    assert sum(r.kernel_launches for r in reps["lazy"]) < sum(r.kernel_launches for r in reps["plain"])
    ahead = tail(lazy)[0] > 3355
    got = lazy.tile()  # the one read: rewind, then the remainder
    assert tail(lazy)[0] == 3355 and tail(lazy)[2] == int(ahead)
    assert np.array_equal(got, oracle_3355)
    assert np.array_equal(plain.tile(), oracle_3355) and np.array_equal(scouts.tile(), oracle_3355)
    ran_all_three(lazy)
    ran_all_three(plain)
    b = scouts.describe()["quiet_blocks"]
    assert b["skip"] == 0 and b["scout"] > 0, b
    print(f"quiet_blocks[{dense}] dense/scout/skipping: lazy {lazy.describe()['quiet_blocks']}, "
          f"lazy_tail=0 {plain.describe()['quiet_blocks']}, quiet_on=101 {b}; tail {tail(lazy)}")


@pytest.mark.parametrize("case", ["linked", "defaults"])
def test_what_runs_beside_it_by_default(gpu, field, oracle, thresholds, case):
    """linked: link=1, the dense blocks run linked on two streams, which scouts and skipping blocks join.
    A launch links to the dense block before it, and with a scout every second block no two dense blocks
    follow each other, so this case scouts every third.
    defaults: nothing set but the scout interval and the thresholds - default group, quiet_rows, quiet_list,
    quiet_chunks and quiet_cols."""
    tune = {"quiet_scout": "2", "quiet_on": str(ON), "quiet_off": str(OFF)}
    if case == "linked":
        tune = {**AUTO, "quiet_scout": "3", "link": "1"}
    sim = sim_of("dpp", tune)
    sim.load(field)
    linked = 0
    for g in CHECK_GENS:
        sim.advance(g - sim.generation)
        linked += sim.last_report.linked_launches
        assert np.array_equal(sim.tile(), oracle[g]), g
    assert mode(sim) == "auto:skipping"
    d = ran_all_three(sim)
    print(f"quiet_blocks[{case}] dense/scout/skipping: {d['quiet_blocks']}, linked launches {linked}")
    if case == "linked":
        assert linked > 0 and d["launch_paths"]["linked"] == linked, (linked, d["launch_paths"])
    else:
        left = ("group", "quiet_skip", "quiet_rows", "quiet_list", "quiet_grid", "quiet_chunks", "quiet_cols", "link")
        assert not set(left) & d["tuning_changed"].keys(), d["tuning_changed"]
        assert d["quiet_list"] is True
