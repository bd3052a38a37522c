"""Lazy tail on the HIP backend (tuning lazy_tail, default -1: where the full
block that ends a run is a skipping launch).  The engine logic is covered on
the CPU backend (tests/test_lazy_tail.py); here the block is the skipping
kernel's, whose tile words must stay valid across the run boundary, and the
replay runs the dense remainder kernels.  Shapes and fields are those of
tests/test_quiet_skip.py; every case compares cells and stop reports with the
fp32 PyTorch oracle and a lazy_tail=0 run."""
import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation
from gol_amd.ops.life_ops import life_step_torch_roll
from gol_amd.utils.checkpoint import load_checkpoint, save_checkpoint

pytestmark = pytest.mark.gpu

W, H, T = 5120, 768, 12
TUNE = {"quiet_skip": "1", "group": "4", "quiet_rows": "96"}
STRIP, GROUP = 62 * 32, 96

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
    """tests/test_quiet_skip.py::field."""
    g = ash()
    clear(g, 180, 230, 2500, 2550)
    put(g, 198, 2518, PULSAR)
    clear(g, 400, 440, 700, 750)
    put(g, 418, 720, PENTADECATHLON)
    clear(g, 560, 620, 3300, 3360)
    put(g, 588, 3328, RPENT)
    for y, x, pat in [(300, STRIP - 6, GLIDER_SE), (330, STRIP + 4, GLIDER_NW),
                      (2 * GROUP - 6, 1000, GLIDER_SE), (3 * GROUP + 4, 1100, GLIDER_NW),
                      (H - 6, 4000, GLIDER_SE), (3, 4100, GLIDER_NW),
                      (500, W - 6, GLIDER_SE), (530, 3, GLIDER_NW)]:
        clear(g, y - 12, y + 16, x - 12, x + 16)
        put(g, y, x, pat)
    return g


CHECK_GENS = (7, 100, 355, 600, 3355)


@pytest.fixture(scope="module")
def oracle(field):
    """The field at CHECK_GENS from the fp32 PyTorch oracle, computed once."""
    out, cur, at = {}, field, 0
    for g in CHECK_GENS:
        cur = life_step_torch_roll(cur, g - at, device="cuda")
        out[g], at = cur, g
    return out


SOUP_SEED, SOUP_FIXED = 57, 456


def soup_field():
    """tests/test_quiet_skip.py::soup_field: frozen at generation SOUP_FIXED."""
    g = ash(still_only=True)
    clear(g, 330, 440, 2400, 2520)
    rng = np.random.default_rng(SOUP_SEED)
    g[372:396, 2448:2472] = rng.random((24, 24)) < 0.35
    return g


def sim_of(lazy=None, gen_limit=100000):
    tune = dict(TUNE) if lazy is None else dict(TUNE, lazy_tail=str(lazy))
    sim = Simulation(LifeConfig(W, H, gen_limit=gen_limit, layout="bits", tune=tune), engine="hip")
    d = sim.describe()
    assert d["row_ring"] and d["tmax"] == T and d["quiet_mode"] == "on", d
    return sim


def tail(sim):
    d = sim.describe()
    return d["spine_generation"], d["tail_overshoots"], d["tail_replays"]


def remainder_blocks(r):
    """Blocks of a remainder of r < T generations (pick_T: 8, 4, 2, 1)."""
    return bin(r).count("1")


def fields(rep):
    return rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct


def test_chunked_runs_never_restart_the_chain(gpu, field, oracle):
    limits = (355, 1355, 2355, 3355)
    lazy, plain = sim_of(), sim_of(lazy=0)
    reps = {}
    for name, sim in (("lazy", lazy), ("plain", plain)):
        sim.load(field)
        reps[name] = [sim.native_engine.run_until(g) for g in limits]  # no read in between
    assert tail(lazy) == (-(-3355 // T) * T, 4, 0)
    assert tail(plain) == (3355, 0, 0)
    assert [fields(r) for r in reps["lazy"]] == [fields(r) for r in reps["plain"]]
    assert [r.executed for r in reps["lazy"]] == [355, 1000, 1000, 1000]
    # One chain of full blocks; without lazy tails every chunk adds its remainder blocks.
    assert sum(r.kernel_launches for r in reps["lazy"]) == -(-3355 // T)
    assert [r.kernel_launches for r in reps["plain"]] == [n // T + remainder_blocks(n % T) for n in (355, 1000, 1000, 1000)]
    launched = sum(lazy.describe()["launch_paths"].values())
    got = lazy.tile()  # the one read: rewind, then the remainder of 3355 - 3348
    assert tail(lazy) == (3355, 4, 1)
    assert sum(lazy.describe()["launch_paths"].values()) - launched == remainder_blocks(3355 % T)
    assert np.array_equal(got, oracle[3355])
    assert np.array_equal(got, plain.tile())
    # The plain run recomputes every tile after each boundary; the lazy one never does.
    dl, dp = lazy.describe(), plain.describe()
    assert dl["quiet_waves_skipped"] > dp["quiet_waves_skipped"] > 0
    assert dl["quiet_waves_skipped"] < dl["quiet_waves_launched"]


def test_stop_inside_the_carried_window(gpu):
    g = soup_field()
    plain = sim_of(lazy=0, gen_limit=3000)
    plain.load(g)
    want = fields(plain.run())
    assert want[1:3] == ("similarity", SOUP_FIXED)
    cells = plain.tile()
    for L in (SOUP_FIXED - T + 1, SOUP_FIXED - 6, SOUP_FIXED - 1):
        sim = sim_of(gen_limit=3000)
        sim.load(g)
        rep = sim.native_engine.run_until(L)
        assert fields(rep) == (L, "limit", -1, False), L
        assert sim.generation == L < SOUP_FIXED <= tail(sim)[0]  # the chain is past the fixed point
        assert fields(sim.run()) == want, L
        assert np.array_equal(sim.tile(), cells), L


@pytest.mark.parametrize("lazy", [None, 1])
@pytest.mark.parametrize("event", ["store_rows", "checkpoint"])
def test_reads_between_chunks(gpu, field, oracle, event, lazy, tmp_path):
    """tests/test_quiet_skip.py::test_everything_that_touches_the_grid_invalidates
    with limits that are no multiples of 12: each read of a grid whose chain is
    ahead replays (lazy_tail=1); in auto, after the first replay, runs followed
    by reads keep their remainder blocks."""
    sim = sim_of(lazy)
    sim.load(field)
    eng = sim.native_engine
    if event == "store_rows":
        runs = 0
        for g in CHECK_GENS[:4]:
            for limit in (g - 3, g):
                runs += (limit - sim.generation) % T != 0
                eng.run_until(limit)
                if limit == g:
                    assert np.array_equal(sim.tile(), oracle[g]), g
                else:
                    assert eng.store_rows(GROUP - 5, 40).shape == (40, W)
        assert tail(sim) == ((600, runs, runs) if lazy else (600, 1, 1))
    else:
        eng.run_until(355)
        assert tail(sim) == (360, 1, 0)
        save_checkpoint(sim, str(tmp_path / "ck"))
        assert tail(sim) == (355, 1, 1)
        eng.run_until(600)
        assert tail(sim) == ((355 + 21 * T, 2, 1) if lazy else (600, 1, 1))  # 245 = 20 blocks and 5
        assert np.array_equal(sim.tile(), oracle[600])
        cfg, grid = load_checkpoint(str(tmp_path / "ck"))
        assert cfg.start_gen == 355
        cfg.gen_limit, cfg.tune = 100000, dict(sim.config.tune)
        resumed = Simulation(cfg, engine="hip")
        resumed.load_text(str(grid))
        resumed.native_engine.run_until(600)
        assert tail(resumed) == (355 + 21 * T, 1, 0)
        assert np.array_equal(resumed.tile(), oracle[600])
        assert tail(resumed) == (600, 1, 1)
    d = sim.describe()
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]
