"""Lazy tail (tuning lazy_tail; csrc/src/engine.cpp): a run whose last epoch is
shorter than a block runs one full block instead and reports its limit.  The
block chain (``spine_generation``) is then up to T - 1 generations past
``generation``; the next run carries the flags of those generations over and
continues from the spine, and anything that needs the grid at ``generation``
rewinds to the block's input and replays the remainder blocks.

All of it is engine logic, so it is checked here on the CPU backend with its
emulated row ring and ``lazy_tail=1`` (forced), against the exact serial loop;
tests/test_lazy_tail_gpu.py covers the skipping kernel's auto mode.

The reference has no counterpart: its loops evaluate one generation per
iteration (src/game.c:169-196)."""
import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation, random_grid, reference_run
from gol_amd.utils.checkpoint import load_checkpoint, save_checkpoint

W, H, END = 256, 96, 600
LAYOUTS = ["bits", "u8"]


def sim_of(layout, lazy=1, drift=0, w=W, h=H, gen_limit=100000, **kw):
    tune = {"cpu_ring": "1", "cpu_drift": str(drift)}
    if lazy is not None:
        tune["lazy_tail"] = str(lazy)
    if layout == "u8":
        tune["u8_via_bits"] = "1"
    sim = Simulation(LifeConfig(w, h, gen_limit=gen_limit, layout=layout, tune=tune, **kw), engine="cpu")
    d = sim.describe()
    assert d["row_ring"] and d["epoch"] == d["tmax"], d
    return sim


def tail(sim):
    d = sim.describe()
    return d["spine_generation"], d["tail_overshoots"], d["tail_replays"]


@pytest.fixture(scope="module")
def soup(native):
    """A 256 x 96 soup of density 0.5 at every generation 0 .. END, from the
    exact serial loop one generation at a time; it is still changing at END."""
    traj = [random_grid(W, H, 11, 0.5)]
    for _ in range(END):
        traj.append(reference_run(traj[-1], 1, check_similarity=False)[0])
    _, gens, _ = reference_run(traj[0], END)
    assert gens == END  # no stop before END: every chunk must report its limit
    return traj


# ---- chunked runs against one run --------------------------------------------
@pytest.mark.parametrize("read", ["every_chunk", "at_end"])
@pytest.mark.parametrize("chunk", ["1", "7", "T-1", "T", "T+1", "100"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_chunked_runs_equal_one_run(native, soup, layout, chunk, read):
    sim = sim_of(layout)
    T = sim.describe()["tmax"]
    n = {"T-1": T - 1, "T": T, "T+1": T + 1}.get(chunk) or int(chunk)
    sim.load(soup[0])
    eng = sim.native_engine
    g, limits, lengths = 0, [], []
    while g < END:
        prev, g = g, min(END, g + n)
        limits.append(g)
        lengths.append(g - prev)
        rep = eng.run_until(g)
        assert (sim.generation, rep.generations, rep.stop_reason, rep.executed) == (g, g, "limit", g - prev)
        assert g <= tail(sim)[0] < g + T
        if read == "every_chunk":
            assert np.array_equal(sim.tile(), soup[g]), g
            assert tail(sim)[0] == g
    assert np.array_equal(sim.tile(), soup[END])
    spine, overshoots, replays = tail(sim)
    assert spine == sim.generation == END
    if read == "at_end":
        # The chain never restarts, so a run ends on a full block wherever
        # its limit is not a multiple of T.
        assert overshoots > 0 or all(x % T == 0 for x in limits)
        assert replays <= 1
        assert replays == (END % T != 0)
    else:
        # Every read brings the chain back to `generation`: each run starts there.
        assert replays == overshoots == sum(x % T != 0 for x in lengths)


# ---- a stop inside the carried window ------------------------------------------
# tests/test_quiet_skip.py::soup_field: a 24 x 24 soup of density 0.35 on a
# background of blocks, frozen at generation SOUP_FIXED.
FW, FH = 5120, 768
SOUP_SEED, SOUP_FIXED = 57, 456
# The cases start from the field at generation FIELD_AT (a resume: start_gen
# and the similarity phase of a loop that began at 0), so each one runs a few
# blocks only; the oracle runs from generation 0.
FIELD_AT = 400


def soup_field():
    g = np.zeros((FH, FW), np.uint8)
    rng = np.random.default_rng(5)
    for y in range(4, FH - 8, 16):
        for x in range(4, FW - 8, 16):
            if rng.integers(0, 6) == 0:
                g[y:y + 2, x:x + 2] = 1
    g[330:440, 2400:2520] = 0
    rng = np.random.default_rng(SOUP_SEED)
    g[372:396, 2448:2472] = rng.random((24, 24)) < 0.35
    return g


@pytest.fixture(scope="module")
def fixed_point(native):
    """The oracle - one run() to 3000 with lazy_tail=0, per layout: generations,
    stop reason, first_unchanged, extinct and the cells - and the field at
    FIELD_AT."""
    g = soup_field()
    out = {}
    for layout in LAYOUTS:
        sim = sim_of(layout, lazy=0, w=FW, h=FH, gen_limit=3000)
        sim.load(g)
        if layout == "bits":
            sim.native_engine.run_until(FIELD_AT)
            out["field"] = sim.tile()
        rep = sim.run()
        out[layout] = ((rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct), sim.tile())
        assert tail(sim)[1] == 0
    assert out["bits"][0][2] == SOUP_FIXED and out["bits"][0][1] == "similarity"
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fixed_point_inside_the_carried_window(native, fixed_point, layout):
    want, cells = fixed_point[layout]
    T = sim_of(layout).describe()["tmax"]
    assert FIELD_AT < SOUP_FIXED - T
    ahead_of_stop = 0
    for L in range(SOUP_FIXED - T + 1, SOUP_FIXED):
        sim = sim_of(layout, w=FW, h=FH, gen_limit=3000, start_gen=FIELD_AT, sim_phase=FIELD_AT % 3)
        sim.load(fixed_point["field"])
        rep = sim.native_engine.run_until(L)
        assert (rep.generations, rep.stop_reason, rep.first_unchanged) == (L, "limit", -1), L
        spine = tail(sim)[0]
        assert sim.generation == L <= spine < L + T
        ahead_of_stop += L < SOUP_FIXED <= spine
        rep = sim.run()
        assert (rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct) == want, L
        assert np.array_equal(sim.tile(), cells), L
    assert ahead_of_stop > 0  # some run ended with the chain already past the fixed point


@pytest.mark.parametrize("layout", LAYOUTS)
def test_extinction_inside_the_carried_window(native, layout):
    """Two isolated cells: generation 1 is empty, generation 2 the first
    unchanged one; the loop reports 1 (src/game.c:177)."""
    g = np.zeros((H, W), np.uint8)
    g[10, 10] = g[50, 100] = 1
    plain = sim_of(layout, lazy=0, gen_limit=1000)
    plain.load(g)
    rep = plain.run()
    want = (rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct)
    assert want == (1, "extinction", 2, True)
    T = plain.describe()["tmax"]
    fields = lambda rep: (rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct)
    for L in (1, 2, T - 1):
        # L = 1 ends before the first unchanged generation; the later limits see
        # the stop themselves.  Either way: what a lazy_tail=0 engine reports.
        sim, plain = sim_of(layout, gen_limit=1000), sim_of(layout, lazy=0, gen_limit=1000)
        sim.load(g)
        plain.load(g)
        first, first_plain = sim.native_engine.run_until(L), plain.native_engine.run_until(L)
        assert tail(sim)[0] == T  # one full block: the chain is past the stop
        assert fields(first) == fields(first_plain)
        second, second_plain = sim.run(), plain.run()
        assert fields(second) == fields(second_plain)
        if L == 1:
            assert fields(first) == (1, "limit", -1, False) and fields(second) == want
        assert not sim.tile().any()


# ---- operations that need the grid ----------------------------------------------
OPS = ["store_rows", "alive_count", "checkpoint", "load", "advance", "run_until_within", "set_generation"]


@pytest.mark.parametrize("drift", [0, 1])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_operations_with_an_overshoot_pending(native, soup, layout, op, drift, tmp_path):
    sim = sim_of(layout, drift=drift)
    T = sim.describe()["tmax"]
    eng = sim.native_engine
    sim.load(soup[0])
    A = 3 * T + 5  # the run ends T - 5 generations short of its fourth block
    eng.run_until(A)
    assert (sim.generation, tail(sim)) == (A, (4 * T, 1, 0))
    later = A + 2 * T + 3
    if op == "store_rows":
        assert np.array_equal(eng.store_rows(7, 30), soup[A][7:37])
        assert tail(sim) == (A, 1, 1)
    elif op == "alive_count":
        assert sim.alive_count() == int(soup[A].sum())
        assert tail(sim) == (A, 1, 1)
    elif op == "checkpoint":
        save_checkpoint(sim, str(tmp_path / "ck"))
        assert tail(sim) == (A, 1, 1)
        cfg, grid = load_checkpoint(str(tmp_path / "ck"))
        assert cfg.start_gen == A
        cfg.gen_limit, cfg.tune = 100000, dict(sim.config.tune)
        resumed = Simulation(cfg, engine="cpu")
        resumed.load_text(str(grid))
        resumed.native_engine.run_until(later)
        assert np.array_equal(resumed.tile(), soup[later])
    elif op == "load":
        # A load drops the chain ahead of it: nothing to replay, nothing carried.
        sim.load(soup[100])
        eng.generation = 0
        assert tail(sim) == (0, 1, 0)
        eng.run_until(later)
        assert np.array_equal(sim.tile(), soup[100 + later])
        return
    elif op == "advance":
        rep = sim.advance(2)  # within the carried generations: no launch
        assert (rep.executed, rep.kernel_launches, sim.generation) == (2, 0, A + 2)
        assert tail(sim) == (4 * T, 1, 0)
        sim.advance(T)  # across the spine
        assert sim.generation == A + 2 + T
        assert np.array_equal(sim.tile(), soup[A + 2 + T])
    elif op == "run_until_within":
        prev = A
        for limit in (A + 1, 4 * T - 1, 4 * T):  # the last one lies on the spine
            rep = eng.run_until(limit)
            assert (rep.generations, rep.executed, sim.generation) == (limit, limit - prev, limit)
            assert rep.kernel_launches == 0 and tail(sim)[0] == 4 * T
            prev = limit
        assert np.array_equal(sim.tile(), soup[4 * T])
        assert tail(sim) == (4 * T, 1, 0)  # the spine itself: nothing to replay
    else:
        eng.generation = 1000  # renumbering needs the grid at the old number first
        assert tail(sim) == (1000, 1, 1)
        eng.run_until(1000 + later - A)
        assert np.array_equal(sim.tile(), soup[later])
        return
    eng.run_until(later)
    assert sim.generation == later
    assert np.array_equal(sim.tile(), soup[later])


# ---- lazy_tail=0 and the default ---------------------------------------------------
@pytest.mark.parametrize("lazy", [0, None])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_off_and_default_keep_the_remainder_blocks(native, soup, layout, lazy):
    """lazy_tail=0, and the default (-1) on the CPU backend, which has no
    skipping kernel: every run ends on its remainder blocks."""
    sim = sim_of(layout, lazy=lazy)
    sim.load(soup[0])
    for g in (5, 100, 333):
        sim.native_engine.run_until(g)
        assert tail(sim) == (g, 0, 0)
    assert np.array_equal(sim.tile(), soup[333])
