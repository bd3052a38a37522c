"""The skipping kernel on the smallest tile tori (csrc/include/gol/quiet.hpp,
quiet::neighbour; csrc/kernels/life_quiet_impl.hpp, life_quiet_cols_impl.hpp).
The other GPU tests run 3 strips x 8 groups, where a tile's nine neighbours
are nine tiles and the last strip is 36 word columns wide.  With one strip a
tile is its own left and right neighbour, with one group its own upper and
lower one, with two both neighbours are the same tile: a tile marks itself up
to nine times in the list kernel's stamps, the column kernel's lane 0 and lane
own + 1 read the tile's own records, and a last strip of 1, 2 or 3 word
columns is narrower than a column group of 2, 4 or 8.

Shapes (bit tiles up to 2048 cells wide have a pitch of 256 bytes, so heights
that are multiples of 16 ring with a halo of 16 rows; groups of 96 rows):

    W x H        strips x groups   owned word columns per strip
    1024 x 96        1 x 1         32
      32 x 192       1 x 2         1
    1024 x 192       1 x 2         32
    2048 x 96        2 x 1         62, 2
    2016 x 192       2 x 2         62, 1
    2048 x 192       2 x 2         62, 2
    2080 x 192       2 x 2         62, 3

Every shape runs through every body of the kernel: one workgroup per tile
(quiet_list=0), the candidate list, short waves (quiet_chunks=24) and the
column kernel with groups of 2, 4 and 8 columns.  Every comparison is exact:
cells against the fp32 PyTorch oracle and a quiet_skip=0 run, stop reports
against the CPU engine; every test asserts that the ring and the plan are the
ones of the table and that waves were skipped.

The reference has no counterpart (every generation rewrites every cell,
src/game_cuda.cu:128-148)."""
import functools

import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation
from gol_amd.ops.life_ops import life_step_torch_roll

from test_quiet_list_gpu import BLINKER, BLOCK, GLIDER_NW, GLIDER_SE, PENTADECATHLON, put

pytestmark = pytest.mark.gpu

T, GROUP, STRIP = 12, 96, 62 * 32
# (W, H): (strips, groups, owned word columns per strip)
SHAPES = {(1024, 96): (1, 1, (32,)), (32, 192): (1, 2, (1,)), (1024, 192): (1, 2, (32,)), (2048, 96): (2, 1, (62, 2)),
          (2016, 192): (2, 2, (62, 1)), (2048, 192): (2, 2, (62, 2)), (2080, 192): (2, 2, (62, 3))}
TUNE = {"quiet_skip": "1", "quiet_rows": str(GROUP)}
BODIES = {"one_group_per_tile": {"quiet_list": "0"},
          "list": {"quiet_list": "1", "quiet_chunks": "1"},
          "short_waves": {"quiet_list": "1", "quiet_chunks": "24"},
          "cols_2": {"quiet_list": "1", "quiet_cols": "1", "quiet_col_group": "2"},
          "cols_4": {"quiet_list": "1", "quiet_cols": "1", "quiet_col_group": "4"},
          "cols_8": {"quiet_list": "1", "quiet_cols": "1", "quiet_col_group": "8"}}

shapes = pytest.mark.parametrize("shape", list(SHAPES), ids=[f"{w}x{h}" for w, h in SHAPES])
shapes_of_several_tiles = pytest.mark.parametrize("shape", [s for s, p in SHAPES.items() if p[0] * p[1] > 1],
                                                 ids=[f"{w}x{h}" for (w, h), p in SHAPES.items() if p[0] * p[1] > 1])
bodies = pytest.mark.parametrize("body", list(BODIES))

PENTADECATHLON_UPRIGHT = ["".join(r[i] for r in PENTADECATHLON) for i in range(10)]


def tiles_of(shape):
    return SHAPES[shape][0] * SHAPES[shape][1]


def sim_of(shape, tune, gen_limit=100000, **kw):
    """A ring tile in blocks of 12 generations, or the test has nothing to say."""
    sim = Simulation(LifeConfig(*shape, gen_limit=gen_limit, layout="bits", tune=dict(tune), **kw), engine="hip")
    d = sim.describe()
    assert d["row_ring"] and d["tmax"] == T, (shape, d["row_ring"], d["row_ring_fallback"], d["tmax"])
    return sim


def body_sim(shape, body, **kw):
    sim = sim_of(shape, {**TUNE, **BODIES[body]}, **kw)
    d = sim.describe()
    assert d["quiet_mode"] == "on" and d["quiet_list"] is (body != "one_group_per_tile")
    assert d["quiet_cols"] is body.startswith("cols")
    return sim


def plain_sim(shape, g, **kw):
    """The dense kernels on the same ring, in blocks of 12 generations too, with field g loaded."""
    sim = sim_of(shape, {**TUNE, "quiet_skip": "0"}, tmax=T, **kw)
    assert sim.describe()["quiet_mode"] == "off"
    sim.load(g)
    return sim


def plan_is_the_tables(sim, shape):
    """Every block of 12 generations was the skipping kernel's, on strips x groups tiles of 4 waves."""
    d = sim.describe()
    blocks = d["quiet_blocks"]["skip"]
    assert blocks > 0 and d["quiet_blocks"]["dense"] == 0
    assert d["quiet_waves_launched"] == 4 * tiles_of(shape) * blocks, (shape, d["quiet_waves_launched"], blocks)
    return d


def skipped_some_not_all(sim, shape, body):
    d = plan_is_the_tables(sim, shape)
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"], (d["quiet_waves_skipped"], d["quiet_waves_launched"])
    if body.startswith("cols") and tiles_of(shape) > 1:
        # (a last strip narrower than the column group: the kernel computes whole groups, so all its columns)
        assert 0 < d["quiet_cols_computed"] <= d["quiet_cols_of_tiles"], (d["quiet_cols_computed"], d["quiet_cols_of_tiles"])
    return d


def clear(g, y0, y1, x0, x1):
    g[np.ix_(np.arange(y0, y1) % g.shape[0], np.arange(x0, x1) % g.shape[1])] = 0


def ash(shape, still_only=False, seed=5):
    """Blocks and blinkers on a 16-cell lattice (about every third site)."""
    W, H = shape
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


def soup_field(shape, seed):
    """A 24 x 24 soup on an empty background, over the row seam (which is a group boundary where there are two
    groups) and over the boundary of the two strips where there are two."""
    W, H = shape
    g = np.zeros((H, W), np.uint8)
    soup = np.random.default_rng(seed).random((24, 24)) < 0.35
    x0 = STRIP - 12 if SHAPES[shape][0] == 2 else (W - 24) // 2
    g[np.ix_(np.arange(H - 12, H + 12) % H, np.arange(x0, x0 + 24))] = soup
    return g


def busy_tile_field(shape):
    """A pentadecathlon (p15: never clean over 12 generations) in the middle of the tile of strip 0 and group 0,
    30 cells or more from its edges (a tile 32 cells wide: upright, 11 cells); ash everywhere else."""
    W, H = shape
    g = ash(shape)
    cx = min(W, STRIP) // 2
    clear(g, 8, GROUP - 8, cx - 52, cx + 52)
    if W == 32:
        put(g, GROUP // 2 - 5, cx - 1, PENTADECATHLON_UPRIGHT)
    else:
        put(g, GROUP // 2 - 1, cx - 5, PENTADECATHLON)
    return g


GLIDER_GENS = 1200


def glider_field(shape):
    """One SE and one NW glider in still-life ash, their lanes of 300 cells cleared; the diagonals are 16
    cells apart modulo 32 (which divides both sides of every torus), so the two never meet.  Both cross the
    row seam; where there are two strips, the SE one crosses their boundary and the column wrap, the NW one the
    column wrap and the narrow strip."""
    W, H = shape
    g = ash(shape, still_only=True)
    x_se = STRIP - 150 if SHAPES[shape][0] == 2 else W // 8
    x_nw = 138 if SHAPES[shape][0] == 2 else (W - W // 8 - x_se) // 32 * 32 + x_se
    assert (x_se - x_nw) % 32 == 0 and H % 32 == 0  # with the rows below: diagonals 16 apart modulo 32
    starts = [(20, x_se, GLIDER_SE), (H - 60, x_nw, GLIDER_NW)]
    for y, x, pat in starts:
        s = 1 if pat is GLIDER_SE else -1
        for t in range(0, GLIDER_GENS // 4 + 31, 8):
            clear(g, y + s * t - 10, y + s * t + 14, x + s * t - 10, x + s * t + 14)
    for y, x, pat in starts:
        put(g, y, x, pat)
    return g


@functools.lru_cache(maxsize=None)
def oracle_of(kind, shape, gens):
    """The field and its states at `gens` from the fp32 PyTorch oracle, once per field and shape."""
    g = {"p2": lambda: soup_field(shape, 2), "busy": lambda: busy_tile_field(shape), "gliders": lambda: glider_field(shape)}[kind]()
    out, cur, at = {}, g, 0
    for n in gens:
        cur = life_step_torch_roll(cur, n - at, device="cuda")
        out[n], at = cur, n
    return g, out


@functools.lru_cache(maxsize=None)
def stops_of(kind, shape):
    """Stop report and cells of the CPU engine and of a quiet_skip=0 run, once per field and shape."""
    g = soup_field(shape, 273) if kind == "freeze" else np.zeros(shape[::-1], np.uint8)
    cpu = Simulation(LifeConfig(*shape, gen_limit=3000), engine="cpu")
    cpu.load(g)
    rep = cpu.run()
    plain = plain_sim(shape, g, gen_limit=3000)
    prep = plain.run()
    return g, report(rep), cpu.tile(), report(prep), plain.tile()


def report(rep):
    return rep.generations, rep.stop_reason, rep.first_unchanged, rep.extinct


def run_and_compare(sim, gens, want, plain=None):
    for n in gens:
        sim.native_engine.run_until(n)
        assert np.array_equal(sim.tile(), want[n]), n
        if plain is not None:
            plain.native_engine.run_until(n)
            assert np.array_equal(plain.tile(), want[n]), n


@shapes
@bodies
def test_soup_settles_to_period_two(gpu, shape, body):
    """Nothing is clean before the soup has settled (generation 166; 177 on 32 x 192); then everything
    skips, with cells left alive."""
    gens = (7, 100, 355, 600)
    g, want = oracle_of("p2", shape, gens)
    assert want[600].any() and np.array_equal(want[600], life_step_torch_roll(want[600], 2, device="cuda"))
    assert not np.array_equal(want[100], life_step_torch_roll(want[100], T, device="cuda"))
    sim = body_sim(shape, body)
    sim.load(g)
    run_and_compare(sim, gens[:2], want)
    d = plan_is_the_tables(sim, shape)
    if tiles_of(shape) == 1:
        assert d["quiet_waves_skipped"] == 0  # its one tile has not been clean yet
    run_and_compare(sim, gens[2:], want)
    d = skipped_some_not_all(sim, shape, body)
    print(f"{shape[0]} x {shape[1]} [{body}]: {d['quiet_waves_launched'] // (4 * d['quiet_blocks']['skip'])} tiles, "
          f"waves skipped {d['quiet_waves_skipped']} of {d['quiet_waves_launched']}")


@shapes
@bodies
def test_soup_freezes_and_the_run_stops(gpu, shape, body):
    g, cpu, cells, plain, plain_cells = stops_of("freeze", shape)
    assert cpu[1] == "similarity" and cells.any(), cpu
    sim = body_sim(shape, body, gen_limit=3000)
    sim.load(g)
    got = report(sim.run())
    assert got == cpu == plain, (got, cpu, plain)
    out = sim.tile()
    assert np.array_equal(out, cells) and np.array_equal(out, plain_cells)
    skipped_some_not_all(sim, shape, body)


@shapes_of_several_tiles
@bodies
def test_one_tile_never_settles(gpu, shape, body):
    """The quiet tiles have the busy one both above and below, or both left and right, or at all four
    corners: one neighbour relation read twice or four times."""
    gens = (355, 720)
    g, want = oracle_of("busy", shape, gens)
    # The pentadecathlon is where it was put (720 = 48 x 15), and it moves within 12 generations.
    assert np.array_equal(want[720][:GROUP], g[:GROUP]) and g[:GROUP].sum() >= 12
    assert not np.array_equal(want[720], life_step_torch_roll(want[720], T, device="cuda"))
    sim = body_sim(shape, body)
    sim.load(g)
    run_and_compare(sim, gens, want, plain_sim(shape, g))
    d = skipped_some_not_all(sim, shape, body)
    if body != "one_group_per_tile":
        assert 1 <= d["quiet_candidates"] <= tiles_of(shape), d["quiet_candidates"]


@shapes
@bodies
def test_gliders_through_every_identification(gpu, shape, body):
    gens = (GLIDER_GENS // 2, GLIDER_GENS)
    g, want = oracle_of("gliders", shape, gens)
    # Both gliders arrive: the ash stands, and ten more cells are alive, elsewhere.
    rest = life_step_torch_roll(g, 4, device="cuda")
    assert want[GLIDER_GENS].sum() == rest.sum() and not np.array_equal(want[GLIDER_GENS], want[GLIDER_GENS // 2])
    sim = body_sim(shape, body)
    sim.load(g)
    run_and_compare(sim, gens, want, plain_sim(shape, g))
    d = plan_is_the_tables(sim, shape)
    assert d["quiet_waves_skipped"] < d["quiet_waves_launched"]
    if tiles_of(shape) > 1:
        # Two strips: the narrow one is empty but for 2 x 256 generations.  Two groups: around generation
        # 224 both gliders are in rows 72 .. 84 of group 0, away from its first and last 12 rows.
        assert d["quiet_waves_skipped"] > 0


@shapes
@bodies
def test_empty_grid_is_extinct(gpu, shape, body):
    g, cpu, cells, plain, _ = stops_of("empty", shape)
    assert cpu[3] and not cells.any(), cpu
    sim = body_sim(shape, body, gen_limit=3000)
    sim.load(g)
    got = report(sim.run())
    assert got == cpu == plain, (got, cpu, plain)
    assert not sim.tile().any()
    plan_is_the_tables(sim, shape)


def test_auto_policy_on_two_by_two(gpu):
    """The auto policy of tests/test_quiet_auto_gpu.py on 2048 x 192: all four tiles are clean once the soup
    has settled."""
    shape, gens = (2048, 192), (7, 100, 355, 600)
    g, want = oracle_of("p2", shape, gens)
    late = [life_step_torch_roll(want[355], n, device="cuda") for n in (5, 5 + T)]  # generations 360 and 372
    clean = [np.array_equal(late[0][y:y + GROUP, x:x1], late[1][y:y + GROUP, x:x1])
             for x, x1 in ((0, STRIP), (STRIP, 2048)) for y in (0, GROUP)]
    assert 100 * sum(clean) // 4 >= 25 + 20
    sim = sim_of(shape, {"quiet_skip": "-1", "quiet_scout": "2", "quiet_on": "25", "quiet_rows": str(GROUP)}, tmax=T)
    assert sim.describe()["quiet_mode"] == "auto:dense"
    sim.load(g)
    run_and_compare(sim, gens, want)
    sim.native_engine.quiet_waves_skipped  # polls the newest report
    d = sim.describe()
    b = d["quiet_blocks"]
    assert d["quiet_mode"] == "auto:skipping" and b["dense"] > 0 and b["scout"] > 0 and b["skip"] > 0, (d["quiet_mode"], b)
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]
    assert d["quiet_waves_launched"] == 4 * 4 * (b["scout"] + b["skip"])
