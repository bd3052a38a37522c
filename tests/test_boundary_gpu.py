"""The bounded plane (boundary="dead") on the HIP engine (MI355X): the plane
kernels against the PyTorch fp32 oracle on the GPU in the classic and grouped
schedules and both layouts, the smallest grids, a tile that would be a row ring
on the torus, subdomains, termination, what describe() reports and the
combinations that are refused."""
import functools

import pytest

from gol_amd import LifeConfig, Simulation, life_step_torch, random_grid, reference_run, simulate
from gol_amd.parallel import InProcessGroup

from test_boundary import TERMINATION, reference_outcome

pytestmark = pytest.mark.gpu


@pytest.fixture
def tune():
    """The byte-layout tests here run the byte kernels themselves; the test of
    the device default (byte grid on bit words) drops the key."""
    return {"u8_via_bits": "0"}


@functools.lru_cache(maxsize=None)
def oracle(W, H, seed, density, gens):
    """Grid and its `gens`-th generation on the plane (fp32 conv on the GPU),
    computed once per case and shared; callers do not modify either."""
    g = random_grid(W, H, seed, density)
    want = life_step_torch(g, gens, device="cuda", boundary="dead")
    g.setflags(write=False)
    want.setflags(write=False)
    return g, want


def run_hip(g, gens, **cfg):
    H, W = g.shape
    sim = Simulation(LifeConfig(W, H, gen_limit=gens, boundary="dead", **cfg), engine="hip")
    sim.load(g)
    rep = sim.advance(gens)
    return sim, rep


def assert_plane(d):
    """What describe() says of every plane engine."""
    assert d["boundary"] == "dead" and "boundary dead" in d["kernel"]
    assert d["drifting"] is False and d["row_ring"] is False and d["quiet_mode"] == "off"
    assert d["halo_words"] > 0
    assert d["launch_paths"]["linked"] == 0 and d["launch_paths"]["chained"] == 0
    assert d["launch_paths"]["skipping"] == 0 and d["launch_paths"]["lds_tiled"] == 0


# ---- 1. bit kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("tmax", [1, 8, 12, 16])
def test_plane_bit_kernels_vs_torch(gpu, tune, tmax):
    """3968 cells = 124 words: two column strips with a tail; 333 rows: several
    row segments with remainders; 3 T + 1 generations: several blocks per epoch
    (epoch = 2 T), whose first ones mask rows that lie deep in the halo."""
    W, H, gens = 3968, 333, 3 * tmax + 1
    g, want = oracle(W, H, 11 + tmax, 0.4, gens)
    sim, _ = run_hip(g, gens, layout="bits", tmax=tmax, epoch=2 * tmax, tune=tune)
    d = sim.describe()
    assert d["tmax"] == tmax and d["epoch"] == 2 * tmax and d["halo_rows"] == 2 * tmax
    assert_plane(d)
    assert (sim.tile() == want).all()
    # the default epoch of a single rank: one block, no deep halo
    sim, _ = run_hip(g, gens, layout="bits", tmax=tmax, tune=tune)
    assert sim.describe()["epoch"] == tmax
    assert (sim.tile() == want).all()


@pytest.mark.parametrize("tmax", [12, 16])
def test_forced_adder_window_runs_dpp(gpu, tune, tmax):
    """xlane=3 on the plane runs the DPP window (the adder window's drifting
    frame is a relabelling of torus columns) and says so."""
    tune["xlane"] = "3"
    W, H, gens = 3968, 333, 3 * tmax + 1
    g, want = oracle(W, H, 11 + tmax, 0.4, gens)
    sim, _ = run_hip(g, gens, layout="bits", tmax=tmax, tune=tune)
    d = sim.describe()
    assert_plane(d)
    assert "dpp plane" in d["kernel"] and "xlane=add runs dpp" in d["kernel"]
    assert (sim.tile() == want).all()


# ---- 2. grouped schedules -----------------------------------------------------------------
@pytest.mark.parametrize("tmax", [4, 16])
@pytest.mark.parametrize("group", [0, 4, 8])
def test_plane_grouped_schedules(gpu, tune, group, tmax):
    tune["group"] = str(group)
    W, H, gens = 6400, 700, 2 * tmax + 3
    g, want = oracle(W, H, tmax, 0.4, gens)
    sim, _ = run_hip(g, gens, layout="bits", tmax=tmax, tune=tune)
    paths = sim.describe()["launch_paths"]
    assert (paths["grouped"] > 0) == (group != 0), paths
    assert_plane(sim.describe())
    assert (sim.tile() == want).all()


# ---- 3. byte kernels ------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(33, 33), (257, 129), (1999, 301)])
def test_plane_byte_kernels(gpu, tune, W, H):
    """Widths that are no multiple of 32: the partial last word's mask."""
    g, want = oracle(W, H, W * 7 + H, 0.4, 17)
    sim, _ = run_hip(g, 17, layout="u8", tune=tune)
    d = sim.describe()
    assert d["u8_compute"] == "bytes" and d["tmax"] <= 16
    assert_plane(d)
    assert (sim.tile() == want).all()


@pytest.mark.parametrize("tmax", [1, 8, 16])
def test_plane_byte_kernels_every_t(gpu, tune, tmax):
    W, H, gens = 1999, 301, 2 * tmax + 5
    g, want = oracle(W, H, 5 + tmax, 0.4, gens)
    sim, _ = run_hip(g, gens, layout="u8", tmax=tmax, tune=tune)
    assert (sim.tile() == want).all()


def test_plane_byte_kernels_cap_t_at_16(gpu, tune):
    """A byte tile large enough for the torus's T = 32 passes."""
    W, H = 32768, 8192
    assert Simulation(LifeConfig(W, H, layout="u8", tune=tune), engine="hip").describe()["tmax"] > 16
    d = Simulation(LifeConfig(W, H, layout="u8", boundary="dead", tune=tune), engine="hip").describe()
    assert d["tmax"] == 16 and "T <= 16" in d["kernel"]


# ---- 4. byte layout on bit words, the device default -------------------------------------------
def test_plane_u8_via_bits(gpu, tune):
    del tune["u8_via_bits"]
    W, H, gens = 2048, 130, 37
    g, want = oracle(W, H, 3, 0.4, gens)
    sim, _ = run_hip(g, gens, layout="u8", tune=tune)
    assert sim.describe()["u8_compute"] == "bits"
    assert_plane(sim.describe())
    assert (sim.tile() == want).all()


# ---- 5. the smallest grids --------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,layout", [(32, 1, "bits"), (32, 2, "bits"), (64, 3, "bits"), (1, 1, "u8"), (2, 3, "u8")])
def test_plane_smallest_grids(gpu, tune, W, H, layout):
    g, want = oracle(W, H, 2, 0.6, 20)
    for tmax in (0, 1):
        sim, _ = run_hip(g, 20, layout=layout, tmax=tmax, tune=tune)
        assert (sim.tile() == want).all(), tmax


# ---- 6. a tile that would be a row ring on the torus ---------------------------------------------------
def test_plane_where_the_torus_is_a_ring(gpu, tune):
    W, H, gens = 8192, 4096, 45
    torus = Simulation(LifeConfig(W, H, tune=tune), engine="hip").describe()
    assert torus["row_ring"] is True, "the torus is no ring here: the check below guards nothing"
    g, want = oracle(W, H, 21, 0.4, gens)
    sim, rep = run_hip(g, gens, tune=tune)
    assert_plane(sim.describe())
    assert rep.linked_launches == 0
    assert (sim.tile() == want).all()


# ---- 7. subdomains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,P,W,H", [("2x2", 4, 32 * 79 * 2, 700), ("1x3", 3, 2048, 390)])
def test_plane_subdomains(gpu, tune, spec, P, W, H):
    gens = 40
    g, want = oracle(W, H, 9, 0.4, gens)
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, decomp=spec, tmax=8, epoch=16, boundary="dead", tune=tune),
                         P, engine="hip", devices=[0])
    grp.load(g)
    grp.advance(gens)
    assert (grp.gather() == want).all()


# ---- 8. termination -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,reason", TERMINATION)
def test_plane_termination_hip(gpu, tune, grid, reason):
    g = grid()
    ref, rgens, rreason = reference_outcome(g)
    assert rreason == reason
    for layout in ("bits", "u8"):
        out, rep = simulate(g, 1000, engine="hip", layout=layout, boundary="dead", tune=tune)
        assert (rep.generations, rep.stop_reason) == (rgens, reason), layout
        assert (out == ref).all(), layout


# ---- 9. refusals -------------------------------------------------------------------------------------------------
def test_plane_refusals_name_the_combination(gpu, tune):
    with pytest.raises(RuntimeError, match="boundary=dead with u8_kernel=lds"):
        Simulation(LifeConfig(200, 128, layout="u8", boundary="dead", tune=dict(tune, u8_kernel="lds")), engine="hip")
    Simulation(LifeConfig(200, 128, layout="u8", tune=dict(tune, u8_kernel="lds")), engine="hip")  # the torus: fine
    with pytest.raises(RuntimeError, match="boundary=dead with graphs=1"):
        Simulation(LifeConfig(256, 128, boundary="dead", graphs="on", tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="boundary=dead with self_exchange"):
        Simulation(LifeConfig(256, 128, boundary="dead", self_exchange=True, tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="boundary=dead with rule B36/S23 on the HIP engine"):
        Simulation(LifeConfig(256, 128, boundary="dead", rule="highlife", tune=tune), engine="hip")
    # the CPU engine runs the rule on the plane
    g = random_grid(256, 64, 1)
    out, _ = simulate(g, 5, engine="cpu", check_similarity=False, rule="highlife", boundary="dead")
    assert (out == life_step_torch(g, 5, rule="highlife", boundary="dead")).all()
    assert (out == reference_run(g, 5, False, rule="highlife", boundary="dead")[0]).all()
