"""The per-generation population census (LifeConfig.census) on the HIP engine
(MI355X): the census kernels against the PyTorch fp32 oracle stepped one
generation at a time on the GPU, in the classic and grouped schedules and both
layouts, the smallest grids, a row-ring tile, subdomains, the RCCL sum, what
describe() reports and the combinations that are refused.  Every case asserts
the whole series and the final grid."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation, life_step_torch, random_grid
from gol_amd.parallel import InProcessGroup

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture
def tune():
    """The byte-layout tests here run the byte kernels themselves; the test of
    the device default (byte grid on bit words) drops the key."""
    return {"u8_via_bits": "0"}


@functools.lru_cache(maxsize=None)
def oracle(W, H, seed, gens, density=0.4):
    """Grid, its `gens`-th generation and the live cells of generations
    1..gens (fp32 conv on the GPU, one generation per call, summed each step),
    computed once per case and shared; callers modify none of them."""
    g = random_grid(W, H, seed, density)
    x, pop = g, []
    for _ in range(gens):
        x = life_step_torch(x, 1, device="cuda")
        pop.append(int(x.sum(dtype=np.int64)))
    pop = np.array(pop, dtype=np.int64)
    for a in (g, x, pop):
        a.setflags(write=False)
    return g, x, pop


def run_hip(g, gens, census=True, **cfg):
    H, W = g.shape
    sim = Simulation(LifeConfig(W, H, gen_limit=gens, check_similarity=False, census=census, **cfg), engine="hip")
    sim.load(g)
    rep = sim.advance(gens)
    return sim, rep


def assert_census(sim, rep, want, pop, path=None):
    """The whole series and the final grid; what describe() says of every
    census engine; the launch path the case is named for."""
    d = sim.describe()
    assert rep.population.dtype == np.int64 and len(rep.population) == len(pop)
    bad = np.flatnonzero(rep.population != pop)
    assert bad.size == 0, (bad[:8], rep.population[bad[:8]], pop[bad[:8]])
    assert (sim.tile() == want).all()
    assert sim.alive_count() == pop[-1]
    assert d["census"] is True and "census" in d["kernel"] and "dpp census" in d["kernel"]
    assert d["drifting"] is False and d["quiet_mode"] == "off" and d["graphs"] is False
    assert d["tail_overshoots"] == 0 and d["tail_replays"] == 0
    paths = d["launch_paths"]
    assert paths["linked"] == 0 and paths["chained"] == 0 and paths["skipping"] == 0 and paths["lds_tiled"] == 0
    assert rep.linked_launches == 0
    if path == "classic":
        assert paths["classic"] > 0 and paths["grouped"] == 0, paths
    elif path == "grouped":
        assert paths["grouped"] > 0, paths
    return d


# ---- 1. bit kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("deep", [True, False])
@pytest.mark.parametrize("tmax", [1, 2, 4, 8, 12, 16])
def test_census_bit_kernels(gpu, tune, tmax, deep):
    """3968 cells = 124 words: two column strips with a tail; 333 rows: several
    row segments with remainders; 3 T + 1 generations.  epoch = 2 T: the first
    block of every epoch computes T halo rows above and below the tile, which
    hold live cells and are not counted."""
    W, H, gens = 3968, 333, 3 * tmax + 1
    g, want, pop = oracle(W, H, 11 + tmax, gens)
    sim, rep = run_hip(g, gens, layout="bits", tmax=tmax, epoch=2 * tmax if deep else 0, tune=tune)
    d = assert_census(sim, rep, want, pop, "classic" if tmax < 4 else "grouped")
    assert d["tmax"] == tmax
    if deep:
        assert d["epoch"] == 2 * tmax and d["halo_rows"] == 2 * tmax and d["row_ring"] is False


# ---- 2. grouped schedules -----------------------------------------------------------------
@pytest.mark.parametrize("tmax", [4, 16])
@pytest.mark.parametrize("group", [0, 4, 8])
def test_census_grouped_schedules(gpu, tune, group, tmax):
    """The classic ends of wave 0 and wave M - 1 of a group, and the rows a
    wave is fed from LDS by the wave below (evaluated once, counted once)."""
    tune["group"] = str(group)
    W, H, gens = 6400, 700, 2 * tmax + 3
    g, want, pop = oracle(W, H, tmax, gens)
    sim, rep = run_hip(g, gens, layout="bits", tmax=tmax, tune=tune)
    assert_census(sim, rep, want, pop, "classic" if group == 0 else "grouped")


# ---- 3. byte kernels ------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(33, 33), (257, 129), (1999, 301)])
def test_census_byte_kernels(gpu, tune, W, H):
    """Widths that are no multiple of 32: the bits beyond W in the last word."""
    g, want, pop = oracle(W, H, W * 7 + H, 17)
    sim, rep = run_hip(g, 17, layout="u8", tune=tune)
    d = assert_census(sim, rep, want, pop)
    assert d["u8_compute"] == "bytes" and d["tmax"] <= 16


@pytest.mark.parametrize("tmax", [1, 8, 16])
def test_census_byte_kernels_every_t(gpu, tune, tmax):
    W, H, gens = 1999, 301, 17
    g, want, pop = oracle(W, H, W * 7 + H, gens)
    sim, rep = run_hip(g, gens, layout="u8", tmax=tmax, tune=tune)
    d = assert_census(sim, rep, want, pop, "classic" if tmax < 4 else "grouped")
    assert d["u8_compute"] == "bytes" and d["tmax"] == tmax


# ---- 4. byte layout on bit words, the device default -------------------------------------------
def test_census_u8_via_bits(gpu, tune):
    del tune["u8_via_bits"]
    W, H, gens = 2048, 130, 37
    g, want, pop = oracle(W, H, 3, gens)
    sim, rep = run_hip(g, gens, layout="u8", tune=tune)
    d = assert_census(sim, rep, want, pop)
    assert d["u8_compute"] == "bits" and "bits wpl=1 dpp census" in d["kernel"]


# ---- 5. the smallest grids --------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,layout", [(32, 1, "bits"), (32, 2, "bits"), (64, 3, "bits"), (1, 1, "u8"), (2, 3, "u8")])
def test_census_smallest_grids(gpu, tune, W, H, layout):
    g, want, pop = oracle(W, H, 2, 20, 0.6)
    for tmax in (0, 1):
        sim, rep = run_hip(g, 20, layout=layout, tmax=tmax, tune=tune)
        assert_census(sim, rep, want, pop)


# ---- 6. a row-ring tile ----------------------------------------------------------------------------------
def test_census_on_a_row_ring(gpu, tune):
    """The census keeps the row ring and the wrapped column reads: a ring block
    covers exactly the owned rows.  The linked launches the torus runs on this
    tile are off."""
    W, H, gens = 8192, 4096, 45
    torus = Simulation(LifeConfig(W, H, tune=tune), engine="hip").describe()
    assert torus["row_ring"] is True, "the torus is no ring here: the check below guards nothing"
    g, want, pop = oracle(W, H, 21, gens)
    sim, rep = run_hip(g, gens, tune=tune)
    d = assert_census(sim, rep, want, pop, "grouped")
    assert d["row_ring"] is True and d["halo_words"] == torus["halo_words"]
    assert rep.linked_launches == 0


# ---- 7. subdomains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,P,W,H", [("2x2", 4, 32 * 79 * 2, 700), ("1x3", 3, 2048, 390)])
def test_census_subdomains(gpu, tune, spec, P, W, H):
    """Every rank reports the global series (the sum over ranks), not its share."""
    gens = 40
    g, want, pop = oracle(W, H, 9, gens)
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, check_similarity=False, decomp=spec, tmax=8, epoch=16,
                                    census=True, tune=tune), P, engine="hip", devices=[0])
    grp.load(g)
    reps = grp.advance(gens)
    assert len(reps) == P
    for rep in reps:
        assert rep.population.tolist() == pop.tolist()
    assert (grp.gather() == want).all()
    for sim in grp.sims:
        paths = sim.describe()["launch_paths"]
        assert paths["linked"] == 0 and paths["chained"] == 0 and paths["skipping"] == 0 and paths["lds_tiled"] == 0


def test_census_rccl_sum(gpu):
    """Two rank processes sharing the GPU: the series goes through the native
    RCCL transport's ncclAllReduce(ncclSum, ncclUint64), covered the way
    tests/test_rccl_multirank.py covers the flag all-reduce."""
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "1"
    env.pop("GOL_HOST_THREADS", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node=2", "--standalone",
           "--local-addr=127.0.0.1", str(REPO / "tests" / "mp_rccl_census_worker.py"), "1x2:bits,2x1:u8"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "CENSUS PASS world=2" in r.stdout, r.stderr[-4000:]


# ---- 8. a forced adder window --------------------------------------------------------------------------------
def test_forced_adder_window_runs_dpp(gpu, tune):
    """xlane=3 with the census runs the DPP window and says so."""
    tune["xlane"] = "3"
    tmax = 12
    W, H, gens = 3968, 333, 3 * tmax + 1
    g, want, pop = oracle(W, H, 11 + tmax, gens)
    sim, rep = run_hip(g, gens, layout="bits", tmax=tmax, tune=tune)
    d = assert_census(sim, rep, want, pop, "grouped")
    assert "xlane=add runs dpp" in d["kernel"]
    assert Simulation(LifeConfig(W, H, layout="bits", tmax=tmax, tune=tune), engine="hip").describe()["drifting"] is True


# ---- 9. refusals -------------------------------------------------------------------------------------------------
def test_census_refusals_name_the_combination(gpu, tune):
    with pytest.raises(RuntimeError, match="census=1 with rule B36/S23 on the HIP engine"):
        Simulation(LifeConfig(256, 128, census=True, rule="highlife", tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="census=1 with boundary=dead on the HIP engine"):
        Simulation(LifeConfig(256, 128, census=True, boundary="dead", tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="census=1 with u8_kernel=lds"):
        Simulation(LifeConfig(200, 128, layout="u8", census=True, tune=dict(tune, u8_kernel="lds")), engine="hip")
    with pytest.raises(RuntimeError, match="census=1 with graphs=1"):
        Simulation(LifeConfig(256, 128, census=True, graphs="on", tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="census=1 with self_exchange"):
        Simulation(LifeConfig(256, 128, census=True, self_exchange=True, tune=tune), engine="hip")
    # each of them is fine without the census
    Simulation(LifeConfig(256, 128, rule="highlife", tune=tune), engine="hip")
    Simulation(LifeConfig(256, 128, boundary="dead", tune=tune), engine="hip")
    Simulation(LifeConfig(200, 128, layout="u8", tune=dict(tune, u8_kernel="lds")), engine="hip")


# ---- 10. census off ----------------------------------------------------------------------------------------------
def test_census_off_on_hip(gpu, tune):
    W, H, gens = 3968, 333, 49
    g, want, pop = oracle(W, H, 27, gens)
    off, rep_off = run_hip(g, gens, census=False, layout="bits", tune=tune)
    assert rep_off.population.dtype == np.int64 and len(rep_off.population) == 0
    d = off.describe()
    assert d["census"] is False and "census" not in d["kernel"]
    assert (off.tile() == want).all()
    on, rep_on = run_hip(g, gens, layout="bits", tune=tune)
    assert_census(on, rep_on, want, pop)
    assert (on.tile() == off.tile()).all()


def test_census_chunked_equals_whole_on_hip(gpu, tune):
    """Chunks whose remainder blocks differ from the whole run's: the same series."""
    W, H = 3968, 333
    g, want, pop = oracle(W, H, 5, 100)
    sim = Simulation(LifeConfig(W, H, gen_limit=10**6, check_similarity=False, census=True, tune=tune), engine="hip")
    sim.load(g)
    got = np.concatenate([sim.advance(n).population for n in (37, 5, 58)])
    assert got.tolist() == pop.tolist()
    assert (sim.tile() == want).all()
