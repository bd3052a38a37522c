"""Cycle detection on the HIP engine (MI355X): the fingerprint kernels against
the NumPy oracle of tests/cycle_oracle.py over grids stepped one generation at a
time by the PyTorch fp32 oracle on the GPU - the classic and grouped schedules,
both layouts, the smallest grids, a row-ring tile, subdomains with non-zero
column offsets, the RCCL sum - the stand-alone tile kernels, find_cycle, the
combinations that are refused and what stays untouched.  Every series case
asserts the whole series and the final grid."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cycle_oracle as co
from gol_amd import LifeConfig, Simulation, life_step_numpy, life_step_torch, random_grid
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
    """Grid, its `gens`-th generation and the fingerprints of generations
    1..gens (fp32 conv on the GPU, one generation per call; the fingerprint of
    each by the NumPy oracle), computed once per case and shared; callers modify
    none of them."""
    g = random_grid(W, H, seed, density)
    x, fps = g, []
    for _ in range(gens):
        x = life_step_torch(x, 1, device="cuda")
        fps.append(co.fingerprint(x))
    fps = np.array(fps, dtype=np.uint64)
    for a in (g, x, fps):
        a.setflags(write=False)
    return g, x, fps


def run_hip(g, gens, fingerprint=True, **cfg):
    H, W = g.shape
    sim = Simulation(LifeConfig(W, H, gen_limit=gens, check_similarity=False, fingerprint=fingerprint, **cfg),
                     engine="hip")
    sim.load(g)
    rep = sim.advance(gens)
    return sim, rep


def assert_series(sim, rep, want, fps, path=None):
    """The whole series and the final grid; what describe() says of every
    fingerprint engine; the launch path the case is named for."""
    d = sim.describe()
    assert rep.fingerprint.dtype == np.uint64 and len(rep.fingerprint) == len(fps)
    bad = np.flatnonzero(rep.fingerprint != fps)
    assert bad.size == 0, (bad[:8], rep.fingerprint[bad[:8]], fps[bad[:8]])
    assert (sim.tile() == want).all()
    assert d["fingerprint"] is True and "dpp fingerprint" in d["kernel"]
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
def test_fingerprint_bit_kernels(gpu, tune, tmax, deep):
    """3968 cells = 124 words: two column strips with a tail; 333 rows: several
    row segments with remainders; 3 T + 1 generations.  epoch = 2 T: the first
    block of every epoch computes T halo rows above and below the tile, which
    hold live cells and are not weighed."""
    W, H, gens = 3968, 333, 3 * tmax + 1
    g, want, fps = oracle(W, H, 11 + tmax, gens)
    sim, rep = run_hip(g, gens, layout="bits", tmax=tmax, epoch=2 * tmax if deep else 0, tune=tune)
    d = assert_series(sim, rep, want, fps, "classic" if tmax < 4 else "grouped")
    assert d["tmax"] == tmax
    if deep:
        assert d["epoch"] == 2 * tmax and d["halo_rows"] == 2 * tmax and d["row_ring"] is False


# ---- 2. grouped schedules -----------------------------------------------------------------
@pytest.mark.parametrize("tmax", [4, 16])
@pytest.mark.parametrize("group", [0, 4, 8])
def test_fingerprint_grouped_schedules(gpu, tune, group, tmax):
    tune["group"] = str(group)
    W, H, gens = 6400, 700, 2 * tmax + 3
    g, want, fps = oracle(W, H, tmax, gens)
    sim, rep = run_hip(g, gens, layout="bits", tmax=tmax, tune=tune)
    assert_series(sim, rep, want, fps, "classic" if group == 0 else "grouped")


# ---- 3. byte kernels ------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(33, 33), (257, 129), (1999, 301)])
def test_fingerprint_byte_kernels(gpu, tune, W, H):
    """Widths that are no multiple of 32: the bits beyond W in the last word."""
    g, want, fps = oracle(W, H, W * 7 + H, 17)
    sim, rep = run_hip(g, 17, layout="u8", tune=tune)
    d = assert_series(sim, rep, want, fps)
    assert d["u8_compute"] == "bytes" and d["tmax"] <= 16


@pytest.mark.parametrize("tmax", [1, 8, 16])
def test_fingerprint_byte_kernels_every_t(gpu, tune, tmax):
    W, H, gens = 1999, 301, 17
    g, want, fps = oracle(W, H, W * 7 + H, gens)
    sim, rep = run_hip(g, gens, layout="u8", tmax=tmax, tune=tune)
    d = assert_series(sim, rep, want, fps, "classic" if tmax < 4 else "grouped")
    assert d["u8_compute"] == "bytes" and d["tmax"] == tmax


def test_fingerprint_u8_via_bits(gpu, tune):
    """The byte layout on bit words, the device default."""
    del tune["u8_via_bits"]
    W, H, gens = 2048, 130, 37
    g, want, fps = oracle(W, H, 3, gens)
    sim, rep = run_hip(g, gens, layout="u8", tune=tune)
    d = assert_series(sim, rep, want, fps)
    assert d["u8_compute"] == "bits" and "bits wpl=1 dpp fingerprint" in d["kernel"]
    assert sim.fingerprint() == int(fps[-1])  # of the live bit image


# ---- 4. the smallest grids --------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,layout", [(32, 1, "bits"), (32, 2, "bits"), (64, 3, "bits"), (1, 1, "u8"), (2, 3, "u8")])
def test_fingerprint_smallest_grids(gpu, tune, W, H, layout):
    g, want, fps = oracle(W, H, 2, 20, 0.6)
    for tmax in (0, 1):
        sim, rep = run_hip(g, 20, layout=layout, tmax=tmax, tune=tune)
        assert_series(sim, rep, want, fps)


# ---- 5. a row-ring tile ----------------------------------------------------------------------------------
def test_fingerprint_on_a_row_ring(gpu, tune):
    """The ring's halo rows are second mappings of owned rows: a ring block
    weighs exactly the owned rows, each by its own global row."""
    W, H, gens = 8192, 4096, 45
    torus = Simulation(LifeConfig(W, H, tune=tune), engine="hip").describe()
    assert torus["row_ring"] is True, "the torus is no ring here: the check below guards nothing"
    g, want, fps = oracle(W, H, 21, gens)
    sim, rep = run_hip(g, gens, tune=tune)
    d = assert_series(sim, rep, want, fps, "grouped")
    assert d["row_ring"] is True and d["halo_words"] == torus["halo_words"]


# ---- 6. subdomains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,P,W,H", [("2x2", 4, 32 * 79 * 2, 700), ("1x3", 3, 2048, 390)])
def test_fingerprint_subdomains(gpu, tune, spec, P, W, H):
    """Every rank reports the global series.  The 2x2 tiles of the right column
    start at word 79 and those of the lower rows at row 350: a wrong global word
    or row index shows here."""
    gens = 40
    g, want, fps = oracle(W, H, 9, gens)
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, check_similarity=False, decomp=spec, tmax=8, epoch=16,
                                    fingerprint=True, tune=tune), P, engine="hip", devices=[0])
    grp.load(g)
    assert grp.fingerprint() == [co.fingerprint(g)] * P
    reps = grp.advance(gens)
    assert len(reps) == P
    for rep in reps:
        assert rep.fingerprint.tolist() == fps.tolist()
    assert (grp.gather() == want).all()
    for sim in grp.sims:
        paths = sim.describe()["launch_paths"]
        assert paths["linked"] == 0 and paths["chained"] == 0 and paths["skipping"] == 0 and paths["lds_tiled"] == 0


def test_fingerprint_byte_subdomains(gpu, tune):
    """Byte kernels on tiles whose first column is word 24 of the grid."""
    W, H, gens = 32 * 24 * 2, 213, 40
    g, want, fps = oracle(W, H, 13, gens)
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, check_similarity=False, decomp="2x1", layout="u8", tmax=8,
                                    epoch=16, fingerprint=True, tune=tune), 2, engine="hip", devices=[0])
    grp.load(g)
    for rep in grp.advance(gens):
        assert rep.fingerprint.tolist() == fps.tolist()
    assert (grp.gather() == want).all() and grp.sims[1].describe()["u8_compute"] == "bytes"


# ---- 7. two RCCL ranks ------------------------------------------------------------------------------------
def test_fingerprint_rccl_sum(gpu):
    """Two rank processes sharing the GPU: the series goes through the native
    RCCL transport's ncclAllReduce(ncclSum, ncclUint64), modulo 2^64."""
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "1"
    env.pop("GOL_HOST_THREADS", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node=2", "--standalone",
           "--local-addr=127.0.0.1", str(REPO / "tests" / "mp_rccl_cycle_worker.py"), "1x2:bits,2x1:u8"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "CYCLE PASS world=2" in r.stdout, r.stderr[-4000:]


# ---- 8. the stand-alone kernels -----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,layout", [(3968, 333, "bits"), (1999, 301, "u8")])
def test_standalone_fingerprint(gpu, tune, W, H, layout):
    g, want, fps = oracle(W, H, 19, 25) if layout == "bits" else oracle(W, H, W * 7 + H, 17)  # shared with 1. and 3.
    sim, rep = run_hip(g, len(fps), layout=layout, tune=tune)
    assert sim.fingerprint() == int(fps[-1]) == int(rep.fingerprint[-1])
    # on an engine without the setting too, before and after a run
    off = Simulation(LifeConfig(W, H, check_similarity=False, layout=layout, tune=tune), engine="hip")
    off.load(g)
    assert off.fingerprint() == co.fingerprint(g)
    off.advance(len(fps))
    assert off.fingerprint() == int(fps[-1])


@pytest.fixture(scope="module")
def board():
    b = co.pattern_board()
    entry, period, grids = co.brute_cycle(b, life_step_numpy, 400)
    assert (entry, period) == (9, 30)
    return b, grids


def test_equal_kernel_rejects_and_confirms(gpu, tune, board):
    """launch_equal through find_cycle's confirmation: with no bits compared
    every period is a candidate, the first search (generation 7) is in the
    transient and every comparison there must say 'differs'; the next one finds
    the repeat."""
    b, grids = board
    sim = Simulation(LifeConfig(96, 48, check_similarity=False, fingerprint=True,
                                tune=dict(tune, cycle_match_bits=0)), engine="hip")
    sim.load(b)
    r = sim.find_cycle(400, 64, 7)
    assert r.period == 30 and r.false_candidates > 0 and r.stop_reason == "cycle"
    assert (sim.tile() == grids[9 + (r.generation - 9) % 30]).all()


# ---- 9. find_cycle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bits", "u8"])
@pytest.mark.parametrize("chunk", [7, 64, 0])
def test_find_cycle_on_the_pattern_board(gpu, tune, board, chunk, layout):
    b, grids = board
    sim = Simulation(LifeConfig(96, 48, check_similarity=False, layout=layout, fingerprint=True, tune=tune),
                     engine="hip")
    sim.load(b)
    r = sim.find_cycle(400, 64, chunk)
    assert r.period == 30 and r.repeats_from == 9 and r.stop_reason == "cycle" and r.false_candidates == 0
    assert r.generation == sim.generation
    assert 9 + 2 * 30 - 1 <= r.generation <= 9 + 2 * 30 - 1 + (chunk or 256) + 30
    assert (sim.tile() == grids[9 + (r.generation - 9) % 30]).all()


def test_find_cycle_on_a_soup(gpu, tune):
    g = random_grid(64, 40, 3, 0.4)
    entry, period, grids = co.brute_cycle(g, life_step_numpy, 6000)
    assert entry is not None and period <= 300, "brute force found no cycle of period <= 300 within the limit"
    sim = Simulation(LifeConfig(64, 40, check_similarity=False, fingerprint=True, tune=tune), engine="hip")
    sim.load(g)
    r = sim.find_cycle(6000, 300)
    assert (r.period, r.repeats_from, r.stop_reason) == (period, entry, "cycle")
    assert (sim.tile() == grids[entry + (r.generation - entry) % period]).all()


def test_bounds_and_stops_on_hip(gpu, tune, board):
    b, _ = board
    sim = Simulation(LifeConfig(96, 48, check_similarity=False, fingerprint=True, tune=tune), engine="hip")
    sim.load(b)
    r = sim.find_cycle(400, 29)
    assert r.period == 0 and r.stop_reason == "limit" and sim.generation == 400
    blk = Simulation(LifeConfig(96, 48, check_similarity=False, fingerprint=True, tune=tune), engine="hip")
    blk.load(co.pattern_board(["block"]))
    r = blk.find_cycle(400, 64)
    assert r.period == 1 and r.stop_reason == "cycle"


# ---- 10. refusals -------------------------------------------------------------------------------------------------
def test_fingerprint_refusals_name_the_combination(gpu, tune):
    with pytest.raises(RuntimeError, match="fingerprint=1 with rule B36/S23 on the HIP engine"):
        Simulation(LifeConfig(256, 128, fingerprint=True, rule="highlife", tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="fingerprint=1 with boundary=dead on the HIP engine"):
        Simulation(LifeConfig(256, 128, fingerprint=True, boundary="dead", tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="fingerprint=1 with census=1 on the HIP engine"):
        Simulation(LifeConfig(256, 128, fingerprint=True, census=True, tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="fingerprint=1 with u8_kernel=lds"):
        Simulation(LifeConfig(200, 128, layout="u8", fingerprint=True, tune=dict(tune, u8_kernel="lds")), engine="hip")
    with pytest.raises(RuntimeError, match="fingerprint=1 with graphs=1"):
        Simulation(LifeConfig(256, 128, fingerprint=True, graphs="on", tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="fingerprint=1 with self_exchange"):
        Simulation(LifeConfig(256, 128, fingerprint=True, self_exchange=True, tune=tune), engine="hip")
    with pytest.raises(RuntimeError, match="fingerprint=1 with decomposition 2x1 of a byte-layout grid 200 cells wide"):
        InProcessGroup(LifeConfig(200, 128, layout="u8", decomp="2x1", fingerprint=True, tune=tune), 2, engine="hip",
                       devices=[0])
    # each of them is fine without the fingerprint
    Simulation(LifeConfig(256, 128, rule="highlife", tune=tune), engine="hip")
    Simulation(LifeConfig(256, 128, boundary="dead", tune=tune), engine="hip")
    Simulation(LifeConfig(256, 128, census=True, tune=tune), engine="hip")
    Simulation(LifeConfig(200, 128, layout="u8", tune=dict(tune, u8_kernel="lds")), engine="hip")
    Simulation(LifeConfig(256, 128, graphs="on", tune=tune), engine="hip")
    Simulation(LifeConfig(256, 128, self_exchange=True, tune=tune), engine="hip")
    InProcessGroup(LifeConfig(200, 128, layout="u8", decomp="2x1", tune=tune), 2, engine="hip", devices=[0])
    # and Px == 1 and the bit layout's splits are fine with it
    InProcessGroup(LifeConfig(200, 128, layout="u8", decomp="1x2", fingerprint=True, tune=tune), 2, engine="hip",
                   devices=[0])
    InProcessGroup(LifeConfig(256, 128, layout="bits", decomp="2x1", fingerprint=True, tune=tune), 2, engine="hip",
                   devices=[0])


# ---- 11. what stays untouched ---------------------------------------------------------------------------------------
def test_census_and_plain_engines_untouched(gpu, tune):
    W, H, gens = 3968, 333, 49
    g, want, fps = oracle(W, H, 27, gens)
    plain, rep_plain = run_hip(g, gens, fingerprint=False, layout="bits", tune=tune)
    d = plain.describe()
    assert len(rep_plain.fingerprint) == 0 and d["fingerprint"] is False and "fingerprint" not in d["kernel"]
    assert d["kernel"].startswith("bit-sliced temporal blocks, T=") and (plain.tile() == want).all()
    cen, rep_cen = run_hip(g, gens, fingerprint=False, census=True, layout="bits", tune=tune)
    dc = cen.describe()
    assert "dpp census" in dc["kernel"] and "fingerprint" not in dc["kernel"]
    assert len(rep_cen.population) == gens and len(rep_cen.fingerprint) == 0 and (cen.tile() == want).all()
    on, rep_on = run_hip(g, gens, layout="bits", tune=tune)
    assert_series(on, rep_on, want, fps)
    assert (on.tile() == plain.tile()).all()


def test_fingerprint_chunked_equals_whole_on_hip(gpu, tune):
    W, H = 3968, 333
    g, want, fps = oracle(W, H, 5, 100)
    sim = Simulation(LifeConfig(W, H, gen_limit=10**6, check_similarity=False, fingerprint=True, tune=tune),
                     engine="hip")
    sim.load(g)
    got = np.concatenate([sim.advance(n).fingerprint for n in (37, 5, 58)])
    assert got.tolist() == fps.tolist()
    assert (sim.tile() == want).all()
