"""Density maps, window reads and pattern placement on the HIP engine
(csrc/kernels/view_ops.hip): every path of the density kernel (whole-word
counts, words cut at block edges, blocks narrower than a word, byte tiles, the
bit image of a byte engine, row rings, rank tiles off the word grid), windows
and stamps at word-straddling offsets, and the engine's preparation of each call
(lazy tail, drifted frame, quiet-tile skipping, subdomains, RCCL).

The oracle is NumPy on the whole host grid (tests/test_view.py) with the
generations stepped by the fp32 PyTorch oracle."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gol_amd import LifeConfig, Simulation, random_grid
from gol_amd.ops.life_ops import life_step_torch, life_step_torch_roll
from gol_amd.parallel import InProcessGroup

from test_view import GLIDER, density_oracle, rects_for

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]


def hip(W, H, **kw):
    kw.setdefault("gen_limit", 1_000_000)
    return Simulation(LifeConfig(W, H, **kw), engine="hip")


def stepped(g, n):
    return np.asarray(life_step_torch(g, n, device="cuda")) if n else np.asarray(g)


def check_windows_and_stamps(sim, want, seed=0):
    """Windows and stamps (alternating copy / or) at rects_for's rectangles and at word-straddling ones;
    returns the grid the engine should now hold."""
    H, W = want.shape
    want = np.array(want)
    rng = np.random.default_rng(seed)
    rects = rects_for(W, H) + [(29, 1, 7, 2), (W - 37, H - 2, 37, 2), (63, 0, 2, 1)]
    for i, (x, y, w, h) in enumerate(rects):
        assert (sim.window(x, y, w, h) == want[y:y + h, x:x + w]).all(), (x, y, w, h)
        stamp = (rng.random((h, w)) < 0.5).astype(np.uint8)
        if i % 2:
            sim.place(stamp, x, y, mode="or")
            want[y:y + h, x:x + w] |= stamp
        else:
            sim.place(stamp, x, y)
            want[y:y + h, x:x + w] = stamp
        assert (sim.window(0, 0, W, H) == want).all(), (x, y, w, h)
    return want


# ---- density ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def strips():
    """3968 x 333 (124 words: a chunk of 31 quads with a tail), advanced 5 generations on the device."""
    W, H = 3968, 333
    g = random_grid(W, H, 41, 0.4)
    sim = hip(W, H, layout="bits")
    sim.load(g)
    sim.advance(5)
    want = stepped(g, 5)
    want.setflags(write=False)
    return sim, want


@pytest.mark.parametrize("bx,by", [(32, 1), (32, 32), (64, 7), (33, 5), (1, 1), (3968, 333), (5000, 400)])
def test_density_bits(gpu, strips, bx, by):
    sim, want = strips
    d = sim.density((by, bx))
    assert d.dtype == np.int64 and (d == density_oracle(want, by, bx)).all()


def test_density_aligned_and_general_kernels_agree(gpu, strips):
    """A block of 32 k + 1 cells takes the kernel that cuts words; 32 of its block columns are one block of
    the whole-word kernel."""
    sim, want = strips
    general = sim.density((64, 33))
    aligned = sim.density((64, 33 * 32))
    pad = np.zeros((general.shape[0], -(-general.shape[1] // 32) * 32), np.int64)
    pad[:, :general.shape[1]] = general
    assert (pad.reshape(pad.shape[0], -1, 32).sum(2) == aligned).all()
    assert aligned.sum() == want.sum() == sim.alive_count()


@pytest.mark.parametrize("W", [33, 257, 1999])
def test_density_byte_kernels(gpu, W):
    H = 70
    g = random_grid(W, H, W, 0.4)
    sim = hip(W, H, layout="u8", tune={"u8_via_bits": "0"})
    assert sim.describe()["u8_compute"] == "bytes"
    sim.load(g)
    sim.advance(3)
    want = stepped(g, 3)
    for by, bx in [(1, 1), (32, 32), (5, 33), (7, 64), (H, W), (H + 9, W + 9)]:
        assert (sim.density((by, bx)) == density_oracle(want, by, bx)).all(), (by, bx)


def test_density_of_the_bit_image_of_a_byte_engine(gpu):
    W, H = 2048, 70
    g = random_grid(W, H, 6, 0.4)
    sim = hip(W, H, layout="u8")
    d = sim.describe()
    assert d["layout"] == "u8" and d["u8_compute"] == "bits"  # the blocks ran on the bit image, which is the state
    sim.load(g)
    sim.advance(20)
    want = stepped(g, 20)
    for by, bx in [(32, 32), (5, 33), (1, 1)]:
        assert (sim.density((by, bx)) == density_oracle(want, by, bx)).all(), (by, bx)
    assert (sim.tile() == want).all()


def test_views_on_a_row_ring(gpu):
    W, H = 96, 48  # the smallest ring of tests/test_row_ring.py
    g = random_grid(W, H, 9, 0.4)
    sim = hip(W, H, layout="bits", tmax=16)
    d = sim.describe()
    assert d["row_ring"], d["row_ring_fallback"]
    sim.load(g)
    sim.advance(37)
    want = stepped(g, 37)
    for by, bx in [(1, 1), (32, 32), (5, 33), (H, W)]:
        assert (sim.density((by, bx)) == density_oracle(want, by, bx)).all(), (by, bx)
    want = check_windows_and_stamps(sim, want)
    sim.advance(37)
    assert (sim.tile() == stepped(want, 37)).all()


# ---- the engine's preparation ------------------------------------------------------------------------

TAIL_W, TAIL_H, T = 5120, 768, 12  # the ring of tests/test_lazy_tail_gpu.py


@pytest.fixture(scope="module")
def tail_oracle():
    g = random_grid(TAIL_W, TAIL_H, 12, 0.3)
    at1000 = np.asarray(life_step_torch_roll(g, 1000, device="cuda"))
    return g, at1000


@pytest.mark.parametrize("op", ["density", "window", "place"])
def test_views_replay_a_lazy_tail(gpu, tail_oracle, op):
    g, want = tail_oracle
    sim = hip(TAIL_W, TAIL_H, layout="bits",
              tune={"quiet_skip": "1", "group": "4", "quiet_rows": "96", "lazy_tail": "1"})
    d = sim.describe()
    assert d["row_ring"] and d["tmax"] == T
    sim.load(g)
    sim.advance(1000)  # 83 blocks and 4 generations: the run ends on a full block
    d = sim.describe()
    assert (d["spine_generation"], d["tail_overshoots"], d["tail_replays"]) == (1008, 1, 0)
    if op == "density":
        assert (sim.density((96, 160)) == density_oracle(want, 96, 160)).all()
    elif op == "window":
        assert (sim.window(2031, 700, 200, 68) == want[700:768, 2031:2231]).all()
    else:
        sim.place(GLIDER, 2047, 95, mode="copy")
    d = sim.describe()
    assert (sim.generation, d["spine_generation"], d["tail_replays"]) == (1000, 1000, 1)
    if op == "place":
        w2 = np.array(want)
        w2[95:98, 2047:2050] = GLIDER
        sim.advance(40)
        assert (sim.tile() == np.asarray(life_step_torch_roll(w2, 40, device="cuda"))).all()


def test_views_with_a_drifted_frame(gpu):
    W, H, n = 2048, 333, 27
    g = random_grid(W, H, 31, 0.4)
    sim = hip(W, H, layout="bits", tmax=12, tune={"xlane": "3"})
    assert sim.describe()["drifting"]
    sim.load(g)
    sim.advance(n)
    assert sim.native_engine.drift == n
    want = stepped(g, n)
    assert (sim.density((5, 33)) == density_oracle(want, 5, 33)).all()
    sim.advance(n)
    assert sim.native_engine.drift == n
    want = stepped(want, n)
    assert (sim.window(2000, 300, 48, 33) == want[300:333, 2000:2048]).all()
    sim.advance(n)
    assert sim.native_engine.drift == n
    want = np.array(stepped(want, n))
    sim.place(GLIDER, 31, 100, mode="or")
    want[100:103, 31:34] |= GLIDER
    sim.advance(n)
    assert (sim.tile() == stepped(want, n)).all()


def test_place_into_a_clean_tile_of_a_skipping_run(gpu):
    """A stamp must make the skipping kernel recompute the tile it fell in."""
    from test_quiet_small_torus_gpu import GROUP, oracle_of, sim_of  # noqa: PLC0415

    shape, gens = (2048, 192), (7, 100, 355, 600)
    g, want = oracle_of("p2", shape, gens)
    sim = sim_of(shape, {"quiet_skip": "-1", "quiet_scout": "2", "quiet_on": "25", "quiet_rows": str(GROUP)}, tmax=T)
    sim.load(g)
    sim.advance(600)
    sim.native_engine.quiet_waves_skipped  # polls the newest report
    assert sim.describe()["quiet_mode"] == "auto:skipping"
    at = np.array(want[600])
    assert not at[30:60, 480:540].any()  # far from the soup: this tile was clean
    sim.place(GLIDER, 500, 40, mode="or")
    at[40:43, 500:503] |= GLIDER
    skipped = sim.describe()["quiet_blocks"]["skip"]
    sim.advance(2 * T)
    sim.native_engine.quiet_waves_skipped
    assert sim.describe()["quiet_blocks"]["skip"] > skipped  # (the policy may answer the recomputed tiles with a scout)
    assert (sim.tile() == np.asarray(life_step_torch_roll(at, 2 * T, device="cuda"))).all()


# ---- windows and stamps --------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,W,H,tune", [("bits", 3968, 333, {}), ("u8", 1999, 333, {"u8_via_bits": "0"}),
                                             ("u8", 2048, 40, {})])
def test_windows_and_stamps(gpu, layout, W, H, tune):
    g = random_grid(W, H, W + H, 0.4)
    sim = hip(W, H, layout=layout, tune=tune)
    sim.load(g)
    sim.advance(4)
    want = check_windows_and_stamps(sim, stepped(g, 4), seed=W)
    assert sim.generation == 4
    sim.advance(6)
    assert (sim.tile() == stepped(want, 6)).all()


@pytest.mark.parametrize("tmax", [1, 12, 16])
def test_place_then_blocks(gpu, tmax):
    W, H = 2048, 333
    sim = hip(W, H, layout="bits", tmax=tmax)
    sim.init_random(1, 0.0)
    want = np.zeros((H, W), np.uint8)
    soup = random_grid(70, 40, 8, 0.5)
    for stamp, x, y in [(GLIDER, 30, 331 - 3), (soup, 2048 - 70, 0), (soup, 991, 150)]:
        sim.place(stamp, x, y, mode="or")
        want[y:y + stamp.shape[0], x:x + stamp.shape[1]] |= stamp
    n = 3 * tmax + 1
    sim.advance(n)
    assert (sim.tile() == stepped(want, n)).all()
    assert sim.density(max(W, H))[0, 0] == stepped(want, n).sum()


# ---- subdomains ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,P,layout,W,H", [("1x2", 2, "bits", 2048, 201), ("2x2", 4, "bits", 32 * 79 * 2, 203),
                                               ("2x2", 4, "u8", 1999, 101)])
def test_views_across_ranks_on_one_gpu(gpu, spec, P, layout, W, H):
    g = random_grid(W, H, 13, 0.4)
    tune = {"u8_via_bits": "0"} if layout == "u8" else {}
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=1000, decomp=spec, layout=layout, tmax=8, epoch=16, tune=tune), P,
                         engine="hip", devices=[0])
    grp.load(g)
    grp.advance(9)
    want = stepped(g, 9)
    for by, bx in [(32, 32), (33, 33), (7, 5), (H, W), (70, 1000)]:
        ds = grp.density((by, bx))
        assert len(ds) == P and all((d == density_oracle(want, by, bx)).all() for d in ds), (by, bx)
    x, y = W // 2 - 20, H // 2 - 9  # over the corner of the four ranks (2x2), the rank boundary (1x2)
    for rect in [(x, y, 41, 19), (0, 0, W, H), (0, H // 2 - 1, W, 3)]:
        ws = grp.window(*rect)
        assert all((v == want[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]).all() for v in ws), rect
    stamp = (np.random.default_rng(3).random((19, 41)) < 0.5).astype(np.uint8)
    grp.place(stamp, x, y)
    want = np.array(want)
    want[y:y + 19, x:x + 41] = stamp
    grp.advance(13)
    assert (grp.gather() == stepped(want, 13)).all()


def test_views_rccl(gpu):
    """Two rank processes sharing the GPU: the block map and the window go through the native RCCL
    transport's 64-bit sum (tests/mp_rccl_view_worker.py), launched like tests/test_census_gpu.py's."""
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "1"
    env.pop("GOL_HOST_THREADS", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node=2", "--standalone",
           "--local-addr=127.0.0.1", str(REPO / "tests" / "mp_rccl_view_worker.py"), "1x2:bits,2x1:u8"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "VIEW PASS world=2" in r.stdout, r.stderr[-4000:]
