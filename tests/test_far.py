"""The sparse oracles of tests/far_oracle.py against whole-grid NumPy, on a grid
a host can hold, and the identical island and soup procedures on the CPU
engine: what tests/test_far_gpu.py trusts on buffers beyond 4 GiB is shown
here to be what a whole-grid oracle gives.  Also the geometry arithmetic of the
largest tiles BASELINE.md lists, against Python's big integers."""
import numpy as np
import pytest

import batch_oracle
import cycle_oracle
import far_oracle as fo
from gol_amd import LifeConfig, Simulation, random_grid
from test_view import density_oracle

W, H, N = 2048, 600, 13  # n = 3 T + 1 at T = 4
SOUP_SEEDS = (5,)        # the seeds tests/test_far_gpu.py draws its dense soups from (far_oracle.run_soup)


def whole_grid_gens(g, n, rule, boundary):
    gens = [g]
    for _ in range(n):
        gens.append(batch_oracle.step(gens[-1][None], rule, boundary)[0])
    return gens


def test_fingerprint_at_sums_to_the_fingerprint():
    g = random_grid(160, 37, 3, 0.4)
    want = cycle_oracle.fingerprint(g)
    parts = [(0, 0, 64, 10), (64, 0, 96, 10), (0, 10, 160, 27)]  # word-aligned windows that tile the grid
    got = sum(cycle_oracle.fingerprint_at(g[y:y + h, x:x + w], y, x // 32) for x, y, w, h in parts) % 2**64
    assert got == want
    assert cycle_oracle.fingerprint_at(g, 0, 0) == want
    # Far from the origin: the share of a window is the fingerprint of the grid that holds only it.
    big = np.zeros((700, 32 * 70), np.uint8)
    big[650:687, 32 * 60:32 * 65] = g
    assert cycle_oracle.fingerprint_at(g, 650, 60) == cycle_oracle.fingerprint(big)


@pytest.mark.parametrize("rule,boundary", [("B3/S23", "torus"), ("B3/S23", "dead"), ("highlife", "torus")])
def test_sparse_expectations_equal_whole_grid(rule, boundary):
    far = fo.small_rows(W, H)
    isles = fo.islands(far, boundary)
    fo.check_plan(isles, far, N, boundary)
    assert len(isles) == (6 if boundary == "torus" else 7)
    assert [a.mode for a in isles[:4]] == ["copy", "or", "copy", "or"]
    sp = fo.Sparse(isles, far, N, rule, boundary)
    g0 = np.zeros((H, W), np.uint8)
    for a in isles:
        for gx, gy, w, h, ox, oy in fo.pieces(a.rect, far, boundary):
            g0[gy:gy + h, gx:gx + w] |= a.soup[oy:oy + h, ox:ox + w]
    if boundary == "torus":  # the corner island wraps both ways
        assert g0[:20, :24].any() and g0[H - 20:, W - 24:].any() and g0[:20, W - 24:].any() and g0[H - 20:, :24].any()
    gens = whole_grid_gens(g0, N, rule, boundary)
    pop, fps = sp.population(), sp.fingerprints()
    by, bx = fo.density_block(far)
    for t in (0, 1, N - 1, N):
        assert (sp.grid(t) == gens[t]).all(), t                                   # windows
        assert pop[t] == gens[t].sum()                                              # alive count
        assert (sp.density(t, by, bx) == density_oracle(gens[t], by, bx)).all()     # density map
        assert (sp.density(t, 7, 33) == density_oracle(gens[t], 7, 33)).all()
    assert pop.tolist() == [int(g.sum()) for g in gens]                             # census series
    assert fps.tolist() == [cycle_oracle.fingerprint(g) for g in gens]              # fingerprint series
    assert len(set(fps.tolist())) == N + 1 and pop[N] > 0


CASES = [dict(), dict(boundary="dead"), dict(census=True), dict(fingerprint=True), dict(rule="highlife"),
         dict(boundary="dead", census=True)]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "torus")
@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_island_and_soup_procedures_on_the_cpu_engine(native, tune, layout, kw):
    far = fo.small_rows(W, H)
    rule, boundary = kw.get("rule", "B3/S23"), kw.get("boundary", "torus")
    sim = Simulation(LifeConfig(W, H, gen_limit=10**6, layout=layout, tmax=4, tune=tune, **kw), engine="cpu")
    flags = dict(census=kw.get("census", False), fingerprint=kw.get("fingerprint", False))
    sp = fo.run_islands(sim, far, N, rule, boundary, **flags)
    assert (sim.tile() == sp.grid(N)).all()
    c0, c = fo.run_soup(sim, far, N, rule, boundary, **flags)
    assert 0 < c < c0
    # The soup procedure's windows are cut from this whole-grid evolution.
    g = random_grid(W, H, 5, 0.4)
    assert c0 == g.sum()
    assert (sim.tile() == whole_grid_gens(g, N, rule, boundary)[N]).all()


def test_procedures_on_a_drifting_ring(native, tune):
    """The CPU backend emulating the adder window's drifting frame on a row ring: every view rotates first."""
    far = fo.small_rows(W, H)
    sim = Simulation(LifeConfig(W, H, gen_limit=10**6, layout="bits", tmax=4,
                                tune=dict(tune, cpu_drift="1", cpu_ring="1")), engine="cpu")
    d = sim.describe()
    assert d["drifting"] and d["row_ring"]
    fo.run_islands(sim, far, N)
    fo.run_soup(sim, far, N)


@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_cycle_confirmation_procedure_on_the_cpu_engine(native, tune, layout):
    sim = Simulation(LifeConfig(W, H, gen_limit=10**6, layout=layout, fingerprint=True, check_similarity=False,
                                tune=dict(tune, cycle_match_bits="0")), engine="cpu")
    fo.run_cycle_confirmation(sim, fo.small_rows(W, H))


def test_a_wrong_cell_is_seen(native, tune):
    """One stray cell anywhere in the grid fails the island procedure (the density map sees it)."""
    far = fo.small_rows(W, H)

    class Stray(Simulation):
        def advance(self, n):
            rep = super().advance(n)
            self.place(np.ones((1, 1), np.uint8), 1700, 250, mode="or")
            return rep

    sim = Stray(LifeConfig(W, H, gen_limit=10**6, layout="bits", tmax=4, tune=tune), engine="cpu")
    with pytest.raises(AssertionError):
        fo.run_islands(sim, far, N)


@pytest.mark.parametrize("seed", SOUP_SEEDS)
def test_rng_density_at_2_26_cells(native, seed):
    """random_grid stays inside the bound the GPU tests hold init_random's count to: the bound tests the
    kernel, not the hash.  And far_oracle's RNG is the package's."""
    g = random_grid(8192, 8192, seed, 0.4)
    mean, six_sigma = fo.count_bound(0.4, 2**26)
    assert abs(int(g.sum()) - mean) <= six_sigma, (int(g.sum()), mean, six_sigma)
    far = fo.Far(8192, 8192, 0, 0)
    for rect in [(0, 0, 70, 9), (8100, 8000, 92, 192), (-30, -5, 60, 10)]:
        x0, y0, w, h = rect
        want = g[np.ix_(np.arange(y0, y0 + h) % 8192, np.arange(x0, x0 + w) % 8192)]
        assert (fo.rng_rect(seed, 0.4, rect, far) == want).all(), rect


def test_far_heights(native):
    hb, hu = fo.far_height(native, "bits"), fo.far_height(native, "u8")
    assert (hb, hu) == (533504, 67584)  # 2^32 + 2^26 bytes at pitches of 8192 and 65536, and 1024 rows
    assert hb * fo.FAR_W > 8 * 2**32 and hu * fo.FAR_W > 2**32  # cells: past 2^32 words' worth, past 2^32
    assert 0.4 * hb * fo.FAR_W - fo.count_bound(0.4, hb * fo.FAR_W)[1] > 2**32  # a 0.4 soup: more than 2^32 live cells


@pytest.mark.parametrize("layout,Wt,Ht,Dv,hw", [
    ("u8", 1048576, 131072, 32, 0),     # 1,048,576^2 bytes on 8 GPUs, row strips: 128 GiB a buffer
    ("u8", 1048576, 131072, 512, 16),   # ... with a deep halo
    ("u8", 524288, 262144, 512, 16),    # ... as 2 x 4 blocks
    ("bits", 1048576, 131072, 256, 0),  # the same tile on bit words
    ("bits", 1048576, 1048576, 192, 12),  # a whole 1,048,576^2 bit grid on one GPU (128 GiB)
    ("bits", 65536, 65536, 256, 0)])
def test_largest_tile_geometry(native, layout, Wt, Ht, Dv, hw):
    lay = native.Layout.Bits if layout == "bits" else native.Layout.U8
    g = native.TileGeom.make(lay, Ht, Wt, Dv, hw)
    wc = Wt + 64 * hw
    wp = -(-wc // 32)
    pitch = -(-(wp * (4 if layout == "bits" else 32)) // 256) * 256
    assert (g.H, g.W, g.Dv, g.hw) == (Ht, Wt, Dv, hw)
    assert (g.Wc(), g.Wp(), g.R(), g.pitch) == (wc, wp, Ht + 2 * Dv, pitch)
    assert g.bytes() == (Ht + 2 * Dv) * pitch
    assert pitch < 2**30 and wp < 2**30 and g.R() < 2**30  # what the block kernels keep in 32 bits
    if Ht * Wt >= 2**37:
        assert g.bytes() > 2**32


def test_largest_decompositions(native):
    n = 1048576
    d = native.Decomposition.make(n, n, 8, "auto", 32)
    assert (d.Px, d.Py, d.nranks()) == (1, 8, 8)
    for r in range(8):
        assert (d.rows(r).begin, d.rows(r).end) == (r * n // 8, (r + 1) * n // 8)
        assert (d.cols(r).begin, d.cols(r).end) == (0, n)
    d = native.Decomposition.make(n, n + 3, 8, "2x4", 32)
    assert (d.Px, d.Py) == (2, 4)
    base, rem = divmod(n + 3, 4)
    for r in range(8):
        py, px = divmod(r, 2)
        b = py * base + min(py, rem)
        assert (d.rows(r).begin, d.rows(r).end) == (b, b + base + (1 if py < rem else 0))
        assert (d.cols(r).begin, d.cols(r).end) == (px * n // 2, (px + 1) * n // 2)
        assert d.rows(r).size() * d.cols(r).size() > 2**36
    # The rows of all tiles are the grid's, once.
    assert sum(d.rows(2 * py).size() for py in range(4)) == n + 3
    # 65536^2 bit-packed on 8 GPUs.
    d = native.Decomposition.make(65536, 65536, 8, "auto", 32)
    assert [d.rows(r).size() for r in range(8)] == [8192] * 8
