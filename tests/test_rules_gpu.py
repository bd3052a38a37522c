"""Life-like rules on the HIP engine (MI355X): every rule kernel compiled from
csrc/kernels/life_rules.def against the PyTorch fp32 oracle on the GPU, in the
classic, grouped, wrapped, folded and row-ring schedules, in both layouts, plus
termination, a closed-form GF(2) identity and what describe() reports."""
import functools

import pytest

from gol_amd import LifeConfig, Simulation, life_step_torch, random_grid, simulate
from gol_amd.parallel import InProcessGroup

from test_rules import LISTED, TERMINATION, gf2_translates, reference_outcome

pytestmark = pytest.mark.gpu

RULES = list(LISTED.values())


@pytest.fixture
def tune():
    """The byte-layout tests here run the byte kernels themselves; the tests of
    the device default (byte grid on bit words) drop the key."""
    return {"u8_via_bits": "0"}


def test_every_listed_rule_is_compiled(gpu):
    """Everything below is parametrised over LISTED: it must be what the
    module was built with, or the cases would test nothing."""
    have = gpu.hip_rules()
    assert have and set(have) == set(RULES) | {"B3/S23"}
    be = gpu.hip_backend(0)
    for rule in RULES:
        assert be.supports_rule(gpu.Layout.Bits, rule) and be.supports_rule(gpu.Layout.U8, rule)


@functools.lru_cache(maxsize=None)
def oracle(W, H, seed, density, gens, rule):
    """Grid and its `gens`-th generation under `rule` (fp32 conv on the GPU),
    computed once per case and shared; callers do not modify either."""
    g = random_grid(W, H, seed, density)
    want = life_step_torch(g, gens, device="cuda", rule=rule)
    g.setflags(write=False)
    want.setflags(write=False)
    return g, want


def run_hip(g, gens, **cfg):
    H, W = g.shape
    sim = Simulation(LifeConfig(W, H, gen_limit=gens, **cfg), engine="hip")
    sim.load(g)
    rep = sim.advance(gens)
    return sim, rep


# ---- 1. every rule x window x T, bit layout -----------------------------------------
@pytest.mark.parametrize("tmax", [1, 8, 12, 16])
@pytest.mark.parametrize("xlane", [0, 3])
@pytest.mark.parametrize("rule", RULES)
def test_rule_kernels_vs_torch(gpu, tune, rule, xlane, tmax):
    """3968 cells = 124 words: two column strips with a tail and a folded last
    strip; 333 rows: several segments with remainders."""
    tune["xlane"] = str(xlane)
    W, H, gens = 3968, 333, 3 * tmax + 1
    g, want = oracle(W, H, 11 + tmax, 0.4, gens, rule)
    sim, _ = run_hip(g, gens, layout="bits", tmax=tmax, rule=rule, tune=tune)
    d = sim.describe()
    assert d["rule"] == rule and d["tmax"] == tmax
    assert sim.native_engine.drifting == (xlane == 3)
    assert (sim.tile() == want).all()


# ---- 2. grouped schedules -----------------------------------------------------------
@pytest.mark.parametrize("tmax", [4, 16])
@pytest.mark.parametrize("group", [0, 4, 8])
@pytest.mark.parametrize("rule", ["B3678/S34678", "B1357/S1357"])
def test_rule_grouped_schedules(gpu, tune, rule, group, tmax):
    tune["group"] = str(group)
    W, H, gens = 6400, 700, 2 * tmax + 3
    g, want = oracle(W, H, tmax, 0.4, gens, rule)
    sim, _ = run_hip(g, gens, layout="bits", tmax=tmax, rule=rule, tune=tune)
    assert (sim.tile() == want).all()


# ---- 3. byte kernels ------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(33, 33), (257, 129), (1999, 301)])
@pytest.mark.parametrize("rule", RULES)
def test_rule_byte_kernels(gpu, tune, rule, W, H):
    g, want = oracle(W, H, W * 7 + H, 0.4, 17, rule)
    sim, _ = run_hip(g, 17, layout="u8", rule=rule, tune=tune)
    assert sim.describe()["u8_compute"] == "bytes" and sim.describe()["tmax"] <= 16
    assert (sim.tile() == want).all()


@pytest.mark.parametrize("tmax", [1, 8, 16])
@pytest.mark.parametrize("xlane", [0, 3])  # the adder request runs the DPP window: no drift
@pytest.mark.parametrize("rule", ["B36/S23", "B2/S"])
def test_rule_byte_kernels_every_t(gpu, tune, rule, xlane, tmax):
    tune["xlane"] = str(xlane)
    W, H, gens = 1999, 301, 2 * tmax + 5
    g, want = oracle(W, H, 5 + tmax, 0.4, gens, rule)
    sim, _ = run_hip(g, gens, layout="u8", tmax=tmax, rule=rule, tune=tune)
    assert (sim.tile() == want).all()


def test_rule_byte_kernels_cap_t_at_16(gpu, tune):
    """A byte tile large enough for the default rule's T = 32 passes."""
    W, H = 32768, 8192
    assert Simulation(LifeConfig(W, H, layout="u8", tune=tune), engine="hip").describe()["tmax"] > 16
    assert Simulation(LifeConfig(W, H, layout="u8", rule="highlife", tune=tune), engine="hip").describe()["tmax"] == 16


# ---- 4. byte layout on bit words, the device default -----------------------------------
@pytest.mark.parametrize("rule", ["B3678/S34678", "B34/S34"])
def test_rule_u8_via_bits(gpu, tune, rule):
    del tune["u8_via_bits"]
    W, H, gens = 2048, 130, 37
    g, want = oracle(W, H, 3, 0.4, gens, rule)
    sim, _ = run_hip(g, gens, layout="u8", rule=rule, tune=tune)
    assert sim.describe()["u8_compute"] == "bits"
    assert (sim.tile() == want).all()


# ---- 5. closed form, no oracle code ------------------------------------------------------
@pytest.mark.parametrize("xlane,tmax", [(0, 16), (3, 12)])
def test_replicator_gf2_identity_hip(gpu, tune, xlane, tmax):
    tune["xlane"] = str(xlane)
    g = random_grid(4096, 128, 11)
    sim, _ = run_hip(g, 32, layout="bits", tmax=tmax, rule="B1357/S1357", tune=tune)
    assert sim.native_engine.drifting == (xlane == 3)
    assert (sim.tile() == gf2_translates(g, 32)).all()


# ---- 6. row ring and subdomains ------------------------------------------------------------
def test_rule_row_ring(gpu, tune):
    W, H, rule = 8192, 4096, "B36/S23"
    g, want = oracle(W, H, 21, 0.4, 45, rule)
    sim, rep = run_hip(g, 45, rule=rule, tune=tune)
    assert sim.describe()["row_ring"] is True
    assert (sim.tile() == want).all()


def test_rule_subdomains_2x2(gpu, tune):
    W, H, gens, rule = 32 * 79 * 2, 700, 40, "B3678/S34678"
    g, want = oracle(W, H, 9, 0.4, gens, rule)
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, decomp="2x2", tmax=8, epoch=16, rule=rule, tune=tune), 4,
                         engine="hip", devices=[0])
    grp.load(g)
    grp.advance(gens)
    assert (grp.gather() == want).all()


# ---- 7. termination ---------------------------------------------------------------------------
@pytest.mark.parametrize("rule,grid,expect", TERMINATION)
def test_rule_termination_hip(gpu, tune, rule, grid, expect):
    g = grid()
    ref, rgens, reason = reference_outcome(g, rule)
    assert reason == expect[0] and expect[1] <= rgens <= expect[2], (reason, rgens)
    for layout in ("bits", "u8"):
        out, rep = simulate(g, 1000, engine="hip", layout=layout, rule=rule, tune=tune)
        assert (rep.generations, rep.stop_reason) == (rgens, reason), layout
        assert (out == ref).all(), layout


# ---- 8. what describe() and the reports say ------------------------------------------------------
def test_rule_runs_are_never_linked(gpu, tune):
    """8192^2 is a tile on which the default rule links its launches; forced
    link=1 / chain=1 are ignored for a rule too."""
    W, H, gens, rule = 8192, 8192, 40, "B36/S23"
    g = random_grid(W, H, 8)
    sim, rep = run_hip(g, gens, tune=tune)
    assert rep.linked_launches > 0, "the default rule no longer links here: the check below shows nothing"
    want = life_step_torch(g, gens, device="cuda", rule=rule)
    for extra in ({}, {"link": "1", "row_ring": "0"}, {"chain": "1"}):
        sim, rep = run_hip(g, gens, rule=rule, tune=dict(tune, **extra))
        d = sim.describe()
        assert d["rule"] == rule and f"rule {rule}" in d["kernel"]
        assert rep.linked_launches == 0, extra
        assert d["launch_paths"]["chained"] == 0 and d["launch_paths"]["linked"] == 0, (extra, d["launch_paths"])
        assert (sim.tile() == want).all(), extra


def test_unlisted_rule_is_refused_with_the_compiled_list(gpu, tune):
    with pytest.raises(RuntimeError) as e:
        Simulation(LifeConfig(256, 256, rule="B37/S23", tune=tune), engine="hip")
    msg = str(e.value)
    assert "B37/S23" in msg and "life_rules.def" in msg
    for rule in RULES:
        assert rule in msg
    # the CPU engine runs it
    g = random_grid(256, 64, 1)
    out, _ = simulate(g, 5, engine="cpu", check_similarity=False, rule="B37/S23")
    assert (out == life_step_torch(g, 5, rule="B37/S23")).all()


@pytest.mark.parametrize("W", [200, 256])
def test_lds_byte_kernels_refuse_rules(gpu, tune, W):
    tune["u8_kernel"] = "lds"
    Simulation(LifeConfig(W, 128, layout="u8", tune=tune), engine="hip")  # B3/S23: fine
    with pytest.raises(RuntimeError, match="u8_kernel=lds"):
        Simulation(LifeConfig(W, 128, layout="u8", rule="highlife", tune=tune), engine="hip")
