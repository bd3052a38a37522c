"""Life-like rules (B/S notation) on the CPU tier: the parser, the bit-sliced
table derivation (exhaustive), the CPU backend against the NumPy oracle, a
closed-form GF(2) identity that needs no oracle code, termination semantics
against the serial loop, the CLIs and the checkpoints."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import gol_amd
from gol_amd import LifeConfig, Simulation, life_step, life_step_numpy, random_grid, reference_run, simulate
from gol_amd.ops.life_ops import life_step_torch, life_step_torch_roll, rule_words
from gol_amd.parallel import InProcessGroup
from gol_amd.utils import io
from gol_amd.utils.checkpoint import load_checkpoint, save_checkpoint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The rules compiled for the HIP engine besides B3/S23 (csrc/kernels/life_rules.def).
LISTED = {"highlife": "B36/S23", "daynight": "B3678/S34678", "seeds": "B2/S", "replicator": "B1357/S1357",
          "lwod": "B3/S012345678", "34life": "B34/S34"}


def _random_unlisted(n, seed=20261019):
    """n rules in canonical text, without B0, none of them listed or B3/S23."""
    rng, out = random.Random(seed), []
    while len(out) < n:
        b, s = rng.randrange(0, 512) & ~1, rng.randrange(0, 512)
        text = "B" + "".join(str(k) for k in range(9) if b >> k & 1) + "/S" + "".join(
            str(k) for k in range(9) if s >> k & 1)
        if text not in LISTED.values() and text != "B3/S23" and text not in out:
            out.append(text)
    return out


UNLISTED = _random_unlisted(5)
RULES = list(LISTED.values()) + UNLISTED


# ---- 1. parser ---------------------------------------------------------------
def test_parser_round_trips_names_case_and_slash(native):
    assert gol_amd.parse_rule("B3/S23") == "B3/S23"
    assert gol_amd.parse_rule("b63/s32") == "B36/S23"  # digits come out ascending
    assert gol_amd.parse_rule("B36S23") == "B36/S23"   # the slash is optional
    assert gol_amd.parse_rule("b2s") == "B2/S"
    assert gol_amd.parse_rule("B/S") == "B/S"
    for text in RULES:
        assert gol_amd.parse_rule(text) == text
        assert gol_amd.parse_rule(text.lower().replace("/", "")) == text
    assert gol_amd.RULES["life"] == gol_amd.RULES["conway"] == "B3/S23"
    for name, text in LISTED.items():
        assert gol_amd.RULES[name] == text
        assert gol_amd.parse_rule(name) == gol_amd.parse_rule(name.upper()) == text
    assert set(native.hip_rules()) == set(LISTED.values()) | {"B3/S23"}


@pytest.mark.parametrize("text,why", [("B03/S23", "B0"), ("B0/S", "B0"), ("B39/S23", "8 neighbours"),
                                      ("B3/S239", "8 neighbours"), ("B33/S23", "repeated"),
                                      ("B3/S223", "repeated"), ("", "start"), ("3/23", "start"), ("B3", "S part"),
                                      ("B3/S23x", "unexpected"), ("S23/B3", "start"), ("lifelike", "start"),
                                      ("B3//S23", "S part")])
def test_parser_refusals(native, text, why):
    with pytest.raises(RuntimeError, match=why):
        gol_amd.parse_rule(text)
    with pytest.raises(RuntimeError):
        LifeConfig(64, 64, rule=text).to_native()


def test_b0_is_refused_by_every_entry_point(native):
    g = random_grid(64, 64, 1)
    for call in (lambda: simulate(g, 4, engine="cpu", rule="B03/S23"), lambda: reference_run(g, 4, rule="B03/S23"),
                 lambda: life_step_numpy(g, 1, rule="B0/S")):
        with pytest.raises(RuntimeError, match="B0"):
            call()


# ---- 2. table derivation, exhaustive -------------------------------------------
def test_table_derivation_exhaustive(native):
    """The general host form (rule_host(Rule, ...), the ops and truth tables
    the HIP kernels use) on all 512 neighbourhoods for every rule without B0,
    against the plain definition."""
    rules, bad = native.rule_tables_check()
    assert rules == 131072
    assert bad == 0


@pytest.mark.parametrize("rule", ["B3/S23"] + RULES)
def test_rule_words_general_form(native, rule):
    """rule_words(rule=) on random words against the definition, and for
    B3/S23 against the 7-op fast form."""
    rng = np.random.default_rng(5)
    b, s = (sum(1 << int(d) for d in part) for part in rule[1:].split("/S"))
    for _ in range(20):
        w = [int(x) for x in rng.integers(0, 2**32, 9)]
        got = rule_words(*w, rule=rule)
        want = 0
        for j in range(32):
            def cell(r, dx):
                x = j + dx
                if x < 0:
                    return w[3 * r] >> 31 & 1
                if x > 31:
                    return w[3 * r + 2] & 1
                return w[3 * r + 1] >> x & 1
            ctr = cell(1, 0)
            n = sum(cell(r, dx) for r in range(3) for dx in (-1, 0, 1)) - ctr
            want |= ((s if ctr else b) >> n & 1) << j
        assert got == want
        if rule == "B3/S23":
            assert got == rule_words(*w)


# ---- 3. CPU backend vs life_step_numpy(rule=) ----------------------------------
# Both layouts wherever the width allows the bit layout (width % 32 == 0).
SHAPES = [(64, 5, "bits"), (64, 5, "u8"), (96, 70, "bits"), (96, 70, "u8"), (33, 33, "u8"), (257, 129, "u8")]


@pytest.mark.parametrize("W,H,layout", SHAPES)
@pytest.mark.parametrize("rule", RULES)
def test_cpu_backend_vs_numpy(native, rule, W, H, layout):
    g = random_grid(W, H, W + 3 * H, 0.4)
    want = {}
    for tmax in (1, 8, 16):
        gens = 2 * tmax + 3
        if gens not in want:
            want[gens] = life_step_numpy(g, gens, rule=rule)
        for drift in ("0", "1"):
            sim = Simulation(LifeConfig(W, H, gen_limit=gens, layout=layout, tmax=tmax, rule=rule,
                                        tune={"cpu_drift": drift}), engine="cpu")
            sim.load(g)
            sim.advance(gens)
            assert sim.describe()["rule"] == rule
            assert (sim.tile() == want[gens]).all(), (tmax, drift)


def test_oracles_agree_with_each_other(native):
    g = random_grid(70, 41, 9, 0.4)
    for rule in RULES:
        want = life_step_numpy(g, 6, rule=rule)
        assert (life_step_torch(g, 6, rule=rule) == want).all()
        assert (life_step_torch_roll(g, 6, rule=rule) == want).all()
        ref, gens, _ = reference_run(g, 6, check_similarity=False, rule=rule)
        if gens == 6:  # the serial loop stops early on an empty grid
            assert (ref == want).all()
        assert (life_step(g, 6, engine="cpu", rule=rule) == want).all()


@pytest.mark.parametrize("rule", ["B3678/S34678", "B1357/S1357"])
@pytest.mark.parametrize("spec,P,W,H,layout", [("2x2", 4, 128, 70, "bits"), ("1x3", 3, 96, 70, "u8")])
def test_cpu_decompositions(native, tune, rule, spec, P, W, H, layout):
    g = random_grid(W, H, 77, 0.4)
    gens = 35
    grp = InProcessGroup(LifeConfig(W, H, gen_limit=gens, decomp=spec, layout=layout, tmax=8, rule=rule, tune=tune),
                         P, engine="cpu")
    grp.load(g)
    grp.advance(gens)
    assert (grp.gather() == life_step_numpy(g, gens, rule=rule)).all()


# ---- 4. closed form, no oracle code ---------------------------------------------
def gf2_translates(g, k):
    """XOR of the eight translates of g by (0 or +-k, 0 or +-k), (0, 0) excluded."""
    out = np.zeros_like(g)
    for dy in (-k, 0, k):
        for dx in (-k, 0, k):
            if (dy, dx) != (0, 0):
                out ^= np.roll(np.roll(g, dy, 0), dx, 1)
    return out


def test_replicator_gf2_identity_cpu(native):
    """B1357/S1357 is the XOR of the eight neighbours: linear over GF(2), so
    2^k generations are the XOR of the eight translates by 2^k cells."""
    g = random_grid(128, 96, 11)
    got = life_step(g, 32, engine="cpu", tmax=16, rule="B1357/S1357")
    assert (got == gf2_translates(g, 32)).all()


# ---- 5. termination semantics ----------------------------------------------------
def reference_outcome(g, rule, limit=1000):
    """(grid, generations, stop reason) of the serial loop: the reason is read
    off what the loop returned, not assumed."""
    ref, gens, _ = reference_run(g, limit, rule=rule)
    if gens < limit:
        reason = "extinction" if not ref.any() else "similarity"
    else:
        reason = "fixed_point" if (life_step_numpy(ref, 1, rule=rule) == ref).all() else "limit"
    return ref, gens, reason


def single_cell():
    g = np.zeros((64, 64), dtype=np.uint8)
    g[20, 30] = 1
    return g


# (rule, grid, what the reference itself must show for the case to mean anything)
TERMINATION = [("B2/S", single_cell, ("extinction", 1, 1)),
               ("B3/S012345678", lambda: random_grid(64, 64, 1, 0.1), ("similarity", 5, 200)),
               ("B3/S012345678", lambda: random_grid(64, 64, 2, 0.1), ("similarity", 5, 200)),
               ("B36/S23", lambda: random_grid(64, 64, 2, 0.1), ("limit", 1000, 1000)),
               ("B36/S23", lambda: random_grid(64, 64, 4, 0.1), ("limit", 1000, 1000)),
               ("B36/S23", lambda: random_grid(64, 64, 1, 0.1), ("similarity", 100, 300))]


@pytest.mark.parametrize("rule,grid,expect", TERMINATION)
def test_termination_vs_reference(native, rule, grid, expect):
    g = grid()
    ref, rgens, reason = reference_outcome(g, rule)
    assert reason == expect[0] and expect[1] <= rgens <= expect[2], (reason, rgens)
    for layout, tmax, poll in (("bits", 0, 0), ("u8", 4, 7), ("bits", 16, 1000)):
        out, rep = simulate(g, 1000, engine="cpu", layout=layout, tmax=tmax, poll_gens=poll, rule=rule)
        assert (rep.generations, rep.stop_reason) == (rgens, reason), (layout, tmax, poll)
        assert (out == ref).all()


# ---- 6. CLIs and checkpoints -------------------------------------------------------
def _gol(gol_bin, args, cwd, ok=True):
    r = subprocess.run([str(gol_bin), *map(str, args)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _py(args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=REPO, GOL_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-m", "gol_amd", *map(str, args)], cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _gens(stdout):
    return int(next(ln for ln in stdout.splitlines() if ln.startswith("Generations")).split()[-1])


def test_cli_rule_cpu_equals_ref(native, gol_bin, tmp_path):
    g = random_grid(64, 64, 3, 0.3)
    io.write_grid(str(tmp_path / "in.txt"), g)
    want = life_step_numpy(g, 40, rule="B36/S23")
    assert not (want == life_step_numpy(g, 40)).all()  # the rule matters on this input
    outs = {}
    for run, name in ((_gol, "gol"), (_py, "py")):
        for engine in ("cpu", "ref"):
            args = [64, 64, "in.txt", "--rule", "highlife", "--engine", engine, "--gens", 40, "--no-similarity",
                    "--output", f"{name}_{engine}.out"]
            r = run(gol_bin, args, tmp_path) if run is _gol else run(args, tmp_path)
            assert _gens(r.stdout) == 40
            outs[name, engine] = (tmp_path / f"{name}_{engine}.out").read_bytes()
    assert len(set(outs.values())) == 1
    assert (io.read_grid(str(tmp_path / "gol_cpu.out"), 64, 64) == want).all()
    # the --style stdout lines do not change with a rule
    plain = _gol(gol_bin, [64, 64, "in.txt", "--engine", "cpu", "--gens", 40, "--no-similarity", "--output", "none"],
                 tmp_path).stdout
    ruled = _gol(gol_bin, [64, 64, "in.txt", "--engine", "cpu", "--gens", 40, "--no-similarity", "--output", "none",
                           "--rule", "B36/S23"], tmp_path).stdout
    strip = lambda s: [ln.split("\t")[0] for ln in s.splitlines()]  # noqa: E731
    assert strip(plain) == strip(ruled)


def test_cli_help_and_metrics_name_the_rule(native, gol_bin, tmp_path):
    assert "--rule" in _gol(gol_bin, ["--help"], tmp_path).stdout
    assert "--rule" in _py(["--help"], tmp_path).stdout
    for run, name in ((_gol, "gol"), (_py, "py")):
        args = [64, 64, "--random", 5, "--rule", "b3678s34678", "--engine", "cpu", "--gens", 5, "--output", "none",
                "--metrics-json", f"{name}.json"]
        run(gol_bin, args, tmp_path) if run is _gol else run(args, tmp_path)
        assert json.loads((tmp_path / f"{name}.json").read_text())["rule"] == "B3678/S34678"
    bad = _gol(gol_bin, [64, 64, "--random", 5, "--rule", "B03/S23", "--engine", "cpu"], tmp_path, ok=False)
    assert "B0" in bad.stderr
    assert "B0" in _py([64, 64, "--random", 5, "--rule", "B03/S23", "--engine", "cpu"], tmp_path, ok=False).stderr


@pytest.mark.parametrize("front", ["gol", "py"])
def test_checkpoint_carries_the_rule(native, gol_bin, tmp_path, front):
    run = (lambda a, ok=True: _gol(gol_bin, a, tmp_path, ok)) if front == "gol" else (
        lambda a, ok=True: _py(a, tmp_path, ok))
    W, H = 96, 64
    g = random_grid(W, H, 3, 0.3)
    io.write_grid(str(tmp_path / "in.txt"), g)
    ref, rgens, _ = reference_run(g, 50, rule="B36/S23")
    assert rgens == 50 and not (ref == reference_run(g, 50)[0]).all()
    run([W, H, "in.txt", "--engine", "cpu", "--rule", "highlife", "--gens", 20, "--checkpoint-every", 7,
         "--checkpoint-dir", "ck", "--output", "a.out"])
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["generation"] == 14 and meta["rule"] == "B36/S23"
    # the default rule leaves meta.json as it always was
    run([W, H, "in.txt", "--engine", "cpu", "--gens", 20, "--checkpoint-every", 7, "--checkpoint-dir", "ck0",
         "--output", "a0.out"])
    assert "rule" not in json.loads((tmp_path / "ck0" / "meta.json").read_text())
    run([W, H, "in.txt", "--engine", "cpu", "--rule", "life", "--gens", 20, "--checkpoint-every", 7,
         "--checkpoint-dir", "ck1", "--output", "a1.out"])
    assert (tmp_path / "ck1" / "meta.json").read_bytes().replace(b"ck1", b"ck0") == \
        (tmp_path / "ck0" / "meta.json").read_bytes()
    # a resume takes the rule from the checkpoint, with or without the same --rule
    for extra in ([], ["--rule", "B36/S23"]):
        out = run([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--output", "b.out", *extra]).stdout
        assert _gens(out) == rgens
        assert (io.read_grid(str(tmp_path / "b.out"), W, H) == ref).all()
    # ... and refuses another one
    bad = run([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--output", "c.out", "--rule", "B3/S23"],
              ok=False)
    assert "B36/S23" in bad.stderr
    # either front end resumes the other's checkpoint
    other = (lambda a: _py(a, tmp_path)) if front == "gol" else (lambda a: _gol(gol_bin, a, tmp_path))
    out = other([W, H, "--engine", "cpu", "--resume", "ck", "--gens", 50, "--output", "d.out"]).stdout
    assert _gens(out) == rgens
    assert (io.read_grid(str(tmp_path / "d.out"), W, H) == ref).all()


def test_checkpoint_api_carries_the_rule(native, tmp_path):
    g = random_grid(64, 64, 2, 0.1)
    rule = "B3/S012345678"
    ref, rgens, reason = reference_outcome(g, rule)
    assert reason == "similarity"
    sim = Simulation(LifeConfig(64, 64, rule="lwod"), engine="cpu")
    sim.load(g)
    sim.native_engine.run_until(5)
    save_checkpoint(sim, str(tmp_path / "ck"))
    cfg, grid = load_checkpoint(str(tmp_path / "ck"))
    assert cfg.rule == rule and cfg.start_gen == 5
    sim2 = Simulation(cfg, engine="cpu")
    sim2.load_text(str(grid))
    rep = sim2.run()
    assert rep.generations == rgens
    assert (sim2.tile() == ref).all()


# ---- 7. the default is untouched ---------------------------------------------------
def test_default_rule_untouched(native):
    assert LifeConfig(64, 64).to_native().rule == "B3/S23"
    assert native.EngineConfig().rule == "B3/S23"
    g = random_grid(96, 64, 8, 0.3)
    plain_out, plain = simulate(g, 300, engine="cpu")
    for rule in ("B3/S23", "life"):
        out, rep = simulate(g, 300, engine="cpu", rule=rule)
        assert (out == plain_out).all()
        assert (rep.generations, rep.stop_reason) == (plain.generations, plain.stop_reason)
        assert (life_step_numpy(g, 9, rule=rule) == life_step_numpy(g, 9)).all()
        assert (reference_run(g, 300, rule=rule)[0] == reference_run(g, 300)[0]).all()
    sim = Simulation(LifeConfig(64, 64), engine="cpu")
    assert sim.describe()["rule"] == "B3/S23" and "rule" not in sim.describe()["kernel"]
    assert "rule B36/S23" in Simulation(LifeConfig(64, 64, rule="highlife"), engine="cpu").describe()["kernel"]
