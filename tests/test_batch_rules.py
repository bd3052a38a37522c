"""A rule per universe (simulate_batch(rules=..., soups=...)), CPU tier: the
cpu engine and both CLIs against a per-universe-rule NumPy oracle, which is
itself checked against tests/batch_oracle.py first."""
from __future__ import annotations

import csv
import json
import re

import numpy as np
import pytest

import batch_oracle as bo
import gol_amd
from gol_amd import life_like_rules, parse_rule, simulate_batch
from test_batch import GOLDEN, check, run_cli

ENGINE = "cpu"


# ---- the oracle: batch_oracle.step / run with a rule per universe ---------------

def masks(rules):
    """(birth, survive) masks of the rules (bit n: at n live neighbours), from the text alone."""
    b = np.zeros(len(rules), np.int64)
    s = np.zeros(len(rules), np.int64)
    for i, rule in enumerate(rules):
        birth, survive = bo.parse_rule(rule)
        b[i] = sum(1 << n for n in birth)
        s[i] = sum(1 << n for n in survive)
    return b, s


def step_rules(g, bmask, smask, boundary="torus"):
    """One generation of g (B, H, W), universe u under (bmask[u], smask[u])."""
    g = g.astype(np.uint8)
    if boundary == "torus":
        n = sum(np.roll(np.roll(g, dy, 1), dx, 2) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    else:
        H, W = g.shape[1:]
        p = np.pad(g, ((0, 0), (1, 1), (1, 1)))
        n = sum(p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if (dy, dx) != (0, 0))
    born = (bmask[:, None, None] >> n) & 1 & (g == 0)
    stay = (smask[:, None, None] >> n) & 1 & (g == 1)
    return (born | stay).astype(np.uint8)


def run_rules(grids, bmask, smask, max_gens, max_period=64, boundary="torus"):
    """batch_oracle.run with a rule per universe."""
    g = np.array(grids, dtype=np.uint8)
    B = g.shape[0]
    gens = np.full(B, max_gens, dtype=np.int32)
    period = np.zeros(B, dtype=np.int32)
    active = np.ones(B, dtype=bool)
    snap, s = g.copy(), 0
    for t in range(1, max_gens + 1):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        g[idx] = step_rules(g[idx], bmask[idx], smask[idx], boundary)
        same = (g[idx] == snap[idx]).all(axis=(1, 2))
        stopped = idx[same]
        gens[stopped] = t
        period[stopped] = t - s
        active[stopped] = False
        if t - s == max_period:
            snap, s = g.copy(), t
    pop = g.sum(axis=(1, 2)).astype(np.int32)
    stop = np.where(period == 0, bo.LIMIT, np.where(pop == 0, bo.EXTINCTION, bo.CYCLE)).astype(np.uint8)
    return gens, period, stop, pop, g


def oracle_cross(rules, soups, max_gens, max_period=64, boundary="torus"):
    """The cross product: universe r*K + j is rule r on soups[j]."""
    K = len(soups)
    b, s = masks(rules)
    return run_rules(np.tile(soups, (len(rules), 1, 1)), np.repeat(b, K), np.repeat(s, K), max_gens, max_period,
                     boundary)


def all_masks():
    i = np.arange(131072, dtype=np.int64)
    return (i & 0xFF) << 1, i >> 8


# The rules of the per-shape tests: the compiled ones and rules that between
# them set and clear every one of B1..B8 and S0..S8.
RULES23 = ["B3/S23", "B36/S23", "B3678/S34678", "B2/S", "B1357/S1357", "B3/S012345678", "B34/S34",
           "B/S", "B12345678/S012345678", "B1/S", "B8/S", "B/S8", "B/S0", "B1/S1", "B2/S0", "B3/S1234",
           "B35678/S5678", "B368/S245", "B4678/S35678", "B1357/S02468", "B45678/S2345", "B2345678/S", "B/S01234567"]


def test_the_rule_list_sets_and_clears_every_digit():
    assert len(RULES23) == 23 == len(set(RULES23)) and RULES23[:7] == list(bo.RULES.values())
    b, s = masks(RULES23)
    for n in range(1, 9):
        assert ((b >> n) & 1).any() and not ((b >> n) & 1).all(), n
    for n in range(9):
        assert ((s >> n) & 1).any() and not ((s >> n) & 1).all(), n
    assert not (b & 1).any()


@pytest.mark.parametrize("boundary", ["torus", "dead"])
def test_the_oracle_is_batch_oracle_with_one_rule(boundary):
    soups = bo.random_soups(32, 16, 5, 0.4, 4)
    for rule in ("B3/S23", "B36/S23", "B35/S236", "B1357/S02468", "B2/S"):
        b, s = masks([rule] * 4)
        assert np.array_equal(step_rules(soups, b, s, boundary), bo.step(soups, rule, boundary))
        want = bo.run(soups, 120, 16, rule, boundary)
        got = run_rules(soups, b, s, 120, 16, boundary)
        for x, y in zip(got, want):
            assert np.array_equal(x, y), rule


# ---- life_like_rules -------------------------------------------------------------

def test_life_like_rules():
    rules = life_like_rules()
    assert len(rules) == 131072 == len(set(rules))
    assert rules[0] == "B/S" and rules[1] == "B1/S" and rules[256] == "B/S0" and rules[(0b1100 << 8) | 0b100] == "B3/S23"
    b, s = masks(rules)
    wb, ws = all_masks()
    assert np.array_equal(b, wb) and np.array_equal(s, ws)  # the documented index formula
    assert not (b & 1).any()  # no B0
    for i in list(range(0, 131072, 997)) + [131071]:
        assert parse_rule(rules[i]) == rules[i]
    assert all(re.fullmatch(r"B[1-8]*/S[0-8]*", r) for r in rules)
    assert gol_amd.life_like_rules is life_like_rules


# ---- the two forms on the cpu engine -------------------------------------------------

@pytest.mark.parametrize("boundary", ["torus", "dead"])
@pytest.mark.parametrize("W,H", [(32, 8), (64, 16), (64, 64)])
def test_cross_product(W, H, boundary):
    K = 3
    soups = bo.random_soups(W, H, 1, 0.4, K)
    want = oracle_cross(RULES23, soups, 100, 16, boundary)
    assert len(set(want[2].tolist())) == 3 or (W, H) == (64, 64)  # every stop reason among the 69
    drawn = simulate_batch(shape=(W, H), random=(1, 0.4), rules=RULES23, soups=K, max_gens=100, max_period=16,
                           boundary=boundary, engine=ENGINE, return_grids=True)
    check(drawn, want)
    assert drawn.rules == RULES23 and drawn.soups == K
    assert "rule table" in drawn.variant and "23 rules x 3" in drawn.variant
    given = simulate_batch(soups, rules=RULES23, soups=K, max_gens=100, max_period=16, boundary=boundary,
                           engine=ENGINE, return_grids=True)
    check(given, want)
    explicit = simulate_batch(batch=69, shape=(W, H), random=(1, 0.4), rules=RULES23, soups=K, max_gens=100,
                              max_period=16, boundary=boundary, engine=ENGINE)
    check(explicit, want)
    # each rule's slice is the one-rule batch on the same soups
    for r in (0, 3, 12, 22):
        one = simulate_batch(batch=K, shape=(W, H), random=(1, 0.4), rule=RULES23[r], max_gens=100, max_period=16,
                             boundary=boundary, engine=ENGINE, return_grids=True)
        sl = slice(r * K, r * K + K)
        check(one, tuple(a[sl] for a in want), RULES23[r])


def test_pairing():
    """rules alone: universe b runs rule b on grid b (or on the soup of seed + b)."""
    W, H, B = 32, 8, 9
    rules = RULES23[2:2 + B]
    soups = bo.random_soups(W, H, 11, 0.45, B)
    b, s = masks(rules)
    want = run_rules(soups, b, s, 80, 8)
    res = simulate_batch(soups, rules=rules, max_gens=80, max_period=8, engine=ENGINE, return_grids=True)
    check(res, want)
    assert res.soups is None and res.rules == rules and "9 rules x 1" in res.variant
    drawn = simulate_batch(batch=B, shape=(W, H), random=(11, 0.45), rules=rules, max_gens=80, max_period=8,
                           engine=ENGINE, return_grids=True)
    check(drawn, want)
    for i in (0, 4, 8):
        one = simulate_batch(soups[i:i + 1], rule=rules[i], max_gens=80, max_period=8, engine=ENGINE, return_grids=True)
        check(one, tuple(a[i:i + 1] for a in want))
    # names and loose notation go through parse_rule
    named = simulate_batch(soups[:2], rules=["HighLife", "b3s23"], max_gens=5, engine=ENGINE)
    assert named.rules == ["B36/S23", "B3/S23"]


def test_soups_one_shares_one_soup():
    """soups=1 is the cross product with K = 1: every rule on the same soup."""
    g = bo.random_soups(32, 16, 29, 0.5, 1)
    rules = RULES23[:5]
    res = simulate_batch(g, rules=rules, soups=1, max_gens=1, max_period=1, engine=ENGINE, return_grids=True)
    for i, rule in enumerate(rules):
        assert np.array_equal(res.grids[i], bo.step(g, rule)[0])


def test_every_rule_for_some_generations():
    """All 131,072 rules on one soup, 8 generations, against the oracle."""
    rules = life_like_rules()
    g = bo.random_soups(32, 8, 1, 0.5, 1)
    b, s = all_masks()
    want = run_rules(np.tile(g, (len(rules), 1, 1)), b, s, 8, 4)
    res = simulate_batch(g, rules=rules, soups=1, max_gens=8, max_period=4, engine=ENGINE, return_grids=True)
    check(res, want)
    assert len(set(want[2].tolist())) == 3


def test_per_rule():
    K = 4
    res = simulate_batch(shape=(32, 16), random=(1, 0.4), rules=RULES23, soups=K, max_gens=150, max_period=16,
                         engine=ENGINE)
    per = res.per_rule()
    R = len(RULES23)
    assert per["counts"].shape == (R, 3) and per["counts"].dtype == np.int64
    assert (per["counts"].sum(axis=1) == K).all()
    assert dict(zip(gol_amd.BATCH_STOP, per["counts"].sum(axis=0).tolist())) == res.counts()
    assert per["mean_generations"].dtype == np.float64 and per["mean_population"].dtype == np.float64
    assert per["max_generations"].dtype == np.int32 and per["max_period"].dtype == np.int32
    for r in range(R):
        sl = slice(r * K, r * K + K)
        assert per["mean_generations"][r] == res.generations[sl].sum() / K
        assert per["mean_population"][r] == res.population[sl].sum() / K
        assert per["max_generations"][r] == res.generations[sl].max() and per["max_period"][r] == res.period[sl].max()
        assert per["counts"][r].tolist() == [int((res.stop[sl] == c).sum()) for c in range(3)]
    assert per["counts"][RULES23.index("B/S")].tolist() == [0, 0, K]  # everything dies at once
    paired = simulate_batch(batch=3, shape=(32, 16), random=(1, 0.4), rules=RULES23[:3], max_gens=20, engine=ENGINE)
    assert paired.per_rule()["counts"].sum(axis=1).tolist() == [1, 1, 1]
    plain = simulate_batch(batch=3, shape=(32, 16), random=(1, 0.4), max_gens=20, engine=ENGINE)
    assert plain.rules is None and plain.soups is None
    with pytest.raises(ValueError, match="rules="):
        plain.per_rule()


# ---- refusals ------------------------------------------------------------------------

def test_refusals():
    base = dict(shape=(32, 16), random=(1, 0.5), max_gens=10, max_period=4, engine=ENGINE)
    with pytest.raises(RuntimeError, match=r"rule 2 of the list.*B0"):
        simulate_batch(rules=["B3/S23", "B2/S", "B03/S23"], **base)
    with pytest.raises(RuntimeError, match=r"rule 1 of the list"):
        simulate_batch(rules=["B3/S23", "B39/S23"], soups=2, **base)
    with pytest.raises(ValueError, match="rule=.* or rules="):
        simulate_batch(rules=["B3/S23"], rule="seeds", **base)
    with pytest.raises(ValueError, match="batch=2, got batch=3"):
        simulate_batch(rules=["B3/S23", "B2/S"], batch=3, **base)
    with pytest.raises(ValueError, match="batch=6, got batch=2"):
        simulate_batch(rules=["B3/S23", "B2/S"], soups=3, batch=2, **base)
    g = np.zeros((3, 8, 32), np.uint8)
    with pytest.raises(ValueError, match=r"grids \(2, H, W\), got 3"):
        simulate_batch(g, rules=["B3/S23", "B2/S"], engine=ENGINE)
    with pytest.raises(ValueError, match=r"grids \(4, H, W\), got 3"):
        simulate_batch(g, rules=["B3/S23", "B2/S"], soups=4, engine=ENGINE)
    with pytest.raises(ValueError, match="soups=0"):
        simulate_batch(rules=["B3/S23"], soups=0, **base)
    with pytest.raises(ValueError, match="goes with rules"):
        simulate_batch(batch=2, soups=2, **base)
    with pytest.raises(ValueError, match="empty"):
        simulate_batch(rules=[], **base)
    with pytest.raises(RuntimeError, match="2\\^24 = 16777216"):
        simulate_batch(rules=life_like_rules(), soups=129, **base)
    # the native layer's own checks (BatchConfig::rules given directly)
    C = gol_amd.native()
    kw = dict(W=32, H=16, seed=1, density=0.5, max_gens=4, max_period=2, engine="cpu")
    with pytest.raises(RuntimeError, match="3 universes, but 2 rules x 2 soups = 4"):
        C.simulate_batch(None, batch=3, rules=["B3/S23", "B2/S"], soups=2, share_soups=True, **kw)
    with pytest.raises(RuntimeError, match="0 soups per rule"):
        C.simulate_batch(None, batch=2, rules=["B3/S23", "B2/S"], soups=0, share_soups=True, **kw)


# ---- the CLIs ---------------------------------------------------------------------------

RULES_FILE = """# a sweep of five
B3/S23
highlife   # by name

  B35/S236
b2s
B1357/S02468
"""
FILE_RULES = ["B3/S23", "B36/S23", "B35/S236", "B2/S", "B1357/S02468"]


def rules_csv_lines(rules, K, res):
    gens, period, stop, pop = (np.asarray(a).reshape(len(rules), K) for a in res[:4])
    out = [["rule", "soups", "limit", "cycle", "extinction", "mean_generations", "max_generations", "max_period",
            "mean_population"]]
    for r, rule in enumerate(rules):
        out.append([rule, str(K)] + [str(int((stop[r] == c).sum())) for c in range(3)] +
                   [f"{gens[r].sum() / K:.6f}", str(gens[r].max()), str(period[r].max()), f"{pop[r].sum() / K:.6f}"])
    return out


def check_cli_files(rules, K, seed, want, out, per, shared=True):
    rows = list(csv.reader(out.read_text().splitlines()))
    assert rows[0] == ["universe", "seed", "rule", "generations", "stop", "period", "population"]
    assert rows[1:] == [[str(u), str(seed + (u % K if shared else u)), rules[u // K], str(want[0][u]),
                         bo.STOP_NAMES[want[2][u]], str(want[1][u]), str(want[3][u])] for u in range(len(rules) * K)]
    assert list(csv.reader(per.read_text().splitlines())) == rules_csv_lines(rules, K, want)


@pytest.mark.parametrize("which", ["gol", "python"])
def test_cli_batch_rules(which, native, tmp_path):
    (tmp_path / "rules.txt").write_text(RULES_FILE)
    K, W, H = 4, 32, 16
    want = oracle_cross(FILE_RULES, bo.random_soups(W, H, 7, 0.4, K), 200, 16)
    c = bo.counts(want[2])
    out, per, metrics = tmp_path / "b.csv", tmp_path / "r.csv", tmp_path / "m.json"
    r = run_cli(which, [W, H, "none", "--batch-rules", "rules.txt", "--soups", K, "--random", "7:0.4", "--gens", 200,
                        "--max-period", 16, "--engine", ENGINE, "--batch-csv", out, "--rules-csv", per,
                        "--metrics-json", metrics], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == (f"Batch: 20 universes: {c['limit']} limit, {c['cycle']} cycle, {c['extinction']} extinction; "
                        f"largest generations {want[0].max()}\nRules: 5 rules x 4 soups\n")
    check_cli_files(FILE_RULES, K, 7, want, out, per)
    rec = json.loads(metrics.read_text())
    assert rec["batch"] == 20 and rec["batch_rules"] == 5 and rec["batch_soups"] == 4
    assert "rule table 5 rules x 4" in rec["batch_variant"]
    # an explicit --batch that agrees; without --soups rule b runs on seed SEED + b
    r = run_cli(which, [W, H, "none", "--batch", 5, "--batch-rules", "rules.txt", "--random", "7:0.4", "--gens", 200,
                        "--max-period", 16, "--engine", ENGINE, "--batch-csv", out, "--rules-csv", per], tmp_path)
    assert r.returncode == 0, r.stderr
    b, s = masks(FILE_RULES)
    paired = run_rules(bo.random_soups(W, H, 7, 0.4, 5), b, s, 200, 16)
    assert r.stdout.endswith("Rules: 5 rules x 1 soups\n") and r.stdout.startswith("Batch: 5 universes: ")
    check_cli_files(FILE_RULES, 1, 7, paired, out, per, shared=False)


def test_the_clis_write_the_same_bytes(native, tmp_path):
    (tmp_path / "rules.txt").write_text(RULES_FILE)
    got = {}
    for which in ("gol", "python"):
        out, per = tmp_path / f"b_{which}.csv", tmp_path / f"r_{which}.csv"
        r = run_cli(which, [64, 8, "none", "--batch-rules", "rules.txt", "--soups", 3, "--random", "3:0.35", "--gens",
                            90, "--boundary", "dead", "--engine", ENGINE, "--batch-csv", out, "--rules-csv", per],
                    tmp_path)
        assert r.returncode == 0, r.stderr
        got[which] = (r.stdout, out.read_bytes(), per.read_bytes())
    assert got["gol"] == got["python"]


@pytest.mark.parametrize("which", ["gol", "python"])
def test_cli_batch_rules_refusals(which, native, tmp_path):
    (tmp_path / "rules.txt").write_text(RULES_FILE)
    (tmp_path / "bad.txt").write_text("B3/S23\n# fine\nB3/S29\n")
    (tmp_path / "b0.txt").write_text("B3/S23\nB01/S\n")
    (tmp_path / "none.txt").write_text("# nothing\n\n")
    base = [32, 16, "none", "--random", "1", "--engine", ENGINE]
    for extra, text in ((["--batch-rules", "bad.txt"], "line 3"), (["--batch-rules", "b0.txt"], "line 2"),
                        (["--batch-rules", "none.txt"], "names no rule"),
                        (["--batch-rules", "missing.txt"], "cannot read"),
                        (["--batch-rules", "rules.txt", "--rule", "seeds"], "--batch-rules with --rule"),
                        (["--batch-rules", "rules.txt", "--batch", 6], "5 rules x 1 soups make 5"),
                        (["--batch-rules", "rules.txt", "--soups", 2, "--batch", 5], "5 rules x 2 soups make 10"),
                        (["--batch-rules", "rules.txt", "--soups", 0], "at least 1"),
                        (["--batch", 4, "--soups", 2], "need --batch-rules"),
                        (["--batch", 4, "--rules-csv", "r.csv"], "need --batch-rules"),
                        (["--batch-rules", "rules.txt", "--census", "c.csv"], "--batch with --census")):
        r = run_cli(which, base + extra, tmp_path)
        assert r.returncode != 0 and text in r.stderr, (extra, r.stderr)
    assert "B0" in run_cli(which, base + ["--batch-rules", "b0.txt"], tmp_path).stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["b0.txt", "bad.txt", "none.txt", "rules.txt"]


@pytest.mark.parametrize("which", ["gol", "python"])
def test_cli_without_the_flag_is_unchanged(which, native, tmp_path):
    """The plain run's stdout (the golden recorded before --batch existed) and a
    --batch run's stdout and CSV header: no Rules line, no rule column."""
    r = run_cli(which, [64, 48, "--random", "7:0.4", "--engine", "cpu", "--gens", 120, "--output", "none"], tmp_path)
    assert r.returncode == 0, r.stderr
    got = re.sub(r"(?<=Execution time:\t)[0-9.]+(?= msecs)", "<ms>", r.stdout)
    assert got.encode() == (GOLDEN / f"stdout_{which}.txt").read_bytes()
    out, metrics = tmp_path / "b.csv", tmp_path / "m.json"
    r = run_cli(which, [32, 16, "none", "--batch", 64, "--random", "1:0.4", "--gens", 1024, "--engine", ENGINE,
                        "--batch-csv", out, "--metrics-json", metrics], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "Batch: 64 universes: 1 limit, 61 cycle, 2 extinction; largest generations 1024\n"
    assert out.read_text().splitlines()[0] == "universe,seed,generations,stop,period,population"
    rec = json.loads(metrics.read_text())
    assert "batch_rules" not in rec and "batch_soups" not in rec
