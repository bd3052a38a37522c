#!/usr/bin/env python3
"""Rule sweeps: the rule-table kernel against the compiled one, and all Life-like rules in one launch
(docs/PERFORMANCE.md "Batched universes", "Rule sweeps").

    python scripts/rule_sweep_ab.py table [--out FILE]   # rules=["B3/S23"] x 65536 soups against rule="B3/S23"
    python scripts/rule_sweep_ab.py sweep [--out FILE]   # 131072 rules x 64 soups of 32 x 16 in one launch

`table` reports kernel_ms of 5 warm calls (median) of both kernels on the same soups, alternating them, at
64 x 64 (the rule word is the same in every lane) and at 32 x 8 (eight universes of a wave; the table is per
lane either way), their ratio, and whether all four result fields are equal.  `sweep` reports kernel_ms,
universes/s and the stop counts of the whole sweep, then times what there was before - the cpu engine, one
simulate_batch(rule=r) call per rule on the same 64 soups - on 256 rules, scales that to 131072 rules, and
compares those calls with the sweep's slices: once on every 512th rule (all of them rules without births,
by the index formula) and once on every 513th.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402

import gol_amd  # noqa: E402

FIELDS = ("generations", "period", "stop", "population")


def equal(a, b, sl=slice(None)) -> bool:
    return all(np.array_equal(getattr(a, f)[sl], getattr(b, f)) for f in FIELDS)


def table() -> dict:
    out = {}
    for (W, H), density in (((64, 64), 0.5), ((32, 8), 0.5)):
        common = dict(shape=(W, H), random=(1, density), max_gens=4096, max_period=64, engine="hip")
        calls = {"compiled": dict(rule="B3/S23", batch=65536, **common),
                 "table": dict(rules=["B3/S23"], soups=65536, **common)}
        res = {k: gol_amd.simulate_batch(**kw) for k, kw in calls.items()}  # warm
        ms = {k: [] for k in calls}
        for _ in range(5):
            for k, kw in calls.items():
                res[k] = gol_amd.simulate_batch(**kw)
                ms[k].append(res[k].kernel_ms)
        med = {k: statistics.median(v) for k, v in ms.items()}
        out[f"{W}x{H}"] = dict(variants={k: r.variant for k, r in res.items()}, kernel_ms=ms, median_ms=med,
                               ratio_table_over_compiled=med["table"] / med["compiled"],
                               sum_generations=int(res["table"].generations.astype(np.int64).sum()),
                               counts=res["table"].counts(), equal=equal(res["table"], res["compiled"]))
    return out


def sweep() -> dict:
    rules = gol_amd.life_like_rules()
    K = 64
    common = dict(shape=(32, 16), random=(1, 0.4), max_gens=1024, max_period=64)
    kw = dict(rules=rules, soups=K, engine="hip", **common)
    gol_amd.simulate_batch(**kw)  # warm
    t0 = time.perf_counter()
    r = gol_amd.simulate_batch(**kw)
    wall = time.perf_counter() - t0
    B = len(rules) * K
    gens = int(r.generations.astype(np.int64).sum())
    per = r.per_rule()
    out = dict(variant=r.variant, universes=B, kernel_ms=r.kernel_ms, call_wall_s=wall,
               universes_per_s=B / (r.kernel_ms * 1e-3), sum_generations=gens, counts=r.counts(),
               rules_all_limit=int((per["counts"][:, 0] == K).sum()), rules_all_extinct=int((per["counts"][:, 2] == K).sum()),
               rules_all_cycle=int((per["counts"][:, 1] == K).sum()), largest_period=int(r.period.max()))
    # Every 512th rule is the sample the comparison was asked for, but index i = 512 j has birth mask
    # (i & 0xFF) << 1 = 0: rules without births, which stop within a few generations.  Every 513th rule
    # (birth mask j & 0xFF, survive mask about 2 j) is the representative one.
    gol_amd.simulate_batch(batch=K, rule=rules[513], engine="cpu", **common)  # warm: the host pool
    for stride in (512, 513):
        sample = list(range(0, len(rules), stride))[:256]
        t0 = time.perf_counter()
        calls = [gol_amd.simulate_batch(batch=K, rule=rules[i], engine="cpu", **common) for i in sample]
        cpu_s = time.perf_counter() - t0
        same = all(equal(r, c, slice(i * K, i * K + K)) for i, c in zip(sample, calls))
        cpu_gens = sum(int(c.generations.astype(np.int64).sum()) for c in calls)
        out[f"cpu_engine_per_rule_calls_every_{stride}th"] = dict(
            rules_timed=len(sample), rules_without_births=sum(rules[i].startswith("B/") for i in sample),
            seconds=cpu_s, sum_generations=cpu_gens, scaled_to_131072_rules_s=cpu_s * len(rules) / len(sample),
            scaled="the sample's time times rules / rules_timed, not a run of all rules",
            sample_equals_sweep_slices=bool(same))
        print("every", f"{stride}th rule:", len(sample), "cpu-engine calls equal the sweep's slices:", same,
              file=sys.stderr)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mode", choices=["table", "sweep"])
    ap.add_argument("--out", default=None, help="also write the record to this JSON file")
    a = ap.parse_args()
    rec = table() if a.mode == "table" else sweep()
    print(json.dumps(rec))
    if a.out:
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
