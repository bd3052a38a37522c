#!/usr/bin/env python3
"""Compare two sets of scripts/bench_matrix.py records, a parent tree's and a
change's: for every configuration, whether all runs of both verified and
agree on the final-grid digest, the per-step exchanges, polls, kernel and
linked launches, halo bytes, triggered sends, kernel, T, D and the overlap and
poll modes; and the ms/step of every run, side by side.  Fields that differ
are listed.  Exit status 1 when a configuration differs.  SUMMARY.jsonl, if
given, receives one line per configuration: every run's ms/step of both sets
and the compared fields (the first run's), small enough to commit in place of
the full records.

    python scripts/matrix_compare.py PARENT.jsonl CHANGE.jsonl [SUMMARY.jsonl]
"""
import collections
import json
import sys


def load(path):
    recs = collections.defaultdict(list)
    for line in open(path):
        r = json.loads(line)
        recs[r["name"]].append(r)
    return recs


def key(r):
    c = r["config"]
    return {"verified": r["verified"], "final_sha256": c["verify"]["final_sha256"],
            "exchanges": c["exchanges_per_step"], "polls": c["polls_per_step"],
            "kernel_launches": c["kernel_launches_per_step"], "linked_launches": c["linked_launches_per_step"],
            "halo_bytes": c["halo_bytes_per_step"], "overlap_mode": c["overlap_mode"], "poll_mode": c["poll_mode"],
            "triggered_sends": c["triggered_sends"], "kernel": c["kernel"], "tmax": c["tmax"], "epoch": c["epoch"]}


def main() -> int:
    P, C = load(sys.argv[1]), load(sys.argv[2])
    if list(P) != list(C):
        print("configurations differ:", sorted(set(P) ^ set(C)))
        return 1
    bad = 0
    summary = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
    print(f"{'config':22s} {'parent ms/step':>24s} {'change ms/step':>24s}  same")
    for n in P:
        kp, kc = [key(r) for r in P[n]], [key(r) for r in C[n]]
        same = all(k == kp[0] for k in kp + kc) and all(k["verified"] for k in kp + kc)
        if not same:
            bad += 1
            for f in kp[0]:
                vp, vc = {json.dumps(k[f]) for k in kp}, {json.dumps(k[f]) for k in kc}
                if vp != vc or len(vp) > 1:
                    print("   ", n, f, "parent", sorted(vp), "change", sorted(vc))
        ms = [" ".join(f"{r['ms_per_step']:.3f}" for r in rs) for rs in (P[n], C[n])]
        print(f"{n:22s} {ms[0]:>24s} {ms[1]:>24s}  {same}")
        if summary:
            summary.write(json.dumps({"name": n, "same": same,
                                      "ms_per_step_parent": [round(r["ms_per_step"], 4) for r in P[n]],
                                      "ms_per_step_change": [round(r["ms_per_step"], 4) for r in C[n]], **kp[0]}) + "\n")
    print("configurations that differ:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
