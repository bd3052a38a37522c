#!/usr/bin/env python3
"""Summarise a rocprofv3 --kernel-trace csv: per kernel totals; the skipping kernel's launches in order."""
import collections
import csv
import glob
import sys

d = sys.argv[1]
step_launches = float(sys.argv[2]) if len(sys.argv) > 2 else 1000 / 12.0
paths = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
rows = []
for p in paths:
    rows += list(csv.DictReader(open(p)))
rows = [r for r in rows if not r["Kernel_Name"].startswith(("void at::", "at::"))]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
tot = collections.defaultdict(lambda: [0, 0.0])
for r in rows:
    t = tot[r["Kernel_Name"][:120]]
    t[0] += 1
    t[1] += dur(r)
allt = sum(t[1] for t in tot.values()) or 1
print(f"kernels: {len(rows)} launches, {allt / 1e3:.1f} ms of device time")
for k, (n, s) in sorted(tot.items(), key=lambda kv: -kv[1][1])[:8]:
    print(f" {100 * s / allt:6.2f} %  n={n:7d}  mean {s / n:8.2f} us  {k}")
q = [r for r in rows if "life_quiet_" in r["Kernel_Name"]]
blocks = [r for r in rows if "life_quiet_" in r["Kernel_Name"] or "life_group_kernel" in r["Kernel_Name"]
          or "life_block_kernel" in r["Kernel_Name"]]
print(f"\nskipping kernel: {len(q)} launches")
if q:
    dq = [dur(r) for r in q]
    print(f"  first 3 launches (us): {' '.join(f'{x:.1f}' for x in dq[:3])}")
    big = [x for x in dq if x > 100]
    print(f"  over 100 us: {len(big)}" + (f" (mean {sum(big) / len(big):.1f} us)" if big else ""))
    last = dq[-1000:]
    print(f"  settled: last {len(last)} skipping launches mean {sum(last) / len(last):.2f} us, "
          f"min {min(last):.2f}, median {sorted(last)[len(last) // 2]:.2f}")
    # Timed region: the last 20 steps of step_launches block launches each.
    n20 = int(round(20 * step_launches))
    if len(blocks) >= n20:
        tl = blocks[-n20:]
        print(f"\ntimed region (last {n20} block launches): {sum(dur(r) for r in tl) / 1e3:.2f} ms of kernel time, "
              f"span {(int(tl[-1]['End_Timestamp']) - int(tl[0]['Start_Timestamp'])) / 1e6:.2f} ms")
        print("  step: launches, mean us per launch, ms of kernel time")
        for s in range(20):
            a, b = int(round(s * step_launches)), int(round((s + 1) * step_launches))
            ds = [dur(r) for r in tl[a:b]]
            print(f"  {s + 1:2d}: {len(ds):3d}  {sum(ds) / len(ds):7.2f}  {sum(ds) / 1e3:6.3f}")
