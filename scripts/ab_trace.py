"""Kernel-time sum per U-Net evaluation of two library builds from ONE rocprofv3 kernel trace of scripts/ab_libs.py (both builds in one
process, rounds interleaved: what separates them is not the clock state of two processes):
    rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python3 scripts/ab_libs.py 4096 <libA.so> <libB.so>
    python3 scripts/ab_trace.py OUT/**/t_kernel_trace.csv
The builds are told apart by the number of launches of an evaluation (the launches between two head_kernel launches), so they must differ
in it.  A round of ab_libs.py is 10 evaluations; printed per build: the mean sum of every round, their median, and max - min over the rounds
(the spread), then per kernel instance the median duration x launches per evaluation."""
import csv, statistics, sys
from collections import defaultdict

rows = [r for r in csv.DictReader(open(sys.argv[1])) if "cld::" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
CONV = ("conv_block_kernel", "conv_pair_kernel", "cld::head_kernel", "chain_", "wino1d_")
ends = [i for i, r in enumerate(rows) if "cld::head_kernel" in r["Kernel_Name"]]
evals = []
for a, e in zip(ends[:-1], ends[1:]):
    ev = [r for r in rows[a + 1:e + 1] if any(k in r["Kernel_Name"] for k in CONV)]
    evals.append(ev)
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
sizes = sorted({len(ev) for ev in evals}, key=lambda n: -sum(len(ev) == n for ev in evals))[:2]
# rounds: maximal runs of consecutive evaluations of one build
rounds = defaultdict(list)
cur, acc = None, []
for ev in evals + [[]]:
    n = len(ev)
    if n != cur:
        if cur in sizes and len(acc) >= 5:
            rounds[cur].append(acc)
        cur, acc = n, []
    acc.append(ev)
for n in sorted(sizes, reverse=True):
    rs = rounds[n][1:]          # the first round of a build is its warm-up
    means = [statistics.mean(sum(dur(r) for r in ev) for ev in rd) for rd in rs]
    print(f"{n} launches per evaluation: {len(rs)} rounds, mean kernel-time sum per evaluation of each: {[round(m, 1) for m in means]} us")
    print(f"    median {statistics.median(means):.1f} us, min {min(means):.1f}, max {max(means):.1f}, spread {max(means) - min(means):.1f} us")
    per = defaultdict(list)
    for rd in rs:
        for ev in rd:
            for r in ev:
                per[r["Kernel_Name"]].append(dur(r))
    nev = sum(len(rd) for rd in rs)
    for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        name = k.replace("void cld::", "").replace("cld::", "")
        print(f"    {statistics.median(v):8.1f} us x {len(v) / nev:4.1f}  {name[:110]}")
