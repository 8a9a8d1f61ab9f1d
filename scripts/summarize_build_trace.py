"""Per-dispatch durations of the row build from a rocprofv3 kernel trace
(scripts/profile_build_trace.sh): one table row per k_build_* dispatch of an
ingest step, in launch order, averaged over the last STEPS steps -- a kernel
launched twice per step (k_build_mid, once per mid list) keeps two rows.
Then every kernel of the run by total time.

Usage: summarize_build_trace.py bench_out/ktrace_LABEL [STEPS]   (markdown on stdout)
"""
import collections
import csv
import glob
import os
import sys

src = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
hits = sorted(glob.glob(os.path.join(src, "trace", "**", "run_kernel_trace.csv"), recursive=True))
if not hits:
    raise SystemExit(f"no run_kernel_trace.csv under {src}")
rows = sorted(({"name": r["Kernel_Name"].split("(")[0], "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"])}
               for r in csv.DictReader(open(hits[-1]))), key=lambda r: r["t0"])
# an ingest step's build starts at its k_build_classes
groups, cur = [], None
for r in rows:
    if "k_build_classes" in r["name"]:
        cur = []
        groups.append(cur)
    elif cur is not None and "k_build_" in r["name"] and "k_build_plan" not in r["name"]:
        cur.append(r)
groups = [g for g in groups if g][-steps:]
if groups:
    shape = [r["name"] for r in groups[-1]]
    same = [g for g in groups if [r["name"] for r in g] == shape]
    print(f"| build dispatch (launch order) | us, mean of {len(same)} steps | min | max |\n|---|---|---|---|")
    for i, name in enumerate(shape):
        d = [(g[i]["t1"] - g[i]["t0"]) / 1e3 for g in same]
        print(f"| {i + 1}. {name} | {sum(d) / len(d):.1f} | {min(d):.1f} | {max(d):.1f} |")
    span = [(max(r["t1"] for r in g) - min(r["t0"] for r in g)) / 1e3 for g in same]
    print(f"| first start to last end | {sum(span) / len(span):.1f} | {min(span):.1f} | {max(span):.1f} |")
    print()
tot = collections.defaultdict(list)
for r in rows:
    tot[r["name"]].append((r["t1"] - r["t0"]) / 1e3)
print("| kernel | calls | avg us | total ms |\n|---|---|---|---|")
for k, d in sorted(tot.items(), key=lambda kv: -sum(kv[1]))[:24]:
    print(f"| {k if len(k) <= 80 else k[:77] + '...'} | {len(d)} | {sum(d) / len(d):.1f} | {sum(d) / 1e3:.2f} |")
