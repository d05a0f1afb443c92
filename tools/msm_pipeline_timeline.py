#!/usr/bin/env python3
"""The pipelined MSM's timeline from a rocprofv3 --kernel-trace CSV: where the tree and the next front lie against the neighbour's
accumulation.

  tools/msm_pipeline_timeline.py KERNEL_TRACE.csv [--last N] [--acc SUBSTR]

Every MSM of the traced run must have the same shape (bench.py --no-legs --no-commits --no-cpu --no-host-boundary --no-pmc): the j-th
launch of k_digits_partition, k_size_order, k_bucket_sum30 and k_tree_tail then belong to MSM j.  Prints, for the last N MSMs (the
timed region of the bench), in microseconds:
  acc      length of MSM k's accumulation
  gap      end of accumulation k -> start of accumulation k+1
  tree     end of accumulation k -> end of its k_tree_tail
  tree_in  1 if that tail ends before accumulation k+1 does (the tree finishes inside the neighbour's accumulation)
  f_start, f_end   start of k_digits_partition / end of k_size_order of MSM k+2, measured from the START of accumulation k+1
  f_in     1 if that front ends before accumulation k+1 does
and the medians."""
import csv
import statistics
import sys


def col(row, *names):
    for n in names:
        if n in row:
            return row[n]
    raise KeyError(names)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    last = int(sys.argv[sys.argv.index("--last") + 1]) if "--last" in sys.argv else 20
    acc_name = sys.argv[sys.argv.index("--acc") + 1] if "--acc" in sys.argv else "k_bucket_sum30"
    args = [a for a in args if a not in (str(last), acc_name)] or args
    kinds = {"acc": acc_name, "tail": "k_tree_tail", "digits": "k_digits_partition", "order": "k_size_order"}
    ev = {k: [] for k in kinds}
    others = {}
    for row in csv.DictReader(open(args[0])):
        name = col(row, "Kernel_Name", "KernelName")
        s, e = int(col(row, "Start_Timestamp", "BeginNs")), int(col(row, "End_Timestamp", "EndNs"))
        for k, sub in kinds.items():
            if sub in name:
                ev[k].append((s, e))
        short = name.split("<")[0].replace("void ", "").replace("porla::", "")
        t = others.setdefault(short, [0, 0])
        t[0] += 1
        t[1] += e - s
    for k in ev:
        ev[k].sort()
    n = min(len(v) for v in ev.values())
    if len({len(v) for v in ev.values()}) != 1:
        print("note: launch counts differ (%s): aligned from the end" % {k: len(v) for k, v in ev.items()})
    for k in ev:
        ev[k] = ev[k][len(ev[k]) - n:]
    lo = max(0, n - last - 2)
    us = lambda ns: ns / 1e3
    rows = []
    print("%4s %8s %8s %8s %7s %8s %8s %5s" % ("msm", "acc", "gap", "tree", "tree_in", "f_start", "f_end", "f_in"))
    for k in range(lo, n - 2):
        a, a1 = ev["acc"][k], ev["acc"][k + 1]
        r = {"acc": us(a[1] - a[0]), "gap": us(a1[0] - a[1]), "tree": us(ev["tail"][k][1] - a[1]),
             "tree_in": int(ev["tail"][k][1] <= a1[1]),
             "f_start": us(ev["digits"][k + 2][0] - a1[0]), "f_end": us(ev["order"][k + 2][1] - a1[0]),
             "f_in": int(ev["order"][k + 2][1] <= a1[1])}
        rows.append(r)
        print("%4d %8.1f %8.1f %8.1f %7d %8.1f %8.1f %5d" % (k, r["acc"], r["gap"], r["tree"], r["tree_in"], r["f_start"], r["f_end"], r["f_in"]))
    if rows:
        med = lambda key: statistics.median(r[key] for r in rows)
        print("%4s %8.1f %8.1f %8.1f %7s %8.1f %8.1f %5s" % ("med", med("acc"), med("gap"), med("tree"),
              "%d/%d" % (sum(r["tree_in"] for r in rows), len(rows)), med("f_start"), med("f_end"),
              "%d/%d" % (sum(r["f_in"] for r in rows), len(rows))))
        span = ev["acc"][n - 2][0] - ev["acc"][lo][0]
        print("accumulation start to start: %.1f us per MSM over %d MSMs" % (us(span) / (n - 2 - lo), n - 2 - lo))
    print("kernel totals over the whole trace (launches, us per launch):")
    for name, (cnt, ns) in sorted(others.items(), key=lambda kv: -kv[1][1])[:16]:
        print("  %-28s %6d %10.1f" % (name, cnt, us(ns) / cnt))


if __name__ == "__main__":
    main()
