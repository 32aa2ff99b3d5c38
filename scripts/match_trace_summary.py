#!/usr/bin/env python
"""Where a gl_match call spends its kernel time, from a rocprofv3 kernel trace of `benchmarks/bench_match.py --calls-only`:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python benchmarks/bench_match.py --calls-only --graphs orkut --out ""
    python scripts/match_trace_summary.py DIR [--out profiles/match_kernel_share.csv]

A call starts at its match_begin_kernel.  Its rounds are counted by match_turn_kernel dispatches (the first turn follows the begin):
the point, pair and collect dispatches between turn k and turn k + 1 belong to round k.  Per call: kernel time by kernel, the share
of round 1, and the launches that ran after the record said done (gated: they return at once).  One CSV line per call; the calls
of one graph and weighting follow each other in the order bench_match.py made them (first the hash weights, then the equal ones)."""
import argparse
import csv
import glob
import os
import sys


KINDS = ("begin", "point", "pair", "collect", "turn", "finish")


def calls_of(rows):
    call = None
    for r in rows:
        name = r["Kernel_Name"]
        if "match_" not in name:
            continue
        kind = name.split("match_")[1].split("_kernel")[0]
        if kind not in KINDS:
            continue
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if kind == "begin":
            if call:
                yield call
            call = {"turns": 0, "us": {}, "round1_us": 0.0, "launches": 0, "start": int(r["Start_Timestamp"]), "end": 0}
        if call is None:
            continue
        call["us"][kind] = call["us"].get(kind, 0.0) + us
        call["launches"] += 1
        call["end"] = int(r["End_Timestamp"])
        if kind == "turn":
            call["turns"] += 1
        elif kind in ("point", "pair", "collect") and call["turns"] == 1:
            call["round1_us"] += us
    if call:
        yield call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    files = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % args.dir)
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = open(args.out, "w") if args.out else sys.stdout
    print(",".join(("call", "launches", "span_us", "kernel_us") + tuple(k + "_us" for k in KINDS) + ("round1_us", "round1_share")), file=out)
    for i, c in enumerate(calls_of(rows)):
        total = sum(c["us"].values())
        print(",".join([str(i), str(c["launches"]), "%.1f" % ((c["end"] - c["start"]) / 1e3), "%.1f" % total] +
                       ["%.1f" % c["us"].get(k, 0.0) for k in KINDS] + ["%.1f" % c["round1_us"], "%.3f" % (c["round1_us"] / total if total else 0.0)]),
              file=out)


if __name__ == "__main__":
    main()
