#!/usr/bin/env python
"""Greedy weighted matching (gl_match) on the stand-ins benchmarks/bench_msf.py uses, at the same scale, one GPU.

Per graph and per weighting ("hash": 1 + hash(lo, hi) % 255, "equal": every weight 1) one JSON line:
  call_ms          gl_match alone (it synchronises itself), wall clock: median of `runs` after three untimed runs; call_ms_min /
                   call_ms_max: the spread.  The plan's first call (verdicts, scratch) is timed once as first_call_ms
  matched, rounds, scans, launches
                   matched edges; rounds in which a vertex pointed or finished; row scans of all rounds; launches enqueued
  round1_scans     the vertices with a row: round 1 scans every row once, i.e. streams every entry; round1_scan_share =
                   round1_scans / scans (a share of the SCANS, not of the time: scripts/match_trace_summary.py gives that)
  us_per_round     call_ms / rounds
  sweep_bytes      12 * entries: 4 B index + 4 B weight + one 4 B mate gather per entry, what round 1 must move at least
  model_ms         sweep_bytes at 6.29 TB/s (the measured float4-copy rate of the card): round 1 as ONE streaming sweep;
                   call_over_model = call_ms / model_ms
  msf_ms           gl_msf (forest words only) on the same plan and weights in the same process; call_over_msf = call_ms / msf_ms
  kcore_ms, kcore_sub_rounds, kcore_us_per_sub_round
                   gl_kcore on the same plan in the same process and its time per sub-round, next to us_per_round
  host_greedy_ms   app._greedy_matching_of on the host, one call; its mates must equal the device's
  total_weight
--ab adds one short line per knob value ("ab": "match_cut=8", call_ms and the statistics), timed on the same plan in the same
process right behind the default line (the knobs are read per call): match_cut 0 / 8 / 32 / 128, match_grid 8 / 16 / 64 / 256,
match_batch 1 / 2 / 4 / 8 / 16 / 32, match_spread 0 / 1 / 4 / 8 / 16 / 32.
--calls-only runs nothing but `runs` calls per graph and weighting: the run to put under a kernel trace.
Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG (match_cut, default 32; match_grid, default 64; match_batch, default 8;
match_spread, default 16) and are recorded with every line.

    python benchmarks/bench_match.py [--graphs googleplus,orkut] [--scale 0.125] [--ab] [--out profiles/match.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from bench_kcore import wall_ms  # noqa: E402
from bench_msf import COPY_BYTES_PER_S, weights_of  # noqa: E402
from bench_truss import _with_knob  # noqa: E402

MATCH_CUT, MATCH_GRID, MATCH_BATCH, MATCH_SPREAD = 32, 64, 8, 16                # the library's defaults (csrc/gl_match.hip)

AB = [("match_cut", v) for v in (0, 8, 32, 128)] + [("match_grid", v) for v in (8, 16, 64, 256)] + \
     [("match_batch", v) for v in (1, 2, 4, 8, 16, 32)] + [("match_spread", v) for v in (0, 1, 4, 8, 16, 32)]


def run_graph(name, raw, runs=5, ab=False, host=True, calls_only=False):
    from graphlily_amd import app, capi, io
    t0 = time.perf_counter()
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    sym, deg = io.symmetrize_weighted(padded, weighted=False)
    prepare_s = time.perf_counter() - t0
    n, nnz = sym.num_rows, sym.nnz
    plan = capi.SpMVPlan(n, n, sym.adj_indptr, sym.adj_indices, sym.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    mate, forest, core = capi.DeviceBuffer(4 * max(1, n)), capi.DeviceBuffer(4 * max(1, nnz)), capi.DeviceBuffer(4 * max(1, n))
    round1 = int(np.count_nonzero(deg))
    first = True
    for kind in ("hash", "equal"):
        w_host = weights_of(sym, kind)
        w = capi.DeviceBuffer.from_host(w_host)
        capi.sync()
        t0 = time.perf_counter()
        stats = plan.match(w, mate)
        first_call_ms = (time.perf_counter() - t0) * 1e3 if first else None
        first = False
        print("%s/%s: %d matched, %d rounds, %d scans, %d launches" % ((name, kind) + stats), file=sys.stderr, flush=True)
        if calls_only:
            for _ in range(runs):
                plan.match(w, mate)
            continue
        call_ms = wall_ms(lambda: plan.match(w, mate), runs)
        got = mate.read(np.uint32, n)
        msf_ms = wall_ms(lambda: plan.msf(w, forest), runs)
        kcore_stats = plan.kcore(core)
        kcore_ms = wall_ms(lambda: plan.kcore(core), runs)
        weighted = io.CSRMatrix(n, n, w_host, sym.adj_indices, sym.adj_indptr)
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
        cols = sym.adj_indices.astype(np.int64)
        once = (got.astype(np.int64)[rows] == cols) & (cols > rows)
        assert int(once.sum()) == stats[0], "the mates and the count of matched edges disagree"
        free = got == 0xffffffff
        assert not np.any(free[rows] & free[cols]), "an edge has two free ends"
        total = float(w_host[once].astype(np.float64).sum())
        host_ms = None
        if host:
            t0 = time.perf_counter()
            want = app._greedy_matching_of(weighted)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(want, got), "the host's greedy matching differs"
        model_ms = 12.0 * nnz / COPY_BYTES_PER_S * 1e3
        knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
        rec = {"graph": name, "weights": kind, "n": n, "nnz": raw.nnz, "symmetric_entries": nnz, "longest_row": int(deg.max()) if n else 0,
               "matched": stats[0], "rounds": stats[1], "scans": stats[2], "launches": stats[3], "total_weight": total,
               "round1_scans": round1, "round1_scan_share": round(round1 / stats[2], 4) if stats[2] else None,
               "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
               "us_per_round": round(call_ms[0] * 1e3 / stats[1], 2) if stats[1] else None,
               "sweep_bytes": 12 * nnz, "model_ms": round(model_ms, 4), "call_over_model": round(call_ms[0] / model_ms, 2) if model_ms > 0 else None,
               "msf_ms": round(msf_ms[0], 4), "call_over_msf": round(call_ms[0] / msf_ms[0], 3) if msf_ms[0] > 0 else None,
               "kcore_ms": round(kcore_ms[0], 4), "kcore_sub_rounds": kcore_stats[2],
               "kcore_us_per_sub_round": round(kcore_ms[0] * 1e3 / kcore_stats[2], 2) if kcore_stats[2] else None,
               "host_greedy_ms": round(host_ms, 2) if host_ms is not None else None, "runs": runs, "prepare_s": round(prepare_s, 3),
               "match_cut": int(knobs.get("match_cut", MATCH_CUT)), "match_grid": int(knobs.get("match_grid", MATCH_GRID)),
               "match_batch": int(knobs.get("match_batch", MATCH_BATCH)),
               "match_spread": int(knobs.get("match_spread", MATCH_SPREAD)), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
        if first_call_ms is not None:
            rec["first_call_ms"] = round(first_call_ms, 4)
        yield rec
        for key, value in AB if ab else ():
            res = _with_knob(key, value, lambda: (plan.match(w, mate), wall_ms(lambda: plan.match(w, mate), runs)))
            assert res[0][:3] == stats[:3] and np.array_equal(mate.read(np.uint32, n), got)
            yield {"graph": name, "weights": kind, "ab": "%s=%d" % (key, value), "call_ms": round(res[1][0], 4),
                   "call_ms_min": round(res[1][1], 4), "call_ms_max": round(res[1][2], 4), "launches": res[0][3], "runs": runs,
                   "rounds": stats[1], "scans": stats[2], "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plan")
    ap.add_argument("--no-host", action="store_true", help="skip the greedy matching on the host")
    ap.add_argument("--calls-only", action="store_true", help="only `runs` calls per graph and weighting (for a kernel trace)")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, runs=args.runs, ab=args.ab, host=not args.no_host, calls_only=args.calls_only):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
