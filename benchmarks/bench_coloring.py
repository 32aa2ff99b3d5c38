#!/usr/bin/env python
"""Graph colouring (GraphColoring / gl_color) on the stand-ins benchmarks/bench_kcore.py uses, at the same scale, one GPU.

Per graph and order (natural, random, largest_first, smallest_last) one JSON line:
  call_ms          gl_color alone (it synchronises itself), priorities already on the device, wall clock: median of `runs` after
                   three untimed runs; call_ms_min / call_ms_max: the spread
  run_ms           GraphColoring.run(order) end to end, the same way: the priorities on the host (for smallest_last a gl_kcore
                   call and the read-back of its order), their upload, gl_color, the 4 n-byte read-back, the host arithmetic
  num_colors, rounds, launches, widest, batches
  us_per_round     call_ms / rounds
  entries_per_s    entries of the symmetric matrix / call_ms (every stored entry is read once by the count and once by the round
                   of its row)
  kcore_call_ms, kcore_steps, kcore_us_per_step
                   gl_kcore on the same plan in the same session, steps = the (scan, peel, turn) triples that did work =
                   degeneracy + 1 scans + sub_rounds peels: the comparison the two passes allow, both being bound by the same
                   thing -- a chain of short dependent launches
  degeneracy       of the graph (gl_kcore); smallest_last needs at most degeneracy + 1 colours
  prepare_s        io.symmetrize_simple on the host (numpy), one call
--verify checks every colouring with app.validate_coloring against the priorities the run used (all four rules).
Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG (color_batch, default 64; color_cut, default 8; color_grid, default 4) and
are recorded; "color_batch", "color_cut" and "color_grid" of a line are the values the run used, whether set or defaulted.

    python benchmarks/bench_coloring.py [--graphs googleplus,orkut] [--scale 0.125] [--verify] [--out profiles/coloring.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from bench_kcore import wall_ms  # noqa: E402

COLOR_BATCH, COLOR_CUT, COLOR_GRID = 64, 8, 4       # the library's defaults (csrc/gl_color.hip): a line records the values its run used
ORDERS = ("natural", "random", "largest_first", "smallest_last")


def run_graph(name, raw, runs=9, verify=False, orders=ORDERS, seed=0):
    import time
    from graphlily_amd import app, capi, io
    t0 = time.perf_counter()
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    sym, deg = io.symmetrize_simple(padded)
    prepare_s = time.perf_counter() - t0
    gc = app.GraphColoring(16, 0, 0)
    gc.set_up_runtime()
    gc.load_and_format_matrix(raw, True)
    gc.send_matrix_host_to_device()
    n = gc.n_
    plan = gc.SpMV_.plan_
    color, prio_buf, core, peel = (capi.DeviceBuffer(4 * n) for _ in range(4))
    kstats = plan.kcore(core, peel)              # (the plan's first call: the two verdicts and the scratch)
    kcore_ms = wall_ms(lambda: plan.kcore(core), runs)
    kcore_steps = kstats[0] + 1 + kstats[2]
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    batch = min(max(int(knobs.get("color_batch", COLOR_BATCH)), 1), 4096)
    recs = []
    for order in orders:
        prio = io.coloring_priorities(deg, order, seed, peel_order=peel.read(np.uint32, n) if order == "smallest_last" else None)
        if prio is not None:
            prio_buf.write(prio)
        dp = prio_buf if prio is not None else None
        stats = plan.color(dp, color)
        call_ms = wall_ms(lambda: plan.color(dp, color), runs)
        got = color.read(np.uint32, n)
        run_ms = wall_ms(lambda: gc.run(order, seed), runs)
        if order != "smallest_last":             # (the driver peels again, and the peeling order is not unique)
            assert np.array_equal(got, gc.colors_) and (gc.num_colors_, gc.rounds_, gc.widest_) == (stats[0], stats[1], stats[3])
        assert (stats[2] - 2) % (2 * batch) == 0, "launches = 2 + 2 x color_batch x batches: is COLOR_BATCH still the library's default?"
        rec = {"graph": name, "order": order, "seed": seed, "n": n, "nnz": raw.nnz, "symmetric_entries": sym.nnz, "longest_row": int(deg.max()),
               "num_colors": stats[0], "rounds": stats[1], "launches": stats[2], "widest": stats[3], "batches": (stats[2] - 2) // (2 * batch),
               "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
               "run_ms": round(run_ms[0], 4), "run_ms_min": round(run_ms[1], 4), "run_ms_max": round(run_ms[2], 4), "runs": runs,
               "us_per_round": round(call_ms[0] * 1e3 / stats[1], 3) if stats[1] else None,
               "entries_per_s": round(sym.nnz / (call_ms[0] * 1e-3), 1) if call_ms[0] > 0 else None,
               "degeneracy": kstats[0], "kcore_call_ms": round(kcore_ms[0], 4), "kcore_steps": kcore_steps,
               "kcore_us_per_step": round(kcore_ms[0] * 1e3 / kcore_steps, 3) if kcore_steps else None,
               "prepare_s": round(prepare_s, 3), "color_batch": batch, "color_cut": int(knobs.get("color_cut", COLOR_CUT)),
               "color_grid": int(knobs.get("color_grid", COLOR_GRID)), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
        if verify:
            rec["verified"] = app.validate_coloring(padded, got, prio) == stats[0]
            if order == "smallest_last":
                rec["verified"] = rec["verified"] and stats[0] <= kstats[0] + 1
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--orders", default=",".join(ORDERS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coloring.jsonl"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--verify", action="store_true", help="check every colouring with app.validate_coloring")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, runs=args.runs, verify=args.verify, orders=args.orders.split(",")):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
