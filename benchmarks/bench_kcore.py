#!/usr/bin/env python
"""k-core decomposition (KCore / gl_kcore) on the graphs benchmarks/bench_graphs.py uses, one GPU.

Per graph one JSON line:
  run_ms           KCore.run() end to end, wall clock: the launches, the per-batch read-backs, the 4 n-byte read-back of the core
                   numbers, the host arithmetic (median of `runs` after three untimed runs; run_ms_min / run_ms_max: the spread)
  call_ms          gl_kcore alone (it synchronises itself), wall clock, the same way; order_ms: with the peeling order as well
  degeneracy, levels, sub_rounds, launches, batches
  entries_peeled_per_s   entries of the symmetric matrix (every row is walked once, when its vertex is peeled) / call_ms
  readback_ms      one copy of the control record to page-locked memory + wait on an IDLE stream (median of 200), and
  readback_share   batches x readback_ms / call_ms: the share of the call spent in the per-batch read-backs -- an estimate:
                   the wait of a real batch also covers the launches that were still running
  prepare_s        io.symmetrize_simple on the host (numpy), one call
--verify checks the core numbers and the order with app.validate_cores (an independent host peel).
Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG (kcore_batch, default 64; kcore_cut, default 8; kcore_grid, default 4) and
are recorded; "kcore_batch" and "kcore_cut" of a line are the values the run used, whether set or defaulted.

    python benchmarks/bench_kcore.py [--graphs googleplus,orkut] [--scale 0.125] [--verify] [--out profiles/kcore.jsonl]
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

KCORE_BATCH, KCORE_CUT = 64, 8       # the library's defaults (csrc/gl_kcore.hip): a line records the values its run used


def wall_ms(fn, runs):
    """wall-clock times of fn() in ms (the stream is idle before every call) after three untimed runs -> (median, min, max)"""
    from graphlily_amd import capi
    for _ in range(3):
        fn()
    ts = []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def run_graph(name, raw, runs=9, verify=False):
    from graphlily_amd import app, capi, io
    t0 = time.perf_counter()
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    sym, deg = io.symmetrize_simple(padded)
    prepare_s = time.perf_counter() - t0
    kc = app.KCore(16, 0, 0)
    kc.set_up_runtime()
    kc.load_and_format_matrix(raw, True)
    kc.send_matrix_host_to_device()
    n = kc.n_
    plan = kc.SpMV_.plan_
    core, order = capi.DeviceBuffer(4 * n), capi.DeviceBuffer(4 * n)
    stats = plan.kcore(core)                  # (the plan's first call: the two verdicts and the scratch)
    call_ms = wall_ms(lambda: plan.kcore(core), runs)
    order_ms = wall_ms(lambda: plan.kcore(core, order), runs)
    run_ms = wall_ms(lambda: kc.run(), runs)
    assert np.array_equal(core.read(np.uint32, n), kc.core_) and (kc.degeneracy_, kc.levels_, kc.sub_rounds_) == stats[:3]
    word = capi.DeviceBuffer(64)
    rb = wall_ms(lambda: word.read(np.uint32, 8), 200)
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    batch = min(max(int(knobs.get("kcore_batch", KCORE_BATCH)), 1), 4096)
    assert (stats[3] - 1) % (3 * batch) == 0, "launches = 1 + 3 x kcore_batch x batches: is KCORE_BATCH still the library's default?"
    batches = (stats[3] - 1) // (3 * batch)
    rec = {"graph": name, "n": n, "nnz": raw.nnz, "symmetric_entries": sym.nnz, "longest_row": int(deg.max()),
           "degeneracy": stats[0], "levels": stats[1], "sub_rounds": stats[2], "launches": stats[3], "batches": batches,
           "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
           "order_ms": round(order_ms[0], 4), "run_ms": round(run_ms[0], 4), "run_ms_min": round(run_ms[1], 4),
           "run_ms_max": round(run_ms[2], 4), "runs": runs,
           "entries_peeled_per_s": round(sym.nnz / (call_ms[0] * 1e-3), 1) if call_ms[0] > 0 else None,
           "readback_ms": round(rb[0], 4), "readback_share": round(batches * rb[0] / call_ms[0], 4) if call_ms[0] > 0 else None,
           "prepare_s": round(prepare_s, 3), "kcore_batch": batch, "kcore_cut": int(knobs.get("kcore_cut", KCORE_CUT)),
           "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    if verify:
        kc.run(order=True)
        rec["verified"] = app.validate_cores(padded, kc.core_, kc.order_) == stats[0]
    return rec


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kcore.jsonl"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--verify", action="store_true", help="check the core numbers and the order with app.validate_cores")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        rec = run_graph(name, raw, runs=args.runs, verify=args.verify)
        rec["scale"] = args.scale
        rec["data"] = "synthetic stand-in"
        print(json.dumps(rec), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
