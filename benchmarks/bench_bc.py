#!/usr/bin/env python
"""Betweenness centrality (BetweennessCentrality / gl_bc_accumulate) on the stand-ins benchmarks/bench_kcore.py uses, one GPU,
16 fixed sources per graph.

Per graph one JSON line:
  bfs_ms             bfs_.pull_push(s, N) alone, wall clock per source: the device-resident schedule and the read-back of the
                     levels, the code path the parent commit has (median over the sources of the median of `runs` calls each,
                     after one untimed call per source; N = the depth the driver settled on)
  accumulate_ms      gl_bc_accumulate alone on the levels that search left on the device, with the stats (it waits at its end)
  bfs_accumulate_ms  both, back to back: what BetweennessCentrality.run() does per source
  ratio              bfs_accumulate_ms / bfs_ms: the number to report
  run_ms_per_source  BetweennessCentrality.run(sources) end to end / 16 (one run after an untimed one): adds the read-back of bc
  edges_swept_per_s  entries of the rows the two sweeps walk (forward: the rows of plan_in on levels >= 2, backward: the rows of
                     plan_out on levels 2 .. D - 1), summed over the sources / the summed accumulate times
  depth, reached     the deepest level and the median number of reached vertices over the sources
  bc_cut, bc_grid    the knob values the run used, whether set through GRAPHLILY_DEBUG or defaulted; layout: which gather layout
                     the library has ("level_first": the only one built)
--verify checks the result with app.validate_betweenness (host BFS levels and the host restatement).

    python benchmarks/bench_bc.py [--graphs googleplus,pokec] [--scale 0.125] [--verify] [--out profiles/bc.jsonl]
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

GRAPHS = "googleplus,ogbl_ppa,hollywood,pokec"
BC_CUT, BC_GRID = 8, 4               # the library's defaults (csrc/gl_bc.hip): a line records the values its run used
NUM_SOURCES = 16


def timed_ms(fn, runs):
    from graphlily_amd import capi
    ts = []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        fn()
        capi.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run_graph(name, raw, runs=5, verify=False):
    from graphlily_amd import app, capi
    d = app.BetweennessCentrality(16, 0, 0, 0)
    d.set_up_runtime()
    t0 = time.perf_counter()
    d.load_and_format_matrix(raw, True)
    prepare_s = time.perf_counter() - t0
    d.send_matrix_host_to_device()
    n = d.n_
    deg_in = np.diff(d.SpMV_.csr_matrix_.adj_indptr.astype(np.int64))
    out_m = d.SpMV_ if d.out_ is None else d.out_
    deg_out = np.diff(out_m.csr_matrix_.adj_indptr.astype(np.int64))
    rng = np.random.default_rng(23)
    sources = [int(s) for s in rng.choice(np.flatnonzero(deg_out[:d.n_real_] > 0), NUM_SOURCES, replace=False)]
    d.run(sources)                            # untimed: the plans' first calls, the depth, the recorded schedule
    t0 = time.perf_counter()
    got = d.run(sources)
    run_ms = (time.perf_counter() - t0) * 1e3
    N = 16                                    # (the driver's own rule: depth_hint = 16, doubled while a search may be truncated)
    while max(d.depths_) >= N + 1 and N < n:
        N = min(2 * N, n)
    bfs, plan_out = d.bfs_, (None if d.out_ is None else d.out_.plan_)
    bc = capi.DeviceBuffer(8 * n)
    t_bfs, t_acc, t_both, swept, reached = [], [], [], 0, []
    for s in sources:
        level = np.array(bfs.pull_push(s, N))
        levels = bfs.levels_[0]
        stats = d.SpMV_.plan_.bc_accumulate(plan_out, levels, bc, 1.0, False)
        D = stats[0]
        swept += int(deg_in[level >= 2].sum()) + int(deg_out[(level >= 2) & (level < D)].sum())
        reached.append(stats[1])
        t_bfs.append(timed_ms(lambda: bfs.pull_push(s, N), runs))
        t_acc.append(timed_ms(lambda: d.SpMV_.plan_.bc_accumulate(plan_out, bfs.levels_[0], bc, 1.0, False), runs))

        def both():
            bfs.pull_push(s, N)
            d.SpMV_.plan_.bc_accumulate(plan_out, bfs.levels_[0], bc, 1.0, True)
        t_both.append(timed_ms(both, runs))
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    bfs_ms, acc_ms, both_ms = float(np.median(t_bfs)), float(np.median(t_acc)), float(np.median(t_both))
    rec = {"graph": name, "n": n, "nnz": raw.nnz, "pattern_entries": int(deg_in.sum()), "directed": bool(d.directed_),
           "longest_row": int(max(deg_in.max(), deg_out.max())), "sources": NUM_SOURCES, "iterations": N, "depth": int(max(d.depths_)),
           "reached": int(np.median(reached)), "bfs_ms": round(bfs_ms, 4), "accumulate_ms": round(acc_ms, 4),
           "bfs_accumulate_ms": round(both_ms, 4), "ratio": round(both_ms / bfs_ms, 3) if bfs_ms > 0 else None,
           "run_ms_per_source": round(run_ms / NUM_SOURCES, 4), "runs": runs,
           "edges_swept_per_s": round(swept / (sum(t_acc) * 1e-3), 1) if sum(t_acc) > 0 else None,
           "overflowed": len(d.overflowed_), "prepare_s": round(prepare_s, 3), "layout": "level_first",
           "bc_cut": int(knobs.get("bc_cut", BC_CUT)), "bc_grid": int(knobs.get("bc_grid", BC_GRID)),
           "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    if verify:
        rec["max_rel_err"] = app.validate_betweenness(raw, got, sources)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=GRAPHS)
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--verify", action="store_true", help="check the result with app.validate_betweenness")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi, datasets
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
