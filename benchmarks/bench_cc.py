#!/usr/bin/env python
"""Weakly connected components (ConnectedComponents / gl_cc_*) on the graphs benchmarks/bench_graphs.py uses, one GPU.

Per graph one JSON line:
  hook_ms          gl_cc_begin + gl_cc_hook by HIP events on the library's stream (median of `runs` after three untimed runs)
  finish_ms        gl_cc_finish with the count, the same way, on the forest the hook left
  finish_rounds    pointer-doubling rounds that did work on that forest, the one that found nothing left to do included (the
                   forest is read back and doubled in numpy: the library enqueues ceil(log2 n) + 1 rounds and the later ones
                   return at once)
  run_ms           ConnectedComponents.run() end to end: the three steps, the synchronisation, the 4 n-byte read-back, the bincount
  floor_ms         (4 B x nnz + 4 B x rows) at 6.3 TB/s, the streaming rate DESIGN.md 4.9 uses; hook_over_floor, pass_over_floor
  bfs_pull_push_ms the BFS pull-push search on the same graph from the same process (bench_graphs' protocol)
  scipy_ms         scipy.sparse.csgraph.connected_components(directed=True, connection="weak") on the host, one call
--verify checks the labels against scipy's, renamed to each class's smallest vertex.

    python benchmarks/bench_cc.py [--graphs googleplus,orkut] [--verify] [--out profiles/cc.jsonl]
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

SPMV_GBPS = 6300.0


def span_ms(fn, runs, before=None):
    """Median GPU time of fn() (HIP events on the library's stream) after three untimed runs; `before` runs untimed each time."""
    from graphlily_amd import capi

    def once():
        if before is not None:
            before()
        capi.span_begin()
        fn()
        return capi.span_end()
    for _ in range(3):
        once()
    return float(np.median([once() for _ in range(runs)]))


def doubling_rounds(forest):
    """-> rounds of p = p[p] until a round changes nothing, that round included"""
    p = forest.astype(np.int64)
    rounds = 0
    while True:
        rounds += 1
        q = p[p]
        if np.array_equal(q, p):
            return rounds
        p = q


def scipy_labels(m, n):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    A = sp.csr_matrix((np.ones(m.nnz, np.int8), m.adj_indices.astype(np.int64), m.adj_indptr.astype(np.int64)), shape=(m.num_rows, m.num_cols))
    t0 = time.perf_counter()
    count, comp = connected_components(A, directed=True, connection="weak")
    t = time.perf_counter() - t0
    smallest = np.full(count, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(comp.shape[0]))
    lab = np.arange(n, dtype=np.uint32)
    lab[:comp.shape[0]] = smallest[comp]
    return lab, t


def run_graph(name, raw, iters, runs=9, verify=False):
    from graphlily_amd import app, capi
    from bench_graphs import bfs_times
    cc = app.ConnectedComponents(16, 0, 0)
    cc.set_up_runtime()
    cc.load_and_format_matrix(raw, True)
    cc.send_matrix_host_to_device()
    n, nnz = cc.n_, cc.get_nnz()
    plan = cc.SpMV_.plan_
    parent, labels, count = capi.DeviceBuffer(4 * n), capi.DeviceBuffer(4 * n), capi.DeviceBuffer(4)

    def hook():
        capi.cc_begin(parent, n)
        plan.cc_hook(parent)
    hook_ms = span_ms(hook, runs)
    hook()
    capi.sync()
    rounds = doubling_rounds(parent.read(np.uint32, n))
    finish_ms = span_ms(lambda: capi.cc_finish(parent, n, labels, count), runs, before=hook)
    for _ in range(3):
        lab = cc.run()
    ts = []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        lab = cc.run()
        ts.append(time.perf_counter() - t0)
    assert np.array_equal(labels.read(np.uint32, n), lab) and int(count.read(np.uint32, 1)[0]) - (n - cc.n_real_) == cc.num_components_
    floor_ms = (4.0 * nnz + 4.0 * n) / (SPMV_GBPS * 1e9) * 1e3
    rec = {"graph": name, "n": n, "nnz": nnz, "components": cc.num_components_, "largest_component": cc.largest_component_,
           "hook_ms": round(hook_ms, 4), "finish_ms": round(finish_ms, 4), "finish_rounds": rounds,
           "run_ms": round(float(np.median(ts)) * 1e3, 4), "floor_ms": round(floor_ms, 4),
           "hook_over_floor": round(hook_ms / floor_ms, 2), "pass_over_floor": round((hook_ms + finish_ms) / floor_ms, 2)}
    if verify:
        want, t = scipy_labels(raw, n)
        rec["scipy_ms"] = round(t * 1e3, 2)
        rec["verified"] = bool(np.array_equal(lab, want))
        assert rec["verified"], "%s: labels differ from scipy's" % name
    else:
        rec["scipy_ms"] = round(scipy_labels(raw, n)[1] * 1e3, 2)
    del cc, plan
    deg = np.diff(raw.adj_indptr.astype(np.int64))
    src = 0 if deg[0] > 0 else int(np.argmax(deg > 0))
    bfs = app.BFS(16, 0, 0, 0)
    bfs.set_up_runtime()
    bfs.load_and_format_matrix(raw, True)
    bfs.send_matrix_host_to_device()
    rec["bfs_pull_push_ms"] = round(bfs_times(bfs, src, iters, runs)["pull_push"]["s"] * 1e3, 4)
    rec["bfs_iters"] = iters
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="googleplus,ogbl_ppa,hollywood,pokec,ogbn_products,orkut")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cc.jsonl"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--verify", action="store_true", help="check the labels against scipy's")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi, datasets
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw, iters = datasets.paper_graph(name, 1.0, device=dev), datasets.PAPER_GRAPHS[name]["iters"]
        rec = run_graph(name, raw, iters, runs=args.runs, verify=args.verify)
        rec["data"] = "synthetic stand-in"
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
