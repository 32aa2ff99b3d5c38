#!/usr/bin/env python
"""The BFS predecessor tree (BFS.parents / gl_bfs_parents) on the graphs benchmarks/bench_graphs.py uses, one GPU.

Per graph one JSON line:
  pull_push_ms        the search, bench_graphs' protocol (14 untimed calls, median wall time of `runs`)
  parents_kernel_ms   the tree pass alone by HIP events (level packing + the row pass; median of `runs` spans)
  parents_ms          BFS.parents() end to end: the pass, the device synchronisation and the 4 n-byte read-back
  entries_read        row entries the pass read (gl_bfs_parents_entries) against the matrix' nnz: what early exit saves
  floor_ms            the full-scan path's floor, (4 B x nnz + 4 B x rows) at 6.3 TB/s (the general SpMV's rate, profiles/README.md)
  teps_nominal        nnz x iterations / pull_push time (the reference's definition, bench_bfs.cpp)
  teps_graph500       input entries with at least one reached endpoint / (search + tree time)
  variants            --ab: the pass's GPU time with one design decision changed at a time (GRAPHLILY_DEBUG knobs, read per call)
and the tree is checked: parents == the numpy definition on the run's own levels is left to the tests; here
app.validate_bfs_tree must pass (--no-validate skips it on the large graphs).

    python benchmarks/bench_bfs_parents.py [--graphs googleplus,orkut] [--ab] [--out profiles/bfs_parents.jsonl]
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

VARIANTS = [("default", {}), ("floats", {"parents_u8": 0}), ("full_scan", {"parents_early": 0}),
            ("full_scan_floats", {"parents_early": 0, "parents_u8": 0}),
            ("cut_0", {"parents_cut": 0}), ("cut_16", {"parents_cut": 16}), ("cut_64", {"parents_cut": 64}),
            ("cut_128", {"parents_cut": 128}), ("cut_512", {"parents_cut": 512}), ("thread_per_row", {"parents_cut": 1 << 30}),
            ("full_scan_thread_per_row", {"parents_early": 0, "parents_cut": 1 << 30}),
            ("grid_16", {"parents_grid": 16}), ("grid_256", {"parents_grid": 256})]


def with_knobs(knobs, fn):
    old = os.environ.get("GRAPHLILY_DEBUG")
    cur = dict(kv.split("=", 1) for kv in (old or "").split(",") if kv)
    cur.update({k: str(v) for k, v in knobs.items()})
    if cur:
        os.environ["GRAPHLILY_DEBUG"] = ",".join("%s=%s" % kv for kv in cur.items())
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("GRAPHLILY_DEBUG", None)
        else:
            os.environ["GRAPHLILY_DEBUG"] = old


def kernel_ms(plan, levels, parent, runs, knobs=None):
    """Median GPU time of one gl_bfs_parents call (HIP events on the library's stream) after three untimed ones."""
    from graphlily_amd import capi

    def once():
        capi.span_begin()
        plan.bfs_parents(levels, parent, None)
        return capi.span_end()

    def series():
        for _ in range(3):
            once()
        return float(np.median([once() for _ in range(runs)]))
    return with_knobs(knobs or {}, series)


def run_graph(name, raw, iters, runs=9, ab=False, validate=True):
    from graphlily_amd import app, capi, io
    from bench_graphs import bfs_times
    deg = np.diff(raw.adj_indptr.astype(np.int64))
    src = 0 if deg[0] > 0 else int(np.argmax(deg > 0))
    bfs = app.BFS(16, 0, 0, 0)
    bfs.set_up_runtime()
    bfs.load_and_format_matrix(raw, True)
    bfs.send_matrix_host_to_device()
    n, nnz = bfs.n_, bfs.get_nnz()
    bt = bfs_times(bfs, src, iters, runs)
    t_pp, d = bt["pull_push"]["s"], bt["pull_push"]["d"]
    d = bfs.pull_push(src, iters, 0.001).copy()           # (parents(): the last run's levels)
    for _ in range(3):
        p = bfs.parents()
    ts = []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        p = bfs.parents()
        ts.append(time.perf_counter() - t0)
    t_par = float(np.median(ts))
    plan = bfs.SpMV_.plan_
    levels = capi.DeviceBuffer.from_host(d)
    parent = capi.DeviceBuffer(4 * n)
    k_ms = kernel_ms(plan, levels, parent, runs)
    read = plan.bfs_parents_entries(levels, parent)
    read_full = with_knobs({"parents_early": 0}, lambda: plan.bfs_parents_entries(levels, parent))
    assert np.array_equal(parent.read(np.uint32, n), p)
    reached = d > 0
    ip = raw.adj_indptr.astype(np.int64)
    rows_reached = np.zeros(ip.shape[0] - 1, bool)
    rows_reached[:] = reached[:ip.shape[0] - 1]
    # input entries with at least one reached endpoint (Graph500 counts the edges of the traversed component)
    touched = 0
    step = 1 << 18
    for r0 in range(0, ip.shape[0] - 1, step):
        r1 = min(ip.shape[0] - 1, r0 + step)
        cols = raw.adj_indices[ip[r0]:ip[r1]]
        rr = np.repeat(rows_reached[r0:r1], np.diff(ip[r0:r1 + 1]))
        touched += int(np.count_nonzero(rr | reached[cols]))
    floor_ms = (4.0 * nnz + 4.0 * n) / (SPMV_GBPS * 1e9) * 1e3
    rec = {"graph": name, "n": n, "nnz": nnz, "iters": iters, "source": src, "reached": int(reached.sum()),
           "rows_sorted": plan.rows_sorted(), "pull_push_ms": round(t_pp * 1e3, 4), "parents_kernel_ms": round(k_ms, 4),
           "parents_ms": round(t_par * 1e3, 4), "parents_kernel_over_search": round(k_ms / (t_pp * 1e3), 3),
           "entries_read": int(read), "entries_read_frac": round(read / max(nnz, 1), 4), "entries_read_full_scan": int(read_full),
           "floor_ms": round(floor_ms, 4), "teps_nominal": round(nnz * iters / t_pp, 1),
           "teps_graph500": round(touched / (t_pp + t_par), 1), "teps_graph500_kernel_only": round(touched / (t_pp + k_ms * 1e-3), 1),
           "edges_touched": touched, "orphans": bfs.orphans_}
    if ab:
        # every variant twice, interleaved with the default, so that drift shows as a spread of the default's figures
        rec["variants"] = {}
        for rep in range(2):
            for label, knobs in VARIANTS:
                rec["variants"].setdefault(label, []).append(round(kernel_ms(plan, levels, parent, runs, knobs), 4))
                assert np.array_equal(parent.read(np.uint32, n), p), label
        rec["full_scan_over_floor"] = round(min(rec["variants"]["full_scan"]) / floor_ms, 2)
    if validate:
        unit = io.CSRMatrix(raw.num_rows, raw.num_cols, np.ones(raw.nnz, np.float32), raw.adj_indices, raw.adj_indptr)
        rec["validated"] = app.validate_bfs_tree(unit, src, d, p, num_iterations=iters) == int(reached.sum())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="googleplus,ogbl_ppa,hollywood,pokec,ogbn_products,orkut")
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--ab", action="store_true", help="also time the pass with one design decision changed at a time")
    ap.add_argument("--no-validate", action="store_true")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi, datasets
    dev = torch.device("cuda:0")
    capi.init(0)
    lines = []
    for name in args.graphs.split(","):
        raw, iters = datasets.paper_graph(name, 1.0, device=dev), datasets.PAPER_GRAPHS[name]["iters"]
        rec = run_graph(name, raw, iters, runs=args.runs, ab=args.ab, validate=not args.no_validate)
        rec["data"] = "synthetic stand-in"
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if args.out:
            with open(args.out, "w") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
