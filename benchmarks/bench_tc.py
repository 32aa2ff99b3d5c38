#!/usr/bin/env python
"""Triangle counting (TriangleCount / gl_tc_count) on the graphs benchmarks/bench_graphs.py uses, one GPU.

Per graph one JSON line:
  total_ms         gl_tc_count without per-vertex counts, by HIP events on the library's stream (median of `runs` after three untimed runs)
  per_vertex_ms    gl_tc_count with them, the same way
  triangles, oriented_entries, longest_oriented_row, longest_undirected_row
  two_hop_entries  sum over v, u in N(v) of |N(u)| on the oriented matrix: the entries the kernel looks up; two_hop_per_s (total-only)
  prepare_s        io.triangle_orient on the host (numpy), one call: what a device-side orientation would have to beat
  run_ms           TriangleCount.run() end to end: the kernel, the synchronisation, the 8 n-byte read-back, the host arithmetic
  scipy_ms         ((L L^T) o L).sum() on the oriented matrix on the host, one call -- the only yardstick there is; null ("not
                   measured") above --scipy-limit two-hop entries
--verify checks the per-vertex counts with app.validate_triangles (an independent scipy statement on the symmetric matrix).
Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG (tc_group, tc_search, tc_short, tc_wave, tc_lds, tc_grid) and are recorded.

    python benchmarks/bench_tc.py [--graphs googleplus,orkut] [--scale 0.125] [--verify] [--out profiles/tc.jsonl]
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


def span_ms(fn, runs):
    """Median GPU time of fn() (HIP events on the library's stream) after three untimed runs."""
    from graphlily_amd import capi

    def once():
        capi.span_begin()
        fn()
        return capi.span_end()
    for _ in range(3):
        once()
    return float(np.median([once() for _ in range(runs)]))


def scipy_total(o):
    import scipy.sparse as sp
    L = sp.csr_matrix((np.ones(o.nnz, np.int64), o.adj_indices.astype(np.int64), o.adj_indptr.astype(np.int64)), shape=(o.num_rows, o.num_cols))
    t0 = time.perf_counter()
    total = int((L @ L.T).multiply(L).sum())
    return total, time.perf_counter() - t0


def run_graph(name, raw, runs=9, verify=False, scipy_limit=2e8):
    from graphlily_amd import app, capi, io
    t0 = time.perf_counter()
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    oriented, deg = io.triangle_orient(padded)
    prepare_s = time.perf_counter() - t0
    lens = np.diff(oriented.adj_indptr.astype(np.int64))
    two_hop = int(lens[oriented.adj_indices].sum())
    tc = app.TriangleCount(16, 0, 0)
    tc.set_up_runtime()
    tc.load_and_format_matrix(raw, True)
    tc.send_matrix_host_to_device()
    n = tc.n_
    plan = tc.SpMV_.plan_
    total, per = capi.DeviceBuffer(8), capi.DeviceBuffer(8 * n)
    plan.tc_count(total)                      # (the plan's first call: the verdict and the bins)
    capi.sync()
    total_ms = span_ms(lambda: plan.tc_count(total), runs)
    per_ms = span_ms(lambda: plan.tc_count(total, per), runs)
    for _ in range(3):
        t = tc.run()
    ts = []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        t = tc.run()
        ts.append(time.perf_counter() - t0)
    assert int(total.read(np.uint64, 1)[0]) == tc.num_triangles_ and np.array_equal(per.read(np.uint64, n), t)
    assert int(t.sum()) == 3 * tc.num_triangles_ and tc.run(per_vertex=False) == tc.num_triangles_
    rec = {"graph": name, "n": n, "nnz": raw.nnz, "oriented_entries": oriented.nnz, "triangles": tc.num_triangles_,
           "transitivity": tc.transitivity_, "longest_oriented_row": int(lens.max()), "longest_undirected_row": int(deg.max()),
           "two_hop_entries": two_hop, "total_ms": round(total_ms, 4), "per_vertex_ms": round(per_ms, 4),
           "two_hop_per_s": round(two_hop / (total_ms * 1e-3), 1) if total_ms > 0 else None,
           "run_ms": round(float(np.median(ts)) * 1e3, 4), "prepare_s": round(prepare_s, 3),
           "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    if two_hop <= scipy_limit:
        want, s = scipy_total(oriented)
        rec["scipy_ms"] = round(s * 1e3, 2)
        assert want == tc.num_triangles_, "%s: %d triangles, scipy counts %d" % (name, tc.num_triangles_, want)
    else:
        rec["scipy_ms"] = None                # not measured
    if verify:
        rec["verified"] = app.validate_triangles(padded, t) == tc.num_triangles_
    return rec


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tc.jsonl"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scipy-limit", type=float, default=2e8, help="two-hop entries above which the host product is not run")
    ap.add_argument("--verify", action="store_true", help="check the per-vertex counts with app.validate_triangles")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        rec = run_graph(name, raw, runs=args.runs, verify=args.verify, scipy_limit=args.scipy_limit)
        rec["scale"] = args.scale
        rec["data"] = "synthetic stand-in"
        print(json.dumps(rec), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
