#!/usr/bin/env python
"""Delta-stepping shortest paths (gl_sssp_delta, app.ShortestPaths) against the Bellman-Ford driver (app.SSSP, weighted), one GPU,
one process.

Graphs: the six stand-ins at --scale (1/8) with seeded integer weights out of 255 values, and a k x k grid with seeded weights, the
high-diameter case.  The source is the vertex with the longest row.  Per graph:
  one line per delta in {default / 8, default, 8 x default, inf}: run_ms = ShortestPaths.run(source, delta, parents=False), wall
      clock (the call synchronises itself), median of `runs` with run_ms_min / run_ms_max, and reached, buckets, rounds,
      relaxations, launches of the last run; parents_ms on the default line: the same with the parent pass
  the default line also carries SSSP(weighted=True).pull_push given the iteration count it NEEDS -- found by doubling from
      rounds_ until its distances equal ShortestPaths' on the reached vertices, to the bit -- as bf_ms / bf_ms_min / bf_ms_max and
      bf_iterations; the two drivers are timed ALTERNATING, one run each, in this process.  bf_over_delta = bf_ms / run_ms
  verified: the distances and parents passed app.validate_shortest_paths (a host Dijkstra in f32) before any time is reported
      (skipped above --validate-below entries: the host loop is Python)
--ab adds one short line per knob value ("ab": "sssp_delta_cut=0"), at the default delta on the same plans.

    python benchmarks/bench_sssp_delta.py [--graphs googleplus,grid] [--scale 0.125] [--grid 512] [--ab] [--out profiles/sssp_delta.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from bench_truss import _with_knob  # noqa: E402

AB = [("sssp_delta_cut", v) for v in (0, 4, 8, 16, 32)] + [("sssp_delta_grid", v) for v in (1, 2, 4, 8, 16)] + \
     [("sssp_delta_batch", v) for v in (1, 4, 16, 64, 256)]


def grid_graph(k, seed):
    from graphlily_amd import io
    at = np.arange(k * k, dtype=np.int64).reshape(k, k)
    a = np.concatenate([at[:, :-1].ravel(), at[:-1, :].ravel()])
    b = np.concatenate([at[:, 1:].ravel(), at[1:, :].ravel()])
    key = np.sort(np.concatenate([a * k * k + b, b * k * k + a]))
    indptr = np.zeros(k * k + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // (k * k), minlength=k * k), out=indptr[1:])
    w = np.random.default_rng(seed).integers(1, 256, size=key.size).astype(np.float32)
    return io.CSRMatrix(k * k, k * k, w, (key % (k * k)).astype(np.uint32), indptr.astype(np.uint32))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(ms, key):
    return {key: round(statistics.median(ms), 4), key + "_min": round(min(ms), 4), key + "_max": round(max(ms), 4)}


def run_graph(name, m, runs, ab, validate_below):
    from graphlily_amd import app, module as M
    sp = app.ShortestPaths(M.num_hbm_channels, 0, 0)
    sp.set_target("hw")
    sp.set_up_runtime("unused.xclbin")
    sp.load_and_format_matrix(m.copy(), True, True)
    sp.send_matrix_host_to_device()
    source = int(np.argmax(np.diff(sp.graph_out_.adj_indptr.astype(np.int64))))
    default = sp.default_delta()
    want = sp.run(source).copy()
    verified = None
    if m.nnz <= validate_below:
        app.validate_shortest_paths(m, source, sp.dist_, sp.parent_)
        verified = True
    base = {"graph": name, "n": sp.n_, "n_real": sp.n_real_, "edges": sp.graph_.nnz, "source": source, "default_delta": float(default),
            "orphans": sp.orphans_, "verified": verified, "runs": runs, "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    bf = app.SSSP(M.num_hbm_channels, 0, 0, 0)
    bf.set_target("hw")
    bf.set_up_runtime("unused.xclbin")
    bf.load_and_format_matrix(m.copy(), True, weighted=True)
    bf.send_matrix_host_to_device()
    iters = max(2, int(sp.rounds_))
    while True:                                                      # the count Bellman-Ford needs, with a host check
        got = bf.pull_push(source, iters)
        got = np.where(got >= np.float32(M.FLOAT_INF), np.float32(np.inf), got)
        if np.array_equal(got.view(np.uint32), want.view(np.uint32)) or iters > 4 * sp.n_:
            break
        iters *= 2
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: Bellman-Ford and delta-stepping disagree" % name
    for label, delta in (("default/8", default / 8), ("default", default), ("8*default", default * 8), ("inf", np.float32(np.inf))):
        sp.run(source, delta, parents=False)
        assert np.array_equal(sp.dist_.view(np.uint32), want.view(np.uint32)), "%s: delta %s changes the distances" % (name, label)
        ms, bf_ms = [], []
        for _ in range(runs):                                        # alternating, one run each
            ms.append(timed(lambda: sp.run(source, delta, parents=False)))
            if label == "default":
                bf_ms.append(timed(lambda: bf.pull_push(source, iters)))
        rec = dict(base, delta=label, delta_value=float(delta), reached=sp.reached_, buckets=sp.buckets_, rounds=sp.rounds_,
                   relaxations=sp.relaxations_, launches=sp.launches_, **spread(ms, "run_ms"))
        if label == "default":
            rec.update(spread(bf_ms, "bf_ms"), bf_iterations=iters, bf_over_delta=round(statistics.median(bf_ms) / statistics.median(ms), 3),
                       **spread([timed(lambda: sp.run(source, delta)) for _ in range(runs)], "parents_ms"))
        yield rec
    for key, value in AB if ab else ():
        ms = _with_knob(key, value, lambda: (sp.run(source, default, parents=False), [timed(lambda: sp.run(source, default, parents=False)) for _ in range(runs)])[1])
        assert np.array_equal(sp.dist_.view(np.uint32), want.view(np.uint32))
        yield dict({"graph": name, "ab": "%s=%d" % (key, value), "delta": "default", "rounds": sp.rounds_, "launches": sp.launches_, "runs": runs},
                   **spread(ms, "run_ms"))


def main():
    from graphlily_amd import datasets
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(list(datasets.PAPER_GRAPHS) + ["grid"]))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--grid", type=int, default=512, help="side of the grid")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sssp_delta.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plans")
    ap.add_argument("--validate-below", type=int, default=1200000, help="entries up to which the host Dijkstra checks the result")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi, io
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in [g for g in args.graphs.split(",") if g]:
        if name == "grid":
            m, scale = grid_graph(args.grid, 5), 1.0
        else:
            raw, scale = datasets.paper_graph(name, args.scale, device=dev), args.scale
            w = np.random.default_rng(4).integers(1, 256, size=raw.nnz).astype(np.float32)
            m = io.CSRMatrix(raw.num_rows, raw.num_cols, w, raw.adj_indices, raw.adj_indptr)
        for rec in run_graph(name, m, args.runs, args.ab, args.validate_below):
            rec.update(scale=scale, data="synthetic stand-in" if name != "grid" else "grid %d x %d" % (args.grid, args.grid))
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
