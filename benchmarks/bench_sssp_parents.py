#!/usr/bin/env python
"""The shortest-path predecessor tree (SSSP.parents / gl_sssp_parents) on the graphs benchmarks/bench_graphs.py uses, with seeded
weights, one GPU.

Per graph one JSON line:
  pull_iteration_ms   one weighted (min,+) SpMV of the pull loop by HIP events (median of `runs` spans): the yardstick
  pull_push_ms        the weighted search, wall time (median of `runs`), `iters` iterations
  parents_kernel_ms   the tree pass alone by HIP events (fill + column scatter + finish pass; median of `runs` spans)
  parents_ms          SSSP.parents() end to end: the pass, the device synchronisation and the 4 n-byte read-back
  entries_read        column entries the pass read (gl_sssp_parents_entries) against the matrix' nnz: every entry of a reached column
  stream_gbps         8 bytes per entry read / parents_kernel_ms
  variants            --ab: the pass's GPU time with one launch parameter changed at a time (GRAPHLILY_DEBUG knobs, read per call)
The tree is compared with the numpy definition by the tests; here --validate runs app.validate_sssp_tree (minutes of numpy on the
large graphs).

    python benchmarks/bench_sssp_parents.py [--graphs orkut] [--iters 24] [--ab] [--out profiles/sssp_parents.jsonl]
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

from bench_bfs_parents import with_knobs  # noqa: E402

VARIANTS = [("default", {}), ("cut_0", {"sssp_parents_cut": 0}), ("cut_16", {"sssp_parents_cut": 16}), ("cut_64", {"sssp_parents_cut": 64}),
            ("cut_256", {"sssp_parents_cut": 256}), ("thread_per_column", {"sssp_parents_cut": 1 << 30}),
            ("grid_16", {"sssp_parents_grid": 16}), ("grid_256", {"sssp_parents_grid": 256})]


def kernel_ms(plan, dist, unreached, source, parent, runs, knobs=None):
    """Median GPU time of one gl_sssp_parents call (HIP events on the library's stream) after three untimed ones."""
    from graphlily_amd import capi

    def once():
        capi.span_begin()
        plan.sssp_parents(dist, unreached, source, parent, None)
        return capi.span_end()

    def series():
        for _ in range(3):
            once()
        return float(np.median([once() for _ in range(runs)]))
    return with_knobs(knobs or {}, series)


def pull_iteration_ms(sssp, dist, runs):
    """Median GPU time of one (min,+) SpMV on the converged distances (the pull loop's step, without its buffer swap)."""
    from graphlily_amd import capi
    out = sssp.backend.alloc(sssp.n_, np.float32)
    sssp.SpMV_.bind_vector_buf(dist)
    sssp.SpMV_.bind_results_buf(out)

    def once():
        capi.span_begin()
        sssp.SpMV_.run()
        return capi.span_end()
    for _ in range(3):
        once()
    return float(np.median([once() for _ in range(runs)]))


def run_graph(name, raw, iters, seed=1, runs=9, ab=False, validate=False):
    from graphlily_amd import app, capi, io, module as M
    raw.adj_data = np.random.default_rng(seed).integers(1, 9, size=raw.nnz).astype(np.float32)
    deg = np.diff(raw.adj_indptr.astype(np.int64))
    src = 0 if deg[0] > 0 else int(np.argmax(deg > 0))
    sssp = app.SSSP(16, 0, 0, 0, semiring=M.TropicalSemiring)
    sssp.set_up_runtime()
    sssp.load_and_format_matrix(raw, True, weighted=True)
    sssp.send_matrix_host_to_device()
    n, nnz = sssp.n_, sssp.get_nnz()
    unreached = sssp.semiring_.zero
    for _ in range(2):
        d = sssp.pull_push(src, iters, 0.05)
    ts = []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        d = sssp.pull_push(src, iters, 0.05)
        ts.append(time.perf_counter() - t0)
    t_pp = float(np.median(ts))
    for _ in range(3):
        p = sssp.parents()
    ts = []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        p = sssp.parents()
        ts.append(time.perf_counter() - t0)
    t_par = float(np.median(ts))
    orphans = sssp.orphans_
    plan = sssp.SpMSpV_.plan_
    dist = capi.DeviceBuffer.from_host(d)
    parent = capi.DeviceBuffer(4 * n)
    k_ms = kernel_ms(plan, dist, unreached, src, parent, runs)
    read = plan.sssp_parents_entries(dist, unreached, src, parent)
    assert np.array_equal(parent.read(np.uint32, n), p)
    it_ms = pull_iteration_ms(sssp, dist, runs)
    reached = d < np.float32(unreached)
    rec = {"graph": name, "n": n, "nnz": nnz, "iters": iters, "source": src, "weights": "integers 1..8, seed %d" % seed,
           "reached": int(reached.sum()), "orphans": orphans, "push_iterations": sssp.push_iterations_,
           "pull_iteration_ms": round(it_ms, 4), "pull_push_ms": round(t_pp * 1e3, 4), "parents_kernel_ms": round(k_ms, 4),
           "parents_ms": round(t_par * 1e3, 4), "parents_kernel_over_pull_iteration": round(k_ms / it_ms, 3),
           "entries_read": int(read), "entries_read_frac": round(read / max(nnz, 1), 4),
           "stream_gbps": round(8.0 * read / (k_ms * 1e-3) / 1e9, 1)}
    if ab:
        # every variant twice, interleaved with the default, so that drift shows as a spread of the default's figures
        rec["variants"] = {}
        for rep in range(2):
            for label, knobs in VARIANTS:
                rec["variants"].setdefault(label, []).append(round(kernel_ms(plan, dist, unreached, src, parent, runs, knobs), 4))
                assert np.array_equal(parent.read(np.uint32, n), p), label
    if validate:
        m = raw.copy()
        io.sssp_zero_diagonal(m)
        # (an unfinished run has orphans, which the validator reports under rule 2: nothing to validate then)
        rec["validated"] = app.validate_sssp_tree(m, src, d, p, unreached) == int(reached.sum()) if orphans == 0 else None
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="orkut")
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ab", action="store_true", help="also time the pass with one launch parameter changed at a time")
    ap.add_argument("--validate", action="store_true")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi, datasets
    dev = torch.device("cuda:0")
    capi.init(0)
    lines = []
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, 1.0, device=dev)
        rec = run_graph(name, raw, args.iters, seed=args.seed, runs=args.runs, ab=args.ab, validate=args.validate)
        rec["data"] = "synthetic stand-in"
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if args.out:
            with open(args.out, "w") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
