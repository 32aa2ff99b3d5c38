#!/usr/bin/env python
"""PageRank.solve against PageRank.pull on the graphs benchmarks/bench_graphs.py uses, one GPU, one process.

Per graph one JSON line, appended to --out:
  pull_iteration_ms    PageRank.pull per iteration: (wall time of 2 N iterations - wall time of N) / N, medians of `runs` -- the
                       chained SpMV with the teleport term folded in, one launch per iteration
  solve_iteration_ms   PageRank.solve per iteration, the same way with tol = 0: SpMV with its helper launch, gl_pagerank_update
                       and its one-workgroup finish, a 4-byte read-back every check_every iterations.  tol = 0 still stops a
                       run whose float32 iteration reaches its fixed point exactly (r == 0), after which the launches are the
                       cheap frozen copies: every timed run is checked to have run all its iterations unconverged
  solve_over_pull      the ratio of the two
  update_ms            gl_pagerank_update alone by HIP events (median of `runs` spans), and update_gbps = (16 n + n / 8) bytes / that
  iterations_to_tol    iterations solve needs for tol (default 1e-6), `converged`, and the last residual
  check_every          wall time in ms of the whole solve to tol (read-back of the ranks included) for check_every in 1, 2, 4, 8,
                       every value twice, interleaved, so that drift shows as the spread of a value's two figures
  mass_pull / mass_solve   the sum of the returned ranks: pull lets the dangling vertices' rank drain away

    python benchmarks/bench_pagerank_solve.py [--graphs orkut] [--tol 1e-6] [--out profiles/pagerank_solve.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DAMPING = 0.85
SWEEP = [1, 2, 4, 8]


def wall_ms(fn, runs):
    from graphlily_amd import capi
    fn()
    ts = []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def update_ms(n, runs):
    """Median GPU time of one gl_pagerank_update (the pass and its finish launch) on vectors of the graph's size"""
    from graphlily_amd import capi
    rng = np.random.default_rng(0)
    x, y, p = (capi.DeviceBuffer.from_host(rng.random(n, dtype=np.float32)) for _ in range(3))
    bits = capi.DeviceBuffer.from_host(rng.integers(0, 1 << 32, size=(n + 31) // 32, dtype=np.uint64).astype(np.uint32))
    ctl = capi.DeviceBuffer(capi.pagerank_ctl_bytes(1))
    capi.pagerank_begin(p, n, bits, x, ctl, 1)

    def once():
        capi.span_begin()
        capi.pagerank_update(y, x, p, bits, n, DAMPING, 0.0, ctl, 1)
        return capi.span_end()
    for _ in range(3):
        once()
    return float(np.median([once() for _ in range(runs)]))


def run_graph(name, raw, tol, runs=7, base=20):
    from graphlily_amd import app
    pr = app.PageRank(16, 0, 0)
    pr.set_up_runtime()
    pr.load_and_format_matrix(raw, DAMPING)
    pr.send_matrix_host_to_device()
    n, nnz = pr.n_, pr.get_nnz()
    pulled = pr.pull(DAMPING, base)
    t_pull = (wall_ms(lambda: pr.pull(DAMPING, 2 * base), runs) - wall_ms(lambda: pr.pull(DAMPING, base), runs)) / base
    solved = pr.solve(DAMPING, tol, 200)          # (also builds the dangling bits, once per load)
    iterations, converged, last = pr.iterations_, pr.converged_, float(pr.residuals_[-1])

    def solve_all(iterations_asked):
        pr.solve(DAMPING, 0.0, iterations_asked)
        if pr.iterations_ != iterations_asked or pr.converged_:
            raise RuntimeError("%s: solve(tol = 0, %d iterations) stopped after %d (r == 0): the slope would time frozen copies"
                               % (name, iterations_asked, pr.iterations_))
    t_solve = (wall_ms(lambda: solve_all(2 * base), runs) - wall_ms(lambda: solve_all(base), runs)) / base
    sweep = {}
    for rep in range(2):
        for ce in SWEEP:
            sweep.setdefault(str(ce), []).append(round(wall_ms(lambda: pr.solve(DAMPING, tol, 200, check_every=ce), runs), 4))
            assert pr.iterations_ == iterations
    u_ms = update_ms(n, runs)
    dangling = int(np.unpackbits(pr._dangling_bits().view(np.uint8), bitorder="little")[:n].sum())
    return {"graph": name, "n": n, "n_real": pr.n_real_, "nnz": nnz, "damping": DAMPING, "dangling": dangling,
            "pull_iteration_ms": round(t_pull, 4), "solve_iteration_ms": round(t_solve, 4),
            "slope_iterations": [base, 2 * base], "solve_over_pull": round(t_solve / t_pull, 3),
            "update_ms": round(u_ms, 4), "update_gbps": round((16.0 * n + n / 8.0) / (u_ms * 1e-3) / 1e9, 1),
            "tol": tol, "iterations_to_tol": iterations, "converged": converged, "last_residual": last,
            "check_every": sweep, "check_every_default": 4,
            "mass_pull": float(pulled.astype(np.float64).sum()), "mass_solve": float(solved.astype(np.float64).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="orkut")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pagerank_solve.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--scale", type=float, default=1.0, help="size of the stand-in relative to the published graph")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi, datasets
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        rec = run_graph(name, raw, args.tol, runs=args.runs)
        rec["data"] = "synthetic stand-in" + ("" if args.scale == 1.0 else " at scale %g" % args.scale)
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
