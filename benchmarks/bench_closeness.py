#!/usr/bin/env python
"""Bit-parallel multi-source BFS (gl_msbfs) on the six stand-ins and orkut_community, one GPU, one process.

Every stand-in is loaded as app.BetweennessCentrality loads it (io.simple_pattern; a symmetric pattern is one plan), so that the
sweep and the yardstick run in the same process on the SAME plan.  Per graph and source count (64 and 256 random real vertices
with an edge, numpy.random.default_rng(29)) one JSON line:
  call_ms            all the sources through gl_msbfs in batches of 64, accumulating from the second on (each call synchronises
                     itself), wall clock: median of `runs` after three untimed runs, with call_ms_min / call_ms_max; hops_ms: the
                     same with d_hops, k n more words to write
  levels, launches   summed over the batches; ms_per_level = call_ms / levels; entries_levels_per_s = entries x levels / call_ms,
                     an UPPER bound on the entries read, since rows that have met all their sources are skipped
  full               vertices that met all 64 sources of the last batch
  bfs_ms             app.BFS.pull_push(s, N) once per source for the same sources -- the parent commit's only way to these
                     distances -- summed (median of `runs` per source after one untimed call), bfs_ms_per_source, and
                     bfs_over_msbfs = bfs_ms / call_ms: above 1 the batched sweep is faster
  verified           --verify: far, reach and harmonic of the first eight sources equal app.validate_closeness's host recomputation;
                     always: the hop rows of four sources equal pull_push's levels, before any time is reported
--ab adds one short line per knob value ("ab": "msbfs_cut=0"), timed on the same plan right behind the default line: msbfs_cut
0 / 4 / 8 / 16 / 32, msbfs_grid 1 / 2 / 4 / 8 / 16, msbfs_batch 1 / 4 / 8 / 16 / 32 / 64.

    python benchmarks/bench_closeness.py [--graphs googleplus,orkut_community] [--scale 0.125] [--ab] [--out profiles/closeness.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from bench_bc import timed_ms  # noqa: E402
from bench_kcore import wall_ms  # noqa: E402
from bench_truss import _with_knob  # noqa: E402

MSBFS_CUT, MSBFS_GRID, MSBFS_BATCH = 8, 4, 16       # the library's defaults (csrc/gl_msbfs.hip)
AB = [("msbfs_cut", v) for v in (0, 4, 8, 16, 32)] + [("msbfs_grid", v) for v in (1, 2, 4, 8, 16)] + \
     [("msbfs_batch", v) for v in (1, 4, 8, 16, 32, 64)]
COUNTS = (64, 256)


def run_graph(name, raw, runs, ab, verify):
    from graphlily_amd import app, capi
    d = app.BetweennessCentrality(16, 0, 0, 0)
    d.set_up_runtime()
    d.load_and_format_matrix(raw, True)
    d.send_matrix_host_to_device()
    n, plan, bfs = d.n_, d.SpMV_.plan_, d.bfs_
    entries = d.SpMV_.get_nnz()
    deg_in = np.diff(d.SpMV_.csr_matrix_.adj_indptr.astype(np.int64))
    rng = np.random.default_rng(29)
    live = np.flatnonzero(deg_in[:d.n_real_] > 0)
    far, harmonic, reach = capi.DeviceBuffer(8 * n), capi.DeviceBuffer(8 * n), capi.DeviceBuffer(4 * n)
    hops = capi.DeviceBuffer(4 * 64 * n)
    for count in COUNTS:
        sources = [int(s) for s in rng.choice(live, min(count, live.size), replace=False)]
        batches = [sources[b:b + 64] for b in range(0, len(sources), 64)]

        def sweep(want_hops=False):
            levels = launches = full = 0
            for i, part in enumerate(batches):
                _, stats = plan.msbfs(part, far, reach, harmonic, i > 0, hops if want_hops else None)
                levels, launches, full = levels + stats[0], launches + stats[2], stats[1]
            return levels, launches, full

        levels, launches, full = sweep(True)
        deepest = max(plan.msbfs(part, far, reach, harmonic, False)[1][0] for part in batches)
        N = 16                                # (BetweennessCentrality's rule: 16, doubled while a search may be truncated)
        while deepest + 1 >= N + 1 and N < n:
            N = min(2 * N, n)
        rows = hops.read(np.uint32, len(batches[-1]) * n).reshape(len(batches[-1]), n)
        for j, s in enumerate(batches[-1][:4]):                      # the yardstick computes the same distances
            level = np.array(bfs.pull_push(s, N)).astype(np.int64)
            assert np.array_equal(np.where(level > 0, level - 1, 0xFFFFFFFF), rows[j].astype(np.int64)), "%s: hops differ from pull_push's levels" % name
        if verify and count == COUNTS[0]:                            # (eight host searches: the larger stand-ins take seconds each)
            plan.msbfs(sources[:8], far, reach, harmonic, False)
            app.validate_closeness(raw, far.read(np.uint64, n), reach.read(np.uint32, n), harmonic.read(np.float64, n), sources[:8],
                                   directed=d.directed_)
        sweep()
        print("%s/%d: %d levels, %d launches, N = %d" % (name, len(sources), levels, launches, N), file=sys.stderr, flush=True)
        call_ms = wall_ms(sweep, runs)
        hops_ms = wall_ms(lambda: sweep(True), runs)
        t_bfs = []
        for s in sources:
            bfs.pull_push(s, N)
            t_bfs.append(timed_ms(lambda: bfs.pull_push(s, N), runs))
        bfs_ms = float(np.sum(t_bfs))
        knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
        yield {"graph": name, "n": n, "n_real": d.n_real_, "entries": entries, "directed": bool(d.directed_), "longest_row": int(deg_in.max()),
               "sources": len(sources), "batches": len(batches), "levels": levels, "deepest": deepest, "launches": launches, "full": full,
               "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
               "hops_ms": round(hops_ms[0], 4), "hops_ms_min": round(hops_ms[1], 4), "hops_ms_max": round(hops_ms[2], 4),
               "ms_per_level": round(call_ms[0] / max(1, levels), 5), "ms_per_source": round(call_ms[0] / len(sources), 5),
               "entries_levels_per_s": round(entries * levels / (call_ms[0] * 1e-3)) if call_ms[0] > 0 else None,
               "bfs_iterations": N, "bfs_ms": round(bfs_ms, 4), "bfs_ms_per_source": round(bfs_ms / len(sources), 5),
               "bfs_ms_per_source_min": round(float(np.min(t_bfs)), 5), "bfs_ms_per_source_max": round(float(np.max(t_bfs)), 5),
               "bfs_over_msbfs": round(bfs_ms / call_ms[0], 3) if call_ms[0] > 0 else None,
               "bfs_over_msbfs_with_hops": round(bfs_ms / hops_ms[0], 3) if hops_ms[0] > 0 else None,
               "verified": bool(verify), "runs": runs, "msbfs_cut": int(knobs.get("msbfs_cut", MSBFS_CUT)),
               "msbfs_grid": int(knobs.get("msbfs_grid", MSBFS_GRID)), "msbfs_batch": int(knobs.get("msbfs_batch", MSBFS_BATCH)),
               "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
        for key, value in AB if ab and count == COUNTS[0] else ():
            res = _with_knob(key, value, lambda: (sweep(), wall_ms(sweep, runs)))
            assert res[0][0] == levels and res[0][2] == full
            yield {"graph": name, "sources": len(sources), "ab": "%s=%d" % (key, value), "call_ms": round(res[1][0], 4),
                   "call_ms_min": round(res[1][1], 4), "call_ms_max": round(res[1][2], 4), "levels": levels, "launches": res[0][1],
                   "runs": runs, "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(list(datasets.PAPER_GRAPHS) + ["orkut_community"]))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closeness.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plan (64 sources)")
    ap.add_argument("--verify", action="store_true", help="check far, reach and harmonic of eight sources against host searches")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in [g for g in args.graphs.split(",") if g]:
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, args.runs, args.ab, args.verify):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
