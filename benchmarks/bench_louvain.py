#!/usr/bin/env python
"""Louvain communities (gl_louvain_move under app.Louvain) on the six stand-ins and on orkut_community, one GPU.

Per graph one JSON line for app.Louvain.run() under gl_color's largest-first colourings:
  run_ms           the whole run() (it waits for the device), wall clock: median of `runs` after one untimed run, which is
                   reported as first_run_ms (verdicts, scratch); run_ms_min / run_ms_max: the spread
  move_ms, color_ms, aggregate_ms, plan_ms
                   the split of the median run (Louvain.timings_): gl_louvain_move with its uploads and the read-back of the
                   labels; gl_color with its read-back; io.aggregate_communities and the relabelling on the host; building the
                   later levels' plans.  aggregate_share = aggregate_ms / run_ms: what a device-side aggregation could win
  levels, level_sizes, level_colors, level_sweeps, level_moves, launches
                   accepted levels, and per level run (a discarded last one included) vertices, classes, sweeps and moves
  communities, largest_community, modularity
                   over the real vertices; Newman's modularity on the host (app.Louvain.modularity)
  lpa_ms, lpa_sweeps, lpa_modularity, lpa_communities
                   gl_lpa on the same plan under the same level-0 colouring: time per call and what it finds
  move0_ms, move0_sweeps, move0_over_lpa
                   gl_louvain_move alone on level 0 (the call the driver's first level makes) next to gl_lpa on the same plan
  purity           orkut_community only: the share of the real vertices whose planted community is the most frequent one
                   among the vertices carrying their label (a reported figure, not a bar)
  networkx_ms, networkx_modularity
                   networkx.algorithms.community.louvain_communities(seed=0) on the host, only for graphs of at most
                   --networkx-entries symmetric entries (a size networkx finishes); the line "rmat_20K" always has it
--ab adds one short line per knob value ("ab": "louvain_table=512", move0_ms), timed on level 0 of the same plan in the same
process right behind the default line (the knobs are read per call): louvain_cut 0 / 4 / 8, louvain_grid 4 / 8 / 16,
louvain_batch 1 / 4 / 16, louvain_table 512 / 1024 / 2048.

    python benchmarks/bench_louvain.py [--graphs googleplus,orkut_community] [--scale 0.125] [--ab] [--out profiles/louvain.jsonl]
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

from bench_kcore import wall_ms  # noqa: E402
from bench_lpa import planted_communities, purity_of  # noqa: E402
from bench_truss import _with_knob  # noqa: E402

LOUVAIN_CUT, LOUVAIN_GRID, LOUVAIN_BATCH, LOUVAIN_TABLE = 8, 8, 4, 2048           # the library's defaults (csrc/gl_louvain.hip)

AB = [("louvain_cut", v) for v in (0, 4, 8)] + [("louvain_grid", v) for v in (4, 8, 16)] + [("louvain_batch", v) for v in (1, 4, 16)] + \
     [("louvain_table", v) for v in (512, 1024, 2048)]


def networkx_louvain(sym):
    import networkx as nx
    import scipy.sparse as sp
    A = sp.csr_matrix((np.ones(sym.nnz, np.float32), sym.adj_indices.astype(np.int64), sym.adj_indptr.astype(np.int64)), shape=(sym.num_rows, sym.num_rows))
    G = nx.from_scipy_sparse_array(A)
    t0 = time.perf_counter()
    parts = nx.algorithms.community.louvain_communities(G, weight=None, seed=0)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, float(nx.algorithms.community.modularity(G, parts, weight=None))


def run_graph(name, raw, runs=3, ab=False, planted=None, networkx_entries=0, tol=1e-7, max_sweeps=100):
    from graphlily_amd import app, capi, module as M
    d = app.Louvain(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    t0 = time.perf_counter()
    d.load_and_format_matrix(raw, True)
    d.send_matrix_host_to_device()
    prepare_s = time.perf_counter() - t0
    sym, deg, n, n_real = d.graph_, d.degrees_, d.n_, d.n_real_
    capi.sync()
    t0 = time.perf_counter()
    got = d.run(tol=tol, max_sweeps=max_sweeps)
    first_run_ms = (time.perf_counter() - t0) * 1e3
    print("%s: %d levels, sizes %s, sweeps %s, modularity %.4f" % (name, d.levels_, d.level_sizes_.tolist(), d.level_sweeps_.tolist(), d.modularity()),
          file=sys.stderr, flush=True)
    times, splits = [], []
    for _ in range(runs):
        capi.sync()
        t0 = time.perf_counter()
        again = d.run(tol=tol, max_sweeps=max_sweeps)
        times.append((time.perf_counter() - t0) * 1e3)
        splits.append(dict(d.timings_))
        assert np.array_equal(again, got)
    mid = int(np.argsort(times)[len(times) // 2])
    split = splits[mid]
    sizes = d.community_sizes_
    # level 0 alone, next to gl_lpa on the same plan under the same colouring
    plan = d.SpMV_.plan_
    color = capi.DeviceBuffer.from_host(np.ascontiguousarray(d.level_colorings_[0], np.uint32))
    label = capi.DeviceBuffer(4 * max(1, n))
    two_m = int(deg.astype(np.int64).sum())
    min_gain = int(np.floor(tol * float(two_m * two_m)))
    move_stats = plan.louvain_move(label, color, None, None, max_sweeps, min_gain)
    move0_ms = wall_ms(lambda: plan.louvain_move(label, color, None, None, max_sweeps, min_gain), runs)
    move0_labels = label.read(np.uint32, n)
    lpa_stats = plan.lpa(label, color, None, 100)
    lpa_ms = wall_ms(lambda: plan.lpa(label, color, None, 100), runs)
    lpa_labels = label.read(np.uint32, n)
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    rec = {"graph": name, "n": n, "nnz": raw.nnz, "symmetric_entries": sym.nnz, "longest_row": int(deg.max()) if n else 0,
           "levels": d.levels_, "level_sizes": d.level_sizes_.tolist(), "level_colors": d.level_colors_.tolist(),
           "level_sweeps": d.level_sweeps_.tolist(), "level_moves": d.level_moves_.tolist(), "launches": d.launches_,
           "communities": d.num_communities_, "largest_community": int(sizes.max()), "modularity": round(d.modularity(), 6),
           "run_ms": round(times[mid], 3), "run_ms_min": round(min(times), 3), "run_ms_max": round(max(times), 3), "first_run_ms": round(first_run_ms, 3),
           "move_ms": round(split["move"] * 1e3, 3), "color_ms": round(split["color"] * 1e3, 3), "aggregate_ms": round(split["aggregate"] * 1e3, 3),
           "plan_ms": round(split["plan"] * 1e3, 3), "aggregate_share": round(split["aggregate"] * 1e3 / times[mid], 3),
           "move0_ms": round(move0_ms[0], 4), "move0_ms_min": round(move0_ms[1], 4), "move0_ms_max": round(move0_ms[2], 4),
           "move0_sweeps": move_stats[0], "move0_moves": move_stats[1], "move0_launches": move_stats[3],
           "lpa_ms": round(lpa_ms[0], 4), "lpa_sweeps": lpa_stats[0], "lpa_modularity": round(d.modularity(lpa_labels), 6),
           "lpa_communities": int(np.unique(lpa_labels[:n_real]).shape[0]), "move0_over_lpa": round(move0_ms[0] / lpa_ms[0], 3) if lpa_ms[0] > 0 else None,
           "runs": runs, "prepare_s": round(prepare_s, 3), "tol": tol,
           "louvain_cut": int(knobs.get("louvain_cut", LOUVAIN_CUT)), "louvain_grid": int(knobs.get("louvain_grid", LOUVAIN_GRID)),
           "louvain_batch": int(knobs.get("louvain_batch", LOUVAIN_BATCH)), "louvain_table": int(knobs.get("louvain_table", LOUVAIN_TABLE)),
           "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    if planted is not None:
        rec["purity"] = round(purity_of(got[:n_real], planted[:n_real]), 4)
        rec["lpa_purity"] = round(purity_of(lpa_labels[:n_real], planted[:n_real]), 4)
        rec["planted_communities"] = int(planted.max()) + 1
    if sym.nnz <= networkx_entries:
        ms, q = networkx_louvain(sym)
        rec["networkx_ms"], rec["networkx_modularity"] = round(ms, 1), round(q, 6)
    yield rec
    for key, value in AB if ab else ():
        res = _with_knob(key, value, lambda: (plan.louvain_move(label, color, None, None, max_sweeps, min_gain),
                                              wall_ms(lambda: plan.louvain_move(label, color, None, None, max_sweeps, min_gain), runs)))
        assert res[0][:3] + res[0][4:] == move_stats[:3] + move_stats[4:] and np.array_equal(label.read(np.uint32, n), move0_labels)
        yield {"graph": name, "ab": "%s=%d" % (key, value), "move0_ms": round(res[1][0], 4), "move0_ms_min": round(res[1][1], 4),
               "move0_ms_max": round(res[1][2], 4), "launches": res[0][3], "sweeps": move_stats[0], "runs": runs,
               "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(["rmat_20K"] + list(datasets.PAPER_GRAPHS) + ["orkut_community"]))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "louvain.jsonl"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-sweeps", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-7)
    ap.add_argument("--networkx-entries", type=int, default=1000000, help="run networkx's Louvain on graphs of at most so many symmetric entries")
    ap.add_argument("--ab", action="store_true", help="also time every knob value on level 0 of the same plan")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        if name == "rmat_20K":
            raw = datasets.rmat(20000, 400000, seed=11, symmetric=False)
        else:
            raw = datasets.paper_graph(name, args.scale, device=dev)
        planted = None
        if name == "orkut_community":
            planted = planted_communities(raw.num_rows, datasets.EXTRA_GRAPHS[name]["seed"])
        for rec in run_graph(name, raw, runs=args.runs, ab=args.ab, planted=planted, networkx_entries=args.networkx_entries, tol=args.tol,
                             max_sweeps=args.max_sweeps):
            rec["scale"] = args.scale if name != "rmat_20K" else 1.0
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
