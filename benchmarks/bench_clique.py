#!/usr/bin/env python
"""k-clique counting (CliqueCount / gl_clique_count) on the six stand-ins and orkut_community, one GPU, one process.

Every stand-in is oriented twice -- by the degree rank (io.triangle_orient's order) and by the degeneracy rank (positions in
gl_kcore's peeling order) -- and per orientation one JSON line:
  k3_ms, k4_ms, k5_ms      gl_clique_count without per-vertex counts, by HIP events on the library's stream: median of `runs`
                           after three untimed runs, with min and max (k*_min_ms, k*_max_ms: the run's own spread)
  k3_per_vertex_ms ...     the same with per-vertex counts
  tc_ms                    gl_tc_count on the SAME plan in the same process, total only; k3_over_tc = k3_ms / tc_ms (above 1 the
                           bit-matrix kernel is slower) -- the yardstick; the two totals are asserted equal before a time is reported
  build_ms, build_share    the call with clique_build_only=1 (staging and matrix building, nothing counted) and its share of k3_ms
  cliques                  {k: count}; longest_row, rows per bin, launches
--ab adds, behind each line, one line per knob value (clique_tiny, clique_mid, clique_lds, clique_grid, clique_waves) on a fresh
plan of the same matrix ("ab": "key=value").  --verify checks k = 3, 4 per vertex with app.validate_cliques (slow: small graphs).

    python benchmarks/bench_clique.py [--graphs googleplus,orkut_community] [--scale 0.125] [--ab] [--out profiles/clique.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

AB = {"clique_tiny": (0, 16), "clique_mid": (0, 64, 128), "clique_lds": (0, 512), "clique_grid": (2, 4, 16, 32), "clique_waves": (4, 8)}


def span_stats(fn, runs):
    """(median, min, max) GPU time of fn() in ms (HIP events on the library's stream) after three untimed runs"""
    from graphlily_amd import capi

    def once():
        capi.span_begin()
        fn()
        return capi.span_end()
    for _ in range(3):
        once()
    t = [once() for _ in range(runs)]
    return float(np.median(t)), float(min(t)), float(max(t))


def with_knob(key, value, fn):
    old = os.environ.get("GRAPHLILY_DEBUG")
    os.environ["GRAPHLILY_DEBUG"] = ",".join(x for x in (old, "%s=%s" % (key, value)) if x)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["GRAPHLILY_DEBUG"]
        else:
            os.environ["GRAPHLILY_DEBUG"] = old


def measure(oriented, runs, ks=(3, 4, 5), per_vertex=True):
    """one plan of `oriented`: the times, the counts and the bins"""
    from graphlily_amd import capi
    plan = capi.SpMVPlan(oriented.num_rows, oriented.num_cols, oriented.adj_indptr, oriented.adj_indices, oriented.adj_data, 0,
                         oriented.num_rows, flags=capi.GL_PLAN_BOOLEAN)
    n = oriented.num_rows
    total, per, tc_total = capi.DeviceBuffer(8), capi.DeviceBuffer(8 * n), capi.DeviceBuffer(8)
    bins = plan.clique_count(3, total, stats=True)              # (the plan's first call: the verdict, the bins, the slabs)
    plan.tc_count(tc_total)
    capi.sync()
    assert int(total.read(np.uint64, 1)[0]) == int(tc_total.read(np.uint64, 1)[0]), "gl_clique_count(3) and gl_tc_count disagree"
    rec = {"bins": list(bins[:3]), "cliques": {}}
    for k in ks:
        med, lo, hi = span_stats(lambda: plan.clique_count(k, total), runs)
        rec["k%d_ms" % k], rec["k%d_min_ms" % k], rec["k%d_max_ms" % k] = round(med, 4), round(lo, 4), round(hi, 4)
        rec["cliques"][str(k)] = int(total.read(np.uint64, 1)[0])
        if per_vertex:
            rec["k%d_per_vertex_ms" % k] = round(span_stats(lambda: plan.clique_count(k, total, per), runs)[0], 4)
            assert int(per.read(np.uint64, n).sum()) == k * rec["cliques"][str(k)]
    rec["tc_ms"] = round(span_stats(lambda: plan.tc_count(tc_total), runs)[0], 4)
    rec["k3_over_tc"] = round(rec["k3_ms"] / rec["tc_ms"], 3) if rec["tc_ms"] > 0 else None
    rec["build_ms"] = round(with_knob("clique_build_only", 1, lambda: span_stats(lambda: plan.clique_count(3, total), runs))[0], 4)
    rec["build_share"] = round(rec["build_ms"] / rec["k3_ms"], 3) if rec["k3_ms"] > 0 else None
    rec["launches"] = plan.clique_count(3, total, stats=True)[3]
    return rec, per.read(np.uint64, n) if per_vertex else None


def run_graph(name, raw, runs=9, ab=False, verify=False):
    from graphlily_amd import app, capi, io
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    kc = app.KCore(16, 0, 0)
    kc.set_up_runtime()
    kc.load_and_format_matrix(raw, True)
    kc.send_matrix_host_to_device()
    kc.run(order=True)
    position = np.empty(kc.n_, dtype=np.uint32)
    position[kc.order_] = np.arange(kc.n_, dtype=np.uint32)
    out = []
    for rank_name, rank in (("degree", None), ("degeneracy", position)):
        oriented, deg = io.orient_by_rank(padded, rank)
        lens = np.diff(oriented.adj_indptr.astype(np.int64))
        base = {"graph": name, "rank": rank_name, "n": oriented.num_rows, "oriented_entries": oriented.nnz,
                "longest_row": int(lens.max()), "degeneracy": int(kc.degeneracy_), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
        try:
            rec, per = measure(oriented, runs)
        except capi.GraphLilyError as e:                        # (a row above 8192 entries: the degree rank on a hub-heavy graph)
            out.append(dict(base, unsupported=str(e)))
            continue
        if verify:
            for k in (3, 4):
                d = app.CliqueCount(16, 0, 0)
                d.set_up_runtime()
                d.load_and_format_matrix(raw, rank)
                d.send_matrix_host_to_device()
                rec["verified_k%d" % k] = app.validate_cliques(padded, k, d.run(k)) == rec["cliques"][str(k)]
            capi.sync()
        out.append(dict(base, **rec))
        if ab:
            for key, values in AB.items():
                for value in values:
                    got = with_knob(key, value, lambda: measure(oriented, runs, per_vertex=False)[0])
                    assert got["cliques"] == rec["cliques"], (key, value)
                    out.append(dict(base, ab="%s=%s" % (key, value), **got))
    return out


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(list(datasets.PAPER_GRAPHS) + ["orkut_community"]))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clique.jsonl"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--ab", action="store_true", help="one line per knob value behind every line")
    ap.add_argument("--verify", action="store_true", help="check k = 3, 4 per vertex with app.validate_cliques (Python sets: small graphs)")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, runs=args.runs, ab=args.ab, verify=args.verify):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
