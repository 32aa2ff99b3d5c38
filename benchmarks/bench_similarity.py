#!/usr/bin/env python
"""Neighbourhood similarity (gl_similarity) on the six stand-ins and orkut_community, one GPU, one process.

Every stand-in is loaded as app.Similarity loads it (io.symmetrize_simple), so that the kernel and its yardsticks run in the same
process on the SAME plan.  Per graph and pair set one JSON line:
  pairs "edges"     every edge {u, v}, u < v: the pairs of Similarity.run_edges
  pairs "two_hop"   up to 2^20 random non-adjacent pairs with a common neighbour (numpy.random.default_rng(30): a random vertex w
                    of degree >= 2 and two of its neighbours, kept when they are not adjacent): link-prediction candidates
  common_ms         gl_similarity, counts only (stats are read back, so the call synchronises), wall clock: median of `runs` after
                    three untimed runs, with common_ms_min / common_ms_max; weighted_ms: the same with the Adamic-Adar table
  pairs_per_s, shorter_entries_per_s
                    pairs / common_ms and the entries of the pairs' SHORTER rows (what the kernel walks) / common_ms
  deferred, launches
  support_ms        (edges only) the support pass of gl_truss alone on the same plan (GRAPHLILY_DEBUG truss_support_only=1, as
                    benchmarks/bench_truss.py takes it): the same intersections for the same edges; similarity_over_support =
                    common_ms / support_ms, above 1 the per-pair kernel is slower
  scipy_ms          the host statement of app.validate_similarity -- the row products S[u] . S[v]^T -- for the first scipy_pairs
                    pairs, one run
  verified          the edge counts equal gl_truss's d_support at the entries above the diagonal, and the two-hop counts equal the
                    scipy statement on the first scipy_pairs pairs, before any time is reported
--ab adds one short line per knob value ("ab": "sim_group=8"), timed on the same plan right behind the default line: sim_group
8 / 16 / 32 / 64, sim_short 0 / 16 / 32 / 64 / 128 / 256, sim_grid 4 / 8 / 16 / 32.

    python benchmarks/bench_similarity.py [--graphs googleplus,orkut_community] [--scale 0.125] [--ab] [--out profiles/similarity.jsonl]
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
from bench_truss import _with_knob  # noqa: E402

SIM_GROUP, SIM_SHORT, SIM_GRID = 16, 64, 16       # the library's defaults (csrc/gl_sim.hip)
AB = [("sim_group", v) for v in (8, 16, 32, 64)] + [("sim_short", v) for v in (0, 16, 32, 64, 128, 256)] + \
     [("sim_grid", v) for v in (4, 8, 16, 32)]
TWO_HOP = 1 << 20
SCIPY_PAIRS = 1 << 14


def two_hop_pairs(graph, deg, count, rng):
    """-> int64[<= count, 2]: random non-adjacent pairs (u, v), u != v, with a common neighbour"""
    n = graph.num_rows
    ip, idx = graph.adj_indptr.astype(np.int64), graph.adj_indices.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    keys = rows * n + idx                                             # ascending: the rows are sorted sets
    mids = np.flatnonzero(deg >= 2)
    out, have = [], 0
    for _ in range(8):
        if mids.size == 0 or have >= count:
            break
        w = rng.choice(mids, size=2 * count)
        a = idx[ip[w] + (rng.random(w.shape[0]) * deg[w]).astype(np.int64)]
        b = idx[ip[w] + (rng.random(w.shape[0]) * deg[w]).astype(np.int64)]
        at = np.minimum(np.searchsorted(keys, a * n + b), keys.shape[0] - 1)
        keep = (a != b) & (keys[at] != a * n + b)
        out.append(np.stack([a[keep], b[keep]], axis=1))
        have += int(keep.sum())
    return np.concatenate(out)[:count] if out else np.zeros((0, 2), np.int64)


def run_graph(name, raw, runs, ab):
    from graphlily_amd import app, capi
    d = app.Similarity(16, 0, 0)
    d.set_up_runtime()
    d.load_and_format_matrix(raw, True)
    d.send_matrix_host_to_device()
    n, plan, graph = d.n_, d.SpMV_.plan_, d.graph_
    deg = d.degrees_.astype(np.int64)
    nnz = graph.nnz
    ip = graph.adj_indptr.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    cols = graph.adj_indices.astype(np.int64)
    above = np.flatnonzero(cols > rows)
    edges = np.stack([rows[above], cols[above]], axis=1)
    # the yardstick on the same plan: the support pass of gl_truss
    truss, support = capi.DeviceBuffer(4 * max(1, nnz)), capi.DeviceBuffer(4 * max(1, nnz))
    _with_knob("truss_support_only", 1, lambda: plan.truss(truss, support))
    want_support = support.read(np.uint32, nnz)[above] if nnz else np.zeros(0, np.uint32)
    support_ms = _with_knob("truss_support_only", 1, lambda: wall_ms(lambda: plan.truss(truss), runs)) if nnz else (0.0, 0.0, 0.0)
    S = app._pattern_as_scipy(graph, n).astype(np.int64)
    rng = np.random.default_rng(30)
    for kind, pairs in (("edges", edges), ("two_hop", two_hop_pairs(graph, deg, TWO_HOP, rng))):
        m = pairs.shape[0]
        if m == 0:
            continue
        pairs_buf = capi.DeviceBuffer.from_host(pairs.astype(np.uint32).ravel())
        common, weighted = capi.DeviceBuffer(4 * m), capi.DeviceBuffer(8 * m)

        def call(table=None):
            return plan.similarity(pairs_buf, common, weighted if table is not None else None, table, True, m)

        stats = call()
        got = common.read(np.uint32, m)
        k = min(m, SCIPY_PAIRS)
        t0 = time.perf_counter()
        host = np.asarray(S[pairs[:k, 0]].multiply(S[pairs[:k, 1]]).sum(axis=1)).ravel()
        scipy_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(got[:k].astype(np.int64), host), "%s/%s: counts differ from the scipy row products" % (name, kind)
        if kind == "edges":
            assert np.array_equal(got, want_support), "%s: edge counts differ from gl_truss's d_support" % name
        else:
            assert got.min() >= 1, "%s: a two-hop pair without a common neighbour" % name
        shorter = int(np.minimum(deg[pairs[:, 0]], deg[pairs[:, 1]]).sum())
        print("%s/%s: %d pairs, %d deferred, %d launches" % (name, kind, m, stats[1], stats[2]), file=sys.stderr, flush=True)
        common_ms = wall_ms(call, runs)
        weighted_ms = wall_ms(lambda: call(d.aa_buf_), runs)
        knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
        rec = {"graph": name, "pairs": kind, "n": n, "n_real": d.n_real_, "entries": nnz, "longest_row": int(deg.max()) if n else 0,
               "m": m, "shorter_entries": shorter, "deferred": stats[1], "launches": stats[2],
               "common_ms": round(common_ms[0], 4), "common_ms_min": round(common_ms[1], 4), "common_ms_max": round(common_ms[2], 4),
               "weighted_ms": round(weighted_ms[0], 4), "weighted_ms_min": round(weighted_ms[1], 4), "weighted_ms_max": round(weighted_ms[2], 4),
               "pairs_per_s": round(m / (common_ms[0] * 1e-3)) if common_ms[0] > 0 else None,
               "shorter_entries_per_s": round(shorter / (common_ms[0] * 1e-3)) if common_ms[0] > 0 else None,
               "scipy_pairs": k, "scipy_ms": round(scipy_ms, 3), "verified": True, "runs": runs,
               "sim_group": int(knobs.get("sim_group", SIM_GROUP)), "sim_short": int(knobs.get("sim_short", SIM_SHORT)),
               "sim_grid": int(knobs.get("sim_grid", SIM_GRID)), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
        if kind == "edges":
            rec.update({"support_ms": round(support_ms[0], 4), "support_ms_min": round(support_ms[1], 4), "support_ms_max": round(support_ms[2], 4),
                        "similarity_over_support": round(common_ms[0] / support_ms[0], 3) if support_ms[0] > 0 else None})
        yield rec
        for key, value in AB if ab else ():
            res = _with_knob(key, value, lambda: (call(), wall_ms(call, runs)))
            assert np.array_equal(common.read(np.uint32, m), got) and res[0][0] == 0
            yield {"graph": name, "pairs": kind, "ab": "%s=%d" % (key, value), "common_ms": round(res[1][0], 4),
                   "common_ms_min": round(res[1][1], 4), "common_ms_max": round(res[1][2], 4), "deferred": res[0][1], "runs": runs,
                   "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(list(datasets.PAPER_GRAPHS) + ["orkut_community"]))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plan")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in [g for g in args.graphs.split(",") if g]:
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, args.runs, args.ab):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
