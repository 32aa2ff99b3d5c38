#!/usr/bin/env python
"""Biconnected components (gl_bicc) on the six stand-ins and orkut_community, one GPU.

Every stand-in is measured as io.symmetrize_simple prepares it (the undirected simple graph of its matrix).  Per graph one JSON line:
  call_ms          gl_bicc with all outputs but the diagnostic tree (it synchronises itself), wall clock: median of `runs` after
                   three untimed runs; call_ms_min / call_ms_max: the spread.  The plan's first call (verdicts, scratch) is timed
                   once as first_call_ms.  blocks_only_ms: the call without vertex_blocks' and edge_component's buffers
  levels_ms, forest_ms, unite_ms, labels_ms, results_ms
                   the phases, as differences of the medians of the call ended behind phase 2, 6, 7 and 8 (bicc_stop = 1 .. 4):
                   roots and levels; parent, nd, pre, low / high; union-find; entry labels; bridges, tops, edge components
  depth, launches, trees, blocks, articulation, bridges, largest_block_share
                   gl_bicc's statistics (over the real vertices) and the share of the edges in the largest block
  cc_ms, scc_ms    gl_cc_labels and gl_scc (plan_out == plan_in: the pattern is symmetric) on the same plan in the same process;
                   call_over_cc, call_over_scc
  networkx_ms, scipy_ms   (--host, on a graph of at most --host-edges edges) networkx.biconnected_components + articulation_points
                   and scipy's connected_components on the host, one call each; app.validate_biconnected must accept gl_bicc's
                   result before any time is reported
--ab adds one short line per knob value ("ab": "bicc_cut=0", call_ms), timed on the same plan in the same process right behind the
default line (the knobs are read per call): bicc_cut 0 / 8 / 16 / 32 / 64, bicc_grid 2 / 4 / 8 / 16 / 64, bicc_batch 1 / 8 / 32 / 128.
Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG and are recorded with every line.

    python benchmarks/bench_bicc.py [--graphs googleplus,orkut] [--scale 0.125] [--ab] [--host] [--out profiles/bicc.jsonl]
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

BICC_CUT, BICC_GRID, BICC_BATCH = 32, 8, 32        # the library's defaults (csrc/gl_bicc.hip)

AB = [("bicc_cut", v) for v in (0, 8, 16, 32, 64)] + [("bicc_grid", v) for v in (2, 4, 8, 16, 64)] + [("bicc_batch", v) for v in (1, 8, 32, 128)]


def host_times(sym, n):
    """-> (networkx ms, scipy ms): the blocks and articulation points, and the components, on the host"""
    import networkx as nx
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    A = sp.csr_matrix((np.ones(sym.nnz, np.int8), sym.adj_indices.astype(np.int64), sym.adj_indptr.astype(np.int64)), shape=(n, n))
    G = nx.from_scipy_sparse_array(A)
    t0 = time.perf_counter()
    blocks = sum(1 for _ in nx.biconnected_components(G))
    cuts = sum(1 for _ in nx.articulation_points(G))
    t1 = time.perf_counter()
    connected_components(A, directed=False)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, blocks, cuts


def run_graph(name, raw, runs=5, ab=False, host_edges=0):
    from graphlily_amd import app, capi, io
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    sym, _ = io.symmetrize_simple(padded)
    n, nnz, n_real = sym.num_rows, sym.nnz, raw.num_rows
    plan = capi.SpMVPlan(n, n, sym.adj_indptr, sym.adj_indices, sym.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    block, vb, ec, label = (capi.DeviceBuffer(4 * max(1, k)) for k in (nnz, n, n, n))
    capi.sync()
    t0 = time.perf_counter()
    stats = plan.bicc(block, vb, ec)
    first_call_ms = (time.perf_counter() - t0) * 1e3
    got = block.read(np.uint32, nnz)
    labels, entries = np.unique(got, return_counts=True)
    assert labels.shape[0] == stats[0] and int(np.count_nonzero(entries == 2)) == stats[2]
    assert int(np.count_nonzero(vb.read(np.uint32, n) >= 2)) == stats[1]
    print("%s: %d blocks, %d articulation points, %d bridges, depth %d, %d launches, %d trees" % ((name,) + stats), file=sys.stderr, flush=True)
    rec = {"graph": name, "n": n, "edges": nnz // 2, "longest_row": int(np.diff(sym.adj_indptr.astype(np.int64)).max())}
    if 0 < nnz // 2 <= host_edges:
        assert app.validate_biconnected(sym, got, vb.read(np.uint32, n), ec.read(np.uint32, n)) == stats[0]
        nx_ms, sp_ms, nx_blocks, nx_cuts = host_times(sym, n)
        assert (nx_blocks, nx_cuts) == stats[:2]
        rec.update(networkx_ms=round(nx_ms, 1), scipy_ms=round(sp_ms, 2), verified=True)
    call_ms = wall_ms(lambda: plan.bicc(block, vb, ec), runs)
    assert np.array_equal(block.read(np.uint32, nnz), got)
    only_ms = wall_ms(lambda: plan.bicc(block), runs)
    upto = [_with_knob("bicc_stop", k, lambda: wall_ms(lambda: plan.bicc(block, vb, ec), runs))[0] for k in (1, 2, 3, 4)]

    def cc():
        plan.cc_labels(label)
        capi.sync()
    cc_ms = wall_ms(cc, runs)
    scc_ms = wall_ms(lambda: plan.scc(None, label), runs)
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    rec.update({"blocks": stats[0], "articulation": stats[1], "bridges": stats[2], "depth": stats[3], "launches": stats[4],
                "trees": stats[5] - (n - n_real), "largest_block_share": round(float(entries.max()) / nnz, 4) if nnz else 0.0,
                "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
                "first_call_ms": round(first_call_ms, 4), "blocks_only_ms": round(only_ms[0], 4),
                "levels_ms": round(upto[0], 4), "forest_ms": round(upto[1] - upto[0], 4), "unite_ms": round(upto[2] - upto[1], 4),
                "labels_ms": round(upto[3] - upto[2], 4), "results_ms": round(call_ms[0] - upto[3], 4), "cc_ms": round(cc_ms[0], 4), "scc_ms": round(scc_ms[0], 4),
                "call_over_cc": round(call_ms[0] / cc_ms[0], 2) if cc_ms[0] > 0 else None,
                "call_over_scc": round(call_ms[0] / scc_ms[0], 2) if scc_ms[0] > 0 else None,
                "us_per_launch": round(1e3 * call_ms[0] / stats[4], 2) if stats[4] else None,
                "runs": runs, "bicc_cut": int(knobs.get("bicc_cut", BICC_CUT)), "bicc_grid": int(knobs.get("bicc_grid", BICC_GRID)),
                "bicc_batch": int(knobs.get("bicc_batch", BICC_BATCH)), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")})
    if "networkx_ms" in rec:
        rec["networkx_over_call"] = round(rec["networkx_ms"] / call_ms[0], 1)
    yield rec
    for key, value in AB if ab else ():
        res = _with_knob(key, value, lambda: (plan.bicc(block, vb, ec), wall_ms(lambda: plan.bicc(block, vb, ec), runs)))
        assert res[0][:4] == stats[:4] and np.array_equal(block.read(np.uint32, nnz), got)
        yield {"graph": name, "ab": "%s=%d" % (key, value), "call_ms": round(res[1][0], 4), "call_ms_min": round(res[1][1], 4),
               "call_ms_max": round(res[1][2], 4), "launches": res[0][4], "depth": stats[3], "runs": runs,
               "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(list(datasets.PAPER_GRAPHS) + ["orkut_community"]))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicc.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plan")
    ap.add_argument("--host", action="store_true", help="validate and time networkx / scipy on the graphs that are small enough")
    ap.add_argument("--host-edges", type=int, default=2_000_000)
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, runs=args.runs, ab=args.ab, host_edges=args.host_edges if args.host else 0):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
