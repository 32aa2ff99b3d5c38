#!/usr/bin/env python
"""Topological levels and critical paths (gl_topo) on the six stand-ins and orkut_community, one GPU, one process.

Every stand-in is symmetrised (io.symmetrize_simple) and ORIENTED into a DAG three ways -- an edge u -> v iff u goes before v:
  natural   by vertex number
  degree    io.triangle_orient's order, (degree, vertex) ascending: hubs last
  random    a seeded permutation (numpy.random.default_rng(11))
and, with --cyclic, also run as bench_scc.py's one-way thinning of the symmetric form, which has cycles: the peeled share is
reported.  Per graph and orientation one JSON line:
  call_ms            gl_topo unweighted (it synchronises itself), wall clock: median of `runs` after three untimed runs, with
                     call_ms_min / call_ms_max; weighted_ms: the same with uniform [0, 1) f32 weights, dist and parent
  levels, widest, peeled, launches, us_per_level = 1000 call_ms / levels, entries_per_s = edges / call_ms
  color_ms, color_rounds, color_us_per_round
                     gl_color on the symmetric form with priorities that induce the SAME DAG (the same dependency counters and as
                     many decrements, plus the search for a colour); rounds_equal_levels says whether its rounds are gl_topo's
                     levels; topo_over_color = us_per_level / color_us_per_round
  verified           level, dist and parent equal app._topological_of's on the host (to the bit) before any time is reported
--networkx adds, on rmat_20K only, the host times of networkx.topological_generations and dag_longest_path_length.
--ab adds one short line per knob value ("ab": "topo_cut=0"), timed on the same plans right behind the default line: topo_cut
0 / 4 / 8 / 16 / 32, topo_grid 1 / 2 / 4 / 8 / 16, topo_batch 1 / 8 / 32 / 64 / 128 / 512.

    python benchmarks/bench_topo.py [--graphs googleplus,orkut_community] [--scale 0.125] [--ab] [--cyclic] [--out profiles/topo.jsonl]
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
from bench_scc import thin_one_way  # noqa: E402
from bench_truss import _with_knob  # noqa: E402

TOPO_CUT, TOPO_GRID, TOPO_BATCH = 8, 4, 64          # the library's defaults (csrc/gl_topo.hip)
AB = [("topo_cut", v) for v in (0, 4, 8, 16, 32)] + [("topo_grid", v) for v in (1, 2, 4, 8, 16)] + \
     [("topo_batch", v) for v in (1, 8, 32, 64, 128, 512)]
ORIENTATIONS = ("natural", "degree", "random")


def rank_of(orientation, deg, n):
    """-> int64[n]: the place of every vertex in the order; an edge goes from the smaller rank to the larger"""
    if orientation == "natural":
        return np.arange(n, dtype=np.int64)
    if orientation == "degree":
        order = np.lexsort((np.arange(n), deg))
    elif orientation == "random":
        order = np.random.default_rng(11).permutation(n)
    else:
        raise KeyError(orientation)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    return rank


def orient(sym, rank):
    """-> (csr_in, csr_out): row v of csr_in keeps the neighbours of smaller rank (its predecessors), row v of csr_out those of
    larger rank; subsets of sym's ascending rows"""
    from graphlily_amd import io
    n = sym.num_rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
    cols = sym.adj_indices.astype(np.int64)
    before = rank[cols] < rank[rows]

    def keep(mask):
        ip = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows[mask], minlength=n), out=ip[1:])
        return io.CSRMatrix(n, n, np.ones(int(mask.sum()), np.float32), cols[mask].astype(np.uint32), ip.astype(np.uint32))
    return keep(before), keep(~before & (cols != rows))


def run_dag(name, orientation, sym, deg, n_real, runs, ab):
    from graphlily_amd import app, capi
    n = sym.num_rows
    rank = rank_of(orientation, deg.astype(np.int64), n)
    cin, cout = orient(sym, rank)

    def boolean(m):
        return capi.SpMVPlan(n, n, m.adj_indptr, m.adj_indices, m.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    pin, pout, psym = boolean(cin), boolean(cout), boolean(sym)
    w = np.random.default_rng(12).random(cin.nnz, dtype=np.float32)
    dw = capi.DeviceBuffer.from_host(w) if cin.nnz else None
    level, dist, parent, color = (capi.DeviceBuffer(4 * max(1, n)) for _ in range(4))
    prio = None if orientation == "natural" else capi.DeviceBuffer.from_host((n - 1 - rank).astype(np.uint32))
    capi.sync()
    t0 = time.perf_counter()
    stats = pin.topo(pout, level)
    first_call_ms = (time.perf_counter() - t0) * 1e3
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(cin.adj_indptr.astype(np.int64)))
    want = app._topological_of(n, cin.adj_indices.astype(np.int64), dst, w)
    assert np.array_equal(level.read(np.uint32, n), want[0]), "%s/%s: the levels differ from the host loop's" % (name, orientation)
    wstats = pin.topo(pout, level, None, dw, dist, parent)
    assert wstats[:3] == stats[:3] and stats[0] == n
    assert np.array_equal(dist.read(np.uint32, n), want[1].view(np.uint32)) and np.array_equal(parent.read(np.uint32, n), want[2]), \
        "%s/%s: dist or parent differ from the host loop's" % (name, orientation)
    print("%s/%s: %d peeled, %d levels, widest %d, %d launches" % ((name, orientation) + stats), file=sys.stderr, flush=True)
    call_ms = wall_ms(lambda: pin.topo(pout, level), runs)
    weighted_ms = wall_ms(lambda: pin.topo(pout, level, None, dw, dist, parent), runs)
    cstats = psym.color(prio, color)
    color_ms = wall_ms(lambda: psym.color(prio, color), runs)
    levels = stats[1]
    us_level, us_round = 1e3 * call_ms[0] / max(1, levels), 1e3 * color_ms[0] / max(1, cstats[1])
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    yield {"graph": name, "orientation": orientation, "n": n, "n_real": n_real, "edges": cin.nnz,
           "longest_in_row": int(np.diff(cin.adj_indptr.astype(np.int64)).max()), "longest_out_row": int(np.diff(cout.adj_indptr.astype(np.int64)).max()),
           "peeled": stats[0], "levels": levels, "widest": stats[2], "launches": stats[3],
           "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
           "weighted_ms": round(weighted_ms[0], 4), "weighted_ms_min": round(weighted_ms[1], 4), "weighted_ms_max": round(weighted_ms[2], 4),
           "first_call_ms": round(first_call_ms, 4), "us_per_level": round(us_level, 3),
           "entries_per_s": round(cin.nnz / (call_ms[0] * 1e-3)) if call_ms[0] > 0 else None,
           "weighted_entries_per_s": round(cin.nnz / (weighted_ms[0] * 1e-3)) if weighted_ms[0] > 0 else None,
           "color_ms": round(color_ms[0], 4), "color_ms_min": round(color_ms[1], 4), "color_ms_max": round(color_ms[2], 4),
           "color_rounds": cstats[1], "colors": cstats[0], "rounds_equal_levels": cstats[1] == levels,
           "color_us_per_round": round(us_round, 3), "topo_over_color": round(us_level / us_round, 3) if us_round > 0 else None,
           "call_over_color": round(call_ms[0] / color_ms[0], 3) if color_ms[0] > 0 else None,
           "verified": True, "runs": runs, "topo_cut": int(knobs.get("topo_cut", TOPO_CUT)), "topo_grid": int(knobs.get("topo_grid", TOPO_GRID)),
           "topo_batch": int(knobs.get("topo_batch", TOPO_BATCH)), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    for key, value in AB if ab else ():
        res = _with_knob(key, value, lambda: (pin.topo(pout, level), wall_ms(lambda: pin.topo(pout, level), runs),
                                              wall_ms(lambda: pin.topo(pout, level, None, dw, dist, parent), runs)))
        assert res[0][:3] == stats[:3] and np.array_equal(level.read(np.uint32, n), want[0])
        yield {"graph": name, "orientation": orientation, "ab": "%s=%d" % (key, value), "call_ms": round(res[1][0], 4),
               "call_ms_min": round(res[1][1], 4), "call_ms_max": round(res[1][2], 4), "weighted_ms": round(res[2][0], 4),
               "levels": levels, "launches": res[0][3], "runs": runs, "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def run_cyclic(name, sym, n_real, runs):
    """the one-way thinning of bench_scc.py: cycles remain, and the peel says which vertices are on or behind one"""
    from graphlily_amd import capi, io
    n = sym.num_rows
    cin, cout, symmetric = io.simple_pattern(thin_one_way(sym))
    assert not symmetric
    pin = capi.SpMVPlan(n, n, cin.adj_indptr, cin.adj_indices, cin.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    pout = capi.SpMVPlan(n, n, cout.adj_indptr, cout.adj_indices, cout.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    level = capi.DeviceBuffer(4 * max(1, n))
    stats = pin.topo(pout, level)
    call_ms = wall_ms(lambda: pin.topo(pout, level), runs)
    peeled_real = int(np.count_nonzero(level.read(np.uint32, n)[:n_real] != 0xFFFFFFFF))
    yield {"graph": name, "orientation": "thinned (cyclic)", "n": n, "n_real": n_real, "edges": cin.nnz, "peeled": stats[0], "levels": stats[1],
           "widest": stats[2], "launches": stats[3], "peeled_share": round(peeled_real / max(1, n_real), 4), "call_ms": round(call_ms[0], 4),
           "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4), "runs": runs, "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def networkx_times(sym, deg):
    """host comparison on one small graph: the natural orientation through networkx"""
    import networkx as nx
    cin, _ = orient(sym, rank_of("natural", deg, sym.num_rows))
    dst = np.repeat(np.arange(sym.num_rows), np.diff(cin.adj_indptr.astype(np.int64)))
    w = np.random.default_rng(12).random(cin.nnz, dtype=np.float32)
    G = nx.DiGraph()
    G.add_nodes_from(range(sym.num_rows))
    G.add_weighted_edges_from(zip(cin.adj_indices.tolist(), dst.tolist(), w.tolist()))
    t0 = time.perf_counter()
    gens = list(nx.topological_generations(G))
    t1 = time.perf_counter()
    length = nx.dag_longest_path_length(G)
    t2 = time.perf_counter()
    return {"networkx_generations_ms": round((t1 - t0) * 1e3, 2), "networkx_longest_path_ms": round((t2 - t1) * 1e3, 2),
            "networkx_levels": len(gens), "networkx_longest_path": length}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(list(datasets.PAPER_GRAPHS) + ["orkut_community"]))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--orientations", default=",".join(ORIENTATIONS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topo.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plans")
    ap.add_argument("--cyclic", action="store_true", help="also run the one-way thinning, which has cycles")
    ap.add_argument("--networkx", action="store_true", help="also time networkx on rmat_20K")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi, io
    dev = torch.device("cuda:0")
    capi.init(0)

    def emit(rec, scale):
        rec["scale"] = scale
        rec["data"] = "synthetic stand-in"
        print(json.dumps(rec), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    graphs = [g for g in args.graphs.split(",") if g]
    for name in graphs + (["rmat_20K"] if args.networkx else []):
        if name == "rmat_20K":
            raw, scale = datasets.rmat(20000, 400000, seed=11, symmetric=False), 1.0
        else:
            raw, scale = datasets.paper_graph(name, args.scale, device=dev), args.scale
        padded = raw.copy()
        io.util_round_csr_matrix_dim(padded, 128, 128)
        sym, deg = io.symmetrize_simple(padded)
        for orientation in args.orientations.split(","):
            for rec in run_dag(name, orientation, sym, deg, raw.num_rows, args.runs, args.ab):
                if name == "rmat_20K" and orientation == "natural" and "ab" not in rec:
                    rec.update(networkx_times(sym, deg.astype(np.int64)))
                emit(rec, scale)
        if args.cyclic:
            for rec in run_cyclic(name, sym, raw.num_rows, args.runs):
                emit(rec, scale)


if __name__ == "__main__":
    main()
