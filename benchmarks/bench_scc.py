#!/usr/bin/env python
"""Strongly connected components (gl_scc) on the six stand-ins, one GPU.

Every stand-in is measured as it is (io.simple_pattern: the simple directed graph of its matrix).  A stand-in whose pattern is
symmetric gives gl_cc_labels' components -- that is asserted -- and is measured ONCE MORE after a seeded ONE-WAY THINNING, so that
there is a directed run per graph: with rng = numpy.random.default_rng(7) and the undirected edges {lo, hi} in ascending (lo, hi)
order, coin = rng.random(edges); an edge with coin < 0.5 keeps both directions, one with coin < 0.75 keeps only lo -> hi, the others
only hi -> lo.  Such a line has "thinned": true.

Per graph and variant one JSON line, under the "largest_first" priorities (io.coloring_priorities on in-degree + out-degree):
  call_ms          gl_scc alone (it synchronises itself), wall clock: median of `runs` after three untimed runs; call_ms_min /
                   call_ms_max: the spread.  The plans' first call (verdicts, scratch) is timed once as first_call_ms
  passes, rounds, launches, trimmed, components, largest_component
                   gl_scc's statistics (over the padded matrix) and the largest component among the real vertices
  natural_ms, natural_passes
                   the same call without priorities (every vertex's number decides)
  cc_ms            gl_cc_labels on the same plan_in in the same process (weak components); call_over_cc = call_ms / cc_ms
  scipy_ms         scipy.sparse.csgraph.connected_components(connection="strong") on the host, one call; its labels, renamed to
                   every class's smallest vertex, must equal gl_scc's before any time is reported
--ab adds one short line per knob value ("ab": "scc_cut=0", call_ms and the statistics), timed on the same plans in the same
process right behind the default line (the knobs are read per call): scc_cut 0 / 4 / 8 / 16 / 32, scc_grid 1 / 2 / 4 / 8 / 16,
scc_batch 1 / 8 / 32 / 128 / 512.  Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG and are recorded with every line.

    python benchmarks/bench_scc.py [--graphs googleplus,orkut] [--scale 0.125] [--ab] [--out profiles/scc.jsonl]
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

SCC_CUT, SCC_GRID, SCC_BATCH = 8, 4, 32            # the library's defaults (csrc/gl_scc.hip)

AB = [("scc_cut", v) for v in (0, 4, 8, 16, 32)] + [("scc_grid", v) for v in (1, 2, 4, 8, 16)] + [("scc_batch", v) for v in (1, 8, 32, 128, 512)]


def thin_one_way(cin, seed=7):
    """the seeded one-way thinning of a symmetric simple pattern (the module's docstring) -> CSRMatrix whose row v lists the
    predecessors of v"""
    from graphlily_amd import io
    n = cin.num_rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(cin.adj_indptr.astype(np.int64)))
    cols = cin.adj_indices.astype(np.int64)
    up = cols > rows                                              # every undirected edge once, (lo, hi) ascending: the rows are sorted
    lo, hi = rows[up], cols[up]
    coin = np.random.default_rng(seed).random(lo.shape[0])
    both, fwd = coin < 0.5, (coin >= 0.5) & (coin < 0.75)
    src = np.concatenate([lo[both], hi[both], lo[fwd], hi[~both & ~fwd]])
    dst = np.concatenate([hi[both], lo[both], hi[fwd], lo[~both & ~fwd]])
    order = np.lexsort((src, dst))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=indptr[1:])
    return io.CSRMatrix(n, n, np.ones(src.shape[0], np.float32), src[order].astype(np.uint32), indptr.astype(np.uint32))


def scipy_strong(cin, n):
    """-> (labels by smallest vertex, seconds of the scipy call alone); row v of cin lists the predecessors of v"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    A = sp.csr_matrix((np.ones(cin.nnz, np.int8), cin.adj_indices.astype(np.int64), cin.adj_indptr.astype(np.int64)), shape=(n, n))
    t0 = time.perf_counter()
    count, comp = connected_components(A, directed=True, connection="strong")      # (the transpose has the same components)
    t = time.perf_counter() - t0
    smallest = np.full(count, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.uint32), t


def run_variant(name, cin, cout, n_real, thinned, runs, ab):
    from graphlily_amd import capi, io
    n = cin.num_rows

    def boolean(m):
        return capi.SpMVPlan(n, n, m.adj_indptr, m.adj_indices, m.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    pin = boolean(cin)
    pout = None if cout is None else boolean(cout)
    deg = (np.diff(cin.adj_indptr.astype(np.int64)) + np.bincount(cin.adj_indices, minlength=n)).astype(np.uint32)
    prio = capi.DeviceBuffer.from_host(io.coloring_priorities(deg, "largest_first", 0))
    label, weak = capi.DeviceBuffer(4 * max(1, n)), capi.DeviceBuffer(4 * max(1, n))
    capi.sync()
    t0 = time.perf_counter()
    stats = pin.scc(pout, label, prio)
    first_call_ms = (time.perf_counter() - t0) * 1e3
    got = label.read(np.uint32, n)
    want, scipy_s = scipy_strong(cin, n)
    assert np.array_equal(got, want), "%s: the labels differ from scipy's strong components" % name
    print("%s%s: %d components, %d passes, %d trimmed, %d rounds, %d launches" % ((name, " (thinned)" if thinned else "") + stats),
          file=sys.stderr, flush=True)
    call_ms = wall_ms(lambda: pin.scc(pout, label, prio), runs)
    assert np.array_equal(label.read(np.uint32, n), want)
    natural = pin.scc(pout, label, None)
    assert np.array_equal(label.read(np.uint32, n), want) and natural[0] == stats[0]
    natural_ms = wall_ms(lambda: pin.scc(pout, label, None), runs)

    def cc():
        pin.cc_labels(weak)
        capi.sync()
    cc_ms = wall_ms(cc, runs)
    if cout is None:
        assert np.array_equal(weak.read(np.uint32, n), want), "%s: a symmetric pattern, and gl_cc_labels disagrees" % name
    sizes = np.unique(got[:n_real], return_counts=True)[1]
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    yield {"graph": name, "thinned": thinned, "symmetric": cout is None, "n": n, "edges": cin.nnz, "longest_row": int(np.diff(cin.adj_indptr.astype(np.int64)).max()),
           "components": stats[0] - (n - n_real), "largest_component": int(sizes.max()), "passes": stats[1], "trimmed": stats[2] - (n - n_real),
           "rounds": stats[3], "launches": stats[4],
           "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
           "first_call_ms": round(first_call_ms, 4), "natural_ms": round(natural_ms[0], 4), "natural_passes": natural[1],
           "natural_rounds": natural[3], "cc_ms": round(cc_ms[0], 4), "call_over_cc": round(call_ms[0] / cc_ms[0], 2) if cc_ms[0] > 0 else None,
           "scipy_ms": round(scipy_s * 1e3, 2), "scipy_over_call": round(scipy_s * 1e3 / call_ms[0], 2) if call_ms[0] > 0 else None,
           "verified": True, "runs": runs, "scc_cut": int(knobs.get("scc_cut", SCC_CUT)), "scc_grid": int(knobs.get("scc_grid", SCC_GRID)),
           "scc_batch": int(knobs.get("scc_batch", SCC_BATCH)), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    for key, value in AB if ab else ():
        res = _with_knob(key, value, lambda: (pin.scc(pout, label, prio), wall_ms(lambda: pin.scc(pout, label, prio), runs)))
        assert res[0][:3] == stats[:3] and np.array_equal(label.read(np.uint32, n), want)
        yield {"graph": name, "thinned": thinned, "ab": "%s=%d" % (key, value), "call_ms": round(res[1][0], 4), "call_ms_min": round(res[1][1], 4),
               "call_ms_max": round(res[1][2], 4), "rounds": res[0][3], "launches": res[0][4], "passes": stats[1], "runs": runs,
               "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def run_graph(name, raw, runs=5, ab=False):
    from graphlily_amd import io
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    cin, cout, symmetric = io.simple_pattern(padded)
    for rec in run_variant(name, cin, cout, raw.num_rows, False, runs, ab and not symmetric):
        yield rec
    if symmetric:
        thin = thin_one_way(cin)
        tin, tout, still = io.simple_pattern(thin)
        assert not still
        for rec in run_variant(name, tin, tout, raw.num_rows, True, runs, ab):
            yield rec


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scc.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plans")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, runs=args.runs, ab=args.ab):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
