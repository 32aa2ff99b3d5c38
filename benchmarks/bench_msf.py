#!/usr/bin/env python
"""Minimum spanning forest (gl_msf) on the stand-ins benchmarks/bench_truss.py uses, at the same scale, one GPU.

Per graph and per weighting ("hash": 1 + hash(lo, hi) % 255, "equal": every weight 1) one JSON line:
  call_ms          gl_msf alone, forest words only (it synchronises itself), wall clock: median of `runs` after three untimed runs;
                   call_ms_min / call_ms_max: the spread.  call_labels_ms: the same with d_labels.  The plan's first call (verdicts,
                   scratch) is timed once as first_call_ms
  rounds, scans    rounds in which a component chose an edge; scans = rounds + 1 (the last scan finds nothing)
  ms_per_round     call_ms / scans
  upper_entries    entries above the diagonal, what one scan streams; upper_entries_per_s = scans * upper_entries / call_ms
  sweep_bytes      12 * upper_entries: 4 B index + 4 B weight + one 4 B comp gather per entry, what one scan must move at least;
  model_ms         scans * sweep_bytes at 6.29 TB/s (the measured float4-copy rate of the card); call_over_model = call_ms / model_ms
  cc_ms            gl_cc_labels on the same plan in the same process (one sweep of the same rows, both triangles, then pointer
                   doubling), with the wait; call_over_scans_cc = call_ms / (scans * cc_ms)
  scipy_ms         scipy.sparse.csgraph.minimum_spanning_tree on the host, one call; its total weight must equal the forest's
  edges, components, launches, total_weight
--ab adds one short line per knob value ("ab": "msf_cut=8", call_ms and the statistics), timed on the same plan in the same process
right behind the default line (the knobs are read per call): msf_cut 0 / 8 / 32 / 128, msf_grid 8 / 16 / 64 / 256, msf_batch 1 / 2 /
4 / 8 / 32, msf_filter 0 / 1.
Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG (msf_cut, default 32; msf_grid, default 64; msf_batch, default 4;
msf_filter, default 1) and are recorded with every line.

    python benchmarks/bench_msf.py [--graphs googleplus,orkut] [--scale 0.125] [--ab] [--out profiles/msf.jsonl]
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

MSF_CUT, MSF_GRID, MSF_BATCH, MSF_FILTER = 32, 64, 4, 1       # the library's defaults (csrc/gl_msf.hip)
COPY_BYTES_PER_S = 6.29e12                                    # float4 copy, measured on the card

AB = [("msf_cut", v) for v in (0, 8, 32, 128)] + [("msf_grid", v) for v in (8, 16, 64, 256)] + \
     [("msf_batch", v) for v in (1, 2, 4, 8, 32)] + [("msf_filter", v) for v in (0, 1)]


def weights_of(sym, kind):
    """one f32 per entry of the symmetric matrix, both entries of an edge alike"""
    if kind == "equal":
        return np.ones(sym.nnz, dtype=np.float32)
    rows = np.repeat(np.arange(sym.num_rows, dtype=np.uint64), np.diff(sym.adj_indptr.astype(np.int64)))
    cols = sym.adj_indices.astype(np.uint64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    h = (lo * np.uint64(0x9e3779b97f4a7c15) + hi * np.uint64(0xc2b2ae3d27d4eb4f)) >> np.uint64(40)
    return (1 + h % np.uint64(255)).astype(np.float32)


def run_graph(name, raw, runs=5, ab=False, host=True):
    from graphlily_amd import capi, io
    import scipy.sparse as sp
    from scipy.sparse.csgraph import minimum_spanning_tree
    t0 = time.perf_counter()
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    sym, deg = io.symmetrize_weighted(padded, weighted=False)
    prepare_s = time.perf_counter() - t0
    n, nnz = sym.num_rows, sym.nnz
    upper = nnz // 2
    plan = capi.SpMVPlan(n, n, sym.adj_indptr, sym.adj_indices, sym.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    forest, labels = capi.DeviceBuffer(4 * max(1, nnz)), capi.DeviceBuffer(4 * (n + 1))
    count = capi.DeviceBuffer(4, ptr=labels.ptr + 4 * n, keepalive=labels)
    first = True
    for kind in ("hash", "equal"):
        w_host = weights_of(sym, kind)
        w = capi.DeviceBuffer.from_host(w_host)
        capi.sync()
        t0 = time.perf_counter()
        stats = plan.msf(w, forest)
        first_call_ms = (time.perf_counter() - t0) * 1e3 if first else None
        first = False
        print("%s/%s: %d edges, %d rounds, %d launches" % (name, kind, stats[0], stats[2], stats[3]), file=sys.stderr, flush=True)
        call_ms = wall_ms(lambda: plan.msf(w, forest), runs)
        call_labels_ms = wall_ms(lambda: plan.msf(w, forest, labels), runs)
        mask = forest.read(np.uint32, nnz) != 0

        def cc():
            plan.cc_labels(labels, count)
            capi.sync()
        cc_ms = wall_ms(cc, runs)
        assert int(count.read(np.uint32, 1)[0]) == stats[1], "gl_cc_labels and gl_msf disagree on the components"
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
        once = mask & (sym.adj_indices.astype(np.int64) > rows)
        total = float(w_host[once].astype(np.float64).sum())
        scipy_ms = None
        if host:
            A = sp.csr_matrix((w_host.astype(np.float64), sym.adj_indices.astype(np.int32), sym.adj_indptr.astype(np.int64)), shape=(n, n))
            t0 = time.perf_counter()
            T = minimum_spanning_tree(A)
            scipy_ms = (time.perf_counter() - t0) * 1e3
            assert T.nnz == stats[0] and float(T.sum()) == total, "scipy's minimum spanning tree has another weight"
        scans = stats[2] + 1
        model_ms = scans * 12.0 * upper / COPY_BYTES_PER_S * 1e3
        knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
        rec = {"graph": name, "weights": kind, "n": n, "nnz": raw.nnz, "symmetric_entries": nnz, "upper_entries": upper,
               "longest_row": int(deg.max()) if n else 0, "edges": stats[0], "components": stats[1], "rounds": stats[2], "scans": scans,
               "launches": stats[3], "total_weight": total,
               "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
               "call_labels_ms": round(call_labels_ms[0], 4), "ms_per_round": round(call_ms[0] / scans, 4),
               "upper_entries_per_s": round(scans * upper / (call_ms[0] * 1e-3), 1) if call_ms[0] > 0 else None,
               "sweep_bytes": 12 * upper, "model_ms": round(model_ms, 4),
               "call_over_model": round(call_ms[0] / model_ms, 2) if model_ms > 0 else None,
               "cc_ms": round(cc_ms[0], 4), "call_over_scans_cc": round(call_ms[0] / (scans * cc_ms[0]), 3) if cc_ms[0] > 0 else None,
               "scipy_ms": round(scipy_ms, 2) if scipy_ms is not None else None, "runs": runs, "prepare_s": round(prepare_s, 3),
               "msf_cut": int(knobs.get("msf_cut", MSF_CUT)), "msf_grid": int(knobs.get("msf_grid", MSF_GRID)),
               "msf_batch": int(knobs.get("msf_batch", MSF_BATCH)), "msf_filter": int(knobs.get("msf_filter", MSF_FILTER)),
               "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
        if first_call_ms is not None:
            rec["first_call_ms"] = round(first_call_ms, 4)
        yield rec
        for key, value in AB if ab else ():
            got = _with_knob(key, value, lambda: (plan.msf(w, forest), wall_ms(lambda: plan.msf(w, forest), runs)))
            assert got[0][:3] == stats[:3] and np.array_equal(forest.read(np.uint32, nnz) != 0, mask)
            yield {"graph": name, "weights": kind, "ab": "%s=%d" % (key, value), "call_ms": round(got[1][0], 4),
                   "call_ms_min": round(got[1][1], 4), "call_ms_max": round(got[1][2], 4), "launches": got[0][3], "runs": runs,
                   "rounds": stats[2], "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msf.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plan")
    ap.add_argument("--no-host", action="store_true", help="skip scipy's minimum_spanning_tree on the host")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, runs=args.runs, ab=args.ab, host=not args.no_host):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
