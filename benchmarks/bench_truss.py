#!/usr/bin/env python
"""k-truss decomposition (KTruss / gl_truss) on the stand-ins benchmarks/bench_kcore.py uses, at the same scale, one GPU.

Per graph one JSON line:
  call_ms          gl_truss alone, truss numbers only (it synchronises itself), wall clock: median of `runs` after three untimed
                   runs; call_ms_min / call_ms_max: the spread.  The plan's first call (verdicts, scratch, edge numbering) is
                   timed once as first_call_ms
  support_ms       the support pass alone (GRAPHLILY_DEBUG truss_support_only=1: the call ends behind it), the same way
  tc_ms            gl_tc_count with per-vertex counts on the degree-oriented form of the same graph in the same process
  peel_ms          call_ms - support_ms; steps = the (scan, peel, turn) triples that did work = levels scanned is not known to the
                   host, so steps = levels + sub_rounds, a lower bound on the scans; us_per_step = peel_ms / steps
  kcore_call_ms, kcore_steps, kcore_us_per_step
                   gl_kcore on the same plan in the same process, steps = degeneracy + 1 scans + sub_rounds peels
  edges_per_s      edges / call_ms;  peeled_edges_per_s = edges / peel_ms
  max_truss, levels, sub_rounds, launches, edges, triangles, max_support
  run_ms           KTruss.run() end to end: gl_truss, the 4 nnz-byte read-back, the host arithmetic
  prepare_s        io.symmetrize_simple on the host (numpy), one call
--ab adds one short line per knob value ("ab": "truss_group=8", call_ms, support_ms and the statistics), timed on the same plan in
the same process right behind the default line (the knobs are read per call): truss_group 1 .. 64, truss_batch 1 / 16 / 64 / 256,
truss_grid 2 / 4 / 8 / 16, truss_spread 0 / 6 / 8 / 10 / 12 / 14.
--verify checks the result with app.validate_truss (both rules; the host peel enumerates every triangle: small graphs only).
Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG (truss_group, default 64; truss_batch, default 64; truss_grid, default 8; truss_spread, default 10)
and are recorded with every line.

    python benchmarks/bench_truss.py [--graphs googleplus,orkut] [--scale 0.125] [--verify] [--out profiles/truss.jsonl]
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

TRUSS_GROUP, TRUSS_BATCH, TRUSS_GRID, TRUSS_SPREAD = 64, 64, 8, 10       # the library's defaults (csrc/gl_truss.hip)


def _with_knob(key, value, fn):
    old = os.environ.get("GRAPHLILY_DEBUG", "")
    os.environ["GRAPHLILY_DEBUG"] = ",".join(x for x in (old, "%s=%s" % (key, value)) if x)
    try:
        return fn()
    finally:
        if old:
            os.environ["GRAPHLILY_DEBUG"] = old
        else:
            del os.environ["GRAPHLILY_DEBUG"]


AB = [("truss_group", v) for v in (1, 2, 4, 8, 16, 32, 64)] + [("truss_batch", v) for v in (1, 16, 64, 256)] + [("truss_grid", v) for v in (2, 4, 8, 16)] + \
    [("truss_spread", v) for v in (0, 6, 8, 10, 12, 14)]


def run_graph(name, raw, runs=5, verify=False, ab=False):
    from graphlily_amd import app, capi, io
    t0 = time.perf_counter()
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    sym, deg = io.symmetrize_simple(padded)
    prepare_s = time.perf_counter() - t0
    kt = app.KTruss(16, 0, 0)
    kt.set_up_runtime()
    kt.load_and_format_matrix(raw, True)
    kt.send_matrix_host_to_device()
    n, nnz = kt.n_, kt.graph_.nnz
    plan = kt.SpMV_.plan_
    truss, support, core = capi.DeviceBuffer(4 * max(1, nnz)), capi.DeviceBuffer(4 * max(1, nnz)), capi.DeviceBuffer(4 * n)
    capi.sync()
    t0 = time.perf_counter()
    stats = plan.truss(truss, support)          # (the plan's first call: the verdicts, the scratch and the edge numbering)
    first_call_ms = (time.perf_counter() - t0) * 1e3
    print("%s: first call %.1f ms, %d edges, %d sub-rounds" % (name, first_call_ms, stats[4], stats[2]), file=sys.stderr, flush=True)
    max_support = int(support.read(np.uint32, nnz).max()) if nnz else 0
    call_ms = wall_ms(lambda: plan.truss(truss), runs)
    support_ms = _with_knob("truss_support_only", 1, lambda: wall_ms(lambda: plan.truss(truss), runs))
    plan.truss(truss)
    run_ms = wall_ms(lambda: kt.run(), runs)
    assert np.array_equal(truss.read(np.uint32, nnz), kt.truss_) and (kt.max_truss_, kt.levels_, kt.sub_rounds_) == stats[:3]
    kstats = plan.kcore(core)
    kcore_ms = wall_ms(lambda: plan.kcore(core), runs)
    kcore_steps = kstats[0] + 1 + kstats[2]
    oriented, _ = io.triangle_orient(padded)
    tc_plan = capi.SpMVPlan(oriented.num_rows, oriented.num_cols, oriented.adj_indptr, oriented.adj_indices, oriented.adj_data, 0,
                            oriented.num_rows, flags=capi.GL_PLAN_BOOLEAN)
    total, per_vertex = capi.DeviceBuffer(8), capi.DeviceBuffer(8 * n)

    def tc():
        tc_plan.tc_count(total, per_vertex)
        capi.sync()
    tc_ms = wall_ms(tc, runs)
    assert int(total.read(np.uint64, 1)[0]) == stats[5], "gl_tc_count and gl_truss disagree on the triangles"
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    steps = stats[1] + stats[2]
    peel_ms = call_ms[0] - support_ms[0]
    rec = {"graph": name, "n": n, "nnz": raw.nnz, "symmetric_entries": nnz, "longest_row": int(deg.max()) if n else 0,
           "max_truss": stats[0], "levels": stats[1], "sub_rounds": stats[2], "launches": stats[3], "edges": stats[4], "triangles": stats[5],
           "max_support": max_support, "degeneracy": kstats[0],
           "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
           "first_call_ms": round(first_call_ms, 4), "support_ms": round(support_ms[0], 4), "tc_ms": round(tc_ms[0], 4),
           "peel_ms": round(peel_ms, 4), "steps": steps, "us_per_step": round(peel_ms * 1e3 / steps, 3) if steps else None,
           "kcore_call_ms": round(kcore_ms[0], 4), "kcore_steps": kcore_steps,
           "kcore_us_per_step": round(kcore_ms[0] * 1e3 / kcore_steps, 3) if kcore_steps else None,
           "edges_per_s": round(stats[4] / (call_ms[0] * 1e-3), 1) if call_ms[0] > 0 else None,
           "peeled_edges_per_s": round(stats[4] / (peel_ms * 1e-3), 1) if peel_ms > 0 else None,
           "run_ms": round(run_ms[0], 4), "runs": runs, "prepare_s": round(prepare_s, 3),
           "truss_group": int(knobs.get("truss_group", TRUSS_GROUP)), "truss_batch": int(knobs.get("truss_batch", TRUSS_BATCH)),
           "truss_grid": int(knobs.get("truss_grid", TRUSS_GRID)), "truss_spread": int(knobs.get("truss_spread", TRUSS_SPREAD)), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    if verify:
        rec["verified"] = app.validate_truss(padded, kt.truss_) == stats[0]
    yield rec
    for key, value in AB if ab else ():
        got = _with_knob(key, value, lambda: (plan.truss(truss), wall_ms(lambda: plan.truss(truss), runs)))
        assert got[0][:3] == stats[:3] and got[0][4:] == stats[4:] and np.array_equal(truss.read(np.uint32, nnz), kt.truss_)
        sup = _with_knob(key, value, lambda: _with_knob("truss_support_only", 1, lambda: wall_ms(lambda: plan.truss(truss), runs)))
        yield {"graph": name, "ab": "%s=%d" % (key, value), "call_ms": round(got[1][0], 4), "call_ms_min": round(got[1][1], 4),
               "call_ms_max": round(got[1][2], 4), "support_ms": round(sup[0], 4), "launches": got[0][3], "runs": runs,
               "max_truss": stats[0], "sub_rounds": stats[2], "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "truss.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--verify", action="store_true", help="check the result with app.validate_truss (small graphs only)")
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plan")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, runs=args.runs, verify=args.verify, ab=args.ab):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
