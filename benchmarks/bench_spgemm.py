#!/usr/bin/env python
"""SpGEMM (gl_spgemm_symbolic / gl_spgemm_numeric): A A on the stand-ins, one GPU, one process.

A is the undirected simple graph of a stand-in (io.symmetrize_simple), every value 1.  Per stand-in three JSON lines -- "unmasked"
and "masked_by_A" under (+,x), "andor" under (||,&&) without a mask:
  symbolic_ms      the symbolic call, which waits: wall clock around it, median of `runs` after one untimed call (the plan's first)
  numeric_ms       the numeric call by HIP events on the library's stream, median / min / max of `runs` after three untimed runs
  products, nnz_c, rows per path (symbolic: by the product bound; numeric: by |C(i)|)
  products_per_s   products / (symbolic_ms + numeric_ms)
  model_bytes      what the model moves: A's row copy once, 4 bytes of B's columns per product in both calls and 4 more of B's
                   values in a numeric call with values, the mask rows once per call, C's offsets, columns and values once
  torch_ms         torch.sparse.mm on the same operands (CSR, f32) where torch accepts them, else null: a point of comparison
                   that no threshold rests on
    python benchmarks/bench_spgemm.py [--graphs googleplus] [--scale 0.125] [--out profiles/spgemm.jsonl]
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

from bench_clique import span_stats  # noqa: E402


def torch_ms(g, dev, runs):
    import torch
    try:
        t = torch.sparse_csr_tensor(torch.from_numpy(g.adj_indptr.astype(np.int64)), torch.from_numpy(g.adj_indices.astype(np.int64)),
                                    torch.from_numpy(g.adj_data), size=(g.num_rows, g.num_cols)).to(dev)
        times = []
        for i in range(runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.sparse.mm(t, t)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return round(float(np.median(times[1:])), 4)
    except Exception:                                            # (a layout or a size this torch build refuses)
        return None


def run_graph(name, raw, dev, runs=9):
    from graphlily_amd import capi, io, module as M
    g, _ = io.symmetrize_simple(raw)
    n = g.num_rows
    plan = capi.SpMVPlan(n, n, g.adj_indptr, g.adj_indices, g.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    val = capi.DeviceBuffer.from_host(g.adj_data)
    indptr = capi.DeviceBuffer(4 * (n + 1))
    torch_time = torch_ms(g, dev, 3)
    out = []
    for what, op, mask in (("unmasked", M.kMulAdd, None), ("masked_by_A", M.kMulAdd, plan), ("andor", M.kLogicalAndOr, None)):
        base = {"graph": name, "what": what, "n": n, "nnz_a": g.nnz, "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
        try:
            times = []
            for i in range(runs + 1):
                t0 = time.perf_counter()
                sym = plan.spgemm_symbolic(plan, indptr, mask)
                times.append(1e3 * (time.perf_counter() - t0))
        except capi.GraphLilyError as e:                         # (nnz(C) >= 2^32)
            out.append(dict(base, unsupported=str(e)))
            continue
        nnz = sym[0]
        idx, cval = capi.DeviceBuffer(4 * max(1, nnz)), capi.DeviceBuffer(4 * max(1, nnz))
        num = plan.spgemm_numeric(plan, op, val, val, indptr, idx, cval, mask, stats=True)
        med, lo, hi = span_stats(lambda: plan.spgemm_numeric(plan, op, val, val, indptr, idx, cval, mask), runs)
        symbolic_ms = float(np.median(times[1:]))
        valued = op != M.kLogicalAndOr
        model = (2 * (4 * (n + 1) + 4 * g.nnz) + 8 * sym[1] + (4 * sym[1] + 4 * g.nnz if valued else 0) + (2 * 4 * g.nnz if mask else 0)
                 + 2 * 4 * (n + 1) + 4 * nnz + (4 * nnz if valued else 0))
        out.append(dict(base, nnz_c=nnz, products=sym[1], symbolic_paths=list(sym[2:]), numeric_paths=list(num[2:]),
                        symbolic_ms=round(symbolic_ms, 4), first_symbolic_ms=round(times[0], 4), numeric_ms=round(med, 4),
                        numeric_min_ms=round(lo, 4), numeric_max_ms=round(hi, 4), model_bytes=model,
                        products_per_s=round(sym[1] / (1e-3 * (symbolic_ms + med)), 1) if symbolic_ms + med > 0 else None,
                        torch_ms=torch_time if what == "unmasked" else None))
    return out


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm.jsonl"))
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, dev, runs=args.runs):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
