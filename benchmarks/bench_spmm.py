#!/usr/bin/env python
"""SpMM (gl_spmm): Y = A X for a dense block of k vectors on the stand-ins under (+,x), one GPU, one process, against the way the
workload is served without it: k SpMVModule.run calls on the same matrix.

Per (stand-in, k) one JSON line:
  spmm_ms          one gl_spmm call by HIP events on the library's stream: median / min / max of `runs` after three untimed calls
  spmv_k_ms        k SpMVModule.run calls (non-blocking, the plan of the module's choice for (+,x)), timed the same way; the two are
                   ALTERNATED run by run, so that both see the same neighbours on the machine
  speedup          spmv_k_ms / spmm_ms (medians)
  paths            rows on the short / wavefront / workgroup path, column tiles
  model_bytes      what the model moves: A's offsets, columns and values once per column tile, X once per column tile at least,
                   Y once; model_gbs = model_bytes / spmm_ms
Columns 0 and k - 1 of Y are checked with app.validate_spmm before anything is timed.
    python benchmarks/bench_spmm.py [--graphs googleplus] [--scale 0.125] [--ks 4,16,64,256] [--out profiles/spmm.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    from graphlily_amd import capi
    capi.span_begin()
    fn()
    return capi.span_end()


def run_graph(name, g, ks, runs=9):
    from graphlily_amd import app, capi, module as M
    n, nc = g.num_rows, g.num_cols
    rng = np.random.default_rng(7)
    spmv = M.SpMVModule()
    spmv.set_semiring(M.ArithmeticSemiring)
    spmv.load_and_format_matrix(g)
    spmv.send_matrix_host_to_device()
    spmv.send_vector_host_to_device(rng.standard_normal(nc).astype(np.float32))
    spmv.blocking = False
    mm = M.SpMMModule()
    mm.set_semiring(M.ArithmeticSemiring)
    mm.load_and_format_matrix(g)
    mm.send_matrix_host_to_device()
    out = []
    for k in ks:
        x = rng.standard_normal((nc, k)).astype(np.float32)
        mm.send_vectors_host_to_device(x)
        mm.run()
        y = mm.send_results_device_to_host()
        cols = sorted({0, k - 1})
        app.validate_spmm(g, x[:, cols], y[:, cols], M.ArithmeticSemiring)
        plan, a_val, xb, yb = mm.plan_, mm.a_val_buf, mm.vectors_buf, mm.results_buf

        def spmm_once():
            plan.spmm(a_val, xb, yb, k, M.kMulAdd, 0.0)

        def spmv_k():
            for _ in range(k):
                spmv.run()
        for _ in range(3):
            timed(spmm_once), timed(spmv_k)
        t_mm, t_mv = [], []
        for _ in range(runs):
            t_mm.append(timed(spmm_once))
            t_mv.append(timed(spmv_k))
        tiles = mm.stats_[3]
        model = tiles * (4 * (n + 1) + 8 * g.nnz) + 4 * nc * k + 4 * n * k
        med_mm, med_mv = float(np.median(t_mm)), float(np.median(t_mv))
        out.append({"graph": name, "k": k, "n": n, "nnz": g.nnz, "knobs": os.environ.get("GRAPHLILY_DEBUG", ""), "paths": list(mm.stats_),
                    "spmm_ms": round(med_mm, 4), "spmm_min_ms": round(min(t_mm), 4), "spmm_max_ms": round(max(t_mm), 4),
                    "spmv_k_ms": round(med_mv, 4), "spmv_k_min_ms": round(min(t_mv), 4), "spmv_k_max_ms": round(max(t_mv), 4),
                    "speedup": round(med_mv / med_mm, 3) if med_mm > 0 else None, "model_bytes": model,
                    "model_gbs": round(model / (1e-3 * med_mm) / 1e9, 1) if med_mm > 0 else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--ks", default="4,16,64,256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm.jsonl"))
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        g = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, g, [int(k) for k in args.ks.split(",")], runs=args.runs):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
