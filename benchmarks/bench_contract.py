#!/usr/bin/env python
"""Graph contraction (gl_contract_symbolic / gl_contract_numeric) on the stand-ins, one GPU, one process.

Per stand-in, on Louvain's own level-0 labels (one gl_louvain_move level under a largest-first colouring), two JSON lines:
  "contract"   contract_ms: SpMVModule.contract -- symbolic + numeric + the download of C, tot and part --, wall clock, median /
               min / max of `runs` after two untimed calls; host_ms: io.aggregate_communities on the same labels in the same
               process, median of three; k, nnz_c, and the groups per path of the symbolic and of the numeric call
  "louvain"    Louvain.run end to end with aggregate="device" and aggregate="host", ALTERNATING in one process after one untimed
               run of each: median / min / max of `runs` each, and timings_["aggregate"] of the last run of each
    python benchmarks/bench_contract.py [--graphs googleplus] [--scale 0.125] [--out profiles/contract.jsonl]
GRAPHLILY_DEBUG knobs are recorded with every line: one invocation per knob value.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(times):
    return {"median": round(float(np.median(times)), 3), "min": round(float(min(times)), 3), "max": round(float(max(times)), 3)}


def run_graph(name, raw, runs):
    from graphlily_amd import app, capi, io, module as M
    d = app.Louvain(M.num_hbm_channels, 1024, 256)
    d.set_target("hw")
    d.set_up_runtime("unused.xclbin")
    d.load_and_format_matrix(raw, True)
    d.send_matrix_host_to_device()
    base = {"graph": name, "n": int(d.graph_.num_rows), "nnz": int(d.graph_.nnz), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    end_to_end = {"device": [], "host": []}
    aggregate_s = {}
    for i in range(runs + 1):
        for how in ("device", "host"):
            t0 = time.perf_counter()
            labels = d.run(aggregate=how)
            if i:
                end_to_end[how].append(1e3 * (time.perf_counter() - t0))
            aggregate_s[how] = d.timings_["aggregate"]
    out = [dict(base, what="louvain", levels=int(d.levels_), device_ms=_stats(end_to_end["device"]), host_ms=_stats(end_to_end["host"]),
                aggregate_ms={how: round(1e3 * s, 3) for how, s in aggregate_s.items()}, communities=int(d.num_communities_))]
    # level 0 alone: the labels of the first dendrogram level, as smallest-member labels
    n = d.graph_.num_rows
    level0 = app._smallest_member_labels(d.dendrogram_[0], n) if d.levels_ else np.arange(n, dtype=np.uint32)
    label_buf = capi.DeviceBuffer.from_host(level0)
    times = []
    for i in range(runs + 2):
        t0 = time.perf_counter()
        c, w, tot, part, num = d.SpMV_.contract(label_buf)
        times.append(1e3 * (time.perf_counter() - t0))
    sym = d.SpMV_.plan_.contract_symbolic(n, label_buf, capi.DeviceBuffer(4 * n), capi.DeviceBuffer(4 * (n + 1)))
    host = []
    for i in range(3):
        t0 = time.perf_counter()
        want = io.aggregate_communities(d.graph_, None, None, level0)
        host.append(1e3 * (time.perf_counter() - t0))
    same = np.array_equal(c.adj_indices, want[0].adj_indices) and np.array_equal(w, want[1]) and np.array_equal(tot, want[2])
    out.append(dict(base, what="contract", k=int(num[0]), nnz_c=int(num[1]), equal_to_host=bool(same), contract_ms=_stats(times[2:]),
                    first_contract_ms=round(times[0], 3), host_ms=_stats(host), symbolic_paths=list(sym[3:5]), numeric_paths=list(num[3:5])))
    return out


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contract.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, raw, args.runs):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
