"""bench.py's contract: a plain run times exactly --steps steps and prints the headline keys only; --dump-outputs writes the
result of the last timed step; everything else comes with --full (the tests that read those legs pass it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_the_last_result(gpu, tmp_path):
    """--steps 7 --warmup 2 at a small scale: the line holds the headline keys with steps = 7, none of the --full legs, and
    DIR/y.npy equals y = A x of the benchmark's own (seeded) inputs, recomputed here in float64."""
    import scipy.sparse as sp
    import torch
    from graphlily_amd import datasets, io
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--scale", "0.02",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "GB/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    for k in ("roofline", "selfcheck_ok", "bfs", "spmspv", "six_graphs", "cpu_baseline", "pattern_plan", "host_buffers"):
        assert k not in rec, k

    # the benchmark's inputs, rebuilt the way bench.py builds them
    dev = torch.device("cuda", 0)
    csr = datasets.paper_graph("orkut", 0.02, device=dev)
    csr.adj_data = np.full(csr.nnz, np.float32(1.0 / csr.num_rows), dtype=np.float32)
    io.util_round_csr_matrix_dim(csr, 16 * 8, 8)
    assert rec["config"]["n"] == csr.num_rows and rec["config"]["nnz"] == csr.nnz
    gen = torch.Generator(device=dev)
    gen.manual_seed(42)
    x = torch.randint(0, 2, (csr.num_cols,), generator=gen, device=dev).float().cpu().numpy()
    A = sp.csr_matrix((csr.adj_data.astype(np.float64), csr.adj_indices.astype(np.int64), csr.adj_indptr.astype(np.int64)),
                      shape=(csr.num_rows, csr.num_cols))
    ref = A @ x.astype(np.float64)
    y = np.load(str(out_dir / "y.npy"))
    assert y.dtype == np.float32 and y.shape == (csr.num_rows,)
    assert np.allclose(y, ref, rtol=1e-5, atol=1e-12)
    assert np.count_nonzero(y) > csr.num_rows // 4
