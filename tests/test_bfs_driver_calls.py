"""The launch sequence of BFS's device-resident schedule driver (app.BFS._pull_push_bits) against a recording stand-in for the C
API: every capi call with its arguments (buffers by allocation order and offset), the results and the driver's state after every
call, under a synthetic clock that drives the packed-or-float choice.  One-GPU runs, emulated ranks with and without the copy
exchange, sliced and all-gathered read-backs, a communicator that cannot be captured, GRAPHLILY_BFS_U8 0 / 1 / 2,
GRAPHLILY_BFS_STREAM 0 / 1, timed calls, 4 / 5 / 6 / 20 / 300 iterations on one object and a failing capture.  The expected log
(tests/golden/bfs_driver_calls.json.gz) was recorded from the driver as one inline function, before it was split into phases:
a change of the driver's structure must leave it as it is.  No GPU."""
import contextlib
import gzip
import json
import os
import random

import numpy as np

from graphlily_amd import app, capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfs_driver_calls.json.gz")
LOG = []
CLOCK = [0.0]
RND = random.Random(7)


def lab(a):
    if isinstance(a, Buf):
        return a.label
    if isinstance(a, np.ndarray):
        return "nd%s%s" % (a.dtype, a.shape)
    if isinstance(a, (list, tuple)):
        return [lab(x) for x in a]
    if isinstance(a, float):
        return repr(a)
    if isinstance(a, (int, str, bool)) or a is None:
        return a
    return type(a).__name__


def rec(name, *a):
    LOG.append([name] + [lab(x) for x in a])


class Buf:
    count = 0

    def __init__(self, nbytes=0, ptr=None, keepalive=None, label=None):
        if label is None:
            Buf.count += 1
        self.nbytes, self.tensor = nbytes, None
        self.label = label or "buf%d[%d]" % (Buf.count, nbytes)
        self.ptr = 0

    @staticmethod
    def from_host(arr):
        b = Buf(arr.nbytes)
        rec("from_host", b, arr)
        return b

    def read_async(self, out, offset=0):
        rec("read_async", self, out, offset)


class Backend:
    def alloc(self, count, dtype):
        b = Buf(count * np.dtype(dtype).itemsize)
        rec("alloc", b)
        return b

    def view(self, buf, first, count, itemsize):
        return Buf(count * itemsize, label="%s+%d:%d" % (buf.label, first * itemsize, count * itemsize))

    def sync(self):
        rec("sync")
        CLOCK[0] += RND.uniform(0.3, 0.6)

    def fill(self, *a):
        rec("fill", *a)

    def init(self):
        pass

    def __getattr__(self, name):
        if name.endswith("Module"):
            return lambda *a: Mod(name)
        raise AttributeError(name)


class Plan:
    handle = 1


class Mod:
    def __init__(self, name):
        self.name, self.plan_ = name, Plan()

    def bits_words(self):
        return (N_ROWS + 31) // 32

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


class Graph:
    fail = False

    def __init__(self):
        self.id = None

    @staticmethod
    @contextlib.contextmanager
    def capture():
        g = Graph()
        rec("capture_begin")
        yield g
        if Graph.fail:
            rec("capture_fail")
            raise capi.GraphLilyError(1, "no capture")
        rec("capture_end")

    def launch(self):
        rec("graph_launch")


def fake(name, ret=None, dt=None):
    def f(*a):
        rec(name, *a)
        if dt:
            CLOCK[0] += RND.uniform(*dt)
        return ret(*a) if callable(ret) else ret
    return f


def ctlwords(*a):
    n = a[-1]
    return (np.arange(n, dtype=np.uint32) * 7 + len(LOG)) % 1000


def install(monkeypatch):
    """the stand-ins, for this test only"""
    del LOG[:]
    CLOCK[0], Buf.count, Graph.fail = 0.0, 0, False
    RND.seed(7)
    for var in ("GRAPHLILY_BFS_U8", "GRAPHLILY_BFS_STREAM"):
        monkeypatch.delenv(var, raising=False)
    put = lambda name, value: monkeypatch.setattr(capi, name, value)      # noqa: E731
    put("DeviceBuffer", Buf)
    put("Graph", Graph)
    for nm in ("bfs_bits_begin", "bfs_bits_shard_step", "bfs_bits_shard_finish", "fill_u32", "levels_pack", "levels_pack_stream",
               "levels_stream_arm", "span_begin"):
        put(nm, fake(nm))
    put("span_end", fake("span_end", 0.25))
    put("host_unpack_threads", lambda: 8)
    put("levels_stream_bytes", lambda n, bits, tw: n * bits // 8 + 4 * tw + 4096)
    put("pinned_empty", lambda count, dtype: np.zeros(count, dtype))
    put("pinned_recycled", lambda count, dtype: np.arange(count, dtype=dtype) % 13)
    put("sync_levels_unpack_stream", fake("sync_levels_unpack_stream", ctlwords, (0.3, 0.6)))
    put("sync_levels_unpack", fake("sync_levels_unpack", None, (0.3, 0.6)))
    monkeypatch.setattr(app, "time", type("T", (), {"perf_counter": staticmethod(lambda: CLOCK[0])}))


class Comm:
    def __init__(self, world=1, rank=0, emulated=False, copy=False, capturable=True):
        self.world_size, self.rank, self.copy = world, rank, copy
        self.distributed = world > 1
        if emulated:
            self.emulated = True
        if capturable:
            self.capturable = True

    def truth_vector(self, k):
        return Buf(label="truth%d" % k)

    def truth_tally(self, key, slots, bounds, col_len, row_len, n):
        rec("truth_tally", key, slots, list(bounds), n)
        return Buf(label="tallytable")

    def exchange_bits(self, bits, k, bounds, tally, slot):
        rec("exchange_bits", bits, k, list(bounds), tally, slot)

    def all_gather_slices(self, t, bounds):
        rec("all_gather_slices", t, list(bounds))


N_ROWS = 1 << 21


def make(comm):
    b = app.BFS(16, 0, 0, 0, comm=comm, backend=Backend())
    n = N_ROWS
    b.n_ = n
    W = comm.world_size
    b.bounds_ = [n * r // W for r in range(W + 1)]
    b.r0_, b.r1_ = b.bounds_[comm.rank], b.bounds_[comm.rank + 1]
    b.col_len_ = np.ones(n, np.uint32)
    b.row_len_ = np.ones(n, np.uint32)
    b.nnz_global_ = 12345678
    return b


def state(b):
    st = b.bits_loop_
    return {"result_range": list(b.result_range_), "readback": getattr(b, "readback_", None), "push": b.push_iterations_, "again": b.push_iterations_again_,
            "counts": b.bfs_slot_counts_.tolist(), "modes": b.bfs_slot_modes_.tolist(), "sched_ms": getattr(b, "schedule_ms_", None),
            "levels": [lab(x) for x in b.levels_], "lev8_key": list(st.get("lev8_key") or []), "h8": None if st.get("h8") is None else st["h8"].shape[0],
            "graphs": sorted(bool(v) for v in st["graphs"].values()), "graph_error": st.get("graph_error"), "N": st["N"], "ctl_words": st["ctl_words"],
            "words": st["words"]}


def call(b, mode, src, N, thr=0.001):
    LOG.append(["CALL", mode, src, N, thr, os.environ.get("GRAPHLILY_BFS_U8"), os.environ.get("GRAPHLILY_BFS_STREAM")])
    d = b._pull_push_bits(src, N, thr) if mode == "pp" else b._pull_push_bits(src, N, -1.0, pull_only=True)
    LOG.append(["RESULT", lab(d), float(d[:5].sum()), state(b)])


def scenario(monkeypatch, comm, gather=True):
    b = make(comm)
    b.gather_result_ = gather
    for k in range(75):
        call(b, "pp", 5, 6)
        if k % 3 == 0:
            call(b, "pull", 5, 6)
    b.time_schedule_ = True
    call(b, "pp", 5, 6)
    call(b, "pull", 7, 6)
    b.time_schedule_ = False
    for u8 in ("0", "2", "1"):
        monkeypatch.setenv("GRAPHLILY_BFS_U8", u8)
        for _ in range(4):
            call(b, "pp", 9, 6)
    monkeypatch.delenv("GRAPHLILY_BFS_U8")
    for stream in ("0", "1", "0"):
        monkeypatch.setenv("GRAPHLILY_BFS_STREAM", stream)
        for _ in range(4):
            call(b, "pp", 9, 6)
            call(b, "pull", 9, 20)      # bytes, and a larger state
    monkeypatch.delenv("GRAPHLILY_BFS_STREAM")
    for _ in range(3):
        call(b, "pull", 1, 300)     # no packing
        call(b, "pp", 1, 4, 0.05)   # smaller N on the larger state
    Graph.fail = True
    for _ in range(4):
        call(b, "pp", 1, 5, 0.05)
    Graph.fail = False


def test_driver_enqueues_what_the_inline_driver_did(monkeypatch):
    install(monkeypatch)
    scenario(monkeypatch, Comm())
    scenario(monkeypatch, Comm(4, 1, emulated=True), gather=False)
    scenario(monkeypatch, Comm(4, 2, emulated=True, copy=True), gather=False)
    scenario(monkeypatch, Comm(4, 2, emulated=True, copy=True), gather=True)
    scenario(monkeypatch, Comm(2, 1, capturable=False), gather=False)
    scenario(monkeypatch, Comm(2, 0, capturable=False), gather=True)
    got = json.loads(json.dumps(LOG))
    with gzip.open(GOLDEN, "rt") as f:
        want = json.load(f)
    assert len(got) == len(want) == 21287
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "entry %d" % k
