"""GPU: every coded form of the boolean layout's entry stream (csrc/gl_spmv_bool.hip) -- raw 4-byte entries, 8-bit deltas, 10-bit
deltas -- in every consumer of the stream, on the constructed matrices of tests/test_bool_stream_cpu.py, bit for bit against the
oracle.  The planner takes the 10-bit decoder on its own only for streams of more than 224 MB; GRAPHLILY_DEBUG bool_compress=3
takes it on any plan whose groups can be coded, and bool_keep=0 / 1 picks the kernels' cache-hint twin that the plan's size would
pick only between 64 MB and 224 MB.  Expectations come from the numpy restatement of the coder applied to the stream that was
actually formatted, and every case asserts on that stream that it reaches what it is there for."""
import functools

import numpy as np
import pytest

from graphlily_amd import app, capi, io, module as M
from graphlily_amd.dist import EmulatedComm
from oracle import oracle as O

from helpers import MASKS, rand01, set_knob, to_oracle
from test_bool_stream_cpu import (GROUP, HUB_ROW, SQUARE_BLOCKS, assert_wide_preconditions, coder, expected_form, group_units, odd_x,
                                  rect, square, stream_facts)

pytestmark = pytest.mark.gpu

HOST, DEV = capi.GL_PLAN_HOST_FORMAT, capi.GL_PLAN_DEVICE_FORMAT
KNOBS = (0, 1, 3)
RUN_KINDS = ("narrow", "wide", "wide_hub", "extremes", "too_wide")
SHAPES = {"unsplit": (1, 1), "split": (3, 4)}          # (spmv_blocks, spmv_segments); the matrix is built for that many row blocks
BFS_ITERS = 24


def _knobs(monkeypatch, blocks, segments, compress, keep=None):
    set_knob(monkeypatch, "spmv_blocks", blocks)
    set_knob(monkeypatch, "spmv_segments", segments)
    set_knob(monkeypatch, "bool_compress", compress)
    set_knob(monkeypatch, "bool_keep", keep)


def _plan(m, flags=0):
    return capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data, 0, m.num_rows, flags=capi.GL_PLAN_BOOLEAN | flags)


def _facts(plan):
    """The coder's verdict on a RAW plan's stream and what the wide deltas meet in it."""
    groups = plan.info()["groups"]
    raw = plan.export("entries")
    assert raw.nbytes == groups * GROUP * 4, "bool_compress=0 keeps the 4-byte entries"
    f = stream_facts(raw, group_units(plan.export("units"), plan.export("spans"), groups))
    f["groups"] = groups
    return f, raw


def _assert_form(plan, raw_plan, raw, predicted, form, what):
    """`plan` holds the stream of raw_plan in `form` (0 raw, 1 / 2 coded), every other array unchanged."""
    groups = raw_plan.info()["groups"]
    ent = plan.export("entries")
    assert plan.info()["groups"] == groups, what
    if form == 0:
        assert np.array_equal(ent, raw), "%s: the plan must keep the 4-byte stream, bit for bit" % (what,)
        assert plan.info()["device_bytes"] == raw_plan.info()["device_bytes"], what
    else:
        assert ent.nbytes == groups * 768, what
        got = ent.view(np.uint8).reshape(groups, 64, 12)
        if not np.array_equal(got, predicted):
            g = np.flatnonzero((got != predicted).any(axis=(1, 2)))
            raise AssertionError("%s: %d of %d coded groups differ from the restatement, first %d: lane 0 holds %s, predicted %s" %
                                 (what, g.size, groups, g[0], got[g[0], 0].tolist(), predicted[g[0], 0].tolist()))
        assert plan.info()["device_bytes"] == raw_plan.info()["device_bytes"] - groups * 256, what
    for nm in ("bases", "units", "hub_rows", "spans"):
        assert np.array_equal(raw_plan.export(nm), plan.export(nm)), (what, nm)


def _check_preconditions(kind, shape, f, raw_plan, what):
    """What the case is there for, read from the plan that was formatted (a failure here is a failure of the test)."""
    if kind == "narrow":
        assert f["bad"] == 0 and f["wide"] == 0, (what, f)
    elif kind in ("too_wide", "far"):
        assert f["bad"] == 1, (what, f)
    elif shape == "unsplit":
        assert_wide_preconditions(f, what)
    else:
        assert f["bad"] == 0 and f["wide"] > 0, (what, f)
    info = raw_plan.info()
    assert (info["segments"] > 1) == (shape == "split") and info["blocks"] == SHAPES[shape][0], (what, info)
    units = raw_plan.export("units").reshape(-1, 8)
    assert np.unique(raw_plan.export("spans").reshape(-1, 4)[:, 0]).size >= 3, "%s: the spans cover three phases" % (what,)
    if shape == "unsplit":
        assert int(units[:, 1].max()) >= 3 and f["interior_padding"], what
    if kind == "wide_hub":
        assert units[0, 5] == 1 and raw_plan.export("hub_rows")[units[0, 4]] == HUB_ROW, what
    else:
        assert not units[:, 5].any(), what
    if kind == "extremes" and shape == "unsplit":
        assert f["all_255"] == 1 and f["all_1023"] == 1 and f["max_index"] >= 255 * 1023, (what, f)


@pytest.mark.parametrize("where", [HOST, DEV], ids=["host", "device"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", RUN_KINDS + ("far",))
def test_each_knob_gives_the_form_the_restatement_predicts(gpu, kind, shape, where, monkeypatch):
    """bool_plan_compress under bool_compress = 0 / 1 / 3 with both formatters.  0: raw.  1: coded (8-bit deltas) only if no group
    is bad and none is wide -- a plan with wide groups stays raw, the 10-bit decoder being kept for streams of more than 224 MB.
    3: coded whenever no group is bad, with bits 8..9 of the wide deltas on the row slots.  Coded bytes equal the restatement's;
    device_bytes drops by 256 per group exactly when coded; bases, units, hub rows and spans never change."""
    blocks, segments = SHAPES[shape]
    sm = rect(kind, blocks)
    what = "%s/%s" % (kind, shape)
    _knobs(monkeypatch, blocks, segments, 0)
    raw_plan = _plan(sm.m, where)
    f, raw = _facts(raw_plan)
    _check_preconditions(kind, shape, f, raw_plan, what)
    predicted, bad, wide = coder(raw)
    assert (bad, wide) == (f["bad"], f["wide"])
    for knob in (1, 3):
        _knobs(monkeypatch, blocks, segments, knob)
        form = expected_form(bad, wide, knob)
        assert form == {"narrow": {1: 1, 3: 2}, "too_wide": {1: 0, 3: 0}, "far": {1: 0, 3: 0}}.get(kind, {1: 0, 3: 2})[knob]
        p = _plan(sm.m, where)
        _assert_form(p, raw_plan, raw, predicted, form, "%s knob %d" % (what, knob))
        hi = (p.export("entries").view(np.uint8).reshape(-1, 64, 12)[:, :, :8].copy().view(np.uint16) >> 14) if form else np.zeros(1)
        assert bool(hi.any()) == (form == 2 and wide > 0), (what, knob)


@functools.lru_cache(maxsize=None)
def _run_inputs(kind, blocks):
    """x, mask and the oracle's six results of a rectangular case, computed once."""
    m = rect(kind, blocks).m
    x, mask = odd_x(m.num_cols), rand01(m.num_rows, 4)
    om = to_oracle(m)
    refs = {(mk, zero): O.spmv(om, x, 1, zero, mask if MASKS[mk] else None, MASKS[mk]) for mk in MASKS for zero in (0.0, 1.0)}
    assert 0.05 < refs[("NoMask", 0.0)].mean() < 0.95, "both outcomes of || must occur"
    return x, mask, refs


@pytest.mark.parametrize("keep", [None, 0, 1], ids=["keep_by_size", "keep0", "keep1"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", RUN_KINDS)
def test_plan_run_under_every_form_equals_the_oracle(gpu, kind, shape, keep, monkeypatch):
    """gl_spmv_run on (||,&&) with every mask and zero = 0 / 1, on the raw, the 8-bit and the 10-bit stream (launch_bool_variant:
    KEEP 0, 2, 6; with bool_keep=1 the twins without the non-temporal hint, KEEP 1, 3, 7), unsplit and split: each equals the
    oracle and therefore the other forms, bit for bit."""
    blocks, segments = SHAPES[shape]
    m = rect(kind, blocks).m
    x, mask, refs = _run_inputs(kind, blocks)
    dx, dm = capi.DeviceBuffer.from_host(x), capi.DeviceBuffer.from_host(mask)
    forms, first = {}, {}
    for knob in KNOBS:
        _knobs(monkeypatch, blocks, segments, knob, keep)
        p = _plan(m)
        if knob == 0:
            f, raw = _facts(p)
            _check_preconditions(kind, shape, f, p, (kind, shape))
        forms[knob] = {1024: 0, 768: 1 + (knob == 3)}[p.export("entries").nbytes // p.info()["groups"]]
        assert forms[knob] == expected_form(f["bad"], f["wide"], knob)
        for mk in MASKS:
            for zero in (0.0, 1.0):
                dy = capi.DeviceBuffer.from_host(np.full(m.num_rows, 7.0, np.float32))
                p.run(dx, dm if MASKS[mk] else None, dy, 1, zero, MASKS[mk])
                got = dy.read(np.float32, m.num_rows)
                ref = refs[(mk, zero)]
                assert np.array_equal(got, ref), "%s/%s knob %d keep %s %s zero %g: %d rows differ, first %d" % (
                    kind, shape, knob, keep, mk, zero, int((got != ref).sum()), int(np.flatnonzero(got != ref)[0]))
                assert np.array_equal(got.view(np.uint32), first.setdefault((mk, zero), got).view(np.uint32)), "the forms differ from one another"
    assert forms[0] == 0 and (forms[3] == 2 or kind == "too_wide")


# ------------------------------------------------------------------ BFS on the square graph
@functools.lru_cache(maxsize=None)
def _bfs_reference(kind):
    g = square(kind).m
    om = to_oracle(g.copy())
    O.util_round_csr_matrix_dim(om, 128, 128)
    om.adj_data = np.ones(om.nnz, np.float32)
    ref = O.bfs(om, 0, BFS_ITERS)
    assert om.num_rows == g.num_rows and np.all(ref != 0) and ref.max() > 8, "every vertex is reached, over many levels"
    return ref


def _square_facts(monkeypatch, blocks, segments=1, r0=0, r1=None, kind="wide"):
    """Preconditions on the square graph's plan (or a row shard's), as the BFS driver formats it."""
    g = square(kind).m
    _knobs(monkeypatch, blocks, segments, 0)
    p = capi.SpMVPlan(g.num_rows, g.num_cols, g.adj_indptr, g.adj_indices, np.ones(g.nnz, np.float32), r0, g.num_rows if r1 is None else r1,
                      flags=capi.GL_PLAN_BOOLEAN | capi.GL_PLAN_NO_MULADD)
    f, _ = _facts(p)
    assert p.info()["blocks"] == blocks
    return f, p.info()


def _assert_stream_form(plan, form):
    ent, groups = plan.export("entries"), plan.info()["groups"]
    assert ent.nbytes == groups * (768 if form else 1024)
    if form == 2:
        assert (ent.view(np.uint8).reshape(groups, 64, 12)[:, :, :8].copy().view(np.uint16) >> 14).any(), "no delta of the plan uses bits 8..9"


def _bfs(g, comm=None):
    b = app.BFS(16, 0, 0, 0, comm=comm)
    b.set_up_runtime()
    b.load_and_format_matrix(g, True)
    b.send_matrix_host_to_device()
    return b


@pytest.mark.parametrize("keep", [None, 1], ids=["keep_by_size", "keep1"])
@pytest.mark.parametrize("knob", KNOBS)
def test_bfs_on_the_wide_square_graph(gpu, knob, keep, monkeypatch):
    """app.BFS pull / push / pull_push on the square `wide` graph (the fused pull epilogue, FUSED == 1): the oracle's levels under
    every knob; with bool_keep=1 the pull once more (KEEP 1 / 7)."""
    ref = _bfs_reference("wide")
    f, info = _square_facts(monkeypatch, SQUARE_BLOCKS)
    assert_wide_preconditions(f, "square")
    assert f["interior_padding"] and info["segments"] == 1
    _knobs(monkeypatch, SQUARE_BLOCKS, 1, knob, keep)
    bfs = _bfs(square().m)
    _assert_stream_form(bfs.SpMV_.plan_, expected_form(f["bad"], f["wide"], knob))
    assert np.array_equal(bfs.pull(0, BFS_ITERS), ref), "pull"
    if keep is None:
        assert np.array_equal(bfs.push(0, BFS_ITERS), ref), "push"
        for thr in (0.1, 0.001):
            assert np.array_equal(bfs.pull_push(0, BFS_ITERS, thr), ref), "pull_push %g" % thr


def _rank(g, k, world, whole):
    comm = EmulatedComm(k, world, copy=(k % 2 == 1))
    b = _bfs(g, comm)
    b.gather_result_ = False
    st = whole.bits_loop_
    comm.set_truth(st["vecs"], st["words"])
    return b


@pytest.mark.parametrize("world,segments", [(2, 1), (4, 1), (4, 3)], ids=["world2", "world4", "world4_split"])
def test_shard_steps_on_the_wide_square_graph(gpu, world, segments, monkeypatch):
    """Every rank of a row-sharded BFS on the 10-bit stream (bool_compress=3): the one-launch shard step (launch_shard_step<1, 6>)
    and, on shard plans cut into column segments, the claiming epilogue of the bit-frontier schedule (FUSED == 2).  One rank at a
    time on one GPU, the exchange emulated from a whole-matrix run; every rank's levels equal the oracle's."""
    ref = _bfs_reference("wide")
    g = square().m
    per = SQUARE_BLOCKS // world
    _knobs(monkeypatch, SQUARE_BLOCKS, 1, 3)
    whole = _bfs(g)
    assert np.array_equal(whole.pull(0, BFS_ITERS), ref)
    for k in range(world):
        f, info = _square_facts(monkeypatch, per, segments, k * g.num_rows // world, (k + 1) * g.num_rows // world)
        assert f["bad"] == 0 and f["wide"] > 0 and (info["segments"] > 1) == (segments > 1), (k, f, info)
        _knobs(monkeypatch, per, segments, 3)
        b = _rank(g, k, world, whole)
        assert (b.r0_, b.r1_) == (k * g.num_rows // world, (k + 1) * g.num_rows // world)
        assert (b.SpMV_.plan_.info()["segments"] > 1) == (segments > 1)
        _assert_stream_form(b.SpMV_.plan_, 2)
        for mode in ("pull", "pull_push"):
            run_whole = (lambda: whole.pull(0, BFS_ITERS)) if mode == "pull" else (lambda: whole.pull_push(0, BFS_ITERS, 0.001))
            assert np.array_equal(run_whole(), ref)          # (the truth vectors are the whole run's, rewritten by every run)
            got = b.pull(0, BFS_ITERS) if mode == "pull" else b.pull_push(0, BFS_ITERS, 0.001)
            r0, r1 = b.result_range_
            assert (r0, r1) == (b.r0_, b.r1_)
            assert np.array_equal(got, ref[r0:r1]), "rank %d/%d %s: %d rows differ" % (k, world, mode, int((got != ref[r0:r1]).sum()))
        del b


@pytest.mark.parametrize("segments", [1, 3], ids=["unsplit", "split"])
@pytest.mark.parametrize("keep", [0, 1], ids=["keep0", "keep1"])
@pytest.mark.parametrize("kind,knob,form", [("wide", 0, 0), ("narrow", 1, 1), ("wide", 3, 2)], ids=["raw", "8bit", "10bit"])
def test_shard_step_under_every_coding_and_cache_hint(gpu, kind, knob, form, keep, segments, monkeypatch):
    """The one-launch shard step's streaming pull under each stream coding, both cache-hint twins and both epilogues
    (launch_shard_step<1 / 2, KEEP 0 .. 7>: the sharded tests above and in test_gpu_bfs_sharded.py leave bool_keep to the plan's
    size, which is never the keeping twin's, and the 8-bit coding to the graph): rank 1 of 4 pulls in every slot."""
    world, k = 4, 1
    ref = _bfs_reference(kind)
    g = square(kind).m
    per = SQUARE_BLOCKS // world
    _knobs(monkeypatch, SQUARE_BLOCKS, 1, knob)
    whole = _bfs(g)       # (the exchange is emulated from this run's bit vectors)
    assert np.array_equal(whole.pull(0, BFS_ITERS), ref)
    f, info = _square_facts(monkeypatch, per, segments, k * g.num_rows // world, (k + 1) * g.num_rows // world, kind)
    assert expected_form(f["bad"], f["wide"], knob) == form and (info["segments"] > 1) == (segments > 1), (f, info)
    _knobs(monkeypatch, per, segments, knob, keep)
    b = _rank(g, k, world, whole)
    assert (b.SpMV_.plan_.info()["segments"] > 1) == (segments > 1)
    _assert_stream_form(b.SpMV_.plan_, form)
    got = b.pull(0, BFS_ITERS)
    r0, r1 = b.result_range_
    assert (r0, r1) == (b.r0_, b.r1_) == (k * g.num_rows // world, (k + 1) * g.num_rows // world)
    assert np.array_equal(got, ref[r0:r1]), "%d rows differ" % int((got != ref[r0:r1]).sum())


def test_spmspv_row_wise_leg_on_the_10_bit_stream(gpu, monkeypatch):
    """gl_spmspv_run's direction switch with the rectangular `wide` matrix attached as a 10-bit plan (bool_plan_run_bits): a
    frontier that holds most columns goes row-wise and gives the oracle's result under every mask."""
    sm = rect("wide")
    _knobs(monkeypatch, 1, 1, 0)
    f, _ = _facts(_plan(sm.m))
    assert_wide_preconditions(f, "wide")
    _knobs(monkeypatch, 1, 1, 3)
    csr = sm.m
    csc = io.csr2csc(csr)
    spmv = M.SpMVModule(16, 0, 0)
    spmv.set_semiring(M.LogicalSemiring)
    spmv.set_up_runtime()
    spmv.load_and_format_matrix(csr, True)
    spmv.send_matrix_host_to_device()
    _assert_stream_form(spmv.plan_, 2)
    # a dense x: nine columns in ten, five in seven of them on (the direction switch counts the non-zeros of the columns that are on)
    rng = np.random.default_rng(10)
    idx = np.flatnonzero(rng.random(csc.num_cols) < 0.9).astype(np.uint32)
    v = M.make_sparse_vec(idx, rng.choice(np.array([1.0, 1.0, -2.0, np.nan, 1e-40, 0.0, -0.0], np.float32), size=idx.size))
    mask = rand01(csc.num_rows, 5)
    oc = to_oracle(csc)
    for mk in MASKS:
        mod = M.SpMSpVModule(0)
        mod.set_semiring(M.LogicalSemiring)
        mod.set_mask_type(MASKS[mk])
        mod.set_up_runtime()
        mod.load_and_format_matrix(csc)
        mod.send_matrix_host_to_device()
        mod.attach_pull(spmv)
        mod.send_mask_host_to_device(mask)
        mod.send_vector_host_to_device(v)
        ref = O.spmspv(oc, v, 1, 0.0, mask, MASKS[mk])
        assert 0.02 < ref.mean() < 0.98
        for rep in range(2):
            mod.run()
            assert mod.plan_.last_direction() == "row-wise"
            got = M.convert_sparse_vec_to_dense_vec(mod.send_results_device_to_host(), csc.num_rows, 0.0)
            assert np.array_equal(got, ref), "%s run %d: %d rows differ" % (mk, rep, int((got != ref).sum()))
