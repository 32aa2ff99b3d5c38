"""GPU parity: the element-wise apply modules vs the CPU oracle, following tests/test_module_apply.cpp."""
import numpy as np
import pytest

from graphlily_amd import capi, module as M
from oracle import oracle as O

from helpers import rand01

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("length", [128, 8, 1000003])
def test_add_scalar_vector_dense(gpu, length):
    # TEST(AddScalarVectorDense, Basic) :54-75 (length 128, val 1, in = (rand()%10)/100)
    inp = (np.random.default_rng(0).integers(0, 10, size=length) / 100.0).astype(np.float32)
    mod = M.eWiseAddModule()
    mod.set_up_runtime()
    mod.send_in_host_to_device(inp)
    mod.allocate_out_buf(length)
    mod.run(length, 1.0)
    assert np.array_equal(mod.send_out_device_to_host(), O.ewise_add(inp, length, 1.0))


@pytest.mark.parametrize("mask_type", [M.kMaskWriteToOne, M.kMaskWriteToZero])
@pytest.mark.parametrize("length", [128, 100001])
def test_assign_vector_dense(gpu, mask_type, length):
    # TEST(AssignVectorDense, Basic) :78-103 (length 128, val 23, WriteToOne)
    mask, inout = rand01(length, 1), rand01(length, 2)
    mod = M.AssignVectorDenseModule()
    mod.set_up_runtime()
    mod.set_mask_type(mask_type)
    mod.send_mask_host_to_device(mask)
    mod.send_inout_host_to_device(inout)
    mod.run(length, 23.0)
    ref = inout.copy()
    O.assign_dense(mask_type, mask, ref, length, 23.0)
    assert np.array_equal(mod.send_inout_device_to_host(), ref)


def test_assign_vector_dense_nomask_is_fatal(gpu):
    mod = M.AssignVectorDenseModule()
    with pytest.raises(SystemExit):
        mod.set_mask_type(M.kNoMask)          # assign_vector_dense_module.h:88-95
    with pytest.raises(capi.GraphLilyError) as e:
        capi.assign_dense(capi.DeviceBuffer(32), capi.DeviceBuffer(32), 8, 1.0, capi.GL_NOMASK)
    assert e.value.code == capi.GL_ERR_INVALID_ARG


def _strided_mask(inout_size, sparsity, seed):
    length = int(np.floor(inout_size * (1 - sparsity)))
    inc = inout_size // length
    vals = np.random.default_rng(seed).integers(0, 10, size=length).astype(np.float32)
    return M.make_sparse_vec(np.arange(length, dtype=np.uint32) * inc, vals)


@pytest.mark.parametrize("inout_size", [8192, 500000])
def test_assign_vector_sparse_no_new_frontier(gpu, inout_size):
    # TEST(AssignVectorSparseNoNewFrontier, Basic) :106-143 (n 8192, 10% dense mask, val 3)
    mask = _strided_mask(inout_size, 0.9, 0)
    inout = np.random.default_rng(1).integers(0, 10, size=inout_size).astype(np.float32)
    mod = M.AssignVectorSparseModule(False)
    mod.set_up_runtime()
    mod.send_mask_host_to_device(mask)
    mod.send_inout_host_to_device(inout)
    mod.run(3.0)
    ref = inout.copy()
    O.assign_sparse(mask, ref, 3.0)
    assert np.array_equal(mod.send_inout_device_to_host(), ref)
    with pytest.raises(SystemExit):
        mod.run()                              # wrong mode exits (assign_vector_sparse_module.h:296-300)


@pytest.mark.parametrize("inout_size,inf", [(128, 255.0), (300000, 999999999.0)])
def test_assign_vector_sparse_new_frontier(gpu, inout_size, inf):
    # TEST(AssignVectorSparseNewFrontier, Basic) :146-206 (n 128, inout in {5, inf})
    mask = _strided_mask(inout_size, 0.9, 2)
    inout = np.where(np.random.default_rng(3).integers(0, 10, size=inout_size) > 5, 5.0, inf).astype(np.float32)
    mod = M.AssignVectorSparseModule(True)
    mod.set_up_runtime()
    mod.send_mask_host_to_device(mask)
    mod.send_inout_host_to_device(inout)
    mod.run()
    ref = inout.copy()
    ref_nf = O.assign_sparse_new_frontier(mask, ref)
    assert np.array_equal(mod.send_inout_device_to_host(), ref)
    nf = mod.send_new_frontier_device_to_host()
    n = int(nf["index"][0])
    assert n == int(ref_nf["index"][0]) and nf["val"][0] == 0.0
    # this build keeps mask order, so the list itself (not just its densification) matches
    assert np.array_equal(nf[:n + 1], ref_nf)
    with pytest.raises(SystemExit):
        mod.run(1.0)


@pytest.mark.parametrize("cnt", [131072, 131073, 140000])
def test_assign_vector_sparse_new_frontier_long_lists(gpu, cnt):
    """The compaction on both sides of its 128-block limit (1024 candidates per block): 131 072 candidates are the longest
    list whose counts the counting launch scans itself, 131 073 and 140 000 (129 and 137 blocks) have every writing block
    add up the counts in front of it.  Twice on one module: the second run finds the ticket word and the counts as the
    first one left them."""
    mask = _strided_mask(2 * cnt, 0.5, 6)
    assert int(mask["index"][0]) == cnt
    inout = np.random.default_rng(7).integers(0, 10, size=2 * cnt).astype(np.float32)
    ref = inout.copy()
    ref_nf = O.assign_sparse_new_frontier(mask, ref)
    assert 0.3 * cnt < int(ref_nf["index"][0]) < 0.7 * cnt     # about half of the candidates relax
    mod = M.AssignVectorSparseModule(True)
    mod.set_up_runtime()
    mod.send_mask_host_to_device(mask)
    for _ in range(2):
        mod.send_inout_host_to_device(inout)
        mod.run()
        assert np.array_equal(mod.send_inout_device_to_host(), ref)
        nf = mod.send_new_frontier_device_to_host()
        n = int(nf["index"][0])
        assert n == int(ref_nf["index"][0]) and nf["val"][0] == 0.0
        assert np.array_equal(nf[:n + 1], ref_nf)


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 2048 * 256 + 3])
def test_fill_u32(gpu, count):
    """gl_buf_fill_u32 between two sentinel words: one thread per word up to 2048 blocks of 256, a grid-stride loop past that."""
    sentinel, value = 0xdeadbeef, 0x01234567
    whole = capi.DeviceBuffer.from_host(np.full(count + 2, sentinel, np.uint32))
    capi.fill_u32(capi.DeviceBuffer(4 * count, ptr=whole.ptr + 4, keepalive=whole), value, count)
    capi.sync()
    got = whole.read(np.uint32, count + 2)
    assert got[0] == sentinel and got[-1] == sentinel
    assert np.all(got[1:-1] == value)


def test_copy_buffer_bind_buffer(gpu):
    # TEST(CopyBufferBindBuffer, Basic) :209-261
    length = 128
    mask, inout = rand01(length, 4), np.zeros(length, np.float32)
    mod = M.AssignVectorDenseModule()
    mod.set_up_runtime()
    mod.set_mask_type(M.kMaskWriteToOne)
    mod.send_mask_host_to_device(mask)
    mod.send_inout_host_to_device(inout)
    mod.copy_buffer_device_to_device(mod.mask_buf, mod.inout_buf, 4 * length)
    assert np.array_equal(mod.send_inout_device_to_host(), mask)
    x_buf = capi.DeviceBuffer.from_host(np.zeros(length, np.float32))
    mod.send_mask_host_to_device(mask)
    mod.bind_inout_buf(x_buf)
    mod.run(length, 2.0)
    ref = np.zeros(length, np.float32)
    O.assign_dense(O.WRITETOONE, mask, ref, length, 2.0)
    assert np.array_equal(x_buf.read(np.float32), ref)


def test_sparse_to_dense(gpu):
    n = 100000
    sv = _strided_mask(n, 0.97, 5)
    cap = capi.DeviceBuffer(8 * (n + 1))
    cap.write(sv)
    dense = capi.DeviceBuffer(4 * n)
    capi.sparse_to_dense(cap, dense, n, 255.0, n)
    capi.sync()
    assert np.array_equal(dense.read(np.float32), O.convert_sparse_vec_to_dense_vec(sv, n, 255.0))


def test_pinned_readback(gpu):
    """gl_host_alloc: page-locked destination for device->host copies (DeviceBuffer.read(out=...))."""
    n = 300000
    src = np.arange(n, dtype=np.float32)
    buf = capi.DeviceBuffer.from_host(src)
    out = capi.pinned_empty(n, np.float32)
    got = buf.read(np.float32, n, out=out)
    assert np.array_equal(got, src) and np.shares_memory(got, out)


# ------------------------------------------------------------------ signed zeros, infinities, NaN and subnormals
_ODD = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-45, 1.5, -2.25, 3e38], np.float32)


def _same_outside_nan(got, want):
    """Bit-equal where `want` is not a NaN, a NaN where it is."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _shifted(nbytes, shift):
    """A device buffer that starts 4 bytes past a 16-byte boundary (shift) or on one."""
    whole = capi.DeviceBuffer(nbytes + 16)
    buf = capi.DeviceBuffer(nbytes, ptr=whole.ptr + (4 if shift else 0), keepalive=whole)
    assert (buf.ptr % 16 != 0) == shift
    return buf


@pytest.mark.parametrize("shift", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("length", [1, 3, 5, 1023, 4099])
def test_add_scalar_odd_values(gpu, length, shift):
    """gl_ewise_add on -0.0, +-inf, NaN and subnormals, with val = -1.5, -0.0, inf and NaN: the float4 body and its scalar
    tail (lengths that are no multiple of 4), and the scalar kernel a pointer off a 16-byte boundary selects."""
    rng = np.random.default_rng(length)
    inp = rng.choice(_ODD, size=length)
    inp[:min(length, _ODD.size)] = _ODD[:min(length, _ODD.size)]
    d_in, d_out = _shifted(4 * length, shift), _shifted(4 * length, shift)
    d_in.write(inp)
    for val in (-1.5, -0.0, np.inf, np.nan):
        capi.ewise_add(d_in, d_out, length, val)
        capi.sync()
        with np.errstate(all="ignore"):
            want = inp + np.float32(val)
        assert _same_outside_nan(d_out.read(np.float32, length), want), val
        assert _same_outside_nan(O.ewise_add(inp, length, val), want), val


@pytest.mark.parametrize("mask_type", [M.kMaskWriteToOne, M.kMaskWriteToZero])
@pytest.mark.parametrize("val", [-0.0, np.nan])
def test_assign_dense_odd_masks(gpu, mask_type, val):
    """gl_assign_dense with -0.0 (zero), NaN, a subnormal and -1 (all non-zero) in the mask; val = -0.0 / NaN written bit for bit."""
    length = 4099
    rng = np.random.default_rng(17)
    mask = rng.choice(np.array([0.0, -0.0, np.nan, 1e-40, -1.0, 1.0], np.float32), size=length)
    inout = rng.choice(_ODD, size=length)
    d_mask, d_inout = capi.DeviceBuffer.from_host(mask), capi.DeviceBuffer.from_host(inout)
    capi.assign_dense(d_mask, d_inout, length, val, mask_type)
    capi.sync()
    got = d_inout.read(np.float32, length)
    ref = inout.copy()
    O.assign_dense(mask_type, mask, ref, length, val)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    written = (mask == 0) if mask_type == M.kMaskWriteToZero else ~(mask == 0)
    assert 0.2 < written.mean() < 0.8
    assert np.all(got.view(np.uint32)[written] == np.float32(val).view(np.uint32))
    assert np.array_equal(got.view(np.uint32)[~written], inout.view(np.uint32)[~written])


def test_assign_sparse_new_frontier_odd_values(gpu):
    """gl_assign_sparse_new_frontier (keep and relax where inout > candidate) with negatives, -0.0 / 0.0 ties (not greater: not
    kept), NaN on either side (never greater: not kept) and +-inf; 140 000 unique candidates = more than 128 chunks, so the
    compaction's second pass over the chunk offsets runs.  The list and inout are the oracle's, bit for bit outside NaN."""
    n, cnt = 300000, 140000
    rng = np.random.default_rng(23)
    alphabet = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, -3.0, -1.0, 2.0, 5.0, 1e-40], np.float32)
    inout = rng.choice(alphabet, size=n)
    idx = np.sort(rng.choice(n, size=cnt, replace=False)).astype(np.uint32)
    mask = M.make_sparse_vec(idx, rng.choice(alphabet, size=cnt))
    mod = M.AssignVectorSparseModule(True)
    mod.set_up_runtime()
    mod.send_mask_host_to_device(mask)
    mod.send_inout_host_to_device(inout)
    mod.run()
    ref = inout.copy()
    ref_nf = O.assign_sparse_new_frontier(mask, ref)
    assert _same_outside_nan(mod.send_inout_device_to_host(), ref)
    nf = mod.send_new_frontier_device_to_host()
    k = int(nf["index"][0])
    assert k == int(ref_nf["index"][0]) and 0.2 * cnt < k < 0.8 * cnt and nf["val"][0] == 0.0
    assert np.array_equal(nf["index"][1:k + 1], ref_nf["index"][1:]) and not np.isnan(ref_nf["val"]).any()
    assert np.array_equal(nf["val"][1:k + 1].view(np.uint32), ref_nf["val"][1:].view(np.uint32))
    # ties and NaN: a candidate -0.0 never replaces 0.0 (nor the reverse), nothing replaces or is replaced by a NaN
    cand, old, new = mask["val"][1:], inout[idx], ref[idx]
    tie = (cand == 0) & (old == 0)
    assert tie.any() and np.array_equal(new.view(np.uint32)[tie], old.view(np.uint32)[tie])
    assert np.isnan(new[np.isnan(old)]).all() and not np.isnan(new[~np.isnan(old)]).any()
