"""The matrices and expectations of tests/test_gpu_bool_stream.py, proven on the CPU alone.

The (||,&&) layout (csrc/gl_spmv_bool.hip) streams its entries in one of three forms -- raw 4-byte entries, 3-byte entries with
8-bit column deltas, 3-byte entries with 10-bit deltas (bits 8..9 in the two spare bits of the 16-bit row slot) -- and which one a
plan takes depends on the gaps between the column-sorted entries of its groups of 256.  This module holds

  * `stream_matrix`: matrices whose gaps are chosen, per row block, from a cycle of listed values (the period is odd, so over the
    groups every value meets every position of a group);
  * `coder`: bool_compress_kernel restated in numpy on the raw stream, the predicted 768-byte groups bit for bit and the
    counts (bad, wide) the planner decides by;
  * `model_stream`: emit_bool_host's grouping of an unsplit plan restated, so that the coder's preconditions (which positions,
    lanes and row slots the wide deltas meet, interior padding, hub rows, phases) can be checked here, without a GPU.

The tests prove the constructor (the deltas of every block are exactly the intended values), the coder (its groups decode to the
raw stream they were made from) and that every case the GPU tests rely on is reached.  Needs no GPU."""
import functools

import numpy as np
import pytest

from graphlily_amd import io

GROUP = 256                          # kBoolGroup
ROW_PAD = 0x3fff                     # kRowPad: the ghost row slot of a padding entry
PHASE_COLS = 36864 * 32              # kBoolPhaseCols
OFFSET_LIMIT = 1 << 18               # 1 << kColOffBits: bit positions a group's entries may lie behind its base
HUB_BIT0 = 15360                     # kBoolHubBit0: row slots from here on are the private bits of hub rows
HUB_SLOTS, HUB_MAX = 32, 31
TALL = HUB_BIT0 - 64                 # the tallest plain block: its row slots use bit 13
NARROW_GAPS = (0, 1, 31, 32, 33, 255)
WIDE_GAPS = (256, 257, 511, 512, 768, 1023)
TOO_WIDE_GAP, FAR_GAP = 1024, 5000
RECT_COLS = 2 * PHASE_COLS + 600000  # three phases
SQUARE_BLOCKS = 80
SQUARE_N = SQUARE_BLOCKS * TALL      # 1 223 680: the smallest square shape with a second phase, i.e. with interior padding
HUB_ROW = 5
KINDS = ("narrow", "wide", "wide_hub", "extremes", "too_wide", "far")
ZERO_EXTRAS = 192                    # explicit 0.0 / -0.0 entries per block: dropped at format time, counted by the block cuts
ODD_X = np.array([0.0] * 30 + [1.0, -0.0, np.nan, -2.0, 1e-40], np.float32)     # one column in nine is on: rows of 1 .. 12 entries go both ways


def gap_cycle(kind):
    """The gaps between a block's column-sorted entries, one period: every listed value of the kind's classes, no two zeros next
    to each other, and a 1 that makes the period odd (7 or 25: coprime to the 256 entries of a group)."""
    if kind == "narrow":
        return np.array(NARROW_GAPS + (1,), np.int64)
    seq = []
    for j, g in enumerate(NARROW_GAPS * 3):
        seq.append(g)
        if j % 3 == 2:
            seq.append(WIDE_GAPS[j // 3])
    return np.array(seq + [1], np.int64)


def block_partition(rows, blocks):
    """`blocks` row ranges of whole 64-row groups, as equal as that allows (the taller ones first)."""
    g = rows // 64
    assert rows % 64 == 0 and g >= blocks
    sizes = [(g // blocks + (1 if b < g % blocks else 0)) * 64 for b in range(blocks)]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


class StreamMatrix:
    """m: the CSR; bstart: the row partition it was built for."""
    def __init__(self, m, bstart, kind, hub_row=None):
        self.m, self.bstart, self.kind, self.hub_row = m, bstart, kind, hub_row


def _patches(kind, block):
    """(first gap index, last + 1, value): the gaps of a block that differ from the cycle."""
    if kind == "extremes":          # entries 0 .. 255 and 256 .. 511 are the block's first two groups
        return [(1, 256, 255), (257, 512, 1023)]
    if kind == "too_wide" and block == 0:
        return [(100, 101, TOO_WIDE_GAP)]
    if kind == "far" and block == 0:
        return [(100, 101, FAR_GAP)]
    return []


def stream_matrix(kind, rows, cols, blocks, tree=False, seed=0):
    """`kind` of KINDS on `blocks` equal row blocks of a rows x cols matrix.  Every block's entries sit at columns that advance by
    gap_cycle (rotated by the block's number; `extremes`, `too_wide` and `far` overwrite some gaps, see _patches) from the block's
    first columns to the last, in random rows of the block -- every row of a block holds an entry when the block has as many
    entries as rows, and every block holds the same number of stored entries, so that the planner's cuts by non-zeros fall on this
    partition.  `wide_hub`: row HUB_ROW also holds the column of every entry that follows a gap of 256 or more.  `tree`: entry
    (i, i // 2) for every row (a square matrix becomes reachable from vertex 0 in 21 steps); no explicit zeros then, values 1.
    Otherwise the values mix 1.0, -3.5 and NaN, and ZERO_EXTRAS entries per block hold 0.0 / -0.0."""
    assert kind in KINDS
    rng = np.random.default_rng([seed, KINDS.index(kind), rows, blocks])
    base = "narrow" if kind == "narrow" else "wide"
    cycle = gap_cycle(base)
    bstart = block_partition(rows, blocks)
    extra = sum((hi - lo) * v for lo, hi, v in _patches(kind, 0))
    periods = (cols - 64 - extra) // int(cycle.sum())
    count = periods * len(cycle)
    keys, vals, fill = [], [], []
    for b in range(blocks):
        r0, R = int(bstart[b]), int(bstart[b + 1] - bstart[b])
        g = np.tile(np.roll(cycle, -b), periods)
        for lo, hi, v in _patches(kind, b):
            g[lo:hi] = v
        g[0] = 0
        c = (b % 32) + np.cumsum(g)
        assert c[-1] < cols
        r = rng.integers(0, R, size=count)
        if count >= R:
            r[:R] = rng.permutation(R)
        for _ in range(4):           # a gap of 0 is the same column in ANOTHER row; with `tree`, not the entry the tree holds
            same = np.flatnonzero((g == 0) & (r == np.roll(r, 1)))
            same = same[same > 0]
            r[same] = (r[same] + 1) % R
            if tree:
                hit = np.flatnonzero((r + r0) // 2 == c)
                r[hit] = (r[hit] + 2) % R
            if kind == "wide_hub" and b == 0:      # the hub row holds the entries placed below and no others
                r[r == HUB_ROW] = HUB_ROW + 3
        k = [(r + r0) * cols + c]
        if kind == "wide_hub" and b == 0:
            at = np.flatnonzero(g >= 256)
            k.append(HUB_ROW * cols + c[at])
        if tree:
            i = np.arange(r0, r0 + R, dtype=np.int64)
            k.append(i * cols + i // 2)
        k = np.concatenate(k)
        assert np.unique(k).size == k.size, "the construction repeats an entry"
        keys.append(k)
        vals.append(np.ones(k.size, np.float32) if tree else rng.choice(np.array([1.0, 1.0, -3.5, np.nan], np.float32), size=k.size))
        fill.append(k.size)
    # explicit zeros, and as many more as bring every block to the same number of stored entries
    for b in range(blocks):
        if tree:
            assert fill[b] == fill[0]
            continue
        r0, R = int(bstart[b]), int(bstart[b + 1] - bstart[b])
        want = ZERO_EXTRAS + max(fill) - fill[b]
        z = np.unique((rng.integers(0, R, size=2 * want) + r0) * cols + rng.integers(0, cols, size=2 * want))
        z = rng.permutation(np.setdiff1d(z, keys[b]))[:want]
        assert z.size == want
        keys.append(z)
        vals.append(rng.choice(np.array([0.0, -0.0], np.float32), size=want))
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    indptr = np.zeros(rows + 1, np.uint32)
    np.cumsum(np.bincount(keys // cols, minlength=rows), out=indptr[1:])
    m = io.CSRMatrix(rows, cols, vals, (keys % cols).astype(np.uint32), indptr)
    return StreamMatrix(m, bstart, kind, HUB_ROW if kind == "wide_hub" else None)


@functools.lru_cache(maxsize=None)
def rect(kind, blocks=1):
    """The rectangular shape of the SpMV tests: TALL rows (one block: the tallest plain one) by three phases of columns."""
    return stream_matrix(kind, TALL, RECT_COLS, blocks)


@functools.lru_cache(maxsize=None)
def square(kind="wide"):
    """The square shape of the BFS tests: SQUARE_BLOCKS blocks of TALL rows, a little over one phase of columns."""
    return stream_matrix(kind, SQUARE_N, SQUARE_N, SQUARE_BLOCKS, tree=True)


def odd_x(n, seed=3):
    """x of 0, -0.0, 1, NaN, -2 and a subnormal: && looks at x != 0 only."""
    return np.random.default_rng(seed).choice(ODD_X, size=n)


def block_deltas(sm, b):
    """The gaps between the column-sorted stored non-zero entries of block b."""
    m = sm.m
    lo, hi = int(m.adj_indptr[sm.bstart[b]]), int(m.adj_indptr[sm.bstart[b + 1]])
    c = np.sort(m.adj_indices[lo:hi][m.adj_data[lo:hi] != 0].astype(np.int64))
    return np.diff(c)


# ------------------------------------------------------------------ the coder, restated
def split_raw(raw):
    """Raw 4-byte entries -> (row slot, bit index behind the group's base, is padding), each groups x 256."""
    e = np.asarray(raw, np.uint32).reshape(-1, GROUP)
    row = (e >> 5) & ROW_PAD
    return row, ((e >> 19) << 5) | (e & 31), row == ROW_PAD


def coder_deltas(raw):
    """Per entry the distance to its predecessor's index (the first entry's: to 0) and per group whether it can be coded at
    all: a padding entry takes its predecessor's index; a group is bad if its real entries' indices go backwards or a
    delta exceeds 1023."""
    row, idx, pad = split_raw(raw)
    idx = idx.astype(np.int64)
    eff = np.maximum.accumulate(np.where(pad, 0, idx), axis=1)          # the running maximum of the real entries' indices
    backwards = np.any(~pad & (idx < eff), axis=1)
    d = np.diff(eff, axis=1, prepend=0)
    return row, d, pad, backwards | np.any(d > 1023, axis=1)


def coder(raw):
    """bool_compress_kernel on the raw stream -> (the 768-byte groups as bytes [groups, 64 lanes, 12], bad, wide): lane l holds the
    16-bit row slots of entries 4 l .. 4 l + 3, bits 8..9 of each entry's delta on top of its slot, then the four low delta bytes.
    bad: groups that cannot be coded; wide: codable groups with a delta above 255.  (A bad group's bytes are never looked at.)"""
    row, d, pad, bad = coder_deltas(raw)
    groups = row.shape[0]
    slots = (row | (((d >> 8) & 3) << 14)).astype(np.uint16).reshape(groups, 64, 4)
    out = np.empty((groups, 64, 12), np.uint8)
    out[:, :, :8] = slots.view(np.uint8).reshape(groups, 64, 8)         # (little-endian words, as the device writes them)
    out[:, :, 8:] = (d & 255).astype(np.uint8).reshape(groups, 64, 4)
    wide = np.any(d > 255, axis=1) & ~bad
    return out, int(bad.sum()), int(wide.sum())


def decode(coded):
    """The decoder's arithmetic on [groups, 64, 12] bytes -> (row slot, bit index), each groups x 256."""
    coded = np.ascontiguousarray(coded, np.uint8).reshape(-1, 64, 12)
    groups = coded.shape[0]
    slots = coded[:, :, :8].copy().view(np.uint16).reshape(groups, GROUP).astype(np.int64)
    d = coded[:, :, 8:].reshape(groups, GROUP).astype(np.int64) | ((slots >> 14) << 8)
    return slots & ROW_PAD, np.cumsum(d, axis=1)


def expected_form(bad, wide, knob):
    """What bool_plan_compress makes of a plan small enough for the Infinity Cache (every plan of a test is): knob 0 keeps the
    4-byte entries; knob 1 codes a plan without bad and without wide groups (8-bit deltas) and leaves one with wide groups raw --
    the 10-bit decoder only pays on a stream of more than 224 MB --; knob 3 codes whatever has no bad group, with the 10-bit decoder.
    -> 0 raw, 1 8-bit deltas, 2 10-bit deltas"""
    if knob == 0 or bad:
        return 0
    if knob == 3:
        return 2
    return 0 if wide else 1


def stream_facts(raw, group_unit):
    """What the GPU tests' preconditions ask of a formatted stream.  group_unit: the unit of every group."""
    row, d, pad, bad = coder_deltas(raw)
    big = (d >= 256) & ~bad[:, None]
    at = np.flatnonzero(big.any(axis=0))
    interior = False
    gu = np.asarray(group_unit)
    for g in np.flatnonzero(pad.any(axis=1)):
        later = np.flatnonzero(gu[g + 1:] == gu[g]) + g + 1
        if later.size and np.any(~pad[later]):
            interior = True
            break
    return {"bad": int(bad.sum()), "wide": int((np.any(d > 255, axis=1) & ~bad).sum()),
            "in_lane": sorted(set((at % 4).tolist())), "lanes": sorted(set((at // 4).tolist())),
            "bit13": bool(np.any(big & ((row & 0x2000) != 0) & ~pad)), "interior_padding": interior,
            "all_255": int(np.sum(np.all(d[:, 1:] == 255, axis=1))), "all_1023": int(np.sum(np.all(d[:, 1:] == 1023, axis=1))),
            "max_index": int(np.cumsum(d, axis=1).max())}


DPP_LANES = (0, 15, 16, 31, 32, 47, 48, 63)       # the row boundaries of bool_wave_scan's DPP steps


def assert_wide_preconditions(f, what):
    assert f["bad"] == 0 and f["wide"] > 0, (what, f)
    assert f["in_lane"] == [0, 1, 2, 3], (what, f)
    assert set(DPP_LANES) <= set(f["lanes"]), (what, f)
    assert f["bit13"], (what, f)


def group_units(units, spans, groups):
    """The unit of every group, from a plan's exported `units` (2 x uint4 per unit) and `spans` (uint4 each)."""
    u, s = np.asarray(units).reshape(-1, 8), np.asarray(spans).reshape(-1, 4)
    out = np.full(groups, -1, np.int64)
    for k in range(u.shape[0]):
        for sp in s[u[k, 0]:u[k, 0] + u[k, 1]]:
            out[sp[1]:sp[2]] = k
    assert np.all(out >= 0), "a group that no span names"
    return out


# ------------------------------------------------------------------ the formatter's grouping, restated (unsplit plans)
def model_stream(sm):
    """emit_bool_host for one unit per block of sm.bstart -> (raw entries, the unit of every group, hub rows per block, phases per
    block): a block's stored non-zero entries sorted by column (stable: ties in row order); a group ends after 256 entries, at a
    phase boundary or when an entry lies 2^18 bit positions behind the group's base (the x word of its first entry), and is
    padded with ghost entries; rows with at least max(256, entries / 48) entries are hub rows."""
    m = sm.m
    ip = m.adj_indptr.astype(np.int64)
    raw, gunit, hubs, nph = [], [], [], []
    for b in range(len(sm.bstart) - 1):
        r0, r1 = int(sm.bstart[b]), int(sm.bstart[b + 1])
        lo, hi = ip[r0], ip[r1]
        keep = m.adj_data[lo:hi] != 0
        col = m.adj_indices[lo:hi][keep].astype(np.int64)
        rowl = (np.repeat(np.arange(r0, r1), np.diff(ip[r0:r1 + 1]))[keep] - r0).astype(np.int64)
        order = np.argsort(col, kind="stable")
        col, rowl = col[order], rowl[order]
        cnt = np.bincount(rowl, minlength=r1 - r0)
        hub = np.flatnonzero(cnt >= max(256, col.size // 48))[:HUB_MAX]
        hub_of = np.full(r1 - r0, -1, np.int64)
        hub_of[hub] = np.arange(hub.size)
        hubs.append(hub)
        ph = col // PHASE_COLS
        cin = col - ph * PHASE_COLS
        cuts = np.flatnonzero(np.diff(ph)) + 1
        nph.append(cuts.size + 1 if col.size else 0)
        for s, e in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [col.size]])):
            while s < e:
                base = cin[s] & ~31
                t = min(e, s + GROUP, s + int(np.searchsorted(cin[s:e], base + OFFSET_LIMIT, side="left")))
                fill = np.arange(t - s)
                h = hub_of[rowl[s:t]]
                slot = np.where(h < 0, rowl[s:t], HUB_BIT0 + (fill & (HUB_SLOTS - 1)) * 32 + h)
                off = cin[s:t] - base
                g = np.full(GROUP, ROW_PAD << 5, np.int64)
                g[:t - s] = ((off >> 5) << 19) | (slot << 5) | (off & 31)
                raw.append(g)
                gunit.append(b)
                s = t
    return np.concatenate(raw).astype(np.uint32), np.array(gunit), hubs, nph


@functools.lru_cache(maxsize=None)
def model_facts(kind, shape):
    sm = square(kind) if shape == "square" else rect(kind)
    raw, gunit, hubs, nph = model_stream(sm)
    f = stream_facts(raw, gunit)
    f["hubs"], f["phases"], f["groups"] = [h.tolist() for h in hubs], max(nph), gunit.size
    return f, raw


# ------------------------------------------------------------------ tests
def test_gap_cycles_are_odd_and_hold_every_listed_value():
    for kind, want in (("narrow", NARROW_GAPS), ("wide", NARROW_GAPS + WIDE_GAPS)):
        c = gap_cycle(kind)
        assert len(c) % 2 == 1 and np.gcd(len(c), GROUP) == 1
        assert set(c.tolist()) == set(want)
        z = np.flatnonzero(c == 0)
        assert not np.any(np.diff(z) == 1) and not (c[0] == 0 and c[-1] == 0)


@pytest.mark.parametrize("kind,shape,blocks", [(k, "rect", b) for k in KINDS for b in (1, 3)] + [("wide", "square", SQUARE_BLOCKS)])
def test_constructed_gaps_are_exactly_the_intended_ones(kind, shape, blocks):
    """For the partition it was given: every block's sorted-column deltas hold each listed value of the kind's classes and nothing
    else (the hub row repeats columns: more zeros; the tree splits gaps: only in the square shape, where the listed values must
    all still occur and nothing above 1023 may); every block stores the same number of entries, its first row is not empty, and
    the explicit zeros are there."""
    sm = square(kind) if shape == "square" else rect(kind, blocks)
    m = sm.m
    ip = m.adj_indptr.astype(np.int64)
    per = np.diff(ip[sm.bstart])
    assert np.all(per == per[0]) and len(sm.bstart) == blocks + 1
    assert np.all(np.diff(ip)[sm.bstart[:-1]] > 0)
    if blocks > 1:
        assert np.all(np.diff(ip) > 0), "a cut by non-zeros falls on the partition only if no row next to it is empty"
    listed = set(NARROW_GAPS) if kind == "narrow" else set(NARROW_GAPS + WIDE_GAPS)
    for b in range(blocks):
        d = block_deltas(sm, b)
        seen = set(np.unique(d).tolist())
        want = set(listed)
        if kind == "too_wide" and b == 0:
            want.add(TOO_WIDE_GAP)
            assert int((d == TOO_WIDE_GAP).sum()) == 1
        if kind == "far" and b == 0:
            want.add(FAR_GAP)
            assert int((d == FAR_GAP).sum()) == 1
        if shape == "square":
            assert want <= seen and max(seen) <= 1023, (b, sorted(seen - want))
        else:
            assert seen == want, (kind, b, sorted(seen ^ want))
    if shape == "rect":
        zeros = m.adj_data[:m.nnz] == 0
        assert zeros.sum() >= ZERO_EXTRAS * blocks and np.signbit(m.adj_data[:m.nnz][zeros]).any() and not np.signbit(m.adj_data[:m.nnz][zeros]).all()
        assert np.isnan(m.adj_data).any() and (m.adj_data == np.float32(-3.5)).any()
        assert int(m.adj_indices.max()) // PHASE_COLS == 2
    if kind == "wide_hub":
        lo, hi = ip[HUB_ROW], ip[HUB_ROW + 1]
        own = np.diff(np.sort(m.adj_indices[lo:hi][m.adj_data[lo:hi] != 0].astype(np.int64)))
        assert hi - lo >= max(256, per[0] // 48) and np.all(own[own > 0] >= 256) and (own >= 256).sum() > 256


def test_the_coder_on_groups_written_by_hand():
    ent = lambda off, row: ((off >> 5) << 19) | (row << 5) | (off & 31)
    g = np.full((4, GROUP), ROW_PAD << 5, np.int64)
    g[0, :3] = [ent(7, 1), ent(7, 2), ent(262, 0x2001)]                 # deltas 7, 0, 255, then padding: delta 0
    g[1, :4] = [ent(0, 9), ent(256, 9), ent(256 + 1023, 3), ent(256 + 1023 + 768, 4)]
    g[2, :3] = [ent(31, 0), ent(31 + 1024, 0), ent(2000, 0)]            # too wide
    g[3, :3] = [ent(40, 0), ent(39, 1), ent(41, 2)]                     # backwards
    g[1, 2] = ROW_PAD << 5                                              # an interior padding entry: its predecessor's index
    out, bad, wide = coder(g.astype(np.uint32).reshape(-1))
    assert (bad, wide) == (3, 0)
    assert out[0, 0].tolist() == [1, 0, 2, 0, 0x01, 0x20, 0xff, 0x3f, 7, 0, 255, 0] and not out[0, 1:, 8:].any()
    # group 1: the padding entry hides index 1279, so the fourth entry lies 1791 behind the second: bad until it moves up
    row, d, pad, isbad = coder_deltas(g.astype(np.uint32).reshape(-1))
    assert d[1, :4].tolist() == [0, 256, 0, 1791] and isbad.tolist() == [False, True, True, True]
    g[1, 3] = ent(256 + 1023, 4)
    out, bad, wide = coder(g.astype(np.uint32).reshape(-1))
    assert (bad, wide) == (2, 1)
    assert out[1, 0].tolist() == [9, 0, 9, 0x40, 0xff, 0x3f, 4, 0xc0, 0, 0, 0, 0xff]
    slots, idx = decode(out[:2])
    assert slots[1, :4].tolist() == [9, 9, ROW_PAD, 4] and idx[1, :4].tolist() == [0, 256, 256, 1279]
    assert [expected_form(b, w, k) for b, w, k in ((0, 0, 0), (0, 0, 1), (0, 0, 3), (0, 2, 1), (0, 2, 3), (1, 0, 1), (1, 2, 3))] == [0, 1, 2, 0, 2, 0, 0]


@pytest.mark.parametrize("kind,shape", [(k, "rect") for k in KINDS] + [("wide", "square")])
def test_the_modelled_streams_reach_what_the_gpu_tests_rely_on(kind, shape):
    """The formatter's grouping restated on every unsplit case: the coder's verdict per kind, its groups decode to the raw
    entries, and the wide cases put a delta of 256 or more at every in-lane position, at the lanes on both sides of every DPP row
    boundary and into a row slot with bit 13; padding inside a unit, three phases (two in the square shape), the hub row."""
    f, raw = model_facts(kind, shape)
    out, bad, wide = coder(raw)
    assert (bad, wide) == (f["bad"], f["wide"])
    if kind == "narrow":
        assert bad == 0 and wide == 0
    elif kind in ("too_wide", "far"):
        assert bad == 1
    else:
        assert_wide_preconditions(f, (kind, shape))
    assert f["interior_padding"] and f["phases"] == (2 if shape == "square" else 3)
    assert f["max_index"] < OFFSET_LIMIT
    assert (f["hubs"][0] == [HUB_ROW]) if kind == "wide_hub" else not any(f["hubs"])
    if kind == "extremes":
        assert f["all_255"] == 1 and f["all_1023"] == 1 and f["max_index"] >= 255 * 1023
    row, idx, pad = split_raw(raw)
    ok = ~coder_deltas(raw)[3]
    slots, didx = decode(out)
    assert np.array_equal(slots[ok], row[ok])
    assert np.array_equal(didx[ok][~pad[ok]], idx[ok][~pad[ok]])
    hi = (out[:, :, :8].copy().view(np.uint16) >> 14).reshape(-1, GROUP)
    assert bool(hi[ok].any()) == (wide > 0)
