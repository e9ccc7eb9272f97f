"""Byte ranges of batch segments (dc_gpu.h "Huffman batch v1: byte ranges") without a device: the
exported entry points and their host argument checks, and the chunk arithmetic of
csrc/dc_batch_range.h as the library compiles it (dc_huff_batch_range_chunks /
dc_huff_batch_range_args) held against a Python restatement and against the CPU oracle: cutting
the oracle's stream at the summed u16 entries and decoding the chunks the library names gives the
wanted bytes. (The header's own exhaustive check, under the host sanitizers, is
tests/c/batch_range_check.c.)
chunk_interval, segment_ranges and batch_ranges are shared with tests/test_gpu_batch_ranges.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_batch_cpu import SEGMENTS, oracle_segment

DC_E_ARG = -1
RANGES_MAX = 1 << 28   # DC_RANGES_MAX
DC_E_CAPACITY = -6
ENTRY_POINTS = ("dc_huff_decode_batch_ranges", "dc_huff_decode_batch_shared_ranges", "dc_huff_batch_range_chunks",
                "dc_huff_batch_range_args")


def chunk_interval(first, count, S):
    """[c_lo, c_hi): the chunks of S symbols that hold a byte of [first, first + count)."""
    lo = first // S
    return (lo, lo) if count == 0 else (lo, (first + count - 1) // S + 1)


def lib_chunk_interval(first, count, S):
    """The same by the library: csrc/dc_batch_range.h as the kernels compile it."""
    from data_compression_amd._lib import core
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    assert core().dc_huff_batch_range_chunks(first, count, S, C.byref(lo), C.byref(hi)) == 0
    return lo.value, hi.value


def segment_ranges(n, S):
    """The (first, count) ranges of the issue for a segment of n bytes, those that fit it."""
    last = (n - 1) // S * S if n else 0   # the last chunk's first byte
    mid = last + (n - last) // 2
    want = [(0, 0), (n, 0), (0, 1), (n - 1, 1), (0, n),
            (S - 1, 2), (S, S), (S + 1, S - 1),
            (mid, n - mid),
            (63 * S - 1, S + 2),
            (5, 64 * S), (5, 64 * S + 1)]
    return [(f, c) for f, c in want if f >= 0 and c >= 0 and f + c <= n]


def batch_ranges(segs, S, seed=7, nrandom=200):
    """The range list of the GPU test as (seg, first, count) rows: segment_ranges of every segment;
    (3, 8192) and (3, 8193) of every segment that holds them, once in a group of four that has both
    kinds (the list is padded with empty ranges to place them) and once (3, 8192) in a group of
    four short ranges; then `nrandom` seeded random ranges."""
    rows = []
    for i, s in enumerate(segs):
        rows += [(i, f, c) for f, c in segment_ranges(s.size, S)]
        if s.size >= 3 + 8193:
            while len(rows) % 4 != 1:
                rows.append((i, 0, 0))
            rows += [(i, 3, 8192), (i, 3, 8193)]
            while len(rows) % 4 != 0:
                rows.append((i, 0, 0))
            rows += [(i, 3, 8192), (i, S, S), (i, 0, 1), (i, 3, 8192)]
    rng = np.random.default_rng(seed)
    full = [i for i, s in enumerate(segs) if s.size]
    for k in range(nrandom):
        i = full[int(rng.integers(len(full)))]
        n = segs[i].size
        f = int(rng.integers(n))
        most = n - f if k % 8 == 0 else min(n - f, 600)   # one in eight may be long
        rows.append((i, f, int(rng.integers(1, most + 1))))
    return np.array(rows, np.int64)


def test_entry_points_are_exported_and_declared():
    from data_compression_amd._lib import core
    L = core()
    for name in ENTRY_POINTS:
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is C.c_int, name
    assert len(L.dc_huff_decode_batch_ranges.argtypes) == 11
    assert len(L.dc_huff_decode_batch_shared_ranges.argtypes) == 12


def _batch(count=0):
    """An HBatch whose arrays are host dummies: the argument checks read no array."""
    from data_compression_amd._lib import HBatch
    b = HBatch()
    b.count, b.n_ary, b.sync_syms = count, 2, 64
    if count:
        dummy = C.create_string_buffer(64)
        p = (C.addressof(dummy) + 15) & ~15   # d_payload must be 16-B aligned
        for f in ("d_lens", "d_mode", "d_bits", "d_pay_off", "d_payload", "d_sync_off", "d_sync_len", "d_status"):
            setattr(b, f, p)
        b.payload_cap = b.sync_cap = 16
        b._keep = dummy
    return b


def _calls(L, ctx, b, tab, arrays, nranges, out=None, cap=0):
    """(own tables, shared) return codes; arrays: seg_off, seg, first, count, out_off, rstatus."""
    so, sg, fi, co, oo, rs = arrays
    bp = C.byref(b) if b is not None else None
    return (L.dc_huff_decode_batch_ranges(ctx, bp, so, sg, fi, co, oo, nranges, out, cap, rs),
            L.dc_huff_decode_batch_shared_ranges(ctx, bp, tab, so, sg, fi, co, oo, nranges, out, cap, rs))


@pytest.fixture()
def dummies():
    keep = [C.create_string_buffer(64) for _ in range(8)]
    ptr = [C.cast(k, C.c_void_p) for k in keep]
    return {"ctx": ptr[0], "tab": ptr[1], "arrays": ptr[2:8], "keep": keep}   # never read: a check fails first


def test_null_arguments_are_argument_errors(dummies):
    from data_compression_amd._lib import core
    L = core()
    d, b = dummies, _batch(3)
    # the context, the batch, the table
    assert _calls(L, None, b, d["tab"], d["arrays"], 1) == (DC_E_ARG, DC_E_ARG)
    assert _calls(L, d["ctx"], None, d["tab"], d["arrays"], 1) == (DC_E_ARG, DC_E_ARG)
    so, sg, fi, co, oo, rs = d["arrays"]   # (the shared call alone: the other would go on to read the context)
    assert L.dc_huff_decode_batch_shared_ranges(d["ctx"], C.byref(b), None, so, sg, fi, co, oo, 1, None, 0, rs) == DC_E_ARG
    assert _calls(L, None, b, d["tab"], d["arrays"], 0) == (DC_E_ARG, DC_E_ARG)   # hbatch_args comes before nranges
    # each array in turn, rstatus last
    for k in range(6):
        arrays = list(d["arrays"])
        arrays[k] = None
        assert _calls(L, d["ctx"], b, d["tab"], arrays, 1) == (DC_E_ARG, DC_E_ARG), k
        assert _calls(L, d["ctx"], _batch(0), d["tab"], arrays, 1) == (DC_E_ARG, DC_E_ARG), k
    # no output buffer for a capacity
    assert _calls(L, d["ctx"], b, d["tab"], d["arrays"], 1, None, 5) == (DC_E_ARG, DC_E_ARG)


def test_no_ranges_is_ok_without_a_launch(dummies):
    """The context is a host dummy: a launch, or any read of it, would not return DC_OK."""
    from data_compression_amd._lib import core
    L = core()
    d = dummies
    none = [None] * 6
    for b in (_batch(0), _batch(3)):
        assert _calls(L, d["ctx"], b, d["tab"], none, 0) == (0, 0)
        assert _calls(L, d["ctx"], b, d["tab"], d["arrays"], 0) == (0, 0)


def test_too_many_ranges_is_an_argument_error(dummies):
    from data_compression_amd._lib import core
    L = core()
    d = dummies
    for n in (RANGES_MAX + 1, 1 << 40, (1 << 64) - 1):
        assert _calls(L, d["ctx"], _batch(3), d["tab"], d["arrays"], n) == (DC_E_ARG, DC_E_ARG), n


def _bits(payload):
    return np.unpackbits(np.ascontiguousarray(payload, np.uint8))   # MSB first, as the stream


@pytest.mark.parametrize("S", (16, 64))
def test_chunk_interval_cuts_the_oracle_stream(S):
    """One 4097-byte segment: for every range of segment_ranges, with [c_lo, c_hi) as the library
    computes it (and as chunk_interval restates it), the bits from the sum of the entries before
    c_lo, for the sum of the entries of [c_lo, c_hi), decode (orc.huff_unpack) to the symbols of
    those chunks, and the range is their slice."""
    seg = SEGMENTS[10]
    assert seg.size == 4097
    lens, mode, bits, payload, sl = oracle_segment(seg, 2, S)
    assert mode == 1 and sl.size == -(-seg.size // S) and int(sl.astype(np.int64).sum()) == bits
    L = np.zeros(259, np.int32)
    L[:256] = lens
    el, ev = orc.canonical(L, 2)
    stream = _bits(payload)
    start = np.concatenate(([0], np.cumsum(sl.astype(np.int64))))
    ranges = segment_ranges(seg.size, S)
    assert (63 * S - 1, S + 2) in ranges and (0, seg.size) in ranges
    assert S != 16 or (5, 64 * S + 1) in ranges   # (at S = 64 the segment is too short for it)
    for first, count in ranges:
        c_lo, c_hi = lib_chunk_interval(first, count, S)
        assert (c_lo, c_hi) == chunk_interval(first, count, S)
        assert c_lo <= c_hi <= sl.size
        if count == 0:
            assert c_lo == c_hi
            continue
        assert c_lo * S <= first < (c_lo + 1) * S and (c_hi - 1) * S < first + count <= c_hi * S
        nsym = min(c_hi * S, seg.size) - c_lo * S
        cut = stream[start[c_lo]: start[c_hi]]
        got = orc.huff_unpack(np.packbits(cut), cut.size, nsym, el, ev, 2)
        assert np.array_equal(got, seg[c_lo * S: c_lo * S + nsym]), (first, count)
        assert np.array_equal(got[first - c_lo * S: first - c_lo * S + count], seg[first: first + count]), (first, count)


def test_batch_ranges_place_both_kinds_in_a_group():
    rows = batch_ranges(SEGMENTS, 64)
    assert len(rows) > 200 + 12 * 10
    groups = [rows[k: k + 4, 2] for k in range(0, len(rows) - 3, 4)]
    assert any((g == 8192).any() and (g == 8193).any() for g in groups)       # a workgroup group with a wave-sized range in it
    assert any((g == 8192).sum() == 2 and g.max() == 8192 for g in groups)    # a wave group at the threshold
    n = np.array([SEGMENTS[i].size for i in rows[:, 0]])
    assert (rows[:, 1] + rows[:, 2] <= n).all() and (rows[:, 1:] >= 0).all()
    from data_compression_amd._lib import core
    L = core()   # every row is a range the library's own argument tests take, with room for it at any offset
    for m, (_, f, c) in zip(n.tolist(), rows.tolist()):
        assert L.dc_huff_batch_range_args(100, 100 + m, f, c, 7, 7 + c) == 0, (m, f, c)


def test_library_chunk_interval_is_the_restatement():
    """dc_huff_batch_range_chunks against chunk_interval: every (first, count) of short segments at
    S = 16, the sync sizes at chunk edges, and u64 values where a sum would wrap."""
    from data_compression_amd._lib import core
    L = core()
    for n in (0, 1, 15, 16, 17, 47, 48, 49):
        for first in range(n + 1):
            for count in range(n - first + 1):
                assert lib_chunk_interval(first, count, 16) == chunk_interval(first, count, 16), (first, count)
    for S in (16, 64, 1024):
        for first in (0, 1, S - 1, S, S + 1, 63 * S - 1, 65535, 2**32 - 1, 2**32, 2**63, 2**64 - S, 2**64 - 2):
            for count in (0, 1, 2, S - 1, S, S + 1, 64 * S + 1, 2**32, 2**63, 2**64 - 1):
                if first + count <= 2**64:   # ranges whose end fits
                    assert lib_chunk_interval(first, count, S) == chunk_interval(first, count, S), (S, first, count)
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    for S in (0, 8, 24, 2048):
        assert L.dc_huff_batch_range_chunks(0, 1, S, C.byref(lo), C.byref(hi)) == DC_E_ARG, S
    assert L.dc_huff_batch_range_chunks(0, 1, 64, None, C.byref(hi)) == DC_E_ARG
    assert L.dc_huff_batch_range_chunks(0, 1, 64, C.byref(lo), None) == DC_E_ARG


def test_library_argument_tests_do_not_wrap():
    """dc_huff_batch_range_args: tests 2 to 4 of the order in dc_gpu.h, in that order."""
    from data_compression_amd._lib import core
    f = core().dc_huff_batch_range_args
    M = 2**64 - 1
    assert f(5, 4, 0, 0, 0, 0) == DC_E_ARG                       # offsets that decrease
    assert f(0, 65537, 0, 0, 0, 0) == DC_E_ARG                   # longer than DC_BATCH_SEG_MAX
    assert f(M - 65536, M, 65536, 0, 0, 0) == 0                  # only the difference is used
    assert f(0, 4097, 4088, 10, 0, 100) == DC_E_ARG              # first + count = len + 1
    assert f(0, 4097, M, 2, 0, 100) == DC_E_ARG                  # first + count wraps to 1
    assert f(0, 4097, 4098, 0, 0, 0) == DC_E_ARG                 # first > len
    assert f(0, 4097, 4097, 0, 0, 0) == 0
    assert f(0, 4097, 7, 20, 81, 100) == DC_E_CAPACITY           # passes out_cap by one byte
    assert f(0, 4097, 7, 20, 80, 100) == 0
    assert f(0, 4097, 7, 20, M, M) == DC_E_CAPACITY              # out_off + count wraps
    assert f(0, 4097, 7, 0, 101, 100) == DC_E_CAPACITY           # out_off > out_cap, even for nothing
    assert f(0, 4097, 4090, 10, 0, 5) == DC_E_ARG                # the range is tested before the output
