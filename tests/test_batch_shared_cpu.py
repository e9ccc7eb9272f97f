"""The shared-table mode of the batched Huffman codec (dc_gpu.h "Huffman batch v1, shared
table") without a device: the expected batch under one table from the CPU oracle alone
(orc.canonical, orc.bitcodes, orc.huff_pack), what the text table does to SEGMENTS, the exported
entry points and their host argument checks. text_table, table_codes and oracle_shared_batch are
shared with tests/test_gpu_batch_shared.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_batch_cpu import KINDS, LENGTHS, SEGMENTS, pack_offsets

DC_E_ARG = -1
SEGMENT_KINDS = [KINDS[j % len(KINDS)] for j in range(len(LENGTHS))] + ["one", "cycle", "random", "enwik", "zipf"]
ENTRY_POINTS = ("dc_huff_encode_batch_shared", "dc_huff_decode_batch_shared", "dc_huff_decode_batch_shared_scatter",
                "dc_huff_table_get_lengths")


def table_codes(lengths, n_ary):
    """(code u32[256], nb u8[256]) of a table of the given lengths: nb 0 is "no code"."""
    code, nb, _ = orc.bitcodes(*orc.canonical(lengths, n_ary), n_ary)
    return code, nb


@functools.lru_cache(maxsize=None)
def text_table(n_ary):
    """The lengths (259, in digits) of the histogram of the enwik, zipf and "one" segments of
    SEGMENTS: the cycle and random segments hold bytes it has no code for."""
    assert len(SEGMENT_KINDS) == len(SEGMENTS)
    text = np.concatenate([s for s, k in zip(SEGMENTS, SEGMENT_KINDS) if k in ("enwik", "zipf", "one")])
    return orc.huffman_lengths(orc.histogram(text), n_ary)


def outcome(seg, nb):
    """'empty', 'nocode' (a byte without a code), 'notsmaller' (coded bits >= 8 len) or 'coded'."""
    if seg.size == 0:
        return "empty"
    nbs = nb[seg].astype(np.int64)
    if (nbs == 0).any():
        return "nocode"
    return "coded" if int(nbs.sum()) < 8 * seg.size else "notsmaller"


def _oracle_shared(segs, code, nb, S):
    mode = np.zeros(len(segs), np.uint8)
    bits = np.zeros(len(segs), np.int64)
    pay_off = np.zeros(len(segs) + 1, np.int64)
    sync_off = np.zeros(len(segs) + 1, np.int64)
    pay, sync = [], []
    for i, seg in enumerate(segs):
        if outcome(seg, nb) == "coded":
            p, b, idx = orc.huff_pack(seg, code, nb, 0, S)
            assert b == int(nb[seg].astype(np.int64).sum())
            sl = np.diff(np.append(idx, np.uint64(b))).astype(np.uint16)
            mode[i], bits[i] = 1, b
        else:   # stored: the bytes, 8 bits a symbol
            p, sl = seg, np.array([8 * min(S, seg.size - c * S) for c in range((seg.size + S - 1) // S)], np.uint16)
            bits[i] = 8 * seg.size
        nbytes = (int(bits[i]) + 7) // 8
        assert p.size == nbytes and sl.size == (seg.size + S - 1) // S
        padded = np.zeros((nbytes + 15) // 16 * 16, np.uint8)   # the pad bytes are zero
        padded[:nbytes] = p
        pay.append(padded)
        sync.append(sl)
        pay_off[i + 1] = pay_off[i] + padded.size
        sync_off[i + 1] = sync_off[i] + sl.size
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return {"mode": mode, "bits": bits, "pay_off": pay_off, "payload": cat(pay, np.uint8), "sync_off": sync_off,
            "sync_len": cat(sync, np.uint16)}


def oracle_shared_batch(segs, code, nb, S):
    """The expected mode / bits / pay_off / payload (zero pads) / sync_off / sync_len of a batch
    whose every segment is coded under (code, nb), or stored. Do not modify the result."""
    return _oracle_shared(segs, np.ascontiguousarray(code, np.uint32), np.ascontiguousarray(nb, np.uint8), S)


@functools.lru_cache(maxsize=None)
def oracle_text_batch(n_ary, S):
    """oracle_shared_batch of SEGMENTS under the text table, computed once per (n_ary, S)."""
    return oracle_shared_batch(SEGMENTS, *table_codes(text_table(n_ary), n_ary), S)


def test_text_table_gives_all_four_outcomes_at_n2():
    _, nb = table_codes(text_table(2), 2)
    got = [outcome(s, nb) for s in SEGMENTS]
    assert set(got) == {"coded", "notsmaller", "nocode", "empty"}
    for s, k, o in zip(SEGMENTS, SEGMENT_KINDS, got):
        if s.size >= 4095 and k in ("cycle", "random"):
            assert o == "nocode", (k, s.size)   # they hold the byte value the text never does
    exp = oracle_text_batch(2, 64)
    assert [int(m) for m in exp["mode"]] == [int(o == "coded") for o in got]


@pytest.mark.parametrize("n_ary,longest", [(2, 14), (3, 18), (17, 15), (16, 12)])
def test_coded_segments_use_long_codes(n_ary, longest):
    """Past the decoder's 12-bit first level at n = 2, 3 and 17 (at n = 2 both 13 and 14 bits)."""
    _, nb = table_codes(text_table(n_ary), n_ary)
    used = {int(nb[s].max()) for s in SEGMENTS if outcome(s, nb) == "coded"}
    assert used and max(used) == longest
    if n_ary == 2:
        assert {13, 14} <= used


def test_every_segment_is_stored_at_n256():
    _, nb = table_codes(text_table(256), 256)
    assert all(outcome(s, nb) in ("empty", "notsmaller", "nocode") for s in SEGMENTS)
    exp = oracle_text_batch(256, 64)
    assert not exp["mode"].any()
    x, off = pack_offsets(SEGMENTS)
    assert np.array_equal(exp["bits"], 8 * np.diff(off))


def test_overlong_codes_are_no_code():
    L = np.zeros(259, np.int32)
    L[[0x41, 0x42, 0x43, 0x44]] = (1, 2, 33, 33)
    _, nb = table_codes(L, 2)
    assert nb[0x41: 0x45].tolist() == [1, 2, 0, 0]
    assert outcome(np.frombuffer(b"ABABAABA" * 10, np.uint8), nb) == "coded"
    assert outcome(np.frombuffer(b"ABCA" * 10, np.uint8), nb) == "nocode"


def test_entry_points_are_exported_and_declared():
    from data_compression_amd._lib import core
    L = core()
    for name in ENTRY_POINTS:
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is C.c_int, name


def test_null_context_or_table_is_an_argument_error():
    from data_compression_amd._lib import HBatch, core
    L = core()
    b = HBatch()
    b.n_ary, b.sync_syms = 2, 64
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)    # never read: the table test comes first
    tab = C.cast(C.create_string_buffer(64), C.c_void_p)    # never read: the context test comes first
    n = C.c_int(0)
    for c, t in ((None, tab), (ctx, None), (None, None)):
        assert L.dc_huff_encode_batch_shared(c, None, None, 0, t, C.byref(b)) == DC_E_ARG
        assert L.dc_huff_decode_batch_shared(c, C.byref(b), t, None, None, 0) == DC_E_ARG
        assert L.dc_huff_decode_batch_shared_scatter(c, C.byref(b), t, None, None, None, 0) == DC_E_ARG
        assert L.dc_huff_table_get_lengths(c, t, None, 0, C.byref(n)) == DC_E_ARG


def test_bounds_hold_the_oracle_batch():
    from data_compression_amd._lib import core
    L = core()
    _, off = pack_offsets(SEGMENTS)
    for n_ary, S in ((2, 64), (2, 16), (17, 64), (256, 64)):
        b = oracle_text_batch(n_ary, S)
        assert b["pay_off"][-1] <= L.dc_huff_batch_payload_bound(int(off[-1]), len(SEGMENTS))
        assert b["sync_off"][-1] <= L.dc_huff_batch_sync_bound(int(off[-1]), len(SEGMENTS), S)
        assert (b["pay_off"] % 16 == 0).all()
