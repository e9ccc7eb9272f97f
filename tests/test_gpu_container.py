"""The host layer of csrc/dc_host.hip against the model of tests/container_model.py, on the device:
both writers byte for byte over the catalogue (dc_huff_compress_host, dc_huff_compress_netstring,
through ctypes so that sync_syms, lengths and max_symbol_value are all reachable), both readers on
the model's own containers (never on what the GPU wrote), the range read at chunk and group edges
from an aligned and an unaligned container, and the nybble / small host wrappers against the oracle.
Every call's out_len, its DC_E_CAPACITY at one byte short, and the bytes it must leave alone
(0xA5) are asserted.

Safety: a malformed container is handed to a reader here only where test_container_model_cpu.py
asserts that dc_huff_container_check rejects it, so the call ends on the host; the "wild" entries
(sizes and offsets far from the true ones) are not handed over at all. The one damage that reaches a
device-side step is a netstring index shifted by at most 64 bits in a group that is not the last
(the index is text that the device parses before the host can hold it to the index rule): every
chunk still starts inside the payload whether or not the rule fires.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import container_model as cm

pytestmark = pytest.mark.gpu
FILL = 0xA5
u8p = C.POINTER(C.c_uint8)


def _core():
    from data_compression_amd._lib import core
    return core()


def _src(b):
    a = np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(1, np.uint8)
    return a, a.ctypes.data_as(u8p)


def _call(fn, head, cap, slack=64):
    """fn(*head, out, cap, &len) into a 0xA5-filled buffer of cap + slack bytes: (rc, len, buffer)"""
    out = np.full(cap + slack, FILL, np.uint8)
    got = C.c_uint64(0)
    rc = fn(*head, out.ctypes.data_as(u8p), cap, C.byref(got))
    return rc, got.value, out


def _untouched(buf, start=0):
    return bool((buf[start:] == FILL).all())


def _writer_args(c):
    keep, px = _src(c.x.tobytes())
    if c.lengths is None:
        return keep, (px, c.x.size, c.n_ary, None, 258, c.S)
    L = np.ascontiguousarray(np.asarray(c.lengths, np.int32)[: c.M + 1])
    return (keep, L), (px, c.x.size, c.n_ary, L.ctypes.data_as(C.POINTER(C.c_int32)), c.M, c.S)


def _exact(fn, head, want, bound):
    """the call writes `want` and nothing after it; one byte short is DC_E_CAPACITY with nothing written"""
    need = len(want)
    assert bound >= need
    for cap in (bound, need):
        rc, got, buf = _call(fn, head, cap)
        assert rc == cm.OK and got == need
        assert buf[:need].tobytes() == want, "first difference at byte %d" % next(
            i for i in range(need) if buf[i] != want[i])
        assert _untouched(buf, need)
    rc, got, buf = _call(fn, head, need - 1)
    assert rc == cm.E_CAPACITY and _untouched(buf)


# ---- writers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cm.catalogue(), ids=repr)
def test_dch1_writer_is_the_model(c):
    L = _core()
    keep, head = _writer_args(c)
    status, want = c.dch1_model()
    bound = int(L.dc_huff_compress_bound(c.x.size, c.S))
    assert bound == cm.compress_bound(c.x.size, c.S)
    if status != cm.OK:      # DC_E_ARG (an arity over 16), DC_E_CODE_TOO_LONG, DC_E_NOCODE: nothing written
        rc, got, buf = _call(L.dc_huff_compress_host, head, bound)
        assert rc == status and _untouched(buf)
        return
    _exact(L.dc_huff_compress_host, head, want, bound)


@pytest.mark.parametrize("c", cm.catalogue(), ids=repr)
def test_netstring_writer_is_the_model(c):
    L = _core()
    keep, head = _writer_args(c)
    want, why = c.ns_model()
    bound = int(L.dc_huff_netstring_bound(c.x.size))
    assert bound == cm.netstring_bound(c.x.size)
    _exact(L.dc_huff_compress_netstring, head, want, bound)


# ---- readers -----------------------------------------------------------------------------------
def _reads(fn, blob, want):
    keep, pb = _src(blob)
    n = len(want)
    rc, got, buf = _call(fn, (pb, len(blob)), n)
    assert rc == cm.OK and got == n
    assert buf[:n].tobytes() == want and _untouched(buf, n)
    if n:
        rc, got, buf = _call(fn, (pb, len(blob)), n - 1)
        assert rc == cm.E_CAPACITY and _untouched(buf)


@pytest.mark.parametrize("c", cm.catalogue(), ids=repr)
def test_readers_decode_the_models_containers(c):
    L = _core()
    status, blob = c.dch1_model()
    if status == cm.OK:
        _reads(L.dc_huff_decompress_host, blob, c.x.tobytes())
    _reads(L.dc_huff_decompress_netstring, c.ns_model()[0], c.x.tobytes())
    _reads(L.dc_huff_decompress_host, c.ns_model()[0], c.x.tobytes())      # no magic: read as netstrings


@pytest.mark.parametrize("entry", cm.reader_inputs(), ids=lambda e: e[0])
def test_netstring_reader_takes_what_no_encoder_writes(entry):
    name, blob, want = entry
    _reads(_core().dc_huff_decompress_netstring, blob, want)


def test_readers_refuse_what_the_check_rejects():
    """DC_E_STREAM and an untouched buffer; the CPU file asserts the check's verdict on each entry"""
    L = _core()
    for name, blob, valid, wild in cm.malformed_dch1():
        if valid or wild:
            continue
        keep, pb = _src(blob)
        assert L.dc_huff_container_check(pb, len(blob)) == cm.E_STREAM, name
        rc, got, buf = _call(L.dc_huff_decompress_host, (pb, len(blob)), 8192)
        assert rc == cm.E_STREAM and _untouched(buf), name
        rc, got, buf = _call(L.dc_huff_decompress_range_host, (pb, len(blob), 1000, 100), 8192)
        assert rc == cm.E_STREAM and _untouched(buf), name
    for name, blob, valid in cm.malformed_netstring():
        if valid:
            continue
        keep, pb = _src(blob)
        assert L.dc_huff_container_check(pb, len(blob)) == cm.E_STREAM, name
        rc, got, buf = _call(L.dc_huff_decompress_netstring, (pb, len(blob)), 8192)
        assert rc == cm.E_STREAM and _untouched(buf), name


@pytest.mark.parametrize("what", ["base", "len"])
@pytest.mark.parametrize("delta", [1, -1, 64, -64])
def test_netstring_reader_holds_the_parsed_index_to_the_rule(delta, what):
    """One base or one length of a group that is not the last, moved by at most 64 bits: the host
    check cannot see it (the index is text), the reader parses it on the device, reads it back and
    refuses it before the decoder runs. The undamaged container decodes."""
    L = _core()
    blob, x = cm.shifted_index(delta, what)
    keep, pb = _src(blob)
    rc, got, buf = _call(L.dc_huff_decompress_netstring, (pb, len(blob)), x.size)
    assert rc == cm.E_STREAM and _untouched(buf)
    t = cm.code_of(x, 2)
    _reads(L.dc_huff_decompress_netstring, cm.segment(x, t, 64), x.tobytes())


# ---- range read ----------------------------------------------------------------------------------
def _ranges(n, S):
    G = 64 * S
    rs = set()
    for e in (S, 2 * S, G, 2 * G, G + S):                 # chunk and group edges
        for d in (-1, 0, 1):
            rs.add((e + d, 2 * S + 1))                    # first on the edge and either side
            rs.add((e + d - (S + 3), S + 3))              # first + count on it
            rs.add((e + d, 1))
    last = (n - 1) // S * S                               # the last, partial chunk
    rs |= {(last, n - last), (last - 1, n - last + 1), (n - 1, 1), (last + 1, 1), (0, n), (G - 1, G + 2)}
    rs |= {(0, 0), (n, 0), (G, 0)}
    return sorted((f, k) for f, k in rs if f >= 0 and f + k <= n)


@pytest.mark.parametrize("S", [16, 64])
def test_range_read_at_the_edges_aligned_and_not(S):
    L = _core()
    n = 2 * 64 * S + 5 * S + 3
    assert n % S and cm.groups(n, S) == 3
    x = cm.skew(n, 70 + S)
    blob = cm.dch1_bytes(x, 2, S)
    assert cm.dch1_ok(blob)
    raw = (C.c_uint8 * (len(blob) + 16))()
    base = C.addressof(raw)
    base += (-base) % 8
    for off in (0, 1):                                    # 8-B aligned, and 1 mod 8: the bases are copied out
        addr = base + off
        C.memmove(addr, blob, len(blob))
        pb = C.cast(addr, u8p)
        assert addr % 8 == off
        for first, count in _ranges(n, S):
            rc, got, buf = _call(L.dc_huff_decompress_range_host, (pb, len(blob), first, count), count)
            assert rc == cm.OK and got == count, (off, first, count)
            assert buf[:count].tobytes() == x[first: first + count].tobytes(), (off, first, count)
            assert _untouched(buf, count), (off, first, count)
            if count:
                rc, got, buf = _call(L.dc_huff_decompress_range_host, (pb, len(blob), first, count), count - 1)
                assert rc == cm.E_CAPACITY and _untouched(buf), (off, first, count)
        for first, count in ((n, 1), (n + 1, 0), (0, n + 1), (2 ** 64 - 1, 2)):
            rc, got, buf = _call(L.dc_huff_decompress_range_host, (pb, len(blob), first, count), n + 1)
            assert rc == cm.E_ARG and _untouched(buf), (off, first, count)
    ns = cm.netstring_bytes(x, 2, S)                      # no random access in the netstring container
    keep, pn = _src(ns)
    rc, got, buf = _call(L.dc_huff_decompress_range_host, (pn, len(ns), 0, 1), 1)
    assert rc == cm.E_ARG and _untouched(buf)


# ---- nybble and small host wrappers ------------------------------------------------------------------
def _texts():
    from data_compression_amd import synth
    return [b"", b"q", synth.english_like(4096, seed=4).tobytes()]


def _wrapper(fn, head_of, data, want):
    keep, pd = _src(data)
    need = len(want)
    rc, got, buf = _call(fn, head_of(pd, len(data)), need)
    assert rc == cm.OK and got == need and buf[:need].tobytes() == want and _untouched(buf, need)
    if need:
        rc, got, buf = _call(fn, head_of(pd, len(data)), need - 1)
        assert rc == cm.E_CAPACITY and _untouched(buf)


@pytest.mark.parametrize("modify", [0, 1])
def test_nybble_host_wrappers_are_the_oracle(modify):
    L = _core()
    for x in _texts():
        comp = orc.nybble_compress(x, bool(modify))
        assert orc.nybble_decompress(comp, bool(modify)) == x
        _wrapper(L.dc_nyb_compress_host, lambda p, n: (p, n, modify), x, comp)
        _wrapper(L.dc_nyb_decompress_host, lambda p, n: (p, n, modify), comp, x)


def test_small_host_wrappers_are_the_oracle():
    L = _core()
    for x in _texts():
        comp = orc.small_compress(x)
        assert orc.small_decompress(comp) == x
        _wrapper(L.dc_small_compress_host, lambda p, n: (p, n), x, comp)
        _wrapper(L.dc_small_decompress_host, lambda p, n: (p, n), comp, x)
