"""Checksums on the device (dc_gpu.h "checksums"): dc_crc32_batch / dc_crc32_verify_batch
(k_crc_batch) and dc_crc32 (k_crc_pieces, k_crc_fold) through the C ABI with 0xA5-prefilled outputs
and through Codec.crc32 / crc32_batch / crc32_verify_batch, then the chains they exist for:
encode_batch(checksum=True) -> decode_batch(verify=True), and crc32_batch at encode ->
crc32_verify_batch with the decode's status for the nybble and the small batch codecs. The
reference is zlib.crc32 everywhere."""
import zlib

import numpy as np
import pytest

from data_compression_amd.device import Codec
from tests.stream_batch_checks import DC_E_ARG, DC_E_CAPACITY, DC_E_STREAM, FILL, _dev, pack_offsets

pytestmark = pytest.mark.gpu

T = Codec.CRC_TILE         # the bytes a wave takes at a time
PIECE = Codec.CRC_PIECE    # dc_crc32's bytes per wave
DC_E_CHECKSUM = Codec.E_CHECKSUM
FILL32 = 0xA5A5A5A5
PAD = 8                    # prefilled entries after the last one of every output


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def codec(torch_cuda):
    return Codec(0)


def _raw(torch, codec, x, beg, end, count, expect=None, status=None):
    """dc_crc32_batch (expect None) or dc_crc32_verify_batch through the C ABI: x a device tensor,
    beg / end device int64 tensors or raw pointers. Host (crc or None, status) of count entries;
    the PAD entries after them must keep their prefill."""
    ptr = lambda v: v if isinstance(v, int) else v.data_ptr()
    st = torch.full((4 * (count + PAD),), FILL, dtype=torch.uint8, device="cuda")
    if status is not None:
        st[: 4 * count] = _dev(torch, np.asarray(status, np.int32).view(np.uint8))
    if expect is None:
        crc = torch.full((4 * (count + PAD),), FILL, dtype=torch.uint8, device="cuda")
        rc = codec.L.dc_crc32_batch(codec.ctx, x.data_ptr(), x.numel(), ptr(beg), ptr(end), count, crc.data_ptr(), st.data_ptr())
    else:
        crc = None
        e = _dev(torch, np.asarray(expect, np.uint32))
        rc = codec.L.dc_crc32_verify_batch(codec.ctx, x.data_ptr(), x.numel(), ptr(beg), ptr(end), count, e.data_ptr(),
                                           st.data_ptr())
    assert rc == 0
    st_h = st.cpu().numpy().view(np.int32)
    assert (st_h[count:].view(np.uint32) == FILL32).all(), "status written past count"
    if crc is not None:
        crc_h = crc.cpu().numpy().view(np.uint32)
        assert (crc_h[count:] == FILL32).all(), "crc written past count"
        crc = crc_h[:count]
    return crc, st_h[:count]


def _zl(data, beg, end):
    return np.array([zlib.crc32(data[b:e].tobytes()) for b, e in zip(beg, end)], np.uint32)


# ---- 1. every length, every alignment --------------------------------------------------------
@pytest.fixture(scope="module")
def every_length():
    """Buffers of 0 .. 2T + 40 bytes, back to back from offset 5: (bytes, offsets, zlib's CRCs)."""
    lens = np.arange(2 * T + 41, dtype=np.int64)
    off = 5 + np.concatenate([[0], np.cumsum(lens)])
    data = np.random.default_rng(1).integers(0, 256, int(off[-1]) + 9, dtype=np.uint8)
    assert {int(o) % 16 for o in off[:-1]} == set(range(16))
    return data, off, _zl(data, off[:-1], off[1:])


@pytest.mark.parametrize("grid", (0, 1))   # DC_OPT_BATCH_GRID 1: one workgroup walks the whole list
def test_every_length_from_every_alignment(torch_cuda, codec, every_length, grid):
    torch = torch_cuda
    data, off, want = every_length
    x, o = _dev(torch, data), _dev(torch, off)
    codec.set_option("batch_grid", grid)
    try:
        crc, st = _raw(torch, codec, x, o.data_ptr(), o.data_ptr() + 8, off.size - 1)
        bstat = codec.batch_status()
    finally:
        codec.set_option("batch_grid", 0)
    assert (st == 0).all() and bstat == 0
    bad = np.flatnonzero(crc != want)
    assert bad.size == 0, ("lengths", bad[:10], [hex(v) for v in crc[bad[:3]]], [hex(v) for v in want[bad[:3]]])
    assert crc[0] == 0   # the empty buffer


# ---- 2. every byte position counts -----------------------------------------------------------
def test_a_flipped_bit_at_every_position(torch_cuda, codec):
    torch = torch_cuda
    L = 2 * T + 13
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, L, dtype=np.uint8)
    X = np.tile(base, (L + 1, 1))
    X[np.arange(L), np.arange(L)] ^= (1 << rng.integers(0, 8, L)).astype(np.uint8)   # copy j: one bit of byte j
    data = np.concatenate([np.zeros(3, np.uint8), X.reshape(-1)])
    off = 3 + L * np.arange(L + 2, dtype=np.int64)
    clean = zlib.crc32(base.tobytes())
    st = codec.crc32_verify_batch(_dev(torch, data), _dev(torch, np.full(L + 1, clean, np.uint32)), offsets=_dev(torch, off))
    assert codec.batch_status() == DC_E_CHECKSUM
    st = st.cpu().numpy()
    assert np.flatnonzero(st[:L] != DC_E_CHECKSUM).size == 0 and st[L] == 0   # the clean copy comes last


# ---- 3. long and uneven buffers; one buffer over the whole device ----------------------------
@pytest.fixture(scope="module")
def long_data():
    return np.random.default_rng(3).integers(0, 256, 3 + (3 << 20) + 7 + 74 + 5, dtype=np.uint8)


def test_a_long_buffer_among_short_ones(torch_cuda, codec, long_data):
    torch = torch_cuda
    lens = [0, 1, (3 << 20) + 7, 3, 70]
    off = 3 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    crc, st = codec.crc32_batch(_dev(torch, long_data), offsets=_dev(torch, off))
    assert codec.batch_status() == 0 and (st.cpu().numpy() == 0).all()
    assert np.array_equal(crc.cpu().numpy(), _zl(long_data, off[:-1], off[1:]))


def test_one_buffer_in_pieces(torch_cuda, codec, long_data):
    torch = torch_cuda
    x = _dev(torch, long_data)
    for n in (0, 1, 15, 16, 17, PIECE - 1, PIECE, PIECE + 1, 5 * PIECE + 3):
        got = codec.crc32(x[3: 3 + n])
        assert got.dtype == torch.uint32 and got.numel() == 1
        assert int(got.cpu().numpy()[0]) == zlib.crc32(long_data[3: 3 + n].tobytes()), n
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert int(codec.crc32(empty).cpu().numpy()[0]) == 0


# ---- 4. the scatter form ----------------------------------------------------------------------
def test_scattered_ranges_and_bad_entries(torch_cuda, codec):
    torch = torch_cuda
    data = np.random.default_rng(4).integers(0, 256, 5000, dtype=np.uint8)
    cap = data.size
    x = _dev(torch, data)
    # two arrays: descending, overlapping, with gaps; entry 1 ends past in_cap, entry 4 ends before it begins
    beg = np.array([4100, 4000, 3000, 2990, 2000, 700, 700, 0, cap, 17], np.int64)
    end = np.array([5000, cap + 1, 4150, 3001, 1999, 1800, 700, 16, cap, 1041], np.int64)
    good = end >= beg
    good &= end <= cap
    want = np.where(good, _zl(data, np.where(good, beg, 0), np.where(good, end, 0)), 0).astype(np.uint32)
    crc, st = _raw(torch, codec, x, _dev(torch, beg), _dev(torch, end), beg.size)
    assert codec.batch_status() == DC_E_CAPACITY   # the lowest failing entry's
    assert st.tolist() == [0, DC_E_CAPACITY, 0, 0, DC_E_ARG, 0, 0, 0, 0, 0]
    assert np.array_equal(crc, want) and crc[1] == 0 and crc[4] == 0
    # through the Python call too
    crc2, st2 = codec.crc32_batch(x, beg=beg, end=end)
    assert np.array_equal(crc2.cpu().numpy(), want) and np.array_equal(st2.cpu().numpy(), st)
    # one array as off / off + 1: entry i = [off[i], off[i + 1])
    off = np.array([7, 1031, 1031, 500, 2600, cap + 9, 64, 3000], np.int64)
    b, e = off[:-1], off[1:]
    good = (e >= b) & (e <= cap)
    want = np.where(good, _zl(data, np.where(good, b, 0), np.where(good, e, 0)), 0).astype(np.uint32)
    o = _dev(torch, off)
    crc, st = _raw(torch, codec, x, o.data_ptr(), o.data_ptr() + 8, off.size - 1)
    assert st.tolist() == [0, 0, DC_E_ARG, 0, DC_E_CAPACITY, DC_E_ARG, 0]
    assert codec.batch_status() == DC_E_ARG
    assert np.array_equal(crc, want)
    # count 0: DC_OK, no write (the prefill check of _raw covers every entry)
    crc, st = _raw(torch, codec, x, o.data_ptr(), o.data_ptr() + 8, 0)
    assert crc.size == 0 and st.size == 0
    _, st = _raw(torch, codec, x, o.data_ptr(), o.data_ptr() + 8, 0, expect=np.zeros(0, np.uint32))
    assert st.size == 0


# ---- 5. what a decode left is carried over -----------------------------------------------------
def test_verify_carries_failed_entries_over(torch_cuda, codec):
    torch = torch_cuda
    data = np.random.default_rng(5).integers(0, 256, 4000, dtype=np.uint8)
    cap = data.size
    beg = np.array([0, cap + 50, 100, 1 << 62, 900, 3000, 2500, 10], np.int64)
    end = np.array([90, cap + 900, 1200, 5, 2100, 2999, cap + 1, 10], np.int64)
    pre = np.array([0, DC_E_STREAM, 0, DC_E_STREAM, 0, 0, 0, 0], np.int32)
    ok = (pre == 0) & (end >= beg) & (end <= cap)
    expect = np.where(ok, _zl(data, np.where(ok, beg, 0), np.where(ok, end, 0)), 0x12345678).astype(np.uint32)
    expect[4] ^= 1   # entry 4: not the bytes that went in
    _, st = _raw(torch, codec, _dev(torch, data), _dev(torch, beg), _dev(torch, end), beg.size, expect=expect, status=pre)
    assert st.tolist() == [0, DC_E_STREAM, 0, DC_E_STREAM, DC_E_CHECKSUM, DC_E_ARG, DC_E_CAPACITY, 0]
    assert codec.batch_status() == DC_E_STREAM   # entry 1: the carried-over entries count
    # a fresh zero status when none is given
    st = codec.crc32_verify_batch(_dev(torch, data), _dev(torch, expect[[0, 2, 4]]), beg=beg[[0, 2, 4]], end=end[[0, 2, 4]])
    assert st.cpu().numpy().tolist() == [0, 0, DC_E_CHECKSUM] and codec.batch_status() == DC_E_CHECKSUM


# ---- 6. the Huffman batch ----------------------------------------------------------------------
ENC_KEYS = {"count", "n_ary", "S", "offsets", "total", "lens", "mode", "bits", "pay_off", "payload", "sync_off",
            "sync_len", "status", "max_bits", "payload_cap", "sync_cap"}
I_EMPTY, I_STORED, I_TEXT = 2, 4, 5   # of huff_input's segments


@pytest.fixture(scope="module")
def huff_input():
    """Text segments of uneven lengths, an empty one (I_EMPTY), flat random bytes (I_STORED) and one
    of 301 bytes (I_TEXT), from offset 3: (bytes, offsets, the text alone)."""
    from data_compression_amd import synth
    text = synth.english_like(9000, seed=66)
    rng = np.random.default_rng(6)
    rnd = np.concatenate([rng.permutation(256) for _ in range(3)]).astype(np.uint8)   # every code 8 bits: stored
    segs = [text[:1000], text[1000:1033], text[:0], text[1033:5000], rnd, text[5000:5301], text[5301:9000]]
    data, off = pack_offsets([np.zeros(3, np.uint8)] + segs)
    return data, off[1:].copy(), text


def _table(codec, torch, text, shared):
    return codec.batch_table(_dev(torch, text), max_bits=12) if shared else None


def _clone(torch, enc, **repl):
    e = dict(enc)
    e["status"] = torch.full_like(enc["status"], 0x5A5A5A5A)
    e.update(repl)
    return e


@pytest.mark.parametrize("shared", (False, True), ids=("own", "table"))
def test_huffman_batch_checksums(torch_cuda, codec, huff_input, shared):
    torch = torch_cuda
    data, off, text = huff_input
    count = off.size - 1
    x = _dev(torch, data)
    table = _table(codec, torch, text, shared)
    enc = codec.encode_batch(x, off, table=table, checksum=True)
    assert codec.batch_status() == 0
    want = _zl(data, off[:-1], off[1:])
    assert enc["crc"].dtype == torch.uint32 and np.array_equal(enc["crc"].cpu().numpy(), want) and want[I_EMPTY] == 0
    assert int(enc["mode"][I_STORED]) == 0 and int(enc["mode"][I_TEXT]) != 0
    # checksum=False: the call as it was
    plain = codec.encode_batch(x, off, table=table)
    assert set(plain) == ENC_KEYS | ({"table"} if shared else set()) and set(enc) == set(plain) | {"crc"}
    for k in ("mode", "bits", "pay_off", "sync_off", "status"):
        assert torch.equal(plain[k], enc[k]), k
    pb = int(plain["pay_off"][-1])
    assert torch.equal(plain["payload"][:pb], enc["payload"][:pb])
    with pytest.raises(ValueError):
        codec.decode_batch(plain, verify=True)
    # verify=True on a clean batch, both layouts
    out, _ = codec.decode_batch(enc, verify=True)
    assert codec.batch_status() == 0 and (enc["status"].cpu().numpy() == 0).all()
    assert np.array_equal(out.cpu().numpy()[: data.size - 3], data[3:])
    starts = np.array([int(off[-1]) + 40 - int(e) for e in off[1:]], np.int64)   # descending, 40 bytes of room in front
    buf = torch.full((int(off[-1]) + 64,), FILL, dtype=torch.uint8, device="cuda")
    codec.decode_batch(enc, out=buf, out_off=starts, verify=True)
    assert codec.batch_status() == 0 and (enc["status"].cpu().numpy() == 0).all()
    h = buf.cpu().numpy()
    for i in range(count):
        assert np.array_equal(h[starts[i]: starts[i] + off[i + 1] - off[i]], data[off[i]: off[i + 1]]), i
    # one damaged byte in the stored segment's payload
    pay = enc["payload"].clone()
    pay[int(enc["pay_off"][I_STORED]) + 123] ^= 0x40
    bad = _clone(torch, enc, payload=pay)
    out, _ = codec.decode_batch(bad)
    assert codec.batch_status() == 0 and (bad["status"].cpu().numpy() == 0).all()      # today's hole: DC_OK ...
    assert not np.array_equal(out.cpu().numpy()[: data.size - 3], data[3:])                          # ... with wrong bytes
    out, _ = codec.decode_batch(bad, verify=True)
    st = bad["status"].cpu().numpy()
    assert st[I_STORED] == DC_E_CHECKSUM and (np.delete(st, I_STORED) == 0).all()
    assert codec.batch_status() == DC_E_CHECKSUM


@pytest.mark.parametrize("shared", (False, True), ids=("own", "table"))
def test_every_single_bit_flip_of_a_text_segment(torch_cuda, codec, huff_input, shared):
    """The record of one 301-byte segment, copied once per payload bit with that bit flipped: the
    decode finds the flip (DC_E_STREAM) or the verify does (DC_E_CHECKSUM); DC_OK never comes with
    bytes that differ from the input."""
    torch = torch_cuda
    data, off, text = huff_input
    seg = data[off[I_TEXT]: off[I_TEXT + 1]]
    n = seg.size
    table = _table(codec, torch, text, shared)
    one = codec.encode_batch(_dev(torch, seg), np.array([0, n], np.int64), table=table, checksum=True)
    assert codec.batch_status() == 0 and int(one["mode"][0]) != 0
    P, nch = int(one["pay_off"][1]), int(one["sync_off"][1])
    assert 8 * P >= int(one["bits"][0]) > 0
    count = 8 * P
    pay = np.tile(one["payload"][:P].cpu().numpy(), (count, 1))
    j = np.arange(count)
    pay[j, j // 8] ^= (1 << (j % 8)).astype(np.uint8)
    dev = lambda a: _dev(torch, a)
    enc = dict(one, count=count, total=count * n, offsets=dev(n * np.arange(count + 1, dtype=np.int64)),
               mode=one["mode"].repeat(count), bits=one["bits"].repeat(count), crc=dev(np.repeat(one["crc"].cpu().numpy(), count)),
               pay_off=dev(P * np.arange(count + 1, dtype=np.int64)), payload=dev(pay.reshape(-1)),
               sync_off=dev(nch * np.arange(count + 1, dtype=np.int64)), sync_len=one["sync_len"][:nch].repeat(count),
               lens=None if shared else one["lens"].repeat(count, 1), payload_cap=count * P, sync_cap=count * nch,
               status=torch.zeros(count, dtype=torch.int32, device="cuda"))
    out, _ = codec.decode_batch(enc)
    st0 = enc["status"].cpu().numpy().copy()
    got = out.cpu().numpy().reshape(count, n)
    out, _ = codec.decode_batch(enc, verify=True)
    st1 = enc["status"].cpu().numpy()
    same = (got == seg[None, :]).all(axis=1)
    assert set(np.unique(st0)) <= {0, DC_E_STREAM} and set(np.unique(st1)) <= {0, DC_E_STREAM, DC_E_CHECKSUM}
    assert np.array_equal(st1 == DC_E_STREAM, st0 == DC_E_STREAM)          # the decode's failures are carried over
    print(f"{count} flips: decode caught {(st0 != 0).sum()}, DC_OK with wrong bytes {((st0 == 0) & ~same).sum()}, "
          f"harmless {((st0 == 0) & same).sum()}")
    assert np.array_equal(st1 == DC_E_CHECKSUM, (st0 == 0) & ~same)        # exactly the wrong bytes the decode passed
    assert np.array_equal(st1 == 0, (st0 == 0) & same)                     # DC_OK only with the input's bytes


# ---- 7. the nybble and the small batch codecs --------------------------------------------------
@pytest.fixture(scope="module")
def short_ascii():
    """100 short ASCII buffers: text, and every tenth one random capitals and digits (LITERAL in
    both codecs)."""
    from data_compression_amd import synth
    text = synth.english_like(20000, seed=77)
    rng = np.random.default_rng(7)
    alnum = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", np.uint8)
    bufs, pos = [], 0
    for i in range(100):
        n = int(rng.integers(20, 300))
        bufs.append(alnum[rng.integers(0, alnum.size, n)] if i % 10 == 3 else text[pos: pos + n])
        pos += n
    return bufs


@pytest.mark.parametrize("which", ("small", "nybble"))
def test_stream_batch_chain(torch_cuda, codec, short_ascii, which):
    torch = torch_cuda
    data, off = pack_offsets(short_ascii)
    x, o = _dev(torch, data), _dev(torch, off)
    crc, cst = codec.crc32_batch(x, offsets=o)
    assert (cst.cpu().numpy() == 0).all() and np.array_equal(crc.cpu().numpy(), _zl(data, off[:-1], off[1:]))
    if which == "small":
        comp, coff, est = codec.small_compress_batch(x, o)
        decode = lambda c: codec.small_decompress_batch_into(c, coff, o)
    else:
        comp, coff, est = codec.nyb_compress_batch(x, o, False)
        decode = lambda c: codec.nyb_decompress_batch_into(c, coff, False, o)
    assert codec.batch_status() == 0
    out, st = decode(comp)
    st = codec.crc32_verify_batch(out, crc, st, offsets=o)
    assert codec.batch_status() == 0 and (st.cpu().numpy() == 0).all()
    # a damaged literal byte of a LITERAL stream (' ', then the raw bytes): the decode cannot tell
    h, ho = comp.cpu().numpy(), coff.cpu().numpy()
    victim = 33
    assert h[ho[victim]] == 0x20 and ho[victim + 1] - ho[victim] == short_ascii[victim].size + 1
    dmg = comp.clone()
    dmg[int(ho[victim]) + 7] ^= 0x01
    out, st = decode(dmg)
    assert (st.cpu().numpy() == 0).all() and codec.batch_status() == 0
    assert not np.array_equal(out.cpu().numpy()[: data.size], data)
    st = codec.crc32_verify_batch(out, crc, st, offsets=o)
    st = st.cpu().numpy()
    assert st[victim] == DC_E_CHECKSUM and (np.delete(st, victim) == 0).all()
    assert codec.batch_status() == DC_E_CHECKSUM
