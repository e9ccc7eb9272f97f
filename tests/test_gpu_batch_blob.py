"""The "DCHB" container of a Huffman batch on the device (dc_gpu.h "Huffman batch v1: container
DCHB"), against the model of tests/batch_blob_model.py:

  seal    the blob dc_huff_batch_seal writes is write() of the arrays read back from the encode, byte
          for byte, whether the payload was encoded in place or copied; a cap of blob_bytes holds it, a
          cap one byte short gives DC_E_CAPACITY and leaves the bytes past the cap alone
  open    containers the model wrote from hand_batch streams (the device never wrote them) open to
          the model's offsets and decode, whole, scattered, by ranges and verified, to the model's bytes
  trip    encode_batch_blob -> host -> batch_open -> decode_batch, and huffman.compress_batch /
          decompress_batch
  damage  one case per field of the header, the directory and the body: blob_check, batch_open and
          the decode report what check() and model_decode say, and no byte outside a segment's own
          output is written (0xA5 guards either side)
  failed  a segment the encode failed seals empty under its status; a record deeper than 15 under
          nybble records gives DC_E_CODE_TOO_LONG at seal and DC_E_STREAM for that segment alone
"""
import zlib

import numpy as np
import pytest

from tests import batch_blob_model as M
from tests import batch_body_model as BB
from tests.test_batch_blob_cpu import KINDS, container, directory_damage, header_damage, lib_check

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 4096
DC_E_CHECKSUM = -9
COUNTS = (0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def codec(torch_cuda):
    from data_compression_amd.device import Codec
    return Codec(0)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t, dt=None):
    a = t.cpu().numpy()
    return a if dt is None else a.view(dt)


def text(rng, n):
    """n compressible bytes: a skewed choice among 40 values"""
    p = 1.0 / np.arange(1, 41)
    return rng.choice(np.arange(60, 100, dtype=np.uint8), n, p=p / p.sum()).astype(np.uint8)


def flat(rng, n):
    """n bytes no table shrinks: every value equally often when 256 divides n (any code then takes
    at least 8 n bits, by Kraft), else uniform random"""
    if n % 256 == 0:
        return rng.permutation(np.repeat(np.arange(256, dtype=np.uint8), n // 256))
    return rng.integers(0, 256, n, dtype=np.uint8)


def segments(lens, seed, random_at=()):
    rng = np.random.default_rng(seed)
    return [flat(rng, n) if i in random_at else text(rng, n) for i, n in enumerate(lens)]


def _mode_kw(torch, codec, kind, x, offsets, n_ary, flags):
    kw = {"checksum": bool(flags & M.CRC)}
    if kind == M.OWN4:
        kw["max_bits"] = 15
    elif kind == M.SHARED:
        kw["table"] = codec.batch_table(x, n_ary, max_bits=16, cover=True)
    elif kind == M.SET:
        half = x.numel() // 2
        rows = [codec.table_get_lengths(codec.batch_table(x[:max(half, 1)].clone(), n_ary, max_bits=16, cover=True))[:256],
                codec.table_get_lengths(codec.batch_table(x, n_ary, max_bits=16))[:256]]
        kw["table_set"] = codec.table_set(rows, n_ary)
    return kw


def model_of_enc(codec, enc, kind, flags):
    """(blob, status): write() of the arrays read back from the encode as a container of the kind and
    flags the test asked for, under the seal's rules for a failed segment (empty and stored, its
    record zeros) and for a record that does not pack"""
    tables = enc.get("table") if kind == M.SHARED else enc.get("table_set") if kind == M.SET else None
    n = enc["count"]
    est = _np(enc["status"]).astype(np.int32)
    ok = est == 0
    off = _np(enc["offsets"])
    a = {"mode": np.where(ok, _np(enc["mode"]), 0).astype(np.uint8), "bits": np.where(ok, _np(enc["bits"]), 0).astype(np.int64),
         "payload": _np(enc["payload"]), "pay_off": _np(enc["pay_off"]), "sync_len": _np(enc["sync_len"], np.uint16),
         "sync_off": _np(enc["sync_off"])}
    if n == 0:   # an encode of no segment returns without a launch: the two offset arrays hold nothing
        a["pay_off"] = a["sync_off"] = np.zeros(1, np.int64)
    seg_len = np.where(ok, off[1:] - off[:-1], 0)
    status = est.copy()
    records = None
    if kind in (M.OWN, M.OWN4):
        a["lens"] = np.where(ok[:, None], _np(enc["lens"]), 0).astype(np.uint8).reshape(n, 256)
        if kind == M.OWN4:
            status[ok & ~M.lens4(a["lens"])[1]] = M.DC_E_CODE_TOO_LONG
    elif kind == M.SHARED:
        records = codec.table_get_lengths(tables)[:256].astype(np.uint8).reshape(1, 256)
    else:
        records = _np(tables)
        a["tid"] = np.where(ok, _np(enc["tid"]), 0).astype(np.uint8)
    crc = np.where(ok, _np(enc["crc"]), 0).astype(np.uint32) if flags & M.CRC else None
    return M.write(a, seg_len, kind, flags, enc["n_ary"], enc["S"], records=records, crc=crc), status


def _first(status):
    bad = [int(v) for v in status if v]
    return bad[0] if bad else 0


def seal_is_the_model(torch, codec, segs, kind, flags, n_ary, S, caps=True, **more):
    """encode, seal (copying), compare with the model; encode in place, compare again; the two caps;
    then open what was sealed (from the host and on the device) and decode it. Returns the blob."""
    data = np.concatenate(segs) if segs else np.zeros(0, np.uint8)
    off = np.concatenate(([0], np.cumsum([s.size for s in segs]))).astype(np.int64)
    x, offsets = _dev(torch, data) if data.size else torch.empty(0, dtype=torch.uint8, device="cuda"), _dev(torch, off)
    kw = dict(n_ary=n_ary, sync_syms=S, **_mode_kw(torch, codec, kind, x, offsets, n_ary, flags))
    kw.update(more)
    lens4 = kind == M.OWN4
    enc = codec.encode_batch(x, offsets, **kw)
    blob, info, status = codec.batch_seal(enc, lens4=lens4)
    first = codec.batch_status()
    want, want_status = model_of_enc(codec, enc, kind, flags)
    n = len(want)
    assert _np(info).tolist() == [n, 0]
    assert _np(blob[:n]).tobytes() == want
    assert _np(status).tolist() == want_status.tolist() and first == _first(want_status)
    assert M.check(want) == 0 and lib_check(want) == 0
    K = {M.SHARED: 1, M.SET: 2}.get(kind, 0)   # (_mode_kw's set has two records)
    assert M.parse(want)["K"] == K and codec.batch_blob_bound(data.size, len(segs), S, kind, flags, K) >= n
    # in place: the same bytes
    blob2, info2, status2 = codec.encode_batch_blob(x, offsets, lens4=lens4, **kw)
    assert _np(info2).tolist() == [n, 0] and _np(blob2[:n]).tobytes() == want
    assert _np(status2).tolist() == want_status.tolist()
    if caps:
        for cap in (n, n - 1):
            buf = torch.full((n + 64,), FILL, dtype=torch.uint8, device="cuda")
            _, infoc, _ = codec.batch_seal(enc, out=buf[:cap], lens4=lens4)
            got = _np(buf)
            assert (got[cap:] == FILL).all(), cap
            if cap == n:
                assert _np(infoc).tolist() == [n, 0] and got[:n].tobytes() == want
            else:
                assert _np(infoc).tolist() == [n, M.DC_E_CAPACITY]
                assert (got[:64] == FILL).all()   # no header
    # open and decode: from the host, and where it lies
    P = M.parse(want)
    moff, mpo, mso = M.derived(P["len"], P["bits"], S)
    alive = want_status != M.DC_E_ARG
    for src in (np.frombuffer(want, np.uint8), blob[:n]):
        op = codec.batch_open(src)
        out, _ = codec.decode_batch(op, verify=bool(flags & M.CRC))
        st = _np(op["status"])
        assert _np(op["container_status"]).tolist() == [0]
        assert np.array_equal(_np(op["offsets"]), moff) and np.array_equal(_np(op["pay_off"]), mpo)
        assert np.array_equal(_np(op["sync_off"]), mso)
        dead = (want_status == M.DC_E_CODE_TOO_LONG) & (P["mode"] == 1)
        assert st.tolist() == np.where(dead, M.DC_E_STREAM, 0).tolist()
        got = _np(out)
        for i, s in enumerate(segs):
            if alive[i] and not dead[i]:
                assert np.array_equal(got[moff[i]: moff[i + 1]], s), i
    return want


# ---- seal is the model, and the round trip ----------------------------------------------------
@pytest.mark.parametrize("flags", (0, M.CRC))
@pytest.mark.parametrize("kind", KINDS)
def test_seal_every_kind_and_flag(torch_cuda, codec, kind, flags):
    """S = 64: lengths 0, 1, S - 1, S, S + 1, 4095, 4096, 65536, a stored one (uniform random) and one
    the encode refuses (65537 bytes, DC_E_ARG)"""
    S = 64
    lens = [0, 1, S - 1, S, S + 1, 4095, 4096, 4096, 65537, 65536, 17]
    segs = segments(lens, 21 + kind, random_at=(7, 8))
    blob = seal_is_the_model(torch_cuda, codec, segs, kind, flags, 2, S)
    P = M.parse(blob)
    assert P["len"].tolist() == [0, 1, S - 1, S, S + 1, 4095, 4096, 4096, 0, 65536, 17]
    assert P["mode"][7] == 0 and P["mode"][6] == 1 and P["mode"][8] == 0 and P["bits"][8] == 0


@pytest.mark.parametrize("count", COUNTS)
def test_seal_counts(torch_cuda, codec, count):
    """the scan's per-thread split and its 8-wide unroll, and section sizes either side of 16"""
    kind = KINDS[COUNTS.index(count) % 4]
    lens = [(1, 0, 15, 16, 17, 40)[i % 6] for i in range(count)]   # (count 1: one byte; segments of no byte at all: the round trip)
    seal_is_the_model(torch_cuda, codec, segments(lens, count), kind, M.CRC if count % 2 else 0, 2, 16, caps=count < 100)


@pytest.mark.parametrize("n_ary,S,kind", ((3, 16, M.OWN), (16, 1024, M.OWN4), (256, 64, M.SHARED), (3, 1024, M.SET),
                                          (16, 16, M.SET), (256, 16, M.OWN)))
def test_seal_arities_and_sync_sizes(torch_cuda, codec, n_ary, S, kind):
    lens = [0, 1, S - 1, S, S + 1, 4095, 4096, 3 * S]
    more = {"max_bits": 12} if kind == M.OWN4 and n_ary == 16 else {}
    seal_is_the_model(torch_cuda, codec, segments(lens, n_ary + S, random_at=(5,)), kind, M.CRC, n_ary, S, **more)


def deep_segment():
    """65535 bytes of 16 values with counts 1, 2, 4, .., 32768: the own table at n = 2 has a 16-digit length"""
    x = np.repeat(np.arange(16, dtype=np.uint8) + 65, 2 ** np.arange(16))
    return np.random.default_rng(2).permutation(x)


def test_failed_and_unpackable_segments(torch_cuda, codec):
    """kind 1 without a cap: the deep segment's record is deeper than 15 (DC_E_CODE_TOO_LONG at
    seal, zeros in the container, DC_E_STREAM for that segment alone at decode); the 65537-byte
    segment keeps the encode's DC_E_ARG and is sealed empty"""
    segs = segments([100, 0, 65537, 200], 9, random_at=(2,))
    segs[1] = deep_segment()
    blob = seal_is_the_model(torch_cuda, codec, segs, M.OWN4, M.CRC, 2, 64, max_bits=None)
    P = M.parse(blob)
    assert P["len"].tolist() == [100, segs[1].size, 0, 200] and P["mode"].tolist() == [1, 1, 0, 1]
    assert not P["records"][1].any() and not P["records"][2].any() and P["records"][0].any()
    x = _dev(torch_cuda, np.concatenate(segs))
    off = np.concatenate(([0], np.cumsum([s.size for s in segs]))).astype(np.int64)
    _, info, status = codec.encode_batch_blob(x, off, lens4=True, n_ary=2, sync_syms=64)
    assert _np(status).tolist() == [0, M.DC_E_CODE_TOO_LONG, M.DC_E_ARG, 0] and codec.batch_status() == M.DC_E_CODE_TOO_LONG
    assert _np(info)[1] == 0


# ---- open reads the model's containers ----------------------------------------------------------
_records = {}


def expected_decode(c, blob, out_cap):
    """(statuses, bytes or None per segment, offsets) of decode_batch on the opened blob, from the
    model: the decoders' own tests in their order on the derived offsets, then model_decode"""
    P = M.parse(blob)
    S, kind, n = P["S"], P["kind"], P["count"]
    off, po, so = M.derived(P["len"], P["bits"], S)
    st, out = [], []
    for i in range(n):
        ln, bits, mode = int(P["len"][i]), int(P["bits"][i]), int(P["mode"][i])
        tid = int(P["tid"][i]) if P["tid"] is not None else 0
        if ln > M.SEG_MAX:
            st.append(M.DC_E_ARG), out.append(None)
            continue
        if off[i + 1] > out_cap:
            st.append(M.DC_E_CAPACITY), out.append(None)
            continue
        if not M.seg_ok(ln, bits, mode, tid, kind, P["K"]) or po[i + 1] > P["pay_total"] or so[i + 1] > P["sync_total"]:
            st.append(M.DC_E_STREAM), out.append(None)
            continue
        if ln == 0:
            st.append(0), out.append(np.zeros(0, np.uint8))
            continue
        rec = None
        if mode == 1:
            lens = P["records"][i] if kind == M.OWN else M.unpack4(P["records"][i])[0] if kind == M.OWN4 else \
                P["records"][tid if kind == M.SET else 0]
            if not BB.own_usable(lens, P["n_ary"]):
                st.append(M.DC_E_STREAM), out.append(None)
                continue
            key = (lens.tobytes(), P["n_ary"])
            if key not in _records:
                _records[key] = BB.make_record(lens, P["n_ary"])
            rec = _records[key]
        r, o = BB.model_decode(rec, mode, bits, P["payload"][po[i]: po[i + 1]], P["sync_len"][so[i]: so[i + 1]], ln, S)
        st.append(r), out.append(o)
    return st, out, off


def open_and_decode(torch, codec, c, blob, verify):
    """batch_open of the blob (host bytes), the model's statuses and offsets, then decode_batch into
    a guarded 0xA5 buffer: every byte of it, every status and batch_status()"""
    op = codec.batch_open(blob)
    P = M.parse(blob)
    assert _np(op["status"]).tolist() == M.seg_status(blob).tolist()
    assert _np(op["container_status"]).tolist() == [0 if M.totals_ok(blob) else M.DC_E_STREAM]
    cap = int(c["seg_len"].sum()) + 70000   # room for a segment that claims more than it has
    st, out, off = expected_decode(c, blob, cap)
    assert np.array_equal(_np(op["offsets"]), off)
    if verify:
        for i in range(len(st)):
            if st[i] == 0 and zlib.crc32(out[i].tobytes()) != int(P["crcs"][i]):
                st[i] = DC_E_CHECKSUM
    image = np.full(GUARD + cap + GUARD, FILL, np.uint8)
    for i, o in enumerate(out):
        if o is not None:
            image[GUARD + off[i]: GUARD + off[i] + o.size] = o
    buf = torch.full((image.size,), FILL, dtype=torch.uint8, device="cuda")
    codec.decode_batch(op, out=buf[GUARD: GUARD + cap], verify=verify)
    first = codec.batch_status()
    assert _np(op["status"]).tolist() == st
    assert first == _first(st)
    assert np.array_equal(_np(buf), image)
    return op, st, out, off


@pytest.mark.parametrize("flags", (0, M.CRC))
@pytest.mark.parametrize("kind", KINDS)
def test_open_reads_the_models_containers(torch_cuda, codec, kind, flags):
    S = 64
    c = container(kind, flags, 2, S, [0, 1, S - 1, S, S + 1, 4095, 4096, 65536, 100, 17, 8192 + 5], seed=31 + kind)
    assert lib_check(c["blob"]) == 0
    op, st, out, off = open_and_decode(torch_cuda, codec, c, c["blob"], verify=bool(flags))
    assert st == [0] * len(c["segs"]) and all(np.array_equal(o, s) for o, s in zip(out, c["segs"]))
    a = c["arrays"]
    assert np.array_equal(_np(op["pay_off"]), a["pay_off"]) and np.array_equal(_np(op["sync_off"]), a["sync_off"])
    assert op["total"] == int(c["seg_len"].sum())
    # the scatter form: segment i alone, in reverse order, 3 bytes apart
    n = len(c["segs"])
    starts = np.zeros(n, np.int64)
    at = GUARD + 1
    for i in reversed(range(n)):
        starts[i] = at
        at += c["segs"][i].size + 3
    image = np.full(at + GUARD, FILL, np.uint8)
    for i, s in enumerate(c["segs"]):
        image[starts[i]: starts[i] + s.size] = s
    buf = torch_cuda.full((image.size,), FILL, dtype=torch_cuda.uint8, device="cuda")
    codec.decode_batch(op, out=buf, out_off=starts, verify=bool(flags))
    assert codec.batch_status() == 0 and np.array_equal(_np(buf), image)
    # ranges: every segment whole, and a short range in its middle
    rows = []
    for i, s in enumerate(c["segs"]):
        rows.append((i, 0, s.size))
        if s.size > 2:
            rows.append((i, s.size // 2, min(70, s.size - s.size // 2)))
    rows = np.array(rows, np.int64)
    got, goff, rst = codec.decode_batch_ranges(op, rows[:, 0], rows[:, 1], rows[:, 2])
    got, goff = _np(got), _np(goff)
    assert not _np(rst).any()
    for r, (i, f, k) in enumerate(rows.tolist()):
        assert np.array_equal(got[goff[r]: goff[r] + k], c["segs"][i][f: f + k]), r


@pytest.mark.parametrize("count", (0, 1, 1023, 1025, 8193))
def test_open_counts(torch_cuda, codec, count):
    kind = (M.SET, M.OWN, M.OWN4, M.SHARED, M.SET)[(0, 1, 1023, 1025, 8193).index(count)]
    c = container(kind, M.CRC, 2, 16, [(0, 1, 15, 16, 17, 33)[i % 6] for i in range(count)], seed=count)
    _, st, out, _ = open_and_decode(torch_cuda, codec, c, c["blob"], verify=True)
    assert not any(st) and all(np.array_equal(o, s) for o, s in zip(out, c["segs"]))


# ---- the round trip through the host ------------------------------------------------------------
@pytest.mark.parametrize("mode", ("own", "own4", "shared", "set"))
def test_round_trip_of_buffers(torch_cuda, codec, mode):
    from data_compression_amd import huffman
    rng = np.random.default_rng(8)
    bufs = [b"", text(rng, 1).tobytes(), text(rng, 65536).tobytes(), rng.integers(0, 256, 300, dtype=np.uint8).tobytes(),
            text(rng, 4097).tobytes()]
    kw = {"mode": "own", "lens4": True, "max_bits": 15} if mode == "own4" else {"mode": mode}
    blob = huffman.compress_batch(bufs, **kw)
    info = huffman.batch_info(blob)
    assert info["blob_bytes"] == len(blob) and info["count"] == len(bufs) and info["total_bytes"] == sum(map(len, bufs))
    assert info["kind"] == ("own", "own4", "shared", "set").index(mode) and info["flags"] == M.CRC
    assert M.check(blob) == 0 and len(blob) < sum(map(len, bufs))
    assert huffman.decompress_batch(blob) == bufs
    assert huffman.decompress_batch(huffman.compress_batch([], checksum=False)) == []
    assert huffman.decompress_batch(huffman.compress_batch([b"", b""])) == [b"", b""]   # buffers, and not a byte


def test_host_pair_reads_the_models_containers_and_reports_damage(torch_cuda):
    """dc_huff_batch_decompress_host (under huffman.decompress_batch) on containers the model wrote:
    the model's bytes for all four kinds; DC_E_STREAM before any device call for a damaged header
    and directory, the decode's DC_E_STREAM for a sync entry, DC_E_CHECKSUM for a stored byte.
    dc_huff_batch_compress_host against its arguments."""
    import ctypes as C

    from data_compression_amd import huffman
    from data_compression_amd._lib import DcError, core
    for kind in KINDS:
        c = container(kind, M.CRC, 2, 64, [100, 64, 300, 4096, 17, 0, 200], seed=12)
        assert huffman.decompress_batch(c["blob"]) == [s.tobytes() for s in c["segs"]]
        P, a = M.parse(c["blob"]), c["arrays"]
        bad = [blob[:m] for _, blob, m in header_damage(c)] + [blob for what, blob in directory_damage(c, 3) if M.check(blob)]
        bad.append(_flip(c["blob"], P["sync_off"] + 2 * (int(a["sync_off"][3]) + 5)))
        for blob in bad:
            with pytest.raises(DcError) as e:
                huffman.decompress_batch(blob)
            assert e.value.rc == M.DC_E_STREAM
        with pytest.raises(DcError) as e:
            huffman.decompress_batch(_flip(c["blob"], P["payload_off"] + int(a["pay_off"][2]) + 7))
        assert e.value.rc == DC_E_CHECKSUM
    L = core()
    off = (C.c_uint64 * 3)(0, 5, 3)
    src, out, got = (C.c_uint8 * 16)(), (C.c_uint8 * 4096)(), C.c_uint64(0)
    call = lambda o, kind=0, flags=0, S=64, K=0, cap=4096: L.dc_huff_batch_compress_host(
        src, o, 2, 2, S, kind, flags, 0, None, K, out, cap, C.byref(got))
    assert call(off) == M.DC_E_ARG                       # offsets that decrease
    off[2] = 9
    assert call(off, kind=4) == M.DC_E_ARG and call(off, flags=2) == M.DC_E_ARG and call(off, S=48) == M.DC_E_ARG
    assert call(off, cap=64) == M.DC_E_CAPACITY and call(None) == M.DC_E_ARG
    assert call(off) == 0 and M.check(bytes(out[: got.value])) == 0 and M.parse(bytes(out[: got.value]))["len"].tolist() == [5, 4]


# ---- damage -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_header_damage_is_refused_before_the_device(torch_cuda, codec, kind):
    from data_compression_amd._lib import DcError
    c = container(kind, M.CRC, 2, 64, [100, 64, 0, 4096, 17], seed=3)
    for what, blob, m in header_damage(c):
        assert M.check(blob, m) == M.DC_E_STREAM and lib_check(blob, m) == M.DC_E_STREAM, what
        with pytest.raises(DcError) as e:
            codec.batch_open(blob[:m])
        assert e.value.rc == M.DC_E_STREAM, what


@pytest.mark.parametrize("kind", KINDS)
def test_directory_damage(torch_cuda, codec, kind):
    """len + 1, len = 65537, bits +- 1, mode 2 and tid = K at a coded segment in the middle: open
    reports the model's statuses, the decode the model's, every other segment is untouched by it
    unless its offsets moved, and nothing is written outside a decoded segment's own bytes"""
    c = container(kind, M.CRC, 2, 64, [100, 64, 300, 4096, 17, 65, 200], seed=4)
    i = 3
    assert c["arrays"]["mode"][i] == 1
    for what, blob in directory_damage(c, i):
        assert lib_check(blob) == M.check(blob), what
        _, st, _, _ = open_and_decode(torch_cuda, codec, c, blob, verify=what.startswith("bits"))
        assert st[i] != 0, what


def _flip(blob, at, bit=0):
    b = bytearray(blob)
    b[at] ^= 1 << bit
    return bytes(b)


@pytest.mark.parametrize("flags", (0, M.CRC))
@pytest.mark.parametrize("kind", KINDS)
def test_body_damage(torch_cuda, codec, kind, flags):
    """a payload byte of a coded segment and of a stored one, and a sync entry: the container rule
    does not see them; the decode gives model_decode's status, and with CRCs stored a segment that
    decodes to other bytes is DC_E_CHECKSUM"""
    c = container(kind, flags, 2, 64, [100, 64, 300, 4096, 17, 65, 200], seed=6)
    P, a = M.parse(c["blob"]), c["arrays"]
    coded, stored = 3, 2
    assert a["mode"][coded] == 1 and a["mode"][stored] == 0
    cases = [("coded", _flip(c["blob"], P["payload_off"] + int(a["pay_off"][coded]) + 40, 3)),
             ("stored", _flip(c["blob"], P["payload_off"] + int(a["pay_off"][stored]) + 7, 0)),
             ("sync", _flip(c["blob"], P["sync_off"] + 2 * (int(a["sync_off"][coded]) + 5), 0))]
    for what, blob in cases:
        assert M.check(blob) == 0 and lib_check(blob) == 0, what
        _, st, out, _ = open_and_decode(torch_cuda, codec, c, blob, verify=bool(flags))
        seg = {"coded": coded, "stored": stored, "sync": coded}[what]
        assert [k for k in range(len(st)) if st[k]] in ([seg], []), what
        if flags or what == "sync":
            assert st[seg] != 0, what   # a sync entry off by one cannot sum to bits; a CRC sees any other byte
        if what == "stored":
            assert st[seg] == (DC_E_CHECKSUM if flags else 0), what


def test_a_damaged_nybble_of_a_record(torch_cuda, codec):
    """kind 1: the length of a byte the segment holds, one digit longer"""
    c = container(M.OWN4, M.CRC, 2, 64, [100, 64, 300, 4096, 17], seed=7)
    P = M.parse(c["blob"])
    i = 3
    sym = int(c["segs"][i][0])
    lens = M.unpack4(P["records"][i])[0]
    assert 0 < lens[sym] < 15
    b = bytearray(c["blob"])
    at = P["rec_off"] + 128 * i + sym // 2
    b[at] = (b[at] & 0x0F) | ((lens[sym] + 1) << 4) if sym % 2 == 0 else (b[at] & 0xF0) | (lens[sym] + 1)
    blob = bytes(b)
    assert M.check(blob) == 0 and lib_check(blob) == 0
    _, st, _, _ = open_and_decode(torch_cuda, codec, c, blob, verify=True)
    assert st[i] != 0 and not any(st[:i]) and not any(st[i + 1:])
