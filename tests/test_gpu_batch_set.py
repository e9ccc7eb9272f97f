"""The table-set mode of the batched Huffman codec on the device: dc_huff_encode_batch_set /
dc_huff_decode_batch_set / dc_huff_decode_batch_set_ranges / dc_huff_batch_set_select /
dc_huff_batch_set_hist (k_hbm_plan, k_hbm_pack, k_hbm_decode, k_hbm_decode_ranges, k_hbm_hist)
through Codec.encode_batch(..., table_set=) / decode_batch / decode_batch_ranges /
batch_set_select / batch_set_hist / batch_table_set. The reference is the model of
tests/test_batch_set_cpu.py (oracle_set_batch: the selection rule in numpy, payloads from the CPU
oracle) for the encode and the input segments for the decode; every byte nobody asked for must
keep its 0xA5 prefill."""
import ctypes as C

import numpy as np
import pytest

from tests.test_batch_cpu import SEGMENTS, content, pack_offsets
from tests.test_batch_ranges_cpu import segment_ranges
from tests.test_batch_set_cpu import (HEXREC, SET_SEGMENTS, TEXT, X, XY, XY_TIE, Y, YX, _hex_segment, oracle_set_batch,
                                      oracle_test_batch, pad259, record_valid, select, set_records)
from tests.test_batch_shared_cpu import table_codes, text_table
from tests.test_gpu_batch import _dev, _gapped
from tests.test_gpu_batch_ranges import _gapped as _gapped_counts

pytestmark = pytest.mark.gpu

FILL = 0xA5
DC_E_ARG, DC_E_CAPACITY, DC_E_STREAM, DC_E_CHECKSUM = -1, -6, -7, -9
ARRAYS = ("tid", "mode", "bits", "pay_off", "sync_off")


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


def _encode(torch, codec, segs, ts, n_ary=2, S=64, **kw):
    """encode_batch under the set `ts` into 0xA5-filled payload and sync buffers: (enc, x, offsets)."""
    x, off = pack_offsets(segs)
    pb, sb = codec.batch_bounds(x.size, len(segs), S)
    payload = torch.full((pb + 48,), FILL, dtype=torch.uint8, device="cuda")
    sync = torch.full((sb + 5,), -23131, dtype=torch.int16, device="cuda")   # 0xA5A5
    enc = codec.encode_batch(_dev(torch, x), _dev(torch, off), n_ary=n_ary, sync_syms=S, payload=payload, sync_len=sync,
                             table_set=ts, **kw)
    assert enc["table_set"] is ts and enc["lens"] is None and "table" not in enc
    assert enc["tid"].dtype == torch.uint8 and enc["tid"].numel() == len(segs)
    return enc, x, off


def _host(enc):
    h = {k: enc[k].cpu().numpy() for k in ARRAYS + ("payload", "status")}
    h["sync_len"] = enc["sync_len"].cpu().numpy().view(np.uint16)
    return h


def _check_encode(h, exp, tag, skip=()):
    """Every array equals the model's, pads included; segments in `skip` wrote no tid / mode / bits."""
    keep = np.array([i not in skip for i in range(len(exp["mode"]))], bool)
    for k in ("tid", "mode", "bits"):
        assert np.array_equal(h[k][keep], exp[k][keep]), tag + (k,)
    for k in ("pay_off", "sync_off"):
        assert np.array_equal(h[k], exp[k]), tag + (k,)
    end = int(exp["pay_off"][-1])
    assert np.array_equal(h["payload"][:end], exp["payload"]), tag + ("payload, pads included",)
    assert (h["payload"][end:] == FILL).all(), tag + ("payload past pay_off[count] written",)
    send = int(exp["sync_off"][-1])
    assert np.array_equal(h["sync_len"][:send], exp["sync_len"]), tag + ("sync_len",)
    assert (h["sync_len"][send:] == 0xA5A5).all(), tag + ("sync_len past sync_off[count] written",)


def _check_decode(torch, codec, enc, segs, tag, bad=None, cap=None, verify=False, wrong=()):
    """ONE scatter decode into a 0xA5 buffer (of `cap` bytes) at gapped, odd offsets: every segment
    not in `bad` (index -> expected status) equals its input, every other byte is untouched
    (`wrong`: segments whose bytes are not looked at). Returns the decoded buffer and the starts."""
    bad = bad or {}
    starts, full = _gapped(segs)
    cap = full if cap is None else cap
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    codec.decode_batch(enc, out=out, out_off=starts, verify=verify)
    st = enc["status"].cpu().numpy()
    h = out.cpu().numpy()
    asked = np.zeros(cap, bool)
    for i, (s, o) in enumerate(zip(segs, starts)):
        if i in bad:
            assert st[i] == bad[i], tag + (i, "status", int(st[i]))
            if bad[i] == DC_E_CHECKSUM:   # decoded clean, then refused by the verify: its bytes are there
                asked[o: o + s.size] = True
            continue
        assert st[i] == 0, tag + (i, int(st[i]))
        if i not in wrong:
            assert np.array_equal(h[o: o + s.size], s), tag + (i, "decoded bytes")
        asked[o: o + s.size] = True
    assert (h[~asked] == FILL).all(), tag + ("bytes outside the good segments written",)
    assert codec.batch_status() == (bad[min(bad)] if bad else 0), tag + ("batch_status",)
    return h, starts


def _grid(codec, grid):
    class _G:
        def __enter__(self):
            codec.set_option("batch_grid", grid)

        def __exit__(self, *a):
            codec.set_option("batch_grid", 0)
    return _G()


# ---- 1: the encode is the model's batch ----------------------------------------------------------
@pytest.mark.parametrize("n_ary,S", [(2, 64), (3, 64), (16, 64), (17, 64), (256, 64), (2, 16), (2, 1024)])
def test_encode_is_the_models_batch_and_round_trips(torch_cuda, codec, n_ary, S):
    ts = codec.table_set(set_records(n_ary), n_ary)
    assert ts.shape == (7, 256) and ts.dtype == torch_cuda.uint8 and ts.data_ptr() % 16 == 0
    enc, x, off = _encode(torch_cuda, codec, SET_SEGMENTS, ts, n_ary, S)
    assert codec.batch_status() == 0
    h = _host(enc)
    assert (h["status"] == 0).all()
    _check_encode(h, oracle_test_batch(n_ary, S), (n_ary, S))
    _check_decode(torch_cuda, codec, enc, SET_SEGMENTS, (n_ary, S))


def test_contiguous_decode_is_the_default(torch_cuda, codec):
    ts = codec.table_set(set_records(2), 2)
    enc, x, off = _encode(torch_cuda, codec, SET_SEGMENTS, ts)
    out, out_off = codec.decode_batch(enc)
    assert codec.batch_status() == 0
    assert np.array_equal(out.cpu().numpy(), x) and np.array_equal(out_off.cpu().numpy(), off)


def test_python_argument_rules(torch_cuda, codec):
    torch = torch_cuda
    ts = codec.table_set(set_records(2), 2)
    x, off = pack_offsets(SEGMENTS[:3])
    tab = codec.table_lengths(_dev(torch, text_table(2)), 2)
    with pytest.raises(ValueError):
        codec.encode_batch(_dev(torch, x), _dev(torch, off), table_set=ts, table=tab)
    with pytest.raises(ValueError):
        codec.encode_batch(_dev(torch, x), _dev(torch, off), table_set=ts, max_bits=12)
    with pytest.raises(ValueError):
        codec.table_set([], 2)
    with pytest.raises(ValueError):
        codec.table_set([np.zeros(256, np.uint8)] * 65, 2)
    # a device table is a record by its lengths; more than 256 entries are cut
    a = codec.table_set([tab, text_table(2), text_table(2)[:256].tolist()], 2).cpu().numpy()
    assert np.array_equal(a[0], text_table(2)[:256]) and np.array_equal(a[1], a[0]) and np.array_equal(a[2], a[0])
    # without table_set the result is what it was
    enc = codec.encode_batch(_dev(torch, x), _dev(torch, off))
    assert "table_set" not in enc and "tid" not in enc and enc["lens"] is not None


# ---- 2: K = 1 is the shared mode -----------------------------------------------------------------
@pytest.mark.parametrize("n_ary", (2, 17))
def test_one_record_is_the_shared_mode(torch_cuda, codec, n_ary):
    """Device against device: the shared-table kernels are the reference of every array."""
    torch = torch_cuda
    rec = text_table(n_ary)[:256]
    enc, x, off = _encode(torch, codec, SEGMENTS, codec.table_set([rec], n_ary), n_ary)
    assert codec.batch_status() == 0
    pb, sb = codec.batch_bounds(x.size, len(SEGMENTS), 64)
    payload = torch.full((pb + 48,), FILL, dtype=torch.uint8, device="cuda")
    sync = torch.full((sb + 5,), -23131, dtype=torch.int16, device="cuda")
    ref = codec.encode_batch(_dev(torch, x), _dev(torch, off), n_ary=n_ary, payload=payload, sync_len=sync,
                             table=codec.table_lengths(_dev(torch, pad259(rec)), n_ary))
    assert codec.batch_status() == 0
    assert set(ref["mode"].cpu().tolist()) == ({0, 1})
    for name in ("mode", "bits", "pay_off", "sync_off", "payload", "sync_len", "status"):
        assert torch.equal(enc[name], ref[name]), name
    assert not enc["tid"].any()
    two, _, _ = _encode(torch, codec, SEGMENTS, codec.table_set([rec, rec], n_ary), n_ary)
    assert not two["tid"].any()
    for name in ("mode", "bits", "pay_off", "sync_off", "payload", "sync_len", "status"):
        assert torch.equal(two[name], ref[name]), name


# ---- 3: K = 64 -----------------------------------------------------------------------------------
def test_sixty_four_records(torch_cuda, codec):
    torch = torch_cuda
    text, zeros = text_table(2)[:256], np.zeros(256, np.uint8)
    last = [zeros] * 63 + [text]
    exp = oracle_set_batch(SEGMENTS, last, 2, 64)
    coded = exp["mode"] == 1
    assert coded.sum() >= 5 and (exp["tid"][coded] == 63).all() and set(exp["tid"].tolist()) == {0, 63}
    enc, _, _ = _encode(torch, codec, SEGMENTS, codec.table_set(last, 2))
    assert codec.batch_status() == 0
    _check_encode(_host(enc), exp, ("text last",))
    _check_decode(torch, codec, enc, SEGMENTS, ("text last",))
    both = [text] + [zeros] * 62 + [text]
    exp = oracle_set_batch(SEGMENTS, both, 2, 64)
    assert not exp["tid"].any()
    enc, _, _ = _encode(torch, codec, SEGMENTS, codec.table_set(both, 2))
    _check_encode(_host(enc), exp, ("text first and last",))


# ---- 4: the table a workgroup keeps --------------------------------------------------------------
def _cache_segments():
    """Records A, A, (a bad tid), (stored), B, A on neighbouring segments."""
    segs = [content("enwik", 4096, 31), content("enwik", 5000, 32), content("enwik", 3000, 33), content("cycle", 4096, 0),
            SET_SEGMENTS[len(SEGMENTS) + 2], content("enwik", 4097, 34)]
    return segs, 2, 3   # the segment whose tid the decode test breaks, the stored one


@pytest.mark.parametrize("grid", (1, 1024))
def test_the_kept_table(torch_cuda, codec, grid):
    torch = torch_cuda
    segs, k_bad, k_stored = _cache_segments()
    recs = set_records(2)
    exp = oracle_set_batch(segs, recs, 2, 64)
    assert exp["tid"].tolist() == [TEXT, TEXT, TEXT, 0, HEXREC, TEXT] and exp["mode"].tolist() == [1, 1, 1, 0, 1, 1]
    assert grid == 1 or grid > len(segs)
    with _grid(codec, grid):
        enc, _, _ = _encode(torch, codec, segs, codec.table_set(recs, 2))
        assert codec.batch_status() == 0
        _check_encode(_host(enc), exp, ("kept table", grid))
        _check_decode(torch, codec, enc, segs, ("kept table", grid))
        enc = dict(enc, tid=enc["tid"].clone())
        enc["tid"][k_bad] = len(recs)
        enc["tid"][k_stored] = 200        # a stored segment reads no tid
        _check_decode(torch, codec, enc, segs, ("kept table, bad tid", grid), bad={k_bad: DC_E_STREAM})


def _dealt_segments():
    """Groups of four as the decoder deals them: short segments of one record (and stored ones) go
    one to a wave; a group with a segment over 8192 bytes or with two records goes to the workgroup."""
    hexs = lambda n, seed: _hex_segment(n, seed)
    groups = [
        [("enwik", 8192), ("enwik", 8191), ("cycle", 8192), ("enwik", 100)],    # one record and a stored one: waves
        [("enwik", 8193), ("enwik", 8192), ("hex", 700), ("enwik", 8192)],      # a long one: the workgroup
        [("hex", 8192), ("hex", 1), ("cycle", 8190), ("hex", 8192)],            # waves, another record
        [("enwik", 8192), ("hex", 8192), ("enwik", 300), ("hex", 17)],          # short, two records: the workgroup
        [("cycle", 4096), ("cycle", 8192), ("cycle", 1), ("cycle", 300)],       # all stored: waves, no table
        [("hex", 300), ("hex", 8192)],                                          # a last group of two
    ]
    flat = [kn for g in groups for kn in g]
    return [hexs(n, 50 + j) if kind == "hex" else content(kind, n, 70 + j) for j, (kind, n) in enumerate(flat)]


@pytest.mark.parametrize("grid", (0, 1))
@pytest.mark.parametrize("S", (64, 16))
def test_decode_paths_meet_at_8_kib(torch_cuda, codec, S, grid):
    segs = _dealt_segments()
    recs = set_records(2)
    exp = oracle_set_batch(segs, recs, 2, S)
    T, H = TEXT, HEXREC
    assert exp["tid"].tolist() == [T, T, 0, T,  T, T, H, T,  H, H, 0, H,  T, H, T, H,  0, 0, 0, 0,  H, H]
    assert exp["mode"].tolist() == [1, 1, 0, 1,  1, 1, 1, 1,  1, 1, 0, 1,  1, 1, 1, 1,  0, 0, 0, 0,  1, 1]
    with _grid(codec, grid):
        enc, _, _ = _encode(torch_cuda, codec, segs, codec.table_set(recs, 2), S=S)
        assert codec.batch_status() == 0
        _check_encode(_host(enc), exp, ("8 KiB", S, grid))
        _check_decode(torch_cuda, codec, enc, segs, ("8 KiB", S, grid))
        # a tid that names no record sends its group to the workgroup, where the segment fails alone
        enc = dict(enc, tid=enc["tid"].clone())
        enc["tid"][1] = len(recs)
        enc["tid"][9] = 255
        enc["tid"][17] = 255   # stored: not read
        enc["tid"][20] = enc["tid"][21] = 255   # a whole group under one tid that names no record
        _check_decode(torch_cuda, codec, enc, segs, ("8 KiB, bad tid", S, grid), bad={i: DC_E_STREAM for i in (1, 9, 20, 21)})


# ---- 5: decode failures stand alone --------------------------------------------------------------
def _too_long_record():
    rec = np.zeros(256, np.uint8)
    rec[[X, Y]] = (1, 33)   # a code of 33 bits: hb_canonical's bad
    return rec


@pytest.mark.parametrize("grid", (0, 1))
@pytest.mark.parametrize("what", ("K", "255", "33 bits"))
def test_a_bad_tid_fails_alone(torch_cuda, codec, what, grid):
    """Grid 1: the workgroup that failed to build a table builds its neighbour's again."""
    torch = torch_cuda
    recs = set_records(2) + [_too_long_record()]
    assert not record_valid(recs[-1], 2)
    segs = [SEGMENTS[5], SEGMENTS[10], content("enwik", 3000, 41), content("cycle", 4096, 0), content("enwik", 700, 42)]
    exp = oracle_set_batch(segs, recs, 2, 64)
    assert exp["mode"].tolist() == [1, 1, 1, 0, 1] and exp["tid"].tolist() == [TEXT] * 3 + [0, TEXT]
    ts = codec.table_set(recs, 2)
    enc, _, _ = _encode(torch, codec, segs, ts)
    _check_encode(_host(enc), exp, (what,))
    value = {"K": len(recs), "255": 255, "33 bits": len(recs) - 1}[what]
    enc = dict(enc, tid=enc["tid"].clone())
    enc["tid"][3] = value                 # the stored segment: decodes
    with _grid(codec, grid):
        _check_decode(torch, codec, enc, segs, (what, "stored"))
        enc["tid"][1] = value
        _check_decode(torch, codec, enc, segs, (what,), bad={1: DC_E_STREAM})
        enc["tid"][2] = value
        _check_decode(torch, codec, enc, segs, (what, "two"), bad={1: DC_E_STREAM, 2: DC_E_STREAM})


def test_a_wrong_valid_record_is_seen_by_the_checksum(torch_cuda, codec):
    """XY and YX give X and Y each other's code: a segment of X and Y alone decodes under the wrong
    one to exactly as many symbols in exactly the bits of every chunk, so the chunk check passes
    with wrong bytes, and only the CRC-32 of the segment sees it."""
    torch = torch_cuda
    recs = set_records(2)
    (ca, na), (cb, nb) = table_codes(pad259(recs[XY]), 2), table_codes(pad259(recs[YX]), 2)
    assert (ca[X], na[X]) == (cb[Y], nb[Y]) and (ca[Y], na[Y]) == (cb[X], nb[X])   # the model: the bit strings swap
    seg = SET_SEGMENTS[XY_TIE]
    assert set(seg.tolist()) == {X, Y} and select(seg, recs, 2)[0] == XY
    segs = [SEGMENTS[10], seg, content("enwik", 3000, 41), content("enwik", 700, 42)]
    enc, _, _ = _encode(torch, codec, segs, codec.table_set(recs, 2), checksum=True)
    assert enc["tid"].cpu().tolist() == [TEXT, XY, TEXT, TEXT]
    _check_decode(torch, codec, enc, segs, ("right record",), verify=True)
    enc = dict(enc, tid=enc["tid"].clone())
    enc["tid"][1] = YX
    h, starts = _check_decode(torch, codec, enc, segs, ("wrong record, no verify",), wrong=(1,))
    swapped = np.where(seg == X, Y, X).astype(np.uint8)
    assert np.array_equal(h[starts[1]: starts[1] + seg.size], swapped)   # clean by the chunk check, and wrong
    _check_decode(torch, codec, enc, segs, ("wrong record",), bad={1: DC_E_CHECKSUM}, verify=True, wrong=(1,))
    # a text segment under the hex record: the stream check or the checksum, never DC_OK
    enc["tid"][1] = XY
    enc["tid"][2] = HEXREC
    starts, cap = _gapped(segs)
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    codec.decode_batch(enc, out=out, out_off=starts, verify=True)
    st = enc["status"].cpu().tolist()
    assert st[2] in (DC_E_STREAM, DC_E_CHECKSUM) and [st[0], st[1], st[3]] == [0, 0, 0]
    assert codec.batch_status() == st[2]


# ---- 6: caps and offsets -------------------------------------------------------------------------
def test_payload_cap_inside_a_segment(torch_cuda, codec):
    recs = set_records(2)
    segs = [SEGMENTS[6], SET_SEGMENTS[len(SEGMENTS) + 2], SEGMENTS[9], SEGMENTS[7], SET_SEGMENTS[XY_TIE]]
    exp = oracle_set_batch(segs, recs, 2, 64)
    k = 2
    pcut, scut = int(exp["pay_off"][k]), int(exp["sync_off"][k])
    cap = pcut + 16
    assert cap < exp["pay_off"][k + 1]
    enc, _, _ = _encode(torch_cuda, codec, segs, codec.table_set(recs, 2), payload_cap=cap)
    assert codec.batch_status() == DC_E_CAPACITY
    h = _host(enc)
    assert h["status"].tolist() == [0, 0] + [DC_E_CAPACITY] * 3
    assert np.array_equal(h["payload"][:pcut], exp["payload"][:pcut])
    assert (h["payload"][pcut:] == FILL).all()      # nothing of segment k, nothing at or past the cap
    assert np.array_equal(h["sync_len"][:scut], exp["sync_len"][:scut])
    assert (h["sync_len"][scut:] == 0xA5A5).all()
    for name in ARRAYS:
        assert np.array_equal(h[name], exp[name]), name
    _check_decode(torch_cuda, codec, enc, segs, ("payload_cap",), bad={i: DC_E_STREAM for i in (2, 3, 4)})


def test_bad_offsets_fail_alone_and_write_nothing(torch_cuda, codec):
    """A decreasing offset pair and a segment of 65 537 bytes: DC_E_ARG, and tid / mode / bits of
    those segments keep their prefill (the arrays are the caller's: the C call on an HBatch)."""
    torch = torch_cuda
    from data_compression_amd._lib import HBatch
    recs = set_records(2)
    good = [SEGMENTS[6], SEGMENTS[10], SET_SEGMENTS[len(SEGMENTS) + 1], SEGMENTS[9]]
    x = np.concatenate(good[:2] + [content("enwik", 65537, 1)] + good[2:])
    cuts = np.cumsum([0] + [s.size for s in good[:2]] + [65537] + [s.size for s in good[2:]])
    # segments: good0, good1, [long], then a pair that decreases, then good2 and good3
    off = np.array([cuts[0], cuts[1], cuts[2], cuts[3], cuts[3] - 7, cuts[3], cuts[4], cuts[5]], np.int64)
    segs = [good[0], good[1], None, None, x[cuts[3] - 7: cuts[3]], good[2], good[3]]
    count, bad = len(off) - 1, (2, 3)
    assert off[3] - off[2] == 65537 and off[4] < off[3]
    model = [np.zeros(0, np.uint8) if s is None else s for s in segs]   # 0 payload bytes, 0 sync entries
    exp = oracle_set_batch(model, recs, 2, 64)
    pb, sb = codec.batch_bounds(x.size, count, 64)
    ts = codec.table_set(recs, 2)
    enc = {"count": count, "n_ary": 2, "S": 64, "offsets": _dev(torch, off), "total": x.size, "lens": None,
           "table_set": ts, "tid": torch.full((count,), FILL, dtype=torch.uint8, device="cuda"),
           "mode": torch.full((count,), FILL, dtype=torch.uint8, device="cuda"),
           "bits": torch.full((count,), -1515870811, dtype=torch.int32, device="cuda"),   # 0xA5A5A5A5
           "pay_off": torch.zeros(count + 1, dtype=torch.int64, device="cuda"),
           "payload": torch.full((pb + 48,), FILL, dtype=torch.uint8, device="cuda"),
           "sync_off": torch.zeros(count + 1, dtype=torch.int64, device="cuda"),
           "sync_len": torch.full((sb + 5,), -23131, dtype=torch.int16, device="cuda"),
           "status": torch.full((count,), -99, dtype=torch.int32, device="cuda")}
    enc["payload_cap"], enc["sync_cap"] = enc["payload"].numel(), enc["sync_len"].numel()
    b = codec._hbatch(enc)
    xd = _dev(torch, x)
    assert codec.L.dc_huff_encode_batch_set(codec.ctx, xd.data_ptr(), enc["offsets"].data_ptr(), count, ts.data_ptr(),
                                            ts.shape[0], enc["tid"].data_ptr(), C.byref(b)) == 0
    assert codec.batch_status() == DC_E_ARG
    h = _host(enc)
    assert h["status"].tolist() == [DC_E_ARG if i in bad else 0 for i in range(count)]
    for i in bad:
        assert (h["tid"][i], h["mode"][i], h["bits"][i]) == (FILL, FILL, -1515870811), i
    _check_encode(h, exp, ("bad offsets",), skip=bad)
    # select writes the same four arrays, and leaves the same entries alone
    sel = {k: torch.full_like(enc[k], 0x5A) for k in ("tid", "mode", "bits", "status")}
    assert codec.L.dc_huff_batch_set_select(codec.ctx, xd.data_ptr(), enc["offsets"].data_ptr(), count, 2, ts.data_ptr(),
                                            ts.shape[0], *(sel[k].data_ptr() for k in ("tid", "mode", "bits", "status"))) == 0
    assert codec.batch_status() == DC_E_ARG
    keep = np.array([i not in bad for i in range(count)])
    for k in ("tid", "mode", "bits"):
        got = sel[k].cpu().numpy()
        assert np.array_equal(got[keep], h[k][keep]) and (got[~keep] == sel[k].new_full((1,), 0x5A).cpu().numpy()).all(), k
    assert np.array_equal(sel["status"].cpu().numpy(), h["status"])


# ---- 7: byte ranges ------------------------------------------------------------------------------
def _range_rows(segs, S, total=256, seed=5):
    """`total` (seg, first, count) rows: the ranges of tests/test_batch_ranges_cpu.py (first and last
    byte, chunk edges +- 1, a whole segment, count 0) of the added segments and of every third of
    SEGMENTS, then seeded random ranges."""
    rows = []
    order = list(range(len(SEGMENTS), len(segs))) + list(range(0, len(SEGMENTS), 3))
    for i in order:
        rows += [(i, f, c) for f, c in segment_ranges(segs[i].size, S)]
    assert len(rows) <= total
    rng = np.random.default_rng(seed)
    full = [i for i, s in enumerate(segs) if s.size]
    while len(rows) < total:
        i = full[int(rng.integers(len(full)))]
        f = int(rng.integers(segs[i].size))
        rows.append((i, f, int(rng.integers(1, min(segs[i].size - f, 600) + 1))))
    return np.array(rows, np.int64)


def _run_ranges(torch, codec, enc, rows, segs, tag, bad=None):
    bad = bad or {}
    offs, cap = _gapped_counts(rows[:, 2])
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    before = enc["status"].clone()
    got, _, st = codec.decode_batch_ranges(enc, _dev(torch, rows[:, 0]), _dev(torch, rows[:, 1]), _dev(torch, rows[:, 2]),
                                           out=out, out_off=_dev(torch, offs))
    assert got is out and torch.equal(enc["status"], before), "the batch's d_status was written"
    h, st = out.cpu().numpy(), st.cpu().numpy()
    asked = np.zeros(cap, bool)
    for r, ((i, f, c), o) in enumerate(zip(rows.tolist(), offs)):
        if r in bad:
            assert st[r] == bad[r], tag + (r, (i, f, c), "status", int(st[r]))
            continue
        assert st[r] == 0, tag + (r, (i, f, c), int(st[r]))
        assert np.array_equal(h[o: o + c], segs[i][f: f + c]), tag + (r, (i, f, c), "decoded bytes")
        asked[o: o + c] = True
    assert (h[~asked] == FILL).all(), tag + ("bytes outside the good ranges written",)
    assert codec.batch_status() == (bad[min(bad)] if bad else 0), tag + ("batch_status",)


@pytest.mark.parametrize("grid", (0, 3))
def test_ranges_sorted_and_unsorted(torch_cuda, codec, grid):
    """Grid 3: each workgroup walks some 85 ranges and keeps its table between those of one tid."""
    torch = torch_cuda
    recs = set_records(2)
    enc, _, _ = _encode(torch, codec, SET_SEGMENTS, codec.table_set(recs, 2))
    assert codec.batch_status() == 0
    tid, mode = enc["tid"].cpu().numpy(), enc["mode"].cpu().numpy()
    rows = _range_rows(SET_SEGMENTS, 64)
    assert len(rows) == 256 and (rows[:, 2] == 0).any()
    assert any(c == SET_SEGMENTS[i].size and c > 64 for i, f, c in rows.tolist())   # a whole segment
    assert {int(tid[i]) for i in rows[:, 0] if mode[i]} == {TEXT, HEXREC, XY, YX} and (mode[rows[:, 0]] == 0).any()
    with _grid(codec, grid):
        _run_ranges(torch, codec, enc, rows, SET_SEGMENTS, ("unsorted", grid))
        by_tid = rows[np.argsort(tid[rows[:, 0]], kind="stable")]
        _run_ranges(torch, codec, enc, by_tid, SET_SEGMENTS, ("sorted by tid", grid))
        # a bad tid: every range with bytes of that segment fails alone when it is coded, none when it is stored
        coded = len(SEGMENTS) + 2
        stored = next(i for i, s in enumerate(SET_SEGMENTS) if s.size >= 4096 and not mode[i])
        assert mode[coded] == 1 and ((rows[:, 0] == coded) & (rows[:, 2] > 0)).sum() >= 3 and (rows[:, 0] == stored).any()
        broken = dict(enc, tid=enc["tid"].clone())
        broken["tid"][coded] = len(recs)
        broken["tid"][stored] = 255
        bad = {r: DC_E_STREAM for r, (i, f, c) in enumerate(by_tid.tolist()) if i == coded and c > 0}
        _run_ranges(torch, codec, broken, by_tid, SET_SEGMENTS, ("bad tid", grid), bad=bad)


# ---- 8: select is the encode's plan --------------------------------------------------------------
def test_select_is_the_encodes_plan(torch_cuda, codec):
    torch = torch_cuda
    ts = codec.table_set(set_records(2), 2)
    enc, x, off = _encode(torch, codec, SET_SEGMENTS, ts)
    payload, sync = enc["payload"].clone(), enc["sync_len"].clone()
    sentinel = torch.full_like(payload, 0x3C)
    codec.timing(True)
    tid, mode, bits, status = codec.batch_set_select(_dev(torch, x), _dev(torch, off), ts)
    names = [n for n, _ in codec.timings()]
    codec.timing(False)
    assert names == ["hbm_plan"]
    assert codec.batch_status() == 0
    for got, name in ((tid, "tid"), (mode, "mode"), (bits, "bits"), (status, "status")):
        assert got.dtype == enc[name].dtype and torch.equal(got, enc[name]), name
    assert torch.equal(enc["payload"], payload) and torch.equal(enc["sync_len"], sync) and (sentinel == 0x3C).all()
    exp = oracle_test_batch(2, 64)
    assert np.array_equal(tid.cpu().numpy(), exp["tid"]) and np.array_equal(bits.cpu().numpy(), exp["bits"])


def test_launches_do_not_depend_on_count(torch_cuda, codec):
    ts = codec.table_set(set_records(2), 2)
    stages = {}
    for segs in (SEGMENTS[5:6], SET_SEGMENTS):
        codec.timing(True)
        enc, _, _ = _encode(torch_cuda, codec, segs, ts)
        ne = [n for n, _ in codec.timings()]
        codec.timing(True)
        codec.decode_batch(enc)
        nd = [n for n, _ in codec.timings()]
        codec.timing(False)
        stages[len(segs)] = (ne, nd)
    assert stages[1] == stages[len(SET_SEGMENTS)]
    assert stages[1] == (["hbm_plan", "hb_scan_pay", "hb_scan_sync", "hbm_pack"], ["hbm_decode"])


def test_count_zero_is_ok(torch_cuda, codec):
    torch = torch_cuda
    ts = codec.table_set(set_records(2), 2)
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    codec.timing(True)
    enc = codec.encode_batch(empty, zero, table_set=ts)
    assert enc["count"] == 0 and enc["table_set"] is ts and enc["tid"].numel() == 0
    out, _ = codec.decode_batch(enc)
    assert out.numel() == 0
    assert all(t.numel() == 0 for t in codec.batch_set_select(empty, zero, ts))
    assert codec.timings() == []   # no launch
    codec.timing(False)
    assert not codec.batch_set_hist(empty, zero, enc["tid"], 3).any()
    assert codec.encode_blocks(empty, table_set=ts)["count"] == 0


# ---- 9: the histograms per record ----------------------------------------------------------------
@pytest.mark.parametrize("grid", (0, 2))
def test_hist_is_numpy(torch_cuda, codec, grid):
    torch = torch_cuda
    K = 5
    x, off = pack_offsets(SEGMENTS)
    assert (off[1:-1] % 2 == 1).any()   # inputs at odd byte offsets
    tid = np.array([(3 * i) % K for i in range(len(SEGMENTS))], np.uint8)
    tid[tid == 2] = 4                   # record 2 stays empty
    tid[7] = K                          # skipped, as is 200
    tid[12] = 200
    exp = np.zeros((K, 256), np.int64)
    for s, k in zip(SEGMENTS, tid):
        if k < K:
            exp[k] += np.bincount(s, minlength=256)
    assert all(exp[k].any() for k in (0, 1, 3, 4)) and not exp[2].any()
    with _grid(codec, grid):
        codec.timing(True)
        got = codec.batch_set_hist(_dev(torch, x), _dev(torch, off), _dev(torch, tid), K)
        names = [n for n, _ in codec.timings()]
        codec.timing(False)
    assert names == ["hbm_hist"] and got.dtype == torch.int64 and got.shape == (K, 256)
    assert np.array_equal(got.cpu().numpy(), exp)
    # bad offsets are skipped
    off2 = off.copy()
    off2[5] = off2[4] - 1 if off2[4] else off2[5]
    exp2 = np.zeros((K, 256), np.int64)
    for i, k in enumerate(tid):
        a, b = int(off2[i]), int(off2[i + 1])
        if k < K and a <= b <= a + 65536:
            exp2[k] += np.bincount(x[a:b], minlength=256)
    got = codec.batch_set_hist(_dev(torch, x), _dev(torch, off2), _dev(torch, tid), K)
    assert np.array_equal(got.cpu().numpy(), exp2) and not np.array_equal(exp, exp2)


# ---- 10: training --------------------------------------------------------------------------------
def test_training(torch_cuda, codec):
    torch = torch_cuda
    from data_compression_amd import synth
    q = 1 << 18
    hexes = np.frombuffer(b"0123456789abcdef", np.uint8)[np.random.default_rng(9).integers(0, 16, q)]
    x = np.concatenate([synth.enwik_like(q, seed=1), hexes, synth.log_like(q, seed=2), synth.zipf_bytes(q, seed=3)])
    assert x.size == 1 << 20
    xd = _dev(torch, x)
    off = torch.arange(0, x.size + 1, 4096, dtype=torch.int64, device="cuda")
    ts = codec.batch_table_set(xd, off, 4)
    assert ts.shape == (4, 256) and ts.dtype == torch.uint8
    recs = ts.cpu().numpy()
    for k in range(4):
        assert codec.L.dc_huff_batch_set_table_ok(np.ascontiguousarray(recs[k]).ctypes.data, 2) == 1, k
    assert (recs[0] > 0).all() and recs.max() <= 12   # record 0 covers every byte; max_bits = 12
    assert torch.equal(codec.batch_table_set(xd, off, 4), ts)   # deterministic
    enc = codec.encode_blocks(xd, 4096, table_set=ts, checksum=True)
    assert codec.batch_status() == 0
    ref = codec.encode_blocks(xd, 4096, table=codec.table_lengths(_dev(torch, pad259(recs[0])), 2))
    assert codec.batch_status() == 0
    bits, ref_bits = enc["bits"].cpu().numpy().astype(np.int64), ref["bits"].cpu().numpy().astype(np.int64)
    assert (bits <= ref_bits).all() and bits.sum() <= ref_bits.sum()   # by construction: record 0 is in the set
    out, _ = codec.decode_batch(enc, verify=True)
    assert codec.batch_status() == 0 and np.array_equal(out.cpu().numpy(), x)
