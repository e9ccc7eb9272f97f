"""The capped Huffman batch on the device: dc_huff_encode_batch_limit (k_hb_plan<true>) through
Codec.encode_batch(max_bits=), bit-exact against tests/test_batch_limit_cpu.py's model in every
array and decoded by every decode call; and the nybble form of the lens records
(dc_huff_batch_lens_pack / _unpack) against the numpy form. Every byte nobody asked for must keep
its 0xA5 prefill."""
import ctypes as C

import numpy as np
import pytest

from tests.test_batch_cpu import SEGMENTS, content, oracle_batch, pack_offsets
from tests.test_batch_limit_cpu import (CASES, CONFIGS, DC_E_CODE_TOO_LONG, HAND, lens_pack, lens_unpack,
                                        oracle_batch_limit)
from tests.test_gpu_batch import FILL, _check_decode, _check_encode, _dev, _encode, _host, _small_segments

pytestmark = pytest.mark.gpu

DC_E_ARG, DC_E_CAPACITY, DC_E_STREAM = -1, -6, -7


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


def _w(n):
    return max(n - 1, 1).bit_length()


def _ranges(segs, S):
    """One range inside each non-empty segment: the first chunk and a byte of the next, the last
    chunk with a byte of the one before, or a piece from the middle, in turn."""
    seg, first, count = [], [], []
    for i, s in enumerate(segs):
        n = s.size
        if n == 0:
            continue
        if i % 3 == 0:
            f, c = 0, min(n, S + 1)
        elif i % 3 == 1:
            f = max(0, n - (n - 1) % S - 2)
            c = n - f
        else:
            f = n // 3
            c = min(n - f, 2 * S + 3)
        seg.append(i), first.append(f), count.append(c)
    return seg, first, count


def _check_all_decodes(torch, codec, enc, segs, x, S, tag):
    _check_decode(torch, codec, enc, segs, tag)                    # the scatter form, gapped and odd
    out, _ = codec.decode_batch(enc)                               # back to back
    assert codec.batch_status() == 0 and np.array_equal(out.cpu().numpy(), x), tag + ("contiguous",)
    seg, first, count = _ranges(segs, S)
    out, out_off, st = codec.decode_batch_ranges(enc, seg, first, count)
    assert codec.batch_status() == 0 and not st.cpu().numpy().any(), tag + ("ranges status",)
    h, oo = out.cpu().numpy(), out_off.cpu().numpy()
    for r, (i, f, c) in enumerate(zip(seg, first, count)):
        assert np.array_equal(h[oo[r]: oo[r] + c], segs[i][f: f + c]), tag + ("range", r, i)


@pytest.mark.parametrize("S", (16, 64))
@pytest.mark.parametrize("n_ary,D", CONFIGS)
def test_capped_encode_is_bit_exact_and_decodes(torch_cuda, codec, n_ary, D, S):
    enc, x, off = _encode(torch_cuda, codec, CASES, n_ary, S, max_bits=D * _w(n_ary))
    assert codec.batch_status() == 0 and enc["max_bits"] == D * _w(n_ary)
    h = _host(enc)
    assert (h["status"] == 0).all()
    exp = oracle_batch_limit(CASES, n_ary, S, D)
    _check_encode(h, exp, (n_ary, D, S))
    _check_all_decodes(torch_cuda, codec, enc, CASES, x, S, (n_ary, D, S))


def _raw_limit(torch, codec, like, x, off, max_digits):
    """dc_huff_encode_batch_limit itself into fresh 0xA5 arrays shaped as the batch `like`."""
    enc = dict(like)
    for k in ("lens", "mode", "bits", "pay_off", "payload", "sync_off", "sync_len", "status"):
        enc[k] = like[k].clone()
        enc[k].view(torch.uint8).fill_(FILL)
    b = codec._hbatch(enc)
    rc = codec.L.dc_huff_encode_batch_limit(codec.ctx, x.data_ptr(), off.data_ptr(), enc["count"], max_digits, C.byref(b))
    return rc, enc


def test_no_cap_is_the_unlimited_call(torch_cuda, codec):
    torch = torch_cuda
    like, x, off = _encode(torch, codec, SEGMENTS)
    xd, od = _dev(torch, x), _dev(torch, off)
    codec.timing(True)
    codec.encode_batch(xd, od)
    names = [n for n, _ in codec.timings()]
    codec.timing(True)
    rc, enc = _raw_limit(torch, codec, like, xd, od, 0)
    assert rc == 0 and [n for n, _ in codec.timings()] == names   # the same kernels
    codec.timing(False)
    assert codec.batch_status() == 0
    for k in ("lens", "mode", "bits", "pay_off", "payload", "sync_off", "sync_len", "status"):
        assert torch.equal(enc[k].view(torch.uint8), like[k].view(torch.uint8)), k   # the 0xA5 past the ends included


def test_a_cap_that_binds_nowhere_is_the_unlimited_batch(torch_cuda, codec):
    enc, x, off = _encode(torch_cuda, codec, SEGMENTS, max_bits=32)
    assert codec.batch_status() == 0
    _check_encode(_host(enc), oracle_batch(SEGMENTS, 2, 64), ("D = 32",))


@pytest.mark.parametrize("grid", (1, 2))
def test_one_workgroup_takes_every_kind_of_segment_in_turn(torch_cuda, codec, grid):
    """Binding, non-binding, no code, empty, one byte, binding again at D = 7: nothing of a segment
    (the failed repair's flag, the class counts, the zeroed record) reaches the next one."""
    segs = [HAND["depth9"], (np.arange(512) % 16).astype(np.uint8), HAND["k200"], np.zeros(0, np.uint8),
            np.full(1, 0x5A, np.uint8), HAND["depth13"]]
    exp = oracle_batch_limit(segs, 2, 64, 7)
    assert exp["mode"].tolist() == [1, 1, 0, 0, 1, 1] and not exp["lens"][2].any() and exp["lens"][4, 0x5A] == 1
    ref, _, _ = _encode(torch_cuda, codec, segs, max_bits=7)
    codec.set_option("batch_grid", grid)
    try:
        enc, x, off = _encode(torch_cuda, codec, segs, max_bits=7)
        assert codec.batch_status() == 0
        h = _host(enc)
        _check_encode(h, exp, ("grid", grid))
        assert np.array_equal(h["lens"], ref["lens"].cpu().numpy())
        _check_all_decodes(torch_cuda, codec, enc, segs, x, 64, ("grid", grid))
    finally:
        codec.set_option("batch_grid", 0)


def test_an_overlong_segment_and_a_decreasing_pair_fail_alone(torch_cuda, codec):
    torch = torch_cuda
    good = [HAND["depth13"], SEGMENTS[10], HAND["enwik4096"], SEGMENTS[9]]
    segs = good[:2] + [content("enwik", 65537, 1)] + good[2:]
    enc, x, off = _encode(torch, codec, segs, max_bits=12)
    assert codec.batch_status() == DC_E_ARG
    h = _host(enc)
    assert h["status"].tolist() == [0, 0, DC_E_ARG, 0, 0]
    exp = oracle_batch_limit(good[:2] + [np.zeros(0, np.uint8)] + good[2:], 2, 64, 12)
    _check_encode(h, exp, ("overlong",), skip=(2,))
    _check_decode(torch, codec, enc, segs, ("overlong",), bad={2: DC_E_ARG})
    # offsets 0, 8192, 4096, 12288: segment 1 runs backwards, segment 2 is x[4096:12288]
    x = np.concatenate([HAND["depth13"], HAND["enwik4096"]])
    offs = np.array([0, 8192, 4096, 12288], np.int64)
    # (the segments overlap, so they pass the bounds of x's size: buffers of their own)
    enc = codec.encode_batch(_dev(torch, x), _dev(torch, offs), max_bits=12,
                             payload=torch.full((16384 + 48,), FILL, dtype=torch.uint8, device="cuda"),
                             sync_len=torch.zeros(16384 // 64 + 3, dtype=torch.int16, device="cuda"))
    assert codec.batch_status() == DC_E_ARG
    h = _host(enc)
    assert h["status"].tolist() == [0, DC_E_ARG, 0]
    exp = oracle_batch_limit([x[:8192], np.zeros(0, np.uint8), x[4096:12288]], 2, 64, 12)
    for k in ("lens", "mode", "bits"):
        assert np.array_equal(h[k][[0, 2]], exp[k][[0, 2]]), k
    end = int(exp["pay_off"][-1])
    assert np.array_equal(h["pay_off"], exp["pay_off"]) and np.array_equal(h["payload"][:end], exp["payload"])
    assert np.array_equal(h["sync_off"], exp["sync_off"])


def test_payload_cap_inside_a_capped_segment(torch_cuda, codec):
    segs = [SEGMENTS[6], SEGMENTS[10], HAND["depth16"], SEGMENTS[7]]
    exp = oracle_batch_limit(segs, 2, 64, 12)
    k = 2
    assert exp["lens"][k].max() == 12   # the cap binds in segment k
    cap = int(exp["pay_off"][k]) + 16   # ends inside segment k
    assert cap < exp["pay_off"][k + 1]
    enc, x, off = _encode(torch_cuda, codec, segs, payload_cap=cap, max_bits=12)
    assert codec.batch_status() == DC_E_CAPACITY
    h = _host(enc)
    assert h["status"].tolist() == [0, 0, DC_E_CAPACITY, DC_E_CAPACITY]
    assert np.array_equal(h["payload"][: int(exp["pay_off"][k])], exp["payload"][: int(exp["pay_off"][k])])
    assert (h["payload"][int(exp["pay_off"][k]):] == FILL).all()   # nothing of segment k, nothing at or past the cap
    for name in ("lens", "mode", "bits", "pay_off", "sync_off"):
        assert np.array_equal(h[name], exp[name]), name


def test_invalid_caps_fail_from_the_host(torch_cuda, codec):
    torch = torch_cuda
    from data_compression_amd._lib import DcError
    x, off = pack_offsets(SEGMENTS[:4])
    xd, od = _dev(torch, x), _dev(torch, off)
    like = codec.encode_batch(xd, od)
    codec.timing(True)
    with pytest.raises(DcError) as e:
        codec.encode_batch(xd, od, max_bits=33)
    assert e.value.rc == DC_E_ARG
    with pytest.raises(ValueError):
        codec.encode_batch(xd, od, n_ary=16, max_bits=3)   # not one 4-bit digit
    like16 = dict(like, n_ary=16)
    assert _raw_limit(torch, codec, like16, xd, od, 9)[0] == DC_E_ARG    # 36 bits
    rc, enc = _raw_limit(torch, codec, like, xd, od, 129)                # over DC_MAX_DIGITS
    assert rc == DC_E_ARG and (enc["lens"] == FILL).all() and (enc["status"].view(torch.uint8) == FILL).all()
    assert codec.timings() == []   # nothing was launched
    codec.timing(False)
    with pytest.raises(ValueError):
        codec.encode_batch(xd, od, table=codec.batch_table(xd, max_bits=12), max_bits=12)
    with pytest.raises(ValueError):
        codec.encode_blocks(xd, block=4096, table=codec.batch_table(xd), max_bits=12)


def test_launches_do_not_depend_on_count(torch_cuda, codec):
    stages = {}
    for count in (1, 300):
        codec.timing(True)
        _encode(torch_cuda, codec, _small_segments(count), max_bits=12)
        stages[count] = [n for n, _ in codec.timings()]
        codec.timing(False)
    assert stages[1] == stages[300] and len(stages[1]) == 4   # plan, two scans, pack


def test_encode_blocks_takes_the_cap(torch_cuda, codec):
    x = HAND["enwik65536"]
    enc = codec.encode_blocks(_dev(torch_cuda, x), block=65536, max_bits=12)
    exp = oracle_batch_limit([x], 2, 64, 12)
    h = _host(enc)
    assert np.array_equal(h["lens"], exp["lens"]) and h["lens"].max() == 12
    out, _ = codec.decode_batch(enc)
    assert codec.batch_status() == 0 and np.array_equal(out.cpu().numpy(), x)


# ---- nybble records ----------------------------------------------------------------------------
def _pack(torch, codec, lens):
    """batch_lens_pack of a host count x 256 array: (lens4, status) on the host."""
    l4, st = codec.batch_lens_pack({"lens": _dev(torch, lens), "count": lens.shape[0]})
    return l4.cpu().numpy(), st.cpu().numpy()


def test_capped_records_pack_and_the_batch_decodes_from_them(torch_cuda, codec):
    torch = torch_cuda
    enc, x, off = _encode(torch, codec, CASES, max_bits=12)
    lens4, st = codec.batch_lens_pack(enc)
    assert codec.batch_status() == 0 and not st.cpu().numpy().any()
    assert lens4.shape == (len(CASES), 128) and lens4.dtype == torch.uint8
    lens = enc["lens"].cpu().numpy()
    assert np.array_equal(lens4.cpu().numpy(), lens_pack(lens)[0])
    back = codec.batch_lens_unpack(lens4)
    assert back.shape == (len(CASES), 256) and np.array_equal(back.cpu().numpy(), lens)
    stored = dict(enc, lens=back)
    _check_all_decodes(torch, codec, stored, CASES, x, 64, ("from nybbles",))


def test_an_uncapped_deep_record_does_not_pack_and_fails_safe(torch_cuda, codec):
    torch = torch_cuda
    segs = [SEGMENTS[10], HAND["enwik65536"], SEGMENTS[9]]
    enc, x, off = _encode(torch, codec, segs)
    assert int(enc["lens"][1].max()) == 16 and int(enc["mode"][1]) == 1
    lens4, st = codec.batch_lens_pack(enc)
    assert codec.batch_status() == DC_E_CODE_TOO_LONG and st.cpu().tolist() == [0, DC_E_CODE_TOO_LONG, 0]
    assert not lens4[1].any()
    stored = dict(enc, lens=codec.batch_lens_unpack(lens4))
    _check_decode(torch, codec, stored, segs, ("zero record",), bad={1: DC_E_STREAM})


@pytest.mark.parametrize("count,grid", [(0, 0), (1, 0), (3, 0), (257, 0), (257, 1)])
def test_record_counts(torch_cuda, codec, count, grid):
    torch = torch_cuda
    lens = np.random.default_rng(count).integers(0, 16, (count, 256)).astype(np.uint8)
    codec.set_option("batch_grid", grid)
    try:
        l4, st = _pack(torch, codec, lens)
        assert count == 0 or codec.batch_status() == 0   # (count 0 launches nothing: the slot is the call's before)
        assert l4.shape == (count, 128) and np.array_equal(l4, lens_pack(lens)[0]) and not st.any() and st.shape == (count,)
        room = torch.full((count * 128 + 64,), FILL, dtype=torch.uint8, device="cuda")   # nothing past the last record
        room[: count * 128] = _dev(torch, l4).view(-1)
        back = codec.batch_lens_unpack(room[: count * 128].view(count, 128))
        assert np.array_equal(back.cpu().numpy(), lens) and np.array_equal(back.cpu().numpy(), lens_unpack(l4))
    finally:
        codec.set_option("batch_grid", 0)


@pytest.mark.parametrize("at", (0, 1, 254, 255))
def test_a_length_of_16_fails_its_record_alone(torch_cuda, codec, at):
    torch = torch_cuda
    lens = np.random.default_rng(7).integers(0, 15, (40, 256)).astype(np.uint8)
    lens[:, at] = 15                        # a 15 there packs
    l4, st = _pack(torch, codec, lens)
    assert codec.batch_status() == 0 and not st.any() and np.array_equal(l4, lens_pack(lens)[0])
    for k in (5, 17, 18, 39):               # records of different waves and lane groups
        lens[k, at] = 16
    exp4, exps = lens_pack(lens)
    l4, st = _pack(torch, codec, lens)
    assert codec.batch_status() == DC_E_CODE_TOO_LONG   # the first failure, record 5
    assert np.array_equal(st, exps) and np.flatnonzero(st).tolist() == [5, 17, 18, 39]
    assert np.array_equal(l4, exp4) and not l4[5].any() and l4[4].any() and l4[6].any() and l4[16].any() and l4[19].any()


def test_the_first_failure_is_the_lowest_index(torch_cuda, codec):
    lens = np.zeros((600, 256), np.uint8)
    lens[[599, 301, 77], 128] = 200
    _, st = _pack(torch_cuda, codec, lens)
    assert np.flatnonzero(st).tolist() == [77, 301, 599]
    assert codec.batch_status() == DC_E_CODE_TOO_LONG


def test_host_rules(torch_cuda, codec):
    torch = torch_cuda
    L, ctx = codec.L, codec.ctx
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    codec.timing(True)
    assert L.dc_huff_batch_lens_pack(ctx, None, 0, None, None) == 0        # count 0: no launch
    assert L.dc_huff_batch_lens_unpack(ctx, None, 0, None) == 0
    assert L.dc_huff_batch_lens_pack(ctx, None, 2, p, st.data_ptr()) == DC_E_ARG
    assert L.dc_huff_batch_lens_pack(ctx, p, 2, None, st.data_ptr()) == DC_E_ARG
    assert L.dc_huff_batch_lens_pack(ctx, p, 2, p + 1024, None) == DC_E_ARG
    assert L.dc_huff_batch_lens_unpack(ctx, None, 2, p) == DC_E_ARG
    assert L.dc_huff_batch_lens_unpack(ctx, p, 2, None) == DC_E_ARG
    assert L.dc_huff_batch_lens_pack(ctx, p, (1 << 28) + 1, p + (1 << 40), st.data_ptr()) == DC_E_ARG   # DC_RANGES_MAX
    # overlap: 2 records are 512 B of lens and 256 B of lens4
    assert L.dc_huff_batch_lens_pack(ctx, p, 2, p + 256, st.data_ptr()) == DC_E_ARG
    assert L.dc_huff_batch_lens_pack(ctx, p + 256, 2, p + 8, st.data_ptr()) == DC_E_ARG
    assert L.dc_huff_batch_lens_unpack(ctx, p, 2, p + 240) == DC_E_ARG
    assert L.dc_huff_batch_lens_unpack(ctx, p, 2, p) == DC_E_ARG
    assert L.dc_huff_batch_lens_pack(ctx, p + 4, 2, p + 1024, st.data_ptr()) == DC_E_ARG   # lens not 16-B aligned
    assert codec.timings() == []
    codec.timing(True)
    buf[:512] = 3
    assert L.dc_huff_batch_lens_pack(ctx, p, 2, p + 512, st.data_ptr()) == 0   # adjacent is not overlapping
    assert L.dc_huff_batch_lens_unpack(ctx, p + 512, 2, p + 1024) == 0
    assert [n for n, _ in codec.timings()] == ["hb_lens_pack", "hb_lens_unpack"]   # one launch each
    codec.timing(False)
    h = buf.cpu().numpy()
    assert (h[512:768] == 0x33).all() and (h[768:1024] == FILL).all() and (h[1024:1536] == 3).all() and (h[1536:] == FILL).all()
    with pytest.raises(ValueError):
        codec.batch_lens_pack(dict(codec.encode_batch(buf[:512], [0, 512], table=codec.batch_table(buf[:512]))))
