"""The batched Huffman codec on the device: dc_huff_encode_batch / dc_huff_decode_batch
(k_hb_plan, k_hb_pack, k_hb_decode) through Codec.encode_batch / decode_batch. The reference is
the CPU oracle's batch (tests/test_batch_cpu.py: oracle_batch) for the encode and the input
segments for the decode; every byte nobody asked for must keep its 0xA5 prefill."""
import numpy as np
import pytest

from tests.test_batch_cpu import SEGMENTS, oracle_batch, pack_offsets

pytestmark = pytest.mark.gpu

FILL = 0xA5
DC_E_ARG, DC_E_CAPACITY, DC_E_STREAM = -1, -6, -7
ARRAYS = ("lens", "mode", "bits", "pay_off", "sync_off")


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


def _encode(torch, codec, segs, n_ary=2, S=64, **kw):
    """encode_batch into 0xA5-filled payload and sync buffers: (enc, x, offsets)."""
    x, off = pack_offsets(segs)
    pb, sb = codec.batch_bounds(x.size, len(segs), S)
    payload = torch.full((pb + 48,), FILL, dtype=torch.uint8, device="cuda")
    sync = torch.full((sb + 5,), -23131, dtype=torch.int16, device="cuda")   # 0xA5A5
    enc = codec.encode_batch(_dev(torch, x), _dev(torch, off), n_ary=n_ary, sync_syms=S, payload=payload,
                             sync_len=sync, **kw)
    return enc, x, off


def _host(enc):
    h = {k: enc[k].cpu().numpy() for k in ARRAYS + ("payload", "status")}
    h["sync_len"] = enc["sync_len"].cpu().numpy().view(np.uint16)
    return h


def _check_encode(h, exp, tag, skip=()):
    """Every array equals the oracle's; segments in `skip` wrote no lens / mode / bits."""
    keep = np.array([i not in skip for i in range(len(exp["mode"]))], bool)
    for k in ("lens", "mode", "bits"):
        assert np.array_equal(h[k][keep], exp[k][keep]), tag + (k,)
    for k in ("pay_off", "sync_off"):
        assert np.array_equal(h[k], exp[k]), tag + (k,)
    end = int(exp["pay_off"][-1])
    assert np.array_equal(h["payload"][:end], exp["payload"]), tag + ("payload, pads included",)
    assert (h["payload"][end:] == FILL).all(), tag + ("payload past pay_off[count] written",)
    send = int(exp["sync_off"][-1])
    assert np.array_equal(h["sync_len"][:send], exp["sync_len"]), tag + ("sync_len",)
    assert (h["sync_len"][send:] == 0xA5A5).all(), tag + ("sync_len past sync_off[count] written",)


def _gapped(segs, lead=3, gap=5):
    """Odd, gapped output starts; returns (starts, capacity)."""
    at, starts = lead, []
    for s in segs:
        starts.append(at)
        at += s.size + gap + (at + s.size + gap) % 2   # keeps most starts odd
    return np.array(starts, np.int64), at + 31


def _check_decode(torch, codec, enc, segs, tag, bad=None, cap=None):
    """ONE decode_batch into a 0xA5 buffer (of `cap` bytes) at gapped, odd offsets: every segment
    not in `bad` (index -> expected status) equals its input, every other byte is untouched."""
    bad = bad or {}
    starts, full = _gapped(segs)
    cap = full if cap is None else cap
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    codec.decode_batch(enc, out=out, out_off=starts)
    st = enc["status"].cpu().numpy()
    h = out.cpu().numpy()
    asked = np.zeros(cap, bool)
    for i, (s, o) in enumerate(zip(segs, starts)):
        if i in bad:
            assert st[i] == bad[i], tag + (i, "status")
            continue
        assert st[i] == 0, tag + (i, int(st[i]))
        assert np.array_equal(h[o: o + s.size], s), tag + (i, "decoded bytes")
        asked[o: o + s.size] = True
    assert (h[~asked] == FILL).all(), tag + ("bytes outside the good segments written",)
    first = min(bad) if bad else None
    assert codec.batch_status() == (bad[first] if bad else 0), tag + ("batch_status",)


@pytest.mark.parametrize("n_ary,S", [(2, 64), (3, 64), (16, 64), (17, 64), (2, 16), (2, 1024)])
def test_encode_is_bit_exact_and_round_trips(torch_cuda, codec, n_ary, S):
    enc, x, off = _encode(torch_cuda, codec, SEGMENTS, n_ary, S)
    assert codec.batch_status() == 0
    h = _host(enc)
    assert (h["status"] == 0).all()
    exp = oracle_batch(SEGMENTS, n_ary, S)
    assert set(exp["mode"].tolist()) == {0, 1}   # both paths are in the batch
    _check_encode(h, exp, (n_ary, S))
    _check_decode(torch_cuda, codec, enc, SEGMENTS, (n_ary, S))


def test_contiguous_decode_is_the_default(torch_cuda, codec):
    enc, x, off = _encode(torch_cuda, codec, SEGMENTS)
    out, out_off = codec.decode_batch(enc)
    assert codec.batch_status() == 0
    assert np.array_equal(out.cpu().numpy(), x) and np.array_equal(out_off.cpu().numpy(), off)


def test_segments_decode_with_the_single_stream_decoder(torch_cuda, codec):
    """16-B aligned payloads: a Huffman-mode segment is a stream of the existing decoder."""
    torch = torch_cuda
    enc, x, off = _encode(torch, codec, SEGMENTS)
    h = _host(enc)
    picks = [i for i, s in enumerate(SEGMENTS) if h["mode"][i] == 1 and s.size >= 4097 and len(np.unique(s)) > 1][:3]
    assert len(picks) == 3
    for i in picks:
        n = SEGMENTS[i].size
        L = np.zeros(259, np.int32)
        L[:256] = h["lens"][i]
        tab = codec.table_lengths(_dev(torch, L), 2)
        sl = h["sync_len"][h["sync_off"][i]: h["sync_off"][i + 1]]
        base = np.concatenate(([0], np.cumsum(sl.astype(np.int64))))[:-1][::64].copy()
        nbytes = int(h["pay_off"][i + 1] - h["pay_off"][i])
        words = torch.zeros(nbytes // 4 + 64, dtype=torch.int32, device="cuda")   # the decoder's read-ahead slack
        words.view(torch.uint8)[:nbytes] = enc["payload"][int(h["pay_off"][i]): int(h["pay_off"][i + 1])]
        lens16 = torch.zeros(sl.size + 2, dtype=torch.int16, device="cuda")
        lens16[: sl.size] = _dev(torch, sl.view(np.int16))
        out = torch.full((n + 64,), FILL, dtype=torch.uint8, device="cuda")
        codec.decode(words, 0, (_dev(torch, base), lens16[: sl.size]), 64, n, tab, out)
        assert codec.decode_status() == 0, i
        assert np.array_equal(out.cpu().numpy()[:n], SEGMENTS[i]), i


def _small_segments(count):
    rng = np.random.default_rng(9)
    from tests.test_batch_cpu import content, KINDS
    return [content(KINDS[j % 4], int(rng.integers(100, 701)), 40 + j) for j in range(count)]


@pytest.mark.parametrize("count,grid", [(1, 0), (300, 0), (300, 7)])
def test_counts(torch_cuda, codec, count, grid):
    """300 segments: more workgroups than the device has CUs; on a grid of 7 workgroups every
    one of them walks 42 or 43 segments (the persistent loop and its uneven tail)."""
    segs = _small_segments(count)
    codec.set_option("batch_grid", grid)
    try:
        enc, x, off = _encode(torch_cuda, codec, segs)
        assert codec.batch_status() == 0
        _check_encode(_host(enc), oracle_batch(segs, 2, 64), (count, grid))
        _check_decode(torch_cuda, codec, enc, segs, (count, grid))
    finally:
        codec.set_option("batch_grid", 0)


def test_count_zero_is_ok(torch_cuda, codec):
    torch = torch_cuda
    enc = codec.encode_batch(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert enc["count"] == 0
    out, _ = codec.decode_batch(enc)
    assert out.numel() == 0
    empty = codec.encode_blocks(torch.zeros(0, dtype=torch.uint8, device="cuda"))
    assert empty["count"] == 0


def test_launches_do_not_depend_on_count(torch_cuda, codec):
    stages = {}
    for count in (1, 300):
        segs = _small_segments(count)
        codec.timing(True)
        enc, _, _ = _encode(torch_cuda, codec, segs)
        ne = [n for n, _ in codec.timings()]
        codec.timing(True)
        codec.decode_batch(enc)
        nd = [n for n, _ in codec.timings()]
        codec.timing(False)
        stages[count] = (ne, nd)
    assert stages[1] == stages[300]
    assert len(stages[1][0]) >= 1 and len(stages[1][1]) >= 1


def test_encode_blocks_cuts_independent_blocks(torch_cuda, codec):
    from data_compression_amd import synth
    x = synth.enwik_like(3 * 4096 + 77, seed=2)
    enc = codec.encode_blocks(_dev(torch_cuda, x), block=4096)
    assert enc["count"] == 4 and enc["offsets"].cpu().tolist() == [0, 4096, 8192, 12288, 12365]
    exp = oracle_batch([x[0:4096], x[4096:8192], x[8192:12288], x[12288:]], 2, 64)
    h = _host(enc)
    end = int(exp["pay_off"][-1])
    assert np.array_equal(h["pay_off"], exp["pay_off"]) and np.array_equal(h["payload"][:end], exp["payload"])
    out, _ = codec.decode_batch(enc)
    assert codec.batch_status() == 0 and np.array_equal(out.cpu().numpy(), x)


def test_an_overlong_segment_fails_alone(torch_cuda, codec):
    from tests.test_batch_cpu import content
    good = [SEGMENTS[6], SEGMENTS[10], SEGMENTS[5], SEGMENTS[9]]
    segs = good[:2] + [content("enwik", 65537, 1)] + good[2:]
    enc, x, off = _encode(torch_cuda, codec, segs)
    assert codec.batch_status() == DC_E_ARG
    h = _host(enc)
    assert h["status"].tolist() == [0, 0, DC_E_ARG, 0, 0]
    exp = oracle_batch(good[:2] + [np.zeros(0, np.uint8)] + good[2:], 2, 64)   # 0 payload bytes, 0 sync entries
    _check_encode(h, exp, ("overlong",), skip=(2,))
    _check_decode(torch_cuda, codec, enc, segs, ("overlong",), bad={2: DC_E_ARG})


def test_payload_cap_inside_a_segment(torch_cuda, codec):
    segs = [SEGMENTS[6], SEGMENTS[10], SEGMENTS[9], SEGMENTS[7]]
    exp = oracle_batch(segs, 2, 64)
    k = 2
    cap = int(exp["pay_off"][k]) + 16   # ends inside segment k
    assert cap < exp["pay_off"][k + 1]
    enc, x, off = _encode(torch_cuda, codec, segs, payload_cap=cap)
    assert codec.batch_status() == DC_E_CAPACITY
    h = _host(enc)
    assert h["status"].tolist() == [0, 0, DC_E_CAPACITY, DC_E_CAPACITY]
    assert np.array_equal(h["payload"][: int(exp["pay_off"][k])], exp["payload"][: int(exp["pay_off"][k])])
    assert (h["payload"][int(exp["pay_off"][k]):] == FILL).all()   # nothing of segment k, nothing at or past the cap
    for name in ("lens", "mode", "bits", "pay_off", "sync_off"):
        assert np.array_equal(h[name], exp[name]), name
    _check_decode(torch_cuda, codec, enc, segs, ("cap",), bad={2: DC_E_STREAM, 3: DC_E_STREAM})


def _corrupt_lens(enc, seg, k, length):
    """A copy of enc in which segment k's most frequent symbol has `length` digits."""
    sym = int(np.bincount(seg, minlength=256).argmax())
    assert int(enc["mode"][k]) == 1 and int(enc["lens"][k, sym]) > 0
    enc = dict(enc, lens=enc["lens"].clone())
    enc["lens"][k, sym] = length
    return enc


# lens: a present symbol loses its code; 200: a length over DC_MAX_DIGITS, 33: a code over 32 bits
# (n = 2), the two records the canonical build itself rejects
@pytest.mark.parametrize("what", ("lens", "lens_200", "lens_33", "sync_len", "mode"))
def test_a_corrupt_segment_fails_alone(torch_cuda, codec, what):
    torch = torch_cuda
    segs = [SEGMENTS[8], SEGMENTS[10], SEGMENTS[9], SEGMENTS[6]]
    enc, x, off = _encode(torch, codec, segs)
    k = 1
    assert int(enc["mode"][k]) == 1
    if what.startswith("lens"):
        enc = _corrupt_lens(enc, segs[k], k, {"lens": 0, "lens_200": 200, "lens_33": 33}[what])
    else:
        enc = dict(enc)
        enc[what] = enc[what].clone()
        if what == "sync_len":
            enc["sync_len"][int(enc["sync_off"][k]) + 3] += 1
        else:
            enc["mode"][k] = 7
    _check_decode(torch, codec, enc, segs, (what,), bad={k: DC_E_STREAM})


def test_a_bad_output_range_is_reported_before_a_bad_lens_record(torch_cuda, codec):
    """A segment whose output ends past out_cap AND whose lens record the canonical build rejects
    is DC_E_CAPACITY: the range is validated before the record is read."""
    torch = torch_cuda
    segs = [SEGMENTS[8], SEGMENTS[10], SEGMENTS[9], SEGMENTS[6]]
    enc, x, off = _encode(torch, codec, segs)
    k = 3
    enc = _corrupt_lens(enc, segs[k], k, 200)
    starts, _ = _gapped(segs)
    cap = int(starts[k]) + 100   # ends inside segment k's output
    assert cap < starts[k] + segs[k].size
    _check_decode(torch, codec, enc, segs, ("precedence",), bad={k: DC_E_CAPACITY}, cap=cap)
