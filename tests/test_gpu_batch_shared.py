"""The shared-table mode of the batched Huffman codec on the device: dc_huff_encode_batch_shared /
dc_huff_decode_batch_shared (k_hbs_plan, k_hbs_pack, k_hbs_decode) through
Codec.encode_batch(..., table=) / decode_batch. The reference is the CPU oracle's batch under one
table (tests/test_batch_shared_cpu.py: oracle_shared_batch) for the encode and the input segments
for the decode; every byte nobody asked for must keep its 0xA5 prefill."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_batch_cpu import SEGMENTS, content, pack_offsets
from tests.test_batch_shared_cpu import oracle_shared_batch, oracle_text_batch, table_codes, text_table
from tests.test_gpu_batch import _dev, _gapped, _small_segments

pytestmark = pytest.mark.gpu

FILL = 0xA5
DC_E_ARG, DC_E_CODE_TOO_LONG, DC_E_CAPACITY, DC_E_STREAM = -1, -3, -6, -7
ARRAYS = ("mode", "bits", "pay_off", "sync_off")


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


@pytest.fixture(scope="module")
def text_tab(torch_cuda, codec):
    """The text table at n = 2 on the device, built from its lengths."""
    return codec.table_lengths(_dev(torch_cuda, text_table(2)), 2)


def _encode(torch, codec, segs, tab, n_ary=2, S=64, x_dev=None, **kw):
    """encode_batch under `tab` into 0xA5-filled payload and sync buffers: (enc, x, offsets)."""
    x, off = pack_offsets(segs)
    pb, sb = codec.batch_bounds(x.size, len(segs), S)
    payload = torch.full((pb + 48,), FILL, dtype=torch.uint8, device="cuda")
    sync = torch.full((sb + 5,), -23131, dtype=torch.int16, device="cuda")   # 0xA5A5
    enc = codec.encode_batch(_dev(torch, x) if x_dev is None else x_dev, _dev(torch, off), n_ary=n_ary, sync_syms=S,
                             payload=payload, sync_len=sync, table=tab, **kw)
    assert enc["table"] is tab and enc["lens"] is None
    return enc, x, off


def _host(enc):
    h = {k: enc[k].cpu().numpy() for k in ARRAYS + ("payload", "status")}
    h["sync_len"] = enc["sync_len"].cpu().numpy().view(np.uint16)
    return h


def _check_encode(h, exp, tag, skip=()):
    """Every array equals the oracle's, pads included; segments in `skip` wrote no mode / bits."""
    keep = np.array([i not in skip for i in range(len(exp["mode"]))], bool)
    for k in ("mode", "bits"):
        assert np.array_equal(h[k][keep], exp[k][keep]), tag + (k,)
    for k in ("pay_off", "sync_off"):
        assert np.array_equal(h[k], exp[k]), tag + (k,)
    end = int(exp["pay_off"][-1])
    assert np.array_equal(h["payload"][:end], exp["payload"]), tag + ("payload, pads included",)
    assert (h["payload"][end:] == FILL).all(), tag + ("payload past pay_off[count] written",)
    send = int(exp["sync_off"][-1])
    assert np.array_equal(h["sync_len"][:send], exp["sync_len"]), tag + ("sync_len",)
    assert (h["sync_len"][send:] == 0xA5A5).all(), tag + ("sync_len past sync_off[count] written",)


def _check_decode(torch, codec, enc, segs, tag, bad=None, cap=None):
    """ONE scatter decode into a 0xA5 buffer (of `cap` bytes) at gapped, odd offsets: every segment
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
            assert st[i] == bad[i], tag + (i, "status", int(st[i]))
            continue
        assert st[i] == 0, tag + (i, int(st[i]))
        assert np.array_equal(h[o: o + s.size], s), tag + (i, "decoded bytes")
        asked[o: o + s.size] = True
    assert (h[~asked] == FILL).all(), tag + ("bytes outside the good segments written",)
    assert codec.batch_status() == (bad[min(bad)] if bad else 0), tag + ("batch_status",)


@pytest.mark.parametrize("n_ary,S", [(2, 64), (3, 64), (16, 64), (17, 64), (2, 16), (2, 1024), (256, 64)])
def test_encode_is_bit_exact_and_round_trips(torch_cuda, codec, n_ary, S):
    tab = codec.table_lengths(_dev(torch_cuda, text_table(n_ary)), n_ary)
    enc, x, off = _encode(torch_cuda, codec, SEGMENTS, tab, n_ary, S)
    assert codec.batch_status() == 0
    h = _host(enc)
    assert (h["status"] == 0).all()
    _check_encode(h, oracle_text_batch(n_ary, S), (n_ary, S))
    _check_decode(torch_cuda, codec, enc, SEGMENTS, (n_ary, S))


def test_contiguous_decode_is_the_default(torch_cuda, codec, text_tab):
    enc, x, off = _encode(torch_cuda, codec, SEGMENTS, text_tab)
    out, out_off = codec.decode_batch(enc)
    assert codec.batch_status() == 0
    assert np.array_equal(out.cpu().numpy(), x) and np.array_equal(out_off.cpu().numpy(), off)


@pytest.mark.parametrize("shift", (0, 1))
def test_table_from_the_histogram_of_the_batch(torch_cuda, codec, shift):
    """batch_table of the whole input; shift 1: an input that is not 16-B aligned (cloned for the
    histogram, coded where it lies)."""
    torch = torch_cuda
    x, _ = pack_offsets(SEGMENTS)
    buf = torch.zeros(x.size + 16, dtype=torch.uint8, device="cuda")
    xd = buf[shift: shift + x.size]
    xd.copy_(_dev(torch, x))
    assert xd.data_ptr() % 16 == shift
    tab = codec.batch_table(xd)
    L = orc.huffman_lengths(orc.histogram(x), 2)
    assert np.array_equal(codec.table_get_lengths(tab), L)
    enc, _, _ = _encode(torch, codec, SEGMENTS, tab, x_dev=xd)
    assert codec.batch_status() == 0
    exp = oracle_shared_batch(SEGMENTS, *table_codes(L, 2), 64)
    assert set(exp["mode"].tolist()) == {0, 1}
    _check_encode(_host(enc), exp, ("batch_table", shift))
    _check_decode(torch, codec, enc, SEGMENTS, ("batch_table", shift))


def test_segments_decode_with_the_single_stream_decoder(torch_cuda, codec):
    """16-B aligned payloads under one table: a coded segment is a stream of the existing decoder."""
    torch = torch_cuda
    tab = codec.table_lengths(_dev(torch, text_table(2)), 2)   # (its own: codec.decode builds its decoder tables)
    enc, x, off = _encode(torch, codec, SEGMENTS, tab)
    h = _host(enc)
    picks = [i for i, s in enumerate(SEGMENTS) if h["mode"][i] == 1 and s.size >= 4097 and len(np.unique(s)) > 1][:3]
    assert len(picks) == 3
    for i in picks:
        n = SEGMENTS[i].size
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


def test_table_persists_by_its_lengths_and_is_not_written(torch_cuda):
    """Encode under table(hist) on one Codec; a second Codec rebuilds the table from
    table_get_lengths and decodes. The first table's bytes are the same before and after."""
    torch = torch_cuda
    from data_compression_amd.device import Codec
    a, b = Codec(0), Codec(0)
    segs = [SEGMENTS[10], SEGMENTS[6], SEGMENTS[9], SEGMENTS[11], SEGMENTS[0]]
    x, _ = pack_offsets(segs)
    tab = a.table(a.hist(_dev(torch, x)), 2)
    before = tab.clone()
    enc, _, _ = _encode(torch, a, segs, tab)
    assert a.batch_status() == 0 and int(enc["mode"].sum()) >= 2
    _check_decode(torch, a, enc, segs, ("first codec",))
    assert torch.equal(tab, before), "the shared table was written by the batch kernels"
    L = a.table_get_lengths(tab)
    assert L.dtype == np.int32 and np.array_equal(L, orc.huffman_lengths(orc.histogram(x), 2))
    enc2 = dict(enc, table=b.table_lengths(_dev(torch, L), 2), status=torch.full_like(enc["status"], -99))
    _check_decode(torch, b, enc2, segs, ("second codec",))
    a.close()
    b.close()


@pytest.mark.parametrize("count,grid", [(1, 0), (5, 0), (300, 0), (300, 7)])
def test_counts(torch_cuda, codec, text_tab, count, grid):
    """300 segments on a grid of 7 workgroups: each walks 42 or 43 segments under the one copy of
    the table it made before its loop."""
    segs = _small_segments(count)
    exp = oracle_shared_batch(segs, *table_codes(text_table(2), 2), 64)
    if count >= 5:
        assert set(exp["mode"].tolist()) == {0, 1}
    codec.set_option("batch_grid", grid)
    try:
        enc, x, off = _encode(torch_cuda, codec, segs, text_tab)
        assert codec.batch_status() == 0
        _check_encode(_host(enc), exp, (count, grid))
        _check_decode(torch_cuda, codec, enc, segs, (count, grid))
    finally:
        codec.set_option("batch_grid", 0)


@pytest.mark.parametrize("S", (64, 16))
def test_decode_paths_meet_at_8_kib(torch_cuda, codec, text_tab, S):
    """The decoder deals segments four at a time: four of at most 8192 bytes to its four waves, a
    group with a longer one to the whole workgroup. Groups on both sides of that size, coded and
    stored, and a last group of two."""
    lens = (8192, 8191, 8192, 100,   8193, 8192, 700, 8192,   8192, 1, 8190, 8192,   300, 8193)
    kinds = ("enwik", "enwik", "cycle", "zipf")
    segs = [content(kinds[j % 4], n, 70 + j) for j, n in enumerate(lens)]
    exp = oracle_shared_batch(segs, *table_codes(text_table(2), 2), S)
    assert set(exp["mode"].tolist()) == {0, 1}
    enc, x, off = _encode(torch_cuda, codec, segs, text_tab, S=S)
    assert codec.batch_status() == 0
    _check_encode(_host(enc), exp, ("8 KiB", S))
    _check_decode(torch_cuda, codec, enc, segs, ("8 KiB", S))


def test_launches_do_not_depend_on_count(torch_cuda, codec, text_tab):
    stages = {}
    for count in (1, 300):
        segs = _small_segments(count)
        codec.timing(True)
        enc, _, _ = _encode(torch_cuda, codec, segs, text_tab)
        ne = [n for n, _ in codec.timings()]
        codec.timing(True)
        codec.decode_batch(enc)
        nd = [n for n, _ in codec.timings()]
        codec.timing(False)
        stages[count] = (ne, nd)
    assert stages[1] == stages[300]
    assert len(stages[1][0]) == 4 and len(stages[1][1]) == 1   # plan, two scans, pack; one decode


def test_a_table_with_overlong_codes_is_usable(torch_cuda, codec):
    torch = torch_cuda
    L = np.zeros(259, np.int32)
    L[[0x41, 0x42, 0x43, 0x44]] = (1, 2, 33, 33)
    tab = codec.table_lengths(_dev(torch, L), 2)
    assert codec.table_status(tab)[0] == DC_E_CODE_TOO_LONG
    code, nb = table_codes(L, 2)
    assert nb[0x41: 0x45].tolist() == [1, 2, 0, 0]
    segs = [np.frombuffer(b"ABABAABA" * 10, np.uint8), np.frombuffer(b"ABCA" * 10, np.uint8)]
    enc, _, _ = _encode(torch, codec, segs, tab)
    assert codec.batch_status() == 0
    h = _host(enc)
    assert h["mode"].tolist() == [1, 0] and h["bits"].tolist() == [110, 320]
    _check_encode(h, oracle_shared_batch(segs, code, nb, 64), ("overlong codes",))
    _check_decode(torch, codec, enc, segs, ("overlong codes",))


def test_a_table_of_another_arity_is_refused(torch_cuda, codec, text_tab):
    """The batch says n = 3, the table is n = 2: DC_E_ARG for every segment, nothing written."""
    torch = torch_cuda
    segs = [SEGMENTS[6], SEGMENTS[10], SEGMENTS[0], SEGMENTS[9]]
    enc, _, _ = _encode(torch, codec, segs, text_tab, n_ary=3)
    assert codec.batch_status() == DC_E_ARG
    assert enc["status"].cpu().tolist() == [DC_E_ARG] * len(segs)
    assert (enc["payload"] == FILL).all() and (enc["sync_len"].view(torch.uint8) == FILL).all()
    good, _, _ = _encode(torch, codec, segs, text_tab)
    assert codec.batch_status() == 0
    _check_decode(torch, codec, dict(good, n_ary=3), segs, ("decode",), bad={i: DC_E_ARG for i in range(len(segs))})
    _check_decode(torch, codec, good, segs, ("decode, the table's arity",))


def test_an_overlong_segment_fails_alone(torch_cuda, codec, text_tab):
    good = [SEGMENTS[6], SEGMENTS[10], SEGMENTS[5], SEGMENTS[9]]
    segs = good[:2] + [content("enwik", 65537, 1)] + good[2:]
    enc, x, off = _encode(torch_cuda, codec, segs, text_tab)
    assert codec.batch_status() == DC_E_ARG
    h = _host(enc)
    assert h["status"].tolist() == [0, 0, DC_E_ARG, 0, 0]
    # 0 payload bytes, 0 sync entries
    exp = oracle_shared_batch(good[:2] + [np.zeros(0, np.uint8)] + good[2:], *table_codes(text_table(2), 2), 64)
    _check_encode(h, exp, ("overlong",), skip=(2,))
    _check_decode(torch_cuda, codec, enc, segs, ("overlong",), bad={2: DC_E_ARG})


@pytest.mark.parametrize("which", ("payload_cap", "sync_cap"))
def test_a_cap_inside_a_segment(torch_cuda, codec, text_tab, which):
    segs = [SEGMENTS[6], SEGMENTS[10], SEGMENTS[9], SEGMENTS[7]]
    exp = oracle_shared_batch(segs, *table_codes(text_table(2), 2), 64)
    k = 2
    pcut, scut = int(exp["pay_off"][k]), int(exp["sync_off"][k])
    cap = pcut + 16 if which == "payload_cap" else scut + 1   # ends inside segment k
    assert cap < (exp["pay_off"] if which == "payload_cap" else exp["sync_off"])[k + 1]
    enc, x, off = _encode(torch_cuda, codec, segs, text_tab, **{which: cap})
    assert codec.batch_status() == DC_E_CAPACITY
    h = _host(enc)
    assert h["status"].tolist() == [0, 0, DC_E_CAPACITY, DC_E_CAPACITY]
    assert np.array_equal(h["payload"][:pcut], exp["payload"][:pcut])
    assert (h["payload"][pcut:] == FILL).all()      # nothing of segment k, nothing at or past the cap
    assert np.array_equal(h["sync_len"][:scut], exp["sync_len"][:scut])
    assert (h["sync_len"][scut:] == 0xA5A5).all()
    for name in ARRAYS:
        assert np.array_equal(h[name], exp[name]), name
    _check_decode(torch_cuda, codec, enc, segs, (which,), bad={2: DC_E_STREAM, 3: DC_E_STREAM})


def test_out_cap_inside_a_segment(torch_cuda, codec, text_tab):
    segs = [SEGMENTS[6], SEGMENTS[10], SEGMENTS[9], SEGMENTS[7]]
    enc, x, off = _encode(torch_cuda, codec, segs, text_tab)
    starts, _ = _gapped(segs)
    cap = int(starts[2]) + 100   # ends inside segment 2's output
    _check_decode(torch_cuda, codec, enc, segs, ("out_cap",), bad={2: DC_E_CAPACITY, 3: DC_E_CAPACITY}, cap=cap)


@pytest.mark.parametrize("last", (6, 11))   # a group of four short segments (one a wave), or one with a long segment
@pytest.mark.parametrize("what", ("mode", "bits", "sync_len"))
def test_a_corrupt_segment_fails_alone(torch_cuda, codec, text_tab, what, last):
    torch = torch_cuda
    segs = [SEGMENTS[8], SEGMENTS[10], SEGMENTS[9], SEGMENTS[last]]
    enc, x, off = _encode(torch, codec, segs, text_tab)
    k = 1
    assert int(enc["mode"][k]) == 1
    enc = dict(enc)
    enc[what] = enc[what].clone()
    if what == "mode":
        enc["mode"][k] = 2
    elif what == "bits":
        enc["bits"][k] += 1
    else:   # the sum is kept: only the per-chunk exactness check can see it
        at = int(enc["sync_off"][k]) + 3
        enc["sync_len"][at] += 1
        enc["sync_len"][at + 1] -= 1
    _check_decode(torch, codec, enc, segs, (what,), bad={k: DC_E_STREAM})


def test_count_zero_is_ok(torch_cuda, codec, text_tab):
    torch = torch_cuda
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    codec.timing(True)
    enc = codec.encode_batch(empty, torch.zeros(1, dtype=torch.int64, device="cuda"), table=text_tab)
    assert enc["count"] == 0 and enc["table"] is text_tab
    out, _ = codec.decode_batch(enc)
    assert out.numel() == 0
    assert codec.timings() == []   # no launch
    codec.timing(False)
    assert codec.encode_blocks(empty, table=text_tab)["count"] == 0
