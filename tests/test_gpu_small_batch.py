"""The batched small front-end on the device: dc_small_compress_batch (k_small_batch_len,
k_scan_u64, k_small_batch_enc) and dc_small_decompress_batch (k_small_batch_dec) through
Codec.small_compress_batch / small_compress_blocks / small_decompress_batch_into. The reference is
the CPU oracle's stream of every buffer alone (tests/test_small_batch_cpu.py: oracle_streams) for
the encode and orc.small_decompress for the decode; every byte nobody asked for must keep its 0xA5
prefill, and so must the whole range of a stream that fails.

One buffer of SMALL_INPUTS (I_HIGH) holds bytes >= 0x80 after byte 0, which the reference codec
does not round-trip (a raw byte with bit 7 set reads back as a pair): its stream decodes to more
bytes than went in, so asked at its input length it is DC_E_STREAM."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.stream_batch_checks import DC_E_ARG, DC_E_CAPACITY, DC_E_STREAM, FILL, _check_streams, _cum, _dev, pack_offsets
from tests.test_small_batch_cpu import I_HIGH, I_HIGH_FIRST, I_RANDOM_100, LITERAL, PRUNED, SMALL_INPUTS, oracle_streams

pytestmark = pytest.mark.gpu

WAVES = 4   # SB_WAVES: buffers a workgroup takes per round


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


def _encode(torch, codec, x, off, out_cap=None):
    """small_compress_batch into a 0xA5-filled buffer of bound + 48 bytes: host (out, out_off, status)."""
    count = len(off) - 1
    out = torch.full((codec.small_batch_bound(x.size, count) + 48,), FILL, dtype=torch.uint8, device="cuda")
    o, oo, st = codec.small_compress_batch(_dev(torch, x), _dev(torch, off), out=out, out_cap=out_cap)
    assert o is out
    return out.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()


@pytest.fixture(scope="module")
def encoded(torch_cuda, codec):
    """SMALL_INPUTS through the batch encode once: host (out, out_off, status), the batch status
    right after the call, and the packed input. Do not modify."""
    x, off = pack_offsets(SMALL_INPUTS)
    h = _encode(torch_cuda, codec, x, off)
    return h + (codec.batch_status(),), x, off


# ---- 1. the list in one call ---------------------------------------------------------------
def test_encode_is_the_oracle_stream_of_every_buffer(encoded):
    (h, oo, st, bstat), x, off = encoded
    want = oracle_streams(SMALL_INPUTS)
    assert {s[0] for s in want} == {PRUNED, LITERAL}   # both forms are in the batch
    assert bstat == 0 and (st == 0).all()
    _check_streams(h, oo, st, want, ())
    assert (h[oo[-1]:] == FILL).all() and h.size - oo[-1] >= 48


def test_same_streams_as_the_single_call(torch_cuda, codec, encoded):
    (h, oo, _, _), x, off = encoded
    sample = [1, 2, 5, 8, 9, 13, 33, 79, 80, 83, 85, 88, 93, I_RANDOM_100, 95, 101, 102, I_HIGH, I_HIGH_FIRST, 406]
    assert len(sample) == 20
    for i in sample:
        one = codec.small_compress(_dev(torch_cuda, SMALL_INPUTS[i])).cpu().numpy()
        assert np.array_equal(one, h[oo[i]: oo[i + 1]]), i


# ---- 2. the pair at every position ---------------------------------------------------------
PAIR_L = 2088   # two wave tiles of 1024 B and a tail


@pytest.fixture(scope="module")
def pair_sweep():
    """2086 buffers of PAIR_L bytes, all 'x' with " b" at 1 and " a" at p = 3 .. L - 1 (2085 of
    them; the first buffer has " b" alone), back to back from offset 5: the second pair lies
    across every lane, granule and tile boundary. (bytes, offsets, oracle streams)."""
    ps = np.arange(3, PAIR_L)
    X = np.full((1 + ps.size, PAIR_L), ord("x"), np.uint8)
    X[:, 1], X[:, 2] = 0x20, ord("b")
    X[1 + np.arange(ps.size), ps] = 0x20
    X[1 + np.arange(ps.size - 1), ps[:-1] + 1] = ord("a")   # (p = L - 1: the space is the last byte)
    data = np.concatenate([np.full(5, ord(" "), np.uint8), X.reshape(-1), np.full(7, ord("a"), np.uint8)])
    off = 5 + PAIR_L * np.arange(X.shape[0] + 1, dtype=np.int64)
    want = oracle_streams(list(X))
    assert all(s[0] == PRUNED and len(s) == PAIR_L - 1 for s in want[1:-1])   # p <= L - 2: two pairs
    assert all(s[0] == LITERAL and len(s) == PAIR_L + 1 for s in (want[0], want[-1]))   # one pair
    return data, off, want


def test_the_pair_at_every_position(torch_cuda, codec, pair_sweep):
    torch = torch_cuda
    data, off, want = pair_sweep
    assert len(want) == 2086
    h, oo, st = _encode(torch, codec, data, off)
    assert codec.batch_status() == 0
    _check_streams(h, oo, st, want, ("sweep",))
    # and back: the streams the device wrote, into the places the buffers came from
    out = torch.full((data.size + 40,), FILL, dtype=torch.uint8, device="cuda")
    o, dst = codec.small_decompress_batch_into(_dev(torch, h[: oo[-1]]), _dev(torch, oo), _dev(torch, off), out=out)
    got = o.cpu().numpy()
    assert (dst.cpu().numpy() == 0).all() and codec.batch_status() == 0
    assert np.array_equal(got[5: off[-1]], data[5: off[-1]])
    assert (got[:5] == FILL).all() and (got[off[-1]:] == FILL).all()


# ---- 3. wave and grid edges ----------------------------------------------------------------
@pytest.fixture(scope="module")
def wave_text():
    """129 buffers of 33 bytes from offset 5 of one text: the starts take every residue mod 16
    (33 = 2 x 16 + 1), 15 in 16 of them no multiple of 16, every buffer sharing its first and last
    granule with its neighbours. (text, oracle streams)."""
    from data_compression_amd import synth
    text = synth.english_like(5 + 33 * 129 + 11, seed=33)
    bufs = [text[5 + 33 * i: 5 + 33 * (i + 1)] for i in range(129)]
    return text, oracle_streams(bufs)


@pytest.mark.parametrize("grid", (0, 1))   # DC_OPT_BATCH_GRID 1: the persistent loop runs count / 4 rounds
@pytest.mark.parametrize("count", (1, WAVES - 1, WAVES, WAVES + 1, 129))
def test_wave_and_grid_edges(torch_cuda, codec, wave_text, count, grid):
    text, want = wave_text
    off = 5 + 33 * np.arange(count + 1, dtype=np.int64)
    codec.set_option("batch_grid", grid)
    try:
        h, oo, st = _encode(torch_cuda, codec, text, off)
        assert codec.batch_status() == 0
        _check_streams(h, oo, st, want[:count], (count, grid))
        out = torch_cuda.full((text.size + 40,), FILL, dtype=torch_cuda.uint8, device="cuda")
        o, dst = codec.small_decompress_batch_into(_dev(torch_cuda, h[: oo[-1]]), _dev(torch_cuda, oo),
                                                   _dev(torch_cuda, off), out=out)
        got = o.cpu().numpy()
        assert (dst.cpu().numpy() == 0).all()
        assert np.array_equal(got[5: off[-1]], text[5: off[-1]])
        assert (got[:5] == FILL).all() and (got[off[-1]:] == FILL).all()
    finally:
        codec.set_option("batch_grid", 0)


# ---- 4. capacity ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 200, 406))   # the first, a middle and the last workgroup of 102
def test_capacity_falls_inside_a_stream(torch_cuda, codec, k):
    x, off = pack_offsets(SMALL_INPUTS)
    want = oracle_streams(SMALL_INPUTS)
    exp_off = _cum(want)
    assert len(want[k]) >= 2 and (len(SMALL_INPUTS) + WAVES - 1) // WAVES == 102
    cap = int(exp_off[k]) + len(want[k]) // 2
    h, oo, st = _encode(torch_cuda, codec, x, off, out_cap=cap)
    assert codec.batch_status() == DC_E_CAPACITY
    _check_streams(h, oo, st, want, (k,), bad={i: DC_E_CAPACITY for i in range(k, len(want))})
    assert (h[exp_off[k]:] == FILL).all()


# ---- 5. a decreasing offset pair -----------------------------------------------------------
def test_a_decreasing_offset_pair_fails_alone(torch_cuda, codec):
    """off[j + 1] set 7 below off[j]: buffer j ends before it starts (DC_E_ARG, 0 bytes), and
    buffer j + 1 starts inside buffer j - 1; every good buffer is coded as what its offsets say."""
    x, off = pack_offsets(SMALL_INPUTS)
    j = 150
    off = off.copy()
    off[j + 1] = off[j] - 7
    want = list(oracle_streams(SMALL_INPUTS))
    want[j] = b""
    want[j + 1] = orc.small_compress(x[off[j + 1]: off[j + 2]].tobytes())
    h, oo, st = _encode(torch_cuda, codec, x, off)
    assert codec.batch_status() == DC_E_ARG
    _check_streams(h, oo, st, want, (), bad={j: DC_E_ARG})


def test_no_buffers_touches_nothing(torch_cuda, codec):
    h, oo, st = _encode(torch_cuda, codec, np.zeros(0, np.uint8), np.zeros(1, np.int64))
    assert (h == FILL).all() and st.size == 0 and oo.tolist() == [0]


# ---- 6. decode into caller ranges ----------------------------------------------------------
def _decode_gapped(torch, codec, streams, lens, tag, bad=None, cap=None):
    """The streams decoded at gapped output starts (lead 3, gap 5) in ONE call. out_off has count
    + 1 entries, so a gap is an entry of its own: the streams lie in REVERSE order in the input
    (a pad byte between them), which makes the input range of every gap entry, [end of stream i,
    start of stream i + 1), end before it starts: DC_E_ARG, nothing read or written. `lens` are
    the lengths asked for; streams in `bad` (index -> status) fail and write nothing. `cap`: the
    output buffer's size when not the whole layout's. Returns the host output and the (starts,
    ends) of the streams."""
    bad = bad or {}
    n = len(streams)
    starts = 3 + np.concatenate([[0], np.cumsum(np.array(lens[:-1], np.int64) + 5)]).astype(np.int64)
    ends = starts + np.array(lens, np.int64)
    cap = int(ends[-1]) + 5 + 31 if cap is None else cap
    data = np.full(sum(map(len, streams)) + n, 0x3F, np.uint8)
    in_off = np.empty(2 * n, np.int64)
    pos = data.size
    for i, s in enumerate(streams):
        pos -= len(s) + 1
        data[pos: pos + len(s)] = np.frombuffer(s, np.uint8)
        in_off[2 * i], in_off[2 * i + 1] = pos, pos + len(s)
    assert (in_off[2::2] < in_off[1:-1:2]).all()   # every gap entry's input range decreases
    out_off = np.empty(2 * n, np.int64)
    out_off[0::2], out_off[1::2] = starts, ends
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    o, st = codec.small_decompress_batch_into(_dev(torch, data), _dev(torch, in_off), _dev(torch, out_off), out=out)
    assert o is out
    h, st = o.cpu().numpy(), st.cpu().numpy()
    assert st.size == 2 * n - 1 and (st[1::2] == DC_E_ARG).all(), tag + ("gap entries",)
    st = st[0::2]
    good = np.zeros(cap, bool)
    for i in range(n):
        assert st[i] == bad.get(i, 0), tag + (i, "status", int(st[i]))
        if i not in bad:
            good[starts[i]: ends[i]] = True
    assert (h[~good] == FILL).all(), tag + ("bytes outside the good streams' ranges written",)
    lowest = DC_E_ARG if n > 1 else 0   # entry 1, the first gap ...
    if 0 in bad:
        lowest = bad[0]                 # ... unless stream 0 (entry 0) fails
    assert codec.batch_status() == lowest, tag + ("batch_status",)
    return h, starts, ends


@pytest.fixture(scope="module")
def decoded_by_oracle():
    return tuple(orc.small_decompress(s) for s in oracle_streams(SMALL_INPUTS))


def test_decode_of_the_oracle_streams_at_gapped_starts(torch_cuda, codec, decoded_by_oracle):
    streams = oracle_streams(SMALL_INPUTS)
    lens = [len(d) for d in decoded_by_oracle]
    assert lens[I_HIGH] > SMALL_INPUTS[I_HIGH].size and lens[I_HIGH_FIRST] == SMALL_INPUTS[I_HIGH_FIRST].size
    h, starts, ends = _decode_gapped(torch_cuda, codec, streams, lens, ("all",))
    for i, d in enumerate(decoded_by_oracle):
        assert h[starts[i]: ends[i]].tobytes() == d, i
    # the high-byte buffer asked at its INPUT length: DC_E_STREAM, and its range keeps the prefill
    lens[I_HIGH] = SMALL_INPUTS[I_HIGH].size
    h, starts, ends = _decode_gapped(torch_cuda, codec, streams, lens, ("high",), bad={I_HIGH: DC_E_STREAM})
    for i, d in enumerate(decoded_by_oracle):
        if i != I_HIGH:
            assert h[starts[i]: ends[i]].tobytes() == d, i


def test_decode_round_trip_of_the_device_streams(torch_cuda, codec, encoded):
    torch = torch_cuda
    (h, oo, _, _), x, off = encoded
    out = torch.full((x.size + 40,), FILL, dtype=torch.uint8, device="cuda")
    o, st = codec.small_decompress_batch_into(_dev(torch, h[: oo[-1]]), _dev(torch, oo), _dev(torch, off), out=out)
    got, st = o.cpu().numpy(), st.cpu().numpy()
    for i, b in enumerate(SMALL_INPUTS):
        if i == I_HIGH:
            assert st[i] == DC_E_STREAM and (got[off[i]: off[i + 1]] == FILL).all()
            continue
        assert st[i] == 0, (i, int(st[i]))
        assert got[off[i]: off[i + 1]].tobytes() == b.tobytes(), i
    assert (got[x.size:] == FILL).all()
    assert codec.batch_status() == DC_E_STREAM


# ---- 7. decode edges -----------------------------------------------------------------------
@pytest.mark.parametrize("delta", (1, -1))
def test_wrong_asked_length_fails_alone_and_writes_nothing(torch_cuda, codec, delta, decoded_by_oracle):
    """A pruned stream (buffer 93: 65 537 bytes of text) and a LITERAL stream (the 100 random bytes)
    asked for one byte more or less than they hold: DC_E_STREAM for exactly those two, and not a
    byte of their ranges written."""
    streams = oracle_streams(SMALL_INPUTS)
    i_pru, i_lit = 93, I_RANDOM_100
    assert streams[i_pru][0] == PRUNED and streams[i_lit][0] == LITERAL
    pick = list(range(86, 100))   # more than one workgroup, around both
    sub = [streams[i] for i in pick]
    lens = [len(decoded_by_oracle[i]) for i in pick]
    bad = {}
    for i in (i_pru, i_lit):
        lens[pick.index(i)] += delta
        bad[pick.index(i)] = DC_E_STREAM
    h, starts, ends = _decode_gapped(torch_cuda, codec, sub, lens, (delta,), bad=bad)
    for p, i in enumerate(pick):
        if p not in bad:
            assert h[starts[p]: ends[p]].tobytes() == decoded_by_oracle[i], (delta, i)


def test_streams_that_hold_nothing(torch_cuda, codec):
    """An empty stream, a lone type byte of either form and an unknown type byte decode to nothing,
    as in the oracle: DC_OK exactly when length 0 was asked for."""
    streams = [b"", b" ", b"\x08", b"Zabc", b"\x08a", b" q"]
    want = [orc.small_decompress(s) for s in streams]
    assert want == [b"", b"", b"", b"", b"a", b"q"]
    h, starts, ends = _decode_gapped(torch_cuda, codec, streams, [len(w) for w in want], ("zero",))
    assert h[starts[4]: ends[4]].tobytes() == b"a" and h[starts[5]: ends[5]].tobytes() == b"q"
    bad = {i: DC_E_STREAM for i in range(4)}
    h, starts, ends = _decode_gapped(torch_cuda, codec, streams, [1, 1, 1, 1, 1, 1], ("one",), bad=bad)
    assert h[starts[4]: ends[4]].tobytes() == b"a" and h[starts[5]: ends[5]].tobytes() == b"q"


def test_a_range_past_the_capacity_fails_alone(torch_cuda, codec, decoded_by_oracle):
    streams = oracle_streams(SMALL_INPUTS)
    pick = [40, 50, 60, 70]
    sub = [streams[i] for i in pick]
    lens = [len(decoded_by_oracle[i]) for i in pick]
    whole = 3 + sum(lens) + 5 * 3
    h, starts, ends = _decode_gapped(torch_cuda, codec, sub, lens, ("cap",), bad={3: DC_E_CAPACITY}, cap=whole - 1)
    for p, i in enumerate(pick[:3]):
        assert h[starts[p]: ends[p]].tobytes() == decoded_by_oracle[i], i


# ---- 8. round trip of blocks, no host read in between --------------------------------------
@pytest.mark.parametrize("block", (4096, 100))
def test_blocks_round_trip_on_the_device(torch_cuda, codec, block):
    torch = torch_cuda
    from data_compression_amd import synth
    n = 1 << 20
    x = _dev(torch, synth.english_like(n, seed=29))
    count = (n + block - 1) // block
    in_off = torch.arange(0, n + block, block, dtype=torch.int64, device="cuda").clamp_(max=n)[: count + 1].contiguous()
    back = torch.full((n + 40,), FILL, dtype=torch.uint8, device="cuda")
    o, oo, st = codec.small_compress_blocks(x, block)
    got, dst = codec.small_decompress_batch_into(o, oo, in_off, out=back)   # (everything above is enqueued)
    assert got is back and st.numel() == count and dst.numel() == count
    assert codec.batch_status() == 0 and int(st.abs().sum()) == 0 and int(dst.abs().sum()) == 0
    assert torch.equal(back[:n], x) and bool((back[n:] == FILL).all())
    assert int(oo[-1]) < n   # text: the pruned form pays
