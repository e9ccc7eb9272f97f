"""The per-entry status of the four byte-stream batch calls (dc_gpu.h "byte-stream batch v1"), at
buffers of 3 to 40 bytes: k_nyb_batch_enc, k_nyb_batch_dec_async, k_small_batch_enc and
k_small_batch_dec decide it in one shared frame (bs_item / bs_report). The expected status of
every entry is frame_status below, written from the header and computed from the two offset arrays
alone; batch_status() is the lowest failing entry's; the output is prefilled, good entries hold the
oracle's bytes, and every other byte keeps the prefill. (The header lets the nybble decode leave
anything in the own range of a stream that fails as DC_E_STREAM; the frame gives no such status, so
nothing is exempt here.)"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.stream_batch_checks import DC_E_ARG, DC_E_CAPACITY, FILL, _check_streams, _cum, _dev, pack_offsets

pytestmark = pytest.mark.gpu

SIZES = (3, 17, 40, 24, 9, 31, 5, 40, 12, 3)


def frame_status(in_off, out_off, out_cap, dec):
    st = []
    for (a, b), (o0, o1) in zip(zip(in_off, in_off[1:]), zip(out_off, out_off[1:])):
        arg = b < a or (dec and o1 < o0)
        st.append(DC_E_ARG if arg else DC_E_CAPACITY if o1 > out_cap or o1 < o0 else 0)
    return st


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


def _buffers():
    from data_compression_amd import synth
    return [synth.english_like(n, seed=500 + i) for i, n in enumerate(SIZES)]


def _lowest(st):
    return next((s for s in st if s != 0), 0)


def _encode_case(torch, codec, compress, call):
    """Ten buffers; the pairs of entries 2 and 7 decrease (each next buffer starts 2 bytes inside
    the one before), and out_cap falls inside stream 4: entries 0, 1, 3 good, 2 DC_E_ARG, 4 to 9
    DC_E_CAPACITY but for 7, which is DC_E_ARG although the capacity ran out before it."""
    x, off = pack_offsets(_buffers())
    off = off.copy()
    for j in (2, 7):
        off[j + 1] = off[j] - 2
    bufs = [x[off[i]: off[i + 1]].tobytes() if off[i + 1] >= off[i] else None for i in range(len(SIZES))]
    want = [b"" if b is None else compress(b) for b in bufs]
    exp_off = _cum(want)
    cap = int(exp_off[4]) + len(want[4]) // 2
    assert exp_off[4] < cap < exp_off[5]
    exp = frame_status(off.tolist(), exp_off.tolist(), cap, False)
    assert exp == [0, 0, DC_E_ARG, 0] + [DC_E_CAPACITY] * 3 + [DC_E_ARG] + [DC_E_CAPACITY] * 2   # every case occurs
    out = torch.full((int(exp_off[-1]) + 48,), FILL, dtype=torch.uint8, device="cuda")
    o, oo, st = call(_dev(torch, x), _dev(torch, off), out=out, out_cap=cap)
    bstat = codec.batch_status()
    h, oo, st = o.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()
    print(call.__name__, "status", st.tolist(), "batch_status", bstat)
    assert st.tolist() == exp
    _check_streams(h, oo, st, want, (call.__name__,), bad={i: s for i, s in enumerate(exp) if s})
    assert bstat == _lowest(exp) == DC_E_ARG


def _decode_case(torch, codec, compress, decompress, call):
    """Four streams A B C D and nine entries. In memory the streams lie B C A D (a pad byte around
    each), in the output A C B D (5 bytes around each):
      0 A good                      1 input pair decreases, output pair rises         DC_E_ARG
      2 B good                      3 input rises, output pair decreases              DC_E_ARG
      4 C good                      5 input rises, output end past out_cap            DC_E_CAPACITY
      6 input pair decreases and output end past out_cap                              DC_E_ARG
      7 input rises, output pair decreases (back below out_cap)                       DC_E_ARG
      8 D good"""
    bufs = [b.tobytes() for b in _buffers()[:4]]
    A, B, C, D = (compress(b) for b in bufs)
    assert [decompress(s) for s in (A, B, C, D)] == bufs
    nA, nB, nC, nD = (len(b) for b in bufs)
    data = np.full(len(A) + len(B) + len(C) + len(D) + 5, 0x3F, np.uint8)
    pos = {}
    p = 1
    for name, s in (("B", B), ("C", C), ("A", A), ("D", D)):
        data[p: p + len(s)] = np.frombuffer(s, np.uint8)
        pos[name] = (p, p + len(s))
        p += len(s) + 1
    oA = 3
    oC = oA + nA + 5
    oB = oC + nC + 5
    oD = oB + nB + 5
    cap = oD + nD + 5
    in_off = [pos["A"][0], pos["A"][1], pos["B"][0], pos["B"][1], pos["C"][0], pos["C"][1], pos["C"][1] + 1, 0,
              pos["D"][0], pos["D"][1]]
    out_off = [oA, oA + nA, oB, oB + nB, oC, oC + nC, cap + 7, cap + 9, oD, oD + nD]
    exp = frame_status(in_off, out_off, cap, True)
    assert exp == [0, DC_E_ARG, 0, DC_E_ARG, 0, DC_E_CAPACITY, DC_E_ARG, DC_E_ARG, 0]
    pairs = list(zip(zip(in_off, in_off[1:]), zip(out_off, out_off[1:])))
    (a, b), (o0, o1) = pairs[1]
    assert b < a and o1 > o0 and o1 <= cap                 # input decreases, output rises
    (a, b), (o0, o1) = pairs[3]
    assert b > a and o1 < o0                               # input rises, output decreases
    (a, b), (o0, o1) = pairs[5]
    assert b > a and o1 > o0 and o1 > cap                  # output end past out_cap
    (a, b), (o0, o1) = pairs[6]
    assert b < a and o1 > o0 and o1 > cap                  # both: the input pair decides
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    o, st = call(_dev(torch, data), _dev(torch, np.array(in_off, np.int64)), _dev(torch, np.array(out_off, np.int64)), out)
    bstat = codec.batch_status()
    assert o is out
    h, st = o.cpu().numpy(), st.cpu().numpy()
    print(call.__name__, "status", st.tolist(), "batch_status", bstat)
    assert st.tolist() == exp
    asked = np.zeros(cap, bool)
    for i, want in ((0, bufs[0]), (2, bufs[1]), (4, bufs[2]), (8, bufs[3])):
        assert h[out_off[i]: out_off[i + 1]].tobytes() == want, (call.__name__, i)
        asked[out_off[i]: out_off[i + 1]] = True
    assert (h[~asked] == FILL).all(), (call.__name__, "bytes of no good entry written")
    assert bstat == _lowest(exp) == DC_E_ARG


@pytest.mark.parametrize("call", ("nyb_compress_batch", "nyb_decompress_batch_into", "small_compress_batch",
                                  "small_decompress_batch_into"))
def test_status_of_every_entry_is_the_frame_rule(torch_cuda, codec, call):
    modes = (False, True) if call.startswith("nyb") else (None,)
    for modify in modes:
        if call == "nyb_compress_batch":
            def run(x, off, out, out_cap):
                return codec.nyb_compress_batch(x, off, modify, out=out, out_cap=out_cap)
            run.__name__ = "%s(modify=%s)" % (call, modify)
            _encode_case(torch_cuda, codec, lambda b: orc.nybble_compress(b, modify), run)
        elif call == "small_compress_batch":
            _encode_case(torch_cuda, codec, orc.small_compress, codec.small_compress_batch)
        elif call == "nyb_decompress_batch_into":
            def run(data, off, out_off, out):
                return codec.nyb_decompress_batch_into(data, off, modify, out_off, out=out)
            run.__name__ = "%s(modify=%s)" % (call, modify)
            _decode_case(torch_cuda, codec, lambda b: orc.nybble_compress(b, modify),
                         lambda s: orc.nybble_decompress(s, modify), run)
        else:
            def run(data, off, out_off, out):
                return codec.small_decompress_batch_into(data, off, out_off, out=out)
            run.__name__ = call
            _decode_case(torch_cuda, codec, orc.small_compress, orc.small_decompress, run)
