"""dc_nyb_decompress at the cuts of its own kernels: this file only runs the catalogue of
tests/nyb_decode_model.py (what it reaches is asserted by tests/test_nyb_decode_model_cpu.py).

Every case goes through dc_nyb_decompress under the modes it names, the input at the byte of a 16-B
granule it names, the output into a view at the byte it names of a buffer of 0xEE with 64 guard bytes
either side; the view is the 2 * m bytes the call is given. Bytes and length must be
oracle.nybble_decompress's, and every byte outside [0, n) must stay 0xEE. One context runs all cases,
so nyb_wtile_off and nyb_adec_seg switch between them. The streams under 64 KiB then go through
dc_nyb_decompress_batch, one call per mode, and each output must equal the single call's.
"""
import ctypes as C

import numpy as np
import pytest

from tests import nyb_decode_model as M

pytestmark = pytest.mark.gpu

FILL = 0xEE
GUARD = 64
DC_E_ARG = -1
_SINGLE = {}   # (stream, modify) -> what the single call gave


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


def _set_or_skip(c, name, value):
    """an A/B variant: the product library has variant 0 alone (DC_AB_KERNELS builds have the others)"""
    from data_compression_amd._lib import DcError
    try:
        c.set_option(name, value)
    except DcError:
        pytest.skip(f"{name}={value}: A/B kernels not in this build (DC_AB_KERNELS)")


def _dev(torch, data, off):
    """data at byte `off` of a 16-B aligned device buffer of 0xE1 (a hit and a literal start, if a
    kernel took a byte beside the stream for an element)"""
    a = np.frombuffer(bytes(data), np.uint8)
    host = np.full(off + a.size + 64, 0xE1, np.uint8)
    host[off: off + a.size] = a
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + off


def _decode(torch, codec, stream, modify, in_align, out_align):
    """dc_nyb_decompress into the guarded view: the bytes, after the length and the guards are checked"""
    from data_compression_amd._lib import check
    m = len(stream)
    keep, src = _dev(torch, stream, in_align)
    start = GUARD + out_align
    buf = torch.full((start + 2 * m + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    ln = C.c_uint64(1 << 40)
    check("dc_nyb_decompress", codec.L.dc_nyb_decompress(codec.ctx, src, m, int(modify), buf.data_ptr() + start, C.byref(ln)))
    h = buf.cpu().numpy()
    n = ln.value
    assert n <= 2 * m, "length %d over the 2 * m = %d bytes given" % (n, 2 * m)
    assert (h[:start] == FILL).all(), "bytes before the output were written"
    assert (h[start + n:] == FILL).all(), "bytes from the returned length on were written"
    del keep
    return h[start: start + n].tobytes()


def _same(got, want, tag):
    assert len(got) == len(want), tag + ("length", len(got), len(want))
    assert got == want, tag + ("bytes differ first at", next(k for k in range(len(want)) if got[k] != want[k]))


def _run_case(torch, codec, c):
    codec.set_option("nyb_wtile_off", c.wtile_off)
    if c.seg:
        codec.set_option("nyb_adec_seg", c.seg)
    try:
        for modify in c.modes:
            got = _decode(torch, codec, c.stream, modify, c.in_align, c.out_align)
            _same(got, M.expected(c.stream, modify), (c.family, c.name, modify))
            _SINGLE[c.stream, modify] = got
            if c.follow is not None:   # first = 1 ignores the state the segments before left
                got = _decode(torch, codec, c.follow, modify, 0, 0)
                _same(got, M.expected(c.follow, modify), (c.family, c.name, modify, "follow"))
    finally:
        codec.set_option("nyb_wtile_off", 0)
        if c.seg:
            codec.set_option("nyb_adec_seg", 0)


@pytest.mark.parametrize("family", tuple(M.FAMILIES))
def test_decode_catalogue(torch_cuda, codec, family):
    cases = M.catalogue(family)
    assert cases
    for c in cases:
        _run_case(torch_cuda, codec, c)


@pytest.mark.parametrize("v1", [3, 1])
def test_resolve_catalogue_under_the_other_resolves(torch_cuda, codec, v1):
    """the resolve family through k_nyb_resolve_s (3) and the one-pass k_nyb_adec (1), where the library has them"""
    _set_or_skip(codec, "nyb_adec_v1", v1)
    try:
        for c in M.catalogue("resolve"):
            _run_case(torch_cuda, codec, c)
    finally:
        codec.set_option("nyb_adec_v1", 0)


@pytest.mark.parametrize("modify", [False, True], ids=["static", "adaptive"])
def test_batch_gives_the_single_calls_outputs(torch_cuda, codec, modify):
    """every catalogue stream under 64 KiB through dc_nyb_decompress_batch (a lane per stream), one call"""
    torch = torch_cuda
    streams = list(dict.fromkeys(c.stream for c in M.catalogue() if modify in c.modes and len(c.stream) < 65536))
    assert len(streams) > 300
    off = np.concatenate(([0], np.cumsum([len(s) for s in streams]))).astype(np.int64)
    data = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()).cuda()
    out, out_off = codec.nyb_decompress_batch(data, torch.from_numpy(off).cuda(), modify)
    out, out_off = out.cpu().numpy(), out_off.cpu().numpy()
    for k, s in enumerate(streams):
        single = _SINGLE.get((s, modify))
        if single is None:
            single = _decode(torch, codec, s, modify, 0, 0)
        _same(out[out_off[k]: out_off[k + 1]].tobytes(), single, ("batch", k, modify))


def test_argument_errors(torch_cuda, codec):
    """NULL pointers: DC_E_ARG and no write; m = 0 with a NULL input is the empty stream"""
    torch = torch_cuda
    L, ctx = codec.L, codec.ctx
    s = M.catalogue("ends")[10].stream
    keep, src = _dev(torch, s, 0)
    buf = torch.full((2 * len(s) + 64,), FILL, dtype=torch.uint8, device="cuda")
    ln = C.c_uint64(77)
    for modify in (0, 1):
        bad = {"no ctx": L.dc_nyb_decompress(None, src, len(s), modify, buf.data_ptr(), C.byref(ln)),
               "no input": L.dc_nyb_decompress(ctx, None, len(s), modify, buf.data_ptr(), C.byref(ln)),
               "no output": L.dc_nyb_decompress(ctx, src, len(s), modify, None, C.byref(ln)),
               "no length": L.dc_nyb_decompress(ctx, src, len(s), modify, buf.data_ptr(), None)}
        assert {k: v for k, v in bad.items() if v != DC_E_ARG} == {}
        assert ln.value == 77 and bool((buf == FILL).all())
        assert L.dc_nyb_decompress(ctx, None, 0, modify, buf.data_ptr(), C.byref(ln)) == 0 and ln.value == 0
        ln.value = 77
    assert bool((buf == FILL).all())
    del keep


def test_segment_option_range(codec):
    """0 and 1 .. 16 Mi; the default path is value 0"""
    from data_compression_amd._lib import DcError
    for v in (1, 64, 16 << 20, 0):
        codec.set_option("nyb_adec_seg", v)
    for v in (-1, (16 << 20) + 1):
        with pytest.raises(DcError):
            codec.set_option("nyb_adec_seg", v)
