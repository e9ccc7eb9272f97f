"""The host driver of the stream codecs (dc_core.hip from `struct dc_ctx` on): which stages each
call launches and in what order, the exit state of the shard-body writes when another call uses
the context's pinned block between plan and write, and that closing a context returns its
workspace.

The stage lists of STAGES were recorded by running `_stages` at the commit before the host-side
refactor (one workspace type, explicit read-backs, one transducer run); they pin the LAUNCH names
and their order per call, which bench.py maps to kernels and bytes. They do not tell the writer
or k_mtf_walk<..> variants apart (a kernel trace does).
"""
import ctypes as C

import numpy as np
import pytest

from data_compression_amd import synth
from data_compression_amd.dist import INITIAL_LISTS
from tests.cpu_engine import CpuEngine
from tests.nyb_shard_stitch import cpu_put

pytestmark = pytest.mark.gpu

TILE = 4096
N1 = 1
N2 = TILE + 1 + 1          # 4097 elements: two tiles
NBIG = 65 * TILE + 4       # adaptive encode: a second mtf_reduce / mtf_down level
TEXT = synth.english_like(NBIG + 16).tobytes()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dev(torch, data, off=0):
    """data at byte `off` of a 16-B aligned device buffer"""
    a = np.frombuffer(bytes(data), np.uint8)
    host = np.full(off + a.size + 64, 0x65, np.uint8)
    host[off: off + a.size] = a
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf[off: off + a.size]


def _timed(codec, fn):
    codec.timing(True)
    try:
        fn()
        return [name for name, _ in codec.timings()]
    finally:
        codec.timing(False)


# ---- stage names ----------------------------------------------------------------------------------
def _nyb_compress(torch, Codec, n, modify, off):
    c = Codec(0)
    x = _dev(torch, TEXT[:n], off)
    return _timed(c, lambda: c.nyb_compress(x, modify))


def _nyb_decompress(torch, Codec, n, modify, off):
    c = Codec(0)
    comp = _dev(torch, c.nyb_compress(_dev(torch, TEXT[:n]), modify).cpu().numpy().tobytes(), off)
    return _timed(c, lambda: c.nyb_decompress(comp, modify))


def _small(torch, Codec, n, decode):
    c = Codec(0)
    x = _dev(torch, TEXT[:n])
    if not decode:
        return _timed(c, lambda: c.small_compress(x))
    comp = _dev(torch, c.small_compress(x).cpu().numpy().tobytes())
    return _timed(c, lambda: c.small_decompress(comp))


def _headers_only(torch, Codec, kind, modify):
    """a stream of its type byte and first byte alone: no elements, no tiles"""
    c = Codec(0)
    if kind == "nyb":
        comp = _dev(torch, b"\xAF\x41")
        return _timed(c, lambda: c.nyb_decompress(comp, modify))
    comp = _dev(torch, b"\x08\x41")
    return _timed(c, lambda: c.small_decompress(comp))


def _small_body(torch, Codec, nelem, left_halo):
    c = Codec(0)
    y = _dev(torch, TEXT[: nelem + 2])
    out = torch.empty(2 * nelem + 64, dtype=torch.uint8, device="cuda")

    def run():
        c.small_body_plan(y, left_halo, nelem)
        c.small_body_write(y, left_halo, nelem, out)
    return _timed(c, run)


def _nyb_body(torch, Codec, n, modify, off):
    c = Codec(0)
    y = _dev(torch, TEXT[:n], off)

    def run():
        c.nyb_body_plan(y, modify, INITIAL_LISTS)
        c.nyb_body_write(y, modify, -1, True)
    return _timed(c, run)


def _nyb_dbody(torch, Codec, n, off):
    c = Codec(0)
    body = c.nyb_compress(_dev(torch, TEXT[:n]), False).cpu().numpy().tobytes()[2:]
    y = _dev(torch, body if body else b"\x00", off)
    m = len(body)

    def run():
        c.nyb_dbody_plan(y[:m], m)
        c.nyb_dbody_write(y[:m], m, 0)
    return _timed(c, run)


def _small_huff_decode(torch, Codec, n):
    c = Codec(0)
    enc = c.small_huff_encode(_dev(torch, TEXT[:n]), sync_syms=64)
    assert enc["fused"] and enc["S"] == 64
    return _timed(c, lambda: c.small_huff_decode(enc))


def _chunked(torch, Codec, n, decode):
    c = Codec(0)
    x = _dev(torch, TEXT[:n])
    if not decode:
        return _timed(c, lambda: c.nyb_compress_chunked(x, True, 1024))
    comp = c.nyb_compress_chunked(x, True, 1024)
    return _timed(c, lambda: c.nyb_decompress_chunked(comp))


def _huff_decodes(torch, Codec, fresh):
    c = Codec(0)
    enc = c.encode(_dev(torch, TEXT[:N2]), sync_syms=64)
    d = Codec(0) if fresh else c
    out = torch.empty(N2 + 64, dtype=torch.uint8, device="cuda")

    def run():
        d.decode_into(enc, out)
        d.decode_range(enc, 100, 3000, out=out)
        d.decode_ranges(enc, [0, 4090], [10, 8], out=out)
    return _timed(d, run)


CASES = {}
for _n in (N1, N2):
    for _mod in (False, True):
        for _off in (0, 3):
            _tag = "%s_n%d_a%d" % ("adaptive" if _mod else "static", _n, _off)
            CASES["nyb_compress_" + _tag] = (_nyb_compress, _n, _mod, _off)
            CASES["nyb_decompress_" + _tag] = (_nyb_decompress, _n, _mod, _off)
            CASES["nyb_body_" + _tag] = (_nyb_body, _n, _mod, _off)
    for _off in (0, 3):
        CASES["nyb_dbody_n%d_a%d" % (_n, _off)] = (_nyb_dbody, _n, _off)
    CASES["small_compress_n%d" % _n] = (_small, _n, False)
    CASES["small_decompress_n%d" % _n] = (_small, _n, True)
    CASES["chunked_compress_n%d" % _n] = (_chunked, _n, False)
    CASES["chunked_decompress_n%d" % _n] = (_chunked, _n, True)
for _off in (0, 3):
    CASES["nyb_compress_adaptive_big_a%d" % _off] = (_nyb_compress, NBIG, True, _off)
for _halo in (False, True):
    for _ne in (1, TILE + 1):
        CASES["small_body_halo%d_nelem%d" % (_halo, _ne)] = (_small_body, _ne, _halo)
CASES["nyb_decompress_static_no_elements"] = (_headers_only, "nyb", False)
CASES["nyb_decompress_adaptive_no_elements"] = (_headers_only, "nyb", True)
CASES["small_decompress_no_elements"] = (_headers_only, "small", False)
CASES["small_huff_decode_S64"] = (_small_huff_decode, N2)
CASES["huff_decodes_after_pack"] = (_huff_decodes, False)
CASES["huff_decodes_fresh_context"] = (_huff_decodes, True)


def _stages(torch, name):
    from data_compression_amd.device import Codec
    fn, *args = CASES[name]
    return fn(torch, Codec, *args)


_SCAN = ["fsm_scan_up", "fsm_scan"]
STAGES = {
    "nyb_compress_static_n1_a0": ["nyb_enc_write"],
    "nyb_decompress_static_n1_a0": [],
    "nyb_body_static_n1_a0": ["nyb_enc_write"],
    "nyb_compress_static_n1_a3": ["nyb_enc_write"],
    "nyb_decompress_static_n1_a3": [],
    "nyb_body_static_n1_a3": ["nyb_enc_write"],
    "nyb_compress_adaptive_n1_a0": ["nyb_enc_write"],
    "nyb_decompress_adaptive_n1_a0": [],
    "nyb_body_adaptive_n1_a0": ["nyb_enc_write"],
    "nyb_compress_adaptive_n1_a3": ["nyb_enc_write"],
    "nyb_decompress_adaptive_n1_a3": [],
    "nyb_body_adaptive_n1_a3": ["nyb_enc_write"],
    "nyb_dbody_n1_a0": ["nyb_dbody_write"],
    "nyb_dbody_n1_a3": ["nyb_dbody_write"],
    "small_compress_n1": ["small_write"],
    "small_decompress_n1": [],
    "chunked_compress_n1": ["nyb_chunk_enc", "nyb_chunk_scan", "nyb_chunk_copy"],
    "chunked_decompress_n1": ["nyb_chunk_dec"],
    "nyb_compress_static_n4098_a0": ["nyb_enc_tiles"] + _SCAN + ["nyb_enc_write"],
    "nyb_decompress_static_n4098_a0": ["nyb_dec_tiles"] + _SCAN + ["nyb_dec_write"],
    "nyb_body_static_n4098_a0": ["nyb_body_tiles"] + _SCAN + ["nyb_body_tiles"] + _SCAN + ["nyb_enc_write"],
    "nyb_compress_static_n4098_a3": ["nyb_enc_tiles"] + _SCAN + ["nyb_enc_write"],
    "nyb_decompress_static_n4098_a3": ["nyb_dec_tiles"] + _SCAN + ["nyb_dec_write"],
    "nyb_body_static_n4098_a3": ["nyb_body_tiles"] + _SCAN + ["nyb_body_tiles"] + _SCAN + ["nyb_enc_write"],
    "nyb_compress_adaptive_n4098_a0": ["mtf_tiles", "mtf_down", "mtf_ranks"] + _SCAN + ["nyb_enc_write"],
    "nyb_decompress_adaptive_n4098_a0": ["nyb_tok_tiles"] + _SCAN + ["nyb_dec_write", "nyb_adec_ctl", "nyb_resolve"],
    "nyb_body_adaptive_n4098_a0": ["mtf_tiles", "mtf_down", "mtf_ranks"] + _SCAN + _SCAN + ["nyb_enc_write"],
    "nyb_compress_adaptive_n4098_a3": ["mtf_tiles", "mtf_down", "mtf_ranks"] + _SCAN + ["nyb_enc_write"],
    "nyb_decompress_adaptive_n4098_a3": ["nyb_tok_tiles"] + _SCAN + ["nyb_dec_write", "nyb_adec_ctl", "nyb_resolve"],
    "nyb_body_adaptive_n4098_a3": ["mtf_tiles", "mtf_down", "mtf_ranks"] + _SCAN + _SCAN + ["nyb_enc_write"],
    "nyb_dbody_n4098_a0": ["nyb_dbody_tiles"] + _SCAN + ["nyb_dbody_tiles"] + _SCAN + ["nyb_dbody_write"],
    "nyb_dbody_n4098_a3": ["nyb_dbody_tiles"] + _SCAN + ["nyb_dbody_tiles"] + _SCAN + ["nyb_dbody_write"],
    "small_compress_n4098": ["small_enc_tiles"] + _SCAN + ["small_write"],
    "small_decompress_n4098": ["small_dec_tiles"] + _SCAN + ["small_dec_write"],
    "chunked_compress_n4098": ["nyb_chunk_enc", "nyb_chunk_scan", "nyb_chunk_copy"],
    "chunked_decompress_n4098": ["nyb_chunk_dec"],
    "nyb_compress_adaptive_big_a0": ["mtf_tiles", "mtf_reduce", "mtf_down", "mtf_down", "mtf_ranks"] + _SCAN + ["nyb_enc_write"],
    "nyb_compress_adaptive_big_a3": ["mtf_tiles", "mtf_reduce", "mtf_down", "mtf_down", "mtf_ranks"] + _SCAN + ["nyb_enc_write"],
    "small_body_halo0_nelem1": ["small_body_tiles"] + _SCAN + ["small_write"],
    "small_body_halo0_nelem4097": ["small_body_tiles"] + _SCAN + ["small_write"],
    "small_body_halo1_nelem1": ["small_body_tiles"] + _SCAN + ["small_write"],
    "small_body_halo1_nelem4097": ["small_body_tiles"] + _SCAN + ["small_write"],
    "nyb_decompress_static_no_elements": ["nyb_dec_write"],
    "nyb_decompress_adaptive_no_elements": ["nyb_dec_write"],
    "small_decompress_no_elements": ["small_dec_write"],
    "small_huff_decode_S64": ["huff_decode", "huff_decode_fix", "small_dec_summ"] + _SCAN + ["small_dec_write"],
    "huff_decodes_after_pack": ["huff_decode", "huff_decode_fix", "huff_decode_ranges", "huff_range_items", "huff_range_scan", "huff_decode_ranges"],
    "huff_decodes_fresh_context": ["dec_tables", "huff_decode", "huff_decode_fix", "dec_tables", "huff_decode_ranges", "dec_tables", "huff_range_items", "huff_range_scan", "huff_decode_ranges"],
}


@pytest.mark.parametrize("name", tuple(CASES))
def test_stage_names(torch_cuda, name):
    assert _stages(torch_cuda, name) == STAGES[name]


def test_every_case_has_its_stages():
    assert set(STAGES) == set(CASES)


# ---- exit state of the shard-body writes --------------------------------------------------------
def _disturb(torch, codec, how):
    """a call on the same context that reads back through its pinned block or the stream"""
    if how == "decode_status":
        codec.decode_status()
    else:
        codec.crc32(torch.arange(0, 200, dtype=torch.uint8, device="cuda"))
        codec.nyb_compress(torch.full((40,), 0x7A, dtype=torch.uint8, device="cuda"), False)


@pytest.mark.parametrize("how", ["decode_status", "crc32_and_compress"])
@pytest.mark.parametrize("modify", [False, True], ids=["static", "adaptive"])
@pytest.mark.parametrize("n", [2, 17, 4098])
def test_body_write_exit_state_after_another_call(torch_cuda, n, modify, how):
    """*h_state_out of dc_nyb_body_write is the model's exit state (and the body the model's) when
    another call runs between the plan and the write: both is_last values, pend_rank -1 and 3"""
    from data_compression_amd._lib import check
    from data_compression_amd.device import Codec
    torch = torch_cuda
    codec = Codec(0)
    x = TEXT[100: 100 + n]
    eng = CpuEngine()
    eng.nyb_body_plan(cpu_put(x), modify, INITIAL_LISTS)
    y = _dev(torch, x)
    for pend in (-1, 3):
        for is_last in (0, 1):
            codec.nyb_body_plan(y, modify, INITIAL_LISTS)
            _disturb(torch, codec, how)   # (a static compress keeps the ranks of the adaptive plan)
            out = torch.full((2 * n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            ln, st = C.c_uint64(1 << 40), C.c_int32(-7)
            check("dc_nyb_body_write", codec.L.dc_nyb_body_write(codec.ctx, y.data_ptr(), n, int(modify), pend, is_last,
                                                                 out.data_ptr(), C.byref(ln), C.byref(st)))
            want = eng.nyb_body_write(cpu_put(x), modify, pend, bool(is_last)).numpy().tobytes()
            assert out[: ln.value].cpu().numpy().tobytes() == want, (pend, is_last)
            assert st.value == eng.nyb_body_state(pend), (pend, is_last, st.value)
    codec.close()


@pytest.mark.parametrize("how", ["decode_status", "crc32_and_compress"])
@pytest.mark.parametrize("n", [2, 17, 4098])
def test_dbody_write_exit_state_after_another_call(torch_cuda, n, how):
    """*h_state_out of dc_nyb_dbody_write is the model's exit state from either entry state"""
    from data_compression_amd._lib import check
    from data_compression_amd.device import Codec
    torch = torch_cuda
    codec = Codec(0)
    comp = codec.nyb_compress(_dev(torch, TEXT[: 2 * n + 64]), False).cpu().numpy().tobytes()
    assert comp[0] == 0xAF and len(comp) >= 2 + n
    body = comp[2: 2 + n]
    eng = CpuEngine()
    plan = eng.nyb_dbody_plan(cpu_put(body), n)
    y = _dev(torch, body)
    for s_in in (0, 1):
        assert codec.nyb_dbody_plan(y, n) == plan
        _disturb(torch, codec, how)
        out = torch.full((2 * n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        ln, st = C.c_uint64(1 << 40), C.c_int32(-7)
        check("dc_nyb_dbody_write", codec.L.dc_nyb_dbody_write(codec.ctx, y.data_ptr(), n, n, s_in, out.data_ptr(),
                                                               C.byref(ln), C.byref(st)))
        want = eng.nyb_dbody_write(cpu_put(body), n, s_in).numpy().tobytes()
        assert out[: ln.value].cpu().numpy().tobytes() == want, s_in
        assert st.value == plan[2 + s_in], (s_in, st.value, plan)
    codec.close()


# ---- context teardown -----------------------------------------------------------------------------
def _grow_every_workspace(torch, codec, x, out):
    """one call of each family that grows a workspace of the context, on the 8 MiB input x"""
    enc = codec.encode(x, sync_syms=64)
    codec.decode_into(enc, out)
    codec.decode_ranges(enc, [0, 1 << 20], [4096, 4096])
    codec.decode_batch(codec.encode_blocks(x, 65536))
    codec.nyb_decompress(codec.nyb_compress(x, True), True)
    codec.small_decompress(codec.small_compress(x))
    codec.nyb_compress_chunked(x, True)
    codec.crc32(x)
    codec.sync()


def test_close_returns_the_workspace(torch_cuda):
    """Free device memory after 16 cycles of create / grow every workspace on 8 MiB / close is
    lower than at the start by less than twice what one live context takes (16 leaked contexts
    would take 16 times that). This only catches buffers that scale with the input: the fixed
    allocations of a context are smaller than the granularity of the device's free-memory figure.
    A first cycle before the measurement leaves torch's caching allocator holding the tensors the
    calls allocate, so the later cycles take no new device memory through torch. (About 7 s on an
    MI355X: 0.4 s of each cycle is the adaptive nybble decode of 8 MiB, whose resolve is one wave.)"""
    from data_compression_amd.device import Codec
    torch = torch_cuda
    n = 8 << 20
    text = torch.from_numpy(np.frombuffer(TEXT, np.uint8).copy()).cuda()
    x = text.repeat(n // text.numel() + 1)[:n].contiguous()
    out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    warm = Codec(0)
    _grow_every_workspace(torch, warm, x, out)
    warm.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    live = None
    for cycle in range(16):
        codec = Codec(0)
        _grow_every_workspace(torch, codec, x, out)
        if cycle == 0:
            live = free0 - torch.cuda.mem_get_info()[0]
        codec.close()
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info()[0]
    print("one live context: %d bytes; lost after 16 cycles: %d bytes" % (live, lost))
    assert live >= n, "a live context holds less than its 8 MiB rank buffer: nothing is measured"
    assert lost < 2 * live, (lost, live)
