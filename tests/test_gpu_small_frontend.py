"""The stand-alone small front-end kernels (k_small_tiles<M>, k_small_write<M> of dc_core.hip,
in their five modes) against the plain model of tests/small_frontend_model.py, byte for byte,
at the kernels' own edges. Every cut these kernels make (dword, uint4, lane, wave quarter, step,
wave, tile) lies on the 16-byte address grid of element 0, so every case runs with the input at
each of the 16 alignments (a view buf[lead: lead + n] of a larger buffer) and the output at
offsets 0, 1, 5, 15 of a buffer filled with 0xEE, of which every byte before the output and
from the returned length on must stay 0xEE. The encoders' inputs carry each case of
small_frontend_model.CASES on each edge, placed from the input's address; the decoders get the
model's streams of those inputs and arbitrary bodies. The *_reaches_* tests assert, from the
inputs and pointers, that the edges, the v_perm patterns and both tile paths are reached.

Encode capacity is n + 1, decode capacity 2 m. The 1024-tile group edge of k_fsm_scan_up stays
with the full-size tests.
"""
import ctypes as C

import numpy as np
import pytest

from tests import small_frontend_model as fm
from tests.small_frontend_model import fe_body, fe_stream, fe_unbody, fe_unstream

pytestmark = pytest.mark.gpu

LEADS = range(16)
OUT_OFFSETS = (0, 1, 5, 15)
FILL = 0xEE
ENCODERS = ("ENC", "BODY0", "BODY1")
DECODERS = ("DEC", "DBODY")
DC_E_STATE = -5


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


def _place(torch, lead, n, make, before=0x20, after=0x61):
    """make(address) -> n bytes, put at buf[lead: lead + n] of a 16-byte aligned device buffer;
    the bytes around them would pair with the stream's ends if a kernel used them."""
    buf = torch.empty(lead + n + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    x = np.asarray(make(buf.data_ptr() + lead), np.uint8)
    assert x.size == n
    host = np.concatenate([np.full(lead, before, np.uint8), x, np.full(64, after, np.uint8)])
    buf.copy_(torch.from_numpy(host))
    return buf[lead: lead + n], x.tobytes()


def _place_dec(torch, lead, c):
    a = np.frombuffer(c, np.uint8)
    return _place(torch, lead, a.size, lambda addr: a, before=0xE1, after=0xE1)[0]


class _Out:
    """cap bytes at offset off of a buffer of 0xEE"""

    def __init__(self, torch, cap, off):
        self.off = off
        self.buf = torch.full((off + cap + 64,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[off: off + cap]

    def taken(self, n):
        h = self.buf.cpu().numpy()
        assert n <= self.view.numel()
        assert (h[: self.off] == FILL).all(), "bytes before the output were written"
        assert (h[self.off + n:] == FILL).all(), "bytes from the returned length on were written"
        return h[self.off: self.off + n].tobytes()


def _run(torch, codec, mode, x, out_off, nelem=None):
    from data_compression_amd._lib import check
    n = x.numel()
    if mode == "ENC":
        o = _Out(torch, n + 1, out_off)
        ln = C.c_uint64(0)
        check("dc_small_compress", codec.L.dc_small_compress(codec.ctx, x.data_ptr(), n, o.view.data_ptr(), C.byref(ln)))
        return o.taken(ln.value)
    if mode in ("BODY0", "BODY1"):
        o = _Out(torch, n + 1, out_off)
        return o.taken(codec.small_body(x, mode == "BODY1", nelem, out=o.view).numel())
    o = _Out(torch, 2 * n, out_off)
    f = codec.small_decompress if mode == "DEC" else codec.small_decompress_body
    return o.taken(f(x, out=o.view).numel())


def _want(mode, x, nelem=None):
    if mode == "ENC":
        return fe_stream(x)
    if mode in ("BODY0", "BODY1"):
        return fe_body(x, mode == "BODY1", nelem)
    return fe_unstream(x) if mode == "DEC" else fe_unbody(x)


def _nelems(mode, n):
    """ENC: the call has none. A body: without and with a right halo."""
    if mode == "ENC":
        return [None]
    return [k for k in (n - 1, n - 2) if k >= 0]


@pytest.fixture(scope="module")
def planted_dev(torch_cuda):
    """(case, lead) -> (device view, bytes, sites), built from the view's address"""
    out = {}
    for lead in LEADS:
        for case in fm.CASES:
            sites = []

            def make(addr):
                x, s = fm.planted(case, addr)
                sites.extend(s)
                return x
            v, x = _place(torch_cuda, lead, fm.ENC_N, make)
            out[case, lead] = (v, x, sites)
    return out


# ---- the encoders ------------------------------------------------------------------------------
def test_planted_inputs_reach_every_edge_and_both_tile_paths(planted_dev):
    """100 % of (mode, alignment, case, edge): the case's bytes are in the input with the edge
    byte on a multiple of the edge width from the granule of element 0, computed here from
    data_ptr(); and for every edge one site lies in a tile that takes the interior path and one
    in a tile that does not."""
    n = fm.ENC_N
    reached = 0
    for mode in ENCODERS:
        for nelem in _nelems(mode, n):
            for (case, lead), (v, x, sites) in planted_dev.items():
                ptr = v.data_ptr()
                assert ptr % 16 == lead
                g0 = (ptr + 1) & ~15                      # the granule of element 0 (stream byte 1)
                T = fm.tiles(ptr, 1, nelem if nelem is not None else n - 1, n, fm.ENC_TILE)
                assert len(T) == 3 and [t["interior"] for t in T] == [False, True, False]
                seq, k = fm.CASES[case]
                for name, E in fm.ENC_EDGES.items():
                    paths = set()
                    for nm, u, e in sites:
                        if nm != name:
                            continue
                        assert (ptr + e - g0) % E == 0 and ptr + e - g0 == u
                        assert x[e - k: e - k + len(seq)] == seq
                        paths |= {T[(u - 1) // fm.ENC_TILE]["interior"], T[u // fm.ENC_TILE]["interior"]}
                    assert paths == {True, False}, (mode, lead, case, name)
                    reached += nelem in (None, n - 1)
    assert reached == len(ENCODERS) * 16 * len(fm.CASES) * len(fm.ENC_EDGES)
    # the planted inputs are far from LITERAL; test_literal_threshold is at it
    assert all(fe_stream(x)[0] == 8 for _, x, _ in planted_dev.values())


@pytest.mark.parametrize("mode", ENCODERS)
def test_planted_edges(torch_cuda, codec, planted_dev, mode):
    bad = []
    for i, ((case, lead), (v, x, _)) in enumerate(planted_dev.items()):
        for j, nelem in enumerate(_nelems(mode, fm.ENC_N)):
            want = _want(mode, x, nelem)
            # every output offset without a right halo; one of them, in turn, with it
            for off in (OUT_OFFSETS if j == 0 else (OUT_OFFSETS[(i + lead) % 4],)):
                got = _run(torch_cuda, codec, mode, v, off, nelem)
                if got != want:
                    d = next((p for p in range(min(len(got), len(want))) if got[p] != want[p]), -1)
                    bad.append((case, lead, nelem, off, len(got), len(want), d))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("mode", ENCODERS + DECODERS)
def test_short_lengths(torch_cuda, codec, mode):
    """n = 1 .. 80 at every alignment (the output offsets in turn)."""
    src = {"DEC": fm.SHORT_STREAM, "DBODY": fm.SHORT_BODY}.get(mode, fm.SHORT)
    bad = []
    for lead in LEADS:
        pad = (0xE1, 0xE1) if mode in DECODERS else (0x20, 0x61)
        whole, _ = _place(torch_cuda, lead, src.size, lambda addr: src, *pad)
        for n in range(1, 81):
            v, x = whole[:n], src[:n].tobytes()
            for nelem in (_nelems(mode, n) if mode in ENCODERS else [None]):
                off = OUT_OFFSETS[(n + lead) % 4]
                got = _run(torch_cuda, codec, mode, v, off, nelem)
                if got != _want(mode, x, nelem):
                    bad.append((lead, n, nelem, off))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("mode", ENCODERS + DECODERS)
def test_lengths_around_the_tiles(torch_cuda, codec, mode):
    """tile - 2 .. tile + 2 and 2 tile - 2 .. 2 tile + 2 at every alignment: with the lead, the
    last tile ends anywhere from 2 bytes short of a tile to 17 bytes into the next."""
    src = {"DEC": fm.AROUND_STREAM, "DBODY": fm.AROUND_BODY}.get(mode, fm.AROUND)
    tile = fm.MODES[mode][1]
    want = {}
    bad = []
    for lead in LEADS:
        pad = (0xE1, 0xE1) if mode in DECODERS else (0x20, 0x61)
        whole, _ = _place(torch_cuda, lead, src.size, lambda addr: src, *pad)
        for n in fm.around_tiles(tile):
            for nelem in (_nelems(mode, n) if mode in ENCODERS else [None]):
                if (n, nelem) not in want:
                    want[n, nelem] = _want(mode, src[:n].tobytes(), nelem)
                off = OUT_OFFSETS[(n + lead) % 4]
                got = _run(torch_cuda, codec, mode, whole[:n], off, nelem)
                if got != want[n, nelem]:
                    bad.append((lead, n, nelem, off, len(got), len(want[n, nelem])))
    assert not bad, (len(bad), bad[:8])


def test_stream_ends(torch_cuda, codec):
    """Stream bytes 0-1 never pair (ENC, BODY0) but bytes 1-2 do; a last ' ' stays; a body pairs
    across its end only into a right halo; BODY1's left halo ' ' closes a pair with byte 1. The
    expected bytes are written out by hand in small_frontend_model.STREAM_ENDS."""
    bad = []
    for k, (name, (mode, x, nelem, want)) in enumerate(fm.STREAM_ENDS.items()):
        a = np.frombuffer(x, np.uint8)
        for lead in LEADS:
            v, _ = _place(torch_cuda, lead, a.size, lambda addr: a)
            got = _run(torch_cuda, codec, mode, v, OUT_OFFSETS[(k + lead) % 4], nelem)
            if got != want:
                bad.append((name, lead, got))
    assert not bad, (len(bad), bad[:8])


def test_literal_threshold(torch_cuda, codec):
    """0, 1 and 2 pairs at n = 2, 3, 17, one tile and one tile plus 1: output n + 1 - pairs >= n
    is LITERAL, ' ' + the input (the writer's grid-stride copy), at every alignment; 2 pairs are
    type 8. Each stream decodes back."""
    cases = fm.literal_inputs()
    assert {p for _, p, _ in cases} == {0, 1, 2} and {n for n, _, _ in cases} == set(fm.LITERAL_N)
    bad = []
    for n, pairs, x in cases:
        xb = x.tobytes()
        want = fe_stream(xb)
        assert (want == b" " + xb) if pairs <= 1 else (want[0] == 8 and len(want) == n - 1)
        for lead in LEADS:
            v, _ = _place(torch_cuda, lead, n, lambda addr: x)
            for off in OUT_OFFSETS:
                if _run(torch_cuda, codec, "ENC", v, off) != want:
                    bad.append(("enc", n, pairs, lead, off))
            c = _place_dec(torch_cuda, lead, want)
            if _run(torch_cuda, codec, "DEC", c, OUT_OFFSETS[lead % 4]) != xb:
                bad.append(("dec", n, pairs, lead))
    assert not bad, (len(bad), bad[:8])


# ---- the decoders -------------------------------------------------------------------------------
def _dec_inputs():
    """name -> type-8 stream (DEC takes it whole, DBODY its body): the model's streams of the
    planted inputs, and the arbitrary bodies behind a header"""
    out = {case: fe_stream(fm.planted(case, 0)[0].tobytes()) for case in fm.CASES}
    out.update({k: bytes([8, 0x41]) + b.tobytes() for k, b in fm.dec_bodies().items()})
    assert all(c[0] == 8 and 2 * fm.DEC_TILE + 1000 < len(c) < 4 * fm.DEC_TILE for c in out.values())
    return out


def test_decode_inputs_reach_every_pattern_and_both_tile_paths(torch_cuda):
    """From the pointers: in the interior tiles of the uniform body every one of the 16 patterns
    of bytes >= 0x80 in a dword occurs at each of the 4 byte phases of the output position, and
    some dword takes nt > 32 (phase + 4 + its bytes >= 0x80 > 8 output bytes pending); the first
    and last tiles, which take the per-byte path, are dense in bytes >= 0x80 too."""
    body = fm.dec_bodies()["uniform"]
    dense = fm.dec_bodies()["all_high"]
    assert (dense >= 0x80).all() and not (fm.dec_bodies()["none_high"] >= 0x80).any()
    for mode in DECODERS:
        c = (bytes([8, 0x41]) if mode == "DEC" else b"") + body.tobytes()
        off0, tile = fm.MODES[mode]
        for lead in LEADS:
            v = _place_dec(torch_cuda, lead, c)
            T = fm.tiles(v.data_ptr(), off0, len(c) - off0, len(c), tile)
            # (a type-8 stream whose byte 2 is on the grid has no partial first tile)
            whole_first = mode == "DEC" and (v.data_ptr() + 2) % 16 == 0
            assert [t["interior"] for t in T] == [whole_first, True, True, False]
            assert all(t["hi"] - t["lo"] > 900 for t in T)   # the per-byte tiles hold elements
            for off in OUT_OFFSETS:
                o = _Out(torch_cuda, 2 * len(c), off)
                pat, ph = fm.dec_interior_dwords(c, v.data_ptr(), mode, o.view.data_ptr())
                assert pat.size == (2 + whole_first) * tile // 4
                assert len(set(zip(pat.tolist(), ph.tolist()))) == 64, (mode, lead, off)
                nt = 8 * ph + 8 * np.array([bin(p).count("1") for p in pat])
                assert (nt > 32).any() and (nt == 32).any() and (nt < 32).any()


@pytest.mark.parametrize("mode", DECODERS)
def test_decode_streams_and_bodies(torch_cuda, codec, mode):
    bad = []
    for name, c in _dec_inputs().items():
        c = c if mode == "DEC" else c[2:]
        want = _want(mode, c)
        if name == "all_high":
            assert len(want) == 2 * len(c) - (3 if mode == "DEC" else 0)   # the capacity, but for the header
        for lead in LEADS:
            v = _place_dec(torch_cuda, lead, c)
            for off in OUT_OFFSETS:
                got = _run(torch_cuda, codec, mode, v, off)
                if got != want:
                    d = next((p for p in range(min(len(got), len(want))) if got[p] != want[p]), -1)
                    bad.append((name, lead, off, len(got), len(want), d))
    assert not bad, (len(bad), bad[:8])


def test_decode_headers_and_types(torch_cuda, codec):
    """in[1] is copied raw whatever it is; m = 1, 2, 3 of type 8; type ' ' with m = 1 and more;
    any other type byte is invalid and gives an empty result (small_compression.c:495-503)."""
    big = fm.text(20000, seed=0x59).tobytes()
    cases = [(bytes([8]), b""), (bytes([8, 0xE1]), b"\xe1"), (bytes([8, 0x41, 0xE1]), b"A a"),
             (bytes([8, 0xE1, 0x41, 0xE2]), b"\xe1A b"), (bytes([8, 0xFF, 0x80, 0xFF]), b"\xff \x00 \x7f"),
             (b" ", b""), (b" abc", b"abc"), (b" " + big, big),
             (b"Axyz", b""), (b"\x00", b""), (b"\x09\xe1\xe1", b""), (b"\xaf" + big[:300], b"")]
    bad = []
    for k, (c, want) in enumerate(cases):
        assert fe_unstream(c) == want
        for lead in LEADS:
            v = _place_dec(torch_cuda, lead, c)
            got = _run(torch_cuda, codec, "DEC", v, OUT_OFFSETS[(k + lead) % 4])
            if got != want:
                bad.append((c[:4], lead, len(got), len(want)))
    assert not bad, (len(bad), bad[:8])


# ---- plan and write, one context, the counted decode -------------------------------------------
def test_plan_then_write(torch_cuda, codec):
    from data_compression_amd._lib import DcError
    torch = torch_cuda
    n = fm.ENC_N
    y, x = _place(torch, 3, n, lambda addr: fm.planted("repeated_pairs", addr)[0])
    y2, _ = _place(torch, 3, n, lambda addr: fm.planted("repeated_pairs", addr)[0])
    for left in (False, True):
        for nelem in (n - 1, n - 2, 1000, 1):
            want = fe_body(x, left, nelem)
            assert codec.small_body_plan(y, left, nelem) == len(want)
            o = _Out(torch, nelem + 7, 5)
            got = codec.small_body_write(y, left, nelem, o.view, head=b"HD")
            assert o.taken(got.numel()) == b"HD" + want
            assert codec.small_body(y, left, nelem).cpu().numpy().tobytes() == want

    out = torch.empty(n + 1, dtype=torch.uint8, device="cuda")

    def state_error(plan, write):
        codec.small_body_plan(*plan)
        with pytest.raises(DcError) as e:
            codec.small_body_write(*write, out)
        assert e.value.rc == DC_E_STATE

    state_error((y, False, n - 2), (y, False, n - 3))    # another nelem
    state_error((y, False, n - 2), (y, True, n - 2))     # another left_halo
    state_error((y, True, n - 2), (y, False, n - 2))
    state_error((y, False, n - 2), (y2, False, n - 2))   # another input
    codec.small_body_plan(y, True, n - 2)
    assert codec.small_body_write(y, True, n - 2, out).cpu().numpy().tobytes() == fe_body(x, True, n - 2)
    with pytest.raises(DcError) as e:                    # a second write without a new plan
        codec.small_body_write(y, True, n - 2, out)
    assert e.value.rc == DC_E_STATE
    codec.small_body(y, False, n - 2)                    # a whole body call is no plan either
    with pytest.raises(DcError) as e:
        codec.small_body_write(y, False, n - 2, out)
    assert e.value.rc == DC_E_STATE


def test_one_context_mixed(torch_cuda):
    """Encode, body, decode, then an encode of another size on one context: each equals the result
    of a fresh context and the model (stale ws.summ, ws.entry or d_meta would show)."""
    from data_compression_amd.device import Codec
    torch = torch_cuda
    big, xb = _place(torch, 7, fm.ENC_N, lambda addr: fm.planted("pair_straddles_edge", addr)[0])
    c_uni = bytes([8, 0x41]) + fm.dec_bodies()["uniform"].tobytes()
    small = fm.text(5000, seed=0x56)
    steps = [("ENC", big, xb, None),
             ("BODY1", big[:71], xb[:71], 69),
             ("DEC", _place_dec(torch, 2, c_uni), c_uni, None),
             ("ENC", _place(torch, 9, small.size, lambda addr: small)[0], small.tobytes(), None),
             ("DBODY", _place_dec(torch, 11, c_uni[2:302]), c_uni[2:302], None),
             ("DEC", _place_dec(torch, 0, bytes([8, 0x41, 0xE1])), bytes([8, 0x41, 0xE1]), None),
             ("BODY0", big, xb, fm.ENC_N - 2)]
    one = Codec(0)
    for k, (mode, v, x, nelem) in enumerate(steps):
        want = _want(mode, x, nelem)
        assert _run(torch, one, mode, v, OUT_OFFSETS[k % 4], nelem) == want, (k, mode, "shared context")
        fresh = Codec(0)
        assert _run(torch, fresh, mode, v, OUT_OFFSETS[k % 4], nelem) == want, (k, mode, "fresh context")
        fresh.close()
    one.close()


def test_counted_decode(torch_cuda, codec):
    """dc_small_huff_decode takes the tile totals from the Huffman decoder's per-group counts
    (k_small_dec_summ) instead of the counting pass: on a planted input whose front-end stream is
    more than one 8 KiB tile it must give what the model and small_decompress of the same M give."""
    torch = torch_cuda
    x = fm.planted("repeated_pairs", 0)[0]
    M = fe_stream(x.tobytes())
    assert M[0] == 8 and len(M) > 2 * fm.DEC_TILE
    xt = torch.from_numpy(x.copy()).cuda()
    enc = codec.small_huff_encode(xt, n_ary=16, sync_syms=64)
    assert enc["n"] == len(M) and not hasattr(enc["bit_base"], "data_ptr")
    got = codec.small_huff_decode(enc)
    assert codec.decode_status() == 0
    m = torch.empty(len(M) + 16, dtype=torch.uint8, device="cuda")
    codec.decode_into(enc, m)
    assert m[: len(M)].cpu().numpy().tobytes() == M
    two = codec.small_decompress(m[: len(M)])
    want = fe_unstream(M)
    assert got.cpu().numpy().tobytes() == want
    assert two.cpu().numpy().tobytes() == want
