"""The bitstream (k_huff_pack, k_huff_decode8, the general decoder, dec_tables_build) at the
arities no other test packs with: group sizes 6..8, 11..15 and 17..32 of the wave merge, the
one-thread merge (n > 32), and digits of w = 5..8 bits (n = 17..256) through the packed codes,
lim[], the decoder tables, decode_long and the exact redo. Bit-exact against the CPU oracle
(orc.huffman_lengths / canonical, pinned to the reference at these arities by
tests/test_oracle.py on tests/golden/huffman_wide.npz)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_gpu_bigcount import DTable   # the dc_dtable layout, one definition

pytestmark = pytest.mark.gpu

ARITIES = (6, 7, 8, 11, 12, 13, 15, 17, 24, 31, 32, 33, 64, 100, 128, 255, 256)


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
def inputs():
    """Text (codes of up to 20 bits here), all 256 byte values, a skewed input; then one
    byte, a partial sync chunk, and one byte into the second 32 KiB block."""
    from data_compression_amd import synth
    out = [("text", synth.enwik_like(100_003, seed=1)),
           ("all256", synth.uniform_bytes(100_003, seed=2, lo=0, hi=255)),
           ("zipf", synth.zipf_bytes(100_003, seed=3))]
    out += [(f"text-{n}", synth.enwik_like(n, seed=1)) for n in (1, 17, 32_769)]
    return out


def _oracle_encode(x, n):
    h = orc.histogram(x)
    L = orc.huffman_lengths(h, n)
    el, ev = orc.canonical(L, n)
    code, nb, mx = orc.bitcodes(el, ev, n)
    return L, el, ev, code, nb, mx


def _fields(tab):
    b = tab.cpu().numpy()
    return DTable.from_buffer_copy(b[: C.sizeof(DTable)].tobytes())


def _off(bit_base):
    return (bit_base >> 3) - ((bit_base >> 5) << 2)   # words start at stream word bit_base / 32


def _check_encode(torch, codec, name, x, n_ary, oracle, S, bit_base=0):
    """encode at bit_base against the oracle's stream; returns the encode."""
    L, el, ev, code, nb, mx = oracle
    payload, bits, idx = orc.huff_pack(x, code, nb, bit_base=bit_base, sync_syms=S)
    xt = torch.from_numpy(x).cuda()
    enc = codec.encode(xt, n_ary=n_ary, sync_syms=S, bit_base=bit_base)
    tag = (name, n_ary, S, bit_base)
    assert np.array_equal(enc["hist"].cpu().numpy().astype(np.uint64), orc.histogram(x)), tag
    assert enc["bits"] == bits, tag
    got = enc["words"].cpu().numpy().view(np.uint8)
    off = _off(bit_base)
    assert np.array_equal(got[off: off + len(payload)], payload), tag
    assert not got[:off].any(), tag
    base, lens = orc.sync_compact(idx, bit_base, bits)
    assert np.array_equal(enc["sync"][0].cpu().numpy().astype(np.uint64)[: len(base)], base), tag
    assert np.array_equal(enc["sync"][1].cpu().numpy().view(np.uint16)[: len(lens)], lens), tag
    return enc


def _check_decode(torch, codec, enc, x, tag):
    out = torch.empty(x.size + 16, dtype=torch.uint8, device="cuda")
    codec.decode_into(enc, out)
    assert codec.decode_status() == 0, tag
    assert np.array_equal(out[: x.size].cpu().numpy(), x), tag


@pytest.mark.parametrize("n_ary", ARITIES)
def test_stream_bit_exact_vs_oracle(torch_cuda, codec, inputs, n_ary):
    torch = torch_cuda
    for name, x in inputs:
        oracle = _oracle_encode(x, n_ary)
        L, el, ev, code, nb, mx = oracle
        assert 0 < mx <= 32, (name, n_ary, mx)
        tag = (name, n_ary)
        # S = 64: the fast decoder, then the general one on the same stream
        enc = _check_encode(torch, codec, name, x, n_ary, oracle, 64)
        _check_decode(torch, codec, enc, x, tag)
        codec.set_option("decode_general", 1)
        try:
            _check_decode(torch, codec, enc, x, tag + ("general",))
        finally:
            codec.set_option("decode_general", 0)
        # S = 256: the general decoder, spans outside the LDS stage
        enc = codec.encode(torch.from_numpy(x).cuda(), n_ary=n_ary, sync_syms=256)
        _check_decode(torch, codec, enc, x, tag + (256,))
        # the oracle's stream under a table made from the lengths alone: no device pack has
        # built the decoder tables for it
        payload, bits, idx = orc.huff_pack(x, code, nb, sync_syms=64)
        words = np.zeros((len(payload) + 3) // 4 + 32, np.uint32)
        words.view(np.uint8)[: len(payload)] = payload
        tab = codec.table_lengths(torch.from_numpy(L.astype(np.int32)).cuda(), n_ary)
        base, lens = orc.sync_compact(idx, 0, bits)
        sync = (torch.from_numpy(base.astype(np.int64)).cuda(), torch.from_numpy(lens.view(np.int16)).cuda())
        out = torch.empty(x.size, dtype=torch.uint8, device="cuda")
        codec.decode(torch.from_numpy(words.view(np.int32)).cuda(), 0, sync, 64, x.size, tab, out)
        assert codec.decode_status() == 0, tag + ("oracle stream",)
        assert np.array_equal(out.cpu().numpy(), x), tag + ("oracle stream",)
        if name == "text":   # a shard's stream at a global bit offset
            for bit_base in (77, (1 << 33) + 5):
                enc = _check_encode(torch, codec, name, x, n_ary, oracle, 64, bit_base=bit_base)
                _check_decode(torch, codec, enc, x, tag + (bit_base,))


def test_n256_all_bytes_takes_the_redo(torch_cuda, codec, inputs):
    """n = 256 on all 256 byte values: 255 dummies join the rarest byte under one node, so that
    byte's code is 16 bits and every other 8. A 16-bit code lies past the fast decoder's 15-bit
    table: its chunks take the exact redo (dc_gpu.h dc_huff_decode_redo_count)."""
    torch = torch_cuda
    x = dict(inputs)["all256"]
    oracle = _oracle_encode(x, 256)
    nb = oracle[4]
    assert set(np.unique(nb).tolist()) == {8, 16}
    enc = _check_encode(torch, codec, "all256", x, 256, oracle, 64)
    _check_decode(torch, codec, enc, x, "all256")
    assert codec.decode_redo_count() > 0


def test_n128_text_is_a_pure_7_bit_code(torch_cuda, codec, inputs):
    torch = torch_cuda
    x = dict(inputs)["text"]
    oracle = _oracle_encode(x, 128)
    enc = _check_encode(torch, codec, "text", x, 128, oracle, 64)
    nbits = np.frombuffer(bytes(_fields(enc["table"]).nbits), np.uint32)
    assert set(np.unique(nbits).tolist()) == {0, 7}
    assert enc["bits"] == 7 * x.size
    _check_decode(torch, codec, enc, x, "text")


@pytest.mark.parametrize("n_ary", [255, 256])
def test_fixed8_text_with_gaps(torch_cuda, codec, inputs, n_ary):
    """n = 255 / 256 on text: every present byte under the root, 8 bits each, the alphabet not
    one run (dc_dtable.fixed8 without the affine map): the byte maps at bit_base 0 and 384 redo
    nothing, the general kernels run at bit_base 8; all bit-exact."""
    torch = torch_cuda
    x = dict(inputs)["text"]
    oracle = _oracle_encode(x, n_ary)
    assert set(np.unique(oracle[4]).tolist()) == {0, 8}
    for bit_base in (0, 384, 8):
        enc = _check_encode(torch, codec, "text", x, n_ary, oracle, 64, bit_base=bit_base)
        assert _fields(enc["table"]).fixed8 == 1, (n_ary, bit_base)
        assert enc["bits"] == 8 * x.size, (n_ary, bit_base)
        _check_decode(torch, codec, enc, x, ("text", n_ary, bit_base))
        if bit_base % 128 == 0:
            assert codec.decode_redo_count() == 0, (n_ary, bit_base)


def test_container_roundtrip_at_wide_arities(torch_cuda):
    from data_compression_amd import huffman as H
    from data_compression_amd import synth
    for data in (b"", b"a", synth.enwik_like(70_000, seed=4).tobytes()):
        for n_ary in (17, 64, 256):
            assert H.decompress(H.compress(data, n_ary)) == data, (len(data), n_ary)


def _skewed(n):
    """Eight byte values, skewed: one digit each at n >= 9, so 5 bits a byte at n = 17 and 32,
    and the Huffman blocks (6-bit text characters, the table and the sync index) come out
    shorter than the raw block. At w >= 6 a code costs a text character or more per byte and
    the raw block always wins: test_container_roundtrip_at_wide_arities covers those."""
    rng = np.random.default_rng(17)
    return rng.choice(np.frombuffer(b"etaoin s", np.uint8), size=n,
                      p=[0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05]).tobytes()


@pytest.mark.parametrize("n_ary", [17, 32])
def test_container_huffman_segment_past_16(torch_cuda, n_ary):
    """The netstring container writes and reads a Huffman segment (#dc1, X, #dcidx, Z blocks)
    at arities past 16, not only the raw block."""
    from data_compression_amd import huffman as H
    data = _skewed(70_001)
    blob = H.compress(data, n_ary)
    assert blob[blob.index(b":") + 1:].startswith(b"\n#dc1 n=%d syms=%d " % (n_ary, len(data)))
    assert b"\nZ" in blob and len(blob) < len(data)
    assert H.decompress(blob) == data


def test_container_refuses_arity_257(torch_cuda):
    """A well-formed Huffman segment whose metadata says n = 257, one past what the table
    kernel takes: DC_E_STREAM from the container's own check, before any table is built."""
    from data_compression_amd import huffman as H
    from data_compression_amd._lib import DcError
    data = _skewed(70_001)
    blob = H.compress(data, 17)
    colon = blob.index(b":")
    ml = int(blob[:colon])
    meta = blob[colon + 1: colon + 1 + ml]
    assert meta.startswith(b"\n#dc1 n=17 ") and blob[colon + 1 + ml: colon + 2 + ml] == b","
    meta = meta.replace(b" n=17 ", b" n=257 ", 1)
    bad = b"%d:" % len(meta) + meta + blob[colon + 1 + ml:]
    with pytest.raises(DcError) as e:
        H.decompress(bad, len(data))
    assert e.value.rc == -7   # DC_E_STREAM
    assert H.decompress(blob, len(data)) == data   # the same context reads the valid one after it
