"""dc_huff_range_span (dc_host.h) through huffman.range_span: pure host arithmetic, no device.
The span it names for a symbol range, cut out of the oracle's stream bit for bit, is a
stream of its own from group g0 on: the oracle decodes the range's symbols from it."""
import numpy as np
import pytest

from oracle import oracle as orc

N = 100_003
SYNCS = (16, 64, 1024)


def range_list(n, S):
    """The symbol ranges of the range tests (tests/test_gpu_ranges.py uses the same list): the
    stream's ends, an empty range, ranges across a chunk and a group boundary, a whole group,
    one over three groups, and one range twice. A range that would pass n at this S is left out
    (at S = 1024 a group is 65536 symbols: the second group is partial)."""
    G = 64 * S
    rs = [(0, 1), (0, n), (n - 1, 1), (n - 17, 17), (5, 0), (70, 10), (S - 1, 2), (G - 1, 2), (G, G),
          (G // 2 + 3, 2 * G + 5), (70, 10)]
    return [(a, c) for a, c in rs if a + c <= n]


@pytest.fixture(scope="module")
def text():
    from data_compression_amd import synth
    x = synth.enwik_like(N, seed=1)
    L = orc.huffman_lengths(orc.histogram(x), 2)
    el, ev = orc.canonical(L, 2)
    code, nb, _ = orc.bitcodes(el, ev, 2)
    return x, el, ev, code, nb


@pytest.mark.parametrize("S", SYNCS)
def test_span_is_a_stream_of_its_own(text, S):
    from data_compression_amd import huffman as H
    x, el, ev, code, nb = text
    payload, bits, idx = orc.huff_pack(x, code, nb, sync_syms=S)
    base, lens = orc.sync_compact(idx, 0, bits)
    allbits = np.unpackbits(payload)
    G = 64 * S
    ranges = range_list(N, S)
    assert len(ranges) >= 9
    for first, count in ranges:
        g0, g1, b0, b1 = H.range_span(N, S, base, bits, first, count)
        tag = (S, first, count)
        assert g0 == first // G and g1 == (max(first + count, first + 1) - 1) // G, tag
        assert b0 == int(base[g0]), tag
        assert b1 == (int(base[g1 + 1]) if g1 + 1 < len(base) else bits), tag
        cut = np.packbits(allbits[b0:b1])
        need = first - g0 * G + count
        got = orc.huff_unpack(cut, b1 - b0, need, el, ev, 2)
        assert np.array_equal(got[need - count:], x[first: first + count]), tag


@pytest.mark.parametrize("S", SYNCS)
def test_span_past_the_end_is_an_argument_error(text, S):
    from data_compression_amd import huffman as H
    from data_compression_amd._lib import DcError
    x, el, ev, code, nb = text
    payload, bits, idx = orc.huff_pack(x, code, nb, sync_syms=S)
    base, _ = orc.sync_compact(idx, 0, bits)
    for first, count in ((N, 1), (0, N + 1), (N + 1, 0), (2**63, 2**63)):
        with pytest.raises(DcError) as e:
            H.range_span(N, S, base, bits, first, count)
        assert e.value.rc == -1, (first, count)
    with pytest.raises(DcError) as e:
        H.range_span(N, 48, base, bits, 0, 1)   # no power of two
    assert e.value.rc == -1
    assert H.range_span(N, S, base, bits, N, 0)[0] == (N - 1) // (64 * S)   # the empty range at the end
