"""The model of the small front-end (tests/small_frontend_model.py) pinned on the CPU: against
the oracle's sequential restatement of small_compression.c:507-665 on every input
test_gpu_small_frontend.py gives the kernels, against hand-written outputs at the stream's
ends, and against the reference's goldens; the LITERAL rule derived from the output length; the
shard bodies' concatenation; and the decoders' answer to an unknown type byte (empty, as
small_compression.c:495-503 leaves it).
"""
import itertools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import small_frontend_model as fm
from tests.small_frontend_model import fe_body, fe_pairs, fe_stream, fe_unbody, fe_unstream


def gpu_encode_inputs():
    """Every input test_gpu_small_frontend.py hands an encoder (the planted ones for each of the
    16 alignments: they are built from the input's address)."""
    for lead in range(16):
        for case in fm.CASES:
            yield fm.planted(case, lead)[0].tobytes()
    for n in range(1, 81):
        yield fm.SHORT[:n].tobytes()
    for n in fm.around_tiles(fm.ENC_TILE):
        yield fm.AROUND[:n].tobytes()
    for _, _, x in fm.literal_inputs():
        yield x.tobytes()
    for mode, x, _, _ in fm.STREAM_ENDS.values():
        yield x
    yield fm.text(5000, seed=0x56).tobytes()


def gpu_decode_streams():
    for case in fm.CASES:
        yield fe_stream(fm.planted(case, 0)[0].tobytes())
    for b in fm.dec_bodies().values():
        yield bytes([8, 0x41]) + b.tobytes()
    for m in range(1, 81):
        yield fm.SHORT_STREAM[:m].tobytes()
    for m in fm.around_tiles(fm.DEC_TILE):
        yield fm.AROUND_STREAM[:m].tobytes()
    for _, _, x in fm.literal_inputs():
        yield fe_stream(x.tobytes())
    yield from (bytes([8]), bytes([8, 0xE1]), bytes([8, 0x41, 0xE1]), bytes([8, 0xE1, 0x41, 0xE2]), b" ", b" abc")


def test_model_matches_the_oracle_on_every_gpu_input():
    k = 0
    for x in gpu_encode_inputs():
        assert fe_stream(x) == orc.small_compress(x), (k, len(x))
        k += 1
    assert k > 16 * len(fm.CASES) + 100


def test_model_matches_the_oracle_on_all_short_strings():
    alphabet = [ord(" "), ord("a"), ord("A"), 0x00, 0xE1]
    assert fe_stream(b"") == orc.small_compress(b"") == b" "
    for n in range(1, 7):
        for t in itertools.product(alphabet, repeat=n):
            x = bytes(t)
            assert fe_stream(x) == orc.small_compress(x), x


def test_inverse_matches_the_oracle():
    k = 0
    for c in gpu_decode_streams():
        assert c[0] in (8, 32)
        assert fe_unstream(c) == orc.small_decompress(c), (k, len(c))
        k += 1
    assert fe_unstream(b"") == orc.small_decompress(b"") == b""
    for m, want in ((1, b""), (2, b"\xe1"), (3, b"\xe1 a")):   # type 8: m = 1, 2, 3
        c = bytes([8, 0xE1, 0xE1])[:m]
        assert fe_unstream(c) == orc.small_decompress(c) == want
    assert fe_unbody(bytes([0x41, 0x80, 0xFF, 0xE1])) == b"A \x00 \x7f a"


def test_model_and_oracle_decode_every_golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "small.npz"))
    kinds = set()
    for i in range(int(d["n_inputs"][0])):
        x, c = d[f"in_{i}"].tobytes(), d[f"comp_{i}"].tobytes()
        assert fe_stream(x) == c
        assert fe_unstream(c) == orc.small_decompress(c) == x   # the LITERAL ones too
        kinds.add(c[0])
    assert kinds == {8, 32}


def test_stream_ends_by_hand():
    for name, (mode, x, nelem, want) in fm.STREAM_ENDS.items():
        if mode == "ENC":
            assert fe_stream(x) == want == orc.small_compress(x), name
        else:
            assert fe_body(x, mode == "BODY1", nelem) == want, name


@pytest.mark.parametrize("n", [5, 6, 17, 100, fm.ENC_TILE, fm.ENC_TILE + 1])
def test_literal_rule(n):
    """The type-8 stream is 2 + (n - 1) - pairs = n + 1 - pairs bytes and LITERAL is taken when
    that is >= n (:651): exactly when the input has at most one pair."""
    for pairs in (0, 1, 2):
        x = fm.with_pairs(n, pairs).tobytes()
        assert fe_pairs(x) == pairs
        c = fe_stream(x)
        assert c == orc.small_compress(x)
        if pairs <= 1:
            assert c == b" " + x
        else:
            assert c[0] == 8 and len(c) == n + 1 - pairs == n - 1
    for nn, p, x in fm.literal_inputs():
        assert fe_pairs(x.tobytes()) == p
        assert (fe_stream(x.tobytes())[0] == 32) == (p <= 1)
    assert {(nn, p) for nn, p, _ in fm.literal_inputs()} >= {(2, 0), (3, 0), (3, 1), (17, 2), (fm.ENC_TILE, 2),
                                                            (fm.ENC_TILE + 1, 1)}


def _shard_bodies(x, cuts):
    out = []
    for r in range(len(cuts) - 1):
        a, b = cuts[r], cuts[r + 1]
        last = b == len(x)
        if r == 0:
            y, nelem = x[: b + (0 if last else 1)], b - 1
        else:
            y, nelem = x[a - 1: b + (0 if last else 1)], b - a
        out.append(fe_body(y, r > 0, nelem))
    return out


def test_shard_bodies_concatenate():
    rng = np.random.default_rng(0x57)
    x = fm.text(4000, seed=0x58).tobytes()
    whole = fe_stream(x)
    assert whole[0] == 8
    sp = [i for i in range(2, len(x) - 1) if x[i] == 32 and 97 <= x[i + 1] <= 122]
    fixed = [[0, sp[0], len(x)], [0, sp[5] + 1, len(x)], [0, 2, 4, 6, len(x)], [0, sp[3], sp[3] + 2, len(x) - 2, len(x)]]
    rand = [[0] + sorted(set(2 * rng.integers(1, len(x) // 2 - 1, size=k))) + [len(x)] for k in (1, 2, 7, 40, 300)]
    for cuts in fixed + [[int(c) for c in r] for r in rand]:
        assert all(b - a >= 2 for a, b in zip(cuts, cuts[1:]))
        assert bytes([8, x[0]]) + b"".join(_shard_bodies(x, cuts)) == whole, cuts
    short = b"x a b c d"
    for c1 in range(2, len(short) - 1):
        assert bytes([8, short[0]]) + b"".join(_shard_bodies(short, [0, c1, len(short)])) == fe_stream(short)


def test_unknown_type_decodes_to_nothing():
    """small_compression.c:495-503: neither 8 nor ' ' is "invalid compressed data" and the output
    stays empty (the nybble decoder's copy rule, nybble_compression.c:806, is its own)."""
    import torch

    from tests.cpu_engine import CpuEngine
    for c in (b"Axyz", b"\x00", b"\x07 a", b"\x09\xe1\xe1", b"\xafabc", b"!" * 100):
        assert orc.small_decompress(c) == b""
        assert fe_unstream(c) == b""
        got = CpuEngine().small_decompress(torch.from_numpy(np.frombuffer(c, np.uint8).copy()))
        assert got.numel() == 0
    assert orc.nybble_decompress(b"Axyz", False) == b"Axyz"   # unchanged


def test_geometry_of_the_planted_inputs():
    """Every (edge, case) sits in a tile that takes the interior path and in one that does not,
    for every alignment, and the planted bytes are where the site says."""
    for lead in range(16):
        T = fm.tiles(lead, 1, fm.ENC_N - 1, fm.ENC_N, fm.ENC_TILE)
        assert [t["interior"] for t in T] == [False, True, False]
        sites = fm.enc_sites(lead)
        for name, E in fm.ENC_EDGES.items():
            mine = [(u, e) for nm, u, e in sites if nm == name]
            assert mine and all(u % E == 0 and e == u + fm.grid_origin(lead, 1) for u, e in mine)
            assert all((lead + e) % 16 == u % 16 for u, e in mine)   # on the address grid
            inside = {T[(u - d) // fm.ENC_TILE]["interior"] for u, _ in mine for d in (0, 1)}
            assert inside == {True, False}, (lead, name)
        for case, (seq, k) in fm.CASES.items():
            x, s2 = fm.planted(case, lead)
            assert s2 == tuple(sites)
            for _, _, e in sites:
                assert x[e - k: e - k + len(seq)].tobytes() == seq
