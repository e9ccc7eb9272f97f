"""The batched Huffman codec (dc_gpu.h "Huffman batch v1") without a device: the two bound
functions (pure host arithmetic, csrc/dc_batch_bound.h), and the expected batch built from the
CPU oracle alone. SEGMENTS and oracle_batch are shared with tests/test_gpu_batch.py."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc

SEG_MAX = 65536
LENGTHS = (0, 1, 2, 15, 16, 17, 255, 256, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536)
KINDS = ("enwik", "zipf", "one", "cycle", "random")


def content(kind, n, seed):
    from data_compression_amd import synth
    if n == 0:
        return np.zeros(0, np.uint8)
    if kind == "enwik":
        return synth.enwik_like(n, seed=seed)
    if kind == "zipf":
        return synth.zipf_bytes(n, seed=seed)
    if kind == "one":
        return np.full(n, 0x41 + seed % 7, np.uint8)
    if kind == "cycle":   # all 256 values in turn: a flat histogram
        return (np.arange(n) % 256).astype(np.uint8)
    return np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)


def _segments():
    segs = [content(KINDS[j % len(KINDS)], n, 11 + j) for j, n in enumerate(LENGTHS)]
    # the three mode cases of the issue, whatever the cycle above gave those lengths
    segs += [content("one", 65536, 3), content("cycle", 65536, 0), content("random", 4096, 0),
             content("enwik", 65536, 5), content("zipf", 4097, 6)]
    return segs


SEGMENTS = _segments()


def pack_offsets(segs):
    """The segments back to back (most offsets odd): (bytes, int64 offsets of count + 1)."""
    off = np.zeros(len(segs) + 1, np.int64)
    off[1:] = np.cumsum([s.size for s in segs])
    return (np.concatenate(segs) if segs else np.zeros(0, np.uint8)), off


def oracle_segment(seg, n_ary, S):
    """(lens u8[256], mode, bits, payload bytes, sync_len u16) of one segment."""
    h = orc.histogram(seg)
    L = orc.huffman_lengths(h, n_ary)[:256] if seg.size else np.zeros(256, np.int32)
    assert L.max(initial=0) <= 255
    el, ev = orc.canonical(L, n_ary)
    code, nb, mx = orc.bitcodes(el, ev, n_ary)
    nch = (seg.size + S - 1) // S
    cbits = int((h * nb.astype(np.uint64)).sum())
    if seg.size and mx <= 32 and cbits < 8 * seg.size:
        payload, bits, idx = orc.huff_pack(seg, code, nb, 0, S)
        assert bits == cbits
        sl = np.diff(np.append(idx, np.uint64(bits))).astype(np.uint16)
        return L.astype(np.uint8), 1, bits, payload, sl
    sl = np.array([8 * min(S, seg.size - c * S) for c in range(nch)], np.uint16)
    return L.astype(np.uint8), 0, 8 * seg.size, seg, sl


def _oracle_batch(segs, n_ary, S):
    lens = np.zeros((len(segs), 256), np.uint8)
    mode = np.zeros(len(segs), np.uint8)
    bits = np.zeros(len(segs), np.int64)
    pay_off = np.zeros(len(segs) + 1, np.int64)
    sync_off = np.zeros(len(segs) + 1, np.int64)
    pay, sync = [], []
    for i, seg in enumerate(segs):
        lens[i], mode[i], bits[i], p, sl = oracle_segment(seg, n_ary, S)
        nbytes = (int(bits[i]) + 7) // 8
        assert p.size == nbytes and sl.size == (seg.size + S - 1) // S
        padded = np.zeros((nbytes + 15) // 16 * 16, np.uint8)   # the pad bytes are zero
        padded[:nbytes] = p
        pay.append(padded)
        sync.append(sl)
        pay_off[i + 1] = pay_off[i] + padded.size
        sync_off[i + 1] = sync_off[i] + sl.size
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return {"lens": lens, "mode": mode, "bits": bits, "pay_off": pay_off, "payload": cat(pay, np.uint8),
            "sync_off": sync_off, "sync_len": cat(sync, np.uint16)}


@functools.lru_cache(maxsize=None)
def _oracle_segments(n_ary, S):
    return _oracle_batch(SEGMENTS, n_ary, S)


def oracle_batch(segs, n_ary, S):
    """The expected lens / mode / bits / pay_off / payload / sync_off / sync_len of a batch, from
    oracle.oracle alone. The batch of SEGMENTS is computed once per (n_ary, S): do not modify."""
    return _oracle_segments(n_ary, S) if segs is SEGMENTS else _oracle_batch(segs, n_ary, S)


@pytest.mark.parametrize("S", (16, 64, 1024))
@pytest.mark.parametrize("count", (0, 1, 300))
@pytest.mark.parametrize("total", (0, 1, 65536, 2**33 + 5))
def test_bounds_are_their_formulas(total, count, S):
    from data_compression_amd._lib import core
    L = core()
    assert L.dc_huff_batch_payload_bound(total, count) == total + 16 * count
    assert L.dc_huff_batch_sync_bound(total, count, S) == -(-total // S) + count


def test_bounds_hold_the_oracle_batch():
    from data_compression_amd._lib import core
    L = core()
    _, off = pack_offsets(SEGMENTS)
    for n_ary, S in ((2, 64), (2, 16), (17, 64)):
        b = oracle_batch(SEGMENTS, n_ary, S)
        assert b["pay_off"][-1] <= L.dc_huff_batch_payload_bound(int(off[-1]), len(SEGMENTS))
        assert b["sync_off"][-1] <= L.dc_huff_batch_sync_bound(int(off[-1]), len(SEGMENTS), S)
        assert (b["pay_off"] % 16 == 0).all()


def test_segments_cover_the_lengths_and_kinds():
    assert sorted({s.size for s in SEGMENTS}) == list(LENGTHS)
    assert all(s.size <= SEG_MAX for s in SEGMENTS)
    _, off = pack_offsets(SEGMENTS)
    assert (off[1:-1] % 2 == 1).sum() >= len(SEGMENTS) // 2   # packed back to back: odd offsets


def test_oracle_puts_the_mode_cases_on_their_sides():
    flat = content("cycle", 65536, 0)
    _, mode, bits, _, _ = oracle_segment(flat, 2, 64)
    L = orc.huffman_lengths(orc.histogram(flat), 2)
    code, nb, _ = orc.bitcodes(*orc.canonical(L, 2), 2)
    assert int(nb.astype(np.int64).sum()) * 256 == 524544   # coded it would take 524544 > 524288 bits
    assert (mode, bits) == (0, 524288)
    rnd = np.random.default_rng(1).integers(0, 256, 4096, dtype=np.uint8)
    _, mode, bits, _, _ = oracle_segment(rnd, 2, 64)
    assert (mode, bits) == (1, 32712)                         # against 32768: Huffman, barely
    one = content("one", 65536, 3)
    lens, mode, bits, _, sl = oracle_segment(one, 2, 64)
    assert (mode, bits, int(lens[one[0]])) == (1, 65536, 1) and (sl == 64).all()
    _, mode, bits, p, sl = oracle_segment(np.zeros(0, np.uint8), 2, 64)
    assert (mode, bits, p.size, sl.size) == (0, 0, 0, 0)      # length 0: stored with 0 bytes
