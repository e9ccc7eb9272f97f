"""The capped Huffman batch (dc_gpu.h: dc_huff_encode_batch_limit) and the nybble form of its lens
records without a device: the expected batch is tests/test_batch_cpu.py's with the lengths of
tests/huff_limit_model.py in place of the oracle's, and the nybble pack / unpack are numpy. The
facts the GPU cases rest on (which segment binds under which cap, which has no code, which turns
stored) are pinned here. CASES, CONFIGS, oracle_batch_limit, lens_pack and lens_unpack are shared
with tests/test_gpu_batch_limit.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import huff_limit_model as hm
from tests.test_batch_cpu import SEGMENTS, content, oracle_batch, oracle_segment

DC_E_CODE_TOO_LONG = -3


def _bytes_of(counts, seed):
    """A segment with exactly these byte counts (symbol i counts[i] times), shuffled."""
    seg = np.repeat(np.arange(len(counts), dtype=np.uint8), np.asarray(counts, np.int64))
    np.random.default_rng(seed).shuffle(seg)
    return seg


def _k200():
    """4096 bytes with 200 distinct values: each once, then 3896 drawn with p ~ 0.97^i."""
    rng = np.random.default_rng(3)
    p = 0.97 ** np.arange(200)
    seg = np.concatenate([np.arange(200), rng.choice(200, 3896, p=p / p.sum())]).astype(np.uint8)
    rng.shuffle(seg)
    return seg


HAND = {
    "depth9": _bytes_of(hm._depth_case(9), 1),       # 512 bytes
    "depth13": _bytes_of(hm._depth_case(13), 2),     # 8192
    "depth16": _bytes_of(hm._depth_case(16), 3),     # 65536
    "random4096": np.random.default_rng(1).integers(0, 256, 4096, dtype=np.uint8),
    "k200": _k200(),
    "fib17": _bytes_of(hm._fib(17), 4),              # 4180
    "enwik65536": content("enwik", 65536, 5),
    "enwik4096": content("enwik", 4096, 5),
}
# one batch for the GPU cases: SEGMENTS, then the hand cases (packed back to back: odd offsets)
CASES = SEGMENTS + list(HAND.values())
# (n_ary, max_digits) of the GPU cases
CONFIGS = ((2, 15), (2, 12), (2, 8), (2, 7), (3, 6), (4, 4), (16, 2), (16, 1))


def oracle_segment_limit(seg, n_ary, S, D):
    """oracle_segment under the table capped at D digits: (lens u8[256], mode, bits, payload bytes,
    sync_len u16). A segment with more distinct bytes than n^D codes is stored with zero lens."""
    h = orc.histogram(seg)
    L = hm.limit_lengths(h, n_ary, D)[0] if seg.size else np.zeros(259, np.int32)
    nch = (seg.size + S - 1) // S
    if L is not None:
        L = L[:256]
        assert L.max(initial=0) <= D
        code, nb, mx = orc.bitcodes(*orc.canonical(L, n_ary), n_ary)
        cbits = int((h * nb.astype(np.uint64)).sum())
        if seg.size and mx <= 32 and cbits < 8 * seg.size:
            payload, bits, idx = orc.huff_pack(seg, code, nb, 0, S)
            assert bits == cbits
            sl = np.diff(np.append(idx, np.uint64(bits))).astype(np.uint16)
            return L.astype(np.uint8), 1, bits, payload, sl
    else:
        L = np.zeros(256, np.int32)
    sl = np.array([8 * min(S, seg.size - c * S) for c in range(nch)], np.uint16)
    return L.astype(np.uint8), 0, 8 * seg.size, seg, sl


def _batch(segs, n_ary, S, D):
    lens = np.zeros((len(segs), 256), np.uint8)
    mode = np.zeros(len(segs), np.uint8)
    bits = np.zeros(len(segs), np.int64)
    pay_off = np.zeros(len(segs) + 1, np.int64)
    sync_off = np.zeros(len(segs) + 1, np.int64)
    pay, sync = [], []
    for i, seg in enumerate(segs):
        lens[i], mode[i], bits[i], p, sl = oracle_segment_limit(seg, n_ary, S, D)
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


_cache = {}


def oracle_batch_limit(segs, n_ary, S, D):
    """The expected arrays of dc_huff_encode_batch_limit, as oracle_batch gives the unlimited ones.
    The batch of CASES is computed once per (n_ary, S, D): do not modify."""
    if segs is not CASES:
        return _batch(segs, n_ary, S, D)
    key = (n_ary, S, D)
    if key not in _cache:
        _cache[key] = _batch(CASES, n_ary, S, D)
    return _cache[key]


def lens_pack(lens):
    """(lens4, status) of dc_huff_batch_lens_pack: byte j = lens[2j] << 4 | lens[2j + 1]; a record
    with a length above 15 is zeros and DC_E_CODE_TOO_LONG."""
    lens = np.asarray(lens, np.uint8).reshape(-1, 256)
    bad = (lens > 15).any(axis=1)
    out = ((lens[:, 0::2] << 4) | (lens[:, 1::2] & 15)).astype(np.uint8)
    out[bad] = 0
    return out, np.where(bad, DC_E_CODE_TOO_LONG, 0).astype(np.int32)


def lens_unpack(lens4):
    lens4 = np.asarray(lens4, np.uint8).reshape(-1, 128)
    out = np.zeros((lens4.shape[0], 256), np.uint8)
    out[:, 0::2] = lens4 >> 4
    out[:, 1::2] = lens4 & 15
    return out


def _rule(seg, n, D):
    """(lengths or None, info) of the model on a segment's histogram."""
    return hm.limit_lengths(orc.histogram(seg), n, D)


def _bits(seg, L, n):
    _, nb, _ = orc.bitcodes(*orc.canonical(L[:256], n), n)
    return int((orc.histogram(seg) * nb.astype(np.uint64)).sum())


def test_hand_segments_have_their_sizes():
    sizes = {k: v.size for k, v in HAND.items()}
    assert sizes == {"depth9": 512, "depth13": 8192, "depth16": 65536, "random4096": 4096, "k200": 4096, "fib17": 4180,
                     "enwik65536": 65536, "enwik4096": 4096}
    assert np.unique(HAND["k200"]).size == 200 and np.unique(HAND["random4096"]).size == 256


@pytest.mark.parametrize("name,D,natural,demotions,bits", [
    ("depth9", 8, 9, 1, 1024), ("depth13", 12, 13, 1, None), ("depth16", 15, 16, 1, 131072), ("depth16", 12, 16, 3, 131200)])
def test_depth_cases_bind(name, D, natural, demotions, bits):
    seg = HAND[name]
    L, info = _rule(seg, 2, D)
    assert (info["natural"], info["binding"], info["demotions"]) == (natural, True, demotions)
    assert L.max() == D
    if bits is not None:
        assert _bits(seg, L, 2) == bits
    lens, mode, b, _, _ = oracle_segment_limit(seg, 2, 64, D)
    assert mode == 1 and lens.max() == D and (bits is None or b == bits)
    if name == "depth9":   # the cap costs nothing there: 1024 bits either way
        assert oracle_segment(seg, 2, 64)[2] == 1024


def test_random_segment_turns_stored_under_8_bits():
    seg = HAND["random4096"]
    L, info = _rule(seg, 2, 8)
    assert info["natural"] == 10 and info["binding"] and (L[:256] == 8).all()
    assert _bits(seg, L, 2) == 32768
    lens, mode, bits, payload, _ = oracle_segment_limit(seg, 2, 64, 8)
    assert (mode, bits) == (0, 32768) and (lens == 8).all() and np.array_equal(payload, seg)
    assert oracle_segment(seg, 2, 64)[1:3] == (1, 32712)   # unlimited: coded, barely


def test_200_values_have_no_7_bit_code_and_a_binding_8_bit_one():
    seg = HAND["k200"]
    assert _rule(seg, 2, 7)[0] is None
    lens, mode, bits, payload, sl = oracle_segment_limit(seg, 2, 64, 7)
    assert (mode, bits) == (0, 8 * 4096) and not lens.any() and np.array_equal(payload, seg) and (sl == 512).all()
    assert oracle_segment(seg, 2, 64)[1] == 1
    L, info = _rule(seg, 2, 8)
    assert info["binding"] and L.max() == 8
    assert oracle_segment_limit(seg, 2, 64, 8)[1] == 1


@pytest.mark.parametrize("n,D,natural,binds", [(3, 6, 8, True), (4, 4, 6, True), (9, 2, 3, True), (16, 2, 2, False)])
def test_fibonacci_segment_at_other_arities(n, D, natural, binds):
    seg = HAND["fib17"]
    L, info = _rule(seg, n, D)
    assert (info["natural"], info["binding"]) == (natural, binds) and L.max() <= D
    assert oracle_segment_limit(seg, n, 64, D)[1] == 1


def test_fibonacci_segment_has_no_one_digit_code_at_16():
    seg = HAND["fib17"]
    assert _rule(seg, 16, 1)[0] is None   # 17 symbols, 16 codes
    lens, mode, _, _, _ = oracle_segment_limit(seg, 16, 64, 1)
    assert mode == 0 and not lens.any()


def test_text_segments():
    for D in (15, 12):
        _, info = _rule(HAND["enwik65536"], 2, D)
        assert info["natural"] == 16 and info["binding"]
    _, info = _rule(HAND["enwik4096"], 2, 12)
    assert info["natural"] == 12 and not info["binding"]


def test_how_many_segments_bind():
    def count(D):
        r = [_rule(s, 2, D) for s in SEGMENTS if s.size]
        return sum(info["binding"] for L, info in r if L is not None), sum(L is None for L, _ in r)
    assert len(SEGMENTS) == 21
    assert count(15) == (2, 0) and count(12) == (3, 0) and count(8)[0] == 11 and count(7)[1] == 8


def test_a_cap_that_never_binds_is_the_unlimited_batch():
    exp, cap = oracle_batch(SEGMENTS, 2, 64), _batch(SEGMENTS, 2, 64, 32)
    for k in exp:
        assert np.array_equal(exp[k], cap[k]), k


@pytest.mark.parametrize("n,D", CONFIGS)
def test_case_batch_has_both_modes_and_lengths_within_the_cap(n, D):
    b = oracle_batch_limit(CASES, n, 64, D)
    assert set(b["mode"].tolist()) == {0, 1} and b["lens"].max() <= D
    assert (b["pay_off"] % 16 == 0).all()


def test_nybble_records_round_trip():
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 16, (7, 256)).astype(np.uint8)
    l4, st = lens_pack(lens)
    assert l4.shape == (7, 128) and not st.any()
    assert l4[3, 0] == (int(lens[3, 0]) << 4 | int(lens[3, 1])) and l4[3, 127] == (int(lens[3, 254]) << 4 | int(lens[3, 255]))
    assert np.array_equal(lens_unpack(l4), lens)
    lens[2, 255] = 16
    l4, st = lens_pack(lens)
    assert st.tolist() == [0, 0, DC_E_CODE_TOO_LONG, 0, 0, 0, 0] and not l4[2].any() and l4[1].any() and l4[3].any()
    assert not lens_unpack(l4)[2].any()


@pytest.mark.parametrize("D,packs", [(15, True), (12, True), (0, False)])
def test_capped_records_always_pack(D, packs):
    """Uncapped, the 64 KiB text segment is 16 deep and has no nybble form; under 15 digits or
    fewer every record has one."""
    lens = oracle_batch_limit(CASES, 2, 64, D)["lens"] if D else oracle_batch(SEGMENTS, 2, 64)["lens"]
    assert (not lens_pack(lens)[1].any()) == packs
