"""The one decode body of the batch Huffman decoders (hb_decode_body, csrc/dc_batch_kernels.inc) seen
from both of its callers: Codec.decode_batch (whole segments: k_hb_decode, k_hbs_decode) and
Codec.decode_batch_ranges (byte ranges: k_hb_decode_ranges, k_hbs_decode_ranges). The two differ in
what they ask of a segment's `bits` record, and must agree on everything else. The batches are the
CPU oracle's, uploaded as they are; outputs are prefilled with 0xA5 and every byte nobody asked for
must keep it (helpers of tests/test_gpu_batch_ranges.py)."""
import numpy as np
import pytest

from tests.test_batch_cpu import SEGMENTS, content, oracle_batch
from tests.test_batch_shared_cpu import oracle_shared_batch, table_codes, text_table
from tests.test_gpu_batch_ranges import (DC_E_STREAM, FILL, MODES, STORED, B, _check, _dev, _enc, _gapped, _run, _upload,
                                         codec, torch_cuda)  # noqa: F401  (the two fixtures)

pytestmark = pytest.mark.gpu


def _pad16(nbytes):
    return (nbytes + 15) & ~15


def _whole(torch, codec, enc, segs, starts, cap):
    """ONE decode_batch of every segment to out[starts[i] ..) of a 0xA5 buffer, with a status array
    of its own (the uploaded one stays at -99 for the range calls): (bytes, status), host side."""
    enc = dict(enc, status=torch.full((len(segs),), -99, dtype=torch.int32, device="cuda"))
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    codec.decode_batch(enc, out=out, out_off=_dev(torch, starts))
    return out.cpu().numpy(), enc["status"].cpu().numpy()


def _check_whole(codec, h, st, segs, starts, tag, bad=()):
    written = np.zeros(h.size, bool)
    for i, (seg, o) in enumerate(zip(segs, starts)):
        if i in bad:
            assert st[i] == DC_E_STREAM, tag + (i, "status", int(st[i]))
            continue
        assert st[i] == 0, tag + (i, "status", int(st[i]))
        assert np.array_equal(h[o: o + seg.size], seg), tag + (i, "decoded bytes")
        written[o: o + seg.size] = True
    assert (h[~written] == FILL).all(), tag + ("bytes outside the good segments written",)
    assert codec.batch_status() == (DC_E_STREAM if bad else 0), tag + ("batch_status",)


@pytest.mark.parametrize("mode", MODES)
def test_the_two_final_comparisons(torch_cuda, codec, mode):
    """A whole-segment decode wants the chunk lengths to sum to `bits` exactly; a range, also the
    range (seg, 0, len), only that its last touched chunk ends within `bits`. So bits + 1 fails the
    first alone, bits - 1 fails both, and nothing else in either call notices."""
    torch = torch_cuda
    good = _enc(torch, codec, mode)
    md, bits = good["mode"].cpu().numpy(), good["bits"].cpu().numpy().astype(np.int64)
    # a coded segment whose payload size stays what it is at bits - 1 and bits + 1: the record test
    # pe - po == pad16((bits + 7) >> 3) then passes, and only the decode's last comparison is left
    fits = [i for i, s in enumerate(SEGMENTS) if md[i] == 1 and bits[i] % 128 != 0 and bits[i] < 8 * s.size
            and _pad16((bits[i] + 6) >> 3) == _pad16((bits[i] + 7) >> 3) == _pad16((bits[i] + 8) >> 3)
            and s.size > 2 * 64 and i not in (B, STORED)]   # (more than two chunks; B and STORED are the bystanders)
    assert fits, "no segment of the oracle batch fits the test"
    seg = min(fits, key=lambda i: SEGMENTS[i].size)
    n = SEGMENTS[seg].size
    starts, cap = _gapped([s.size for s in SEGMENTS])
    # the segment whole, its first chunk alone (ends far below bits either way), and other segments
    rows = [(seg, 0, n), (B, 0, SEGMENTS[B].size), (seg, 0, 64), (STORED, 5, 300), (B, 100, 4000)]
    for delta, range_bad in ((+1, {}), (-1, {0: DC_E_STREAM})):
        enc = dict(good, bits=good["bits"].clone())
        enc["bits"][seg] += delta
        h, st = _whole(torch, codec, enc, SEGMENTS, starts, cap)
        _check_whole(codec, h, st, SEGMENTS, starts, (mode, delta, "whole"), bad=(seg,))
        h, st, offs = _run(torch, codec, enc, rows)
        _check(codec, h, st, rows, offs, (mode, delta, "ranges"), bad=range_bad)


# one wave round of chunks (64) and one workgroup round (256) at S = 16 and one more, and the two
# sides of HBS_WAVE_SEG (the shared-table kernels give a segment or range of up to 8192 bytes to a wave)
EDGE_S = 16
EDGE_LENGTHS = (1, 15, 16, 17, 64 * 16 - 1, 64 * 16, 64 * 16 + 1, 256 * 16 + 1, 8192, 8193)
PHASES = (0, 1, 15)


def _edge_segments():
    """Per length: text (coded in both modes), random bytes (stored under a table of their own once
    they are long enough), all byte values in turn (stored under the text table: it lacks some)."""
    return [content(kind, n, 21 + j) for j, n in enumerate(EDGE_LENGTHS) for kind in ("enwik", "random", "cycle")]


def _phased(segs, rot):
    """Output starts whose 16-B phase goes through PHASES, segment j beginning at PHASES[(j + rot) % 3]."""
    at, starts = 0, []
    for j, s in enumerate(segs):
        at = (at + 15) // 16 * 16 + 16 + PHASES[(j + rot) % 3]   # (past the segment before, one piece free)
        starts.append(at)
        at += s.size
    return np.array(starts, np.int64), at + 31


@pytest.mark.parametrize("mode", MODES)
def test_whole_segment_ranges_are_the_whole_segment_decode(torch_cuda, codec, mode):
    torch = torch_cuda
    segs = _edge_segments()
    if mode == "own":
        exp = oracle_batch(segs, 2, EDGE_S)
    else:
        exp = oracle_shared_batch(segs, *table_codes(text_table(2), 2), EDGE_S)
    assert set(exp["mode"].tolist()) == {0, 1}
    for n in EDGE_LENGTHS[4:]:   # both modes at every length that can show a chunk-round or stage edge
        assert {int(m) for m, s in zip(exp["mode"], segs) if s.size == n} == {0, 1}, (mode, n)
    enc = _upload(torch, codec, mode, segs, exp, 2, EDGE_S)
    whole = np.array([(i, 0, s.size) for i, s in enumerate(segs)], np.int64)
    inner = np.array([(i, 1, s.size - 2) for i, s in enumerate(segs) if s.size >= 3], np.int64)
    for grid in (0, 1):
        codec.set_option("batch_grid", grid)
        try:
            for rot in range(3):   # every segment at each of the three phases
                starts, cap = _phased(segs, rot)
                assert {int(p) for p in starts % 16} == set(PHASES)
                tag = (mode, grid, rot)
                h0, st0 = _whole(torch, codec, enc, segs, starts, cap)
                _check_whole(codec, h0, st0, segs, starts, tag + ("whole",))
                h, st, _ = _run(torch, codec, enc, whole, starts, cap)
                _check(codec, h, st, whole, starts, tag + ("ranges",), segs=segs)
                assert np.array_equal(h, h0), tag
                # first and last touched chunk partial: the range mask is on at both ends
                offs = starts[inner[:, 0]] + 1
                h, st, _ = _run(torch, codec, enc, inner, offs, cap)
                _check(codec, h, st, inner, offs, tag + ("inner ranges",), segs=segs)
        finally:
            codec.set_option("batch_grid", 0)
