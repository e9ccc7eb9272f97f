"""What the tests of the two byte-stream batch codecs (nybble batch v1, small batch v1) share: the
status codes, the prefill byte, the packing of a list of buffers and the check of an encoded batch
against the oracle's streams. A plain module: no fixtures, no tests."""
import numpy as np

FILL = 0xA5
DC_E_ARG, DC_E_CAPACITY, DC_E_STREAM = -1, -6, -7


def pack_offsets(bufs):
    """The buffers back to back (most offsets odd): (bytes, int64 offsets of count + 1)."""
    off = np.zeros(len(bufs) + 1, np.int64)
    off[1:] = np.cumsum([b.size for b in bufs])
    return (np.concatenate(bufs) if bufs else np.zeros(0, np.uint8)), off


def _dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()   # (np.frombuffer arrays are read-only)


def _cum(streams):
    off = np.zeros(len(streams) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in streams])
    return off


def _check_streams(h, oo, st, want, tag, bad=None):
    """Every stream not in `bad` (index -> status) is the oracle's at its place; a bad one takes
    the bytes want[i] says (b"" for DC_E_ARG) and writes none; all else keeps the prefill."""
    bad = bad or {}
    exp_off = _cum(want)
    assert np.array_equal(oo, exp_off), tag + ("out_off",)
    written = np.zeros(h.size, bool)
    for i, s in enumerate(want):
        if i in bad:
            assert st[i] == bad[i], tag + (i, "status", int(st[i]))
            continue
        assert st[i] == 0, tag + (i, int(st[i]))
        assert h[exp_off[i]: exp_off[i + 1]].tobytes() == s, tag + (i, "stream")
        written[exp_off[i]: exp_off[i + 1]] = True
    assert (h[~written] == FILL).all(), tag + ("bytes of no good stream written",)
