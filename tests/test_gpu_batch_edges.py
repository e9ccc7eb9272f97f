"""The batch Huffman bodies at their own edges, on the device: every case of the catalogue of
tests/batch_body_model.py (codes, window, units, chunks, phase, mode, deal, damage) through
Codec.encode_batch / decode_batch / decode_batch_ranges in the own, shared and set modes, compared
byte for byte with the model. This file only runs the catalogue: what each case plants is asserted
from the model in tests/test_batch_body_model_cpu.py (test_<family>_reach_*).

A decode case is a hand batch (streams the device never wrote) decoded into a 0xA5 buffer with
4096 guard bytes either side, each segment at the 16-byte phase the case names; every byte of the
buffer, every status and batch_status() are compared. Every whole-segment case is asked again as
byte ranges. An encode case goes into 0xA5-filled payload / sync_len of the documented bounds plus
a guard; every byte and entry inside and outside is compared, and the batch decodes back."""
import numpy as np
import pytest

from tests import batch_body_model as M

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 4096


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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _grid:
    def __init__(self, codec, grid):
        self.codec, self.grid = codec, grid

    def __enter__(self):
        self.codec.set_option("batch_grid", self.grid)

    def __exit__(self, *a):
        self.codec.set_option("batch_grid", 0)


def _pad259(lens):
    L = np.zeros(259, np.int32)
    L[:256] = lens
    return L


_tables = {}


def _mode_args(torch, codec, case):
    """what the mode adds to an enc dict or an encode call: table= / table_set="""
    key = (case.mode, case.n_ary, tuple(r["lens"].tobytes() for r in case.records or ()))
    if key not in _tables:
        if case.mode == "shared":
            _tables[key] = {"table": codec.table_lengths(_dev(torch, _pad259(case.records[0]["lens"])), case.n_ary)}
        elif case.mode == "set":
            _tables[key] = {"table_set": codec.table_set([r["lens"] for r in case.records], case.n_ary)}
        else:
            _tables[key] = {}
    return _tables[key]


def _upload(torch, codec, case):
    """the case's hand batch as the dict encode_batch returns; status prefilled with -99"""
    b = case.batch()
    lens = np.array([len(s) for s, _ in case.items], np.int64)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    count = len(lens)
    enc = {"count": count, "n_ary": case.n_ary, "S": case.S, "offsets": _dev(torch, off), "total": int(off[-1]),
           "lens": _dev(torch, b["lens"]) if case.mode == "own" else None,
           "mode": _dev(torch, b["mode"]), "bits": _dev(torch, b["bits"].astype(np.int32)),
           "pay_off": _dev(torch, b["pay_off"]), "payload": _dev(torch, np.append(b["payload"], np.zeros(16, np.uint8))),
           "sync_off": _dev(torch, b["sync_off"]), "sync_len": _dev(torch, np.append(b["sync_len"], np.uint16(0)).view(np.int16)),
           "status": torch.full((count,), -99, dtype=torch.int32, device="cuda"),
           "payload_cap": int(b["pay_off"][-1]), "sync_cap": int(b["sync_off"][-1])}
    enc.update(_mode_args(torch, codec, case))
    if case.mode == "set":
        enc["tid"] = _dev(torch, b["tid"])
    return enc


def _phased(counts, phases):
    """output starts past a guard, start i at 16-byte phase phases[i], at least 5 bytes between"""
    at, starts = GUARD, []
    for c, ph in zip(counts, phases):
        at += (ph - at) % 16
        starts.append(at)
        at += int(c) + 5
    return np.array(starts, np.int64), at + GUARD


def _first_failure(st):
    bad = [v for v in st if v]
    return bad[0] if bad else 0


def _run_decode(torch, codec, case):
    enc = _upload(torch, codec, case)
    want_st, want = case.outcome()
    lens = [len(s) for s, _ in case.items]
    starts, cap = _phased(lens, case.phases)
    image = np.full(cap, FILL, np.uint8)
    for o, n, st, w in zip(starts, lens, want_st, want):
        if st == 0:
            image[o: o + n] = w
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    with _grid(codec, case.grid):
        codec.decode_batch(enc, out=out, out_off=starts)
        status = codec.batch_status()
    got_st = enc["status"].cpu().tolist()
    assert got_st == want_st, (case, [i for i, (a, b) in enumerate(zip(got_st, want_st)) if a != b][:8])
    h = out.cpu().numpy()
    if not np.array_equal(h, image):
        at = int(np.nonzero(h != image)[0][0])
        seg = int(np.searchsorted(starts, at, side="right")) - 1
        raise AssertionError((case, "byte", at, "segment", seg, "at", at - int(starts[seg]), "of", lens[seg], int(h[at]), int(image[at])))
    assert status == _first_failure(want_st), (case, "batch_status")
    return enc


def _run_ranges(torch, codec, case, enc):
    rows = case.rows()
    phases = getattr(case, "range_phases", None) or [(5 * r + 1) % 16 for r in range(len(rows))]
    want = [M.range_outcome(case, r) for r in rows]
    offs, cap = _phased([r[2] for r in rows], phases)
    image = np.full(cap, FILL, np.uint8)
    for o, (i, f, c), (st, w) in zip(offs, rows, want):
        if st == 0:
            image[o: o + c] = w
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    a = np.array(rows, np.int64).reshape(-1, 3)
    before = enc["status"].clone()
    with _grid(codec, case.grid):
        _, _, rst = codec.decode_batch_ranges(enc, _dev(torch, a[:, 0]), _dev(torch, a[:, 1]), _dev(torch, a[:, 2]), out=out,
                                              out_off=_dev(torch, offs))
        status = codec.batch_status()
    got_st, want_st = rst.cpu().tolist(), [st for st, _ in want]
    assert got_st == want_st, (case, [(rows[r], got_st[r], want_st[r]) for r in range(len(rows)) if got_st[r] != want_st[r]][:8])
    h = out.cpu().numpy()
    if not np.array_equal(h, image):
        at = int(np.nonzero(h != image)[0][0])
        r = int(np.searchsorted(offs, at, side="right")) - 1
        raise AssertionError((case, "byte", at, "range", rows[r], "at", at - int(offs[r]), int(h[at]), int(image[at])))
    assert status == _first_failure(want_st), (case, "batch_status of the ranges")
    assert torch.equal(enc["status"], before), (case, "the batch's status was written by the ranges call")


def _run_encode(torch, codec, case):
    exp = case.expected()
    x = np.concatenate(case.segs) if case.segs else np.zeros(0, np.uint8)
    lens = np.array([len(s) for s in case.segs], np.int64)
    off = case.lead + np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    host = np.full(case.lead + x.size + 64, case.after, np.uint8)
    host[case.lead: case.lead + x.size] = x
    xd = _dev(torch, host)
    assert xd.data_ptr() % 16 == 0
    count = len(case.segs)
    pb, sb = codec.batch_bounds(int(x.size), count, case.S)
    payload = torch.full((pb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    sync = torch.full((sb + GUARD,), -23131, dtype=torch.int16, device="cuda")   # 0xA5A5
    with _grid(codec, case.grid):
        enc = codec.encode_batch(xd, _dev(torch, off), n_ary=case.n_ary, sync_syms=case.S, payload=payload, sync_len=sync,
                                 payload_cap=pb, sync_cap=sb, **_mode_args(torch, codec, case))
        status = codec.batch_status()
    assert status == 0 and not enc["status"].any(), (case, status)
    names = ("mode", "bits", "pay_off", "sync_off") + (("tid",) if case.mode == "set" else ()) + (("lens",) if case.mode == "own" else ())
    for k in names:
        got = enc[k].cpu().numpy()
        if not np.array_equal(got, exp[k]):
            i = int(np.nonzero((got != exp[k]).reshape(count if k in ("mode", "bits", "tid", "lens") else count + 1, -1).any(axis=1))[0][0])
            raise AssertionError((case, k, "entry", i, got[i].tolist() if k != "lens" else "record", exp[k][i].tolist() if k != "lens" else ""))
    pend, send = int(exp["pay_off"][-1]), int(exp["sync_off"][-1])
    assert pend <= pb and send <= sb
    hp = enc["payload"].cpu().numpy()
    if not np.array_equal(hp[:pend], exp["payload"]):
        at = int(np.nonzero(hp[:pend] != exp["payload"])[0][0])
        seg = int(np.searchsorted(exp["pay_off"], at, side="right")) - 1
        raise AssertionError((case, "payload byte", at, "segment", seg, "at", at - int(exp["pay_off"][seg]), int(hp[at]), int(exp["payload"][at])))
    assert (hp[pend:] == FILL).all(), (case, "payload past pay_off[count] written")
    hs = enc["sync_len"].cpu().numpy().view(np.uint16)
    assert np.array_equal(hs[:send], exp["sync_len"]), (case, "sync_len", int(np.nonzero(hs[:send] != exp["sync_len"])[0][0]))
    assert (hs[send:] == 0xA5A5).all(), (case, "sync_len past sync_off[count] written")
    # and back (the decoder is held by the hand batches; this ties the two ends of one call together)
    out, _ = codec.decode_batch(enc)
    assert codec.batch_status() == 0 and np.array_equal(out.cpu().numpy()[: x.size], x), (case, "round trip")


def _cases(kind):
    return [pytest.param(c, id=c.name) for c in M.catalogue() if c.kind == kind]


@pytest.mark.parametrize("case", _cases("enc"))
def test_encode_is_the_models_batch(torch_cuda, codec, case):
    _run_encode(torch_cuda, codec, case)


@pytest.mark.parametrize("case", _cases("dec"))
def test_decode_is_the_models_bytes(torch_cuda, codec, case):
    """the whole segments (a case of ranges alone has one whole segment to decode first), then the
    same batch as byte ranges: the RANGE instantiation over the same plantings"""
    enc = _run_decode(torch_cuda, codec, case)
    _run_ranges(torch_cuda, codec, case, enc)
