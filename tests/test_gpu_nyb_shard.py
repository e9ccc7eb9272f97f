"""The nybble shard-body calls of dist.ShardedNybble on the device, call by call: dc_nyb_mtf_summary,
dc_nyb_body_plan, dc_nyb_body_write, dc_nyb_dbody_plan, dc_nyb_dbody_write against the plain model
of the same call with the same arguments (the nyb_* methods of tests/cpu_engine.py, pinned to the
oracle by tests/test_nyb_shard_cpu.py), byte for byte and number for number.

Geometry (dc_core.hip): a lane codes 16 elements, a wave 1024, a tile is 4096 (FSM_TILE ==
MTF_TILE); k_nyb_enc_wtile takes 4 tiles a workgroup, k_nyb_tiles 8; k_mtf_reduce / k_mtf_down fan
64 tiles. COUNTS holds the element counts (len - 1) around each of these.
Input alignment: the input is a view at byte 0, 2, 3, 15 of a 16-B aligned buffer. mtf_run takes
k_mtf_walk<0/2> unless ((d_in + 1) & 15) >= 4, so 0, 2 and 15 take <0/2> and 3 takes <1/3>; only
offset 0 takes the k_nyb_enc_wtile writers, the others k_fsm_write<M_NYB_ENC>, as does offset 0
under nyb_wtile_off (a Codec of its own).
Every write goes into a buffer of 0xEE at offset 0, 1, 2 or 15 (1 and 2: what a 1- and 2-byte head
give Codec.nyb_body_write); every byte before the output and from the returned length on, up to
and past the documented capacity, must stay 0xEE.
"""
import ctypes as C

import numpy as np
import pytest

from data_compression_amd import synth
from data_compression_amd.dist import INITIAL_LISTS, compose_lists, compose_summaries
from oracle import oracle as orc
from tests.cpu_engine import CpuEngine
from tests.nyb_shard_stitch import cpu_put, dstitch, stitch
from tests.test_nyb_shard_cpu import ALPHABETS, arbitrary_bodies, draw, same_summary

pytestmark = pytest.mark.gpu

FILL = 0xEE
DC_E_ARG = -1
TILE = 4096
SHORT = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65)
COUNTS = SHORT + (1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 4 * TILE - 1, 4 * TILE + 1, 8 * TILE + 1)
BIG = 65 * TILE + 3                      # elements: a second level of k_mtf_reduce / k_mtf_down
OUT_OFFSETS = (0, 1, 2, 15)
DIN_OFFSETS = (0, 2, 5, 15)              # 2: what rank 0's seg[2:] gives
# (name, input offset, nyb_wtile_off)
VARIANTS = (("a0", 0, False), ("a2", 2, False), ("a3", 3, False), ("a15", 15, False), ("a0_wtile_off", 0, True))
VIDS = [v[0] for v in VARIANTS]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def codecs(torch_cuda):
    """(the default Codec, one with nyb_wtile_off = 1)"""
    from data_compression_amd.device import Codec
    off = Codec(0)
    off.set_option("nyb_wtile_off", 1)
    return Codec(0), off


@pytest.fixture(scope="module")
def codec(codecs):
    return codecs[0]


def _dev(torch, data, off=0, around=0x65):
    """data at byte `off` of a 16-B aligned device buffer; `around` fills the bytes beside it (an
    'e': a hit, if a kernel took it for an element)"""
    a = np.frombuffer(bytes(data), np.uint8)
    host = np.full(off + a.size + 64, around, np.uint8)
    host[off: off + a.size] = a
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf[off: off + a.size]


class _Out:
    """cap bytes at offset off of a 16-B aligned buffer of 0xEE"""

    def __init__(self, torch, cap, off):
        self.off, self.cap = off, cap
        self.buf = torch.full((off + cap + 64,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + off

    def taken(self, n):
        h = self.buf.cpu().numpy()
        assert n <= self.cap, "returned length %d over the capacity %d" % (n, self.cap)
        assert (h[: self.off] == FILL).all(), "bytes before the output were written"
        assert (h[self.off + n:] == FILL).all(), "bytes from the returned length on were written"
        return h[self.off: self.off + n].tobytes()

    def untouched(self):
        return bool((self.buf.cpu().numpy() == FILL).all())


def _body_write(torch, codec, y, modify, pend, is_last, out_off):
    """dc_nyb_body_write into a guarded buffer of the documented 2 * len: (bytes, *h_state_out)"""
    from data_compression_amd._lib import check
    o = _Out(torch, 2 * y.numel(), out_off)
    ln, st = C.c_uint64(1 << 40), C.c_int32(-7)
    check("dc_nyb_body_write", codec.L.dc_nyb_body_write(codec.ctx, y.data_ptr(), y.numel(), int(modify), pend,
                                                         int(is_last), o.ptr, C.byref(ln), C.byref(st)))
    return o.taken(ln.value), st.value


def _dbody_write(torch, codec, y, m, s_in, out_off):
    from data_compression_amd._lib import check
    o = _Out(torch, 2 * m, out_off)
    ln, st = C.c_uint64(1 << 40), C.c_int32(-7)
    check("dc_nyb_dbody_write", codec.L.dc_nyb_dbody_write(codec.ctx, y.data_ptr(), y.numel(), m, s_in, o.ptr,
                                                           C.byref(ln), C.byref(st)))
    return o.taken(ln.value), st.value


# ---- inputs and their model, computed once ---------------------------------------------------------
def _random_lists(rng):
    """each row 8 distinct bytes of 0..255: bytes >= 0x80 and a zero among them"""
    rows = np.stack([rng.permutation(256)[:8] for _ in range(16)]).astype(np.uint8)
    rows[3, 5] = 0 if 0 not in rows[3] else rows[3, 5]
    return rows


def _bases():
    rng = np.random.default_rng(0x5EED)
    n = COUNTS[-1] + 1
    out = {"english": synth.english_like(n).tobytes(), "uniform": synth.uniform_bytes(n).tobytes()}
    for name, alpha in ALPHABETS.items():
        out[name] = draw(alpha, n, rng)
    return out


BASES = _bases()
FAMILIES = tuple(BASES)
# the adaptive entry lists of a family in the count tests: the initial lists, or random rows
ENTRY = {f: (INITIAL_LISTS.copy() if f in ("english", "text") else _random_lists(np.random.default_rng(len(f))))
         for f in FAMILIES}
_MODEL = {}


def model(x, modify, lists, combos):
    """(plan, {(pend, is_last): (body, exit state)}) of the shard buffer x, cached"""
    key = (x, modify, None if lists is None else lists.tobytes(), tuple(combos))
    if key not in _MODEL:
        eng = CpuEngine()
        t = cpu_put(x)
        plan = eng.nyb_body_plan(t, modify, lists)
        w = {(p, l): (eng.nyb_body_write(t, modify, p, bool(l)).numpy().tobytes(), eng.nyb_body_state(p))
             for p, l in combos}
        _MODEL[key] = (plan, w, list(eng._plan[1]))
    return _MODEL[key]


def _check_shard(torch, codec, x, in_off, modify, lists, combos, tag):
    """plan and every write of `combos` on the device against the model; the output offsets in turn"""
    plan, writes, _ = model(x, modify, lists if modify else None, combos)
    y = _dev(torch, x, in_off)
    got = codec.nyb_body_plan(y, modify, lists)
    assert got == plan, (tag, "plan", got, plan)
    for i, ((pend, is_last), (body, state)) in enumerate(writes.items()):
        out, st = _body_write(torch, codec, y, modify, pend, is_last, OUT_OFFSETS[(i + len(x)) % 4])
        assert len(out) == len(body), (tag, pend, is_last, "length", len(out), len(body))
        assert out == body, (tag, pend, is_last, "bytes differ first at",
                             next(k for k in range(len(body)) if out[k] != body[k]))
        assert st == state, (tag, pend, is_last, "exit state", st, state)


# ---- nyb_body_plan / nyb_body_write: every count, family, alignment and writer ---------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_body_plan_and_write_at_every_count(torch_cuda, codecs, family, variant):
    """Static and adaptive, all five plan numbers, then the body from both entry states with and
    without is_last, at each element count of COUNTS."""
    _, in_off, wtile_off = variant
    codec = codecs[1 if wtile_off else 0]
    for count in COUNTS:
        x = BASES[family][: count + 1]
        combos = ((-1, 0), (-1, 1), (count % 8, 0), ((count + 3) % 8, 1))
        for modify in (False, True):
            _check_shard(torch_cuda, codec, x, in_off, modify, ENTRY[family], combos, (family, count, modify))


def _product_inputs():
    """per short count >= 1: a text whose first element is a hit or a miss, whose last element is
    a hit or a miss, after a run of 0 or 1 more hits that follows a miss (so the shard ends both
    pending and not, from either entry state)"""
    rng = np.random.default_rng(0xA7)
    out = []
    for count in SHORT[1:]:
        for first in b"eq":
            for last in b"tq":
                for run in (0, 1):
                    el = bytearray(draw(ALPHABETS["text"], count, rng))
                    el[0] = first
                    el[-1] = last
                    if count >= 3 + run:
                        el[-2 - run] = ord("x")
                        for k in range(run):
                            el[-2 - k] = ord("a")
                    out.append(bytes([ord("n")]) + bytes(el))
    return out


PRODUCT = _product_inputs()


def _product_combos(first_hit):
    pends = range(-1, 8) if first_hit else (-1, 3)
    return tuple((p, l) for p in pends for l in (0, 1))


def test_product_inputs_reach_every_end():
    """from the model's ranks: both first elements, both last elements, and shards that end pending
    and not, from either entry state, on the last shard and before it"""
    for modify in (False, True):
        seen, pends = set(), set()
        for x in PRODUCT:
            rk = CpuEngine()._ranks(x, modify, INITIAL_LISTS)
            plan, w, _ = model(x, modify, INITIAL_LISTS if modify else None, _product_combos(rk[0] != 0xFF))
            for (p, l), (_, state) in w.items():
                seen.add((rk[0] != 0xFF, rk[-1] != 0xFF, p >= 0, state))
                if rk[0] != 0xFF and len(rk) > 1:
                    pends.add((p, l))
        # (a last miss never ends pending: 2 first x 2 entry states; a last hit ends either way)
        want = {(f, False, e, 0) for f in (False, True) for e in (False, True)}
        want |= {(f, True, e, s) for f in (False, True) for e in (False, True) for s in (0, 1)}
        assert seen == want, (modify, sorted(want - seen))
        assert pends == {(p, l) for p in range(-1, 8) for l in (0, 1)}


@pytest.mark.parametrize("modify", [False, True], ids=["static", "adaptive"])
@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
def test_body_write_argument_product(torch_cuda, codecs, variant, modify):
    """pend_rank -1, 0..7 (every value where the first element is a hit: only then does lane 0 of
    tile 0 write it) x is_last x first element hit / miss x last element hit / miss x the parity
    of the closing run of hits, at the short counts, through each writer."""
    _, in_off, wtile_off = variant
    codec = codecs[1 if wtile_off else 0]
    for x in PRODUCT:
        first_hit = CpuEngine()._ranks(x[:2], modify, INITIAL_LISTS)[0] != 0xFF
        _check_shard(torch_cuda, codec, x, in_off, modify, INITIAL_LISTS, _product_combos(first_hit), (x, modify))


@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
def test_body_write_of_a_shard_of_no_elements(torch_cuda, codecs, variant):
    """len = 1: the state passes through; one byte, d_in[0], only when a nybble is pending and the
    shard ends the stream (the odd tail), else nothing. (fsm_count's ntiles == 0 branch counts that
    byte in the length and no writer has an element to store it from: dc_nyb_body_write copies it.)"""
    _, in_off, wtile_off = variant
    codec = codecs[1 if wtile_off else 0]
    for byte in (0x65, 0x00, 0xC1):
        y = _dev(torch_cuda, bytes([byte]), in_off, around=0x11)
        for modify in (False, True):
            assert codec.nyb_body_plan(y, modify, INITIAL_LISTS) == [0, 0, 0, 1, 0xFF]
            for pend in range(-1, 8):
                for is_last in (0, 1):
                    out, st = _body_write(torch_cuda, codec, y, modify, pend, is_last, OUT_OFFSETS[(pend + 1) % 4])
                    want = bytes([byte]) if pend >= 0 and is_last else b""
                    assert out == want, (byte, modify, pend, is_last, out)
                    assert st == (1 if pend >= 0 else 0)
                    mp, mw, _ = model(bytes([byte]), modify, INITIAL_LISTS if modify else None, ((pend, is_last),))
                    assert mw[pend, is_last] == (want, st) and mp == [0, 0, 0, 1, 0xFF]


# ---- nyb_body_plan: entry lists and the last rank ---------------------------------------------------
@pytest.mark.parametrize("in_off", [0, 3], ids=["walk2", "walk3"])
def test_body_plan_under_composed_and_random_lists(torch_cuda, codec, in_off):
    """Adaptive entry lists composed from a DEVICE summary of the stretch before the shard (as the
    ranks of ShardedNybble compose them), and random rows, on every family."""
    rng = np.random.default_rng(0xC0)
    for family in FAMILIES:
        base = BASES[family]
        for count in (1, 17, 65, 1025, TILE + 1):
            k = 300
            summ = codec.nyb_mtf_summary(_dev(torch_cuda, base[: k + 1], in_off))
            for lists in (compose_lists(INITIAL_LISTS, *summ), _random_lists(rng)):
                _check_shard(torch_cuda, codec, base[k: k + count + 1], in_off, True, lists, ((-1, 1), (2, 0)),
                             (family, count))


LAST_COUNTS = tuple(range(1, 41)) + (TILE, TILE + 1)


@pytest.mark.parametrize("in_off", [0, 3], ids=["walk2", "walk3"])
def test_adaptive_plan_last_rank_of_a_first_touch(torch_cuda, codec, in_off):
    """h_plan[4] is ws.rk[len - 2], where k_mtf_walk leaves 0xFE for a first touch and k_mtf_resolve
    settles the tile's last element: shards of 1..40 elements, and of a tile and one more, whose
    last element's byte 'Z' is nowhere before it in the shard and sits in its context's entry list
    at each rank in turn, or not at all. The write that follows carries that rank out."""
    rng = np.random.default_rng(0x1A)
    ranks = set()
    for count in LAST_COUNTS:
        x = b"a" + draw(b"ab", count - 1, rng) + b"Z"
        assert x.index(b"Z") == count and all(((p >> 3) & 15) == 12 for p in x[:-1])
        for r in list(range(8)) + [None]:
            lists = _random_lists(rng)
            row = [int(v) for v in rng.permutation(256) if v != ord("Z")][:8]
            if r is not None:
                row[r] = ord("Z")
            lists[12] = row
            plan, _, _ = model(x, True, lists, ((-1, 1), (5, 1)))
            ranks.add(plan[4])
            _check_shard(torch_cuda, codec, x, in_off, True, lists, ((-1, 1), (5, 1)), (count, r))
    assert ranks == set(range(8)) | {0xFF}, ranks


@pytest.mark.parametrize("in_off", [0, 3])
def test_static_plan_last_rank(torch_cuda, codec, in_off):
    for count in (1, 2, 17, TILE, TILE + 1):
        for k, last in enumerate(b" etaoinsZ\x00\xe5"):
            x = BASES["text"][: count] + bytes([last])
            plan, _, _ = model(x, False, None, ((-1, 1),))
            assert plan[4] == (k if k < 8 else 0xFF)
            _check_shard(torch_cuda, codec, x, in_off, False, None, ((-1, 1),), (count, last))


# ---- nyb_mtf_summary -------------------------------------------------------------------------------
SUMMARY_COUNTS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE - 1,
                  2 * TILE, 2 * TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1)


def _summary_bases():
    rng = np.random.default_rng(0x50)
    n = SUMMARY_COUNTS[-1] + 1
    out = dict(BASES)
    # lists that never fill: most contexts keep fewer than 8 entries
    out.update(two=draw(b"ab", n, rng), two_zero=draw(b"a\x00", n, rng), three=draw(b"e x", n, rng),
               three_zero=draw(b"e\x00x", n, rng))
    late = bytearray(draw(b"abc", n, rng))
    late[1 + TILE + 4000] = 0            # the second tile's only zero byte, late in it
    out["one_zero_late"] = bytes(late)
    return {k: v[:n] for k, v in out.items()}


SUMMARY_BASES = _summary_bases()
_SUMM = {}


def _model_summary(name, count):
    if (name, count) not in _SUMM:
        _SUMM[name, count] = CpuEngine().nyb_mtf_summary(cpu_put(SUMMARY_BASES[name][: count + 1]))
    return _SUMM[name, count]


def test_summary_inputs_keep_short_lists_and_a_lone_zero():
    short = {name: int((_model_summary(name, 3 * TILE)[1] < 8).sum()) for name in SUMMARY_BASES}
    assert all(short[k] >= 14 for k in ("two", "two_zero", "three", "three_zero", "one_zero_late")), short
    el = SUMMARY_BASES["one_zero_late"][1:]
    assert el[TILE: 2 * TILE].count(0) == 1 and el[TILE + 4000] == 0 and el.count(0) == 1


@pytest.mark.parametrize("in_off", [0, 2, 3, 15], ids=["walk0_a0", "walk0_a2", "walk1_a3", "walk0_a15"])
@pytest.mark.parametrize("name", tuple(SUMMARY_BASES))
def test_mtf_summary(torch_cuda, codec, name, in_off):
    """lists and counts (only the first cnt[c] entries of a list are defined), up to 3 tiles"""
    for count in SUMMARY_COUNTS:
        got = codec.nyb_mtf_summary(_dev(torch_cuda, SUMMARY_BASES[name][: count + 1], in_off))
        want = _model_summary(name, count)
        assert np.array_equal(got[1], want[1]), (name, count, "counts", got[1], want[1])
        assert same_summary(got, want), (name, count, got, want)


@pytest.fixture(scope="module")
def big_text():
    return synth.english_like(BIG + 1, seed=0xB16).tobytes()


def _model_summary_of(x):
    if "big" not in _SUMM:
        _SUMM["big"] = CpuEngine().nyb_mtf_summary(cpu_put(x))
    return _SUMM["big"]


@pytest.mark.parametrize("in_off", [0, 3], ids=["walk0", "walk1"])
def test_mtf_summary_over_two_reduce_levels(torch_cuda, codec, big_text, in_off):
    """65 * 4096 + 3 elements: 66 tiles, so k_mtf_reduce / k_mtf_down run a second level. Route:
    directly against the model's summary of the whole input (a fraction of a second, computed once
    for both walks); and the device's own summaries of a prefix of 64 tiles and a ragged one and
    of the rest, two calls, compose to it."""
    want = _model_summary_of(big_text)
    whole = codec.nyb_mtf_summary(_dev(torch_cuda, big_text, in_off))
    assert np.array_equal(whole[1], want[1]) and same_summary(whole, want)
    cut = 64 * TILE + 9
    prefix = codec.nyb_mtf_summary(_dev(torch_cuda, big_text[: cut + 1], in_off))
    tail = codec.nyb_mtf_summary(_dev(torch_cuda, big_text[cut:], in_off))
    assert same_summary(compose_summaries(*prefix, *tail), want)


# ---- nyb_dbody_plan / nyb_dbody_write --------------------------------------------------------------
DBODY_M = (0, 1, 2, 15, 16, 17, 1023, 1025, TILE - 1, TILE + 1, 2 * TILE + 1)


DBODY_NAMES = ("oracle_text", "oracle_high", "random", "pairs", "low")


@pytest.fixture(scope="module")
def dbodies():
    """bodies of the oracle's streams, and bodies that no encoder need have written"""
    rng = np.random.default_rng(0xDB)
    out = {"oracle_text": orc.nybble_compress(BASES["english"], False)[2:],
           "oracle_high": orc.nybble_compress(BASES["high"], False)[2:]}
    for name, s in arbitrary_bodies(rng, sizes=(DBODY_M[-1] + 16,)):
        out[name.rstrip("0123456789")] = s[2:]
    assert tuple(out) == DBODY_NAMES and all(len(b) >= DBODY_M[-1] + 8 for b in out.values())
    return out


def _check_dbody(torch, codec, buf, m, in_off, tag):
    eng = CpuEngine()
    t = cpu_put(buf)
    plan = eng.nyb_dbody_plan(t, m)
    y = _dev(torch, buf, in_off, around=0xE1)
    got = codec.nyb_dbody_plan(y, m)
    assert got == plan, (tag, "plan", got, plan)
    for s_in in (0, 1):
        want = eng.nyb_dbody_write(t, m, s_in).numpy().tobytes()
        out, st = _dbody_write(torch, codec, y, m, s_in, OUT_OFFSETS[(m + s_in) % 4])
        assert len(out) == len(want) == plan[s_in], (tag, s_in, "length", len(out), len(want), plan)
        assert out == want, (tag, s_in, "bytes differ first at", next(k for k in range(len(want)) if out[k] != want[k]))
        assert st == plan[2 + s_in], (tag, s_in, "exit state", st, plan)


@pytest.mark.parametrize("in_off", DIN_OFFSETS)
@pytest.mark.parametrize("name", DBODY_NAMES)
def test_dbody_plan_and_write(torch_cuda, codec, dbodies, name, in_off):
    """m bytes without (len = m) and with (len = m + 1) the byte of right halo, from both states"""
    for m in DBODY_M:
        for halo in (0, 1):
            _check_dbody(torch_cuda, codec, dbodies[name][7: 7 + m + halo], m, in_off, (name, m, halo))


@pytest.mark.parametrize("in_off", DIN_OFFSETS)
def test_dbody_halo_nybble(torch_cuda, codec, dbodies, in_off):
    """a last byte whose low nybble is < 8 takes the halo byte's high nybble, reached at the high
    nybble (a pair byte, from state 0) and at the low one (from state 1)"""
    seen = set()
    for m in (1, 2, 17, TILE + 1):
        for last in (0x93, 0x35, 0xF0):
            for halo in (0x00, 0x7F, 0xF0):
                buf = dbodies["oracle_text"][: m - 1] + bytes([last, halo])
                _check_dbody(torch_cuda, codec, buf, m, in_off, (m, last, halo))
                eng = CpuEngine()
                for s_in in (0, 1):
                    out, s = eng._dwalk(buf, m, s_in)
                    if s == 1:
                        assert out[-1] == ((last & 7) << 4) + (halo >> 4)
                        seen.add((s_in if m == 1 else None, halo))
    assert {(s, h) for s in (0, 1) for h in (0x00, 0x7F, 0xF0)} <= seen


# ---- stitched against the oracle --------------------------------------------------------------------
def test_stitched_shards_equal_the_oracle(torch_cuda, codec, big_text):
    """The one larger case: whole streams from the device's shard calls (tests/nyb_shard_stitch.py)
    over 65 * 4096 + 3 bytes, cut so that a shard holds a tile, one element less, one more, with a
    shard of no elements at the end; a second shard of 65 tiles takes the second reduce level."""
    text = big_text[: BIG - 2] + b"qe"    # a miss, then one hit: the stream ends with a nybble pending,
    n = len(text)                         # and the closing shard of no elements writes the odd tail
    put = lambda b: _dev(torch_cuda, b)
    for modify in (False, True):
        want = orc.nybble_compress(text, modify)
        assert want[0] == 0xAF
        for cuts in ((TILE + 1, n), (TILE, n), (TILE + 2, n), (TILE + 1, 2 * TILE, 3 * TILE + 1, 3 * TILE + 1, n)):
            assert stitch(codec, text, cuts, modify, put=put) == want, (modify, cuts)
    stream = orc.nybble_compress(text, False)
    want = orc.nybble_decompress(stream, False)
    assert want == text
    mt = len(stream) - 2
    for halo in (True, False):
        for cuts in ((TILE, mt), (TILE - 1, TILE + 1, mt), (TILE + 1, TILE + 1)):
            assert dstitch(codec, stream, cuts, halo, put=put) == want, (halo, cuts)


# ---- one context, interleaved calls -----------------------------------------------------------------
def _ab():
    a = BASES["english"][: 2 * TILE + 18]
    b = BASES["text"][: TILE + 7]
    return a, b


def test_write_twice_after_one_plan(torch_cuda, codec):
    """the second write takes the d_fraw copy of the tile summaries (summ_fresh is false)"""
    a, _ = _ab()
    plan, w, _ = model(a, True, INITIAL_LISTS, ((4, 1),))
    y = _dev(torch_cuda, a)
    assert codec.nyb_body_plan(y, True, INITIAL_LISTS) == plan
    one = _body_write(torch_cuda, codec, y, True, 4, 1, 1)
    two = _body_write(torch_cuda, codec, y, True, 4, 1, 2)
    assert one == two == w[4, 1]


def test_static_compress_between_plan_and_write(torch_cuda, codec):
    a, b = _ab()
    plan, w, _ = model(a, True, INITIAL_LISTS, ((4, 1),))
    y = _dev(torch_cuda, a)
    assert codec.nyb_body_plan(y, True, INITIAL_LISTS) == plan
    assert codec.nyb_compress(_dev(torch_cuda, b), False).cpu().numpy().tobytes() == orc.nybble_compress(b, False)
    assert _body_write(torch_cuda, codec, y, True, 4, 1, 1) == w[4, 1]


def test_summary_between_plan_and_write_is_refused(torch_cuda, codec):
    """the ranks are gone: DC_E_ARG (plan this input first), and nothing written"""
    a, b = _ab()
    y = _dev(torch_cuda, a)
    codec.nyb_body_plan(y, True, INITIAL_LISTS)
    want = CpuEngine().nyb_mtf_summary(cpu_put(b))
    assert same_summary(codec.nyb_mtf_summary(_dev(torch_cuda, b)), want)
    o = _Out(torch_cuda, 2 * len(a), 1)
    ln, st = C.c_uint64(0), C.c_int32(0)
    rc = codec.L.dc_nyb_body_write(codec.ctx, y.data_ptr(), len(a), 1, 4, 1, o.ptr, C.byref(ln), C.byref(st))
    assert rc == DC_E_ARG and o.untouched()


# ---- argument errors: no launch ----------------------------------------------------------------------
def test_argument_errors(torch_cuda, codec):
    L, ctx = codec.L, codec.ctx
    x = BASES["text"][:40]
    y = _dev(torch_cuda, x)
    o = _Out(torch_cuda, 2 * len(x), 0)
    ln, st = C.c_uint64(0), C.c_int32(0)
    plan = np.zeros(5, np.uint64)
    lists = np.ascontiguousarray(INITIAL_LISTS)
    summ, cnt = np.zeros(128, np.uint8), np.zeros(16, np.uint8)
    p, lp = plan.ctypes.data, lists.ctypes.data
    bw = lambda **k: L.dc_nyb_body_write(k.get("ctx", ctx), k.get("y", y.data_ptr()), k.get("n", len(x)), 0,
                                         k.get("pend", -1), 1, k.get("out", o.ptr), k.get("ln", C.byref(ln)), C.byref(st))
    dw = lambda **k: L.dc_nyb_dbody_write(k.get("ctx", ctx), k.get("y", y.data_ptr()), k.get("n", len(x)),
                                          k.get("m", len(x)), k.get("s", 0), k.get("out", o.ptr),
                                          k.get("ln", C.byref(ln)), C.byref(st))
    assert L.dc_nyb_body_plan(ctx, y.data_ptr(), len(x), 0, None, p) == 0
    bad = {
        "pend_rank 8": bw(pend=8),
        "write: no ctx": bw(ctx=None), "write: no input": bw(y=None), "write: no output": bw(out=None),
        "write: no length": bw(ln=None), "write: len 0": bw(n=0),
        "adaptive plan without lists": L.dc_nyb_body_plan(ctx, y.data_ptr(), len(x), 1, None, p),
        "plan: no ctx": L.dc_nyb_body_plan(None, y.data_ptr(), len(x), 0, lp, p),
        "plan: no input": L.dc_nyb_body_plan(ctx, None, len(x), 0, lp, p),
        "plan: no plan": L.dc_nyb_body_plan(ctx, y.data_ptr(), len(x), 0, lp, None),
        "plan: len 0": L.dc_nyb_body_plan(ctx, y.data_ptr(), 0, 0, lp, p),
        "summary: no ctx": L.dc_nyb_mtf_summary(None, y.data_ptr(), len(x), summ.ctypes.data, cnt.ctypes.data),
        "summary: no input": L.dc_nyb_mtf_summary(ctx, None, len(x), summ.ctypes.data, cnt.ctypes.data),
        "summary: no lists": L.dc_nyb_mtf_summary(ctx, y.data_ptr(), len(x), None, cnt.ctypes.data),
        "summary: no counts": L.dc_nyb_mtf_summary(ctx, y.data_ptr(), len(x), summ.ctypes.data, None),
        "dbody write: len = m + 2": dw(m=len(x) - 2), "dbody write: m > len": dw(m=len(x) + 1),
        "dbody write: s_in 2": dw(s=2), "dbody write: s_in -1": dw(s=-1),
        "dbody write: no ctx": dw(ctx=None), "dbody write: no input": dw(y=None), "dbody write: no output": dw(out=None),
        "dbody write: no length": dw(ln=None),
        "dbody plan: len = m + 2": L.dc_nyb_dbody_plan(ctx, y.data_ptr(), len(x), len(x) - 2, p),
        "dbody plan: no ctx": L.dc_nyb_dbody_plan(None, y.data_ptr(), len(x), len(x), p),
        "dbody plan: no input": L.dc_nyb_dbody_plan(ctx, None, len(x), len(x), p),
        "dbody plan: no plan": L.dc_nyb_dbody_plan(ctx, y.data_ptr(), len(x), len(x), None),
    }
    assert {k: v for k, v in bad.items() if v != DC_E_ARG} == {}
    assert o.untouched()
