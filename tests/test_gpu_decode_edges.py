"""The S = 64 Huffman decoder (k_huff_decode8), its exact redo (k_huff_decode8_fix) and the decoder
tables dec_tables_build writes into dc_dtable, held to tests/huff_decode_model.py at their edges.

A case is the oracle's payload and sync index under a table made from lengths alone
(dc_huff_table_lengths), in a buffer of exactly the catalogue's `words`, decoded into a 16-B aligned
view of a buffer of 0xA5 with 4096 guard bytes on both sides. Every case asserts the bytes (the
model's), dc_huff_decode_status, the guards, dc_huff_decode_redo_count (the model's geometry), and
that the general decoder (decode_general = 1) gives the same bytes. What the catalogue reaches is
asserted on the CPU by tests/test_huff_decode_model_cpu.py; this file only runs it.
"""
import ctypes as C

import numpy as np
import pytest

from tests import huff_decode_model as M
from tests.test_gpu_bigcount import DTable

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5


class DTableDec(C.Structure):   # include/dc_gpu.h dc_dtable, whole
    _fields_ = list(DTable._fields_) + [("fixed8_affine", C.c_int32), ("fixed8_lo", C.c_int32),
                                        ("fixed8_count", C.c_int32), ("dlut14", C.c_uint16 * (1 << 14)),
                                        ("dlut15", C.c_uint16 * (1 << 15))]


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
def dev_tables(torch_cuda, codec):
    """name -> device table from the catalogue table's lengths, made once"""
    made = {}

    def get(name):
        if name not in made:
            t = M.table(name)
            made[name] = codec.table_lengths(torch_cuda.from_numpy(t["lengths"]).cuda(), t["n_ary"])
            assert codec.table_status(made[name]) == (0, t["max_bits"]), name
        return made[name]
    return get


class _Stream:
    """a case's words and index on the device"""

    def __init__(self, torch, case, payload=None):
        self.words = torch.from_numpy(case.word_array(payload).view(np.int32)).cuda()
        self.sync = (torch.from_numpy(case.base.astype(np.int64)).cuda(),
                     torch.from_numpy(case.lens.view(np.int16)).cuda())
        self.bit_base = torch.tensor([case.bit_base], dtype=torch.int64).cuda() if case.dev else case.bit_base
        assert self.words.numel() == case.words and self.words.data_ptr() % 16 == 0


def _decode(torch, codec, case, tab, stream=None):
    """one decode into a poisoned, guarded buffer: (bytes, status, redo count)"""
    s = stream or _Stream(torch, case)
    buf = torch.full((2 * GUARD + case.n,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD: GUARD + case.n]
    assert out.data_ptr() % 16 == 0
    codec.decode(s.words, s.bit_base, s.sync, 64, case.n, tab, out)
    st = codec.decode_status()
    redo = codec.decode_redo_count()
    h = buf.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + case.n:] == FILL).all(), (case, "guard bytes written")
    return h[GUARD: GUARD + case.n], st, redo


def _check(torch, codec, case, tab, stream=None, general=True):
    dec, geo = case.model()
    stream = stream or _Stream(torch, case)
    got, st, redo = _decode(torch, codec, case, tab, stream)
    bad = np.nonzero(got != dec["out"])[0]
    assert bad.size == 0, (case, "first wrong byte", int(bad[0]), "of", case.n)
    assert st == 0, (case, st)
    assert redo == geo["count"], (case, redo, geo["count"])
    if general:
        codec.set_option("decode_general", 1)
        try:
            again, st, _ = _decode(torch, codec, case, tab, stream)
        finally:
            codec.set_option("decode_general", 0)
        assert st == 0 and np.array_equal(again, got), (case, "general decoder")


def test_words_needed_is_the_models(codec):
    for bb, bits in ((0, 0), (0, 1), (31, 1), (31, 2), (77, 12345), ((1 << 33) + 5, 999_999), (128, 32 * 7)):
        assert codec.words_needed(bb, bits) == M.words_needed(bb, bits)


@pytest.mark.parametrize("name", list(M.TABLES))
def test_decoder_tables_match_model(torch_cuda, codec, dev_tables, name):
    """every entry of lut, dlut, dlut2, dlut14 and dlut15, dlut2_k and dec_ready after one decode"""
    assert C.sizeof(DTableDec) == codec.table_bytes
    (case,) = [c for c in M.family("tables") if c.tab == name]
    tab = dev_tables(name)
    _decode(torch_cuda, codec, case, tab)
    f = DTableDec.from_buffer_copy(tab.cpu().numpy().tobytes())
    t = M.table(name)
    assert f.dec_ready == 1 and f.status == 0 and f.max_bits == t["max_bits"] and f.n_ary == t["n_ary"]
    assert np.array_equal(np.frombuffer(bytes(f.code), np.uint32), t["code"])
    assert np.array_equal(np.frombuffer(bytes(f.nbits), np.uint32), t["nbits"].astype(np.uint32))
    assert f.dlut2_k == t["dlut2_k"], (name, f.dlut2_k, t["dlut2_k"], t["E"], t["K"])
    for field, dt in (("lut", np.uint32), ("dlut", np.uint16), ("dlut2", np.uint16), ("dlut14", np.uint16),
                      ("dlut15", np.uint16)):
        got = np.frombuffer(bytes(getattr(f, field)), dt)
        bad = np.nonzero(got != t[field])[0]
        assert bad.size == 0, (name, field, bad.size, "entries; first", int(bad[0]), hex(int(got[bad[0]])),
                               hex(int(t[field][bad[0]])))


@pytest.mark.parametrize("fam", M.FAMILIES)
def test_decode_catalogue(torch_cuda, codec, dev_tables, fam):
    for case in M.family(fam):
        _check(torch_cuda, codec, case, dev_tables(case.tab))


@pytest.mark.parametrize("pct", M.SCHED_PCT)
def test_scheduler_at_small_sizes(torch_cuda, codec, dev_tables, pct):
    """1..45 tuples under each static share; each decode is followed at once, on the same context,
    by a decode of another size into a fresh poisoned buffer: the last wave out of the first must
    have reset the dequeue heads."""
    torch, tab = torch_cuda, dev_tables("b16")
    cases = [M.sched_case(t) for t in M.SCHED_TUPLES]
    streams = [_Stream(torch, c) for c in cases]
    codec.set_option("decode_static_pct", pct)
    try:
        for i, case in enumerate(cases):
            _check(torch, codec, case, tab, streams[i], general=False)
            j = (i + 4) % len(cases)
            _check(torch, codec, cases[j], tab, streams[j], general=False)
    finally:
        codec.set_option("decode_static_pct", 60)


def _on_device(torch, codec, enc, x, check_general):
    """decode enc into a guarded buffer, compared on the device"""
    n = x.numel()
    buf = torch.full((2 * GUARD + n,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD: GUARD + n]
    codec.decode_into(enc, out)
    assert codec.decode_status() == 0
    redo = codec.decode_redo_count()
    assert torch.equal(out, x)
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n:] == FILL).all())
    if check_general:
        codec.set_option("decode_general", 1)
        try:
            g = torch.empty_like(x)
            codec.decode_into(enc, g)
            assert codec.decode_status() == 0
        finally:
            codec.set_option("decode_general", 0)
        assert torch.equal(g, out)
    return redo


def test_scheduler_static_then_dynamic(torch_cuda, codec):
    """the one size at which Ks is 1 and 2 (Ts 2816 and 5632) and the tail is dequeued"""
    torch = torch_cuda
    from data_compression_amd import synth
    n = (2 * 2816 + 300) * 8192 + 4097
    piece = torch.from_numpy(synth.enwik_like(1 << 20, seed=21)).cuda()
    x = piece.repeat(n // piece.numel() + 1)[:n].contiguous()
    enc = codec.encode(x, n_ary=2, sync_syms=64)
    try:
        for pct in M.SCHED_PCT:
            s = M.model_schedule((n + 8191) // 8192, pct)
            assert (s["Ks"], s["Ts"]) == {0: (0, 0), 60: (1, 2816), 100: (2, 5632)}[pct]
            codec.set_option("decode_static_pct", pct)
            _on_device(torch, codec, enc, x, check_general=pct == 60)
    finally:
        codec.set_option("decode_static_pct", 60)


def test_redo_list_parts(torch_cuda, codec, dev_tables):
    """17 x 256 groups, none fast: a redo workgroup's window lists 1088 chunks, in two parts"""
    torch = torch_cuda
    xh, idx, bits = M.redo_list_input()
    x = torch.from_numpy(xh).cuda()
    tab = dev_tables("b32")
    codec.hist(x)
    assert int(codec.plan(tab).item()) == bits
    enc = {"words": codec.alloc_words(0, bits), "sync": codec.alloc_sync(x.numel(), 64), "S": 64, "bit_base": 0,
           "n": x.numel(), "table": tab}
    codec.pack(x, tab, 0, enc["words"], enc["sync"], 64)
    assert codec.pack_status(tab) == 0
    assert np.array_equal(enc["sync"][1][:4096].cpu().numpy().view(np.uint16), np.full(4096, 608, np.uint16))
    redo = _on_device(torch, codec, enc, x, check_general=True)
    assert redo == M.REDO_LIST_GROUPS * 64


@pytest.mark.parametrize("pct", (0, 100))
def test_decode_sequences(torch_cuda, codec, dev_tables, pct):
    """all redone, then none, then some, on one context: each exact with its own redo count"""
    by = {c.name: c for c in M.catalogue()}
    seq = [by["rows32"], by["span-lead0-%d-first" % M.SPAN_LAST_FAST], by["batch-positions"], by["rows32"]]
    counts = [c.model()[1]["count"] for c in seq]
    assert counts[0] == 64 * seq[0].model()[1]["ngroups"] and counts[1] == 0 and 0 < counts[2] < 64 * 4
    codec.set_option("decode_static_pct", pct)
    try:
        for c in seq:
            _check(torch_cuda, codec, c, dev_tables(c.tab), general=False)
    finally:
        codec.set_option("decode_static_pct", 60)


@pytest.mark.parametrize("first", (None, 0xC3))
def test_c5_counts_through_the_redo(torch_cuda, codec, first):
    """dc_small_huff_decode at n = 16: the redo adds the pairs of the chunks it rewrites to the fast
    decoder's counts per group; pairs and 4-digit codes share groups, the partial last chunk holds
    a pair, and with x[0] >= 0x80 the raw byte M[1] is no pair."""
    torch = torch_cuda
    xh, case = M.c5_case(first)
    dec, geo = case.model()
    assert (case.x[geo["redo"].reshape(-1)[: dec["bad"].size].repeat(64)[: case.n]] >= 0x80).any()
    x = torch.from_numpy(xh.copy()).cuda()
    enc = codec.small_huff_encode(x, n_ary=16, sync_syms=64)
    assert enc["n"] == case.n and enc["bits"] == case.bits and enc["words"].numel() >= case.words
    enc["words"] = enc["words"][: case.words]
    buf = torch.full((2 * GUARD + 2 * case.n,), FILL, dtype=torch.uint8, device="cuda")
    out = codec.small_huff_decode(enc, out=buf[GUARD: GUARD + 2 * case.n])
    assert codec.decode_status() == 0
    assert codec.decode_redo_count() == geo["count"]
    assert out.numel() == xh.size and np.array_equal(out.cpu().numpy(), xh)
    h = buf.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + xh.size:] == FILL).all()


@pytest.mark.parametrize("tab,seed", (("t89", 1), ("n3", 4)))
def test_damage_stays_in_its_chunk(torch_cuda, codec, dev_tables, tab, seed):
    """Bits flipped inside a dozen chunks of a valid stream at the documented capacity. Under the
    complete 8/9-bit code every bit pattern decodes: status 0, every byte the model's. Under
    n = 3 a damaged chunk may hold an invalid digit: DC_E_STREAM, untouched chunks exact, damaged
    ones compared up to the model's first invalid symbol."""
    torch = torch_cuda
    case, payload, chunks, dd = M.damage_case(tab, seed)
    got, st, _ = _decode(torch, codec, case, dev_tables(tab), _Stream(torch, case, payload))
    touched = np.zeros(dd["bad"].size, bool)
    touched[chunks] = True
    wrong = []
    for c in range(dd["bad"].size):
        lo = c * 64
        hi = min(lo + (int(dd["good"][c]) if touched[c] else 64), case.n)
        want = dd["out"][lo:hi] if touched[c] else case.x[lo:hi]
        if not np.array_equal(got[lo:hi], want):
            wrong.append((c, bool(touched[c]), int(dd["good"][c])))
    assert not wrong, (tab, wrong)
    assert st == (M.DC_E_STREAM if dd["bad"].any() else 0), (tab, st)
    assert bool(dd["bad"].any()) == (tab == "n3")
