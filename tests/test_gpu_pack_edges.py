"""The Huffman pack (k_huff_pack) and its plan (k_plan_total, k_block_local, k_block_final_wide), held
to tests/huff_pack_model.py at their own edges.

A case is an input under a table made from lengths alone (dc_huff_table_lengths): hist -> plan ->
pack_async into a view of a buffer of 0xFF (or zeros) with GW guard words on both sides, the sync
index into arrays of exactly dc_huff_sync_chunks / _groups entries inside poisoned buffers. Every
case asserts the plan total, dc_huff_block_hist and dc_huff_plan_offsets entry for entry (the
model's), every word the stream touches (the oracle's, zero bits before bit_base and after the last
code), that every other word, every guard and every index entry past the counts is untouched,
dc_huff_pack_status, and that a decode of the device's own stream gives the input back. Every buffer
is larger than the capacity the call is given, so a wrong kernel overwrites a guard of ours and
never leaves the allocation. What the catalogue reaches is asserted on the CPU by
tests/test_huff_pack_model_cpu.py; this file only runs it.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import huff_pack_model as M

pytestmark = pytest.mark.gpu

GW = 16384                      # guard words: more than the longest block of the catalogue codes to
GS = 64                         # guard entries of the index arrays
LEN_POISON, BASE_POISON = 0x5A5A, 0x5A5A5A5A5A5A5A5A


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
    """name -> device table from the model table's lengths, made once"""
    made = {}

    def get(name):
        if name not in made:
            t = M.table(name)
            made[name] = codec.table_lengths(torch_cuda.from_numpy(t["lengths"]).cuda(), t["n_ary"])
            assert codec.table_status(made[name]) == (0, t["max_bits"]), name
        return made[name]
    return get


class _Out:
    """the guarded buffers of one pack: words (cap of them, `shift` words off 16 bytes), lens, base"""

    def __init__(self, torch, codec, n, S, shift, cap, fill):
        self.fill, self.shift, self.cap = fill, shift, cap
        self.buf = torch.full((2 * GW + 4 + cap,), -1 if fill else 0, dtype=torch.int32, device="cuda")
        self.words = self.buf[GW + shift: GW + shift + cap]
        assert self.buf.data_ptr() % 16 == 0 and (self.words.data_ptr() % 16 == 0) == (shift == 0)
        self.groups, self.chunks = codec.sync_sizes(n, S)
        assert (self.groups, self.chunks) == (-(-(-(-n // S)) // M.GROUP), -(-n // S))
        self.lbuf = torch.full((2 * GS + self.chunks,), LEN_POISON, dtype=torch.int16, device="cuda")
        self.bbuf = torch.full((2 * GS + self.groups,), BASE_POISON, dtype=torch.int64, device="cuda")
        self.sync = (self.bbuf[GS: GS + self.groups], self.lbuf[GS: GS + self.chunks])

    def host(self):
        return (self.buf.cpu().numpy().view(np.uint8), self.lbuf.cpu().numpy().view(np.uint16),
                self.bbuf.cpu().numpy().view(np.uint64))

    def assert_words(self, what, want, zero_words=()):
        """the first len(want) bytes of the view are `want`, the words zero_words (past them) are
        zero, and every other byte of the buffer is the fill"""
        h = self.host()[0].copy()
        lo = 4 * (GW + self.shift)
        bad = np.nonzero(h[lo: lo + want.size] != want)[0]
        assert bad.size == 0, (what, "first wrong word", int(bad[0]) // 4, "of", want.size // 4, bad.size, "bytes")
        h[lo: lo + want.size] = self.fill
        for w in zero_words:
            assert not h[lo + 4 * w: lo + 4 * w + 4].any(), (what, "word", w, "not zeroed")
            h[lo + 4 * w: lo + 4 * w + 4] = self.fill
        bad = np.nonzero(h != self.fill)[0]
        assert bad.size == 0, (what, "written outside the stream: word", (int(bad[0]) - lo) // 4, "of the view;",
                               bad.size, "bytes")

    def assert_index(self, what, lens=None, base=None):
        """the index is (lens, base), or untouched; its guards are untouched"""
        _, l, b = self.host()
        for got, want, poison, g in ((l, lens, LEN_POISON, "lens"), (b, base, BASE_POISON, "base")):
            k = got.size - 2 * GS
            assert (got[:GS] == poison).all() and (got[GS + k:] == poison).all(), (what, g, "guard written")
            if want is None:
                assert (got[GS: GS + k] == poison).all(), (what, g, "written")
            else:
                bad = np.nonzero(got[GS: GS + k] != want)[0]
                assert bad.size == 0, (what, g, "first wrong entry", int(bad[0]), "of", k, int(got[GS + bad[0]]),
                                       int(want[bad[0]]))


def _plan(torch, codec, x, tab, case):
    """hist -> plan of the device input x: the total, block histograms and offsets are the model's"""
    codec.hist(x)
    total = int(codec.plan(tab).item())
    bh, _, off = case.plan()
    assert total == int(off[-1]), (case, total, int(off[-1]))
    got_bh = np.zeros(bh.size, np.uint16)
    assert codec.L.dc_huff_block_hist(codec.ctx, got_bh.ctypes.data, got_bh.size) == 0
    bad = np.nonzero(got_bh != bh.reshape(-1))[0]
    assert bad.size == 0, (case, "block histogram: block", int(bad[0]) // 256, "byte", int(bad[0]) % 256)
    got_off, hn = np.zeros(off.size, np.uint64), C.c_uint64(0)
    assert codec.L.dc_huff_plan_offsets(codec.ctx, got_off.ctypes.data, got_off.size, C.byref(hn)) == 0
    assert hn.value == off.size
    bad = np.nonzero(got_off != off)[0]
    assert bad.size == 0, (case, "plan offsets: first wrong entry", int(bad[0]), int(got_off[bad[0]]), int(off[bad[0]]))


def _run(torch, codec, case, tab, fill=0xFF):
    payload, bits, idx, base, lens = case.stream()
    x = torch.from_numpy(case.x).cuda()
    assert x.data_ptr() % 16 == 0
    _plan(torch, codec, x, tab, case)
    cap = codec.words_needed(case.bit_base, bits)
    assert cap == M.words_needed(case.bit_base, bits)
    out = _Out(torch, codec, case.n, case.S, case.shift, cap, fill)
    bit_base = torch.tensor([case.bit_base], dtype=torch.int64).cuda() if case.dev else case.bit_base
    codec.set_option("pack_grid", case.grid)
    try:
        codec.pack_async(x, tab, bit_base, out.words, out.sync, case.S)
        st = codec.pack_status(tab)
    finally:
        codec.set_option("pack_grid", 0)
    out.assert_words(case, case.word_bytes())
    out.assert_index(case, lens, base)
    assert st == 0, (case, st)
    # one decode of the device's own stream
    back = torch.full((case.n + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    codec.decode(out.words.clone(), case.bit_base, (out.sync[0].clone(), out.sync[1].clone()), case.S, case.n, tab,
                 back[:case.n])
    assert codec.decode_status() == 0, case
    assert np.array_equal(back[:case.n].cpu().numpy(), case.x), case


@pytest.mark.parametrize("fam", M.FAMILIES)
def test_pack_catalogue(torch_cuda, codec, dev_tables, fam):
    """every case into 0xFF; the stores family, and one case of every other, into zeros as well"""
    cases = M.family(fam)
    for case in cases:
        _run(torch_cuda, codec, case, dev_tables(case.tab))
    for case in cases if fam == "stores" else cases[:1]:
        _run(torch_cuda, codec, case, dev_tables(case.tab), fill=0)


@pytest.mark.parametrize("name", ("tail-4097", "sync-64-slow", "plan-65"))
def test_fused_plans_give_the_plan_total(torch_cuda, codec, name):
    """dc_huff_encode_plan and dc_huff_table_plan against hist -> table -> plan, and the oracle"""
    torch, case = torch_cuda, M.case(name)
    x = torch.from_numpy(case.x).cuda()
    h = orc.histogram(case.x)
    el, ev = orc.canonical(orc.huffman_lengths(h, 2), 2)
    _, nb, _ = orc.bitcodes(el[:256], ev[:256], 2)
    want = int((h * nb.astype(np.uint64)).sum())
    hist = codec.hist(x)
    assert int(codec.plan(codec.table(hist, 2)).item()) == want
    assert int(codec.encode_plan(x, 2)[2].item()) == want
    hist = codec.hist(x)
    assert int(codec.table_plan(hist, 2)[1].item()) == want


# ---- refused packs ---------------------------------------------------------------------------
def _refused(torch, codec, x, tab, nbits, bit_base, cap, S=64):
    """hist -> plan -> pack_async of x into `cap` words of 0xFF: (the buffers, the status, the words
    of the plan below cap)"""
    xd = torch.from_numpy(x).cuda()
    codec.hist(xd)
    _, _, off = M.plan_model(x, nbits)
    assert int(codec.plan(tab).item()) == int(off[-1])
    out = _Out(torch, codec, x.size, S, 0, cap, 0xFF)
    codec.pack_async(xd, tab, bit_base, out.words, out.sync, S)
    return out, xd, codec.pack_status(tab), M.boundary_words(off, bit_base, cap)


@pytest.mark.parametrize("bit_base", (0, 77))
def test_capacity_exact_and_one_word_short(torch_cuda, codec, dev_tables, bit_base):
    """words_cap = the words the stream touches (no slack): packed, nothing from words_cap on is
    touched. One word fewer: DC_E_CAPACITY from pack_status, no code bit and no index entry
    written; the plan kernels have zeroed the block-boundary words below words_cap (they run before
    the pack looks at its capacity), nothing else. dc_huff_pack, which reads the total first,
    refuses every capacity below dc_huff_words_needed and writes nothing at all."""
    torch, tab = torch_cuda, dev_tables("b16")
    x, _ = M.refused_input()
    case = M.Case("capacity-%d" % bit_base, "capacity", "b16", x, bit_base=bit_base)
    nw = M.words_touched(bit_base, case.bits)
    out, xd, st, _ = _refused(torch, codec, x, tab, M.table("b16")["nbits"], bit_base, nw)
    assert st == 0
    out.assert_words(case, case.word_bytes())
    out.assert_index(case, case.stream()[4], case.stream()[3])
    out, xd, st, zeroed = _refused(torch, codec, x, tab, M.table("b16")["nbits"], bit_base, nw - 1)
    assert st == M.DC_E_CAPACITY
    assert len(zeroed) == 3 and zeroed[0] == 0      # the three block starts; the last word is past words_cap
    out.assert_words(case, np.zeros(0, np.uint8), zero_words=zeroed)
    out.assert_index(case)
    # the synchronous call: its bound includes the decoder's slack
    need = codec.words_needed(bit_base, case.bits)
    for cap in (nw - 1, nw, need - 1):
        o = _Out(torch, codec, x.size, 64, 0, cap, 0xFF)
        rc = codec.L.dc_huff_pack(codec.ctx, xd.data_ptr(), x.size, tab.data_ptr(), bit_base, o.words.data_ptr(), cap,
                                  o.sync[0].data_ptr(), o.sync[1].data_ptr(), 64)
        assert rc == M.DC_E_CAPACITY, (cap, rc)
        o.assert_words(case, np.zeros(0, np.uint8))
        o.assert_index(case)
    # the status is the plan's: a pack refused for capacity leaves it at DC_E_CAPACITY for every
    # later pack of that plan, a new plan starts clean
    assert codec.pack_status(tab) == M.DC_E_CAPACITY
    codec.plan(tab)
    o = _Out(torch, codec, x.size, 64, 0, need, 0xFF)
    codec.pack(xd, tab, bit_base, o.words, o.sync, 64)
    assert codec.pack_status(tab) == 0
    o.assert_words(case, case.word_bytes())
    o.assert_index(case, case.stream()[4], case.stream()[3])


@pytest.mark.parametrize("bit_base", (0, 77))
def test_byte_without_a_code(torch_cuda, codec, dev_tables, bit_base):
    """A present byte whose length is 0: DC_E_NOCODE from dc_huff_pack (nothing written) and from
    pack_status after pack_async, which wrote no code bit and no index entry: only the plan's zeros
    in the block-boundary words (the offsets of the plan count the byte as 0 bits)."""
    torch, tab = torch_cuda, dev_tables("b16")
    _, bad = M.refused_input()
    nbits = M.table("b16")["nbits"]
    bits = int(M.plan_model(bad, nbits)[2][-1])
    cap = M.words_needed(bit_base, bits)
    out, xd, st, zeroed = _refused(torch, codec, bad, tab, nbits, bit_base, cap)
    assert st == M.DC_E_NOCODE
    assert len(zeroed) == 4 and zeroed[-1] == M.words_touched(bit_base, bits) - 1
    out.assert_words("nocode", np.zeros(0, np.uint8), zero_words=zeroed)
    out.assert_index("nocode")
    o = _Out(torch, codec, bad.size, 64, 0, cap, 0xFF)
    rc = codec.L.dc_huff_pack(codec.ctx, xd.data_ptr(), bad.size, tab.data_ptr(), bit_base, o.words.data_ptr(), cap,
                              o.sync[0].data_ptr(), o.sync[1].data_ptr(), 64)
    assert rc == M.DC_E_NOCODE
    o.assert_words("nocode", np.zeros(0, np.uint8))
    o.assert_index("nocode")


# ---- status ----------------------------------------------------------------------------------
def test_status_of_a_plan_outlives_thirty_later_plans(torch_cuda, codec, dev_tables):
    torch, tab = torch_cuda, dev_tables("b16")
    x, bad = M.refused_input()
    nbits = M.table("b16")["nbits"]
    cap = M.words_needed(0, int(M.plan_model(x, nbits)[2][-1]))
    out, _, st, _ = _refused(torch, codec, bad, tab, nbits, 0, cap)
    g = codec.plan_gen()
    assert st == M.DC_E_NOCODE and codec.pack_status(tab, g) == M.DC_E_NOCODE
    xd = torch.from_numpy(x).cuda()
    codec.hist(xd)
    gens = []
    for i in range(30):
        codec.plan(tab)
        gens.append(codec.plan_gen())
        assert gens[-1] == (g + i + 1) & 0xFFFFFFFF
        codec.pack_async(xd, tab, 0, out.words, out.sync, 64)
        assert codec.pack_status(tab) == 0 and codec.pack_status(tab, gens[-1]) == 0
    assert codec.pack_status(tab, g) == M.DC_E_NOCODE
    assert all(codec.pack_status(tab, gi) == 0 for gi in gens)
    codec.plan(tab)     # the 31st: g's flags are recycled
    assert codec.pack_status(tab, g) == M.DC_E_STATE
    assert codec.pack_status(tab) == 0 and codec.pack_status(tab, gens[0]) == 0


def test_pack_out_of_order_and_bad_arguments(torch_cuda, codec, dev_tables):
    torch, tab = torch_cuda, dev_tables("b16")
    x, _ = M.refused_input()
    case = M.Case("state", "state", "b16", x)
    xd, other = torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda()
    out = _Out(torch, codec, x.size, 64, 0, M.words_needed(0, case.bits), 0xFF)
    L, ctx = codec.L, codec.ctx

    def pack(fn, xp, n, base, lens, S, words=out.words.data_ptr()):
        return fn(ctx, xp, n, tab.data_ptr(), 0, words, out.cap, base, lens, S)

    b, l = out.sync[0].data_ptr(), out.sync[1].data_ptr()
    for fn in (L.dc_huff_pack_async, L.dc_huff_pack):
        codec.hist(xd)
        assert pack(fn, xd.data_ptr(), x.size, b, l, 64) == M.DC_E_STATE            # no plan
        codec.plan(tab)
        assert pack(fn, other.data_ptr(), x.size, b, l, 64) == M.DC_E_STATE         # another pointer
        assert pack(fn, xd.data_ptr(), x.size - 16, b, l, 64) == M.DC_E_STATE       # another n
        assert pack(fn, xd.data_ptr() + 16, x.size - 16, b, l, 64) == M.DC_E_STATE
        assert pack(fn, xd.data_ptr(), x.size, b, None, 64) == M.DC_E_ARG           # one index array alone
        assert pack(fn, xd.data_ptr(), x.size, None, l, 64) == M.DC_E_ARG
        for S in (8, 24, 2048):
            assert pack(fn, xd.data_ptr(), x.size, b, l, S) == M.DC_E_ARG
        assert pack(fn, xd.data_ptr(), x.size, b, l, 64, words=None) == M.DC_E_ARG
    codec.small_huff_plan(xd)                                                       # a front-end plan in between
    assert pack(L.dc_huff_pack_async, xd.data_ptr(), x.size, b, l, 64) == M.DC_E_STATE
    # an input pointer off 16 bytes is refused by the histogram, and the pack of it by its order
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    codec.hist(xd)
    codec.plan(tab)
    for d in (1, 4, 8):
        assert L.dc_huff_hist(ctx, xd.data_ptr() + d, x.size - 16, hist.data_ptr()) == M.DC_E_ARG
        assert pack(L.dc_huff_pack_async, xd.data_ptr() + d, x.size - 16, b, l, 64) == M.DC_E_STATE
    codec.sync()
    out.assert_words("refused", np.zeros(0, np.uint8))
    out.assert_index("refused")
    # the refused histogram left the state of the good one: its pack goes through
    assert pack(L.dc_huff_pack_async, xd.data_ptr(), x.size, b, l, 64) == 0
    assert codec.pack_status(tab) == 0
    out.assert_words(case, case.word_bytes())
    out.assert_index(case, case.stream()[4], case.stream()[3])


def test_two_packs_after_one_plan(torch_cuda, codec, dev_tables):
    torch, tab = torch_cuda, dev_tables("b16")
    case = M.case("base-77")
    x = torch.from_numpy(case.x).cuda()
    codec.hist(x)
    codec.plan(tab)
    outs = [_Out(torch, codec, case.n, 64, 0, M.words_needed(77, case.bits), fill) for fill in (0xFF, 0)]
    for o in outs:
        codec.pack_async(x, tab, 77, o.words, o.sync, 64)
    assert codec.pack_status(tab) == 0
    for o in outs:
        o.assert_words(case, case.word_bytes())
        o.assert_index(case, case.stream()[4], case.stream()[3])
    assert np.array_equal(outs[0].words.cpu().numpy()[: M.words_touched(77, case.bits)],
                          outs[1].words.cpu().numpy()[: M.words_touched(77, case.bits)])
