"""The fused C5 encode (k_hist_blocks<1, true>, the msym half of the plan kernels, k_fe_pack<false>) and
its two shard calls (dc_small_huff_shard_hist, dc_small_huff_shard_pack_async: k_fe_pack<true>), held
to tests/fe_pack_model.py at their own edges.

A case is an input and, for a shard, the four values of d_shard written by the test: the fused plan
(or the shard histogram followed by dc_huff_table_plan on the case's histogram), then the pack into a
view of a buffer of 0xFF (or zeros) with GW guard words on both sides, the sync arrays holding exactly
the documented entry counts inside poisoned buffers. Every case asserts the histogram, the plan
total, the symbol total, dc_huff_block_hist and dc_huff_plan_offsets entry for entry, every word the
stream owns and every word it does not, every index entry inside the documented counts and every one
outside, and the status; then the device's own stream is decoded (dc_small_huff_decode for a whole
stream, dc_huff_decode under the local index for a shard, under the stitched global index for the
stitched streams). Every buffer is larger than the capacity the call is given, so a wrong kernel
overwrites a guard of ours and never leaves the allocation; no case provokes a fault, and the bad
arguments are those the ABI refuses before any launch. What the catalogue reaches is asserted on the
CPU by tests/test_fe_pack_model_cpu.py; this file only runs it.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import fe_pack_model as M

pytestmark = pytest.mark.gpu

GW = 16384                      # guard words: more than the longest block codes to
GS = 64                         # guard entries of the index arrays
LEN_POISON, BASE_POISON = M.LEN_POISON, 0x5A5A5A5A5A5A5A5A


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


class _Index:
    """a u16 length array of exactly n16 entries and a u64 base array of ngr, inside poison"""

    def __init__(self, torch, n16, ngr):
        self.n16, self.ngr = n16, ngr
        self.lbuf = torch.full((2 * GS + n16,), LEN_POISON, dtype=torch.int16, device="cuda")
        self.bbuf = torch.full((2 * GS + ngr,), BASE_POISON, dtype=torch.int64, device="cuda")
        self.sync = (self.bbuf[GS: GS + ngr], self.lbuf[GS: GS + n16])
        assert self.sync[1].data_ptr() % 4 == 0

    def host(self):
        return self.lbuf.cpu().numpy().view(np.uint16), self.bbuf.cpu().numpy().view(np.uint64)

    def assert_guards(self, what):
        l, b = self.host()
        for got, k, poison in ((l, self.n16, LEN_POISON), (b, self.ngr, BASE_POISON)):
            assert (got[:GS] == poison).all() and (got[GS + k:] == poison).all(), (what, "index guard written")

    def assert_is(self, what, lens, base):
        """lens: all n16 entries as expected; base: the first entries, poison after them"""
        self.assert_guards(what)
        l, b = self.host()
        bad = np.nonzero(l[GS: GS + self.n16] != lens)[0]
        assert bad.size == 0, (what, "length entry", int(bad[0]), "of", self.n16, int(l[GS + bad[0]]), int(lens[bad[0]]))
        want = np.full(self.ngr, BASE_POISON, np.uint64)
        want[: base.size] = base
        bad = np.nonzero(b[GS: GS + self.ngr] != want)[0]
        assert bad.size == 0, (what, "base entry", int(bad[0]), "of", self.ngr, int(b[GS + bad[0]]), int(want[bad[0]]))


class _Out:
    """the guarded buffers of one pack"""

    def __init__(self, torch, case, cap):
        self.fill, self.shift, self.cap = case.fill, case.shift, cap
        self.buf = torch.full((2 * GW + 4 + cap,), -1 if case.fill else 0, dtype=torch.int32, device="cuda")
        self.words = self.buf[GW + case.shift: GW + case.shift + cap]
        assert self.buf.data_ptr() % 16 == 0 and (self.words.data_ptr() % 16 == 0) == (case.shift % 4 == 0)
        self.local = _Index(torch, *M.sync_entries(case.n, case.S, False))
        self.glob = _Index(torch, *M.sync_entries(case.n, case.S, True)) if case.shard else None

    def word_bytes(self, nbytes):
        lo = 4 * (GW + self.shift)
        return self.buf.cpu().numpy().view(np.uint8)[lo: lo + nbytes].copy()

    def assert_words(self, what, want):
        h = self.buf.cpu().numpy().view(np.uint8).copy()
        lo = 4 * (GW + self.shift)
        bad = np.nonzero(h[lo: lo + want.size] != want)[0]
        assert bad.size == 0, (what, "first wrong word", int(bad[0]) // 4, "of", want.size // 4, bad.size, "bytes")
        h[lo: lo + want.size] = self.fill
        bad = np.nonzero(h != self.fill)[0]
        assert bad.size == 0, (what, "written outside the stream: word", (int(bad[0]) - lo) // 4, "of the view;",
                               bad.size, "bytes")

    def assert_guards(self, what):
        h = self.buf.cpu().numpy().view(np.uint8)
        lo = 4 * (GW + self.shift)
        assert (h[:lo] == self.fill).all() and (h[lo + 4 * self.cap:] == self.fill).all(), (what, "word guard written")
        self.local.assert_guards(what)
        if self.glob:
            self.glob.assert_guards(what)


def _plan_state(codec, case, e):
    """after the pack: the symbol total, the block histograms and the block bit offsets are the model's"""
    assert codec.small_huff_symbols() == e["m"].size, case
    bh = e["bh"].astype(np.uint16).reshape(-1)
    got = np.zeros(bh.size, np.uint16)
    assert codec.L.dc_huff_block_hist(codec.ctx, got.ctypes.data, got.size) == 0
    bad = np.nonzero(got != bh)[0]
    assert bad.size == 0, (case, "block histogram: block", int(bad[0]) // 256, "byte", int(bad[0]) % 256)
    off = e["off"]
    got_off, hn = np.zeros(off.size, np.uint64), C.c_uint64(0)
    assert codec.L.dc_huff_plan_offsets(codec.ctx, got_off.ctypes.data, got_off.size, C.byref(hn)) == 0
    assert hn.value == off.size
    bad = np.nonzero(got_off != off)[0]
    assert bad.size == 0, (case, "plan offsets: entry", int(bad[0]), int(got_off[bad[0]]), int(off[bad[0]]))


def _padded(torch, codec, wb, bit, bits):
    """the stream's words with the decoder's slack after them"""
    w = torch.zeros(codec.words_needed(bit, bits), dtype=torch.int32, device="cuda")
    w[: wb.size // 4] = torch.from_numpy(wb.view(np.int32).copy()).cuda()
    return w


def _run(torch, codec, case):
    """One case end to end. Returns (table, what stitch() takes of the device's output), or None for
    a case whose status is DC_E_FALLBACK."""
    e = case.expected()
    bit, sym, lb, rb = case.ctx
    x = torch.from_numpy(case.x.copy()).cuda()
    assert x.data_ptr() % 16 == 0
    want_hist = e["hist"].astype(np.int64)
    if case.shard:
        shard = torch.tensor(case.ctx, dtype=torch.int64).cuda()
        hist = codec.small_shard_hist(x, shard)
        tab, total = codec.table_plan(torch.from_numpy(case.table_hist().astype(np.int64)).cuda(), case.n_ary)
    else:
        hist, tab, total = codec.small_huff_plan(x, case.n_ary)
    assert np.array_equal(hist.cpu().numpy(), want_hist), (case, "histogram of M")
    assert int(total.item()) == e["bits"], (case, "plan total", int(total.item()), e["bits"])
    nw = M.words_touched(bit, e["bits"])
    cap = nw if case.exact_cap else codec.words_needed(bit, e["bits"])
    out = _Out(torch, case, cap)
    codec.set_option("pack_grid", case.grid)
    try:
        if case.shard:
            codec.small_shard_pack_async(x, tab, shard, out.words, out.local.sync, out.glob.sync, case.S)
        else:
            codec.small_huff_pack_async(x, tab, bit, out.words, out.local.sync, case.S)
        st = codec.pack_status(tab)
    finally:
        codec.set_option("pack_grid", 0)
    assert st == case.status(), (case, st, case.geometry()["reasons"])
    _plan_state(codec, case, e)
    if st:
        out.assert_guards(case)
        return None
    out.assert_words(case, e["word_bytes"])
    out.local.assert_is(case, M.expected_len_array(e, out.local.n16, False), e["base"])
    if case.shard:
        out.glob.assert_is(case, M.expected_len_array(e, out.glob.n16, True), e["gbase"])
    # a decode of the device's own stream
    m = e["m"].size
    w = _padded(torch, codec, out.word_bytes(4 * nw), bit, e["bits"])
    sync = (out.local.sync[0][: e["base"].size].clone(), out.local.sync[1][: e["lens"].size].clone())
    if case.shard:
        back = torch.full((m + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        codec.decode(w, bit, sync, case.S, m, tab, back[:m])
        assert codec.decode_status() == 0, case
        assert np.array_equal(back[:m].cpu().numpy(), e["m"]), (case, "decode under the local index")
        gl, gb = out.glob.host()
        return tab, {"bit": bit, "bits": e["bits"], "sym": sym, "nsym": m, "S": case.S, "word_bytes": out.word_bytes(4 * nw),
                     "glens": gl[GS: GS + e["glens"].size], "gbase": gb[GS: GS + e["gbase"].size]}
    enc = {"words": w, "bit_base": bit, "sync": sync, "S": case.S, "n": m, "table": tab}
    # (the oracle's inverse of M: the input itself unless it holds a raw byte >= 0x80, which decodes as a pair)
    want = np.frombuffer(orc.small_decompress(e["m"].tobytes()), np.uint8)
    assert np.array_equal(codec.small_huff_decode(enc).cpu().numpy(), want), (case, "dc_small_huff_decode")
    return tab, None


@pytest.mark.parametrize("fam", M.FAMILIES)
def test_fe_catalogue(torch_cuda, codec, fam):
    for case in M.family(fam):
        _run(torch_cuda, codec, case)


def test_fe_stitched(torch_cuda, codec):
    """every part through the two shard calls; the parts' words, u16 parts and group bases stitched
    with no process group are the whole stream's, and decode under the stitched global index"""
    torch = torch_cuda
    for s in M.stitched():
        runs = [_run(torch, codec, p) for p in s.parts]
        tab = runs[-1][0]
        wb, bits, lens, base = M.stitch([r[1] for r in runs])
        e = s.whole.expected()
        assert bits == e["bits"] and np.array_equal(wb, e["word_bytes"]), s
        assert np.array_equal(lens, e["lens"]) and np.array_equal(base, e["base"]), s
        m = e["m"].size
        back = torch.full((m + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        sync = (torch.from_numpy(base.view(np.int64).copy()).cuda(), torch.from_numpy(lens.view(np.int16).copy()).cuda())
        codec.decode(_padded(torch, codec, wb, e["bit"], bits), e["bit"], sync, s.whole.S, m, tab, back[:m])
        assert codec.decode_status() == 0, s
        assert np.array_equal(back[:m].cpu().numpy(), e["m"]), (s, "decode under the stitched index")


# ---- state -----------------------------------------------------------------------------------
def test_fe_refused_arguments_and_order(torch_cuda, codec):
    torch, L, ctx = torch_cuda, codec.L, codec.ctx
    case = M.case("cuts-space|letter")
    e = case.expected()
    x, other = torch.from_numpy(case.x.copy()).cuda(), torch.from_numpy(case.x.copy()).cuda()
    out = _Out(torch, case, M.words_touched(0, e["bits"]))
    sh = M.Case("state-shard", "state", case.x, ctx=(0, 0, -1, -1))
    gout = _Out(torch, sh, out.cap)
    shard = torch.tensor(sh.ctx, dtype=torch.int64).cuda()
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    tab, tot = codec.alloc_table(), torch.zeros(1, dtype=torch.int64, device="cuda")
    b, l = out.local.sync[0].data_ptr(), out.local.sync[1].data_ptr()
    gb, gl = gout.glob.sync[0].data_ptr(), gout.glob.sync[1].data_ptr()

    def plan(n=case.n, msv=258):
        return L.dc_small_huff_plan(ctx, x.data_ptr(), n, msv, 2, hist.data_ptr(), tab.data_ptr(), tot.data_ptr())

    def pack(xp=x.data_ptr(), n=case.n, lens=l):
        return L.dc_small_huff_pack_async(ctx, xp, n, tab.data_ptr(), 0, out.words.data_ptr(), out.cap, b, lens, case.S)

    def spack(lens=l, glens=gl):
        return L.dc_small_huff_shard_pack_async(ctx, x.data_ptr(), case.n, tab.data_ptr(), shard.data_ptr(),
                                                out.words.data_ptr(), out.cap, b, lens, gb, glens, case.S)

    for n in (0, 1):
        assert plan(n=n) == M.DC_E_FALLBACK
        assert L.dc_small_huff_shard_hist(ctx, x.data_ptr(), n, shard.data_ptr(), hist.data_ptr()) == M.DC_E_FALLBACK
    for msv in (0, 254):
        assert plan(msv=msv) == M.DC_E_ARG
    assert plan() == 0
    assert pack(lens=l + 2) == M.DC_E_ARG and spack(lens=l + 2) == M.DC_E_ARG and spack(glens=gl + 2) == M.DC_E_ARG
    assert pack(xp=other.data_ptr()) == M.DC_E_STATE and pack(n=case.n - 16) == M.DC_E_STATE
    # after a plain histogram and plan: not the front-end's
    codec.hist(x)
    codec.plan(tab)
    assert pack() == M.DC_E_STATE and spack() == M.DC_E_STATE
    # a front-end histogram with no plan after it
    codec.small_shard_hist(x, shard)
    assert pack() == M.DC_E_STATE and spack() == M.DC_E_STATE
    codec.sync()
    out.assert_words("refused", np.zeros(0, np.uint8))
    for o in (out.local, gout.glob):
        l16, b64 = o.host()
        assert (l16 == LEN_POISON).all() and (b64 == BASE_POISON).all()
    # the refused calls left the context usable: the plan and pack go through
    assert plan() == 0 and pack() == 0 and codec.pack_status(tab) == 0
    out.assert_words(case, e["word_bytes"])
    out.local.assert_is(case, M.expected_len_array(e, out.local.n16, False), e["base"])


def test_fe_two_packs_after_one_plan(torch_cuda, codec):
    torch = torch_cuda
    case = M.case("sync-64-boundary-parities")
    e = case.expected()
    x = torch.from_numpy(case.x.copy()).cuda()
    _, tab, _ = codec.small_huff_plan(x, case.n_ary)
    outs = []
    for fill in (0xFF, 0):
        c = M.Case("two", "state", case.x, S=case.S, fill=fill)
        outs.append(_Out(torch, c, M.words_touched(0, e["bits"])))
        codec.small_huff_pack_async(x, tab, 0, outs[-1].words, outs[-1].local.sync, case.S)
    assert codec.pack_status(tab) == 0
    for o in outs:      # the second pack's plan zeroed the shared dwords again before it added
        o.assert_words(case, e["word_bytes"])
        o.local.assert_is(case, M.expected_len_array(e, o.local.n16, False), e["base"])
