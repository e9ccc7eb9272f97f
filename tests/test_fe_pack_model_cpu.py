"""tests/fe_pack_model.py against the oracle, and the reach of its case catalogue (no GPU).

The model is what tests/test_gpu_fe_edges.py holds the fused C5 encode and its two shard calls to.
Here it is pinned to the oracle (the symbols of every cutting are orc.small_compress, every expected
stream decodes back through orc.huff_unpack, every stitched case is its whole stream), and the
*_reach_* tests assert from geometry() that the catalogue has been on every row of the edge table in
DESIGN.md section 6 ("The fused C5 encode and its shard calls at their own edges"), so the GPU file
only has to run the cases. What the geometry shows unreachable is asserted unreachable."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import fe_pack_model as M

X, Q, SP = M.X, M.Q, M.SPACE
HQ = 0x80 | Q


def _blocks(c, **kw):
    return c.geometry(**kw)["blocks"]


def _all_cases():
    return M.catalogue() + [p for s in M.stitched() for p in s.parts]


# ---- the model against the oracle ------------------------------------------------------------
def test_symbols_of_every_whole_stream_are_the_oracles():
    seen = 0
    for c in M.catalogue():
        if c.shard:
            continue
        fe = orc.small_compress(c.x.tobytes())
        if c.geometry()["reasons"]["literal"]:
            assert fe == b" " + c.x.tobytes(), c
            continue
        assert M.stream_symbols(c.x).tobytes() == fe, c
        seen += 1
    assert seen >= 40


def test_symbols_of_every_cutting_are_the_oracles():
    for s in M.stitched():
        got = b"".join(M.stream_symbols(p.x, p.ctx[2], p.ctx[3]).tobytes() for p in s.parts)
        assert got == orc.small_compress(s.whole.x.tobytes()), s
        # the contexts: each part starts at the bit and symbol where the one before it ended
        for a, b in zip(s.parts, s.parts[1:]):
            ea = a.expected()
            assert (b.ctx[0], b.ctx[1]) == (a.ctx[0] + ea["bits"], a.ctx[1] + ea["m"].size), (s, a)


def test_every_two_way_cut_of_a_short_stream_is_the_oracles():
    x = M.case("ends-pair-at-1-2").x[:64]
    fe = orc.small_compress(x.tobytes())
    assert fe[0] == 8
    for k in range(2, x.size - 1):
        got = M.stream_symbols(x[:k], -1, int(x[k])).tobytes() + M.stream_symbols(x[k:], int(x[k - 1]), -1).tobytes()
        assert got == fe, k


@pytest.mark.parametrize("fam", M.FAMILIES + ("stitched",))
def test_expected_streams_decode_back_and_histograms_sum(fam):
    cases = M.family(fam) if fam != "stitched" else [p for s in M.stitched() for p in s.parts]
    for c in cases:
        e = c.expected()
        payload, bit, bits = e["word_bytes"], c.ctx[0] & 31, e["bits"]
        payload = np.packbits(np.unpackbits(payload)[bit: bit + bits])
        assert np.array_equal(orc.huff_unpack(payload, bits, e["m"].size, e["enc_len"], e["enc_val"], e["n_ary"]), e["m"]), c
        assert np.array_equal(e["bh"].sum(axis=0).astype(np.uint64), orc.histogram(e["m"])), c
        assert int(e["lens"].astype(np.int64).sum()) == bits == int(e["glens"].sum()), c
        g = c.geometry()
        assert (g["total"], g["mtot"]) == (bits, e["m"].size), c
        # the plan's offsets are the bit of each block's first symbol
        sb = e["nbits"][e["m"]]
        at = np.concatenate([[0], np.cumsum(sb)])
        assert np.array_equal(at[e["msym"]], e["off"].astype(np.int64)), c


def test_stitched_cases_are_their_whole_streams():
    assert len(M.stitched()) >= 20 and {len(s.parts) for s in M.stitched()} == {2, 3, 4}
    for s in M.stitched():
        w, bits, lens, base = M.stitch([p.expected() for p in s.parts])
        e = s.whole.expected()
        assert bits == e["bits"] and np.array_equal(w, e["word_bytes"]), s
        assert np.array_equal(lens, e["lens"]) and np.array_equal(base, e["base"]), s
        assert all(p.n >= 2 and p.status() == 0 for p in s.parts)


def test_stitched_reach_cuts_inside_a_pair_before_a_space_after_a_letter_and_at_the_ends():
    kinds = set()
    for s in M.stitched():
        x = s.whole.x
        y = M.symbols(x)
        for k in s.cuts:
            if y[k - 1] < 0:
                kinds.add("inside a pair")
            if y[k] < 0:
                kinds.add("before a pair's space")
            if k >= 2 and y[k - 2] < 0:
                kinds.add("after a pair's letter")
            for name, v in (("byte 2", 2), ("n - 2", x.size - 2), ("block - 1", M.BLOCK - 1), ("block + 1", M.BLOCK + 1)):
                if k == v:
                    kinds.add(name)
    assert kinds == {"inside a pair", "before a pair's space", "after a pair's letter", "byte 2", "n - 2", "block - 1",
                     "block + 1"}


# ---- what the plan zeroes, what the pack adds ------------------------------------------------
def test_every_atomic_add_lands_in_a_dword_the_plan_zeroed_and_no_plain_store_does():
    """k_fe_pack adds into the dwords hd and td of each block and stores every other length plainly;
    k_block_final_wide zeroes one dword per block boundary. They must be the same dwords, for the
    local and for the global array; UNREACHABLE: a dword with a plain store in one half and an add
    in the other (the issue's "other half belongs to the neighbouring block's plain store")."""
    for c in _all_cases():
        g = c.geometry()
        for pre, sym in (("", None),) + ((("g", c.ctx[1]),) if c.shard else ()):
            c0e = ((c.ctx[1] // c.S) & ~1) if pre else 0
            zeroed = set(M.zeroed_dwords(g["msym"], c.S, sym))
            added, stored = set(), set()
            for r in g["blocks"]:
                added |= {(ch - c0e) >> 1 for ch in r[pre + "atomic"]}
                if r[pre + "tail_add"] is not None:
                    assert r[pre + "tail_add"] >= c0e, (c, r["b"])
                    added.add((r[pre + "tail_add"] - c0e) >> 1)
                stored |= {(ch - c0e) >> 1 for ch in r[pre + "plain"]}
            assert added <= zeroed, (c, pre, sorted(added - zeroed))
            assert not (stored & zeroed), (c, pre, sorted(stored & zeroed))


def test_documented_index_sizes_hold_every_entry_written():
    for c in _all_cases():
        e = c.expected()
        n16, ngr = M.sync_entries(c.n, c.S, False)
        assert e["lens"].size <= n16 - 2 and 2 * max(M.zeroed_dwords(e["msym"], c.S)) + 2 <= n16 and e["base"].size <= ngr, c
        if c.shard:
            n16, ngr = M.sync_entries(c.n, c.S, True)
            assert e["glens"].size <= n16 - 2 and e["gbase"].size <= ngr, c
            assert 2 * max(M.zeroed_dwords(e["msym"], c.S, c.ctx[1])) + 2 <= n16, c


# ---- ends ------------------------------------------------------------------------------------
def test_ends_reach_every_size_and_the_streams_first_and_last_bytes():
    assert {c.n for c in M.family("ends")} >= {2, 3, 15, 16, 17, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65537}
    for n in (2, 3):
        assert M.case("ends-n%d" % n).geometry()["reasons"]["literal"]
    y = lambda name: M.symbols(M.case(name).x)
    assert y("ends-last-space")[-1] == SP                         # a symbol: nothing follows
    assert list(y("ends-space-letter-at-0")[:2]) == [SP, Q]       # no pair at 0-1
    assert list(y("ends-pair-at-1-2")[:3]) == [X, -1, HQ]
    assert list(y("ends-two-spaces-letter")[:4]) == [X, SP, -1, HQ]
    assert y("ends-high-first-byte")[0] == 0xE1
    full = [r["full"] for c in M.family("ends") for r in _blocks(c)]
    assert True in full and False in full


# ---- cuts ------------------------------------------------------------------------------------
CUT_WANT = {"space|letter": ([-1, HQ], 1), "pair-starts-on": ([-1, HQ], 0), "pair-ends-before": ([-1, HQ], 2),
            "space|other": ([SP, ord("Q")], 1)}


def test_cuts_reach_every_pattern_on_every_boundary_in_a_full_and_in_the_partial_block():
    for pat, (want, k) in CUT_WANT.items():
        c = M.case("cuts-" + pat)
        y = M.symbols(c.x)
        g = _blocks(c)
        assert [r["full"] for r in g] == [True, False]
        assert {b for b, _ in c.sites} == {"dword", "lane", "wave", "piece", "block"} and len(c.sites) == 9
        for (bname, e), _ in c.sites.items():
            width = {"dword": 4, "lane": 16, "wave": 1024, "piece": 4096, "block": 32768}[bname]
            nxt = {"dword": 16, "lane": 1024, "wave": 4096, "piece": 32768, "block": 1 << 30}[bname]
            assert e % width == 0 and e % nxt != 0, (pat, bname, e)
            assert list(y[e - k: e - k + 2]) == want and y[e - k - 1] == X and y[e - k + 2] == X, (pat, bname, e)
    # which block counts a pair that straddles the block cut: the letter's
    c = M.case("cuts-space|letter")
    bh = M.block_hists(c.x)
    yb = M.symbols(c.x)
    assert yb[M.BLOCK] == HQ and bh[1, HQ] == (yb[M.BLOCK:] == HQ).sum() and bh[0, HQ] == (yb[:M.BLOCK] == HQ).sum()
    y = M.symbols(M.case("cuts-both-ends-of-a-lane").x)
    for e in (2064, M.BLOCK + 2064):
        assert list(y[e - 1: e + 17]) == [-1, HQ] + [X] * 14 + [-1, HQ]
    c = M.case("cuts-dense-block")
    r = _blocks(c)[1]
    assert r["m1"] - r["m0"] == M.BLOCK // 2 and (r["Ck"] == 8).all()


# ---- sync ------------------------------------------------------------------------------------
def test_sync_reach_a_chunk_start_on_a_pieces_first_and_last_symbol_at_every_S():
    for S in M.SYNCS:
        st = [s for r in _blocks(M.case("sync-%d-text" % S)) for s in r["starts"]]
        assert any(j0 == 0 for _, _, j0, Ck in st) and any(j0 == Ck - 1 for _, _, j0, Ck in st), S
        assert {k for k, _, _, _ in st} == set(range(8)) or S == 1024
    st = _blocks(M.case("sync-16-j0-0-and-15"))[0]["starts"]
    assert {(j0, Ck) for _, _, j0, Ck in st} >= {(0, 16), (15, 16), (0, 15)}


def test_sync_two_chunk_starts_in_one_piece_are_unreachable():
    """a piece holds at most 16 symbols and S >= 16: j0 + S < Ck never holds"""
    for c in _all_cases():
        for r in _blocks(c):
            assert not r["two_in_a_piece"] and not r.get("gtwo_in_a_piece", False), c
            assert r["Ck"].max() <= 16


def test_sync_reach_both_halves_of_a_dword_added_by_two_blocks():
    for name in ("sync-1024-boundary-parities", "sync-64-boundary-parities"):
        g = _blocks(M.case(name))
        par = {r["tail_add"] & 1 for r in g if r["tail_add"] is not None}
        assert par == {0, 1}, name
    g = _blocks(M.case("sync-1024-boundary-parities"))
    assert (g[-1]["nc"], g[-1]["hd"] == g[-1]["td"], g[-1]["full"]) == (0, True, False)      # a last block inside one chunk
    # an atomic add to the head dword and a different tail dword in one block, and plain stores between
    r = _blocks(M.case("sync-64-boundary-parities"))[1]
    assert r["hd"] != r["td"] and r["plain"] and {c >> 1 for c in r["atomic"]} <= {r["hd"], r["td"]}


def test_sync_reach_chunk_counts_around_the_groups_and_an_odd_count():
    for S in (16, 64):
        for cnt in (63, 64, 65, 127, 128, 129):
            e = M.case("sync-%d-chunks%d" % (S, cnt)).expected()
            assert e["m"].size == cnt * S and e["lens"].size == cnt and e["base"].size == -(-cnt // 64)
        assert M.case("sync-%d-n-1" % S).expected()["lens"].size == 64
        assert M.case("sync-%d-n+1" % S).expected()["lens"].size == 65
    assert {c.S for c in M.family("sync")} == set(M.SYNCS)


# ---- fit -------------------------------------------------------------------------------------
def test_fit_reach_both_sides_of_lim_at_each_sh_and_first_bit():
    """at S = 16, in the shard call (two lists beside the stage, 5-bit codes) and in the whole-stream
    call (one list, 7-bit codes): block 1 takes lim - sh words and fits, or one more and does not"""
    seen = set()
    for c in M.family("fit"):
        g = c.geometry()
        nb = c.expected()["nbits"]
        if c.shard:
            assert set(nb[M.FIT_ALPHABET]) == {5} and (nb > 0).sum() == 31 and g["z"] == 0
            assert g["lim"] == M.FIT_LIM2 == 5112 and g["cbw"] == 2050
        else:
            assert set(nb[nb > 0]) == {7} and (nb > 0).sum() == 127 and g["z"] == M.SPACE and not g["reasons"]["literal"]
            assert set(c.table_hist()[nb > 0]) == {M.FIT_COUNT}
            assert g["lim"] == M.FIT_LIM1 == 7162 and g["cbw"] == 2050
        r0, r1 = g["blocks"][:2]
        assert r0["fits"] and r0["full"] and r1["full"] and all(r["fits"] for r in g["blocks"][2:])
        over = r1["nw_blk"] + r1["sh"] - g["lim"]
        assert over in (0, 1) and r1["fits"] == (over == 0) and g["fallback"] == (over == 1), c
        assert c.status() == (M.DC_E_FALLBACK if over else 0)
        seen.add((c.k, r1["sh"], r1["abs31"], over))
    assert seen == {(k, sh, f, o) for k in (1, 2) for sh in range(4) for f in (0, 1, 31) for o in (0, 1)}


# ---- shard -----------------------------------------------------------------------------------
def test_shard_reach_the_first_symbol_and_first_bit_residues():
    S = 64
    got = {c.name: c for c in M.family("shard")}
    assert got["shard-sym-0modS"].ctx[1] % S == 0 and got["shard-sym-1modS"].ctx[1] % S == 1
    assert got["shard-sym-Sm1modS"].ctx[1] % S == S - 1
    assert (got["shard-chunk-even"].ctx[1] // S) % 2 == 0 and (got["shard-chunk-odd"].ctx[1] // S) % 2 == 1
    assert [got["shard-sym-" + k].ctx[1] % (64 * S) for k in ("0mod64S", "64S-1", "64S+1")] == [0, 64 * S - 1, 1]
    # the group base a shard owns: the one at its first symbol, none for a symbol later
    assert got["shard-sym-0mod64S"].expected()["g0"] == 1 and got["shard-sym-0mod64S"].expected()["gbase"].size >= 1
    assert got["shard-sym-64S+1"].expected()["g0"] == 2
    assert {c.ctx[0] % 32 for c in M.family("shard") if c.name.startswith("shard-bit-")} == {0, 1, 31, 5}
    assert any(c.ctx[0] == (1 << 33) + 5 for c in M.family("shard"))
    # an odd first chunk: entry 0 of the global array is the chunk before it, zeroed by the plan
    e = got["shard-chunk-odd"].expected()
    assert e["c0"] - e["c0e"] == 1 and M.expected_len_array(e, 2048, True)[0] == 0
    e = got["shard-S1024-sym-odd-chunk-0modS"].expected()
    assert e["c0"] & 1 and e["sym"] % 1024 == 0 and M.expected_len_array(e, 2048, True)[0] == 0


def test_shard_reach_every_pair_of_bytes_across_both_ends():
    lefts = {}
    for lname, lb in (("start", -1), ("space", SP), ("letter", Q), ("other", X)):
        for fname, fb in (("letter", Q), ("space", SP), ("other", X)):
            c = M.case("shard-before-%s-first-%s" % (lname, fname))
            assert (c.ctx[2], int(c.x[0])) == (lb, fb)
            lefts[(lname, fname)] = int(M.symbols(c.x, c.ctx[2], c.ctx[3])[0])
    assert lefts[("space", "letter")] == HQ and lefts[("start", "letter")] == Q and lefts[("letter", "letter")] == Q
    assert lefts[("start", "space")] == SP                   # position 0 of the stream starts no pair
    assert lefts[("space", "space")] == lefts[("other", "space")] == -1
    assert all(v == X for (l, f), v in lefts.items() if f == "other")
    rights = {}
    for tname, tb in (("space", SP), ("other", X)):
        for aname, rb in (("none", -1), ("letter", Q), ("other", X)):
            c = M.case("shard-last-%s-after-%s" % (tname, aname))
            assert (int(c.x[-1]), c.ctx[3]) == (tb, rb)
            rights[(tname, aname)] = int(M.symbols(c.x, c.ctx[2], c.ctx[3])[-1])
            code = M.D.codes(c.lengths(), c.n_ary)[0]
            assert code[SP] != 0 and code[X] == 0          # a space coded where none belongs sets a bit
    assert rights == {("space", "none"): SP, ("space", "letter"): -1, ("space", "other"): SP, ("other", "none"): X,
                      ("other", "letter"): X, ("other", "other"): X}


def test_shard_reach_two_bytes_one_chunk_and_the_zero_symbol_block():
    c = M.case("shard-2-bytes-pair-both-sides")
    assert list(M.symbols(c.x, c.ctx[2], c.ctx[3])) == [HQ, -1] and c.expected()["m"].size == 1
    r = _blocks(c)[0]
    assert (r["gnc"], r["gtail_add"], r["nc"]) == (0, 1, 1)       # symbol 127 of chunk 1: its last
    c = M.case("shard-inside-one-chunk")
    assert all(r["gnc"] == 0 and r["ghd"] == r["gtd"] for r in _blocks(c)) and c.n < c.S
    for name, on in (("shard-zero-symbol-block-on-a-word", True), ("shard-zero-symbol-block-off-a-word", False)):
        c = M.case(name)
        g = c.geometry()
        r = g["blocks"][-1]
        assert (r["n"], r["zero_symbols"], r["s_bits"], r["starts_on_word"]) == (1, True, 0, on)
        assert r["nw_blk"] == (0 if on else 1) and (r["nc"], r["gnc"]) == (0, 0)
        assert r["words"][0] == (g["nwords"] if on else g["nwords"] - 1)
    # UNREACHABLE in the whole-stream call: nothing follows its last byte, so its space is a symbol
    assert all(not r["zero_symbols"] for c in M.catalogue() if not c.shard for r in _blocks(c))


def test_no_block_touches_a_word_at_or_past_the_streams_word_count():
    """With thread 0's OR of the block's first word guarded by nw_blk > 0. Without the guard (the
    kernel as it was) the zero-symbol last block that starts on a word boundary ORs zero into the
    word at index = the stream's word count, which words_cap need not hold: no comparison of bytes
    sees an OR of zero, so the model says it. (geometry's `guard` restates the kernel's line by hand:
    this test does not fail if the kernel loses its guard; it records which case reaches the word.)"""
    hit = []
    for c in _all_cases():
        for r in _blocks(c):
            assert r["past_end"] == [], (c, r["b"])
        hit += [c.name for r in _blocks(c, guard=False) if r["past_end"]]
    assert "shard-zero-symbol-block-on-a-word" in hit and "shard-zero-symbol-block-off-a-word" not in hit
    c = M.case("shard-zero-symbol-block-on-a-word")
    assert _blocks(c, guard=False)[-1]["past_end"] == [c.geometry()["nwords"]]


# ---- stores, seq, plan, fallback ---------------------------------------------------------------
def test_stores_reach_every_output_shift_tail_and_the_one_word_block():
    assert {(c.shift, c.fill) for c in M.family("stores")} >= {(s, f) for s in range(4) for f in (0, 0xFF)}
    tails = {r["tail"] for c in M.family("stores") + M.family("ends") + M.family("sync") for r in _blocks(c) if "tail" in r}
    assert tails >= {0, 1, 2, 3}
    heads = {r["head"] for c in M.catalogue() for r in _blocks(c) if "head" in r}
    assert heads >= {0, 1, 2, 3}
    assert any(not g["vec_out"] for g in (c.geometry() for c in M.family("stores")))
    nw = {r["nw_blk"] for c in M.catalogue() for r in _blocks(c)}
    assert {0, 1, 2} <= nw
    assert _blocks(M.case("stores-one-word"))[0]["one_word"]
    ends = {(r["ends_on_word"], r["last_or"]) for c in M.catalogue() for r in _blocks(c)}
    assert {(True, False), (False, True), (False, False)} <= ends


def test_seq_reach_the_planted_orders_under_each_grid():
    """sh 3 -> 0 -> 2 (stage words 0..2 unused, then used) and a block ending mid-word -> one ending on
    a word (the stage's last word OR-ed and cleared by t == 64, then stored plainly), each run by one
    workgroup in a row; by default a workgroup runs two blocks, so the three steps reach it as pairs"""
    for name in M.SEQS:
        for g in M.SEQ_GRIDS:
            c = M.case("seq-%s-grid%d" % (name, g))
            b = _blocks(c)
            runs, nblocks = M.seq_runs(name, g)
            assert len(b) == nblocks and all(r["fits"] and r["full"] for r in b) and c.status() == 0
            for ps, steps in runs:
                for i, p in enumerate(ps[1:]):
                    assert b[p]["before"][-1] == ps[i] and b[p]["wg"] == b[ps[i]]["wg"], (c, p)     # in a row
                got = [(b[p]["sh"], b[p]["abs31"], b[p]["ends_on_word"], b[p]["last_or"]) for p in ps]
                if name == "sh-3-0-2":
                    want = {(96, None): 3, (0, None): 0, (64, None): 2}
                    assert [v[0] for v in got] == [want[s] for s in steps] and all(v[1] == 0 for v in got), (c, got)
                else:
                    assert [(v[2], v[3]) for v in got] == [(False, True), (True, False)], (c, got)
                    assert b[ps[0]]["nwa"] > 4 and b[ps[1]]["last_plain"] == b[ps[1]]["nwa"]
    full = [[r["sh"] for r in _blocks(M.case("seq-sh-3-0-2-grid%d" % g))[1::g]][:3] for g in (1, 2)]
    assert full == [[3, 0, 2], [3, 0, 2]]


def test_seq_reach_what_one_workgroup_runs_in_a_row():
    for g, want in ((1, [[], [0], [0, 1], [0, 1, 2], [0, 1, 2, 3]]), (2, [[], [], [0], [1], [0, 2]]), (0, [[], [], [], [0], [1]])):
        assert [r["before"] for r in _blocks(M.case("seq-long-short-grid%d" % g))] == want
    r = _blocks(M.case("seq-long-short-grid1"))
    assert r[0]["s_bits"] > 2 * r[1]["s_bits"] and r[2]["s_bits"] > 2 * r[3]["s_bits"]          # long -> short -> long -> short
    assert len({b["sh"] for b in r}) >= 3 and {b["ends_on_word"] for c in M.family("seq") for b in _blocks(c)} == {True, False}
    for g in M.SEQ_GRIDS:
        b = _blocks(M.case("seq-fits-over-fits-zero-grid%d" % g))
        assert [x["fits"] for x in b] == [True, False, True, True] and b[3]["zero_symbols"]
    assert _blocks(M.case("seq-fits-over-fits-zero-grid1"))[3]["before"] == [0, 1, 2]


def test_plan_reach_the_second_and_third_workgroup_and_a_block_of_one_symbol():
    for nb, wgs in ((65, 2), (129, 3)):
        c = M.case("plan-%d-blocks" % nb)
        e = c.expected()
        assert e["bh"].shape[0] == nb and -(-nb // M.PLAN_WG_BLOCKS) == wgs
        assert len({int(v) for v in np.diff(e["msym"])}) > 2         # the blocks differ: cbase is a real sum
    e = M.case("plan-32768-of-one").expected()
    assert e["bh"][0, X] == 32768 and e["bh"][0, 8] == 1 and e["msym"][1] == 32769


def test_fallback_reach_each_reason():
    r = lambda name: {k for k, v in M.case(name).geometry()["reasons"].items() if v}
    assert r("fallback-no-pair") == {"literal"} and r("fallback-one-pair") == {"literal"}
    assert r("fallback-every-value-coded") == {"no_z"}
    assert r("fit-shard-sh2-bit1-over") == {"overflow"}
    # a shard is never LITERAL on its own: the test is the whole stream's
    c = M.Case("x", "x", np.full(100, X, np.uint8), ctx=(0, 5, X, X))
    assert not c.geometry()["fallback"]
    zs = {c.geometry()["z"] for c in M.catalogue()}
    assert 0 in zs and len(zs) >= 3 and None in zs


def test_qmode_and_wide_halves():
    qs = {c.geometry()["qmode"] for c in M.catalogue()}
    assert qs == {True, False}
    assert any(r["halves_over_64"] for c in M.catalogue() for r in _blocks(c))
