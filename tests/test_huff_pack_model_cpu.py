"""tests/huff_pack_model.py against the oracle, and the reach of its case catalogue (no GPU).

The model is what tests/test_gpu_pack_edges.py holds k_huff_pack and the plan kernels to. Here it is
pinned to the oracle (every catalogue stream decodes to its input through orc.huff_unpack, the plan's
offsets are the oracle's sync index at block starts), and the *_reach_* tests assert from
pack_geometry that the catalogue has been on both sides of every cut of the pack's edge table in
DESIGN.md section 6, so the GPU file only has to run the cases. What cannot be reached at the
documented contract is asserted as unreachable."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import huff_pack_model as M


def _blocks(c, detail=True):
    return c.geometry(detail)["blocks"]


# ---- the model against the oracle ------------------------------------------------------------
@pytest.mark.parametrize("fam", M.FAMILIES)
def test_streams_decode_back_and_plan_is_the_index_at_block_starts(fam):
    for c in M.family(fam):
        t = M.table(c.tab)
        payload, bits, idx, base, lens = c.stream()
        if c.bit_base & 7:      # orc.huff_unpack starts at bit 0 of its first byte
            payload = np.packbits(np.unpackbits(payload)[c.bit_base & 7: (c.bit_base & 7) + bits])
        assert np.array_equal(orc.huff_unpack(payload, bits, c.n, t["enc_len"], t["enc_val"], t["n_ary"]), c.x), c
        bh, bbits, off = c.plan()
        assert int(off[-1]) == bits and int(bh.astype(np.int64).sum()) == c.n, c
        starts = idx[(np.arange(off.size - 1) * M.BLOCK) // c.S] - np.uint64(c.bit_base)
        assert np.array_equal(starts, off[:-1]), c
        assert int(lens.astype(np.int64).sum()) == bits and int(base[0]) == c.bit_base, c
        assert lens.size == -(-c.n // c.S) and base.size == -(-lens.size // M.GROUP), c
        g = c.geometry(fam != "plan")
        assert g["total"] == bits and [r["bits"] for r in g["blocks"]] == [int(v) for v in bbits], c
        # the expected words: the payload between zero bits
        w = c.word_bytes()
        assert w.size == 4 * M.words_touched(c.bit_base, bits) and M.words_needed(c.bit_base, bits) == w.size // 4 + 24


def test_boundary_words_are_the_block_starts_and_a_partial_end():
    x, bad = M.refused_input()
    nb = M.table("b16")["nbits"]
    assert nb[200] == 0 and (nb[x] > 0).all() and (bad == 200).sum() == 3
    for inp in (x, bad):
        _, _, off = M.plan_model(inp, nb)
        for bb in (0, 77):
            nw = M.words_touched(bb, int(off[-1]))
            ws = M.boundary_words(off, bb, nw)
            assert ws[0] == 0 and len(ws) == 4 and ws[-1] == nw - 1
            assert all((bb + int(o)) & 31 for o in off[1:])       # every boundary inside a word
            assert M.boundary_words(off, bb, nw - 1) == ws[:-1]


# ---- fit -------------------------------------------------------------------------------------
def test_fit_reach_both_sides_of_the_stage_at_each_sh():
    r = _blocks(M.case("fit-b0-9216-fast"))[0]
    assert (r["path"], r["sh"], r["abs31"], r["nw_blk"]) == ("fast", 0, 0, M.PACK_BLK_WORDS)
    r = _blocks(M.case("fit-b0-9216-base32-fast"))[0]
    assert (r["path"], r["sh"], r["abs31"], r["nw_blk"]) == ("fast", 0, 0, M.PACK_BLK_WORDS)
    r = _blocks(M.case("fit-b0-abs1-slow"))[0]
    assert (r["path"], r["sh"], r["abs31"], r["nw_blk"], r["bits"]) == ("slow", 0, 1, 9217, 32 * 9216)
    for sh in range(4):
        b0, b1 = _blocks(M.case("fit-b1-sh%d-fast" % sh))
        assert b0["path"] == "fast" and b1["before"] == [0]       # one workgroup runs both
        assert (b1["path"], b1["sh"], b1["abs31"], b1["nw_blk"] + sh) == ("fast", sh, 0, M.PACK_BLK_WORDS)
        if sh:
            s0, s1 = _blocks(M.case("fit-b1-sh%d-slow" % sh))
            assert (s1["path"], s1["sh"], s1["abs31"], s1["nw_blk"] + sh) == ("slow", sh, 0, M.PACK_BLK_WORDS + 1)
            assert s1["bits"] == b1["bits"] + 1 and s0["path"] == "fast" and s1["before"] == [0]
    assert _blocks(M.case("fit-b1-sh1-fast"))[1]["nw_blk"] == 9215
    for a in (1, 31):   # at sh = 0 the far side is a block that starts inside a word
        b0, b1 = _blocks(M.case("fit-b1-abs%d-slow" % a))
        assert (b1["path"], b1["sh"], b1["abs31"], b1["nw_blk"], b1["bits"]) == ("slow", 0, a, 9217, 32 * 9216)


# ---- halves ----------------------------------------------------------------------------------
def test_halves_reach_63_64_65_in_both_halves_of_the_edge_lanes():
    assert {(k, t) for k, t, h in M.HALF_SPOTS} == {(k, t) for k in (0, 7) for t in (0, 63, 64, 255)}
    for v in (63, 64, 65):
        c = M.case("halves-%d" % v)
        (r,) = _blocks(c)
        assert r["path"] == "fast" and not r["qmode"]
        for k, t, h in M.HALF_SPOTS:
            assert r["Th"][k, t, h] == v and bool(r["as_half"][k, t, h]) == (v <= 64), (v, k, t, h)
        assert (r["Th"] == v).sum() == len(M.HALF_SPOTS) and (r["Th"] > 64).sum() == (16 if v == 65 else 0)
        assert not r["percode"].any()      # a half of 65 bits: two quarters, none above 64


def test_halves_reach_quarters_of_64_and_65_and_the_code_by_code_flush():
    for tab, longest, in65 in (("b20", 20, 17), ("b32", 32, 32)):
        (r,) = _blocks(M.case("quarters-" + tab))
        assert r["path"] == "fast" and not r["qmode"]
        Q = r["Q"]
        for q in (0, 1):
            for h in (0, 1):    # each quarter of each half: 64 bits gathered, 65 bits code by code
                assert ((Q[:, :, h, q] == 64) & r["as_quarter"][:, :, h, q]).any(), (tab, h, q)
                assert ((Q[:, :, h, q] == 65) & r["percode"][:, :, h, q]).any(), (tab, h, q)
                assert ((Q[:, :, h, q] == 4 * longest) & r["percode"][:, :, h, q]).any(), (tab, h, q)
        assert r["percode_max"] == longest
        # the 65-bit quarters hold the table's 17- / 32-bit code
        x = M.case("quarters-" + tab).x.reshape(M.PIECES, 256, 2, 2, 4)
        nb = M.table(tab)["nbits"]
        assert all(in65 in nb[x[i]] for i in zip(*np.nonzero(Q == 65)))
        assert (Q > 64).sum() == (Q == 65).sum() + (Q == 4 * longest).sum()


def test_halves_reach_quarter_mode_within_two_bits_of_its_threshold():
    off, on = M.case("qmode-off"), M.case("qmode-on")
    (a,), (b,) = _blocks(off), _blocks(on)
    assert 2 * off.bits - 11 * off.n == 0 and not a["qmode"] and a["path"] == "fast"
    assert 2 * on.bits - 11 * on.n == 2 and b["qmode"] and b["path"] == "fast"
    assert (off.x != on.x).sum() == 1
    # half mode: halves of 44 bits and the planted 63 and 64 gathered whole, 65 as quarters
    assert a["as_half"].sum() > 3000 and all(((a["Th"] == v) & a["as_half"]).any() for v in (44, 63, 64))
    assert ((a["Th"] == 65) & ~a["as_half"]).any() and a["percode"].any()
    # quarter mode: no half gathered whole, the same quarters of 64 and 65 bits
    assert not b["as_half"].any() and b["as_quarter"].sum() > 8000
    assert ((b["Q"] == 64) & b["as_quarter"]).any() and ((b["Q"] == 65) & b["percode"]).any()


# ---- seq -------------------------------------------------------------------------------------
SEQ_WANT = {   # per step: what the block must be
    "long-short": [dict(path="fast", sh=0, nwa=9216), dict(path="fast", sh=0, nwa=7168)],
    "fast-slow-fast": [dict(path="fast", sh=0), dict(path="slow", sh=1, full=True), dict(path="fast", sh=1, nwa=9216)],
    "sh-3-0-2": [dict(path="fast", sh=3, nwa=9216), dict(path="fast", sh=0, nwa=8002), dict(path="fast", sh=2, nwa=9216)],
    "on-word": [dict(path="fast", starts_on_word=True, ends_on_word=False),
                dict(path="fast", starts_on_word=False, ends_on_word=True, abs31=7),
                dict(path="fast", starts_on_word=True, ends_on_word=True)],
    "slow-ragged": [dict(path="slow", full=True, sh=2), dict(path="slow", full=False)],
}


@pytest.mark.parametrize("grid", M.SEQ_GRIDS)
@pytest.mark.parametrize("name", list(M.SEQS))
def test_seq_reach_each_sequence_under_each_grid(name, grid):
    c = M.case("seq-%s-grid%d" % (name, grid))
    g = c.geometry()
    blocks, nb = g["blocks"], len(g["blocks"])
    assert g["grid"] == (grid or (nb + 1) // 2)
    runs = M.seq_blocks(c)
    if grid == 0:   # a workgroup runs two blocks: a sequence of three is reached as its two pairs
        assert all(len(r["before"]) <= 1 for r in blocks) and len(runs) == len(M.SEQS[name]) - 1
    else:
        assert len(runs) == 1 and len(runs[0]) == len(M.SEQS[name])
    for j, run in enumerate(runs):
        for i, b in enumerate(run):
            r = blocks[b]
            assert r["wg"] == blocks[run[0]]["wg"], (c, b)
            assert r["before"][-i:] == run[:i] if i else True, (c, b, r["before"])
            for key, v in SEQ_WANT[name][(j if grid == 0 else 0) + i].items():
                assert r[key] == v, (c, b, key, r[key], v)
    if name == "long-short":
        assert blocks[runs[0][0]]["nw_blk"] > blocks[runs[0][1]]["nw_blk"]


# ---- stores ----------------------------------------------------------------------------------
def test_stores_reach_every_shift_and_end():
    seen, tails = set(), set()
    for c in M.family("stores"):
        g = c.geometry()
        r = g["blocks"][0]
        end = (c.bit_base + r["bits"]) & 31
        assert r["path"] == "fast" and g["vec_out"] == (c.shift == 0) and r["sh"] == 0
        assert r["last_or"] == (end != 0) and r["last_plain"] == r["nwa"] - (end != 0)
        assert g["blocks"][1]["path"] == "slow" and not g["blocks"][1]["full"]
        seen.add((c.shift, end))
        if c.shift == 0:
            tails.add((r["tail"], end))
    assert seen == {(s, e) for s in range(4) for e in M.STORE_ENDS}
    assert tails == {(t, e) for t in range(4) for e in M.STORE_ENDS}
    # the head words sh + 1 .. 3: three, two, one and none
    heads = {(r["sh"], r["head"]) for c in M.family("fit") + M.family("seq") for r in _blocks(c) if r["path"] == "fast"}
    assert heads == {(0, 3), (1, 2), (2, 1), (3, 0)}


def test_stores_nq_zero_is_unreachable():
    """A full block holds 32768 codes of at least one bit (a byte without a code refuses the pack
    before any block is coded), so nw_blk >= 1024: nq >= 255, hend = 4 and nw_blk > 1 always."""
    for name in ("b16", "b20", "b32", "t89", "f8"):
        nb = M.table(name)["nbits"]
        assert nb[nb > 0].min() >= 1
    fast = [r for c in M.catalogue() for r in _blocks(c, c.family != "plan") if r["path"] == "fast"]
    assert len(fast) > 100
    assert min(r["nw_blk"] for r in fast) >= 1024
    assert min(r["nq"] for r in fast if "nq" in r) >= 255 and min(r["last_plain"] for r in fast) >= 4
    short = M.pack_geometry(np.full(M.BLOCK, M.by_len("b16")[1], np.uint8), M.table("b16")["nbits"])["blocks"][0]
    assert (short["nw_blk"], short["nq"], short["head"], short["tail"]) == (1024, 256, 3, 0)


# ---- tail ------------------------------------------------------------------------------------
def test_tail_reach_every_lane_count_and_tile_end():
    sizes = {c.n for c in M.family("tail")}
    assert set(M.TAIL_SIZES) <= sizes
    tiles = [t for c in M.family("tail") for r in _blocks(c) if r["path"] == "slow" for t in r["tiles"]]
    assert all(not r["full"] for c in M.family("tail") for r in _blocks(c) if r["path"] == "slow")
    assert any(t["cnt0"] == 255 and t["cnt_part"] == 1 for t in tiles)            # n = 1, 15
    assert any(t["cnt0"] == 255 and t["cnt16"] == 1 for t in tiles)               # n = 16
    assert any(t["cnt16"] == 1 and t["cnt_part"] == 1 for t in tiles)             # n = 17
    assert any(t["cnt16"] == 255 and t["cnt_part"] == 1 for t in tiles)           # 4095
    assert any(t["cnt16"] == 256 for t in tiles)                                   # a whole tile
    assert {t["end_aligned"] for t in tiles} == {True, False}
    (r,) = _blocks(M.case("tail-b32-full-lanes"))
    assert [t["tile_bits"] for t in r["tiles"]] == [131072, 32 * 21] and r["tiles"][0]["lane_bits_max"] == 512
    (r,) = _blocks(M.case("tail-ones-17"))
    assert r["tiles"][0]["tile_bits"] == 17 and r["tiles"][0]["one_word"] == 2
    (r,) = _blocks(M.case("tail-ones-%d" % (2 * M.TILE + 33)))
    assert r["tiles"][0]["one_word"] == 128 and r["tiles"][0]["lane_bits_max"] == 16   # two lanes per word
    assert len(r["tiles"]) == 3 and r["tiles"][2]["tile_bits"] == 33
    # 32768 + 1 and 2 * 32768 - 1: a fast block, then a block of one byte and of all but one
    assert [r["path"] for r in _blocks(M.case("tail-%d" % (M.BLOCK + 1)))] == ["fast", "slow"]
    assert [r["n"] for r in _blocks(M.case("tail-%d" % (2 * M.BLOCK - 1)))] == [M.BLOCK, M.BLOCK - 1]


# ---- sync ------------------------------------------------------------------------------------
def test_sync_reach_every_chunk_size_on_every_path():
    form = {16: "one", 32: "shfl", 64: "dpp", 128: "shfl", 256: "shfl", 512: "shfl", 1024: "shfl"}
    for S in M.SYNCS:
        fast, slow, ragged = (M.case("sync-%d-%s" % (S, k)) for k in ("fast", "slow", "ragged"))
        assert [(r["path"], r["sync"]) for r in _blocks(fast)] == [("fast", form[S])] * 2 and fast.n % S == 0
        b = _blocks(slow)
        assert [(r["path"], r["full"], r["sync"]) for r in b] == [("slow", True, "xor"), ("slow", False, "xor")]
        assert slow.n % S == 1 and b[0]["nw_blk"] > M.PACK_BLK_WORDS
        assert [(r["path"], r["full"]) for r in _blocks(ragged)] == [("slow", False)] and ragged.n % S == S - 1
    for S in (16, 64, 512):
        counts = {c.stream()[4].size for c in M.family("sync") if c.S == S}
        assert set(M.SYNC_COUNTS) <= counts, (S, counts)
        assert {M.case("sync-%d-n%+d" % (S, d)).n % S for d in (-1, 1)} == {S - 1, 1}
    c = M.case("sync-1024-three-blocks")
    assert [r["path"] for r in _blocks(c)] == ["fast"] * 3
    assert c.stream()[3].size == 2 and int(c.stream()[3][1]) == int(c.plan()[2][2])    # a group base in blocks 0 and 2 only
    assert (M.case("sync-1024-b32").stream()[4][:3] == 32768).all()


# ---- base ------------------------------------------------------------------------------------
def test_base_reach_every_bit_base_and_the_byte_map():
    cs = M.family("base")
    assert {c.bit_base for c in cs if c.tab == "b16" and not c.dev} == set(M.BIT_BASES)
    assert sorted(c.bit_base for c in cs if c.dev) == sorted(M.DEV_BASES)
    for c in cs:
        if c.tab == "b16":
            assert [r["path"] for r in _blocks(c)] == ["fast", "slow"] and _blocks(c)[0]["abs31"] == c.bit_base & 31
    maps = {(c.bit_base, c.shift): c.geometry()["bytemap"] for c in cs if c.tab == "f8"}
    assert maps == {(0, 0): True, (128, 0): True, (8, 0): False, (0, 1): False}
    assert M.table("f8")["fixed8"] and not M.table("t89")["fixed8"]
    for c in cs:
        if c.tab == "f8":
            want = ["fixed8", "fixed8"] if c.geometry()["bytemap"] else ["fast", "slow"]
            assert [r["path"] for r in _blocks(c)] == want


# ---- plan ------------------------------------------------------------------------------------
def test_plan_reach_every_last_workgroup_and_the_largest_count():
    last = {}
    for c in M.family("plan"):
        nblocks = c.plan()[2].size - 1
        last[nblocks] = M.plan_workgroups(nblocks)
        assert len(set(int(v) for v in c.plan()[1][:-1])) > 1 or nblocks < 3     # the blocks differ
    assert last == {1: (1, 1), 2: (1, 2), 63: (1, 63), 64: (1, 64), 65: (2, 1), 128: (2, 64), 129: (3, 1)}
    bh = M.case("plan-32768-of-one").plan()[0]
    assert bh.dtype == np.uint16 and int(bh.max()) == 32768
