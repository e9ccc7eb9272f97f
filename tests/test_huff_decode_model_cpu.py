"""tests/huff_decode_model.py against the oracle, and the reach of its case catalogue (no GPU).

The model is what tests/test_gpu_decode_edges.py holds k_huff_decode8, k_huff_decode8_fix and the
dc_dtable decoder tables to. Here it is pinned to the oracle (every catalogue stream decodes to its
input, as orc.huff_unpack does), its tables are checked against the codes they were searched from,
and the *_reach_* tests assert from the model that the catalogue hits every row of the decoder's
edge table in DESIGN.md section 6, so the GPU file only has to run the cases."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import huff_decode_model as M

BIG_TUPLES = 2 * 2816 + 300 + 1     # test_scheduler_static_then_dynamic: n = (2 * 2816 + 300) * 8192 + 4097


def _all_cases():
    return M.catalogue() + [M.sched_case(t) for t in M.SCHED_TUPLES] + [M.c5_case(None)[1], M.c5_case(0xC3)[1]]


def test_model_decodes_every_stream_to_its_input_and_to_the_oracles():
    for c in _all_cases():
        dec, _ = c.model()
        assert not dec["bad"].any() and np.array_equal(dec["out"], c.x), c
        assert (dec["good"] == np.minimum(64, c.n - 64 * np.arange(dec["good"].size))).all(), c
        t = M.table(c.tab)
        payload, bits = c.payload, c.bits
        if c.bit_base:
            payload, bits, _ = orc.huff_pack(c.x, t["code"], t["nbits"].astype(np.uint8), sync_syms=64)
            assert bits == c.bits
        assert np.array_equal(orc.huff_unpack(payload, bits, c.n, t["enc_len"], t["enc_val"], t["n_ary"]), c.x), c
        # the index the decoder gets: group bases and u16 lengths that sum to the stream
        assert int(c.lens.astype(np.int64).sum()) == c.bits and int(c.base[0]) == c.bit_base, c


def _lookup(t, win):
    """(sym, bits) of the code at the start of the LSB-first window `win` (>= 32 bits), by the
    model's tables: dlut, then dlut2, then the canonical search (here: over the codes)"""
    e = int(t["dlut"][win & 4095])
    if e & 255:
        return e >> 8, e & 255
    k = t["dlut2_k"]
    if k:
        e2 = int(t["dlut2"][((e >> 8) << k) | ((win >> 12) & ((1 << k) - 1))])
        if e2:
            return e2 >> 8, e2 & 255
    for s in np.nonzero(t["nbits"])[0]:
        b = int(t["nbits"][s])
        if win & ((1 << b) - 1) == M._rev(int(t["code"][s]), b):
            return int(s), b
    return None


@pytest.mark.parametrize("name", list(M.TABLES))
def test_tables_give_every_code_back(name):
    t = M.table(name)
    past14, past15 = set(), set()
    for s in np.nonzero(t["nbits"])[0]:
        b = int(t["nbits"][s])
        r = M._rev(int(t["code"][s]), b)
        for fill in (0, (1 << 33) - 1, 0x155555555):
            win = (r | (fill << b)) & ((1 << 40) - 1)
            assert _lookup(t, win) == (int(s), b), (name, s)
            for field, B, past in (("dlut14", 14, past14), ("dlut15", 15, past15)):
                e = int(t[field][win & ((1 << B) - 1)])
                if e & 255:
                    assert (e >> 8, e & 255) == (int(s), b), (name, field, s)
                else:
                    past.add(b)
                    assert e == (0 if B == 15 else int(t["dlut"][win & 4095])), (name, field, s)
            if b <= 12:     # lut: the MSB-first window whose first code is s
                v = int(t["lut"][M._rev(win & 4095, 12)])
                assert v & 255 == s and (v >> 24) & 31 == b and v >> 29 in (1, 2), (name, s)
                if v >> 29 == 2:
                    assert _lookup(t, win >> b) == ((v >> 16) & 255, ((v >> 8) & 255) - b), (name, s)
    # the K >= 2 / K >= 3 rule: what each wide table leaves to the escape
    ok14, ok15 = t["l2ok"] and t["K"] >= 2, t["l2ok"] and t["K"] >= 3
    lens = {int(b) for b in t["nbits"] if b}
    assert past14 == {b for b in lens if b > 14 or (b > 12 and not ok14)}
    assert past15 == {b for b in lens if b > 15 or (b > 12 and not ok15)}
    assert np.array_equal(M.in_dlut15(t), (t["nbits"] > 0) & ~np.isin(t["nbits"], sorted(past15)))


def test_tables_reach_every_second_level_condition():
    T = {n: M.table(n) for n in M.TABLES}
    assert [T[n]["max_bits"] for n in ("b12", "b13", "b14", "b15", "b16", "b20", "b23", "b32")] == [12, 13, 14, 15, 16, 20, 23, 32]
    assert (T["b32"]["nbits"][1:34] == list(range(1, 33)) + [32]).all()
    # the pair at the capacity: 28 << 8 = 7168 fits, 29 << 8 does not
    assert (T["e28"]["E"], T["e28"]["K"], T["e28"]["l2ok"]) == (28, 8, True)
    assert (T["e29"]["E"], T["e29"]["K"], T["e29"]["l2ok"]) == (29, 8, False)
    assert int((T["e28"]["nbits"] > 0).sum()) == 74 and int((T["e29"]["nbits"] > 0).sum()) == 75
    for n in ("e28", "e29"):
        nb = T[n]["nbits"]
        assert sum(2.0 ** -int(b) for b in nb if b) == 1.0
    # E >= 1 fails (no code past 12 bits), E <= 256 fails (an incomplete code: n = 3, n = 5); a
    # table of byte symbols whose status is DC_OK has max_bits <= 32, so that test cannot fail
    assert T["b12"]["E"] == 0 and T["t89"]["E"] == 0 and not T["b12"]["l2ok"]
    assert T["n3"]["E"] > 256 and T["n5"]["E"] > 256 and not T["n3"]["l2ok"] and T["n5"]["n_ary"] == 5
    assert T["n16"]["max_bits"] == 16 and T["n16"]["l2ok"]
    assert [T[n]["dlut2_k"] for n in ("b13", "b14", "b15", "b20")] == [1, 2, 3, 8]
    assert all(T[n]["max_bits"] <= 32 for n in T)
    assert sorted(set(T["t89"]["nbits"].tolist())) == [7, 8, 9]


def test_tables_13_and_14_bit_codes_go_to_the_redo():
    """K = max_bits - 12 is 1 or 2 there, so dlut15 (K >= 3) resolves no code
    past 12 bits and every chunk that holds one is redone; at 15 bits none is."""
    for name, share in (("b13", True), ("b14", True), ("b15", False)):
        t = M.table(name)
        assert bool((~M.in_dlut15(t) & (t["nbits"] > 0)).any()) == share
    # a chunk of 64 symbols drawn by code probability holds a 13-bit code of b13 with 1 - (1 - 2^-12)^64
    assert abs(1 - (1 - 2.0 ** -12) ** 64 - 0.0155) < 1e-3


def test_span_reach_both_sides_at_both_leads_and_positions():
    seen = set()
    for c in M.family("span"):
        _, geo = c.model()
        g = max(range(4), key=lambda k: geo["span"][k])
        total = geo["lead"][g] + geo["span"][g]
        assert g in (2, 3) and total in (M.SPAN_LAST_FAST, M.SPAN_LAST_FAST + 1), c
        assert geo["fast"].tolist() == [True, total == M.SPAN_LAST_FAST], c
        assert geo["nw"][g] + 4 == (1088 if total == M.SPAN_LAST_FAST else 1089), c
        # the slow group's partner is fast by itself, and redone with it
        assert geo["nw"][g ^ 1] + 4 <= 1088 and geo["count"] == (0 if geo["fast"][1] else 128), c
        seen.add((geo["lead"][g], total - M.SPAN_LAST_FAST, g & 1))
    assert seen == {(lead, d, p) for lead in (0, 127) for d in (0, 1) for p in (0, 1)}


def test_sizes_reach_partial_chunks_groups_and_tuples():
    ns = [c.n for c in M.family("sizes")]
    assert ns == list(M.SIZES)
    assert any(n % 64 for n in ns) and any(n % 4096 == 0 and (n // 4096) % 2 for n in ns)
    for c in M.family("sizes"):
        _, geo = c.model()
        whole = c.n // (2 * 4096)
        assert geo["fast"].tolist() == [True] * whole + [False] * (geo["ntuples"] - whole), c
        # 64 slots for every group of a tuple that is not fast, a partial last group too
        assert geo["redo"][2 * whole:].all() and geo["redo"][2 * whole:].size == 64 * (geo["ngroups"] - 2 * whole), c
    assert any(0 < c.model()[1]["redo"][: 2 * (c.n // 8192)].sum() for c in M.family("sizes"))


def test_buffer_end_reach_every_residue_and_bit_base():
    cs = M.family("bufend")
    assert {c.words % 4 for c in cs if c.name.startswith("words-mod4")} == {0, 1, 2, 3}
    assert {c.bit_base for c in cs} == set(M.BIT_BASES) and sum(c.dev for c in cs) == 1
    for c in cs:
        assert c.words == M.words_needed(c.bit_base, c.bits) + (64 if c.name == "spare-64" else 0), c
    a, b = [c for c in cs if c.name in ("spare-0", "spare-64")]
    assert np.array_equal(a.x, b.x) and abs(a.words - b.words) == 64
    # at the documented capacity the 24 slack words always satisfy wo + nw + 4 <= words: a whole
    # last tuple is fast with and without spare words (the words test guards shorter buffers)
    assert a.model()[1]["fast"].all() and b.model()[1]["fast"].all()


def _restages(c):
    dec, geo = c.model()
    out = {}
    for ch in np.nonzero(geo["redo"].reshape(-1)[: dec["bad"].size])[0]:
        out[int(ch)] = M.model_restage(int(geo["pos"][ch]), dec["sbits"][ch], c.words)
    return out


def test_redo_reach_rows_lists_and_lanes():
    by = {c.name: c for c in M.family("redo")}
    r = _restages(by["rows32"])
    calls = {v[0] for v in r.values()}
    assert 0 in calls and 1 in calls and max(calls) >= 3
    lens = by["rows32"].lens
    assert lens.min() < 20 * 32 and lens.max() > 60 * 32 and not by["rows32"].model()[1]["fast"].any()
    assert by["rows32"].n % 64 and by["rows32"].lens[-1] == 17 * 32      # a lane's partial last chunk
    for lane in (0, 31, 63):
        geo = by["one-flag-lane%d" % lane].model()[1]
        assert geo["fast"].all() and np.nonzero(geo["redo"].reshape(-1))[0].tolist() == [lane]
    geo = by["all-64-flagged"].model()[1]
    assert geo["fast"].all() and geo["redo"].sum(axis=1).tolist() == [0, 64]
    c = by["flags-in-last-group"]
    geo = c.model()[1]
    assert geo["ngroups"] == 4 and c.n % 4096 and geo["redo"][2:].all() and 0 < geo["redo"][:2].sum() < 128
    # row_base's clamp guards buffers shorter than the documented capacity: with its 24 slack
    # words a chunk starts at word <= words - 25, under the clamp (words - 20) & ~3, in every case
    for c in M.catalogue():
        assert not any(cl for _, cl in _restages(c).values()), c


def test_redo_reach_a_second_part_of_the_list():
    x, idx, bits = M.redo_list_input()
    assert x.size == M.REDO_LIST_GROUPS * 4096 and 17_000_000 < x.size < 19_000_000
    words = M.words_needed(0, bits)
    geo = M.model_geometry(idx, bits, 0, x.size, words, np.zeros(idx.size, bool))
    assert not geo["fast"].any() and geo["count"] == M.REDO_LIST_GROUPS * 64
    assert M.redo_parts(geo["redo"]) == 2     # 17 groups of 64 chunks a workgroup: 1088 > 1024
    assert M.REDO_LIST_GROUPS <= M.FIX_GRID * M.FIX_NT      # one window each (the second: 1 GiB)


def test_codes_reach_every_batch_position():
    (c,) = M.family("codes")
    dec, geo = c.model()
    t = M.table("b16")
    assert geo["fast"].all() and t["l2ok"] and t["K"] == 4
    sb = dec["sbits"]
    flagged = geo["redo"].reshape(-1)
    assert (flagged == (sb == 16).any(axis=1)).all()
    for b in (13, 14, 15, 16):      # its longest code in each of the 4 positions of a batch
        rows = np.nonzero((sb.max(axis=1) == b) & ((sb == b).sum(axis=1) == 1))[0]
        assert {int(np.argmax(sb[r] == b)) % 4 for r in rows} == {0, 1, 2, 3}, b
    quads = sb.reshape(-1, 16, 4)
    assert ((quads == 15).all(axis=2).any(axis=1) & ~flagged).any()      # the 60-bit window, decoded fast
    # a batch that ends exactly on a 64-bit boundary of the window registers (qb == 64)
    start = geo["pos"] + 63
    qb = (start[:, None] + np.cumsum(quads.sum(axis=2), axis=1)) % 64
    assert ((qb == 0).any(axis=1) & ~flagged).any()


def test_scheduler_reach_every_shape():
    shapes = set()
    for nt in M.SCHED_TUPLES:
        assert M.sched_case(nt).model()[1]["ntuples"] == nt
        for pct in M.SCHED_PCT:
            s = M.model_schedule(nt, pct)
            got = [t for lo, hi in s["slices"] for t in range(lo, hi)]
            assert got == list(range(s["Ts"], nt)) and s["Ts"] == s["Ks"] * s["waves"], (nt, pct)
            assert s["grid"] == min(-(-nt // 11), 256)
            if s["Ks"] == 0 and s["empty"]:
                shapes.add("all dynamic, empty slices")
            if s["Dh"] == 1:
                shapes.add("Dh = 1")
            if s["Ts"] == nt:
                assert pct == 100 and nt % 11 == 0 and s["Dh"] == 0
                shapes.add("all static")
            assert s["Ts"] in (0, nt)      # the hand-over needs more than a grid of tuples: below
            if s["steals"]:
                shapes.add("steal")
    assert shapes == {"all dynamic, empty slices", "Dh = 1", "all static", "steal"}
    assert M.model_schedule(1, 0)["empty"] == 7 and M.model_schedule(2816, 60)["Ks"] == 0   # below 2816: all dequeued
    big = [M.model_schedule(BIG_TUPLES, p) for p in M.SCHED_PCT]
    assert [(s["Ks"], s["Ts"]) for s in big] == [(0, 0), (1, 2816), (2, 5632)] and all(s["Ts"] < BIG_TUPLES for s in big)


def test_damage_reach():
    for tab, seed in (("t89", 1), ("n3", 4)):
        case, p, chunks, dd = M.damage_case(tab, seed)
        dec, geo = case.model()
        nch = dec["bad"].size
        assert len(chunks) == 12 and chunks.max() < nch - 4 and not np.array_equal(p, case.payload)
        assert np.array_equal(case.word_array(p).view(np.uint8)[len(p):], case.word_array().view(np.uint8)[len(p):])
        same = np.ones(nch, bool)
        same[chunks] = False
        for c in range(nch):      # untouched chunks decode as before; a damaged one ends inside its group
            lo, hi = c * 64, min(c * 64 + 64, case.n)
            assert same[c] == np.array_equal(dd["out"][lo:hi], case.x[lo:hi]) or not same[c], (tab, c)
            if not same[c] and geo["fast"][c // 128]:      # (the redo reads the buffer itself)
                assert int(dd["end"][c]) <= int(case.idx[(c // 64 + 1) * 64]), (tab, c)
        assert geo["fast"][chunks // 128].any() and not geo["fast"][chunks // 128].all()
        if tab == "t89":
            assert M.table(tab)["E"] == 0 and not dd["bad"].any() and (dd["good"][chunks] == 64).all()
        else:
            late = dd["bad"][chunks] & (dd["good"][chunks] >= 8)
            assert 2 * int(late.sum()) >= len(chunks) and not dd["bad"][same].any()


def test_c5_reach():
    for first in (None, 0xC3):
        x, c = M.c5_case(first)
        m, t = c.x, M.table(c.tab)
        dec, geo = c.model()
        assert m[0] == 8 and m[1] == x[0] and (first is None or m[1] >= 0x80)
        assert orc.small_decompress(m.tobytes()) == x.tobytes()
        assert t["n_ary"] == 16 and (t["nbits"][m] == 16).any() and t["max_bits"] >= 16
        tail = m[-(c.n % 64):]
        assert c.n % 64 and (tail >= 0x80).any()
        rows = np.zeros(geo["redo"].size * 64, np.uint8)
        rows[: c.n] = m
        rows = rows.reshape(-1, 64)
        flagged = geo["redo"].reshape(-1) & np.repeat(geo["fast"], 128)[: geo["redo"].size]
        assert flagged.any() and ((rows[flagged] >= 0x80).any(axis=1)).all()
        # ... in groups that also hold chunks the fast decoder counts itself
        assert ((geo["redo"].sum(axis=1) > 0) & (geo["redo"].sum(axis=1) < 64)).any()
