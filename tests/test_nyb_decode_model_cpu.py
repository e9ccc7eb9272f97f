"""tests/nyb_decode_model.py pinned to the oracle, and its catalogue held to what its families claim.

parse + resolve must be oracle.nybble_decompress in both modes on every catalogue stream and on a few
thousand random ones. The *_reach_* tests assert, from geometry() and resolve_trace() alone, that the
catalogue reaches the cuts tests/test_gpu_nyb_decode_edges.py is there for; each fails when its family
is emptied (test_reach_tests_fail_on_an_empty_family).
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import nyb_decode_model as M

TILE, GROUP = M.TILE, M.GROUP


def _geo(case):
    return M.geometry(case.stream, case.in_align, case.out_align, case.wtile_off)


# ---- the model is the oracle ------------------------------------------------------------------------
def test_pack_tokens_and_the_pad_nybble():
    assert M.pack_tokens(0x41, []) == bytes([0xAF, 0x41])
    assert M.pack_tokens(0x41, [("hit", 3), ("lit", 0x5C), ("hit", 0)]) == bytes([0xAF, 0x41, 0xB5, 0xC8])
    with pytest.raises(ValueError):
        M.pack_tokens(0x41, [("hit", 3)])
    # the pad is a token: a hit, or a literal start whose other half is 0
    s = M.pack_tokens(0x41, [("hit", 3)], pad=0x9)
    assert M.parse(s).tokens.tolist() == [0x83, 0x81] and orc.nybble_decompress(s, False) == b"Aae"
    s = M.pack_tokens(0x41, [("hit", 3)], pad=0x4)
    assert M.parse(s).tokens.tolist() == [0x83, 0x40] and orc.nybble_decompress(s, False) == b"Aa@"
    s = M.pack_tokens(0x41, [("lit", 0x12), ("hit", 7)], pad=0x0)
    assert M.parse(s).tokens.tolist() == [0x12, 0x87, 0x00] and orc.nybble_decompress(s, True) == b"A\x12s\x00"


@pytest.mark.parametrize("family", tuple(M.FAMILIES))
def test_model_is_the_oracle_on_the_catalogue(family):
    cases = M.catalogue(family)
    assert cases
    for c in cases:
        for modify in c.modes:
            assert M.decompress(c.stream, modify) == M.expected(c.stream, modify), (c.family, c.name, modify)
        if c.follow is not None:
            assert M.decompress(c.follow, True) == M.expected(c.follow, True)


def test_model_is_the_oracle_on_random_streams():
    rng = np.random.default_rng(0x0AC1E)
    for k in range(3000):
        n = int(rng.integers(0, 90))
        hi = (256, 128, 16)[k % 3]
        s = bytes([0xAF]) + bytes(rng.integers(0, hi, n, dtype=np.uint8)) if k % 50 else bytes(rng.integers(0, 256, n, dtype=np.uint8))
        for modify in (False, True):
            assert M.decompress(s, modify) == orc.nybble_decompress(s, modify), (s, modify)


def test_parse_is_the_carry():
    """entry states, bytes emitted and token positions against a plain walk, element by element"""
    rng = np.random.default_rng(7)
    for n in (0, 1, 2, 5, 64, 300):
        s = bytes([0xAF, 0x33]) + bytes(rng.integers(0, 256, n, dtype=np.uint8))
        P = M.parse(s)
        st, pos = 0, 0
        for j, x in enumerate(s[2:]):
            H, L = x >> 7, (x >> 3) & 1
            assert (int(P.s[j]), int(P.first[j]), int(P.emit[j])) == (st, pos, 1 if st else 1 + H)
            pos += 1 if st else 1 + H
            st = (1 - L) & (st | H)
        assert int(P.s[n]) == st and P.tokens.size == pos


def test_geometry_compositions_compose():
    """a tile's (c0, c1, s0, s1) from its entry state give the next tile's entry and o_tile"""
    for c in M.catalogue("cuts")[:4] + M.catalogue("dense")[:2]:
        G = _geo(c)
        for a, b in zip(G["tiles"], G["tiles"][1:]):
            assert b["entry"] == (a["s1"] if a["entry"] else a["s0"])
            assert b["o_tile"] == a["o_tile"] + (a["c1"] if a["entry"] else a["c0"]) == a["s_end"]
            assert 0 <= a["P"] < 16 and (a["o_al"] + c.out_align) % 16 == 0


# ---- reach ------------------------------------------------------------------------------------------
def reach_cuts():
    seen = set()
    for c in M.catalogue("cuts"):
        G = _geo(c)
        assert G["path"] == "k_nyb_dec_wtile"
        P = G["parsed"]
        for B in range(TILE + 4, G["nelem"], 4):
            pat = M.cut_pattern(P, B)
            if pat:
                seen.add((M.cut_kind(B), pat, int(P.s[(B - 1) // TILE * TILE])))
    want = {(k, p, e) for k in M.KINDS for p in M.PATTERNS for e in (0, 1)}
    assert want <= seen, sorted(want - seen)


def reach_ends():
    cases = M.catalogue("ends")
    ms = {len(c.stream) for c in cases}
    assert {2, 3, 4} <= ms and {n + 2 for n in M.END_COUNTS} <= ms
    assert M.geometry(M.pack_tokens(1, []))["ntiles"] == 0
    assert any(c.stream[1] >= 0x80 and c.stream[1] & 4 for c in cases) and any(c.stream[1] >= 0x80 and not c.stream[1] & 4 for c in cases)
    seen = set()
    for c in cases:
        P = M.parse(c.stream)
        n = P.x.size
        if not n:
            continue
        s, H, L = int(P.s[n - 1]), bool(P.H[n - 1]), bool(P.L[n - 1])
        kind = ("s1_hit" if L else "s1_lit") if s else ("lit" if not H else "hh" if L else "h_lit")
        seen.add((n, kind))
        if kind in ("h_lit", "s1_lit"):   # the literal that starts in the last low nybble takes 0
            assert P.tokens[-1] == (P.x[-1] & 7) << 4
    edge = [n for n in M.END_ALL if n >= 2]
    assert {(n, k) for n in edge for k in M.ENDS} <= seen
    assert {k for _, k in seen if _ == 1} == {"hh", "h_lit", "lit"}


def reach_dense():
    pairs, nts, full, last_only = set(), set(), set(), True
    lits = alt = False
    for c in M.catalogue("dense"):
        G = _geo(c)
        q = G["quads"]
        pairs |= {(int(a), int(b)) for a, b in q}
        nts |= {int(v) for v in G["nt"]}
        last_only &= bool((q[:-1, 1] >= 32).all())
        for t in G["tiles"]:
            emitted = t["s_end"] - t["o_tile"]
            if emitted == 2 * TILE:   # the fsmp fields' largest count and the stage's largest fill
                full.add((t["P"], min(t["T"], 1)))
                assert t["stage"] == t["P"] + 2 * TILE <= M.STAGE
            if t["nv"] < TILE and emitted == 2 * t["nv"]:
                full.add((t["P"], "partial"))
            lits |= t["nv"] == TILE and emitted == TILE
            alt |= t["nv"] == TILE and emitted == TILE + TILE // 2
    want = {(nb, L) for nb in (0, 8, 16, 24) for L in range(8, 72, 8)}
    assert pairs == want and len(want) == 32, sorted(want - pairs)
    assert last_only
    assert 32 in nts and 64 in nts and max(nts) == 88
    assert full == {(p, k) for p in range(16) for k in (0, 1, "partial")}
    assert lits and alt


def reach_stores():
    seen, forms = set(), set()
    for c in M.catalogue("stores"):
        G = _geo(c)
        t = G["tiles"][-1]
        assert t["T"] == 1 and t["entry"] == 0
        seen.add((c.out_align, t["s_end"] - t["o_tile"]))
        for u in G["tiles"]:
            forms |= {"vec"} if u["vec"] else set()
            forms |= {"bytewise"} if u["bytewise"] else set()
            if u["one_granule"] and u["P"] > 0 and u["stage"] < 16:
                forms.add("inside one granule")
            if u["granules"] == 2 and u["vec"] == 0:
                forms.add("both granules bytewise")
    assert seen == {(o, b) for o in range(16) for b in M.STORE_BYTES}
    assert forms == {"vec", "bytewise", "inside one granule", "both granules bytewise"}
    phases = {(c.out_align + _geo(c)["tiles"][-1]["o_tile"]) % 16 for c in M.catalogue("stores")}
    assert phases == set(range(16))


def reach_align():
    cases = M.catalogue("align")
    seen = {(c.in_align, bool(c.wtile_off), _geo(c)["path"]) for c in cases}
    assert {(a, False, "k_fsm_write") for a in (1, 2, 3, 5, 15)} <= seen
    assert (0, False, "k_nyb_dec_wtile") in seen and (0, True, "k_fsm_write") in seen
    fifth = {(t["sh"] != 0, t["fifth"]) for c in cases for t in _geo(c)["tiles"]}
    assert {(True, True), (True, False), (False, False)} <= fifth
    load63 = {t["lane63_load"] for c in cases for t in _geo(c)["tiles"] if _geo(c)["path"] == "k_nyb_dec_wtile"}
    assert load63 == {True, False}
    # one context goes from the wave-per-tile writer to k_fsm_write and back
    order = [_geo(c)["path"] for c in cases if c.in_align == 0]
    assert any(order[i: i + 3] == ["k_nyb_dec_wtile", "k_fsm_write", "k_nyb_dec_wtile"] for i in range(len(order)))


def reach_scan():
    cases = M.catalogue("scan")
    assert all(c.modes == M.STATIC for c in cases)
    crossing = set()
    ntiles = set()
    for c in cases:
        P = M.parse(c.stream)
        nt = (P.x.size + TILE - 1) // TILE
        ntiles.add(nt)
        for gb in range(GROUP, nt, GROUP):
            B = gb * TILE
            prop = ~P.H & ~P.L
            run = bool(prop[B - 3 * TILE: B + 1000].all())   # the run covers the group's last three tiles and more
            crossing.add((int(P.s[B]), run))
            if run and P.s[B]:
                g = B - 1 - int(np.argmax(~prop[B - 1:: -1]))   # the generate that feeds the run: in the group before
                assert P.H[g] and not P.L[g] and (g // TILE) // GROUP == gb // GROUP - 1
    assert ntiles == set(M.SCAN_TILES) == {GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1}
    assert {(1, True), (0, True)} <= crossing


def reach_resolve():
    hits, lits, swar, zeros, ntoks = set(), set(), set(), set(), set()
    for c in M.catalogue("resolve"):
        assert c.modes == M.ADAPTIVE and c.seg == 0
        tr = M.resolve_trace(c.stream)
        hits |= set(tr["hits"])
        lits |= set(tr["lits"])
        swar |= set(tr["swar"])
        zeros |= set(tr["zeros"])
        ntoks.add(tr["ntok"])
        assert len(tr["segments"]) <= 1
    assert hits == {(c, r, b) for c in range(16) for r in range(8) for b in (0, 1)}
    assert lits == set(range(8)) | {None}
    assert swar == {"lo", "hi"}
    assert None in zeros and 0 in zeros and any(z for z in zeros if z)
    assert set(M.RESOLVE_COUNTS) <= ntoks and {n % 64 for n in M.RESOLVE_COUNTS} == {0, 1, 2, 63, 127 % 64, 191 % 64, 255 % 64}
    # nine different literals in one context: the first is gone, the other eight are its list
    nine = next(c for c in M.catalogue("resolve") if c.name == "nine")
    out = M.expected(nine.stream, True)
    assert out[-15::2] == bytes([0x1B] + list(range(0x17, 0x10, -1)))


def reach_segments():
    per = {}
    for c in M.catalogue("segments"):
        assert c.modes == M.ADAPTIVE and c.seg and c.follow is not None
        tr = M.resolve_trace(c.stream, c.seg)
        per.setdefault(c.seg, []).append(tr)
        for lists, _ in tr["cuts"]:
            assert all(row != list(M.DICT) for row in lists)   # no context still holds its initial list
    assert set(per) == set(M.SEGS)
    for seg, trs in per.items():
        assert {t["ntok"] for t in trs} == {seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1, 3 * seg + 7}
        assert sum(len(t["cuts"]) >= 2 for t in trs) >= 2          # at least two restores in one decode, twice
        assert {len(t["segments"]) for t in trs} == {1, 2, 3, 4}


REACH = {"cuts": reach_cuts, "ends": reach_ends, "dense": reach_dense, "stores": reach_stores, "align": reach_align,
         "scan": reach_scan, "resolve": reach_resolve, "segments": reach_segments}


@pytest.mark.parametrize("family", tuple(REACH))
def test_catalogue_reach(family):
    REACH[family]()


def test_types_reach_every_type():
    streams = [c.stream for c in M.catalogue("types")]
    assert b"" in streams and bytes([0xAF]) in streams
    assert {len(s) for s in streams if s[:1] == b" "} == {1, 2, TILE + 1}
    assert any(s and s[0] not in (0xAF, 0x20) and len(s) > 1 for s in streams)


@pytest.mark.parametrize("family", tuple(REACH))
def test_reach_tests_fail_on_an_empty_family(family, monkeypatch):
    M.catalogue(family)
    monkeypatch.setitem(M._CAT, family, [])
    with pytest.raises((AssertionError, StopIteration)):
        REACH[family]()


def test_every_case_reaches_something_of_its_own():
    """no two cases are the same call"""
    keys = [(c.stream, c.in_align, c.out_align, c.wtile_off, c.modes, c.seg) for c in M.catalogue() if c.name[-6:] != "-again"]
    assert len(keys) == len(set(keys))
