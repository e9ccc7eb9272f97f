"""Plain model of the whole-stream nybble decode (dc_nyb_decompress) and of the cuts of its kernels,
and the catalogue of streams that reaches them. numpy, plain Python and the oracle only.

Semantics: `parse` restates the token structure of a stream as a carry over its elements, `resolve`
turns tokens into bytes (the static dictionary, or move-to-front with drop-last over 16 contexts);
tests/test_nyb_decode_model_cpu.py pins parse + resolve to oracle.nybble_decompress, which stays the
expected output of every case.

Geometry (dc_core.hip; element j = stream byte j + 2, tile = 4096 elements):
  k_nyb_tiles<M_NYB_DEC>   a wave per tile, 2 tiles a wave, 8 a workgroup; a lane takes 64 elements as
                           four 16-B granules of the address grid; sh = the tile's first byte's place
                           in its granule; lane 63 reads a fifth granule when sh != 0
  k_fsm_scan_up / _scan    groups of 1024 tile summaries
  k_nyb_dec_wtile          when there are tiles, the input is on 16 bytes and nyb_wtile_off is clear:
                           a wave per tile, 4 tiles a workgroup, 64 elements a lane as four blocks of
                           16, quads of 4 elements placed in the stage at bit nb with L bits
                           (nt = nb + L), R[16] from the next lane (lane 63: a dword load of its own
                           when the stream goes on), NV: the elements of a block whose next byte
                           exists
  k_fsm_write<M_NYB_DEC>   otherwise: a workgroup per tile, 16 elements a lane, the same quads
  the stage                2 * 4096 + 32 bytes at o_al, the 16-B granule of the tile's first output
                           byte; the store writes whole granules as uint4 and the granules shared with
                           the neighbours bytewise
  adec_fast                the adaptive resolve, one launch of k_nyb_resolve_c per segment of tokens
                           (blocks of 64, then one at a time), lists and previous byte saved between
"""
from collections import namedtuple

import numpy as np

from oracle import oracle as orc

MAGIC = 0xAF
TILE = 4096
GROUP = 1024            # tiles per scan group
STAGE = 2 * TILE + 32   # bytes of a tile's stage
WG_WRITE, WAVE_COUNT, WG_COUNT = 4, 2, 8   # tiles per writer workgroup, count wave, count workgroup
ADEC_SEG = 16 << 20
DICT = b" etaoins"


# ---- streams by hand --------------------------------------------------------------------------------
def nybbles(tokens):
    out = []
    for kind, v in tokens:
        if kind == "hit":
            assert 0 <= v < 8
            out.append(8 | v)
        else:
            assert kind == "lit" and 0 <= v < 0x80
            out += [v >> 4, v & 15]
    return out


def pack_tokens(seed, tokens, pad=None):
    """0xAF, the seed byte, the nybbles of the tokens; an odd count takes the pad nybble the case
    names (itself a token: a hit, or a literal start whose other half is 0)"""
    nyb = nybbles(tokens)
    if len(nyb) & 1:
        if pad is None:
            raise ValueError("odd nybble count: name the pad nybble")
        nyb.append(pad & 15)
    else:
        assert pad is None
    return bytes([MAGIC, seed]) + bytes((nyb[i] << 4) | nyb[i + 1] for i in range(0, len(nyb), 2))


def even(tokens):
    """the same number of tokens with an even nybble count: the first hit becomes a literal"""
    tokens = list(tokens)
    if len(nybbles(tokens)) & 1:
        k = next((i for i, t in enumerate(tokens) if t[0] == "hit"), None)
        if k is None:
            tokens[0] = ("hit", tokens[0][1] & 7)
        else:
            tokens[k] = ("lit", 0x41 + tokens[k][1])
    return tokens


# ---- semantics --------------------------------------------------------------------------------------
def _states(H, L, s0):
    """entry state of every element and the exit state: s' = ~L & (s | H)"""
    n = H.size
    g = H & ~L
    p = ~H & ~L
    # the state after element j is g at the last element <= j that does not propagate, s0 if none
    idx = np.where(~p, np.arange(n), -1)
    last = np.maximum.accumulate(idx) if n else idx
    after = np.where(last >= 0, g[np.maximum(last, 0)], bool(s0))
    s = np.empty(n + 1, bool)
    s[0] = bool(s0)
    s[1:] = after
    return s


Parsed = namedtuple("Parsed", "x H L s emit first tokens")


def parse(stream):
    """the token structure of a 0xAF stream of >= 2 bytes: per element its byte x, flags H and L, entry
    state s (n + 1 entries: the last is the exit state), bytes emitted, the index of its first token;
    tokens: a hit 0x80 | rank, a literal itself"""
    a = np.frombuffer(bytes(stream), np.uint8)
    assert a.size >= 2 and a[0] == MAGIC
    x = a[2:].astype(np.int64)
    n = x.size
    H, L = (x & 0x80) != 0, (x & 8) != 0
    s = _states(H, L, 0)
    s_in = s[:n]
    emit = 1 + (H & ~s_in).astype(np.int64)
    first = np.concatenate(([0], np.cumsum(emit)))[:n] if n else np.zeros(0, np.int64)
    nxt = np.concatenate((x[1:] >> 4, [0])) if n else x     # a literal in the last low nybble takes 0
    lo = np.where(L, 0x80 | (x & 7), ((x & 7) << 4) | nxt)
    hi = np.where(H, 0x80 | ((x >> 4) & 7), x)
    tok = np.zeros(int(emit.sum()), np.int64)
    tok[first] = np.where(s_in, lo, hi)
    two = emit == 2
    tok[first[two] + 1] = lo[two]
    return Parsed(x, H, L, s, emit, first, tok.astype(np.uint8))


def resolve(seed, tokens, modify):
    """out[0] = seed, then each token's byte: a hit is the entry at its rank of the list of context
    (previous byte >> 3) & 15, a literal is itself; modify: move to front, the last entry drops"""
    tokens = np.asarray(tokens, np.uint8)
    if not modify:
        d = np.frombuffer(DICT, np.uint8)
        return bytes([seed]) + np.where(tokens & 0x80, d[tokens & 7], tokens).astype(np.uint8).tobytes()
    lists = [list(DICT) for _ in range(16)]
    out = bytearray([seed])
    for t in tokens.tolist():
        row = lists[(out[-1] >> 3) & 15]
        v = row[t & 7] if t & 0x80 else t
        p = row.index(v) if v in row else 7
        del row[p]
        row.insert(0, v)
        out.append(v)
    return bytes(out)


def decompress(stream, modify):
    """orc.nybble_decompress restated: parse + resolve for 0xAF, the copies for the other types"""
    stream = bytes(stream)
    if not stream:
        return b""
    if stream[0] == MAGIC:
        return b"" if len(stream) < 2 else resolve(stream[1], parse(stream).tokens, modify)
    return stream[1:] if stream[0] == 0x20 else stream


# ---- geometry ---------------------------------------------------------------------------------------
def geometry(stream, in_align=0, out_align=0, wtile_off=0):
    """the cuts the kernels make of this call; see the module docstring"""
    P = parse(stream)
    m, n = len(stream), len(stream) - 2
    ntiles = (n + TILE - 1) // TILE
    path = "k_nyb_dec_wtile" if ntiles and in_align % 16 == 0 and not wtile_off else "k_fsm_write"
    G = {"m": m, "nelem": n, "ntiles": ntiles, "path": path, "parsed": P, "tiles": []}
    opos = 1 + np.concatenate((P.first, [P.tokens.size]))   # output position of each element's first byte
    for T in range(ntiles):
        a, b = T * TILE, min(n, (T + 1) * TILE)
        H, L = P.H[a:b], P.L[a:b]
        s0, s1 = _states(H, L, 0), _states(H, L, 1)
        o_tile, s_end = int(opos[a]), int(opos[b])
        o_al = ((out_align + o_tile) & ~15) - out_align
        ng = (s_end - o_al + 15) // 16 if s_end > o_tile else 0
        vec = [g for g in range(ng) if o_al + 16 * g >= o_tile and o_al + 16 * g + 16 <= s_end]
        sh = (a + 2 + in_align) & 15
        t = {"T": T, "nv": b - a, "entry": int(P.s[a]),
             "c0": int((b - a) + (H & ~s0[:-1]).sum()), "c1": int((b - a) + (H & ~s1[:-1]).sum()),
             "s0": int(s0[-1]), "s1": int(s1[-1]),
             "o_tile": o_tile, "s_end": s_end, "o_al": o_al, "P": o_tile - o_al, "stage": s_end - o_al,
             "granules": ng, "vec": len(vec), "bytewise": ng - len(vec),
             "one_granule": ng == 1,
             "group": T // GROUP, "wg_write": T // WG_WRITE, "wave_count": T // WAVE_COUNT, "wg_count": T // WG_COUNT,
             "sh": sh, "fifth": sh != 0 and (a + 2 - sh + TILE) < m,
             # k_nyb_dec_wtile: lane 63's own dword (stream bytes j0 + 64 ..) when the stream goes on
             "lane63_load": path == "k_nyb_dec_wtile" and a + 63 * 64 + 64 < m}
        assert t["stage"] <= STAGE and (t["c1"] if t["entry"] else t["c0"]) == s_end - o_tile
        G["tiles"].append(t)
    # quads of four elements: (nb, L) and nt; every quad with an element in it
    nq = (n + 3) // 4
    pad = np.zeros(4 * nq, np.int64)
    pad[:n] = P.emit
    Lq = 8 * pad.reshape(nq, 4).sum(axis=1) if nq else np.zeros(0, np.int64)
    nbq = 8 * ((opos[: 4 * nq: 4] + out_align) & 3) if nq else np.zeros(0, np.int64)
    G["quads"] = np.stack((nbq, Lq), axis=1) if nq else np.zeros((0, 2), np.int64)
    G["nt"] = nbq + Lq
    # the block whose NV mask is short: the one with the stream's last element (its next byte is absent)
    block = 16
    G["nv_short"] = None
    if n:
        kb = (n - 1) // block * block
        lane_el = 64 if path == "k_nyb_dec_wtile" else 16
        G["nv_short"] = {"tile": kb // TILE, "lane": kb % TILE // lane_el, "block": kb % lane_el // block,
                         "nvc": n - kb - 1}
    return G


# ---- the adaptive resolve, traced -------------------------------------------------------------------
def resolve_trace(stream, seg=0):
    """per hit (context, rank, bit 2 of the previous byte); per literal its position in its list (0..7,
    None when absent) and, when its list holds v at p and v ^ 1 at p + 1 inside one dword, which
    ('lo' / 'hi'); the token count, its residue and blocks of 64 per segment; the lists at every cut"""
    P = parse(stream)
    seg = seg or ADEC_SEG
    lists = [list(DICT) for _ in range(16)]
    prev = stream[1]
    hits, lits, swar, cuts, zeros = [], [], [], [], []
    ntok = int(P.tokens.size)
    for i, t in enumerate(P.tokens.tolist()):
        if i and i % seg == 0:
            cuts.append(([list(r) for r in lists], prev))
        c = (prev >> 3) & 15
        row = lists[c]
        if t & 0x80:
            hits.append((c, t & 7, (prev >> 2) & 1))
            v, p = row[t & 7], t & 7
        else:
            v = t
            p = row.index(v) if v in row else None
            lits.append(p)
            if v == 0:
                zeros.append(p)
            if p is not None and p < 7 and row[p + 1] == v ^ 1 and p // 4 == (p + 1) // 4:
                swar.append("lo" if p < 4 else "hi")
            p = 7 if p is None else p
        del row[p]
        row.insert(0, v)
        prev = v
    segs = [(k, min(k + seg, ntok)) for k in range(0, ntok, seg)]
    return {"hits": hits, "lits": lits, "swar": swar, "zeros": zeros, "ntok": ntok, "cuts": cuts, "segments": segs,
            "blocks": [((b - a) // 64, (b - a) % 64) for a, b in segs]}


# ---- the catalogue ----------------------------------------------------------------------------------
# stream: the bytes; in_align / out_align: the byte of a 16-B granule the input / the output view starts
# at; wtile_off: nyb_wtile_off; modes: the modify values it runs under; seg: nyb_adec_seg; follow: a
# stream decoded on the same context right after (adaptive), or None
Case = namedtuple("Case", "family name stream in_align out_align wtile_off modes seg follow")
BOTH, STATIC, ADAPTIVE = (False, True), (False,), (True,)
KILL, GEN, PROP, LITK = 0x99, 0x94, 0x41, 0x4A   # H L; H ~L; ~H ~L; ~H L
PATTERNS = ("hh", "split", "lit_before", "gen_last", "prop_run")
KINDS = ("dword", "block", "lane", "tile", "count_wave", "wg_write", "wg_count")


def _case(family, name, stream, in_align=0, out_align=0, wtile_off=0, modes=BOTH, seg=0, follow=None):
    return Case(family, name, bytes(stream), in_align, out_align, wtile_off, modes, seg, follow)


def _stream(elements, seed=0x65):
    return bytes([MAGIC, seed]) + np.asarray(elements, np.uint8).tobytes()


def _filler(n, rng):
    """elements of every class, two-byte and one-byte ones mixed"""
    return rng.choice(np.array([0x99, 0x8B, 0x94, 0xA2, 0x41, 0x33, 0x4A, 0x6F, 0x20, 0x65, 0xF7, 0x08], np.uint8), n)


def plant(el, B, pattern):
    """one pattern across the cut before element B"""
    put = {"hh": {-2: KILL, -1: 0x9A, 0: 0xB9},
           "split": {-3: KILL, -2: GEN, -1: PROP, 0: 0x5A},
           "lit_before": {-2: KILL, -1: LITK, 0: 0x9C},
           "gen_last": {-2: KILL, -1: 0x93, 0: 0x2B},
           "prop_run": {-4: KILL, -3: 0x95, -2: 0x31, -1: 0x42, 0: 0x53, 1: 0x64, 2: 0x7F}}[pattern]
    for d, v in put.items():
        el[B + d] = v


def cut_kind(B):
    """the largest unit that begins at element B (B a multiple of 4)"""
    for kind, unit in (("wg_count", 8 * TILE), ("wg_write", 4 * TILE), ("count_wave", 2 * TILE), ("tile", TILE),
                       ("lane", 64), ("block", 16), ("dword", 4)):
        if B % unit == 0:
            return kind
    return None


def cut_pattern(P, B):
    """what the stream does across the cut before element B, or None"""
    if B < 2 or B >= P.x.size:
        return None
    s, H, L = P.s, P.H, P.L
    prop = ~H & ~L
    if not s[B]:
        if not s[B - 1] and not H[B - 1]:
            return "lit_before"
        if L[B - 1] and H[B]:
            return "hh"
        return None
    if H[B - 1] and not L[B - 1] and not s[B - 1]:
        return "gen_last"
    if s[B - 1] and prop[B - 1]:
        return "prop_run" if prop[B] else ("split" if L[B] else None)
    return None


# the cuts planted in a short stream (tile 1 entered in the state asked, tile 2's end) and a long one
SHORT_CUTS = (TILE + 100, TILE + 208, TILE + 448, 3 * TILE)
LONG_CUTS = (2 * TILE, 4 * TILE, 8 * TILE)


def _cuts():
    out = []
    rng = np.random.default_rng(0xC075)
    for e in (0, 1):
        for pat in PATTERNS:
            for name, cuts, n in (("short", SHORT_CUTS, 3 * TILE + 50), ("long", LONG_CUTS, 8 * TILE + 50)):
                el = _filler(n, rng)
                for B in cuts:
                    el[(B - 1) // TILE * TILE - 1] = GEN if e else KILL   # the entry of the tile before the cut
                for B in cuts:
                    plant(el, B, pat)
                out.append(_case("cuts", "%s-%s-e%d" % (name, pat, e), _stream(el), out_align=(len(out) * 5) % 16))
    return out


END_COUNTS = tuple(range(1, 66)) + tuple(c + d for c in (TILE, 2 * TILE, 4 * TILE, 8 * TILE) for d in (-1, 0, 1))
END_ALL = (1, 2, 3, 4, 15, 16, 17, 63, 64, 65) + END_COUNTS[65:]
# the last element: hit hit; a hit, then a literal start with no byte after it; a literal's high nybble
# (the whole byte); entered in state 1 with a hit / with a literal start in its low nybble
ENDS = {"hh": (None, 0x9A), "h_lit": (None, 0xB5), "lit": (None, 0x45), "s1_hit": (GEN, 0x7C), "s1_lit": (GEN, 0x73)}


def _ends():
    rng = np.random.default_rng(0xE7D5)
    out = [_case("ends", "m2", _stream([])), _case("ends", "m3", _stream([0x3B]), out_align=3),
           _case("ends", "m4", _stream([0x94, 0x3C]), out_align=15),
           _case("ends", "seed-e1", _stream(_filler(70, rng), seed=0xE1), out_align=1),
           _case("ends", "seed-84", _stream(_filler(4097, rng), seed=0x84), out_align=9)]
    for count in END_COUNTS:
        kinds = tuple(ENDS) if count in END_ALL else (tuple(ENDS)[count % 5],)
        for k in kinds:
            before, last = ENDS[k]
            if before is not None and count < 2:
                continue
            el = _filler(count, rng)
            if count >= 2:
                el[-2] = KILL if before is None else before
            el[-1] = last
            out.append(_case("ends", "%d-%s" % (count, k), _stream(el), out_align=(count + len(k)) % 16))
    return out


def _dense():
    rng = np.random.default_rng(0xDE5E)
    out = []
    hits = rng.choice(np.array([0x88, 0x99, 0xAB, 0xFC, 0xDE, 0x8F], np.uint8), 2 * TILE + 777)
    for ph in range(16):   # a full tile of hits as tile 0, as tile 1, and a partial last one, at every phase
        out.append(_case("dense", "hits-ph%d" % ph, _stream(hits), out_align=ph))
    lits = rng.choice(np.array([0x41, 0x2A, 0x33, 0x7F, 0x00, 0x6B], np.uint8), TILE + 300)
    out.append(_case("dense", "lits", _stream(lits), out_align=7))
    for sh in (0, 1):
        alt = np.tile(np.array([0x9A, 0x4A], np.uint8), TILE)[sh: sh + TILE + 35]
        out.append(_case("dense", "alt%d" % sh, _stream(alt), out_align=2 + 9 * sh))
    # every (nb, L): mixed quads at the four byte phases, and the short last quads (L < 32)
    tails = ([0x41], [0x9A], [0x41, 0x33], [0x9A, 0x41], [0x41, 0x33, 0x2A], [0x9A, 0x9B], [0x9A, 0x9B, 0x41],
             [0x9A, 0x9B, 0x9C])
    for oa in range(4):
        out.append(_case("dense", "mix-a%d" % oa, _stream(_filler(700 + oa, rng)), out_align=oa))
        for k, tail in enumerate(tails):
            out.append(_case("dense", "tail%d-a%d" % (k, oa), _stream([0x41, 0x33, 0x2A, 0x4A] + tail), out_align=oa))
    return out


STORE_BYTES = (1, 2, 15, 16, 17, 31, 32, 33)


def _stores():
    rng = np.random.default_rng(0x5702)
    out = []
    for off in range(16):
        for nb in STORE_BYTES:
            el = _filler(TILE + nb, rng)
            el[TILE - 1] = KILL
            el[TILE:] = rng.choice(np.array([0x41, 0x2A, 0x33, 0x7F], np.uint8), nb)   # one byte each
            out.append(_case("stores", "off%d-b%d" % (off, nb), _stream(el), out_align=off))
    return out


def _align():
    rng = np.random.default_rng(0xA119)
    out = []
    for n in (50, TILE + 1, 2 * TILE + 9):
        el = _filler(n, rng)
        for a in (0, 1, 2, 3, 5, 14, 15):   # (14: the tiles begin on a granule, sh = 0)
            out.append(_case("align", "n%d-a%d" % (n, a), _stream(el), in_align=a, out_align=(a * 3 + n) % 16))
        out.append(_case("align", "n%d-a0-wtile_off" % n, _stream(el), wtile_off=1, out_align=6))
        out.append(_case("align", "n%d-a0-again" % n, _stream(el), out_align=11))   # the option cleared again
    return out


SCAN_TILES = (1023, 1024, 1025, 2049)


def _scan():
    rng = np.random.default_rng(0x5CA7)
    out = []
    for nt in SCAN_TILES:
        n = (nt - 1) * TILE + 1234
        el = _filler(n, rng)
        run = (GROUP - 3) * TILE - 17
        for gb in range(GROUP, nt, GROUP):   # state 1 carried over 6 tiles and a group's boundary, its generate before
            g0, g1 = run + (gb - GROUP) * TILE, min(n - 3, (gb + 3) * TILE + 5)
            el[g0] = 0x95
            el[g0 + 1: g1] = rng.choice(np.array([0x41, 0x33, 0x12, 0x70], np.uint8), g1 - g0 - 1)
        out.append(_case("scan", "t%d" % nt, _stream(el), modes=STATIC, out_align=nt % 16))
        if nt == GROUP + 1:   # the same stream without its generate: state 0 crosses
            el = el.copy()
            el[run] = KILL
            out.append(_case("scan", "t%d-no-generate" % nt, _stream(el), modes=STATIC, out_align=5))
    return out


def _types():
    rng = np.random.default_rng(0x7E5)
    text = bytes(rng.integers(0, 256, TILE, dtype=np.uint8))
    return [_case("types", "empty", b""), _case("types", "af-alone", bytes([MAGIC]), out_align=3),
            _case("types", "literal-1", b" "), _case("types", "literal-2", b" \xe9", out_align=1),
            _case("types", "literal-4097", b" " + text, out_align=13),
            _case("types", "type-08", b"\x08" + text[:99], out_align=2), _case("types", "type-7f-alone", b"\x7f")]


RESOLVE_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 4160)


def _random_tokens(n, rng):
    return even([("hit", int(rng.integers(0, 8))) if rng.random() < 0.55 else ("lit", int(rng.integers(0, 0x80)))
                 for _ in range(n)])


def _resolve():
    rng = np.random.default_rng(0x4E50)
    out = [_case("resolve", "n%d" % n, pack_tokens(0x65, _random_tokens(n, rng)), modes=ADAPTIVE, out_align=n % 16)
           for n in RESOLVE_COUNTS]
    # every context, every rank, the previous byte with bit 2 clear and set
    toks = [t for c in range(16) for b in (0, 1) for r in range(8) for t in (("lit", (c << 3) | (b << 2) | (r & 3)), ("hit", r))]
    out.append(_case("resolve", "ctx-rank", pack_tokens(0x20, toks), modes=ADAPTIVE, out_align=4))
    # a literal at each position of its list (a fresh context each), and absent
    toks = []
    for p, c in enumerate((0, 1, 2, 3, 5, 6, 7, 8)):   # (contexts no byte of this case leads to otherwise)
        toks += [("lit", (c << 3) | 1), ("lit", DICT[p])]
    toks += [("lit", (9 << 3) | 1), ("lit", 0x5A)]
    out.append(_case("resolve", "lit-pos", pack_tokens(0x65, toks), modes=ADAPTIVE, out_align=8))
    # 0x00: absent, then in its list at 0, then further back (its own context is 0)
    toks = [("lit", 0x51), ("lit", 0x00), ("lit", 0x00), ("lit", 0x03), ("lit", 0x05), ("lit", 0x00), ("lit", 0x00),
            ("hit", 2)]
    out.append(_case("resolve", "zero", pack_tokens(0x65, even(toks)), modes=ADAPTIVE, out_align=12))
    # v at p and v ^ 1 at p + 1: context 5 holds 0x28..0x2F, whose bytes keep the context
    for name, fill in (("lo", []), ("hi", [0x2C, 0x2D, 0x2E, 0x2F])):
        toks = [("lit", v) for v in [0x28, 0x2B, 0x2A] + fill + [0x2A]] + [("hit", r) for r in (0, 1, 5, 7)]
        out.append(_case("resolve", "swar-" + name, pack_tokens(0x65, even(toks)), modes=ADAPTIVE, out_align=1))
    # nine different literals into context 11 (0x59 sends the context there), then the list read out
    toks = []
    for v in list(range(0x10, 0x18)) + [0x1B]:
        toks += [("lit", 0x59), ("lit", v)]
    for r in range(8):
        toks += [("lit", 0x59), ("hit", r)]
    out.append(_case("resolve", "nine", pack_tokens(0x65, even(toks)), modes=ADAPTIVE, out_align=15))
    return out


SEGS = (64, 65, 100, 128, 4096)
TOUCH_ALL = [("lit", (c << 3) | 1) for c in range(16)] + [("lit", 0x02)]   # every context's list leaves the initial


def _segments():
    rng = np.random.default_rng(0x5E65)
    follow = pack_tokens(0x74, _random_tokens(150, rng))
    out = []
    for seg in SEGS:
        for n in (seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1, 3 * seg + 7):
            toks = even(TOUCH_ALL + _random_tokens(n - len(TOUCH_ALL), rng))
            out.append(_case("segments", "s%d-n%d" % (seg, n), pack_tokens(0x6F, toks), modes=ADAPTIVE, seg=seg,
                             follow=follow, out_align=(seg + n) % 16))
    return out


FAMILIES = {"cuts": _cuts, "ends": _ends, "dense": _dense, "stores": _stores, "align": _align, "scan": _scan,
            "types": _types, "resolve": _resolve, "segments": _segments}
_CAT = {}


def catalogue(family=None):
    """the cases of a family (built once), or all of them"""
    if family is None:
        return [c for f in FAMILIES for c in catalogue(f)]
    if family not in _CAT:
        _CAT[family] = FAMILIES[family]()
    return _CAT[family]


_WANT = {}


def expected(stream, modify):
    """orc.nybble_decompress of a stream, computed once"""
    key = (stream, bool(modify))
    if key not in _WANT:
        _WANT[key] = orc.nybble_decompress(stream, bool(modify))
    return _WANT[key]
