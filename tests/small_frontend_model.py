"""A plain model of the small front-end and the geometry of its device kernels (TEST
INFRASTRUCTURE, shared by test_small_frontend_cpu.py and test_gpu_small_frontend.py).

The model restates small_compression.c:507-665 element by element with numpy: stream byte i
(i >= 1) emits nothing when it is the letter of a pair, 0x80 + the letter when it is the space
of one, and itself otherwise; a pair is ' ' followed by 'a'..'z', and stream bytes 0-1 never
close one (byte 0 is copied raw, :610). test_small_frontend_cpu.py pins it to the oracle.

The geometry restates sm_tile / SmMode of dc_core.hip: everything k_small_tiles and
k_small_write cut at lies on the 16-byte address grid of element 0, so the inputs that put
pairs on those cuts are built from the address the input will have.
"""
import functools

import numpy as np

SPACE = 0x20


def _a(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), np.uint8)


def _lower(a):
    return (a >= ord("a")) & (a <= ord("z"))


# ---- the model ---------------------------------------------------------------------------
def fe_body(y, left_halo, nelem):
    """dc_small_compress_body's contract (dc_gpu.h): the front-end output of stream bytes
    y[1 .. nelem], no header, no LITERAL fallback; y[0] is left context when left_halo, else
    the stream's raw first byte; y[nelem + 1], when present, is the right halo."""
    a = _a(y)
    if nelem == 0:
        return b""
    assert nelem + 1 <= a.size
    i = np.arange(1, nelem + 1)
    low, sp = _lower(a), a == SPACE
    second = sp[i - 1] & low[i]
    if not left_halo:
        second &= i >= 2
    nxt_low = np.zeros(nelem, bool)
    has = i + 1 < a.size
    nxt_low[has] = low[i[has] + 1]
    start = sp[i] & nxt_low
    val = a[i].astype(np.int64)
    val[start] = 0x80 + a[i[start] + 1]
    return val[~second].astype(np.uint8).tobytes()


def fe_pairs(x):
    """The pairs the front-end codes in the whole stream x."""
    n = len(x)
    return (n - 1) - len(fe_body(x, False, n - 1)) if n else 0


def fe_stream(x):
    """dc_small_compress / compress_bytestring: type byte 8, the raw first byte, the body; or
    ' ' + x (LITERAL) when that is not shorter than x (:651-664)."""
    x = bytes(x)
    n = len(x)
    if n == 0:
        return b" "
    body = fe_body(x, False, n - 1)
    if 2 + len(body) >= n:
        return b" " + x
    return bytes([8, x[0]]) + body


def fe_unbody(b):
    """dc_small_decompress_body: every byte >= 0x80 becomes ' ' and the byte - 0x80."""
    a = _a(b)
    pair = a >= 0x80
    pos = np.arange(a.size) + np.cumsum(pair) - pair
    out = np.empty(a.size + int(pair.sum()), np.uint8)
    out[pos] = np.where(pair, SPACE, a)
    out[pos[pair] + 1] = a[pair] & 0x7F
    return out.tobytes()


def fe_unstream(c):
    """dc_small_decompress / decompress_bytestring (:453-505): type 8 -> the raw byte c[1] and
    the decoded body; ' ' -> the bytes after it; anything else is invalid: empty."""
    c = bytes(c)
    if not c:
        return b""
    if c[0] == 8:
        return c[1:2] + fe_unbody(c[2:]) if len(c) >= 2 else b""
    if c[0] == SPACE:
        return c[1:]
    return b""


# ---- the kernels' geometry -----------------------------------------------------------------
# mode -> (FsmOff: the stream index of element 0, SmMode::tile)
MODES = {"ENC": (1, 16384), "BODY0": (1, 16384), "BODY1": (1, 16384), "DEC": (2, 8192), "DBODY": (0, 8192)}
ENC_TILE, DEC_TILE = 16384, 8192
# what each kernel cuts at, in bytes from the granule of element 0 (DESIGN.md has the table)
ENC_EDGES = {"dword": 4, "uint4": 16, "lane": 64, "quarter": 256, "step": 1024, "wave": 4096, "tile": 16384}
DEC_EDGES = {"dword": 4, "uint4": 16, "lane": 32, "quarter": 256, "step": 1024, "wave": 2048, "tile": 8192}


def grid_origin(addr, off):
    """Stream index of grid byte 0 (sm_tile's T.base of tile 0): <= off, may be negative."""
    return off - ((addr + off) & 15)


def tiles(addr, off, nelem, length, tile):
    """sm_tile for every tile of the launch: base, lo, hi, two, nxt and the interior flag."""
    lead = (addr + off) & 15
    clamp = lambda v: min(max(v, 0), tile)
    out = []
    for t in range((lead + nelem + tile - 1) // tile if nelem else 0):
        base = off - lead + t * tile
        T = {"base": base, "lo": clamp(off - base), "hi": clamp(off + nelem - base), "two": clamp(2 - base),
             "nxt": clamp(length - 1 - base)}
        T["interior"] = T["lo"] == 0 and T["hi"] == tile and T["two"] == 0 and T["nxt"] == tile
        out.append(T)
    return out


# ---- inputs ----------------------------------------------------------------------------------
_POOL = np.frombuffer(b"etaoinshrdlucmfwypetaoinshrdlu" + b" " * 14 + b"ABCXYZ" + b"0123.,:-/\n" +
                      bytes([0x00, 0x60, 0x7B, 0x7F, 0x80, 0xE1, 0xFA, 0xFF]), np.uint8)


def text(n, seed):
    """Dense in pairs and lone spaces, with a few bytes of every other kind (0x00, the
    neighbours of 'a' and 'z', bytes >= 0x80, which the encoder passes through)."""
    return _POOL[np.random.default_rng(seed).integers(0, _POOL.size, size=n)].copy()


# name -> (bytes, k): bytes[k] is the first byte at or after the edge
CASES = {
    "pair_ends_on_edge": (b" q", 2),
    "pair_straddles_edge": (b" q", 1),
    "pair_starts_on_edge": (b" q", 0),
    "uppercase_straddles": (b" Q", 1),
    "lone_space_then_pair": (b"  a", 2),
    "space_then_a_minus_1": (b" `", 1),
    "space_then_z_plus_1": (b" {", 1),
    "space_then_nul": (b" \x00", 1),
    "space_then_e1": (b" \xe1", 1),
    "repeated_pairs": (b" a a a", 3),
}
ENC_N = 2 * ENC_TILE + 1100   # a partial first tile, an interior tile, a partial last tile


def enc_sites(addr, n=ENC_N):
    """(edge name, grid byte u, stream index e) of the places where a case is planted: for each
    edge width E one multiple of E that is no multiple of the next wider edge, in each of the
    tiles; the tile edge itself between the tiles. No two closer than 16 bytes."""
    org = grid_origin(addr, 1)
    widths = sorted(ENC_EDGES.items(), key=lambda kv: kv[1])
    taken, out = [], []
    for k, (name, E) in enumerate(widths):
        wider = widths[k + 1][1] if k + 1 < len(widths) else None
        for t in range(3):
            lo, hi = t * ENC_TILE + 24, min((t + 1) * ENC_TILE, n - 8 - org)   # stream indices 8 .. n - 8
            if wider is None:
                cand = [t * ENC_TILE] if t else []
            else:
                cand = [u for u in range(t * ENC_TILE + E, (t + 1) * ENC_TILE, E) if u % wider and lo <= u < hi]
            for u in cand:
                if all(abs(u - v) >= 16 for v in taken):
                    taken.append(u)
                    out.append((name, u, org + u))
                    break
    return out


@functools.lru_cache(maxsize=None)
def _planted(case, lead):
    seq, k = CASES[case]
    x = text(ENC_N, seed=0x5F + lead)
    sites = enc_sites(lead)
    for _, _, e in sites:
        s = e - k
        assert s - 1 >= 3 and s + len(seq) + 1 <= ENC_N
        x[s - 1] = ord("X")               # nothing before or after the case joins it
        x[s: s + len(seq)] = _a(seq)
        x[s + len(seq)] = ord("X")
    x.setflags(write=False)
    return x, tuple(sites)


def planted(case, addr):
    """The ENC_N-byte input for an encoder whose d_in will be at address addr, with `case` on
    every site of enc_sites(addr); and the sites. Only addr & 15 matters."""
    return _planted(case, addr & 15)


SHORT = text(80, seed=0x51)                       # lengths 1..80 are its prefixes
SHORT_BODY = np.random.default_rng(0x52).integers(0, 256, size=80).astype(np.uint8)
SHORT_STREAM = np.concatenate([[8], SHORT_BODY[:79]]).astype(np.uint8)


def around_tiles(tile):
    """tile - 2 .. tile + 2 and 2 * tile - 2 .. 2 * tile + 2"""
    return [t + d for t in (tile, 2 * tile) for d in range(-2, 3)]


AROUND = text(2 * ENC_TILE + 2, seed=0x53)
AROUND_BODY = np.random.default_rng(0x54).integers(0, 256, size=2 * DEC_TILE + 2).astype(np.uint8)
AROUND_STREAM = np.concatenate([[8], AROUND_BODY[:-1]]).astype(np.uint8)


def with_pairs(n, pairs):
    """n bytes with exactly `pairs` pairs, as far apart as they fit: the first at bytes 1-2, the
    last on the last two bytes. None when n is too short for them."""
    x = np.full(n, ord("x"), np.uint8)
    if pairs == 0:
        return x
    if n < 1 + 2 * pairs:
        return None
    at = [1] if pairs == 1 else [1, n - 2]
    for s in at:
        x[s], x[s + 1] = SPACE, ord("k")
    return x


LITERAL_N = (2, 3, 17, ENC_TILE, ENC_TILE + 1)


def literal_inputs():
    """(n, pairs, x) around the LITERAL threshold: 0 and 1 pairs are LITERAL, 2 are type 8."""
    return [(n, p, with_pairs(n, p)) for n in LITERAL_N for p in (0, 1, 2) if with_pairs(n, p) is not None]


E1, E2, E3 = 0x80 + ord("a"), 0x80 + ord("b"), 0x80 + ord("c")
# name -> (mode, input, nelem, expected output), the expected bytes written out by hand
STREAM_ENDS = {
    "bytes_0_1_never_pair": ("ENC", b" qx a b c", None, bytes([8, 32, ord("q"), ord("x"), E1, E2, E3])),
    "bytes_1_2_pair": ("ENC", b"x a b c", None, bytes([8, ord("x"), E1, E2, E3])),
    "last_space_stays": ("ENC", b"x a b c ", None, bytes([8, ord("x"), E1, E2, E3, 32])),
    "body0_bytes_0_1_never_pair": ("BODY0", b" qx a b c", 8, bytes([ord("q"), ord("x"), E1, E2, E3])),
    "body0_right_halo_pairs": ("BODY0", b"xx a b c", 6, bytes([ord("x"), E1, E2, E3])),
    "body0_no_halo_space_stays": ("BODY0", b"xx a b ", 6, bytes([ord("x"), E1, E2, 32])),
    "body1_right_halo_pairs": ("BODY1", b"xx a b c", 6, bytes([ord("x"), E1, E2, E3])),
    "body1_no_halo_space_stays": ("BODY1", b"xx a b ", 6, bytes([ord("x"), E1, E2, 32])),
    "body1_halo_space_closes_pair": ("BODY1", b" qx a", 4, bytes([ord("x"), E1])),
    "body0_same_input_keeps_q": ("BODY0", b" qx a", 4, bytes([ord("q"), ord("x"), E1])),
    "body1_halo_space_uppercase": ("BODY1", b" Qx", 2, b"Qx"),
    "body1_bytes_1_2_pair": ("BODY1", b"x ab", 3, bytes([E1, ord("b")])),
    "body0_bytes_1_2_pair": ("BODY0", b"x ab", 3, bytes([E1, ord("b")])),
}

DEC_N = 3 * DEC_TILE + 1000   # a partial first tile, two interior tiles (16 KiB), a partial last


@functools.lru_cache(maxsize=None)
def dec_bodies():
    """Arbitrary bodies: uniform bytes, every byte >= 0x80 (the output is 2 m: the fullest
    stage), no byte >= 0x80."""
    rng = np.random.default_rng(0x55)
    out = {"uniform": rng.integers(0, 256, size=DEC_N), "all_high": rng.integers(0x80, 256, size=DEC_N),
           "none_high": rng.integers(0, 0x80, size=DEC_N)}
    return {k: v.astype(np.uint8) for k, v in out.items()}


def dec_interior_dwords(a, addr, mode, out_addr):
    """For a decode of the m bytes `a` at address addr into out_addr: the (pattern of bytes >=
    0x80, byte phase of the output position on entry) of every dword of the interior tiles, as
    k_small_write's v_perm path meets them. pattern bit k = byte k of the dword."""
    off, tile = MODES[mode]
    a = _a(a)
    nelem = a.size - off
    high = (a >= 0x80).astype(np.int64)
    head = 1 if mode == "DEC" else 0
    pos = head + np.arange(nelem) + np.cumsum(high[off:]) - high[off:]   # output index of each element
    pats, phases = [], []
    for T in tiles(addr, off, nelem, a.size, tile):
        if not T["interior"]:
            continue
        k = T["base"] + np.arange(0, tile, 4)
        pats.append(high[k] + 2 * high[k + 1] + 4 * high[k + 2] + 8 * high[k + 3])
        phases.append((out_addr + pos[k - off]) & 3)
    if not pats:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(pats), np.concatenate(phases)
