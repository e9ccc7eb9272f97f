"""A plain model of the two persisted Huffman formats of csrc/dc_host.hip: the "DCH1" binary
container (include/dc_host.h) and the netstring container (DESIGN.md "Netstring container"), with
the case catalogues of test_container_model_cpu.py and test_gpu_container.py (TEST INFRASTRUCTURE:
numpy and the oracle only, no import of the product).

Everything starts from the oracle: orc.huffman_lengths, orc.canonical, orc.bitcodes, orc.huff_pack
with sync_syms, orc.sync_compact and orc.base64url. The model then states

  writers   dch1_bytes, netstring_bytes: the bytes a writer must produce, the writer's decisions
            included (the sync size it picks, raw or Huffman form and why)
  parsers   parse_dch1, parse_netstring: a container as its pieces (lengths, index, payload bits,
            raw runs), by the reader's rules (whitespace, "%i" lengths, skipped "#" blocks);
            decode_dch1 / decode_netstring decode the pieces with orc.huff_unpack
  rules     index_ok (the index rule), dch1_ok (the header rule and the index rule), netstring_ok
            (what the host can see of a netstring container), written here from the documents and
            not from csrc/dc_container_check.h

The order of the netstring writer's decisions is dc_huff_compress_netstring's: (1) the table has no
stream of <= 32 bits per code, (2) a length over 35 has no character, (3) the Huffman form is not
smaller than the raw form, (4) a byte of the input has no code. (3) is decided from the planned
bits, in which a byte without a code counts as 0 bits, before the pack finds (4).
"""
import functools

import numpy as np

from oracle import oracle as orc

HEADER = 288
MAGIC = b"DCH1"
GROUP = 64
NS_MAX = 32768                       # payload bytes of a block, type bytes included
LEN_CHARS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
MAX_DIGITS = 128
MAX_SYMS = 1024
OK, E_ARG, E_CODE_TOO_LONG, E_NOCODE, E_CAPACITY, E_STREAM = 0, -1, -3, -4, -6, -7


class Refused(Exception):
    """a writer's status other than DC_OK"""

    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


class Malformed(Exception):
    """a container a reader must answer with DC_E_STREAM"""


# ---- arithmetic ------------------------------------------------------------------------------
def digit_bits(n_ary):
    return max(1, (n_ary - 1).bit_length())


def sync_ok(S):
    return 16 <= S <= 1024 and S & (S - 1) == 0


def chunks(n, S):
    return -(-n // S)


def groups(n, S):
    return -(-chunks(n, S) // GROUP)


def index_bytes(n, S):
    return 8 * groups(n, S) + 2 * chunks(n, S)


def choose_sync(n, bits):
    """dc_huff_choose_sync, restated"""
    if n == 0:
        return 64
    return 64 if 64.0 * 64.0 * (bits / n) / 8.0 <= 4200.0 else 32


def compress_bound(n, S):
    """dc_huff_compress_bound"""
    return HEADER + index_bytes(n, S or 64) + 4 * n + 64


def netstring_bound(n):
    return len_raw(n) + 16


# ---- the code of an input ----------------------------------------------------------------------
def code_of(x, n_ary, lengths=None, M=258):
    """The table a writer builds: L (lengths in digits of symbols 0..M, as given or from x's own
    histogram), el / ev (the canonical code; its min / max scan stops before M as the reference's
    does), the packed codes of the bytes, max_bits (33: some byte's code passes 32 bits), bits (the
    planned payload bits; a byte without a code counts 0) and nocode."""
    x = np.ascontiguousarray(x, np.uint8)
    hist = orc.histogram(x) if x.size else np.zeros(256, np.uint64)
    if lengths is None:
        M = 258
        L = np.asarray(orc.huffman_lengths(hist, n_ary), np.int32)
    else:
        L = np.asarray(lengths, np.int32)[: M + 1]
        assert L.size == M + 1
    size = max(M + 1, 259)
    el, ev = orc.canonical(L, n_ary, max_sym=M, size=size)
    w = digit_bits(n_ary)
    t = {"L": L, "M": M, "el": el, "ev": ev, "w": w, "n_ary": n_ary, "hist": hist,
         "bad": bool(L[:M].size and int(L[:M].max()) > MAX_DIGITS)}
    lb = el[:256].astype(np.int64) * w
    if lb.max() > 32:
        t.update(max_bits=33, code=None, nb=None, bits=None, nocode=None)
        return t
    code, nb, mx = orc.bitcodes(el[:256], ev[:256], n_ary)
    assert mx == lb.max()
    t.update(max_bits=int(mx), code=code, nb=nb, bits=int((hist * nb.astype(np.uint64)).sum()),
             nocode=bool(((hist > 0) & (nb == 0)).any()))
    return t


def packed(x, t, S):
    """(payload bytes, bits, bases u64, lens u16) of x under the table t"""
    x = np.ascontiguousarray(x, np.uint8)
    if x.size == 0:
        return np.zeros(0, np.uint8), 0, np.zeros(0, np.uint64), np.zeros(0, np.uint16)
    payload, bits, idx = orc.huff_pack(x, t["code"], t["nb"], sync_syms=S)
    bases, lens = orc.sync_compact(idx, 0, bits)
    return payload[: (bits + 7) // 8], bits, bases.astype(np.uint64), lens.astype(np.uint16)


# ---- DCH1 --------------------------------------------------------------------------------------
def dch1_pieces(n_ary, n, bits, S, len_bytes, bases, lens, payload, version=1, w=None, flags=0):
    """the layout of include/dc_host.h from its pieces (any of them may be wrong on purpose)"""
    h = np.zeros(HEADER, np.uint8)
    h[:4] = np.frombuffer(MAGIC, np.uint8)
    h[4:8] = [version, n_ary, digit_bits(n_ary) if w is None else w, flags]
    h[8:16] = np.array([n], np.uint64).view(np.uint8)
    h[16:24] = np.array([bits], np.uint64).view(np.uint8)
    h[24:28] = np.array([S], np.uint32).view(np.uint8)
    h[32:288] = np.asarray(len_bytes, np.uint8)[:256]
    return (h.tobytes() + np.asarray(bases, np.uint64).tobytes() + np.asarray(lens, np.uint16).tobytes() +
            np.asarray(payload, np.uint8).tobytes())


def dch1_bytes(x, n_ary, S, lengths=None, M=258):
    """What dc_huff_compress_host writes; Refused(status) where it writes nothing."""
    x = np.ascontiguousarray(x, np.uint8)
    if not 2 <= n_ary <= 16 or (S and not sync_ok(S)):
        raise Refused(E_ARG)
    t = code_of(x, n_ary, lengths, M)
    if t["bad"]:
        raise Refused(E_ARG)
    if t["max_bits"] > 32:
        raise Refused(E_CODE_TOO_LONG)
    if S == 0:
        S = choose_sync(x.size, t["bits"])
    if t["nocode"]:
        raise Refused(E_NOCODE)
    payload, bits, bases, lens = packed(x, t, S)
    return dch1_pieces(n_ary, x.size, bits, S, np.maximum(t["el"][:256], 0), bases, lens, payload)


def parse_dch1(blob):
    """The fields of a DCH1 container, unjudged (dch1_ok judges); Malformed where the sections do
    not fit the bytes."""
    b = np.frombuffer(bytes(blob), np.uint8)
    if b.size < HEADER or bytes(b[:4]) != MAGIC:
        raise Malformed("header")
    p = {"version": int(b[4]), "n_ary": int(b[5]), "w": int(b[6]), "flags": int(b[7]),
         "n": int(b[8:16].view(np.uint64)[0]), "bits": int(b[16:24].view(np.uint64)[0]),
         "S": int(b[24:28].view(np.uint32)[0]), "lengths": b[32:288].astype(np.int32), "m": b.size}
    if not sync_ok(p["S"]):
        raise Malformed("S")
    ng, nc = groups(p["n"], p["S"]), chunks(p["n"], p["S"])
    nbytes = -(-p["bits"] // 8)
    if HEADER + 8 * ng + 2 * nc + nbytes > b.size:
        raise Malformed("size")
    o = HEADER
    p["bases"] = b[o: o + 8 * ng].copy().view(np.uint64)
    o += 8 * ng
    p["lens"] = b[o: o + 2 * nc].copy().view(np.uint16)
    o += 2 * nc
    p["payload"] = b[o: o + nbytes]
    return p


def index_ok(n, S, bases, lens, bits, bit_base=0):
    """The index rule (DESIGN.md "Containers read from a file"): S valid; as many bases and lengths
    as n and S give; bases[0] == bit_base; each base + its group's 64 lengths == the next base; the
    last == bit_base + bits; a chunk of k symbols is at most 32 k bits long."""
    if not sync_ok(S):
        return False
    nc, ng = chunks(n, S), groups(n, S)
    if len(bases) != ng or len(lens) != nc:
        return False
    pos = bit_base
    for g in range(ng):
        if int(bases[g]) != pos:
            return False
        for c in range(g * GROUP, min(g * GROUP + GROUP, nc)):
            if int(lens[c]) > 32 * min(S, n - c * S):
                return False
            pos += int(lens[c])
    return pos == bit_base + bits


def dch1_ok(blob):
    """The header rule and the index rule of a DCH1 container"""
    try:
        p = parse_dch1(blob)
    except Malformed:
        return False
    if p["version"] != 1 or not 2 <= p["n_ary"] <= 16 or p["w"] != digit_bits(p["n_ary"]) or p["flags"]:
        return False
    if int(p["lengths"].max()) > MAX_DIGITS or p["bits"] > 32 * p["n"]:
        return False
    return index_ok(p["n"], p["S"], p["bases"], p["lens"], p["bits"])


def unpack(payload, bits, n, lengths, M, n_ary):
    if n == 0:
        return b""
    size = max(M + 1, 259)
    el, ev = orc.canonical(np.asarray(lengths, np.int32)[: M + 1], n_ary, max_sym=M, size=size)
    buf = np.concatenate([np.asarray(payload, np.uint8), np.zeros(8, np.uint8)])
    return orc.huff_unpack(buf, bits, n, el, ev, n_ary, max_sym=M).tobytes()


def decode_dch1(blob):
    p = parse_dch1(blob)
    return unpack(p["payload"], p["bits"], p["n"], p["lengths"], 258, p["n_ary"])


# ---- netstrings --------------------------------------------------------------------------------
def block(payload, fmt="%d"):
    return (fmt % len(payload)).encode() + b":" + payload + b","


def framed(text, prefix, C=None, fmt="%d"):
    """text in blocks of prefix + up to C characters (the writer: all that a block holds)"""
    C = NS_MAX - len(prefix) if C is None else C
    return b"".join(block(prefix + text[i: i + C], fmt) for i in range(0, len(text), C))


def raw_bytes(x, fmt="%d"):
    """the reference's pass-through form: blocks of <= 32766 bytes; an empty input is one empty block"""
    x = bytes(x)
    return framed(x, b"\n\n", fmt=fmt) if x else b"2:\n\n,"


def framed_len(nchar, tl):
    """bytes of nchar characters in blocks of tl prefix bytes + up to 32768 - tl characters"""
    C = NS_MAX - tl
    full, last = divmod(nchar, C)
    return full * (len(str(NS_MAX)) + 1 + NS_MAX + 1) + (len(str(last + tl)) + 1 + tl + last + 1 if last else 0)


def len_raw(n):
    return framed_len(n, 2) if n else 5


def huffman_size(n, n_ary, bits, S, M):
    """bytes of the Huffman form: #dc1 and X blocks, the index text and the payload text framed"""
    meta = len("\n#dc1 n=%d syms=%d bits=%d S=%d M=%d" % (n_ary, n, bits, S, M))
    xb = len("\nX%d:" % M) + M + 1
    return (len(str(meta)) + 1 + meta + 1) + (len(str(xb)) + 1 + xb + 1) + \
        framed_len(-(-index_bytes(n, S) * 8 // 6), 8) + framed_len(-(-bits // 6), 2)


def segment(x, t, S, fmt="%d", zsplit=None, isplit=None, alt=False, with_M=True, between=b"", xlen=None):
    """One Huffman segment of x under the table t. The writer's form by default; for reader-only
    inputs: fmt (how block lengths are written), zsplit / isplit (characters per Z / #dcidx block),
    alt ("+" and "/" for "-" and "_"), with_M (False: no M= in #dc1), between (bytes put between
    consecutive Z blocks and between consecutive #dcidx blocks)."""
    x = np.ascontiguousarray(x, np.uint8)
    payload, bits, bases, lens = packed(x, t, S)
    M = t["M"]
    meta = "\n#dc1 n=%d syms=%d bits=%d S=%d" % (t["n_ary"], x.size, bits, S) + (" M=%d" % M if with_M else "")
    xb = "\nX%d:" % M + "".join(LEN_CHARS[max(int(v), 0)] for v in t["L"][: M + 1])
    ibytes = np.frombuffer(bases.tobytes() + lens.tobytes(), np.uint8)
    itext = orc.base64url(ibytes, ibytes.size * 8)
    ztext = orc.base64url(payload, bits)
    if alt:
        itext, ztext = (s.replace(b"-", b"+").replace(b"_", b"/") for s in (itext, ztext))

    def blocks(text, prefix, C):
        C = NS_MAX - len(prefix) if C is None else C
        return between.join(block(prefix + text[i: i + C], fmt) for i in range(0, len(text), C))

    return block(meta.encode(), fmt) + block(xb.encode(), fmt) + blocks(itext, b"\n#dcidx:", isplit) + \
        blocks(ztext, b"\nZ", zsplit)


def netstring_form(x, n_ary, S, lengths=None, M=258):
    """(bytes, why): what dc_huff_compress_netstring writes and which decision made it: "huffman",
    or raw for "empty", "maxbits", "len35", "notsmaller", "nocode", in the writer's order."""
    x = np.ascontiguousarray(x, np.uint8)
    if not 2 <= n_ary <= 256 or (S and not sync_ok(S)) or (lengths is not None and not 0 <= M < MAX_SYMS):
        raise Refused(E_ARG)
    if x.size == 0:
        return raw_bytes(x), "empty"
    t = code_of(x, n_ary, lengths, M)
    if t["bad"] or t["max_bits"] <= 0 or t["max_bits"] > 32:
        return raw_bytes(x), "maxbits"
    if int(t["L"].max()) > 35:
        return raw_bytes(x), "len35"
    if S == 0:
        S = choose_sync(x.size, t["bits"])
    # the size test comes before the pack and sees the planned bits: zero for a byte without a code
    if huffman_size(x.size, n_ary, t["bits"], S, t["M"]) >= len_raw(x.size):
        return raw_bytes(x), "notsmaller"
    if t["nocode"]:
        return raw_bytes(x), "nocode"
    seg = segment(x, t, S)
    assert len(seg) == huffman_size(x.size, n_ary, t["bits"], S, t["M"])
    return seg, "huffman"


def netstring_bytes(x, n_ary, S, lengths=None, M=258):
    return netstring_form(x, n_ary, S, lengths, M)[0]


def _strtoll0(s):
    """strtoll(s, &end, 0) on the text before ':': sign, 0x hex, 0 octal, else decimal; the value of
    the longest prefix that is a number, None where there is none"""
    i, neg = 0, False
    if i < len(s) and s[i] in "+-":
        neg = s[i] == "-"
        i += 1
    if s[i: i + 2].lower() == "0x" and i + 2 < len(s) and s[i + 2] in "0123456789abcdefABCDEF":
        base, i, digs = 16, i + 2, "0123456789abcdefABCDEF"
    elif s[i: i + 1] == "0":
        base, digs = 8, "01234567"
    else:
        base, digs = 10, "0123456789"
    j = i
    while j < len(s) and s[j] in digs:
        j += 1
    if j == i:
        return None
    v = int(s[i:j], base)
    return -v if neg else v


def ns_blocks(blob):
    """[(type, payload, offset)] by ns_next's rules: leading whitespace skipped, a NUL or the end
    of the bytes ends the walk, the length is "%i" text of at most 31 characters before ':', 2 <=
    length <= 32768, the payload starts with '\\n' and is followed by ',' inside the bytes."""
    blob = bytes(blob)
    out, q, m = [], 0, len(blob)
    while True:
        while q < m and blob[q] in b" \n\t\r":
            q += 1
        if q >= m or blob[q] == 0:
            return out
        k = 0
        while q + k < m and k < 31 and blob[q + k] != 0x3A:
            k += 1
        if q + k >= m or blob[q + k] != 0x3A or k == 0:
            raise Malformed("length")
        ln = _strtoll0(blob[q: q + k].decode("latin-1"))
        if ln is None or ln < 2 or ln > NS_MAX:
            raise Malformed("length value")
        d = q + k + 1
        if d + ln >= m or blob[d + ln] != 0x2C or blob[d] != 0x0A:
            raise Malformed("frame")
        out.append((chr(blob[d + 1]), blob[d + 2: d + ln], d + 2))
        q = d + ln + 1


def _meta(payload, key):
    """key=value of a #dc1 block: the key at the start or after a space, a decimal value (clamped at
    2^64 - 1 as strtoull clamps)"""
    kl = len(key)
    for i in range(len(payload) - kl - 1):
        if (i == 0 or payload[i - 1] == 0x20) and payload[i: i + kl] == key and payload[i + kl] == 0x3D:
            j = i + kl + 1
            while j < len(payload) and payload[j] in b" \t\n\r":
                j += 1
            if j < len(payload) and payload[j] in b"+-":
                j += 1
            e = j
            while e < len(payload) and 0x30 <= payload[e] <= 0x39:
                e += 1
            return min(int(payload[j:e] or b"0"), 2 ** 64 - 1)
    return None


_B64_VAL = np.full(256, -1, np.int16)
_B64_VAL[np.frombuffer(B64.encode(), np.uint8)] = np.arange(64)
_B64_VAL[ord("+")], _B64_VAL[ord("/")] = 62, 63


def b64_bytes(text, bits):
    """the first `bits` bits of base64url text (6 per character, MSB first), zero-padded to bytes"""
    v = _B64_VAL[np.frombuffer(bytes(text), np.uint8)]
    if (v < 0).any() or 6 * v.size < bits:
        raise Malformed("text")
    b = ((v[:, None] >> np.arange(5, -1, -1)) & 1).astype(np.uint8).reshape(-1)[:bits]
    return np.packbits(b)


def parse_netstring(blob):
    """[("raw", bytes) | ("huff", {n_ary, syms, bits, S, M, lengths, itext, ztext})] in order, by the
    reader's rules: a raw block or a "#dc1 " block ends the segment before it; "#dcidx:" blocks
    and Z blocks add to the open segment's texts; other "#" blocks are skipped; a finished
    segment needs its metadata (n, syms, bits, S), a table, n_ary 2..256, a valid S, bits <= 32
    syms, ceil(bits / 6) Z characters and ceil(8 ib / 6) index characters. The sum of the sizes
    must stay below 2^64. Malformed otherwise."""
    segs, total = [], 0
    new = lambda: {"meta": False, "table": False, "M": 258, "lengths": np.zeros(MAX_SYMS, np.int32), "itext": b"",
                   "ztext": b""}
    seg = new()

    def close():
        nonlocal seg, total
        if not seg["meta"] and not seg["ztext"]:
            return
        if not seg["meta"] or not seg["table"] or not 2 <= seg["n_ary"] <= 256:
            raise Malformed("segment")
        if not sync_ok(seg["S"]) or seg["bits"] > 32 * seg["syms"] or len(seg["ztext"]) != -(-seg["bits"] // 6):
            raise Malformed("segment metadata")
        if len(seg["itext"]) != -(-index_bytes(seg["syms"], seg["S"]) * 8 // 6):
            raise Malformed("index text")
        total += seg["syms"]
        segs.append(("huff", seg))
        seg = new()

    for typ, payload, _ in ns_blocks(blob):
        if typ == "\n":
            close()
            segs.append(("raw", payload))
            total += len(payload)
        elif typ == "#":
            if payload[:4] == b"dc1 ":
                close()
                vals = [_meta(payload, k) for k in (b"n", b"syms", b"bits", b"S")]
                if None in vals:
                    raise Malformed("#dc1")
                seg["n_ary"], seg["syms"], seg["bits"], seg["S"] = vals
                seg["meta"] = True
                mv = _meta(payload, b"M")
                if mv is not None:
                    seg["M"] = mv
                if seg["M"] >= MAX_SYMS:
                    raise Malformed("M")
            elif payload[:6] == b"dcidx:":
                seg["itext"] += payload[6:]
        elif typ == "X":
            head = payload[:15]
            j = 0
            while j < len(head) and 0x30 <= head[j] <= 0x39:
                j += 1
            if j == 0 or j >= len(head) or head[j] != 0x3A or int(head[:j]) >= MAX_SYMS:
                raise Malformed("X header")
            Mx = int(head[:j])
            if len(payload) != j + 1 + Mx + 1:
                raise Malformed("X count")
            for i, ch in enumerate(payload[j + 1:]):
                if chr(ch) not in LEN_CHARS:
                    raise Malformed("X character")
                seg["lengths"][i] = LEN_CHARS.index(chr(ch))
            seg["M"], seg["table"] = Mx, True
        elif typ == "Z":
            seg["ztext"] += payload
        else:
            raise Malformed("block type")
    close()
    if total >= 2 ** 64:
        raise Malformed("size")
    return segs


def netstring_ok(blob):
    try:
        parse_netstring(blob)
        return True
    except Malformed:
        return False


def netstring_size(blob):
    return sum(len(s) if k == "raw" else s["syms"] for k, s in parse_netstring(blob))


def segment_index(seg):
    """(bases, lens) of a parsed Huffman segment"""
    ng, nc = groups(seg["syms"], seg["S"]), chunks(seg["syms"], seg["S"])
    ib = b64_bytes(seg["itext"], 8 * (8 * ng + 2 * nc))
    return ib[: 8 * ng].copy().view(np.uint64), ib[8 * ng: 8 * ng + 2 * nc].copy().view(np.uint16)


def decode_netstring(blob):
    out = []
    for kind, s in parse_netstring(blob):
        if kind == "raw":
            out.append(s)
            continue
        bases, lens = segment_index(s)
        if not index_ok(s["syms"], s["S"], bases, lens, s["bits"]):
            raise Malformed("index")
        out.append(unpack(b64_bytes(s["ztext"], s["bits"]), s["bits"], s["syms"], s["lengths"], s["M"], s["n_ary"]))
    return b"".join(out)


# ---- inputs ------------------------------------------------------------------------------------
def skew(n, seed, values=b"etaoin s"):
    """compressible bytes: eight values with probabilities from 0.3 to 0.05"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.frombuffer(values, np.uint8), size=n, p=[0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05])


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


FIX4 = np.arange(0x40, 0x50, dtype=np.uint8)     # the 16 byte values of the fixed 4-bit code


def fix4_lengths():
    L = np.zeros(259, np.int32)
    L[FIX4] = 4
    return L


def fix4(n, seed):
    return FIX4[np.random.default_rng(seed).integers(0, 16, n)]


def chain_lengths(m, M=258):
    """lengths 1, 2, .., m, m on bytes 1..m + 1 (a complete binary code)"""
    L = np.zeros(M + 1, np.int32)
    L[1: m + 2] = list(range(1, m + 1)) + [m]
    return L


def chain_input(m, n, seed):
    """every coded byte once, then the six shortest codes"""
    rng = np.random.default_rng(seed)
    return np.concatenate([np.arange(1, m + 2), rng.integers(1, 7, n - m - 1)]).astype(np.uint8)


class Case:
    """One writer call: x, n_ary, S (0: the writer's choice), lengths / M (None: from x). dch1 /
    ns: the call is made on that format."""

    def __init__(self, name, x, n_ary=2, S=64, lengths=None, M=258, dch1=True, ns=True):
        self.name, self.n_ary, self.S, self.lengths, self.M, self.dch1, self.ns = name, n_ary, S, lengths, M, dch1, ns
        self.x = np.ascontiguousarray(x, np.uint8)

    @functools.lru_cache(maxsize=None)
    def dch1_model(self):
        """(status, bytes)"""
        try:
            return OK, dch1_bytes(self.x, self.n_ary, self.S, self.lengths, self.M)
        except Refused as r:
            return r.status, b""

    @functools.lru_cache(maxsize=None)
    def ns_model(self):
        """(bytes, why)"""
        return netstring_form(self.x, self.n_ary, self.S, self.lengths, self.M)

    def __repr__(self):
        return self.name


SIZES_S = (16, 64, 1024)
ARITIES = (2, 3, 4, 9, 16)
NS_ONLY_ARITIES = (17, 256)
RAW_SIZES = (1, 32766, 32767, 65533)
Z_EDGES = (49149, 49150, 98298)
IDX_EDGES = (184976, 184977)


@functools.lru_cache(maxsize=None)
def catalogue():
    cs = []
    for S in SIZES_S:
        x = skew(64 * S + 1, S)
        for n in (0, 1, S - 1, S, S + 1, 64 * S - 1, 64 * S, 64 * S + 1):
            cs.append(Case("size-S%d-n%d" % (S, n), x[:n], 2, S))
    cs.append(Case("size-S0-n0", x[:0], 2, 0))
    cs.append(Case("size-S0-dense", noise(700, 3), 3, 0))      # ten bits per symbol: the writer picks 32
    cs.append(Case("size-S0-sparse", skew(700, 4), 2, 0))
    xa = skew(4097, 5)
    for a in ARITIES:
        cs.append(Case("arity-%d" % a, xa, a, 64))
    for a in NS_ONLY_ARITIES:
        cs.append(Case("arity-%d" % a, xa, a, 64))            # DCH1 refuses it: DC_E_ARG
    # caller lengths
    x255 = skew(3000, 6, bytes([1, 2, 3, 4, 5, 6, 7, 254]))
    cs.append(Case("M255", x255, 2, 64, orc.huffman_lengths(orc.histogram(x255), 2)[:256], 255))
    x100 = skew(3000, 7, bytes([100, 33, 34, 35, 36, 37, 38, 99]))
    cs.append(Case("M100", x100, 2, 64, orc.huffman_lengths(orc.histogram(x100), 2)[:101], 100))
    cs.append(Case("letters", chain_input(32, 3000, 8), 2, 64, chain_lengths(32)))
    cs.append(Case("len33", chain_input(33, 3000, 9), 2, 64, chain_lengths(33)))
    cs.append(Case("len36", chain_input(36, 3000, 10), 2, 64, chain_lengths(36)))
    L = chain_lengths(20)
    L[257] = 36                                               # no byte's code: only the X block meets it
    cs.append(Case("len36-sym257", chain_input(20, 3000, 11), 2, 64, L))
    xm = skew(3000, 12)
    Lm = orc.huffman_lengths(orc.histogram(xm), 2).copy()
    xm = xm.copy()
    xm[1500] = ord("z")                                       # a byte the lengths miss
    cs.append(Case("nocode", xm, 2, 64, Lm))
    for n in RAW_SIZES:
        cs.append(Case("raw-%d" % n, noise(n, n), 2, 64))
    for n in Z_EDGES:
        cs.append(Case("zedge-%d" % n, fix4(n, n), 2, 64, fix4_lengths()))
    for n in IDX_EDGES:
        cs.append(Case("idxedge-%d" % n, fix4(n, n), 2, 16, fix4_lengths()))
    return cs


def case(name):
    return next(c for c in catalogue() if c.name == name)


# ---- reader-only inputs --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reader_inputs():
    """[(name, container, the bytes it decodes to)]: netstring containers that no encoder writes"""
    xa, xb = skew(5000, 20), skew(4099, 21, b"netsring")
    ta, tb = code_of(xa, 2), code_of(xb, 4)
    sa, sb = segment(xa, ta, 64), segment(xb, tb, 16)
    A, Bb = xa.tobytes(), xb.tobytes()
    out = []
    for k in (1, 15, 16, 17):      # the segment's output starts k bytes in: 16 is aligned, the others are not
        r = noise(k, 30 + k).tobytes()
        out.append(("raw%d-then-huffman" % k, raw_bytes(r) + sa, r + A))
    r = noise(33, 40).tobytes()
    out.append(("huffman-raw-huffman", sa + raw_bytes(r) + sb, A + r + Bb))
    other = block(b"\n#other metadata")
    out.append(("other-between-Z", segment(xa, ta, 64, zsplit=700, between=other), A))
    out.append(("other-between-dcidx", segment(xb, tb, 16, isplit=100, between=other), Bb))
    out.append(("hex-lengths", segment(xa, ta, 64, fmt="0x%x") + raw_bytes(r, fmt="0X%X"), A + r))
    out.append(("octal-lengths", segment(xa, ta, 64, fmt="0%o"), A))
    out.append(("plus-lengths", segment(xa, ta, 64, fmt="+%d"), A))
    xf = fix4(4000, 23)             # random bits: both characters occur
    out.append(("plus-slash-text", segment(xf, code_of(xf, 2, fix4_lengths()), 64, alt=True), xf.tobytes()))
    for k in (1, 2, NS_MAX - 2):
        xs = xa[:600] if k < 3 else fix4(Z_EDGES[0] + 30, 22)
        ts = ta if k < 3 else code_of(xs, 2, fix4_lengths())
        out.append(("Z-split-%d" % k, segment(xs, ts, 64, zsplit=k), xs.tobytes()))
    out.append(("whitespace", b" \n\t" + sa.replace(b",", b",\r\n \t", 3) + b"\n\n" + raw_bytes(r) + b" \n", A + r))
    out.append(("nul-after-last", sa + b"\0" + b"garbage that is no block", A))
    out.append(("no-M", segment(xa, ta, 64, with_M=False), A))
    return out


# ---- malformed containers --------------------------------------------------------------------------
def _u64(v):
    return np.array([v % 2 ** 64], np.uint64)


@functools.lru_cache(maxsize=None)
def malformed_base():
    """the valid 8 KiB S = 16 container every malformed DCH1 entry starts from: (x, pieces)"""
    x = skew(8192, 50)
    t = code_of(x, 2)
    payload, bits, bases, lens = packed(x, t, 16)
    return x, {"n_ary": 2, "n": x.size, "bits": bits, "S": 16, "len_bytes": np.maximum(t["el"][:256], 0),
               "bases": bases, "lens": lens, "payload": payload}


@functools.lru_cache(maxsize=None)
def malformed_dch1():
    """[(name, container, valid, wild)]: one field wrong at a time. valid: the rules' verdict (two
    entries pass them: every chunk still starts inside the payload). wild: the entry holds an index or a size
    far from the true one; it goes to the host checks alone, never to a device."""
    x, P = malformed_base()
    out = []

    def add(name, wild=False, valid=False, cut=None, **kw):
        q = dict(P)
        q.update(kw)
        blob = dch1_pieces(**q)
        out.append((name, blob[:cut] if cut else blob, valid, wild))

    add("valid", valid=True)
    add("version-2", version=2)
    for a in (0, 1, 17):
        add("n_ary-%d" % a, n_ary=a, w=1)
    add("wrong-w", w=2)
    add("flags-1", flags=1)
    for S in (0, 8, 48, 2048):
        add("S-%d" % S, S=S)
    add("n-plus-1", n=P["n"] + 1)
    # one symbol fewer leaves every count and every sum as it was: the rules pass it (the last chunk
    # is longer than its 15 symbols need, and decodes to the input less its last symbol)
    add("n-minus-1", valid=True, n=P["n"] - 1)
    for name, b in (("2^64-1", 2 ** 64 - 1), ("2^64-7", 2 ** 64 - 7), ("2^63", 2 ** 63)):
        add("bits-" + name, wild=True, bits=b)
    add("bits-plus-1", bits=P["bits"] + 1)     # (the payload's last byte has room for it or not: the sum decides)
    ng, nc, nb = P["bases"].size, P["lens"].size, P["payload"].size
    for name, end in (("header", HEADER), ("bases", HEADER + 8 * ng), ("lens", HEADER + 8 * ng + 2 * nc),
                      ("payload", HEADER + 8 * ng + 2 * nc + nb)):
        add("cut-1-at-" + name, cut=end - 1)

    def bases(g, v):
        b = P["bases"].copy()
        b[g] = _u64(v)[0]
        return b

    add("bases0-1", bases=bases(0, 1))
    add("bases1-plus-1", bases=bases(1, int(P["bases"][1]) + 1))
    add("bases1-minus-1", bases=bases(1, int(P["bases"][1]) - 1))
    add("bases1-2^63", wild=True, bases=bases(1, 2 ** 63))
    add("bases1-bits-plus-1", wild=True, bases=bases(1, P["bits"] + 1))
    add("bases-descending", wild=True, bases=P["bases"][::-1].copy())

    def lens(c, v):
        b = P["lens"].copy()
        b[c] = v
        return b

    add("len-plus-1", lens=lens(70, int(P["lens"][70]) + 1))
    add("len-minus-1", lens=lens(70, int(P["lens"][70]) - 1))
    add("len-0xFFFF", wild=True, lens=lens(70, 0xFFFF))
    sw = P["lens"].copy()
    a, b = next((a, b) for a in range(64, 100) for b in range(a + 1, 100) if sw[a] != sw[b])
    sw[a], sw[b] = sw[b], sw[a]
    # two lengths of one group swapped: every sum holds, so the rules cannot see it; the chunks
    # between them start at wrong bits inside the payload, and decode to wrong bytes or to an
    # invalid code (DC_E_STREAM): safe, and a checksum's to catch
    add("lens-swapped-in-group", valid=True, lens=sw)
    return out


@functools.lru_cache(maxsize=None)
def malformed_netstring():
    """[(name, container, valid)]: one thing wrong at a time in what the host can see"""
    x = skew(5000, 60)
    t = code_of(x, 2)
    good = segment(x, t, 64)
    pay = [b"\n" + typ.encode("latin-1") + p for typ, p, _ in ns_blocks(good)]     # #dc1, X, #dcidx, Z
    assert len(pay) == 4 and b"".join(block(p) for p in pay) == good

    def swap(i, payload):
        q = list(pay)
        q[i] = payload
        return b"".join(block(p) for p in q)

    meta = pay[0].decode()
    big = swap(0, meta.replace("syms=%d " % x.size, "syms=%d " % 2 ** 63).encode())
    return [("valid", good, True),
            ("missing-comma", good[:-1] + b";", False),
            ("length-1", b"1:\n," + good, False),
            ("length-32769", block(b"\n\n" + b"a" * 32767) + good, False),
            ("no-colon-in-31", b"0" * 31 + b"5:\n\nabc," + good, False),
            ("block-ends-at-m", good + b"5:\n\nabc", False),
            ("dc1-without-bits", swap(0, meta.replace(" bits=", " bots=").encode()), False),
            ("Z-before-dc1", block(b"\nZAAAA") + good, False),
            ("X-wrong-count", swap(1, pay[1][:-1]), False),
            ("X-bad-character", swap(1, pay[1][:20] + b"a" + pay[1][21:]), False),
            ("X-M-1024", swap(1, b"\nX1024:" + b"1" * 1025), False),
            ("zchars-plus-1", swap(3, pay[3] + b"A"), False),
            ("zchars-minus-1", swap(3, pay[3][:-1]), False),
            ("ichars-plus-1", swap(2, pay[2] + b"A"), False),
            ("ichars-minus-1", swap(2, pay[2][:-1]), False),
            ("syms-sum-wraps", big + big, False)]      # 2^63 + 2^63: also what dc_huff_netstring_info sums


def shifted_index(delta, what):
    """The valid netstring segment of malformed_netstring with one base (what = "base": group 1 of
    3) or one length (what = "len": a chunk of group 0) of its index moved by delta (|delta| <= 64
    bits): (container, x). Every chunk still starts inside the payload, whether or not a reader
    checks the index."""
    assert abs(delta) <= 64
    x = skew(3 * 64 * 64 - 100, 61)
    t = code_of(x, 2)
    payload, bits, bases, lens = packed(x, t, 64)
    bases, lens = bases.copy(), lens.copy()
    assert bases.size == 3
    if what == "base":
        bases[1] = _u64(int(bases[1]) + delta)[0]
    else:
        lens[5] = int(lens[5]) + delta
    ib = np.frombuffer(bases.tobytes() + lens.tobytes(), np.uint8)
    good = segment(x, t, 64)
    old = block(b"\n#" + ns_blocks(good)[2][1])
    assert good.count(old) == 1 and int(lens[5]) >= 0
    return good.replace(old, block(b"\n#dcidx:" + orc.base64url(ib, ib.size * 8))), x
