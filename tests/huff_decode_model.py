"""A plain model of the S = 64 Huffman decoder (k_huff_decode8), its exact redo
(k_huff_decode8_fix) and the decoder tables of dc_dtable (dec_tables_build), with the case
catalogue of test_huff_decode_model_cpu.py and test_gpu_decode_edges.py (TEST INFRASTRUCTURE:
numpy and the oracle only, no import of the product).

Everything starts from a length array (in digits) and n_ary: the oracle gives the canonical
codes (orc.canonical, orc.bitcodes), the stream (orc.huff_pack) and the sync index
(orc.sync_compact). The model then states, by definition and not by the kernels' construction:

  model_tables    every entry of lut, dlut, dlut2, dlut2_k, dlut14, dlut15 (include/dc_gpu.h): for
                  every window value, the code that is its prefix, found by search
  model_decode    each chunk decoded from its own index position by binary search among the
                  left-justified codes, on the payload followed by zero bits: what a valid stream
                  decodes to (x) and what a damaged chunk decodes to
  model_geometry  which tuples the fast decoder takes and which chunk slots the redo rewrites
                  (the sum is Codec.decode_redo_count())
  model_schedule  the tuple scheduler's static deal and its eight dequeue slices
  model_restage   how often the redo re-stages a lane's row for one chunk

The numbers are those of dc_core.hip; a change there changes them here with it.
"""
import functools

import numpy as np

from oracle import oracle as orc

S = 64                  # symbols per chunk
GROUP = 64              # chunks per group (DC_SYNC_GROUP)
GSYM = S * GROUP        # symbols per group
NC = 2                  # groups per tuple
NW = 11                 # waves per workgroup of k_huff_decode8
GRID_MAX = 256
STAGE_WORDS = 1088      # D8_STAGE_WORDS
LUT_BITS = 12           # DC_LUT_BITS
LUT2_CAP = 7168         # DC_LUT2_CAP
K_MAX = 8
ROW = 20                # D8F_ROW: words of a lane's staged span in the redo
LIST = 1024             # D8F_LIST: listed chunks per part
FIX_GRID, FIX_NT = 256, 1024   # the redo's workgroups, and the groups of one window
SPAN_LAST_FAST = (STAGE_WORDS - 4 - 3) * 32 + 31   # lead + span: nw = (lead + span) / 32 + 3, nw + 4 <= 1088
DC_E_STREAM = -7


def words_needed(bit_base, bits):
    """dc_huff_words_needed"""
    return (((bit_base & 31) + bits + 31) >> 5) + 24


def _rev(v, b):
    r = 0
    for _ in range(b):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


# ---- codes -----------------------------------------------------------------------------------
def codes(lengths, n_ary):
    """(code, nbits, max_bits, lengths[259], enc_len, enc_val): the packed codes of the 256 byte
    values from their lengths in digits, and the canonical table they come from"""
    L = np.zeros(259, np.int32)
    L[: len(lengths)] = lengths
    el, ev = orc.canonical(L, n_ary)
    code, nb, mx = orc.bitcodes(el[:256], ev[:256], n_ary)
    return code, nb.astype(np.int64), int(mx), L, el, ev


# ---- tables ----------------------------------------------------------------------------------
def _search(B, code, nbits, lo, hi):
    """For every LSB-first window of B bits (bit 0 = the stream's next bit): the symbol and length
    of the code of lo..hi bits that is its prefix; length 0 where there is none."""
    W = np.arange(1 << B, dtype=np.uint32)
    sym = np.zeros(1 << B, np.uint32)
    bits = np.zeros(1 << B, np.uint32)
    for s in range(256):
        b = int(nbits[s])
        if lo <= b <= hi and b <= B:
            hit = (W & np.uint32((1 << b) - 1)) == np.uint32(_rev(int(code[s]), b))
            sym[hit] = s
            bits[hit] = b
    return sym, bits


def model_tables(code, nbits, n_ary):
    """The decoder tables as include/dc_gpu.h defines them (n_ary is not needed beyond the codes:
    a window that holds a digit >= n_ary is the prefix of no code)."""
    nbits = np.asarray(nbits, np.int64)
    max_bits = int(nbits.max())
    sym12, bits12 = _search(LUT_BITS, code, nbits, 1, LUT_BITS)
    # lut: the MSB-first window e is the LSB-first window of its reversed bits
    rev12 = np.array([_rev(e, LUT_BITS) for e in range(1 << LUT_BITS)], np.uint32)
    s0, n0 = sym12[rev12], bits12[rev12]
    e = np.arange(1 << LUT_BITS, dtype=np.uint32)
    nxt = (e << n0) & np.uint32((1 << LUT_BITS) - 1)    # the window after the first code, zero bits behind
    s1, n1 = s0[nxt], n0[nxt]
    two = (n0 > 0) & (n1 > 0) & (n1 <= LUT_BITS - n0)
    lut = np.where(n0 > 0, s0 | (n0 << 8) | (n0 << 24) | (np.uint32(1) << 29), 0).astype(np.uint32)
    lut = np.where(two, s0 | ((n0 + n1) << 8) | (s1 << 16) | (n0 << 24) | (np.uint32(2) << 29), lut).astype(np.uint32)
    # dlut: escapes (windows of no code of <= 12 bits) numbered in index order
    esc = bits12 == 0
    ids = (np.cumsum(esc) - esc).astype(np.uint32)
    E = int(esc.sum())
    dlut = np.where(esc, (ids & 255) << 8, bits12 | (sym12 << 8)).astype(np.uint16)
    K = min(max(max_bits - LUT_BITS, 1), K_MAX)
    l2ok = 1 <= E <= 256 and (E << K) <= LUT2_CAP and max_bits <= 32
    dlut2 = np.zeros(LUT2_CAP, np.uint16)
    if l2ok:
        # entry [id << K | t]: the 12 + K bit window (prefix of escape id, then t)
        pre = np.nonzero(esc)[0].astype(np.uint32)
        W = (pre[:, None] | (np.arange(1 << K, dtype=np.uint32)[None, :] << LUT_BITS)).reshape(-1)
        v = np.zeros(W.size, np.uint32)
        for s in range(256):
            b = int(nbits[s])
            if LUT_BITS < b <= LUT_BITS + K:
                hit = (W & np.uint32((1 << b) - 1)) == np.uint32(_rev(int(code[s]), b))
                v[hit] = b | (s << 8)
        dlut2[: W.size] = v

    def wide(B, zero_escape):
        sym, bits = _search(B, code, nbits, 1, B)
        second = l2ok and K >= B - LUT_BITS      # codes of 13..B bits: only through the second level
        have = (bits > 0) & ((bits <= LUT_BITS) | second)
        i = np.arange(1 << B, dtype=np.uint32) & np.uint32((1 << LUT_BITS) - 1)
        none = np.zeros(1 << B, np.uint32) if zero_escape else (ids[i] & 255) << 8
        return np.where(have, bits | (sym << 8), none).astype(np.uint16)

    return {"lut": lut, "dlut": dlut, "dlut2": dlut2, "dlut2_k": K if l2ok else 0, "dlut14": wide(14, False),
            "dlut15": wide(15, True), "E": E, "K": K, "l2ok": l2ok, "max_bits": max_bits,
            "code": np.asarray(code, np.uint32), "nbits": nbits, "n_ary": n_ary}


def in_dlut15(tables):
    """per byte value: its code has a dlut15 entry (the fast decoder decodes it)"""
    nb = tables["nbits"]
    return (nb > 0) & ((nb <= LUT_BITS) | ((nb <= 15) & bool(tables["l2ok"] and tables["K"] >= 3)))


# ---- per-chunk decode ------------------------------------------------------------------------
def model_decode(payload, bit_base, idx, n, tables):
    """Chunk c decodes min(64, n - 64 c) symbols from bit idx[c] (absolute; payload byte 0 holds
    bit bit_base & ~7) of the payload followed by zero bits. An invalid code ends the chunk and
    marks it. Returns out (n bytes, 0 where nothing was decoded), bad (per chunk), good (symbols
    decoded per chunk), sbits (chunks x 64: each decoded symbol's code length) and end (the bit
    after each chunk's last decoded symbol)."""
    code, nb = tables["code"].astype(np.uint64), tables["nbits"]
    have = np.nonzero(nb > 0)[0]
    lj = code[have] << (32 - nb[have]).astype(np.uint64)     # left-justified in 32 bits
    order = np.argsort(lj)
    lj, syms = lj[order], have[order]
    nch = (n + S - 1) // S
    buf = np.concatenate([np.ascontiguousarray(payload, np.uint8), np.zeros(S * 4 + 16, np.uint8)]).astype(np.uint64)
    pos = np.asarray(idx, np.uint64).astype(np.int64)[:nch] - (bit_base & ~7)
    cnt = np.minimum(S, n - S * np.arange(nch, dtype=np.int64))
    out = np.zeros((nch, S), np.uint8)
    sbits = np.zeros((nch, S), np.uint8)
    bad = np.zeros(nch, bool)
    good = np.zeros(nch, np.int64)
    for k in range(S):
        live = (cnt > k) & ~bad
        if not live.any():
            break
        c = np.nonzero(live)[0]
        p = pos[c]
        b = p >> 3
        v = np.zeros(c.size, np.uint64)
        for q in range(5):
            v = (v << np.uint64(8)) | buf[b + q]
        top = (v >> (8 - (p & 7)).astype(np.uint64)) & np.uint64(0xFFFFFFFF)
        j = np.searchsorted(lj, top, side="right") - 1
        jj = np.maximum(j, 0)
        s = syms[jj]
        ok = (j >= 0) & ((top >> (32 - nb[s]).astype(np.uint64)) == code[s])
        g = c[ok]
        out[g, k] = s[ok]
        sbits[g, k] = nb[s[ok]]
        pos[g] += nb[s[ok]]
        good[g] += 1
        bad[c[~ok]] = True
    return {"out": out.reshape(-1)[:n].copy(), "bad": bad, "good": good, "sbits": sbits,
            "end": pos + (bit_base & ~7)}


def chunks_past_dlut15(dec, tables, n):
    """per chunk: it holds an invalid code or a symbol without a dlut15 entry"""
    nch = dec["bad"].size
    out = np.zeros(nch * S, np.uint8)
    out[:n] = dec["out"]
    ok = in_dlut15(tables)[out.reshape(nch, S)] | (dec["sbits"] == 0)
    return dec["bad"] | ~ok.all(axis=1)


# ---- geometry --------------------------------------------------------------------------------
def model_geometry(idx, bits, bit_base, n, words, long_chunk):
    """Per tuple: fast (both groups whole inside n, and for each nw + 4 <= 1088 and wo + nw + 4 <=
    words). Per chunk slot (groups x 64): redone. long_chunk: per chunk, chunks_past_dlut15."""
    idx = [int(v) for v in idx]
    nch = (n + S - 1) // S
    ngroups = (nch + GROUP - 1) // GROUP
    ntuples = (ngroups + NC - 1) // NC
    end = bit_base + bits
    wb = 32 * (bit_base >> 5)
    lead, span, nw, wo, gok = [], [], [], [], []
    for g in range(ngroups):
        rel = idx[g * GROUP] - wb
        e = idx[(g + 1) * GROUP] if (g + 1) * GROUP < nch else end
        lead.append(rel & 127)
        wo.append((rel >> 5) & ~3)
        span.append(e - idx[g * GROUP])
        nw.append((lead[g] + span[g]) // 32 + 3)
        gok.append(nw[g] + 4 <= STAGE_WORDS and wo[g] + nw[g] + 4 <= words)
    fast = [(t * NC + NC) * GSYM <= n and all(gok[t * NC: t * NC + NC]) for t in range(ntuples)]
    redo = np.zeros((ngroups, GROUP), bool)
    lc = np.zeros(ngroups * GROUP, bool)
    lc[:nch] = long_chunk
    for g in range(ngroups):
        redo[g] = lc[g * GROUP: (g + 1) * GROUP] if fast[g // NC] else True
    return {"fast": np.array(fast), "redo": redo, "count": int(redo.sum()), "lead": lead, "span": span, "nw": nw,
            "wo": wo, "ngroups": ngroups, "ntuples": ntuples,
            "pos": np.array([v - wb for v in idx[:nch]], np.int64)}


def model_restage(pos, sbits, words):
    """The redo of one chunk that starts at bit pos (from the stream's first word) and holds codes
    of sbits bits: (restage() calls, row_base clamped)."""
    lim = (words - ROW) & ~3 if words > ROW else 0
    a0 = min((pos >> 5) & ~3, lim)
    cb0 = pos - (a0 << 5)
    wa, sh, calls = cb0 >> 5, cb0 & 31, 0
    sb = [int(b) for b in sbits if b]
    for q in range(0, len(sb), 4):
        if wa >= ROW - 6:
            wa -= wa & ~3
            calls += 1
        for b in sb[q: q + 4]:
            sh += b
            if sh >= 32:
                sh -= 32
                wa += 1
    return calls, a0 != (pos >> 5) & ~3


def redo_parts(redo):
    """Most parts (of LIST chunks) that one redo workgroup's first window takes"""
    ngroups = redo.shape[0]
    per = redo.sum(axis=1)
    worst = 0
    for b in range(FIX_GRID):
        g0, g1 = ngroups * b // FIX_GRID, ngroups * (b + 1) // FIX_GRID
        worst = max(worst, -(-int(per[g0: min(g1, g0 + FIX_NT)].sum()) // LIST))
    return worst


# ---- scheduler -------------------------------------------------------------------------------
def model_schedule(ntuples, static_pct):
    """Ks static tuples per wave (Ts in all), then 8 slices of Dh tuples: [lo, hi) each."""
    grid = min((ntuples + NW - 1) // NW, GRID_MAX)
    stride = grid * NW
    Ks = ntuples * static_pct // 100 // stride
    Ts = Ks * stride
    Dh = (ntuples - Ts + 7) // 8
    slices = []
    for h in range(8):
        lo = Ts + h * Dh
        hi = min(lo + Dh, ntuples)
        slices.append((min(lo, hi), hi))
    return {"grid": grid, "waves": stride, "Ks": Ks, "Ts": Ts, "Dh": Dh, "slices": slices,
            "empty": sum(1 for lo, hi in slices if lo == hi),
            # a workgroup's waves all start on slice blockIdx & 7: with fewer tuples there than
            # waves that dequeue, some wave finds it empty and steals
            "steals": any(hi - lo < NW for h, (lo, hi) in enumerate(slices) if h < grid) and Ts < ntuples}


# ---- tables of the catalogue -----------------------------------------------------------------
def _chain(m):
    """lengths 1, 2, .., m, m on bytes 1..m + 1: a complete binary code of max_bits m"""
    L = np.zeros(256, np.int32)
    L[1: m + 2] = list(range(1, m + 1)) + [m]
    return L


def _pair(e29):
    """K = 8 with E = 28 (4 x 12, 55 x 13) or E = 29 (3 x 12, 57 x 13): Kraft sum 1"""
    mid = [12] * 3 + [13] * 57 if e29 else [12] * 4 + [13] * 55
    ls = list(range(1, 8)) + mid + list(range(14, 20)) + [20, 20]
    L = np.zeros(256, np.int32)
    L[10: 10 + len(ls)] = ls
    return L


def _from_freq(n_ary, f):
    return np.asarray(orc.huffman_lengths(f, n_ary))[:256].astype(np.int32)


def _levels(n_ary, levels):
    """n_ary - 1 symbols per level with counts n_ary^level: lengths reach `levels` digits"""
    f = np.zeros(259, np.uint64)
    f[1: 1 + levels * (n_ary - 1)] = np.repeat(np.uint64(n_ary) ** np.arange(levels, dtype=np.uint64), n_ary - 1)
    return _from_freq(n_ary, f)


def _t89():
    L = np.full(256, 8, np.int32)
    L[:2] = 7
    L[252:] = 9
    return L


def _zipf(n_ary, k):
    f = np.zeros(259, np.uint64)
    f[32: 32 + k] = (1_000_000 // (np.arange(k) + 1) ** 2 + 1).astype(np.uint64)
    return _from_freq(n_ary, f)


TABLES = {
    "b12": (2, lambda: _chain(12)), "b13": (2, lambda: _chain(13)), "b14": (2, lambda: _chain(14)),
    "b15": (2, lambda: _chain(15)), "b16": (2, lambda: _chain(16)), "b20": (2, lambda: _chain(20)),
    "b23": (2, lambda: _chain(23)), "b32": (2, lambda: _chain(32)),
    "e28": (2, lambda: _pair(False)), "e29": (2, lambda: _pair(True)),
    "n3": (3, lambda: _zipf(3, 40)), "n5": (5, lambda: _zipf(5, 60)), "n16": (16, lambda: _levels(16, 4)),
    "t89": (2, _t89),
}


@functools.lru_cache(maxsize=None)
def table(name):
    """{"n_ary", "lengths" (259 int32 for dc_huff_table_lengths), the codes, model_tables}"""
    n_ary, make = TABLES[name]
    code, nb, mx, L, el, ev = codes(make(), n_ary)
    t = dict(model_tables(code, nb, n_ary))
    t.update(name=name, lengths=L, enc_len=el, enc_val=ev)
    assert t["max_bits"] == mx
    return t


# ---- streams ---------------------------------------------------------------------------------
class Case:
    """One decode: input x under a table at bit_base, in a buffer of `words` words."""

    def __init__(self, name, family, tab, x, bit_base=0, spare=0, dev=False):
        self.name, self.family, self.tab, self.bit_base, self.dev = name, family, tab, bit_base, dev
        self.x = np.ascontiguousarray(x, np.uint8)
        self.n = self.x.size
        t = table(tab)
        self.payload, self.bits, idx = orc.huff_pack(self.x, t["code"], t["nbits"].astype(np.uint8),
                                                     bit_base=bit_base, sync_syms=S)
        self.idx = np.asarray(idx, np.uint64)
        self.base, self.lens = orc.sync_compact(self.idx, bit_base, self.bits)
        self.words = words_needed(bit_base, self.bits) + spare

    def word_array(self, payload=None):
        """the stream as the decoder takes it: word 0 = stream word bit_base / 32"""
        p = self.payload if payload is None else payload
        w = np.zeros(self.words, np.uint32)
        off = (self.bit_base >> 3) - ((self.bit_base >> 5) << 2)
        w.view(np.uint8)[off: off + len(p)] = p
        return w

    @functools.lru_cache(maxsize=None)
    def model(self):
        """(model_decode, model_geometry) of the undamaged stream"""
        t = table(self.tab)
        dec = model_decode(self.payload, self.bit_base, self.idx, self.n, t)
        geo = model_geometry(self.idx, self.bits, self.bit_base, self.n, self.words,
                             chunks_past_dlut15(dec, t, self.n))
        return dec, geo

    def __repr__(self):
        return self.name


def draw(tab, n, seed, cap=14, only=None):
    """n symbols of the table, a code of b bits drawn with weight 2^-min(b, cap); every coded byte
    once at the front when n allows"""
    nb = table(tab)["nbits"]
    have = np.nonzero(nb > 0)[0] if only is None else np.asarray(only)
    p = 2.0 ** -np.minimum(nb[have], cap)
    rng = np.random.default_rng(seed)
    x = have[rng.choice(have.size, size=n, p=p / p.sum())].astype(np.uint8)
    if n >= 2 * have.size and only is None:
        x[: have.size] = have
    return x


def _by_len(tab):
    nb = table(tab)["nbits"]
    return {int(b): int(np.nonzero(nb == b)[0][0]) for b in np.unique(nb) if b}


SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096, 3 * 4096 + 1, 16 * 4096 - 1, 16 * 4096 + 1)
BIT_BASES = (0, 1, 31, 32, 77, 127, 128, (1 << 33) + 5)
SCHED_TUPLES = (1, 2, 7, 8, 9, 11, 12, 22, 23, 33, 45)
SCHED_PCT = (0, 60, 100)


def _span_case(lead, total, second):
    """Four groups under the 8/9-bit table; the group at position `second` of tuple 1 has
    lead + span = total at that lead. A group of 8-bit codes spans 32768 bits (0 mod 128), so the
    lead of every later group is (bit_base & 31) + the 9-bit codes before it."""
    rng = np.random.default_rng(lead * 7 + total + second)
    x = rng.integers(2, 252, 4 * GSYM).astype(np.uint8)      # 8-bit codes
    bit_base = min(lead, 31)
    extra = lead - bit_base
    tg = 2 + second

    def nines(g, k):
        at = g * GSYM + rng.choice(GSYM, size=k, replace=False)
        x[at] = rng.integers(252, 256, k)

    nines(0, extra)
    nines(tg, total - lead - 8 * GSYM)
    return Case("span-lead%d-%d-%s" % (lead, total, "second" if second else "first"), "span", "t89", x, bit_base)


def _one_flag(lanes, group=0, name=None):
    """One fast tuple under b20, codes of <= 3 bits except one 17-bit code in each chunk of `lanes`"""
    by = _by_len("b20")
    x = draw("b20", 2 * GSYM, 5 + len(lanes) + lanes[0], only=[by[1], by[2], by[3]])
    for ln in lanes:
        x[group * GSYM + ln * S + (ln * 5) % S] = by[17]
    return Case(name or "one-flag-lane%d" % lanes[0], "redo", "b20", x)


def _rows32():
    """b32: chunks of 1- and 2-bit codes (under 20 words), half 32-bit codes, and all 32-bit
    codes (64 words), in turn; a partial last chunk of 32-bit codes"""
    by = _by_len("b32")
    n = 2 * GSYM + 5 * S + 17
    x = draw("b32", n, 32, only=[by[1], by[2]])
    for c in range((n + S - 1) // S):
        lo, hi = c * S, min(c * S + S, n)
        if c % 3 == 1:
            x[lo:hi:2] = by[32]
        elif c % 3 == 2:
            x[lo:hi] = by[32]
    x[-17:] = by[32]
    return Case("rows32", "redo", "b32", x)


def _batch_positions():
    """b16 (13..15 bits through dlut15, 16 bits to the redo): chunk c holds, by c % 6: nothing
    long; a 15-bit, a 16-bit code at symbol (c / 6) % 64; four 15-bit codes as batch (c / 6) % 16;
    a 13-bit, a 14-bit code at symbol (c / 6) % 64"""
    by = _by_len("b16")
    n = 4 * GSYM
    x = draw("b16", n, 16, only=[by[1], by[2], by[3], by[4]])
    for c in range(n // S):
        kind, at = c % 6, (c // 6) % S
        if kind == 3:
            b = (c // 6) % 16
            x[c * S + 4 * b: c * S + 4 * b + 4] = by[15]
        elif kind:
            x[c * S + at] = by[{1: 15, 2: 16, 4: 13, 5: 14}[kind]]
    return Case("batch-positions", "codes", "b16", x)


def _residue_cases():
    """words_needed at each residue mod 4: prefixes of one input"""
    x = draw("b16", 3 * GSYM + 300, 77)
    cum = np.cumsum(table("b16")["nbits"][x])
    out, seen = [], set()
    for n in range(3 * GSYM + 37, x.size):
        r = words_needed(0, int(cum[n - 1])) % 4
        if r not in seen:
            seen.add(r)
            out.append(Case("words-mod4-%d" % r, "bufend", "b16", x[:n]))
    return out


@functools.lru_cache(maxsize=None)
def catalogue():
    cs = []
    for name in TABLES:
        cs.append(Case("table-" + name, "tables", name, draw(name, 2 * NC * GSYM + GSYM + 5, len(name) + TABLES[name][0])))
    for lead in (0, 127):
        for total in (SPAN_LAST_FAST, SPAN_LAST_FAST + 1):
            for second in (0, 1):
                cs.append(_span_case(lead, total, second))
    for n in SIZES:
        cs.append(Case("size-%d" % n, "sizes", "b16", draw("b16", n, n)))
    cs += _residue_cases()
    xb = draw("b16", NC * GSYM + GSYM + 1, 99)
    for bb in BIT_BASES:
        cs.append(Case("bit-base-%d" % bb, "bufend", "b16", xb, bb))
    cs.append(Case("bit-base-77-dev", "bufend", "b16", xb, 77, dev=True))
    cs.append(Case("spare-64", "bufend", "b16", xb[: NC * GSYM], 0, spare=64))
    cs.append(Case("spare-0", "bufend", "b16", xb[: NC * GSYM], 0))
    cs.append(_rows32())
    for ln in (0, 31, 63):
        cs.append(_one_flag([ln]))
    cs.append(_one_flag(list(range(GROUP)), group=1, name="all-64-flagged"))
    cs.append(Case("flags-in-last-group", "redo", "b20", draw("b20", NC * GSYM + GSYM + 3 * S + 5, 20)))
    cs.append(_batch_positions())
    return cs


FAMILIES = ("tables", "span", "sizes", "bufend", "redo", "codes")


def family(name):
    return [c for c in catalogue() if c.family == name]


@functools.lru_cache(maxsize=None)
def sched_case(ntuples):
    """ntuples tuples of short b16 codes; an odd count ends in a partial group"""
    n = ntuples * NC * GSYM - (37 if ntuples % 2 else 0)
    return Case("sched-%d" % ntuples, "sched", "b16", draw("b16", n, 1000 + ntuples))


# ---- damage ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def damage_case(tab, seed):
    """A valid stream of three whole tuples and a partial one; bits flipped inside a dozen chunks,
    none among the last four and none in the last ten lanes of its group (so a damaged chunk that
    decodes past its end stays inside its group's span). Returns (case, damaged payload, chunks,
    model_decode of the damaged payload)."""
    only = None
    if tab == "n3":     # short codes: a damaged chunk keeps some good symbols
        nb = table(tab)["nbits"]
        only = np.nonzero((nb > 0) & (nb <= 6))[0]
    case = Case("damage-%s" % tab, "damage", tab, draw(tab, 3 * NC * GSYM + GSYM + 100, seed, only=only))
    rng = np.random.default_rng(seed)
    nch = (case.n + S - 1) // S
    ok = [c for c in range(nch - 4) if c % GROUP < GROUP - 10]
    chunks = np.sort(rng.choice(ok, size=12, replace=False))
    p = case.payload.copy()
    for c in chunks:
        lo, ln = int(case.idx[c]) - (case.bit_base & ~7), int(case.lens[c])
        for _ in range(2):
            b = lo + ln // 4 + int(rng.integers(0, ln // 2))    # past the chunk's first symbols
            p[b >> 3] ^= 0x80 >> (b & 7)
    return case, p, chunks, model_decode(p, case.bit_base, case.idx, case.n, table(tab))


# ---- C5 --------------------------------------------------------------------------------------
def c5_text(n, seed, first=None):
    """Text-like bytes (< 0x80): lower-case words (pairs for the front-end) with three tiers of
    rarer bytes, so that a 16-ary code of the front-end stream has codes of 4 digits"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxz", np.uint8)
    pl = 1.0 / (np.arange(26) + 1.0)
    body = letters[rng.choice(26, size=n, p=pl / pl.sum())].copy()
    body[rng.random(n) < 0.18] = 0x20
    tiers = ((list(range(1, 8)) + list(range(14, 23)), 1), (list(range(33, 48)), 40), (list(range(65, 80)), 1500))
    for vals, count in tiers:
        for v in vals:
            k = max(1, count * n // 300_000)
            body[rng.choice(n, size=k, replace=False)] = v
    if first is not None:
        body[0] = first
    return body


@functools.lru_cache(maxsize=None)
def c5_case(first=None):
    """(x, the Case of its front-end stream M under the 16-ary code of M's histogram): M ends in a
    partial chunk that holds a pair. first: x[0] (>= 0x80: M[1] is a byte >= 0x80 that is no pair)."""
    text = c5_text(150_000, 5, first).tobytes()
    for extra in range(8):
        x = text + b" ab cd ef gh ij kl mn op qr st uv wx yz ab cd ef" + b"e" * extra
        m = np.frombuffer(orc.small_compress(x), np.uint8)
        if m.size % S and (m[-(m.size % S):] >= 0x80).any():
            break
    name = "c5-%s" % first
    L = np.asarray(orc.huffman_lengths(orc.histogram(m), 16))[:256].astype(np.int32)
    TABLES[name] = (16, lambda: L)
    return np.frombuffer(x, np.uint8), Case(name, "c5", name, m)


# ---- the redo's list in parts ------------------------------------------------------------------
REDO_LIST_GROUPS = 17 * 256


def redo_list_input():
    """9- and 10-bit codes of b32 in turn: every group spans 38912 bits, past the stage, so no
    tuple is fast and every chunk is listed. (x, idx, bits) without packing: a chunk is 608 bits."""
    by = _by_len("b32")
    x = np.tile(np.array([by[9], by[10]], np.uint8), REDO_LIST_GROUPS * GSYM // 2)
    nch = x.size // S
    return x, np.arange(nch, dtype=np.uint64) * np.uint64(608), nch * 608
