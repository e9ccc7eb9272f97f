"""A plain model of the fused C5 encode (k_hist_blocks<1, true>, the lcnt / msym half of k_block_local
and k_block_final_wide, k_fe_pack<false> / k_fe_pack<true>) and of its two shard calls, with the case
catalogue of test_fe_pack_model_cpu.py and test_gpu_fe_edges.py (TEST INFRASTRUCTURE: numpy and the
oracle only, no import of the product).

The expected stream and sync index are the oracle's (orc.huff_pack, orc.sync_compact) over the symbols
of the input. One thing is modelled, not inherited from small_frontend_model.fe_body: fe_body emits a
pair's symbol at the space, the kernels count and code it at the letter (letter | 0x80) and the space
carries no symbol. The stream M is the same; which 32 KiB block, and which shard, owns the symbol of a
pair that straddles a cut is not. The model follows the kernels (dc_gpu.h, d_shard).

  symbols      per input position the symbol byte or -1, for a shard with the bytes either side
  block_hists  256 counts per 32 KiB input block (dc_huff_block_hist), the type byte in block 0
  expected     payload words, bits, local index, block bit offsets, and for a shard its part of the
               stream's global index
  geometry     which of the kernels' cuts an input reaches, block by block
  stitch       the shards' words, u16 parts and group bases merged into one stream, no process group

The numbers are those of dc_core.hip; a change there changes them here with it.
"""
import functools

import numpy as np

from oracle import oracle as orc
from tests import huff_decode_model as D
from tests import small_frontend_model as F
from tests.pack_block_model import (BLOCK, GROUP, PIECE, PIECES, PLAN_WG_BLOCKS,  # noqa: F401 (the tests')
                                    seq_layout, store_cuts, words_touched)
from tests.pack_block_model import PACK_BLK_WORDS as STAGE

SPACE = 0x20
SYNCS = (16, 32, 64, 256, 1024)
DC_E_ARG, DC_E_STATE, DC_E_FALLBACK = -1, -5, -8
LEN_POISON = 0x5A5A

words_needed = D.words_needed


def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def _lower(a):
    return (a >= ord("a")) & (a <= ord("z"))


# ---- the symbols -----------------------------------------------------------------------------
def symbols(x, lb=-1, rb=-1):
    """int16 per position of x: its symbol byte, or -1 (a pair's space). lb / rb: the input bytes
    either side of the shard; lb = -1: the stream starts here (position 0 neither closes nor starts
    a pair, position 1 closes none); rb = -1: nothing follows."""
    x = _u8(x).astype(np.int16)
    n = x.size
    prev = np.concatenate([[max(lb, 0) if lb >= 0 else 0], x[:-1]]).astype(np.int16)
    nxt = np.concatenate([x[1:], [rb if rb >= 0 else 0]]).astype(np.int16)
    pos = np.arange(n)
    sec = (prev == SPACE) & _lower(x)
    start = (x == SPACE) & _lower(nxt)
    if lb < 0:
        sec &= pos >= 2
        start &= pos >= 1
    y = x.copy()
    y[sec] |= 0x80
    y[start] = -1
    return y


def stream_symbols(x, lb=-1, rb=-1):
    """the shard's symbols of M in order (the type byte 8 first when it starts the stream)"""
    y = symbols(x, lb, rb)
    m = y[y >= 0].astype(np.uint8)
    return np.concatenate([np.array([8], np.uint8), m]) if lb < 0 else m


def block_hists(x, lb=-1, rb=-1):
    """(nblocks, 256) uint16: the symbols counted in the 32 KiB input block of their position"""
    y = symbols(x, lb, rb)
    nblocks = (y.size + BLOCK - 1) // BLOCK
    bh = np.zeros((nblocks, 256), np.int64)
    for b in range(nblocks):
        yb = y[b * BLOCK: (b + 1) * BLOCK]
        bh[b] = np.bincount(yb[yb >= 0], minlength=256)
    if lb < 0:
        bh[0, 8] += 1
    assert bh.max() <= 0xFFFF
    return bh


def own_lengths(x, n_ary, lb=-1, rb=-1, extra=None):
    """the 259 code lengths (digits) of the n-ary Huffman code of the M histogram of x (+ extra)"""
    h = block_hists(x, lb, rb).sum(axis=0).astype(np.uint64)
    if extra is not None:
        h = h + np.asarray(extra, np.uint64)
    return orc.huffman_lengths(h, n_ary), h


# ---- the expected stream ---------------------------------------------------------------------
def expected(x, ctx, lengths, n_ary, S):
    """ctx = (global bit, global first symbol, byte before or -1, byte after or -1); (0, 0, -1, -1)
    with the bit_base in ctx[0] is the whole-stream call."""
    bit, sym, lb, rb = ctx
    m = stream_symbols(x, lb, rb)
    code, nb, mx, L, el, ev = D.codes(lengths, n_ary)
    assert (nb[m] > 0).all(), "a symbol without a code"
    payload, bits, idx = orc.huff_pack(m, code, nb.astype(np.uint8), bit_base=bit, sync_syms=S)
    idx = np.asarray(idx, np.uint64)
    base, lens = orc.sync_compact(idx, bit, bits)
    bh = block_hists(x, lb, rb)
    off = np.zeros(bh.shape[0] + 1, np.uint64)
    off[1:] = np.cumsum((bh * nb[None, :256]).sum(axis=1))
    msym = np.zeros(bh.shape[0] + 1, np.int64)
    msym[1:] = np.cumsum(bh.sum(axis=1))
    assert int(off[-1]) == bits and int(msym[-1]) == m.size
    w = np.zeros(4 * words_touched(bit, bits), np.uint8)
    o = (bit >> 3) - ((bit >> 5) << 2)
    w[o: o + len(payload)] = payload
    # the shard's part of the global index
    sb = nb[m].astype(np.int64)
    rel = np.cumsum(sb) - sb
    gi = sym + np.arange(m.size, dtype=np.int64)
    c0 = sym // S
    c0e = c0 & ~1
    glens = np.zeros(int(gi[-1] // S - c0e + 1), np.int64)
    np.add.at(glens, gi // S - c0e, sb)
    g0 = -(-sym // (GROUP * S))
    at = np.nonzero(gi % (GROUP * S) == 0)[0]
    gbase = np.array([bit + int(rel[i]) for i in at], np.uint64)
    assert at.size == 0 or int(gi[at[0]]) // (GROUP * S) == g0
    return {"m": m, "bits": bits, "bit": bit, "sym": sym, "S": S, "word_bytes": w, "idx": idx, "base": base, "lens": lens,
            "off": off, "msym": msym, "bh": bh, "c0": c0, "c0e": c0e, "glens": glens, "g0": g0, "gbase": gbase,
            "nbits": nb, "enc_len": el, "enc_val": ev, "n_ary": n_ary, "hist": bh.sum(axis=0)}


def zeroed_dwords(msym, S, sym=None):
    """The dwords of the u16 length array that k_block_final_wide zeroes: of the local array (sym =
    None), the one holding the last chunk begun before each block boundary b = 1..nblocks; of the
    global array, the same for b = 0..nblocks over global chunks, from chunk c0 & ~1."""
    out = set()
    if sym is None:
        for m in msym[1:]:
            out.add(((int(m) - 1) // S) >> 1)
        return sorted(out)
    c0e = (sym // S) & ~1
    for m in msym:
        g = sym + int(m)
        if g > 0 and (g - 1) // S >= c0e:
            out.add(((g - 1) // S - c0e) >> 1)
    return sorted(out)


def expected_len_array(e, entries, glob):
    """the u16 array of `entries` entries after the pack: the chunk lengths, zero in the other half of
    a dword the plan zeroed, the poison elsewhere"""
    a = np.full(entries, LEN_POISON, np.int64)
    for d in zeroed_dwords(e["msym"], e["S"], e["sym"] if glob else None):
        a[2 * d: 2 * d + 2] = 0
    if glob:
        k = e["c0"] - e["c0e"]
        a[k: e["glens"].size] = e["glens"][k:]
        if k:
            assert a[0] == 0       # an odd first chunk: entry 0, the chunk before it, is in a zeroed dword
    else:
        a[: e["lens"].size] = e["lens"]
    return a.astype(np.uint16)


def sync_entries(n, S, glob):
    """the documented u16 entries of d_sync_len (n + 1 symbols) and d_gsync_len (n + 1 + 2 S)"""
    chunks = -(-(n + 1 + (2 * S if glob else 0)) // S)
    return -(-chunks // 2) * 2 + 2, -(-chunks // GROUP)


# ---- stitch ----------------------------------------------------------------------------------
def stitch(parts):
    """parts: per shard {"bit", "bits", "sym", "m" or "nsym", "S", "word_bytes", "glens" (from entry 0 =
    chunk c0 & ~1), "gbase"}, in stream order. Returns (word bytes from word bit0 / 32, bits, lens,
    base) of the whole stream."""
    S = parts[0]["S"]
    bit0 = parts[0]["bit"]
    end = parts[-1]["bit"] + parts[-1]["bits"]
    w = np.zeros(4 * words_touched(bit0, end - bit0), np.uint8)
    nsym = lambda p: p["nsym"] if "nsym" in p else p["m"].size
    mtot = parts[-1]["sym"] + nsym(parts[-1])
    lens = np.zeros(-(-mtot // S), np.int64)
    base = np.zeros(-(-lens.size // GROUP), np.uint64)
    seen = np.zeros(base.size, bool)
    for p in parts:
        o = 4 * ((p["bit"] >> 5) - (bit0 >> 5))
        w[o: o + p["word_bytes"].size] |= p["word_bytes"]
        c0 = p["sym"] // S
        c0e = c0 & ~1
        c1 = (p["sym"] + nsym(p) - 1) // S
        lens[c0: c1 + 1] += np.asarray(p["glens"], np.int64)[c0 - c0e: c1 - c0e + 1]
        g0 = -(-p["sym"] // (GROUP * S))
        g1 = -(-(p["sym"] + nsym(p)) // (GROUP * S))
        assert not seen[g0: g1].any()
        base[g0: g1] = np.asarray(p["gbase"], np.uint64)[: g1 - g0]
        seen[g0: g1] = True
    assert seen.all() and lens.max() <= 0xFFFF
    return w, end - bit0, lens.astype(np.uint16), base


# ---- geometry --------------------------------------------------------------------------------
def geometry(x, ctx, lengths, n_ary, S, k=1, shift=0, grid=0, guard=True):
    """k_fe_pack's cuts for the input x: k = 1 the whole-stream call, 2 the shard call; shift: words
    from a 16-byte boundary to d_words; grid: DC_OPT_PACK_GRID; guard: thread 0's OR of the block's
    first word only when the block has a word. The flag is a hand-kept restatement of pack_store_block's
    `if (t == 0 && nw_blk > 0)` in dc_pack_block.inc (False: that line without `nw_blk > 0`): nothing ties
    it to the source, and an OR of zero shows in no byte, so what the tests assert from it is a
    property of the model and of the catalogue, not a check of the kernel."""
    bit, sym, lb, rb = ctx
    x = _u8(x)
    n = x.size
    first = lb < 0
    y = symbols(x, lb, rb)
    code, nb, mx, L, el, ev = D.codes(lengths, n_ary)
    has = y >= 0
    sbits = np.where(has, nb[np.where(has, y, 0)], 0).astype(np.int64)
    nblocks = (n + BLOCK - 1) // BLOCK
    bh = block_hists(x, lb, rb)
    off = np.concatenate([[0], np.cumsum((bh * nb[None, :256]).sum(axis=1))]).astype(np.int64)
    msym = np.concatenate([[0], np.cumsum(bh.sum(axis=1))]).astype(np.int64)
    total, mtot = int(off[-1]), int(msym[-1])
    free = np.nonzero(nb[:256] == 0)[0]
    z = int(free[0]) if free.size else None
    slog = S.bit_length() - 1
    cbw = (BLOCK >> slog) + 2
    lim = STAGE - k * cbw - 4
    vec_out = shift % 4 == 0
    qmode = 2 * total > 11 * mtot
    word_base = bit >> 5
    nwords = words_touched(bit, total)
    g = min(nblocks, grid if grid else (nblocks + 1) // 2)
    blocks = []
    for b in range(nblocks):
        lo, hi = b * BLOCK, min(b * BLOCK + BLOCK, n)
        m0, m1 = int(msym[b]), int(msym[b + 1])
        s_bits = int(off[b + 1] - off[b])
        blk_abs = bit + int(off[b])
        fw = blk_abs >> 5
        nw_blk = ((blk_abs & 31) + s_bits + 31) >> 5
        sh = (fw - word_base) & 3 if vec_out else 0
        r = {"b": b, "full": hi - lo == BLOCK, "n": hi - lo, "m0": m0, "m1": m1, "s_bits": s_bits, "abs31": blk_abs & 31,
             "nw_blk": nw_blk, "sh": sh, "fits": nw_blk + sh <= lim, "lim": lim, "wg": b % g,
             "before": list(range(b % g, b, g)), "zero_symbols": m1 == m0, "one_word": nw_blk == 1,
             "ends_on_word": (blk_abs + s_bits) & 31 == 0, "starts_on_word": blk_abs & 31 == 0}
        # the words the block touches, from the stream's first word
        w0 = fw - word_base
        touched = set(range(w0, w0 + nw_blk))
        if not guard or nw_blk > 0:
            touched.add(w0)                       # thread 0's OR of the block's first word
        r["words"] = (w0, w0 + nw_blk)
        r["past_end"] = sorted(w for w in touched if w >= nwords)
        r.update(store_cuts(sh, nw_blk, r["ends_on_word"], vec_out))
        # the chunks: local (M = 0) and, for a shard, global
        for pre, M in (("", 0),) + ((("g", sym),) if k == 2 else ()):
            cf = (M + m0 + S - 1) >> slog
            ct = (M + m1 - 1) >> slog
            nc = max(ct - cf + 1, 0)
            hd = ((M + m0 - 1) >> slog) >> 1 if M + m0 > 0 else None
            td = ct >> 1
            cs = list(range(cf, cf + nc))
            atom = [c for c in cs if (c >> 1) in (hd, td)]
            r.update({pre + "cf": cf, pre + "ct": ct, pre + "nc": nc, pre + "hd": hd, pre + "td": td,
                      pre + "atomic": atom, pre + "plain": [c for c in cs if c not in atom],
                      pre + "tail_add": cf - 1 if (M + m0) & (S - 1) else None})
        # the pieces: lane t of piece p codes input bytes [p * 4096 + 16 t, + 16)
        hb = np.zeros(BLOCK, bool)
        hb[: hi - lo] = has[lo:hi]
        bb = np.zeros(BLOCK, np.int64)
        bb[: hi - lo] = sbits[lo:hi]
        Ck = hb.reshape(PIECES * 256, 16).sum(axis=1)
        mi = m0 + (1 if b == 0 and first else 0) + np.cumsum(Ck) - Ck
        starts = []
        for pre, M in (("", 0),) + ((("g", sym),) if k == 2 else ()):
            j0 = (-(mi + M)) & (S - 1)
            at = np.nonzero(j0 < Ck)[0]
            r[pre + "starts"] = [(int(i) // 256, int(i) % 256, int(j0[i]), int(Ck[i])) for i in at]
            r[pre + "two_in_a_piece"] = bool(((j0 + S) < Ck).any())
        r["Ck"] = Ck
        Th = bb.reshape(PIECES * 256, 2, 8).sum(axis=-1)
        Q = bb.reshape(PIECES * 256, 4, 4).sum(axis=-1)
        r.update(qmode=qmode, halves_over_64=int((Th > 64).sum()), quarters_over_64=int((Q > 64).sum()),
                 half_gathers=0 if qmode else int((Th <= 64).sum()))
        blocks.append(r)
    reasons = {"literal": k == 1 and mtot >= n, "no_z": z is None, "overflow": any(not r["fits"] for r in blocks)}
    return {"z": z, "reasons": reasons, "fallback": any(reasons.values()), "total": total, "mtot": mtot, "nwords": nwords,
            "lim": lim, "cbw": cbw, "qmode": qmode, "grid": g, "vec_out": vec_out, "blocks": blocks, "msym": msym,
            "off": off}


# ---- cases -----------------------------------------------------------------------------------
class Case:
    """One fused encode. ctx None: the whole-stream call at bit_base (its table is the input's own);
    ctx = (bit, sym, lb, rb): the shard call, under the table dc_huff_table_plan makes of `hist`
    (default: the shard's own histogram of M)."""

    def __init__(self, name, family, x, ctx=None, bit_base=0, S=64, n_ary=2, hist=None, shift=0, grid=0,
                 exact_cap=False, sites=None, fill=0xFF):
        self.name, self.family, self.S, self.n_ary, self.shift, self.grid = name, family, S, n_ary, shift, grid
        self.x = _u8(x)
        self.x.setflags(write=False)
        self.n = self.x.size
        self.shard = ctx is not None
        self.ctx = tuple(int(v) for v in ctx) if self.shard else (bit_base, 0, -1, -1)
        self._hist, self.exact_cap, self.sites, self.fill = hist, exact_cap, sites or {}, fill

    @property
    def k(self):
        return 2 if self.shard else 1

    @functools.lru_cache(maxsize=None)
    def table_hist(self):
        """the 256 counts the table is made of"""
        if self._hist is not None:
            return np.asarray(self._hist, np.uint64)
        return block_hists(self.x, self.ctx[2], self.ctx[3]).sum(axis=0).astype(np.uint64)

    @functools.lru_cache(maxsize=None)
    def lengths(self):
        return orc.huffman_lengths(self.table_hist(), self.n_ary)

    @functools.lru_cache(maxsize=None)
    def geometry(self, guard=True):
        return geometry(self.x, self.ctx, self.lengths(), self.n_ary, self.S, self.k, self.shift, self.grid, guard)

    @functools.lru_cache(maxsize=None)
    def expected(self):
        return expected(self.x, self.ctx, self.lengths(), self.n_ary, self.S)

    def status(self):
        return DC_E_FALLBACK if self.geometry()["fallback"] else 0

    def __repr__(self):
        return self.name


X, Q = ord("X"), ord("q")


def plain(n, pairs=()):
    """n bytes 'x' with a pair ' q' starting at each position of `pairs`"""
    x = np.full(n, ord("x"), np.uint8)
    for p in pairs:
        x[p], x[p + 1] = SPACE, Q
    return x


def spread(n, count, lo=8):
    """`count` pair positions spread over [lo, n - 2), at least 2 apart"""
    assert 2 * count <= n - 2 - lo
    return [lo + int(i) * ((n - 2 - lo) // count) for i in range(count)] if count else []


# ---- ends ------------------------------------------------------------------------------------
END_SIZES = (2, 3, 15, 16, 17, 4095, 4096, 4097, 32767, 32768, 32769, 2 * BLOCK - 1, 2 * BLOCK + 1)


def _ends_cases():
    cs = []
    for n in END_SIZES:
        x = F.text(n, seed=n)
        if n >= 8:      # two pairs at least: not LITERAL
            x[1:7] = np.frombuffer(b" a b c", np.uint8)
        cs.append(Case("ends-n%d" % n, "ends", x))
    base = F.text(300, seed=7)
    base[8:14] = np.frombuffer(b" a b c", np.uint8)

    def var(name, edit):
        x = base.copy()
        edit(x)
        cs.append(Case("ends-" + name, "ends", x))

    def last_space(x):
        x[-2:] = [X, SPACE]

    def first_space(x):
        x[0:3] = [SPACE, Q, X]

    def pair_1_2(x):
        x[0:4] = [X, SPACE, Q, X]

    def two_spaces(x):
        x[0:4] = [X, SPACE, SPACE, Q]

    def high_first(x):
        x[0:2] = [0xE1, X]

    for name, fn in (("last-space", last_space), ("space-letter-at-0", first_space), ("pair-at-1-2", pair_1_2),
                     ("two-spaces-letter", two_spaces), ("high-first-byte", high_first)):
        var(name, fn)
    return cs


# ---- cuts ------------------------------------------------------------------------------------
# pattern -> (bytes, k): bytes[k] is the first byte at or after the cut
CUT_PATTERNS = {"space|letter": (b" q", 1), "pair-starts-on": (b" q", 0), "pair-ends-before": (b" q", 2),
                "space|other": (b" Q", 1)}
# boundary -> the cut positions: in the full block 0 and in the partial block 1; the block cut between
CUT_SITES = {"dword": (8196, BLOCK + 8196), "lane": (2064, BLOCK + 2064), "wave": (5120, BLOCK + 5120),
             "piece": (12288, BLOCK + 12288), "block": (BLOCK,)}
CUT_N = BLOCK + 4 * PIECE + 100


def _plant(x, e, seq, k):
    s = e - k
    x[s - 1] = X
    x[s: s + len(seq)] = np.frombuffer(seq, np.uint8)
    x[s + len(seq)] = X


def _cuts_cases():
    cs = []
    for i, (name, (seq, k)) in enumerate(CUT_PATTERNS.items()):
        x = F.text(CUT_N, seed=0x60 + i)
        sites = {}
        for bname, es in CUT_SITES.items():
            for e in es:
                _plant(x, e, seq, k)
                sites[(bname, e)] = e
        cs.append(Case("cuts-" + name, "cuts", x, sites=sites))
    # a pair across both boundaries of one 16-byte lane, in a full and in the partial block
    x = F.text(CUT_N, seed=0x70)
    for e in (2064, BLOCK + 2064):
        x[e - 2: e + 18] = X
        x[e - 1], x[e] = SPACE, Q
        x[e + 15], x[e + 16] = SPACE, Q
    cs.append(Case("cuts-both-ends-of-a-lane", "cuts", x, sites={("lane", 2064): 2064, ("lane", BLOCK + 2064): BLOCK + 2064}))
    # every other byte a space before a letter, across a whole block and both its boundaries
    x = F.text(2 * BLOCK + 300, seed=0x71)
    x[BLOCK - 3: 2 * BLOCK + 3: 2] = SPACE
    x[BLOCK - 2: 2 * BLOCK + 4: 2] = Q
    cs.append(Case("cuts-dense-block", "cuts", x, S=16))
    return cs


# ---- sync ------------------------------------------------------------------------------------
def _sync_cases():
    cs = []
    for S in SYNCS:
        cs.append(Case("sync-%d-text" % S, "sync", _pairs_text(2 * BLOCK + 1234, S), S=S))
    # S = 16, pieces of 16 symbols: before the first pair symbol index = position + 1, so every piece's
    # chunk start is its last symbol (j0 = 15); after it index = position and it is the first (j0 = 0)
    cs.append(Case("sync-16-j0-0-and-15", "sync", plain(2 * PIECE, [33, 2000, 6001]), S=16))
    # the spanning chunk of the block boundaries: odd (31), even (62), and a last block inside one chunk
    x = np.concatenate([plain(BLOCK, [1, 9]), plain(BLOCK, spread(BLOCK, 1100)), plain(BLOCK, [5]), plain(50)])
    cs.append(Case("sync-1024-boundary-parities", "sync", x, S=1024))
    x = np.concatenate([plain(BLOCK, [1, 9]), plain(BLOCK, spread(BLOCK, 104)), plain(BLOCK, [5]), plain(700)])
    cs.append(Case("sync-64-boundary-parities", "sync", x, S=64))
    for S in (16, 64):
        for c in (63, 64, 65, 127, 128, 129):       # chunks = ceil((n - 1) / S): two pairs, the type byte
            cs.append(Case("sync-%d-chunks%d" % (S, c), "sync", plain(c * S + 1, [1, 9]), S=S))
        for d in (-1, 1):
            cs.append(Case("sync-%d-n%+d" % (S, d), "sync", plain(64 * S + 1 + d, [1, 9]), S=S))
    return cs


def _pairs_text(n, seed):
    x = F.text(n, seed=seed)
    x[1:7] = np.frombuffer(b" a b c", np.uint8)
    return x


# ---- fit -------------------------------------------------------------------------------------
# the shard call's alphabet of 31 values, 5 bits each under a uniform histogram (the binary code has
# a phantom 32nd leaf; 32 values give one 6-bit code): ' ', 'A'..'N', the letters 'a'..'h' and their
# pair symbols
FIT_ALPHABET = [SPACE] + list(range(ord("A"), ord("O"))) + list(range(ord("a"), ord("i"))) + \
    [0x80 | v for v in range(ord("a"), ord("i"))]
FIT_S = 16
FIT_LIM2 = STAGE - 2 * ((BLOCK >> 4) + 2) - 4       # 5112
FIT_LIM1 = STAGE - ((BLOCK >> 4) + 2) - 4           # 7162


def fit_hist():
    h = np.zeros(256, np.uint64)
    h[FIT_ALPHABET] = 100
    return h


def fit_block(symbols_wanted):
    """a full block of 'A' with ' a' pairs: exactly symbols_wanted symbols"""
    pairs = BLOCK - symbols_wanted
    x = np.full(BLOCK, ord("A"), np.uint8)
    at = np.array(spread(BLOCK, pairs, lo=4))
    x[at], x[at + 1] = SPACE, ord("a")
    return x


def _fit_solve(per, lim, sh, f, over, extra=0, s0_from=BLOCK // 2 + 8):
    """(first bit f0 of the stream, symbols of block 0, symbols of block 1): block 1 starts at bit f of
    a word that is sh words past a 16-byte boundary and takes lim - sh (+ 1: over) words. extra: the
    symbols block 0 holds beside those of its positions (the type byte)."""
    W = lim - sh + (1 if over else 0)
    s1 = (32 * W - f) // per                    # the most symbols whose bits end inside word W
    assert 32 * (W - 1) < f + per * s1 <= 32 * W and s1 <= BLOCK
    for s0 in range(s0_from, BLOCK):
        for f0 in range(32):
            end = f0 + per * (s0 + extra)
            if end % 32 == f and (end // 32) % 4 == sh and ((end + 31) >> 5) <= lim:
                return f0, s0, s1
    raise AssertionError


# the whole-stream call's alphabet of 127 values, 7 bits each when their counts are about equal: 126
# filler values (no space, no lowercase letter; the type byte's 8 among them) and the pair symbol of 'a'
FIT_FILLER = np.array(list(range(0, 32)) + list(range(33, 97)) + list(range(123, 153)), np.uint8)


FIT_COUNT = 520     # of every one of the 127 values in M: the reference's binary code with its phantom
#                     leaf is 7 bits for all only when no two counts differ by more than 1


def fit_whole_stream(s0, s1):
    """two full blocks of s0 and s1 symbols (' a' pairs in a row from position 4, the 126 filler values
    in turn elsewhere), then the pairs and filler bytes that bring every value of M to FIT_COUNT"""
    p0, p1 = BLOCK - s0, BLOCK - s1
    k = FIT_COUNT - p0 - p1
    fill = 2 * (p0 + p1) - 17        # 126 * FIT_COUNT filler symbols in all, the type byte one of them
    assert k >= 0 and fill > 0
    x = np.zeros(2 * BLOCK + 2 * k + fill, np.uint8)
    at = np.concatenate([4 + 2 * np.arange(p0), BLOCK + 4 + 2 * np.arange(p1), 2 * BLOCK + 2 * np.arange(k)])
    pair = np.zeros(x.size, bool)
    pair[at] = pair[at + 1] = True
    seq = np.tile(FIT_FILLER, FIT_COUNT)
    x[~pair] = np.delete(seq, 8)     # (one 8 fewer: the type byte)
    x[at], x[at + 1] = SPACE, ord("a")
    return x


def _fit_cases():
    cs = []
    for sh in range(4):
        for f in (0, 1, 31):
            for over in (False, True):
                f0, s0, s1 = _fit_solve(5, FIT_LIM2, sh, f, over)
                x = np.concatenate([fit_block(s0), fit_block(s1)])
                cs.append(Case("fit-shard-sh%d-bit%d-%s" % (sh, f, "over" if over else "fits"), "fit", x,
                               ctx=(f0, 3 * FIT_S, ord("A"), ord("A")), S=FIT_S, hist=fit_hist()))
                # the whole-stream call
                f0, s0, s1 = _fit_solve(7, FIT_LIM1, sh, f, over, extra=1, s0_from=BLOCK - 440)
                x = fit_whole_stream(s0, s1)
                cs.append(Case("fit-whole-sh%d-bit%d-%s" % (sh, f, "over" if over else "fits"), "fit", x, bit_base=f0,
                               S=FIT_S))
    return cs


# ---- shard -----------------------------------------------------------------------------------
SH_N = BLOCK + PIECE + 50


def _shard_x(seed=0x90):
    x = F.text(SH_N, seed=seed)
    x[0:2] = [X, X]
    x[-2:] = [X, X]
    return x


def _shard_cases():
    cs = []
    x = _shard_x()
    S = 64
    for name, sym in (("sym-0modS", 5 * S), ("sym-1modS", 5 * S + 1), ("sym-Sm1modS", 6 * S - 1), ("chunk-even", 6 * S + 7),
                      ("chunk-odd", 7 * S + 7), ("sym-0mod64S", 64 * S), ("sym-64S-1", 64 * S - 1), ("sym-64S+1", 64 * S + 1)):
        cs.append(Case("shard-" + name, "shard", x, ctx=(77, sym, X, X), S=S))
    for S2 in (16, 1024):
        xs = x if S2 > 16 else x[:20000]      # (S = 16: a full block of this text is past the shard call's lim)
        cs.append(Case("shard-S%d-sym-Sm1" % S2, "shard", xs, ctx=(77, 3 * S2 - 1, X, X), S=S2))
        cs.append(Case("shard-S%d-sym-odd-chunk-0modS" % S2, "shard", xs, ctx=(77, 3 * S2, X, X), S=S2))
    for bit in (0, 1, 31, (1 << 33) + 5):
        cs.append(Case("shard-bit-%d" % bit, "shard", x, ctx=(bit, 100, X, X), S=S, exact_cap=True))
    # (byte before) x (first byte); (last byte) x (byte after)
    for lname, lb in (("start", -1), ("space", SPACE), ("letter", Q), ("other", X)):
        for fname, fb in (("letter", Q), ("space", SPACE), ("other", X)):
            y = x.copy()
            y[0:3] = [fb, Q, X] if fb == SPACE else [fb, X, X]
            cs.append(Case("shard-before-%s-first-%s" % (lname, fname), "shard", y, ctx=(33, 0 if lb < 0 else 200, lb, X), S=S))
    for tname, tb in (("space", SPACE), ("other", X)):
        for aname, rb in (("none", -1), ("letter", Q), ("other", X)):
            y = x.copy()
            y[-1] = tb
            # ('X' the most frequent: the all-zero code is its, and a space coded by mistake shows)
            h = block_hists(y, X, rb).sum(axis=0)
            h[X] += 10 * y.size
            cs.append(Case("shard-last-%s-after-%s" % (tname, aname), "shard", y, ctx=(33, 200, X, rb), S=S, hist=h))
    # two bytes: the first a pair's letter, the second a pair's space; and two plain ones
    hist2 = np.zeros(256, np.uint64)
    hist2[[X, Q, SPACE, 0x80 | Q]] = (5, 3, 2, 1)
    cs.append(Case("shard-2-bytes-pair-both-sides", "shard", [Q, SPACE], ctx=(95, 127, SPACE, Q), S=S, hist=hist2, exact_cap=True))
    cs.append(Case("shard-2-bytes-plain", "shard", [X, SPACE], ctx=(64, 128, X, X), S=S, hist=hist2, exact_cap=True))
    # inside one global chunk: ncg = 0 in every block
    cs.append(Case("shard-inside-one-chunk", "shard", plain(40, [3]), ctx=(7, 5 * 1024 + 100, X, X), S=1024, exact_cap=True))
    # the last block one byte, a space before the letter after the shard: it holds no symbol
    y = np.concatenate([_pairs_text(BLOCK, 0x91), [SPACE]])
    y[-2] = X
    bits0 = int(expected(y, (0, 64, X, Q), own_lengths(y, 2, X, Q)[0], 2, S)["bits"])
    cs.append(Case("shard-zero-symbol-block-on-a-word", "shard", y, ctx=((-bits0) % 32 + 64, 64, X, Q), S=S, exact_cap=True))
    cs.append(Case("shard-zero-symbol-block-off-a-word", "shard", y, ctx=((-bits0) % 32 + 64 + 5, 64, X, Q), S=S, exact_cap=True))
    return cs


# ---- stores ----------------------------------------------------------------------------------
def _stores_cases():
    cs = []
    x = _pairs_text(BLOCK + 600, 0xA0)
    for shift in range(4):
        for fill in (0xFF, 0):
            cs.append(Case("stores-shift%d-into-%02x" % (shift, fill), "stores", x, shift=shift, fill=fill, exact_cap=True))
    for d in range(4):      # tails of 0..3 words: the stream grows by a few symbols
        cs.append(Case("stores-tail-%d" % d, "stores", _pairs_text(BLOCK + 600 + 5 * d, 0xA0), exact_cap=True))
    cs.append(Case("stores-one-word", "stores", [X, SPACE], ctx=(3, 9, X, X), hist=np.bincount([X, SPACE, 1], minlength=256),
                   exact_cap=True))
    return cs


# ---- seq -------------------------------------------------------------------------------------
SEQ_GRIDS = (1, 2, 0)


# Planted orders, in the shard call under the 5-bit table (a block of s symbols is 5 s bits exactly).
# A step: (the block's first bit mod 128 = 32 sh + (blk_abs & 31), or None; the first bit mod 128 of
# the block after it, or None). One workgroup runs the steps in a row.
SEQS = {
    "sh-3-0-2": [(96, None), (0, None), (64, None)],
    # ends 7 bits into a word (t == 64 ORs and clears the stage's last word), then ends on a word
    # (the next block stores that stage word plainly)
    "mid-word-then-on-a-word": [(0, 39), (None, 64)],
}
SEQ_S = 64      # (lim = 9216 - 2 * 514 - 4 words: every block of 5-bit codes fits)


def seq_runs(name, grid):
    """[(block positions, the steps they hold)] of a planted seq case, blocks in all"""
    return seq_layout(SEQS[name], grid)


def _seq_planted(name, grid):
    runs, nblocks = seq_runs(name, grid)
    start = {}
    for ps, steps in runs:
        for b, (at, nxt) in zip(ps, steps):
            for k, v in ((b, at), (b + 1, nxt)):
                if v is not None:
                    assert start.get(k, v) == v, (name, grid, k)
                    start[k] = v
    f0 = 5                              # the shard's first bit, in its word 0
    cum, parts = f0, []
    for b in range(nblocks):
        sy = 30000
        if b + 1 in start:              # 5 sy = start[b + 1] - cum (mod 128); 77 = 1 / 5
            sy += ((start[b + 1] - cum - 5 * sy) * 77) % 128
        parts.append(fit_block(sy))
        cum += 5 * sy
    return Case("seq-%s-grid%d" % (name, grid), "seq", np.concatenate(parts), ctx=(f0, 3 * SEQ_S, ord("A"), ord("A")),
                S=SEQ_S, hist=fit_hist(), grid=grid)


def _seq_cases():
    cs = [_seq_planted(name, g) for name in SEQS for g in SEQ_GRIDS]
    # long -> short blocks (few pairs, then dense pairs), five blocks; every grid
    x = np.concatenate([_pairs_text(BLOCK, 0xB0), plain(BLOCK, spread(BLOCK, 12000)), _pairs_text(BLOCK, 0xB1),
                        plain(BLOCK, spread(BLOCK, 16000)), _pairs_text(777, 0xB2)])
    for g in SEQ_GRIDS:
        cs.append(Case("seq-long-short-grid%d" % g, "seq", x, grid=g))
    # fits -> overflows -> fits under the shard call's lim, and the zero-symbol block last
    f0, s0, s1 = _fit_solve(5, FIT_LIM2, 0, 0, True)
    x = np.concatenate([fit_block(s0), fit_block(s1), fit_block(20000), [SPACE]])
    for g in SEQ_GRIDS:
        cs.append(Case("seq-fits-over-fits-zero-grid%d" % g, "seq", x, ctx=(f0, 3 * FIT_S, ord("A"), ord("a")), S=FIT_S,
                       hist=fit_hist(), grid=g))
    return cs


# ---- plan ------------------------------------------------------------------------------------
def _plan_cases():
    cs = []
    pat = _pairs_text(BLOCK + 17, 0xC0)
    for nb in (65, 129):
        cs.append(Case("plan-%d-blocks" % nb, "plan", np.resize(pat, nb * BLOCK - 5), S=1024))
    x = np.full(BLOCK + 100, X, np.uint8)          # 32768 of one symbol in a block: bit 15 of the u16 count
    x[BLOCK:] = _pairs_text(100, 0xC1)
    cs.append(Case("plan-32768-of-one", "plan", x))
    return cs


# ---- fallback --------------------------------------------------------------------------------
def _fallback_cases():
    cs = [Case("fallback-no-pair", "fallback", np.full(5000, X, np.uint8)),
          Case("fallback-one-pair", "fallback", plain(5000, [77]))]
    x = np.concatenate([np.arange(256, dtype=np.uint8), _pairs_text(3000, 0xD0)])
    cs.append(Case("fallback-every-value-coded", "fallback", x))
    return cs


FAMILIES = ("ends", "cuts", "sync", "fit", "shard", "stores", "seq", "plan", "fallback")


@functools.lru_cache(maxsize=None)
def catalogue():
    cs = (_ends_cases() + _cuts_cases() + _sync_cases() + _fit_cases() + _shard_cases() + _stores_cases() + _seq_cases() +
          _plan_cases() + _fallback_cases())
    assert len({c.name for c in cs}) == len(cs)
    return cs


def family(name):
    return [c for c in catalogue() if c.family == name]


def case(name):
    (c,) = [c for c in catalogue() if c.name == name]
    return c


# ---- stitched --------------------------------------------------------------------------------
class Stitched:
    """A whole stream cut into shards at `cuts`: the shard cases (their ctx from the whole stream
    under its own table) and the whole-stream case they must stitch to."""

    def __init__(self, name, whole, cuts):
        self.name, self.whole, self.cuts = name, whole, tuple(cuts)
        x, n = whole.x, whole.n
        ks = [0] + list(cuts) + [n]
        assert all(b - a >= 2 for a, b in zip(ks, ks[1:])), (name, ks)
        y = symbols(x)
        nb = D.codes(whole.lengths(), whole.n_ary)[1]
        bits_at = np.concatenate([[0], np.cumsum(np.where(y >= 0, nb[np.where(y >= 0, y, 0)], 0))]).astype(np.int64)
        syms_at = np.concatenate([[0], np.cumsum(y >= 0)]).astype(np.int64)
        t8 = int(nb[8])
        self.parts = []
        for q, (a, b) in enumerate(zip(ks, ks[1:])):
            ctx = (whole.ctx[0] + (int(bits_at[a]) + t8 if a else 0), int(syms_at[a]) + 1 if a else 0,
                   int(x[a - 1]) if a else -1, int(x[b]) if b < n else -1)
            self.parts.append(Case("%s-part%d" % (name, q), "stitched", x[a:b].copy(), ctx=ctx, S=whole.S, n_ary=whole.n_ary,
                                   hist=whole.table_hist(), exact_cap=True))

    def __repr__(self):
        return self.name


def _pair_at(x, lo):
    """the first ' ' + letter at or after lo"""
    y = symbols(x)
    return int(np.nonzero(y[lo:] < 0)[0][0]) + lo


@functools.lru_cache(maxsize=None)
def stitched():
    out = []
    # (at S = 16 a full block of text is past the shard call's lim: the S = 16 streams here are short)
    for name in ("cuts-space|letter", "cuts-pair-starts-on", "sync-64-boundary-parities", "sync-16-j0-0-and-15",
                 "sync-1024-boundary-parities", "ends-n65537", "ends-last-space"):
        w = case(name)
        n = w.n
        p = _pair_at(w.x, n // 3)
        out.append(Stitched("stitched-%s-2-inside-a-pair" % name, w, [p + 1]))
        if n > BLOCK + 8:
            out.append(Stitched("stitched-%s-3-block-1" % name, w, [p, BLOCK - 1]) if p < BLOCK - 3 else
                       Stitched("stitched-%s-3-block-1" % name, w, [BLOCK - 1, p]))
            out.append(Stitched("stitched-%s-4-ends-and-block+1" % name, w, sorted({2, BLOCK + 1, n - 2})))
        else:
            out.append(Stitched("stitched-%s-3-ends" % name, w, [2, n - 2]))
            out.append(Stitched("stitched-%s-4-after-a-letter" % name, w, sorted({2, p + 2, n - 2})))
    return out
