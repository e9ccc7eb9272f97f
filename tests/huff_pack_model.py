"""A plain model of the Huffman pack (k_huff_pack) and its plan (k_plan_total, k_block_local,
k_block_final_wide), with the case catalogue of test_huff_pack_model_cpu.py and
test_gpu_pack_edges.py (TEST INFRASTRUCTURE: numpy and the oracle only, no import of the product).

The expected stream and sync index are the oracle's (orc.huff_pack, orc.sync_compact) under codes
made from lengths alone (huff_decode_model.codes). The model adds what the oracle does not state:

  plan_model      per 32 KiB block: its histogram (256 x u16), its bits, the exclusive bit
                  offsets with the total last (dc_huff_block_hist, dc_huff_plan_offsets)
  pack_geometry   which of k_huff_pack's cuts an input reaches, block by block: the path (byte map,
                  fast, slow), sh and nw_blk, quarter mode, every 8-code half's and 4-code
                  quarter's bits, the store phase's words, the slow path's lanes and tiles, and
                  which workgroup runs the block after which others
  boundary_words  the words k_block_final_wide zeroes before the pack looks at its guards

The chain tables b16, b20 and b32 have exactly one byte per code length, so a case composes any
bit count per half, quarter, lane, tile and block exactly; t89 (7, 8 and 9 bits) and f8 (every
byte 8 bits) give the 8/9-bit side. The numbers are those of dc_core.hip; a change there changes
them here with it.
"""
import functools

import numpy as np

from oracle import oracle as orc
from tests import huff_decode_model as D
from tests.pack_block_model import (BLOCK, GROUP, PACK_BLK_WORDS, PIECES, PLAN_WG_BLOCKS,  # noqa: F401 (the tests')
                                    seq_layout, store_cuts, words_touched)
from tests.pack_block_model import PIECE as TILE

SYNCS = (16, 32, 64, 128, 256, 512, 1024)
DC_E_ARG, DC_E_NOCODE, DC_E_STATE, DC_E_CAPACITY = -1, -4, -5, -6

words_needed = D.words_needed


# ---- tables ----------------------------------------------------------------------------------
OWN_TABLES = {"f8": (2, lambda: np.full(256, 8, np.int32))}


@functools.lru_cache(maxsize=None)
def table(name):
    """{"n_ary", "lengths" (259 int32), "code", "nbits", "enc_len", "enc_val", "max_bits", "fixed8"}"""
    if name in OWN_TABLES:
        n_ary, make = OWN_TABLES[name]
        code, nb, mx, L, el, ev = D.codes(make(), n_ary)
        t = {"name": name, "n_ary": n_ary, "lengths": L, "code": np.asarray(code, np.uint32), "nbits": nb,
             "enc_len": el, "enc_val": ev, "max_bits": mx}
    else:
        t = dict(D.table(name))
    have = t["nbits"][t["nbits"] > 0]
    t["fixed8"] = bool(have.size and (have == 8).all())     # dc_dtable.fixed8
    return t


def by_len(tab):
    """code length -> the (first) byte of that length"""
    nb = table(tab)["nbits"]
    return {int(b): int(np.nonzero(nb == b)[0][0]) for b in np.unique(nb) if b}


# ---- plan ------------------------------------------------------------------------------------
def plan_model(x, nbits):
    """(block histograms nblocks x 256 u16, bits per block, exclusive offsets + total: nblocks + 1)"""
    x = np.ascontiguousarray(x, np.uint8)
    nblocks = (x.size + BLOCK - 1) // BLOCK
    bh = np.zeros((nblocks, 256), np.uint16)
    for b in range(nblocks):
        bh[b] = np.bincount(x[b * BLOCK: (b + 1) * BLOCK], minlength=256)
    bits = (bh.astype(np.uint64) * np.asarray(nbits, np.uint64)[None, :256]).sum(axis=1)
    off = np.zeros(nblocks + 1, np.uint64)
    off[1:] = np.cumsum(bits)
    return bh, bits, off


def plan_workgroups(nblocks):
    """(workgroups of k_block_local, blocks the last one holds)"""
    nwg = (nblocks + PLAN_WG_BLOCKS - 1) // PLAN_WG_BLOCKS
    return nwg, nblocks - PLAN_WG_BLOCKS * (nwg - 1)


def boundary_words(off, bit_base, words_cap):
    """The word indices (from stream word bit_base / 32) that k_block_final_wide zeroes: the word
    of every block's first bit, and the stream's last word when it is partial; below words_cap."""
    off = [int(v) for v in off]
    wb = bit_base >> 5
    ws = {((bit_base + o) >> 5) - wb for o in off[:-1]}
    if (bit_base + off[-1]) & 31:
        ws.add(((bit_base + off[-1]) >> 5) - wb)
    return sorted(w for w in ws if w < words_cap)


# ---- geometry --------------------------------------------------------------------------------
def pack_geometry(x, nbits, bit_base=0, out_word_shift=0, S=64, grid=0, detail=True):
    """k_huff_pack's cuts for input x under the code lengths nbits, restated from the kernel.
    out_word_shift: words from a 16-byte boundary to the output pointer (vec_out = shift % 4 == 0);
    grid: DC_OPT_PACK_GRID (0 = a block pair per workgroup). Returns {"qmode", "bytemap", "total",
    "grid", "blocks": [per block ...]}; with detail = False the per-lane arrays are left out."""
    x = np.ascontiguousarray(x, np.uint8)
    nbits = np.asarray(nbits, np.int64)
    n = x.size
    sb = nbits[x]
    nblocks = (n + BLOCK - 1) // BLOCK
    _, bbits, off = plan_model(x, nbits)
    total = int(off[-1])
    vec_out = out_word_shift % 4 == 0
    qmode = 2 * total > 11 * n
    have = nbits[nbits > 0]
    bytemap = bool(have.size and (have == 8).all()) and vec_out and (bit_base & 127) == 0
    g = min(nblocks, grid if grid else (nblocks + 1) // 2)
    word_base = bit_base >> 5
    cm = S >> 4
    blocks = []
    for b in range(nblocks):
        lo, hi = b * BLOCK, min(b * BLOCK + BLOCK, n)
        full = hi - lo == BLOCK
        bits = int(bbits[b])
        blk_abs = bit_base + int(off[b])
        first_word = blk_abs >> 5
        nw_blk = ((blk_abs & 31) + bits + 31) >> 5
        sh = (first_word - word_base) & 3 if vec_out else 0
        path = "fixed8" if bytemap else "fast" if full and nw_blk + sh <= PACK_BLK_WORDS else "slow"
        run = blk_abs + bits
        r = {"b": b, "full": full, "n": hi - lo, "bits": bits, "abs31": blk_abs & 31, "sh": sh, "nw_blk": nw_blk,
             "path": path, "qmode": qmode, "wg": b % g, "before": list(range(b % g, b, g)),
             "ends_on_word": run & 31 == 0, "starts_on_word": blk_abs & 31 == 0,
             "sync": None if path == "fixed8" else "xor" if path == "slow" else
             "one" if cm == 1 else "dpp" if cm == 4 else "shfl"}
        if path == "fast":
            r.update(store_cuts(sh, nw_blk, run & 31 == 0, vec_out))
            if detail:
                s8 = sb[lo:hi].reshape(PIECES, 256, 2, 2, 4)     # piece, lane, half, quarter, code
                Q = s8.sum(axis=-1)
                Th = Q.sum(axis=-1)
                as_half = (Th <= 64) & (not qmode)
                qs = ~as_half[..., None] & np.ones_like(Q, bool)      # quarters that are gathered
                percode = qs & (Q > 64)
                r.update(Th=Th, Q=Q, as_half=as_half, as_quarter=qs & (Q <= 64), percode=percode,
                         percode_max=int(s8[percode].max()) if percode.any() else 0)
        elif path == "slow" and detail:
            tiles, tile_abs = [], blk_abs
            for k in range(PIECES):
                t0 = lo + k * TILE
                if t0 >= hi:
                    break
                cnt = np.clip(hi - (t0 + 16 * np.arange(256)), 0, 16)
                lb = np.zeros(TILE, np.int64)
                lb[: min(TILE, hi - t0)] = sb[t0: min(t0 + TILE, hi)]
                T = lb.reshape(256, 16).sum(axis=1)
                As = tile_abs + np.cumsum(T) - T
                tb = int(T.sum())
                tiles.append({"cnt0": int((cnt == 0).sum()), "cnt_part": int(((cnt > 0) & (cnt < 16)).sum()),
                              "cnt16": int((cnt == 16).sum()), "one_word": int(((T > 0) & ((As & 31) + T < 32)).sum()),
                              "lane_bits_max": int(T.max()), "tile_bits": tb, "end_aligned": (tile_abs + tb) & 31 == 0})
                tile_abs += tb
            r["tiles"] = tiles
        blocks.append(r)
    return {"qmode": qmode, "bytemap": bytemap, "total": total, "grid": g, "vec_out": vec_out, "blocks": blocks}


# ---- cases -----------------------------------------------------------------------------------
class Case:
    """One pack: input x under a table at bit_base, into words `shift` words off a 16-byte boundary,
    with a sync index of S symbols per chunk, under DC_OPT_PACK_GRID = grid."""

    def __init__(self, name, family, tab, x, bit_base=0, shift=0, S=64, grid=0, dev=False):
        self.name, self.family, self.tab, self.bit_base, self.shift = name, family, tab, bit_base, shift
        self.S, self.grid, self.dev = S, grid, dev
        self.x = np.ascontiguousarray(x, np.uint8)
        self.n = self.x.size

    @functools.lru_cache(maxsize=None)
    def stream(self):
        """the oracle's (payload, bits, idx, group bases, chunk lengths)"""
        t = table(self.tab)
        payload, bits, idx = orc.huff_pack(self.x, t["code"], t["nbits"].astype(np.uint8), bit_base=self.bit_base,
                                           sync_syms=self.S)
        idx = np.asarray(idx, np.uint64)
        base, lens = orc.sync_compact(idx, self.bit_base, bits)
        return payload, bits, idx, base, lens

    @property
    def bits(self):
        return self.stream()[1]

    def word_bytes(self):
        """the bytes of the words the stream touches: zero bits before bit_base and after the last code"""
        payload, bits = self.stream()[:2]
        w = np.zeros(4 * words_touched(self.bit_base, bits), np.uint8)
        o = (self.bit_base >> 3) - ((self.bit_base >> 5) << 2)
        w[o: o + len(payload)] = payload
        return w

    @functools.lru_cache(maxsize=None)
    def plan(self):
        return plan_model(self.x, table(self.tab)["nbits"])

    @functools.lru_cache(maxsize=None)
    def geometry(self, detail=True):
        return pack_geometry(self.x, table(self.tab)["nbits"], self.bit_base, self.shift, self.S, self.grid, detail)

    def __repr__(self):
        return self.name


# ---- composing inputs ------------------------------------------------------------------------
def split(total, k, longest):
    """k code lengths of 1..longest that sum to total, the long ones first"""
    assert k <= total <= k * longest, (total, k, longest)
    out = []
    for i in range(k):
        v = min(longest, total - (k - 1 - i))
        out.append(v)
        total -= v
    return out


def _put(x, at, tab, lens):
    by = by_len(tab)
    x[at: at + len(lens)] = [by[v] for v in lens]


def tune(x, tab, free, target):
    """change the bytes at the positions `free` (each to another code length of the chain table)
    until x codes to exactly `target` bits"""
    by = by_len(tab)
    nb = table(tab)["nbits"]
    longest = max(by)
    diff = target - int(nb[x].sum())
    for p in free:
        if diff == 0:
            break
        cur = int(nb[x[p]])
        new = min(max(cur + diff, 1), longest)
        x[p] = by[new]
        diff -= new - cur
    assert diff == 0, diff
    return x


def t89_block(bits, seed, n=BLOCK):
    """n bytes under t89 (7 bits: bytes 0, 1; 9 bits: 252..255; 8 bits: the rest) coding to `bits`"""
    rng = np.random.default_rng(seed)
    x = rng.integers(2, 252, n).astype(np.uint8)
    d = bits - 8 * n
    assert abs(d) <= n, (bits, n)
    at = rng.choice(n, size=abs(d), replace=False)
    x[at] = rng.integers(252, 256, abs(d)) if d > 0 else rng.integers(0, 2, abs(d))
    return x


def chain_draw(tab, n, seed, lo=1, hi=None, geometric=True):
    """n bytes of a chain table with code lengths lo..hi: weight 2^-length, or uniform over lengths"""
    by = by_len(tab)
    ls = np.array([v for v in sorted(by) if v >= lo and (hi is None or v <= hi)])
    p = 2.0 ** -(ls - ls.min()) if geometric else np.ones(ls.size)
    rng = np.random.default_rng(seed)
    pick = ls[rng.choice(ls.size, size=n, p=p / p.sum())]
    return np.array([by[int(v)] for v in ls], np.uint8)[np.searchsorted(ls, pick)]


# ---- fit: both sides of PACK_BLK_WORDS -------------------------------------------------------
def _fit_cases():
    cs = []
    nines = lambda seed: t89_block(9 * BLOCK, seed)
    cs.append(Case("fit-b0-9216-fast", "fit", "t89", nines(1)))
    cs.append(Case("fit-b0-9216-base32-fast", "fit", "t89", nines(2), bit_base=32))
    cs.append(Case("fit-b0-abs1-slow", "fit", "t89", nines(3), bit_base=1))
    for sh in range(4):
        # block 0: 8192 + sh words, so block 1 starts sh words past a 16-byte boundary
        b0 = t89_block(32 * (8192 + sh), 10 + sh)
        fast = t89_block(32 * (PACK_BLK_WORDS - sh), 20 + sh)          # nw_blk + sh = 9216
        cs.append(Case("fit-b1-sh%d-fast" % sh, "fit", "t89", np.concatenate([b0, fast])))
        if sh:
            slow = t89_block(32 * (PACK_BLK_WORDS - sh) + 1, 30 + sh)  # one bit more: 9217
            cs.append(Case("fit-b1-sh%d-slow" % sh, "fit", "t89", np.concatenate([b0, slow])))
    # block 1 starts one bit into a word: 9216 words of bits take 9217
    cs.append(Case("fit-b1-abs1-slow", "fit", "t89", np.concatenate([t89_block(32 * 8192 + 1, 40), nines(41)])))
    cs.append(Case("fit-b1-abs31-slow", "fit", "t89", np.concatenate([t89_block(32 * 8192 + 31, 42), nines(43)])))
    return cs


# ---- halves: 63, 64, 65 bits per half and quarter; the quarter-mode threshold ----------------
HALF_LANES = (0, 63, 64, 255)
HALF_PIECES = (0, 7)
HALF_SPOTS = [(k, t, h) for k in HALF_PIECES for t in HALF_LANES for h in (0, 1)]


def _spot(k, t, h):
    return k * TILE + t * 16 + 8 * h


def _halves_block(tab, fill, spots):
    """a full block of `fill` lengths (cycled) with the 8 code lengths of `spots` planted:
    {(piece, lane, half): [8 lengths]}"""
    by = by_len(tab)
    x = np.resize(np.array([by[v] for v in fill], np.uint8), BLOCK).copy()
    for (k, t, h), lens in spots.items():
        assert len(lens) == 8
        _put(x, _spot(k, t, h), tab, lens)
    return x


def _quarter_plan(tab):
    """the 16 spots under b20 / b32: quarters of 64 and 65 bits in the first and second quarter
    (65 with the table's 17- or 32-bit code), a quarter of four longest codes"""
    m = 32 if tab == "b32" else 17
    q64 = split(64, 4, m if tab == "b32" else 16)
    q65 = [m] + split(65 - m, 3, 31 if tab == "b32" else 16)
    longest = [max(by_len(tab))] * 4
    short = [1, 1, 1, 1]
    kinds = [q64 + short, short + q64, q65 + short, short + q65, longest + short, short + longest, q64 + q65, q65 + q64]
    return {s: kinds[i // 2] for i, s in enumerate(HALF_SPOTS)}      # a kind in both halves of a lane


def _halves_cases():
    cs = []
    for v in (63, 64, 65):
        spots = {s: split(v, 8, 20) for s in HALF_SPOTS}
        cs.append(Case("halves-%d" % v, "halves", "b20", _halves_block("b20", [1], spots)))
    for tab in ("b20", "b32"):
        cs.append(Case("quarters-" + tab, "halves", tab, _halves_block(tab, [1], _quarter_plan(tab))))
    # the same plantings in a block of 5- and 6-bit codes, tuned by symbols of piece 3 to the
    # quarter-mode threshold: 2 * total == 11 * n (half mode) and 11 * n + 2 (quarter mode)
    spots = {s: split((63, 64, 65)[i % 3], 8, 20) for i, s in enumerate(HALF_SPOTS)}
    spots.update({(1, t, h): v for (k, t, h), v in _quarter_plan("b20").items() if k == 0})
    free = list(range(3 * TILE, 3 * TILE + 1024))
    for name, target in (("qmode-off", 11 * BLOCK // 2), ("qmode-on", 11 * BLOCK // 2 + 1)):
        x = tune(_halves_block("b20", [5, 6], spots), "b20", free, target)
        cs.append(Case(name, "halves", "b20", x))
    return cs


# ---- seq: what one workgroup runs in a row ----------------------------------------------------
# a step: (the block's first bit mod 128 = 32 sh + (blk_abs & 31), or None; its bits; its symbols).
# Consecutive steps agree: each ends where the next one wants to start.
SEQS = {
    "long-short": [(0, 32 * 9216, BLOCK), (0, 32 * 7168, BLOCK)],
    "fast-slow-fast": [(0, 32 * 9213, BLOCK), (32, 32 * 9216, BLOCK), (32, 32 * 9215, BLOCK)],
    "sh-3-0-2": [(96, 32 * 9213, BLOCK), (0, 32 * 8002, BLOCK), (64, 32 * 9214, BLOCK)],
    # ends 7 bits into a word; starts there and ends on a word; starts on it
    "on-word": [(64, 32 * 8001 + 7, BLOCK), (103, 32 * 8000 + 25, BLOCK), (0, 32 * 8000, BLOCK)],
    "slow-ragged": [(64, 32 * 9216, BLOCK), (None, 8 * 1234 + 5, 1234)],
}
SEQ_GRIDS = (1, 2, 0)


def _seq_case(name, grid):
    runs, nblocks = seq_layout(SEQS[name], grid)
    want = {}
    for ps, r in runs:
        want.update(dict(zip(ps, r)))
    parts, cum = [], 0
    for b in range(nblocks):
        if b in want:
            at, bits, n = want[b]
            assert at is None or cum % 128 == at, (name, grid, b)
        else:       # a filler: it ends where the next step wants to start
            at = want[b + 1][0] if b + 1 in want else None
            bits, n = 32 * 8000, BLOCK
            if at is not None:
                bits += (at - (cum + bits)) % 128
        parts.append(t89_block(bits, 1000 + 17 * b + len(name) + grid, n))
        cum += bits
    return Case("seq-%s-grid%d" % (name, grid), "seq", "t89", np.concatenate(parts), grid=grid)


def seq_blocks(case):
    """[(block positions of each run)] of a seq case"""
    name = case.name[4: case.name.rindex("-grid")]
    return [ps for ps, _ in seq_layout(SEQS[name], case.grid)[0]]


# ---- stores ----------------------------------------------------------------------------------
STORE_ENDS = (0, 1, 31)


def _stores_cases():
    cs = []
    for shift in range(4):
        for w in (range(8000, 8004) if shift == 0 else (8000 + shift,)):
            for e in STORE_ENDS:
                x = np.concatenate([t89_block(32 * w + e, 7 * w + e + shift), t89_block(8 * 100 + 3, w + e, 100)])
                cs.append(Case("stores-shift%d-w%d-end%d" % (shift, w, e), "stores", "t89", x, shift=shift))
    return cs


# ---- tail ------------------------------------------------------------------------------------
TAIL_SIZES = (1, 15, 16, 17, 4095, 4096, 4097, 32767, BLOCK + 1, 2 * BLOCK - 1)


def _tail_cases():
    cs = [Case("tail-%d" % n, "tail", "b16", D.draw("b16", n, n)) for n in TAIL_SIZES]
    b32, b16 = by_len("b32"), by_len("b16")
    # every lane 512 bits, a tile of 131072 bits, then a lane of 5 codes
    cs.append(Case("tail-b32-full-lanes", "tail", "b32", np.full(TILE + 16 + 5, b32[32], np.uint8)))
    for n in (17, 31, TILE + 1, 2 * TILE + 33):     # 1-bit codes: two lanes per word, a tile of 17 bits
        cs.append(Case("tail-ones-%d" % n, "tail", "b16", np.full(n, b16[1], np.uint8)))
    return cs


# ---- sync ------------------------------------------------------------------------------------
SYNC_COUNTS = (63, 64, 65, 127, 128, 129)


def _sync_cases():
    cs = []
    for S in SYNCS:
        cs.append(Case("sync-%d-fast" % S, "sync", "b16", D.draw("b16", 2 * BLOCK, S), S=S))
        # a full block of 8..16-bit codes (12 bits a symbol: slow), then S + 1 symbols
        cs.append(Case("sync-%d-slow" % S, "sync", "b16",
                       chain_draw("b16", BLOCK + S + 1, S + 1, lo=8, geometric=False), S=S))
        cs.append(Case("sync-%d-ragged" % S, "sync", "b16", D.draw("b16", 5 * S - 1, S + 2), S=S))
    for S in (16, 64, 512):
        for c in SYNC_COUNTS:
            cs.append(Case("sync-%d-chunks%d" % (S, c), "sync", "b16", D.draw("b16", c * S, S + c), S=S))
        for d in (-1, 1):
            cs.append(Case("sync-%d-n%+d" % (S, d), "sync", "b16", D.draw("b16", 64 * S + d, S + 5 + d), S=S))
    cs.append(Case("sync-1024-three-blocks", "sync", "b16", D.draw("b16", 3 * BLOCK, 1024), S=1024))
    # every chunk 32768 bits: the longest length a u16 has to hold
    cs.append(Case("sync-1024-b32", "sync", "b32", np.full(3 * 1024 + 5, by_len("b32")[32], np.uint8), S=1024))
    return cs


# ---- base ------------------------------------------------------------------------------------
BIT_BASES = (0, 1, 31, 32, 77, 127, 128, (1 << 33) + 5)
DEV_BASES = (77, (1 << 33) + 5)


def _base_cases():
    x = D.draw("b16", BLOCK + TILE + 1, 99)
    cs = [Case("base-%d" % bb, "base", "b16", x, bit_base=bb) for bb in BIT_BASES]
    cs += [Case("base-%d-dev" % bb, "base", "b16", x, bit_base=bb, dev=True) for bb in DEV_BASES]
    rng = np.random.default_rng(8)
    x8 = rng.integers(0, 256, BLOCK + 1001).astype(np.uint8)
    for bb, shift in ((0, 0), (128, 0), (8, 0), (0, 1)):     # the byte map, and the general pack of 8-bit codes
        cs.append(Case("base-f8-%d-shift%d" % (bb, shift), "base", "f8", x8, bit_base=bb, shift=shift))
    return cs


# ---- plan ------------------------------------------------------------------------------------
PLAN_BLOCKS = (1, 63, 64, 65, 128, 129)


def _plan_cases():
    pat = D.draw("b16", BLOCK + 17, 123)      # its period is not the block's: every block differs
    cs = [Case("plan-%d" % nb, "plan", "b16", np.resize(pat, nb * BLOCK - (5 if nb % 2 else 0))) for nb in PLAN_BLOCKS]
    one = np.full(BLOCK + 100, by_len("b16")[1], np.uint8)   # a count of 32768 in a u16
    one[BLOCK:] = D.draw("b16", 100, 5)
    cs.append(Case("plan-32768-of-one", "plan", "b16", one))
    return cs


FAMILIES = ("fit", "halves", "seq", "stores", "tail", "sync", "base", "plan")


@functools.lru_cache(maxsize=None)
def catalogue():
    cs = _fit_cases() + _halves_cases()
    cs += [_seq_case(name, g) for name in SEQS for g in SEQ_GRIDS]
    cs += _stores_cases() + _tail_cases() + _sync_cases() + _base_cases() + _plan_cases()
    assert len({c.name for c in cs}) == len(cs)
    return cs


def family(name):
    return [c for c in catalogue() if c.family == name]


def case(name):
    (c,) = [c for c in catalogue() if c.name == name]
    return c


# ---- refused packs ---------------------------------------------------------------------------
def refused_input():
    """three blocks under b16 whose boundaries fall inside words, and the same with byte 200
    (no code under b16) once in every block"""
    x = D.draw("b16", 2 * BLOCK + 777, 61)
    bad = x.copy()
    bad[[5, BLOCK + 5, 2 * BLOCK + 5]] = 200
    return x, bad
