"""A plain model of the batch Huffman bodies (hb_pack_seg, hb_record_check, hb_decode_body,
hb_canonical, hb_decode_slow, the two LUT fills and the dealing of k_hbs_decode / k_hbm_decode),
with the case catalogue of test_batch_body_model_cpu.py and test_gpu_batch_edges.py (TEST
INFRASTRUCTURE: numpy and the oracle only, no import of the product).

Everything starts from a lens record (256 code lengths in digits), n_ary, S and a segment's
bytes; the codes are the oracle's (orc.canonical, orc.bitcodes through huff_decode_model.codes),
the stream is orc.huff_pack's.

  expected_segment  mode, bits, the padded payload and the u16 sync entries of one segment
  expected_batch    the arrays of a whole batch in the own, shared or set mode (tid: the lowest
                    index of equal costs; records without a code for a present byte are skipped)
  hand_batch        the arrays of a batch for Codec.decode_batch / decode_batch_ranges built WITHOUT
                    the encoder, each segment under any record (or stored): a stream the device
                    never wrote. It is coded whenever bits <= 8 len, which the record check allows
                    and no plan ever writes at equality.
  model_decode      what hb_decode_body makes of a (possibly damaged) segment: chunk by chunk from
                    its sync position on the payload followed by zero words, every code found by
                    search among the record's codes; DC_OK and the bytes, or DC_E_STREAM
  geometry          the cuts of the pack and of the decode that a segment reaches (pack_geometry,
                    load_geometry, decode_geometry, write_geometry)
  deal_shared / deal_set   which path a group of four takes, and the record a workgroup holds,
                    builds, keeps and loses along its run under batch_grid 1, 2 and the default
  own_over_32       a histogram of at most 65536 bytes whose own table passes 32 bits (n = 5:
                    chain_counts), or None where depth_weight_bound shows there is none (n = 2, 3, 17)

The numbers are those of csrc/dc_batch_kernels.inc and dc_batch_shared_kernels.inc (HB_UNIT 16,
HB_THREADS 256, HB_LUT_BITS 12, HBS_WAVE_SEG 8192, the 128-byte pad of HB_OIDX, the default grid
of 512 workgroups): a change there changes them here with it.
"""
import functools

import numpy as np

from oracle import oracle as orc
from tests import huff_decode_model as D
from tests import huff_pack_model as P
from tests.test_batch_cpu import oracle_segment

HB_UNIT, HB_THREADS, HB_LUT_BITS, HBS_WAVE_SEG = 16, 256, 12, 8192
SEG_MAX = 65536
GRID_DEFAULT = 512
DC_OK, DC_E_ARG, DC_E_STREAM = 0, -1, -7
NONE = -1   # `have`: no table held


def digit_bits(n_ary):
    return max(int(n_ary) - 1, 1).bit_length()


def pad16(n):
    return (n + 15) // 16 * 16


# ---- records ---------------------------------------------------------------------------------
def _levels(n_ary, levels):
    """n_ary - 1 bytes per level with counts n_ary^level: lengths reach `levels` digits"""
    f = np.zeros(259, np.uint64)
    f[1: 1 + levels * (n_ary - 1)] = np.repeat(np.uint64(n_ary) ** np.arange(levels, dtype=np.uint64), n_ary - 1)
    return np.asarray(orc.huffman_lengths(f, n_ary))[:256].astype(np.int32)


def _n256():
    """bytes 0..199 one digit (8 bits), 200..255 two digits (16 bits)"""
    L = np.ones(256, np.int32)
    L[200:] = 2
    return L


OWN_RECORDS = {"n17": (17, lambda: _levels(17, 6)), "n256": (256, _n256)}
RECORD_NAMES = ("b12", "b13", "b16", "b23", "b32", "t89", "f8", "n3", "n5", "n16", "n17", "n256")


@functools.lru_cache(maxsize=None)
def record(name):
    """{"name", "n_ary", "w", "lens" (u8[256]), "code", "nbits", "enc_len", "enc_val", "by" (bits -> a byte)}"""
    if name in OWN_RECORDS:
        n_ary, make = OWN_RECORDS[name]
        lens = make()
    else:
        t = P.table(name)
        n_ary, lens = t["n_ary"], np.asarray(t["lengths"][:256])
    return make_record(lens, n_ary, name)


def make_record(lens, n_ary, name="?"):
    code, nb, mx, L, el, ev = D.codes(np.asarray(lens, np.int32)[:256], n_ary)
    nb = np.asarray(nb, np.int64)
    by = {int(b): int(np.nonzero(nb == b)[0][0]) for b in np.unique(nb) if b}
    return {"name": name, "n_ary": int(n_ary), "w": digit_bits(n_ary), "lens": np.asarray(lens, np.int64)[:256].astype(np.uint8),
            "code": np.asarray(code, np.uint32), "nbits": nb, "enc_len": el, "enc_val": ev, "by": by}


def record_valid(lens, n_ary):
    """the set's rule: every length L has L w <= 32, and Kraft in exact integers"""
    L = [int(v) for v in np.asarray(lens)[:256]]
    if any(v * digit_bits(n_ary) > 32 for v in L):
        return False
    top = max(L)
    return sum(n_ary ** (top - v) for v in L if v > 0) <= n_ary ** top


def own_usable(lens, n_ary):
    """hb_canonical's bad, negated: no length over 32 bits"""
    return int(np.asarray(lens).max(initial=0)) * digit_bits(n_ary) <= 32


# ---- one segment -----------------------------------------------------------------------------
def stored_sync(n, S):
    return np.array([8 * min(S, n - c * S) for c in range((n + S - 1) // S)], np.uint16)


def coded(rec, seg, S):
    """(bits, payload padded to 16, u16 sync entries) of seg under rec, by orc.huff_pack"""
    p, bits, idx = orc.huff_pack(seg, rec["code"], rec["nbits"].astype(np.uint8), 0, S)
    sl = np.diff(np.append(idx, np.uint64(bits))).astype(np.uint16)
    pay = np.zeros(pad16((bits + 7) // 8), np.uint8)
    pay[: p.size] = p
    return int(bits), pay, sl


def expected_segment(rec, seg, S, at_equality=False):
    """(mode, bits, padded payload, sync entries): coded when every byte has a code and the bits
    are < 8 len (at_equality: <=, the decoder's rule, for hand_batch), else stored"""
    seg = np.ascontiguousarray(seg, np.uint8)
    n = seg.size
    if n and rec is not None:
        nbs = rec["nbits"][seg]
        cb = int(nbs.sum())
        if (nbs > 0).all() and (cb < 8 * n or (at_equality and cb == 8 * n)):
            bits, pay, sl = coded(rec, seg, S)
            assert bits == cb
            return 1, bits, pay, sl
    pay = np.zeros(pad16(n), np.uint8)
    pay[:n] = seg
    return 0, 8 * n, pay, stored_sync(n, S)


def select(seg, records, n_ary):
    """(tid, usable): the cheapest valid record with a code for every byte, the lowest of equal ones"""
    h = np.bincount(seg, minlength=256).astype(np.int64)
    best = None
    for k, r in enumerate(records):
        L = np.asarray(r["lens"], np.int64)
        if not record_valid(L, n_ary) or ((h > 0) & (L == 0)).any():
            continue
        c = int((h * L).sum())
        if best is None or c < best[0]:
            best = (c, k)
    return (best[1], True) if best else (0, False)


def _assemble(parts, extra=None):
    out = dict(extra or {})
    out["mode"] = np.array([p[0] for p in parts], np.uint8)
    out["bits"] = np.array([p[1] for p in parts], np.int64)
    for name, off, j, dt in (("payload", "pay_off", 2, np.uint8), ("sync_len", "sync_off", 3, np.uint16)):
        out[name] = np.concatenate([p[j] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
        out[off] = np.concatenate(([0], np.cumsum([p[j].size for p in parts]))).astype(np.int64)
    return out


def expected_batch(mode, segs, n_ary, S, records=None):
    """The arrays an encode writes. mode "own": lens / mode / bits / ...; "shared" (records: one
    record): mode / bits / ...; "set": tid as well."""
    if mode == "own":
        parts, lens = [], np.zeros((len(segs), 256), np.uint8)
        for i, s in enumerate(segs):
            s = np.ascontiguousarray(s, np.uint8)
            L = orc.huffman_lengths(orc.histogram(s), n_ary)[:256] if s.size else np.zeros(256, np.int32)
            if not own_usable(L, n_ary):
                # k_hb_plan's `maxbits <= 32` false: the record is written as it is, the segment stored
                # (orc.bitcodes answers -1 for such a table, which oracle_segment's `mx <= 32` lets through)
                lens[i] = L
                parts.append(expected_segment(None, s, S))
                continue
            lens[i], m, b, p, sl = oracle_segment(s, n_ary, S)
            pay = np.zeros(pad16(p.size), np.uint8)
            pay[: p.size] = p
            parts.append((m, b, pay, sl))
        return _assemble(parts, {"lens": lens})
    if mode == "shared":
        return _assemble([expected_segment(records[0], s, S) for s in segs])
    tid, parts = np.zeros(len(segs), np.uint8), []
    for i, s in enumerate(segs):
        k, usable = select(s, records, n_ary) if len(s) else (0, False)
        tid[i] = k
        parts.append(expected_segment(records[k] if usable else None, s, S))
    return _assemble(parts, {"tid": tid})


def hand_batch(mode, items, n_ary, S, records=None):
    """items: (segment bytes, k) with k the index in `records` of the record that codes it, or None
    for a stored segment. Returns the arrays of expected_batch plus "segs"; own mode: lens[i] is
    the record's (zeros for a stored segment), set mode: tid 255 on the stored ones."""
    parts, lens, tid = [], np.zeros((len(items), 256), np.uint8), np.full(len(items), 255, np.uint8)
    for i, (s, k) in enumerate(items):
        part = expected_segment(records[k] if k is not None else None, s, S, at_equality=True)
        assert part[0] == (k is not None and len(s) > 0), (i, "the record does not code this segment within 8 len bits")
        if part[0]:
            lens[i], tid[i] = records[k]["lens"], k
        parts.append(part)
    out = _assemble(parts, {"segs": [np.ascontiguousarray(s, np.uint8) for s, _ in items]})
    if mode == "own":
        out["lens"] = lens
    if mode == "set":
        out["tid"] = tid
    return out


# ---- the decoder -----------------------------------------------------------------------------
def words_be(pay):
    """the payload as HB_WORD gives it: big-endian dwords"""
    return np.ascontiguousarray(pay, np.uint8).view(">u4").astype(np.uint64)


def _search_tables(rec):
    if "_search" not in rec:
        by = {}
        for s in range(256):
            if 0 < rec["nbits"][s] <= 32:
                by.setdefault(int(rec["nbits"][s]), {})[int(rec["code"][s])] = s
        rec["_search"] = sorted(by.items())
    return rec["_search"]


def lookup(rec, win):
    """(symbol, bits) of the code that leads the 32-bit window, by search; (None, 0): no code"""
    for L, d in _search_tables(rec):
        s = d.get(win >> (32 - L))
        if s is not None:
            return s, L
    return None, 0


def model_decode(rec, mode, bits, pay, sl, n, S, chunks=None, trace=None):
    """hb_decode_body on one segment (chunks: only these, as a range does; then the sum test is
    "the last one ends within bits"): (status, bytes or None). trace: a list that takes
    (chunk, symbol, wbits before the refill test, code bits, word indices read so far)."""
    nch = (n + S - 1) // S
    sl = np.asarray(sl, np.int64)
    if mode > 1 or bits > 8 * n or (mode == 0 and bits != 8 * n) or len(pay) != pad16((bits + 7) // 8) or sl.size != nch:
        return DC_E_STREAM, None
    pos = np.concatenate(([0], np.cumsum(sl)))
    todo = range(nch) if chunks is None else chunks
    out = np.zeros(n, np.uint8)
    if mode == 0:
        for c in todo:
            if sl[c] != 8 * min(S, n - c * S):
                return DC_E_STREAM, None
        out[:] = pay[:n]
    else:
        w = words_be(pay)
        nw = w.size
        word = lambda k: int(w[k]) if k < nw else 0
        for c in todo:
            p, cnt, used = int(pos[c]), min(S, n - c * S), 0
            k, sh = p >> 5, p & 31
            win = (((word(k) << 32) | word(k + 1)) << sh) & (2 ** 64 - 1)
            wbits, k = 64 - sh, k + 2
            for j in range(cnt):
                pre = wbits
                if wbits < 32:
                    win |= word(k) << (32 - wbits)
                    k, wbits = k + 1, wbits + 32
                s, nb = lookup(rec, win >> 32)
                if trace is not None:
                    trace.append((c, j, pre, nb, k))
                if not nb:
                    return DC_E_STREAM, None
                out[c * S + j] = s
                win, wbits, used = (win << nb) & (2 ** 64 - 1), wbits - nb, used + nb
            if used != sl[c]:
                return DC_E_STREAM, None
    end = int(pos[max(todo) + 1]) if len(todo) else 0
    if (chunks is None and int(pos[-1]) != bits) or (chunks is not None and end > bits):
        return DC_E_STREAM, None
    return DC_OK, out


# ---- geometry --------------------------------------------------------------------------------
def pack_geometry(rec, seg, addr=0):
    """The cuts of hb_pack_seg for a coded segment whose first byte lies at address `addr`."""
    seg = np.ascontiguousarray(seg, np.uint8)
    n = seg.size
    units = (n + HB_UNIT - 1) // HB_UNIT
    nb = rec["nbits"][seg]
    pos = np.concatenate(([0], np.cumsum(nb)))
    bits = int(pos[-1])
    nacc = pos[:-1] & 31
    g = {"len": n, "units": units, "rounds": (units + HB_THREADS - 1) // HB_THREADS,
         "scan_threads": (units + 15) // 16, "units_last_thread": units - 16 * ((units - 1) // 16),
         "n": nb, "nacc": nacc, "shift": 64 - nacc - nb, "flush": nacc + nb >= 32,
         "bits": bits, "words": (bits + 31) // 32, "psize": pad16((bits + 7) // 8),
         "last_piece": (pad16((bits + 7) // 8) // 16 - 1) if bits else -1,
         "closing_or": np.array([int(pos[min(16 * (u + 1), n)]) & 31 != 0 for u in range(units)], bool)}
    g.update(load_geometry(n, addr))
    return g


def load_geometry(n, addr):
    """hb_load16 of every unit: a = address & 3, and which of the five dwords lie at or past the end"""
    units = (n + HB_UNIT - 1) // HB_UNIT
    s = addr + HB_UNIT * np.arange(units)
    a = s & 3
    past = (s - a)[:, None] + 4 * np.arange(5)[None, :] >= addr + n
    mis = (-addr) & 3
    return {"a": a, "past": past, "mis": mis, "hist_head": min(mis, n), "hist_dwords": (n - min(mis, n)) // 4,
            "hist_tail": (n - min(mis, n)) % 4}


def decode_geometry(rec, seg, S, NT, phase=0, first=0, count=None):
    """The cuts of hb_decode_body for a coded segment (first / count: a range of it): chunks and
    rounds, and per symbol of the touched chunks wbits before the refill test, the refill, LUT hit
    or slow search, and the words read."""
    seg = np.ascontiguousarray(seg, np.uint8)
    n = seg.size
    count = n if count is None else count
    nch = (n + S - 1) // S
    c_lo, c_hi = first // S, (first + count + S - 1) // S
    nb = rec["nbits"][seg]
    pos = np.concatenate(([0], np.cumsum(nb)))
    bits = int(pos[-1])
    nw = pad16((bits + 7) // 8) // 4
    cpos = pos[np.arange(c_lo, c_hi) * S]
    sym = np.arange(c_lo * S, min(c_hi * S, n))
    chunk = sym // S
    sh = pos[chunk * S] & 31
    u = pos[sym] - pos[chunk * S]
    wlook = np.where((sh == 0) & (u == 0), 64, 32 + ((64 - sh - u) % 32))
    wpre = np.where(sym % S == 0, 64 - sh, np.roll(wlook, 1) - np.roll(nb[sym], 1))
    refill = wpre < 32
    last = np.minimum((np.arange(c_lo, c_hi) + 1) * S, n)
    # words: k, k + 1 at the start, one more per refill
    nref = np.add.reduceat(refill.astype(np.int64), (np.arange(c_lo, c_hi) - c_lo) * S) if c_hi > c_lo else np.zeros(0, np.int64)
    wmax = (cpos >> 5) + 1 + nref
    g = {"nch": nch, "c_lo": c_lo, "c_hi": c_hi, "rounds": (c_hi - c_lo + NT - 1) // NT, "NT": NT,
         "pos": cpos, "sh": cpos & 31, "clen": pos[last] - cpos, "sym": sym, "wpre": wpre, "refill": refill,
         "slow": nb[sym] > HB_LUT_BITS, "n": nb[sym], "nw": nw, "word_max": wmax, "past_nw": wmax >= nw,
         "first_partial": first % S != 0, "last_partial": (first + count) % S != 0 and first + count != n,
         "row_negative": c_lo * S < first}
    g.update(write_geometry(phase, count))
    return g


def write_geometry(phase, n):
    """the staged write: head bytes, 16-byte pieces, tail bytes, and whether a staged byte lies
    either side of a 128-byte pad (HB_OIDX)"""
    head = min((16 - phase) & 15, n)
    nbody = (n - head) >> 4
    return {"phase": phase, "head": head, "nbody": nbody, "tail": n - head - 16 * nbody,
            "below_head": n < ((16 - phase) & 15), "crosses_pad": (phase + n - 1) >> 7 > phase >> 7 if n else False}


def geometry(rec, seg, S, NT=64, addr=0, phase=0, first=0, count=None):
    """{"pack", "decode"}: the cuts a coded segment reaches in hb_pack_seg (its first byte at
    address addr) and in hb_decode_body (NT 64: a wave, 256: the workgroup; first / count: a range)"""
    return {"pack": pack_geometry(rec, seg, addr), "decode": decode_geometry(rec, seg, S, NT, phase, first, count)}


def oidx(p):
    return p + 4 * (p >> 7)


# ---- dealing ---------------------------------------------------------------------------------
def grid_of(work, opt=0):
    cap = opt if opt else GRID_DEFAULT
    return min(work, cap)


def deal_shared(lengths):
    """per group of four: ("wave" | "wg", nseg)"""
    out = []
    for g in range(0, len(lengths), 4):
        grp = lengths[g: g + 4]
        out.append(("wave" if all(v <= HBS_WAVE_SEG for v in grp) else "wg", len(grp)))
    return out


def deal_set(lengths, modes, tids, records, n_ary, grid=0):
    """k_hbm_decode: per group (workgroup, path, the record held before the group, after it).
    The wave path needs all short and the coded ones of one record that builds."""
    ngroups = (len(lengths) + 3) // 4
    G = grid_of(ngroups, grid)
    per = (ngroups + G - 1) // G if G else 0
    K = len(records)
    usable = lambda k: k < K and own_usable(records[k]["lens"], n_ary)
    out = []
    for wg in range(G):
        have = NONE
        for g in range(min(per * wg, ngroups), min(per * wg + per, ngroups)):
            idx = list(range(4 * g, min(4 * g + 4, len(lengths))))
            before, ev = have, []

            def table(k):   # hbm_table
                nonlocal have
                if k >= K:
                    return False
                if k == have:
                    ev.append("kept")
                    return True
                ok = usable(k)
                ev.append("built" if ok else "reset")
                have = k if ok else NONE
                return ok

            waves, k = True, NONE
            for i in idx:
                waves = waves and lengths[i] <= HBS_WAVE_SEG
                if waves and modes[i] == 1:
                    waves = k == NONE or tids[i] == k
                    k = int(tids[i])
            if waves and k != NONE:
                waves = table(k)
            if not waves:
                for i in idx:
                    if modes[i] == 1 and lengths[i] > 0:
                        table(int(tids[i]))
            out.append({"wg": wg, "group": g, "path": "wave" if waves else "wg", "nseg": len(idx), "have_before": before,
                        "have_after": have, "events": ev})
    return out


# ---- composing inputs ------------------------------------------------------------------------
def fill(rec, n, seed=0, short=None):
    """n bytes of the record's shortest codes (or of `short` bits), two values in turn by a seed"""
    b = min(rec["by"]) if short is None else short
    have = np.nonzero(rec["nbits"] == b)[0]
    rng = np.random.default_rng(seed)
    return have[rng.integers(0, have.size, n)].astype(np.uint8)


def plant(rec, n, spots, seed=0):
    """fill(rec, n) with the byte of `bits` code bits at each (position, bits) of spots"""
    x = fill(rec, n, seed)
    for at, b in spots:
        x[at] = rec["by"][b]
    return x


def every_length(rec):
    """one byte of each code length of the record that fits 32 bits"""
    return np.array([rec["by"][b] for b in sorted(rec["by"]) if b <= 32], np.uint8)


class Case:
    """One call. kind "enc": encode `segs` (mode shared / set / own) from an input buffer whose first
    segment starts `lead` bytes past a 16-byte boundary, with `after` filling what follows the
    segments; the result is expected_batch's. kind "dec": decode the hand_batch of `items` in
    `mode`, segment i to an output start of phase starts[i] % 16; `damage` (a function of the
    hand batch's arrays) then alters the stream, and the expected statuses are model_decode's.
    ranges: None, or rows (segment, first, count) for decode_batch_ranges."""

    def __init__(self, name, family, kind, mode, n_ary, S, records, segs=None, items=None, lead=0, after=0x00, grid=0,
                 phases=None, damage=None, tid=None, ranges=None):
        self.name, self.family, self.kind, self.mode, self.n_ary, self.S = name, family, kind, mode, n_ary, S
        self.records, self.segs, self.items, self.lead, self.after, self.grid = records, segs, items, lead, after, grid
        self.phases, self.damage, self.tid, self.ranges = phases, damage, tid, ranges

    def __repr__(self):
        return self.name

    # encode
    def expected(self):
        return _expected(self)

    # decode
    def batch(self):
        return _batch(self)

    def outcome(self):
        """(statuses, list of bytes or None) of the whole-segment decode, by model_decode"""
        return _outcome(self)

    def rows(self):
        """the (segment, first, count) rows of the ranges call: self.ranges, or for every segment
        the whole of it and a short range in its first, a middle and its last chunk"""
        if self.ranges is not None:
            return [tuple(r) for r in self.ranges]
        rows = []
        for i, (s, _) in enumerate(self.items):
            n, S = len(s), self.S
            if n == 0:
                rows.append((i, 0, 0))
                continue
            nch = (n + S - 1) // S
            rows.append((i, 0, n))
            for c in sorted({0, nch // 2, nch - 1}):
                lo, hi = c * S, min(n, c * S + S)
                f = lo + (1 if hi - lo > 2 else 0)
                rows.append((i, f, max(1, min(S // 2, hi - f - (1 if hi - f > 1 else 0)))))
        return rows


@functools.lru_cache(maxsize=None)
def _expected(case):
    return expected_batch(case.mode, case.segs, case.n_ary, case.S, case.records)


@functools.lru_cache(maxsize=None)
def _batch(case):
    b = hand_batch(case.mode, case.items, case.n_ary, case.S, case.records)
    if case.tid is not None:
        b["tid"] = np.array(case.tid, np.uint8)
    if case.damage is not None:
        b = case.damage({k: (v.copy() if hasattr(v, "copy") else v) for k, v in b.items()})
    return b


def segment_view(b, i):
    """(mode, bits, payload, sync entries) of segment i of a batch's arrays"""
    return (int(b["mode"][i]), int(b["bits"][i]), b["payload"][b["pay_off"][i]: b["pay_off"][i + 1]],
            b["sync_len"][b["sync_off"][i]: b["sync_off"][i + 1]])


def _record_of(case, b, i):
    if case.mode == "own":
        return make_record(b["lens"][i], case.n_ary) if own_usable(b["lens"][i], case.n_ary) else None
    k = int(b["tid"][i]) if case.mode == "set" else 0
    return case.records[k] if k < len(case.records) and own_usable(case.records[k]["lens"], case.n_ary) else None


@functools.lru_cache(maxsize=None)
def _outcome(case):
    b = case.batch()
    st, out = [], []
    for i, (s, k) in enumerate(case.items):
        m, bits, pay, sl = segment_view(b, i)
        if case.damage is None and case.tid is None:
            st.append(DC_OK)       # an undamaged hand batch decodes: pinned to orc.huff_unpack on the CPU side
            out.append(np.ascontiguousarray(s, np.uint8))
            continue
        rec = _record_of(case, b, i) if m == 1 else None
        if m == 1 and rec is None and len(s):
            st.append(DC_E_STREAM)
            out.append(None)
            continue
        r, o = model_decode(rec, m, bits, pay, sl, len(s), case.S)
        st.append(r if len(s) or r else DC_OK)
        out.append(o)
    return st, out


def range_outcome(case, row):
    """(status, bytes or None) of one range row, by model_decode over the chunks it touches"""
    i, f, c = row
    b = case.batch()
    s = case.items[i][0]
    if c == 0:
        return DC_OK, np.zeros(0, np.uint8)
    m, bits, pay, sl = segment_view(b, i)
    rec = _record_of(case, b, i) if m == 1 else None
    if m == 1 and rec is None:
        return DC_E_STREAM, None
    if case.damage is None and case.tid is None:
        return DC_OK, np.ascontiguousarray(s[f: f + c], np.uint8)
    S = case.S
    r, o = model_decode(rec, m, bits, pay, sl, len(s), S, chunks=range(f // S, (f + c + S - 1) // S))
    return r, (o[f: f + c] if o is not None else None)


# ---- the catalogue ---------------------------------------------------------------------------
PHASE_SIZES = (1, 2, 3, 14, 15, 16, 17, 31, 32, 33, 127, 128, 129, 130, 255, 256, 257, 258, 8191, 8192)
UNIT_LENS = (1, 15, 16, 17, 4079, 4080, 4081, 4095, 4096, 4097, 4112, 16 * 16 + 1, 16 * 16 * 255 + 1, 65535, 65536)
CHUNK_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)


def _long_spots(rec, n, S):
    """the longest code first in a chunk, last in a chunk, last in the segment"""
    top = max(b for b in rec["by"] if b <= 32)
    spots = [(n - 1, top)]
    if n > S:
        spots += [(S, top), (2 * S - 1 if n >= 2 * S else S - 1, top)]
    return spots


def _with_every_length(rec, n, S, seed):
    x = plant(rec, n, _long_spots(rec, n, S), seed)
    ev = every_length(rec)
    at = 1 if n > ev.size + 2 else 0
    x[at: at + min(ev.size, n - at - 1)] = ev[: max(0, min(ev.size, n - at - 1))]
    return x


def _coded_or_padded(rec, x):
    """x, with shortest codes appended until it codes within 8 len bits (a hand batch needs that)"""
    short = min(rec["by"])
    assert short < 8, rec["name"]
    nb = int(rec["nbits"][x].sum())
    extra = max(0, -(-(nb - 8 * x.size) // (8 - short)))
    return np.concatenate([x, fill(rec, extra, 9)]) if extra else x


def _codes_cases():
    cs = []
    for name in RECORD_NAMES:
        rec = record(name)
        n_ary = rec["n_ary"]
        if name in ("f8", "n256"):   # 8 bits a code at best: coded only by hand, at equality
            x = fill(rec, 300, 1)
        else:
            x = _coded_or_padded(rec, _with_every_length(rec, 700, 64, 2))
        y = x[: x.size // 3 + 1]
        y = _coded_or_padded(rec, y) if name not in ("f8", "n256") else y
        for mode in ("own", "shared", "set"):
            recs = [rec] if mode != "set" else [record("f8") if n_ary == 2 else make_record(np.zeros(256), n_ary, "zeros"), rec]
            k = len(recs) - 1
            cs.append(Case(f"codes-{name}-{mode}-dec", "codes", "dec", mode, n_ary, 64, recs,
                           items=[(x, k), (y, k), (x[:5], None), (x[::-1].copy(), k)], phases=(3, 0, 9, 15)))
        for mode in ("shared", "set"):
            recs = [rec] if mode == "shared" else [make_record(np.zeros(256), n_ary, "zeros"), rec]
            cs.append(Case(f"codes-{name}-{mode}-enc", "codes", "enc", mode, n_ary, 64, recs, segs=[x, y, x[::-1].copy()], lead=5))
    return cs


def _window_cases():
    rec = record("b32")
    cs, items = [], []
    # a 32-bit code starting at bit 0, 1 and 31 mod 32 (1-bit codes before it), four in a row, and 1-bit codes only
    for lead in (0, 1, 31, 32, 33):
        items.append(plant(rec, lead + 80, [(lead, 32)], lead))
    items.append(plant(rec, 200, [(7, 32), (8, 32), (9, 32), (10, 32)], 3))
    items.append(fill(rec, 64 * 5 + 3, 4))
    # wbits before the refill test exactly 32 and 31: a chunk from bit 0 under codes of 32 and of 1 + 32 bits
    items.append(plant(rec, 200, [(0, 32), (1, 32)], 5))
    items.append(plant(rec, 200, [(0, 32), (1, 1), (2, 32)], 6))
    # bits = 0, 1, 127 mod 128 and 0, 1, 31 mod 32 with a long code last
    for want in (128, 129, 255, 160, 161, 191):
        n = want - 31      # n - 1 one-bit codes and one of 32 bits
        items.append(plant(rec, n, [(n - 1, 32)], want))
    for mode in ("own", "shared", "set"):
        recs = [rec] if mode != "set" else [record("f8"), rec]
        k = len(recs) - 1
        cs.append(Case(f"window-{mode}-dec", "window", "dec", mode, 2, 64, recs, items=[(x, k) for x in items],
                       phases=tuple(range(len(items)))))
    for mode in ("shared", "set"):
        recs = [rec] if mode == "shared" else [record("f8"), rec]
        cs.append(Case(f"window-{mode}-enc", "window", "enc", mode, 2, 64, recs, segs=items, lead=1))
    return cs


def _units_cases():
    rec = record("t89")
    nocode = make_record(np.where(np.arange(256) == 0xEE, 0, record("t89")["lens"]), 2, "t89-hole")
    cs = []
    segs = [fill(rec, n, n, short=7) for n in UNIT_LENS]
    segs.append(np.full(65536, 1, np.uint8))            # 65536 equal bytes: past a u16 counter
    for after in (0x00, 0xFF, 0xEE):
        for lead in ((0, 1, 2, 3) if after == 0 else (3,)):
            for mode, recs in (("shared", [nocode]), ("set", [record("f8"), nocode]), ("own", None)):
                cs.append(Case(f"units-{mode}-lead{lead}-after{after:02x}", "units", "enc", mode, 2, 64, recs, segs=segs, lead=lead,
                               after=after))
    # each of the 16 alignments, short segments (len < mis included), own and shared
    small = [fill(rec, n, 40 + n, short=7) for n in (1, 2, 3, 5, 15, 16, 17, 33)]
    for lead in range(16):
        for mode, recs in (("shared", [nocode]), ("own", None)):
            cs.append(Case(f"units-{mode}-align{lead}", "units", "enc", mode, 2, 16, recs, segs=small, lead=lead, after=0xEE))
    return cs


def _chunks_cases():
    rec, b32 = record("b16"), record("b32")
    cs = []
    for S in (16, 64, 1024):
        items = []
        for nch in CHUNK_COUNTS:
            for last in (1, S - 1):
                n = (nch - 1) * S + last
                if n <= SEG_MAX and n > 0:
                    items.append(P.chain_draw("b16", n, nch + last, lo=1, hi=8))
        if S == 16:
            assert len(items) % 4 == 0
            items.append(P.chain_draw("b16", 8192, 8, lo=1, hi=8))     # 512 chunks in a wave: a group of four short
            items += [P.chain_draw("b16", n, n, lo=1, hi=8) for n in (33, 1, 700)]
            items.append(P.chain_draw("b16", 65536, 7, lo=1, hi=8))    # 4096 chunks
        items = [(x, 0) for x in items]
        recs = [rec]
        if S == 1024:   # a chunk of 32768 bits: 1024 codes of 32 bits, 1-bit codes around it
            x = fill(b32, 8192, 1)
            x[1024: 2048] = b32["by"][32]
            recs = [rec, b32]
            items.append((x, 1))
        for mode in ("own", "set", "shared"):
            its = items if mode != "shared" else [it for it in items if it[1] == 0]
            cs.append(Case(f"chunks-S{S}-{mode}-dec", "chunks", "dec", mode, 2, S, recs if mode != "shared" else [rec], items=its,
                           phases=tuple((5 * i) % 16 for i in range(len(its)))))
        enc_segs = [x for x, k in items if k == 0]
        cs.append(Case(f"chunks-S{S}-shared-enc", "chunks", "enc", "shared", 2, S, [rec], segs=enc_segs, lead=7))
        if S == 1024:
            cs.append(Case("chunks-S1024-b32-enc", "chunks", "enc", "shared", 2, S, [b32], segs=[items[-1][0]], lead=2))
            cs.append(Case("chunks-S1024-b32-shared-dec", "chunks", "dec", "shared", 2, S, [b32], items=[(items[-1][0], 0)], phases=(11,)))
    return cs


PHASE_HALVES = (("small", tuple(n for n in PHASE_SIZES if n <= 33)), ("large", tuple(n for n in PHASE_SIZES if n > 33)))


def _phase_cases():
    """every phase x every size, in each of: wave and workgroup instance, stored and coded (two
    cases each, the sizes up to 33 and those above, to keep a call short), and ranges"""
    rec = record("b16")
    cs = []
    for long in (False, True):   # all short: the wave instance; with one of 8193: the workgroup instance
        for md in (0, 1):
            for half, sizes in PHASE_HALVES:
                items, phases = [], []
                for n in sizes:
                    for ph in range(16):
                        items.append((P.chain_draw("b16", n, n + ph, lo=1, hi=6), 0 if md else None))
                        phases.append(ph)
                if long:
                    # one long segment in every group of four
                    merged, mph = [], []
                    for i, (it, ph) in enumerate(zip(items, phases)):
                        if i % 3 == 0:
                            merged.append((P.chain_draw("b16", 8193, i, lo=1, hi=6), 0 if md else None))
                            mph.append(ph)
                        merged.append(it)
                        mph.append(ph)
                    items, phases = merged, mph
                for mode in ("shared", "set", "own") if not long else ("shared", "set"):
                    cs.append(Case(f"phase-{'wg' if long or mode == 'own' else 'wave'}-mode{md}-{mode}-{half}", "phase", "dec", mode,
                                   2, 64, [rec], items=items, phases=tuple(phases)))
    # ranges with the same (phase, count) whose first and last touched chunks are partial
    x = P.chain_draw("b16", 20000, 77, lo=1, hi=6)
    rows = []
    for j, n in enumerate(PHASE_SIZES):
        for ph in range(16):
            rows.append((0, 64 * (j + 1) + 5 + ph, n, ph))
    for mode in ("shared", "set", "own"):
        cs.append(Case(f"phase-ranges-{mode}", "phase", "dec", mode, 2, 64, [rec], items=[(x, 0)], phases=(0,),
                       ranges=[r[:3] for r in rows]))
        cs[-1].range_phases = [r[3] for r in rows]
    return cs


def _t89_at(cost_minus_8n, n, seed):
    """n bytes that cost 8 n + cost_minus_8n bits under t89"""
    x = P.t89_block(8 * n + cost_minus_8n, seed, n=n)
    x[x == 0xEE] = 0xED     # (both 8 bits: 0xEE is the byte the "hole" records leave without a code)
    return x


def _mode_cases():
    t89, f8 = record("t89"), record("f8")
    hole = make_record(np.where(np.arange(256) == 0xEE, 0, t89["lens"]), 2, "t89-hole")
    cs = []
    segs = [_t89_at(d, n, 3 * n + d + 1) for n in (1000, 17) for d in (-1, 0, 1)]
    miss = [np.concatenate(([0xEE], _t89_at(-5, 99, 1))).astype(np.uint8), np.concatenate((_t89_at(-5, 99, 2), [0xEE])).astype(np.uint8),
            np.array([0xEE], np.uint8)]
    cs.append(Case("mode-t89-shared", "mode", "enc", "shared", 2, 64, [t89], segs=segs, lead=3))
    cs.append(Case("mode-hole-shared", "mode", "enc", "shared", 2, 64, [hole], segs=segs + miss, lead=3))
    cs.append(Case("mode-f8-shared", "mode", "enc", "shared", 2, 64, [f8], segs=segs[:2] + [fill(f8, 4096, 1)], lead=0))
    # the set: equality under the cheapest record; two records of equal cost; an invalid record cheaper than every valid one
    ones = make_record(np.ones(256), 2, "ones")
    cs.append(Case("mode-set", "mode", "enc", "set", 2, 64, [ones, f8, t89, make_record(t89["lens"], 2, "t89-again"), hole],
                   segs=segs + miss, lead=3))
    cs.append(Case("mode-set-hole-first", "mode", "enc", "set", 2, 64, [hole, t89, ones], segs=segs + miss, lead=9))
    own = own_equality_segment()
    assert own is not None, "the search for an own table that costs exactly 8 len bits found none"
    cs.append(Case("mode-own-equality", "mode", "enc", "own", 2, 64, None, segs=[own, own[:-1], np.append(own, own[0])], lead=1))
    return cs + _own_over32_cases()


@functools.lru_cache(maxsize=None)
def own_equality_segment():
    """A segment whose own Huffman code costs exactly 8 len bits, found with the oracle: 256 values
    with counts c and 2c (Kraft-complete lengths 8 +- 1 balance only where the cost is exactly
    8 n). None if the search finds none."""
    # 128 bytes of count 3 (9 bits) would need 64 of 7 bits ...: search small families
    for a in range(1, 5):
        for lo in range(2, 255, 2):
            # `lo` values twice as frequent as the rest would get 7 bits, 2 lo of the rest 9 bits
            counts = np.full(256, a, np.int64)
            counts[:lo] = 2 * a + 1
            seg = np.repeat(np.arange(256, dtype=np.uint8), counts)
            if seg.size > SEG_MAX:
                continue
            L = orc.huffman_lengths(orc.histogram(seg), 2)[:256]
            if int((counts * L).sum()) == 8 * seg.size and L.max() > 8:
                return np.random.default_rng(lo).permutation(seg)
    return None


def chain_counts(n_ary, levels):
    """A light histogram whose n-ary tree (orc.huffman_lengths) is `levels` digits deep: 2 (n - 1)
    values of count 1, which with the one dummy leaf (count 1, the highest index) make the first
    two merges, n and 2 n - 1; then per level n - 1 values one heavier than the node of two merges
    before, so that every merge takes n - 1 leaves and the node before it, and the node before that
    is always gone: leaf[k + 1] = node[k - 1] + 1, node[k + 1] = node[k] + (n - 1) leaf[k + 1]."""
    n = int(n_ary)
    counts, nodes = [1] * (2 * (n - 1)), [n, 2 * n - 1]
    while len(nodes) < levels:
        leaf = nodes[-2] + 1
        counts += [leaf] * (n - 1)
        nodes.append(nodes[-1] + (n - 1) * leaf)
    return np.array(counts, np.int64)


def depth_weight_bound(n_ary, depth):
    """A lower bound on the bytes of a segment whose own n-ary table has a code of `depth` digits.
    The builder (orc.huffman_lengths) adds 1 to n - 1 dummy leaves of count 1 and merges the n
    lightest active items each time, so the sums of the merges never decrease. Let v[0] be a leaf
    of that depth and v[k + 1] the parent of v[k]. Any other child s of v[k + 1] was either active
    when v[k] was made and not taken, so s >= every child of v[k], v[k - 1] among them, or it was
    made after v[k], so s >= v[k] >= v[k - 1]. Hence v[k + 1] >= v[k] + (n - 1) v[k - 1], with
    v[0] >= 1 and v[1] >= n; the root is the bytes and the dummies."""
    a, b = 1, int(n_ary)
    for _ in range(depth - 1):
        a, b = b, b + (n_ary - 1) * a
    return b - (n_ary - 1)


def lengths_of_counts(counts, n_ary):
    h = np.zeros(259, np.uint64)
    h[: len(counts)] = counts
    return orc.huffman_lengths(h, n_ary)[:256]


def over_32_digits(n_ary):
    """the fewest digits that pass 32 bits"""
    return 32 // digit_bits(n_ary) + 1


@functools.lru_cache(maxsize=None)
def own_over_32(n_ary):
    """A histogram (counts of the byte values 0, 1, ..) of at most 65536 bytes whose oracle lengths
    pass 32 bits at n_ary, or None. Where depth_weight_bound already passes 65536 there is none;
    elsewhere the search is chain_counts, confirmed by the oracle."""
    need = over_32_digits(n_ary)
    if depth_weight_bound(n_ary, need) > SEG_MAX:
        return None
    c = chain_counts(n_ary, need)
    if c.size <= 256 and int(c.sum()) <= SEG_MAX and int(lengths_of_counts(c, n_ary).max()) >= need:
        return c
    return None


def segment_of_counts(counts, seed):
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(len(counts), dtype=np.uint8), counts))


def _plant_lens(seg_index, lens, mode=None):
    """segment seg_index carries this lens record (and this mode): what the encoder leaves beside a
    segment it stored because its own table passes 32 bits"""
    def f(b):
        b["lens"][seg_index] = lens
        if mode is not None:
            b["mode"][seg_index] = mode
        return b
    return f


def _own_over32_cases():
    """n = 5: the own table of a segment of 57248 bytes has codes of 11 digits = 33 bits. The plan
    writes the record and stores the segment; the decoder takes the stored segment whatever its
    record, and refuses a segment that claims to be coded under it. Beside it the same family one
    digit shallower (10 digits = 30 bits: coded)."""
    n_ary = 5
    counts = own_over_32(n_ary)
    assert counts is not None, "no own table over 32 bits within 65536 bytes at n = 5"
    need = over_32_digits(n_ary)
    L = lengths_of_counts(counts, n_ary)
    assert int(L.max()) == need and need * digit_bits(n_ary) == 33
    big = segment_of_counts(counts, 5)
    below = segment_of_counts(chain_counts(n_ary, need - 1), 6)
    rec = make_record(lengths_of_counts(chain_counts(n_ary, need - 1), n_ary), n_ary, "n5-own-30")
    small = below[:300]
    cs = [Case("mode-own-over32-n5", "mode", "enc", "own", n_ary, 64, None, segs=[below, big, small, big[::-1].copy()], lead=3)]
    items = [(below, 0), (big, None), (_coded_or_padded(rec, np.sort(small)), 0)]
    cs.append(Case("mode-own-over32-n5-stored-dec", "mode", "dec", "own", n_ary, 64, [rec], items=items, phases=(2, 7, 13),
                   damage=_plant_lens(1, L)))
    cs.append(Case("mode-own-over32-n5-coded-dec", "mode", "dec", "own", n_ary, 64, [rec], items=items, phases=(2, 7, 13),
                   damage=_plant_lens(1, L, mode=1)))
    return cs


def _deal_cases():
    rec, hexr = record("b16"), record("t89")
    cs = []
    short = lambda n, seed: P.chain_draw("b16", n, seed, lo=1, hi=6)
    for count in (1, 2, 3, 4, 5, 7, 8):
        items = [(short(300 + 17 * i, i), 0) for i in range(count)]
        for mode in ("shared", "set"):
            for grid in (1, 2, 0):
                cs.append(Case(f"deal-count{count}-{mode}-grid{grid}", "deal", "dec", mode, 2, 64, [rec], items=items,
                               phases=tuple(range(count)), grid=grid))
    groups = [[(short(400, 1), 0), (short(8192, 2), 0), (short(1, 3), 0), (short(64, 4), 0)],           # four short
              [(short(500, 5), 0), (short(8193, 6), 0), (short(20, 7), 0), (short(8192, 8), 0)],        # one of 8193
              [(short(100, 9), 0), (np.zeros(0, np.uint8), None), (short(90, 10), 0), (short(80, 11), 0)],   # a zero length inside
              [(short(100, 12), 0), (_t89_at(-20, 300, 1), 1), (short(90, 13), 0), (short(80, 14), 0)],      # two records
              [(short(100, 15), 0), (short(300, 16), None), (short(90, 17), 0), (short(80, 18), None)],      # coded and stored
              [(_t89_at(-9, 200, 2), 1), (_t89_at(-9, 100, 3), 1)]]
    flat = [it for g in groups for it in g]
    for grid in (1, 2, 0):
        cs.append(Case(f"deal-groups-set-grid{grid}", "deal", "dec", "set", 2, 64, [rec, hexr], items=flat,
                       phases=tuple((3 * i) % 16 for i in range(len(flat))), grid=grid))
        bad_tid = [255 if k is None else k for _, k in flat]
        bad_tid[2] = 3        # >= K on a coded segment of a wave group: DC_E_STREAM, neighbours exact
        bad_tid[14] = 2       # a record with a code of 33 bits: no table, and the one held is lost
        too_long = np.zeros(256, np.int64)
        too_long[[0x58, 0x59]] = (1, 33)
        cs.append(Case(f"deal-badtid-set-grid{grid}", "deal", "dec", "set", 2, 64,
                       [rec, hexr, {"name": "33 bits", "lens": too_long.astype(np.uint8)}], items=flat,
                       phases=tuple((3 * i) % 16 for i in range(len(flat))), grid=grid, tid=tuple(bad_tid)))
        only0 = [(s, (0 if k is not None else None)) for s, k in flat if k in (0, None)]
        cs.append(Case(f"deal-groups-shared-grid{grid}", "deal", "dec", "shared", 2, 64, [rec], items=only0,
                       phases=tuple((3 * i) % 16 for i in range(len(only0))), grid=grid))
    return cs


def _flip(seg_index, bit):
    def f(b):
        at = int(b["pay_off"][seg_index]) * 8 + bit
        b["payload"][at >> 3] ^= 0x80 >> (at & 7)
        return b
    return f


def _move_sync(seg_index, chunk, d):
    """entry `chunk` moved by d, its neighbour compensating: the sum stays"""
    def f(b):
        so = int(b["sync_off"][seg_index])
        b["sync_len"][so + chunk] = int(b["sync_len"][so + chunk]) + d
        b["sync_len"][so + chunk + 1] = int(b["sync_len"][so + chunk + 1]) - d
        return b
    return f


def _bits_less(seg_index):
    def f(b):
        b["bits"][seg_index] -= 1
        return b
    return f


def _bits_more(seg_index):
    """bits one more than the chunks sum to, where that leaves the padded size as it is"""
    def f(b):
        i = seg_index
        assert pad16((int(b["bits"][i]) + 8) // 8) == int(b["pay_off"][i + 1] - b["pay_off"][i])
        b["bits"][i] += 1
        return b
    return f


def _all(*fns):
    def f(b):
        for fn in fns:
            b = fn(b)
        return b
    return f


def _damage_cases():
    cs = []
    # every segment bad, then the same batch clean, on one context: nothing of a failed call stays
    rec = record("b16")
    its = [(_coded_or_padded(rec, _with_every_length(rec, n, 64, n)), 0) for n in (600, 900, 700, 8300, 500, 300, 200, 100)]
    for mode in ("own", "shared", "set"):
        for what, fn in (("all-bad", _all(*[_move_sync(i, 0, 1) for i in range(len(its))])), ("all-good", None)):
            cs.append(Case(f"damage-b16-{what}-{mode}", "damage", "dec", mode, 2, 64, [rec], items=its, phases=tuple(range(8)),
                           damage=fn))
    for name in ("n3", "b16", "n256"):
        rec = record(name)
        if name == "n256":
            mk = lambda n, seed: fill(rec, n, seed)
        else:
            mk = lambda n, seed, rec=rec: _coded_or_padded(rec, _with_every_length(rec, n, 64, seed))
        items = [(mk(600, 1), 0), (mk(900, 2), 0), (mk(700, 3), 0), (mk(8300, 4), 0), (mk(500, 5), 0)]
        bits1 = int(rec["nbits"][items[1][0]][:64 * 3].sum())   # the start of chunk 3 of segment 1
        plans = {"flip": _flip(1, bits1 + 5), "flip-long": _flip(3, 40), "sync+1": _move_sync(1, 2, 1), "sync-1": _move_sync(1, 2, -1),
                 "bits-1": _bits_less(1), "bits+1": _bits_more(1)}
        if name == "n256":
            # the first digit 200 names a two-digit code: 16 bits where the chunk has 8 left a symbol
            def two_digit(b):
                b["payload"][int(b["pay_off"][1]) + 70] = 200
                b["payload"][int(b["pay_off"][1]) + 71] = 3
                return b
            plans = {"two-digit": two_digit, "bits-1": _bits_less(1)}
        for what, fn in plans.items():
            for mode in ("own", "shared", "set"):
                recs = [rec] if mode != "set" else [make_record(np.zeros(256), rec["n_ary"], "zeros"), rec]
                k = len(recs) - 1
                cs.append(Case(f"damage-{name}-{what}-{mode}", "damage", "dec", mode, rec["n_ary"], 64, recs,
                               items=[(s, k) for s, _ in items], phases=(1, 2, 3, 4, 5), damage=fn))
    # 1-bit codes to a payload of exactly 8 x 128 bits; the last chunk's first bit set makes its codes
    # longer than its bits: the decoder asks for words past the payload, which read as zero
    rec = record("b32")
    x = fill(rec, 1024, 1)
    for what, fn, mid in (("tail", _flip(1, 1024 - 64), x), ("last-bit", _flip(1, 1024 - 1), x),
                          ("bits+1", _bits_more(1), x[:1000]), ("bits-1", _bits_less(1), x[:1000])):   # three short: the wave instance
        for mode in ("own", "shared", "set"):
            recs = [rec] if mode != "set" else [record("f8"), rec]
            cs.append(Case(f"damage-b32-{what}-{mode}", "damage", "dec", mode, 2, 64, recs,
                           items=[(fill(rec, 300, 2), len(recs) - 1), (mid, len(recs) - 1), (fill(rec, 200, 3), len(recs) - 1)],
                           phases=(7, 8, 9), damage=fn))
    return cs


FAMILIES = ("codes", "window", "units", "chunks", "phase", "mode", "deal", "damage")
_MAKERS = {"codes": _codes_cases, "window": _window_cases, "units": _units_cases, "chunks": _chunks_cases,
           "phase": _phase_cases, "mode": _mode_cases, "deal": _deal_cases, "damage": _damage_cases}


@functools.lru_cache(maxsize=None)
def family(name):
    cs = _MAKERS[name]()
    assert len({c.name for c in cs}) == len(cs), name
    return tuple(cs)


def catalogue():
    return tuple(c for f in FAMILIES for c in family(f))


def case(name):
    return next(c for c in catalogue() if c.name == name)
