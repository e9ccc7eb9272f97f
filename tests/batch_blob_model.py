"""A plain model of the "DCHB" container of a Huffman batch (dc_gpu.h "Huffman batch v1: container
DCHB"), written from the format's description alone (TEST INFRASTRUCTURE: numpy and zlib only, no
import of the product).

  layout   the offsets of sections 1 to 7, from count, kind, flags and K
  write    the container of a batch's arrays (those of batch_body_model.expected_batch / hand_batch,
           or the arrays read back from an encode): bytes
  parse    the fields and sections of a container, as they lie (no rule is applied beyond what
           finding the sections takes)
  check    the container rule: DC_OK or DC_E_STREAM
  bound    the bytes that always hold a seal
  derived  pay_off, sync_off and offsets as open derives them from len and bits
"""
import struct
import zlib

import numpy as np

DC_OK, DC_E_ARG, DC_E_CODE_TOO_LONG, DC_E_CAPACITY, DC_E_STREAM = 0, -1, -3, -6, -7
MAGIC = b"DCHB"
HEADER = 64
OWN, OWN4, SHARED, SET = 0, 1, 2, 3
CRC = 1
COUNT_MAX = 1 << 28   # DC_RANGES_MAX
SEG_MAX = 65536       # DC_BATCH_SEG_MAX
SET_MAX = 64          # DC_BATCH_SET_MAX
SYNC_MAX = 1024       # DC_SYNC_MAX
U64 = 1 << 64


def pad16(n):
    return (n + 15) // 16 * 16


def kind_ok(kind, flags, K):
    if kind not in (OWN, OWN4, SHARED, SET) or flags & ~CRC:
        return False
    return K == 0 if kind in (OWN, OWN4) else K == 1 if kind == SHARED else 1 <= K <= SET_MAX


def sync_ok(S):
    return 16 <= S <= SYNC_MAX and S & (S - 1) == 0


def layout(count, kind, flags, K):
    """{"len_off", "bits_off", "mode_off", "tid_off", "crc_off", "rec_off", "rec_bytes",
    "payload_off"} (an absent section: 0), or None for arguments the format does not take."""
    if not 0 <= count <= COUNT_MAX or not kind_ok(kind, flags, K):
        return None
    L, at = {}, HEADER
    for name, size, present in (("len", 4 * count, True), ("bits", 4 * count, True), ("mode", count, True),
                                ("tid", count, kind == SET), ("crc", 4 * count, bool(flags & CRC))):
        L[name + "_off"] = at if present else 0
        at += pad16(size) if present else 0
    L["rec_off"] = at
    L["rec_bytes"] = {OWN: 256 * count, OWN4: 128 * count}.get(kind, 256 * K)
    L["payload_off"] = at + L["rec_bytes"]
    return L


def bound(total_bytes, count, S, kind, flags, K):
    """0 for illegal arguments or a bound that does not fit 64 bits"""
    L = layout(count, kind, flags, K)
    if L is None or not sync_ok(S):
        return 0
    b = L["payload_off"] + pad16(total_bytes + 16 * count) + pad16(2 * (-(-total_bytes // S) + count))
    return b if b < U64 else 0


def lens4(lens):
    """(count x 128 nybble records, ok[count]): a record with a length above 15 is zeros"""
    lens = np.asarray(lens, np.uint8).reshape(-1, 256)
    ok = (lens <= 15).all(axis=1)
    rec = ((lens[:, 0::2] << 4) | (lens[:, 1::2] & 15)).astype(np.uint8)
    rec[~ok] = 0
    return rec, ok


def unpack4(rec):
    rec = np.asarray(rec, np.uint8).reshape(-1, 128)
    out = np.zeros((rec.shape[0], 256), np.uint8)
    out[:, 0::2], out[:, 1::2] = rec >> 4, rec & 15
    return out


def header(kind, flags, K, n_ary, S, count, total_bytes, sync_total, pay_total, blob_bytes):
    h = MAGIC + struct.pack("<BBBBHHIQQQQQI", 1, kind, flags, K, n_ary, S, 0, count, total_bytes, sync_total, pay_total,
                            blob_bytes, 0)
    return h + struct.pack("<I", zlib.crc32(h))


def reseal(blob):
    """the blob with its header CRC made right again (for damage inside the header)"""
    b = bytearray(blob)
    b[60:64] = struct.pack("<I", zlib.crc32(bytes(b[:60])))
    return bytes(b)


def write(arrays, seg_len, kind, flags, n_ary, S, records=None, crc=None):
    """arrays: "mode", "bits", "payload", "pay_off", "sync_len", "sync_off", and "lens" (kinds 0 and
    1) or "tid" (kind 3); seg_len: the segments' byte lengths; records: the K x 256 record section of
    kinds 2 and 3; crc: u32[count] with flag bit 0."""
    seg_len = np.asarray(seg_len, np.int64)
    n = seg_len.size
    K = 0 if kind in (OWN, OWN4) else np.asarray(records).reshape(-1, 256).shape[0]
    L = layout(n, kind, flags, K)
    assert L is not None
    pay_total, sync_total = int(arrays["pay_off"][n]), int(arrays["sync_off"][n])
    sync_at = L["payload_off"] + pay_total
    out = np.zeros(sync_at + pad16(2 * sync_total), np.uint8)

    def put(off, a, dt):
        raw = np.ascontiguousarray(np.asarray(a).astype(dt)).view(np.uint8).reshape(-1)
        out[off: off + raw.size] = raw

    put(L["len_off"], seg_len, "<u4")
    put(L["bits_off"], arrays["bits"], "<u4")
    put(L["mode_off"], arrays["mode"], np.uint8)
    if kind == SET:
        put(L["tid_off"], arrays["tid"], np.uint8)
    if flags & CRC:
        put(L["crc_off"], crc, "<u4")
    if kind == OWN:
        put(L["rec_off"], np.asarray(arrays["lens"]).reshape(-1), np.uint8)
    elif kind == OWN4:
        put(L["rec_off"], lens4(arrays["lens"])[0].reshape(-1), np.uint8)
    else:
        put(L["rec_off"], np.asarray(records).reshape(-1), np.uint8)
    put(L["payload_off"], np.asarray(arrays["payload"])[:pay_total], np.uint8)
    put(sync_at, np.asarray(arrays["sync_len"])[:sync_total], "<u2")
    out[:HEADER] = np.frombuffer(header(kind, flags, K, n_ary, S, n, int(seg_len.sum()), sync_total, pay_total, out.size),
                                 np.uint8)
    return out.tobytes()


def parse_header(blob):
    """the header's fields, whatever they hold (None: fewer than 64 bytes)"""
    if len(blob) < HEADER:
        return None
    f = struct.unpack("<4sBBBBHHIQQQQQII", bytes(blob[:HEADER]))
    names = ("magic", "version", "kind", "flags", "K", "n_ary", "S", "zero12", "count", "total_bytes", "sync_total",
             "pay_total", "blob_bytes", "zero56", "crc")
    return dict(zip(names, f))


def header_ok(blob, m=None):
    """the header rule; the parsed header with its layout, or None"""
    m = len(blob) if m is None else m
    H = parse_header(blob[:HEADER]) if m >= HEADER else None
    if H is None or H["magic"] != MAGIC or H["version"] != 1 or H["crc"] != zlib.crc32(bytes(blob[:60])):
        return None
    if not 2 <= H["n_ary"] <= 256 or not sync_ok(H["S"]) or H["zero12"] or H["zero56"]:
        return None
    L = layout(H["count"], H["kind"], H["flags"], H["K"]) if H["count"] <= COUNT_MAX else None
    if L is None or H["pay_total"] % 16:
        return None
    H.update(L)
    H["sync_off"] = L["payload_off"] + H["pay_total"]
    if H["sync_off"] + pad16(2 * H["sync_total"]) != H["blob_bytes"] or H["blob_bytes"] > m:
        return None
    return H


def parse(blob):
    """The header's fields and the sections as arrays: "len", "bits", "mode", "tid", "crc" (None when
    absent), "records" (rows of 256, or of 128 for kind 1), "payload", "sync_len". The header must
    pass its rule (an AssertionError otherwise): the sections cannot be found without it."""
    H = header_ok(blob)
    assert H is not None, "parse: the header breaks its rule"
    a, n = np.frombuffer(bytes(blob), np.uint8), H["count"]

    def get(off, size, dt):
        return a[off: off + size].view(dt).copy()

    H["len"] = get(H["len_off"], 4 * n, "<u4")
    H["bits"] = get(H["bits_off"], 4 * n, "<u4")
    H["mode"] = get(H["mode_off"], n, np.uint8)
    H["tid"] = get(H["tid_off"], n, np.uint8) if H["kind"] == SET else None
    H["crcs"] = get(H["crc_off"], 4 * n, "<u4") if H["flags"] & CRC else None
    H["records"] = get(H["rec_off"], H["rec_bytes"], np.uint8).reshape(-1, 128 if H["kind"] == OWN4 else 256)
    H["payload"] = get(H["payload_off"], H["pay_total"], np.uint8)
    H["sync_len"] = get(H["sync_off"], 2 * H["sync_total"], "<u2")
    return H


def seg_ok(length, bits, mode, tid, kind, K):
    """the per-segment rule"""
    if length > SEG_MAX or mode > 1 or bits > 8 * length or (mode == 0 and bits != 8 * length):
        return False
    return not (kind == SET and mode == 1 and tid >= K)


def derived(length, bits, S):
    """(offsets, pay_off, sync_off): the exclusive scans of len, round_up_16(ceil(bits / 8)) and
    ceil(len / S), count + 1 entries each"""
    length, bits = np.asarray(length, np.int64), np.asarray(bits, np.int64)
    scan = lambda v: np.concatenate(([0], np.cumsum(v))).astype(np.int64)
    return scan(length), scan(((bits + 7) // 8 + 15) // 16 * 16), scan((length + S - 1) // S)


def seg_status(blob):
    """DC_OK or DC_E_STREAM per segment, as open reports them (the header must pass its rule)"""
    P = parse(blob)
    tid = P["tid"] if P["tid"] is not None else np.zeros(P["count"], np.uint8)
    return np.array([DC_OK if seg_ok(int(l), int(b), int(m), int(t), P["kind"], P["K"]) else DC_E_STREAM
                     for l, b, m, t in zip(P["len"], P["bits"], P["mode"], tid)], np.int32)


def totals_ok(blob):
    P = parse(blob)
    off, po, so = derived(P["len"], P["bits"], P["S"])
    return int(off[-1]) == P["total_bytes"] and int(po[-1]) == P["pay_total"] and int(so[-1]) == P["sync_total"]


def check(blob, m=None):
    """the container rule on the first m bytes of blob: DC_OK or DC_E_STREAM"""
    blob = bytes(blob) if m is None else bytes(blob[:m]) + bytes(max(0, m - len(blob)))
    if header_ok(blob) is None:
        return DC_E_STREAM
    return DC_OK if (seg_status(blob) == DC_OK).all() and totals_ok(blob) else DC_E_STREAM
