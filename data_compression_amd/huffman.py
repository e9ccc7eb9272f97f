"""Python mirror of n_ary_huffman.c's public interface, calling libdc_huffman.so (the
drop-in C-ABI) -- same names, argument meaning and array conventions as the reference
(n_ary_huffman.c:461-493, :1161-1208, :1382-1612, :1621-1678), so the parity tests read
like the reference's own tests. Every call runs the gfx950 kernels of libdc_core.so.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import DcError, core, load

_L = None


def lib():
    global _L
    if _L is None:
        _L = load("libdc_huffman.so")
        ip = C.POINTER(C.c_int)
        _L.histogram.argtypes = [C.c_char_p, C.c_int, ip]
        _L.histogram.restype = None
        _L.huffman.argtypes = [C.c_int, ip, C.c_int, ip]
        _L.huffman.restype = None
        _L.convert_lengths_to_encode_table.argtypes = [C.c_int, ip, C.c_int, ip, C.POINTER(C.c_uint)]
        _L.convert_lengths_to_encode_table.restype = None
        _L.represent_items_with_codes.argtypes = [C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                                  C.c_int, C.c_char_p]
        _L.represent_items_with_codes.restype = C.c_int
        _L.dc_huff_compress.argtypes = [C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
        _L.dc_huff_compress.restype = C.c_int
        _L.dc_huff_decompress.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p]
        _L.dc_huff_decompress.restype = C.c_int
    return _L


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def histogram(text: bytes, max_symbol_value: int = 258) -> np.ndarray:
    """histogram(text, max_symbol_value, h) -- counts up to the first NUL."""
    h = np.zeros(max_symbol_value + 1, dtype=np.int32)
    lib().histogram(bytes(text), max_symbol_value, _ip(h))
    return h


def huffman(max_leaf_value: int, symbol_frequencies, compressed_symbols: int) -> np.ndarray:
    f = np.zeros(max_leaf_value + 1, dtype=np.int32)
    src = np.asarray(symbol_frequencies, dtype=np.int64)[: max_leaf_value + 1]
    f[: len(src)] = src
    out = np.zeros(max_leaf_value + 1, dtype=np.int32)
    lib().huffman(max_leaf_value, _ip(f), compressed_symbols, _ip(out))
    return out


def convert_lengths_to_encode_table(max_symbol_value: int, canonical_lengths, compressed_symbols: int,
                                    encode_length_table=None, encode_value_table=None, size=None):
    """Returns (encode_length_table, encode_value_table). Pass pre-filled arrays to see
    which entries the function leaves untouched (index max_symbol_value, :1421)."""
    size = size or (max_symbol_value + 1)
    L = np.zeros(size, dtype=np.int32)
    src = np.asarray(canonical_lengths, dtype=np.int32)
    L[: len(src)] = src
    el = np.zeros(size, np.int32) if encode_length_table is None else np.array(encode_length_table, np.int32)
    ev = np.zeros(size, np.uint32) if encode_value_table is None else np.array(encode_value_table, np.uint32)
    lib().convert_lengths_to_encode_table(max_symbol_value, _ip(L), compressed_symbols, _ip(el),
                                          ev.ctypes.data_as(C.POINTER(C.c_uint)))
    return el, ev


def represent_items_with_codes(max_symbol_value: int, canonical_lengths, compressed_symbols: int,
                               original_text: bytes, start: int = 0, bufsize: int | None = None):
    """Returns (count, compressed_text bytes [start:start+count]) or (-1, b"")."""
    L = np.zeros(max_symbol_value + 1, dtype=np.int32)
    src = np.asarray(canonical_lengths, dtype=np.int32)
    L[: len(src)] = src
    n = len(original_text)
    if bufsize is None:
        bufsize = start + (n * 32 + 5) // 6 + 8
    out = C.create_string_buffer(bufsize + 1)
    txt = C.create_string_buffer(bytes(original_text), n + 1)
    r = lib().represent_items_with_codes(max_symbol_value, _ip(L), compressed_symbols, bufsize, n, txt,
                                         start, out)
    if r < 0:
        return r, b""
    return r, out.raw[start : start + r]


def compress(data: bytes, n_ary: int = 2, lengths=None, max_symbol_value: int = 258) -> bytes:
    """dc_huff_compress (same parameters as the reference's static compress,
    n_ary_huffman.c:1688) -> netstring blocks (raw, or #dc1 + X + #dcidx + Z).
    lengths None: the input's own Huffman lengths (histogram -> huffman on the GPU)."""
    data = bytes(data)
    n = len(data)
    if lengths is None:
        lengths = huffman(max_symbol_value, histogram_bytes(data, max_symbol_value), n_ary)
    L = np.zeros(max_symbol_value + 1, dtype=np.int32)
    L[: len(lengths)] = np.asarray(lengths, dtype=np.int32)
    cap = int(core().dc_huff_netstring_bound(n)) + 1
    out = C.create_string_buffer(cap)
    r = lib().dc_huff_compress(max_symbol_value, _ip(L), n_ary, cap - 1, n, C.create_string_buffer(data, n + 1), out)
    if r < 0:
        raise DcError("dc_huff_compress", r)
    return out.raw[:r]


def compress_dch1(data: bytes, n_ary: int = 2, sync_syms: int = 0) -> bytes:
    """The binary "DCH1" container (dc_huff_compress_host; dc_host.h)."""
    data = bytes(data)
    n = len(data)
    cap = int(core().dc_huff_compress_bound(n, sync_syms))
    out = (C.c_uint8 * cap)()
    got = C.c_uint64(0)
    src = (C.c_uint8 * max(n, 1)).from_buffer_copy(data + b"\0")
    rc = core().dc_huff_compress_host(src, n, n_ary, None, 258, sync_syms, out, cap, C.byref(got))
    if rc:
        raise DcError("dc_huff_compress_host", rc)
    return bytes(out[: got.value])


def decompress(blob: bytes, max_decompressed_size: int | None = None) -> bytes:
    """dc_huff_decompress: a netstring container (this build's or the reference compress()'s
    raw blocks) or a DCH1 container."""
    blob = bytes(blob)
    if max_decompressed_size is None:
        nn = C.c_uint64(0)
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        rc = core().dc_huff_container_info(buf, len(blob), C.byref(nn), None, None)
        if rc:
            raise DcError("dc_huff_container_info", rc)
        max_decompressed_size = int(nn.value)
    out = C.create_string_buffer(max_decompressed_size + 1)
    r = lib().dc_huff_decompress(len(blob), blob, max_decompressed_size, out)
    if r < 0:
        raise DcError("dc_huff_decompress", r)
    return out.raw[:r]


def range_span(n: int, sync_syms: int, sync_base, end_bit: int, first: int, count: int):
    """dc_huff_range_span (pure host arithmetic, no device): the part of a stream that symbols
    [first, first + count) need, as (g0, g1, first payload bit, end payload bit). sync_base:
    the stream's u64 group bases; end_bit: bit_base + payload bits."""
    base = np.ascontiguousarray(sync_base, dtype=np.uint64)
    out = (C.c_uint64 * 4)()
    rc = core().dc_huff_range_span(n, sync_syms, base.ctypes.data_as(C.POINTER(C.c_uint64)), end_bit, first, count,
                                   out)
    if rc:
        raise DcError("dc_huff_range_span", rc)
    return tuple(int(v) for v in out)


def decompress_range(blob: bytes, first: int, count: int) -> bytes:
    """dc_huff_decompress_range_host: bytes [first, first + count) of what a DCH1 container
    holds, uploading only the index entries and payload bytes of the groups the range touches.
    A netstring container (no binary index) or a range past the end raises DcError (DC_E_ARG)."""
    if not isinstance(blob, bytes):
        blob = bytes(blob)
    buf = C.cast(C.c_char_p(blob), C.POINTER(C.c_uint8))   # read in place: no copy of the container
    out = (C.c_uint8 * max(count, 1))()
    got = C.c_uint64(0)
    rc = core().dc_huff_decompress_range_host(buf, len(blob), first, count, out, count, C.byref(got))
    if rc:
        raise DcError("dc_huff_decompress_range_host", rc)
    return bytes(out[: got.value])


def compress_batch(buffers, n_ary: int = 2, sync_syms: int = 64, mode: str = "own", max_bits=None, checksum: bool = True,
                   lens4: bool = False, k: int = 4) -> bytes:
    """Many small buffers (each at most 65536 bytes) into one "DCHB" container (dc_gpu.h
    "container DCHB"), by dc_huff_batch_compress_host: what to write to a file.
    mode "own": a table per buffer; max_bits caps them. lens4 stores them as 128-byte nybble
    records, which hold lengths up to 15: max_bits then defaults to 15, and a larger one raises
    DcError (DC_E_CODE_TOO_LONG) for a buffer whose table is deeper.
    mode "shared": one table, built on the device from all the bytes (capped at max_bits).
    mode "set": k tables trained on the buffers (Codec.batch_table_set; max_bits 12 by default).
    checksum: a CRC-32 per buffer is stored, and verified by decompress_batch.
    A buffer that cannot be encoded raises DcError with its status."""
    from .device import Codec
    if mode not in ("own", "shared", "set"):
        raise ValueError("compress_batch mode: own, shared or set")
    bufs = [bytes(b) for b in buffers]
    data = b"".join(bufs)
    off = np.concatenate(([0], np.cumsum([len(b) for b in bufs]))).astype(np.uint64)
    kind = {"own": 1 if lens4 else 0, "shared": 2, "set": 3}[mode]
    if kind == 1 and max_bits is None:
        max_bits = 15
    records, K = None, 0
    if mode == "set":
        import torch
        c = Codec()
        try:
            x = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(f"cuda:{c.device}")
            ts = c.batch_table_set(x, off.astype(np.int64), k, n_ary, **({} if max_bits is None else {"max_bits": max_bits}))
            records = np.ascontiguousarray(ts.cpu().numpy(), np.uint8)
        finally:
            c.close()
        K = records.shape[0]
    cap = int(core().dc_huff_batch_blob_bound(len(data), len(bufs), sync_syms, kind, int(bool(checksum)), K or (kind == 2)))
    if cap == 0:
        raise ValueError("compress_batch: sync_syms or the number of buffers is outside the DCHB format")
    out = (C.c_uint8 * cap)()
    got = C.c_uint64(0)
    src = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data + b"\0")
    rc = core().dc_huff_batch_compress_host(
        src, off.ctypes.data_as(C.POINTER(C.c_uint64)), len(bufs), n_ary, sync_syms, kind, int(bool(checksum)),
        Codec.max_digits(n_ary, max_bits), None if records is None else records.ctypes.data_as(C.POINTER(C.c_uint8)), K,
        out, cap, C.byref(got))
    if rc:
        raise DcError("dc_huff_batch_compress_host", rc)
    return bytes(out[: got.value])


def batch_info(blob) -> dict:
    """dc_huff_batch_blob_check, then dc_huff_batch_blob_info, of a container in host memory
    (pure host, no device): the header's fields and section offsets. DcError (DC_E_STREAM) for a
    blob that breaks the container rule."""
    from ._lib import HBlobInfo
    blob = bytes(blob)
    buf = C.cast(C.c_char_p(blob), C.c_void_p)
    rc = core().dc_huff_batch_blob_check(buf, len(blob))
    if rc:
        raise DcError("dc_huff_batch_blob_check", rc)
    info = HBlobInfo()
    rc = core().dc_huff_batch_blob_info(buf, len(blob), C.byref(info))
    if rc:
        raise DcError("dc_huff_batch_blob_info", rc)
    return info.as_dict()


def decompress_batch(blob) -> list:
    """The buffers of a "DCHB" container, as a list of bytes, by dc_huff_batch_decompress_host:
    the container rule is checked on the host before the first device call; stored CRCs are
    verified. DcError with the status of the first failing buffer (DC_E_STREAM, DC_E_CHECKSUM)
    when one does not decode."""
    blob = bytes(blob)
    info = batch_info(blob)
    n, total = info["count"], info["total_bytes"]
    out = (C.c_uint8 * max(total, 1))()
    off = (C.c_uint64 * (n + 1))()
    count = C.c_uint64(0)
    src = C.cast(C.c_char_p(blob), C.POINTER(C.c_uint8))
    rc = core().dc_huff_batch_decompress_host(src, len(blob), out, total, off, C.byref(count))
    if rc:
        raise DcError("dc_huff_batch_decompress_host", rc)
    data = bytes(out[:total])
    return [data[off[i]: off[i + 1]] for i in range(n)]


def histogram_bytes(data: bytes, max_symbol_value: int = 258) -> np.ndarray:
    """Histogram of an arbitrary byte string (NULs included), via the device API."""
    from .device import Codec
    c = Codec.host_default()
    return c.histogram_host(np.frombuffer(bytes(data), dtype=np.uint8), max_symbol_value)
