"""Device-resident pipelines on torch tensors (HBM) over libdc_core.so.

`Codec` owns one dc_ctx bound to a HIP stream (torch's current stream by default, so
torch.cuda events and synchronisation see the kernels). Stages map 1:1 onto dc_gpu.h:

    hist = c.hist(x)                      # H1  histogram()             n_ary_huffman.c:461
    tab  = c.table(hist, n_ary)           # H2-H6 huffman()+convert()   :1161, :1382
    bits = c.plan(tab)                    # per-block bit counts + scan (:2485 formula)
    c.pack(x, tab, bit_base, words, sync, S)          # H7 encode (build-defined v1)
    c.decode(words, bit_base, sync, S, n, tab, out)   # H8 decode
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import DcError, check, core

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _ptr(t) -> int:
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


class Codec:
    _host_default = None

    def __init__(self, device: int = 0, stream=None, own_stream: bool = False):
        self.L = core()
        self.ctx = C.c_void_p()
        if own_stream:
            check("dc_ctx_create_owned", self.L.dc_ctx_create_owned(C.byref(self.ctx), device))
        else:
            # torch's current stream (its default stream has handle 0 = the HIP NULL stream)
            if stream is not None:
                handle = stream if isinstance(stream, int) else stream.cuda_stream
            elif torch is not None and torch.cuda.is_available():
                handle = torch.cuda.current_stream(device).cuda_stream
            else:
                handle = 0
            check("dc_ctx_create", self.L.dc_ctx_create(C.byref(self.ctx), device, handle or None))
        self.device = device
        self.table_bytes = int(self.L.dc_dtable_size())

    @classmethod
    def host_default(cls):
        if cls._host_default is None:
            cls._host_default = cls(own_stream=True)
        return cls._host_default

    def close(self):
        if self.ctx:
            self.L.dc_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers --------------------------------------------------------------------
    def sync(self):
        check("dc_ctx_sync", self.L.dc_ctx_sync(self.ctx))

    def timing(self, enable: bool):
        check("dc_ctx_set_timing", self.L.dc_ctx_set_timing(self.ctx, int(enable)))

    OPTIONS = {"hist_grid": 1, "pack_grid": 2, "decode_static_pct": 3, "decode_general": 4, "hist_prefetch": 5,
               "decode_variant": 6, "nyb_adec_v1": 7, "pack_block": 8, "nyb_wtile_off": 9, "batch_grid": 10,
               "nyb_adec_seg": 11}

    def set_option(self, name, value: int):
        """dc_ctx_set_option (dc_gpu.h DC_OPT_*): tuning knobs of this context."""
        check("dc_ctx_set_option", self.L.dc_ctx_set_option(self.ctx, self.OPTIONS.get(name, name), int(value)))

    def timings(self, max_n: int = 1024):
        names = (C.c_char_p * max_n)()
        ms = (C.c_float * max_n)()
        n = self.L.dc_ctx_timings(self.ctx, names, ms, max_n)
        if n < 0:
            raise DcError("dc_ctx_timings", n)
        return [(names[i].decode(), float(ms[i])) for i in range(n)]

    def _t(self, nbytes, dtype=None):
        return torch.empty(nbytes, dtype=dtype or torch.uint8, device=f"cuda:{self.device}")

    # ---- Huffman stages ---------------------------------------------------------------
    def hist(self, x, out=None):
        out = out if out is not None else self._t(256, torch.int64)
        check("dc_huff_hist", self.L.dc_huff_hist(self.ctx, _ptr(x), x.numel(), _ptr(out)))
        return out

    @staticmethod
    def max_digits(n_ary: int, max_bits) -> int:
        """The cap of the *_limit calls for a longest code of max_bits bits: max_bits // w digits
        with w = ceil(log2 n_ary) bits a digit; 0 (no cap) for None. ValueError when not even
        one digit fits."""
        if max_bits is None:
            return 0
        w = max(int(n_ary) - 1, 1).bit_length()
        d = int(max_bits) // w
        if d < 1:
            raise ValueError(f"max_bits {max_bits} holds no {w}-bit digit of an n_ary = {n_ary} code")
        return d

    def table(self, hist, n_ary: int, max_symbol_value: int = 258, out=None, max_bits=None):
        """dc_huff_table; with max_bits, dc_huff_table_limit: no code longer than max_bits bits
        (dc_gpu.h "Length-limited tables"; at n_ary 2, 15 keeps every code in the fast decoder's
        table and 12 in the first-level table)."""
        out = out if out is not None else self._t(self.table_bytes)
        if max_bits is not None:
            check("dc_huff_table_limit", self.L.dc_huff_table_limit(
                self.ctx, _ptr(hist), max_symbol_value, n_ary, self.max_digits(n_ary, max_bits), _ptr(out)))
            return out
        check("dc_huff_table", self.L.dc_huff_table(self.ctx, _ptr(hist), max_symbol_value, n_ary, _ptr(out)))
        return out

    def alloc_table(self):
        """An uninitialised device table (dc_dtable bytes), e.g. a broadcast target."""
        return self._t(self.table_bytes)

    def table_freq(self, freq, n_ary: int, max_symbol_value: int, out=None, max_bits=None):
        out = out if out is not None else self._t(self.table_bytes)
        if max_bits is not None:
            check("dc_huff_table_freq_limit", self.L.dc_huff_table_freq_limit(
                self.ctx, _ptr(freq), max_symbol_value, n_ary, self.max_digits(n_ary, max_bits), _ptr(out)))
            return out
        check("dc_huff_table_freq",
              self.L.dc_huff_table_freq(self.ctx, _ptr(freq), max_symbol_value, n_ary, _ptr(out)))
        return out

    def table_lengths(self, lengths, n_ary: int, max_symbol_value: int = 258, out=None):
        out = out if out is not None else self._t(self.table_bytes)
        check("dc_huff_table_lengths",
              self.L.dc_huff_table_lengths(self.ctx, _ptr(lengths), max_symbol_value, n_ary, _ptr(out)))
        return out

    def table_status(self, tab):
        mb = C.c_int32(0)
        st = self.L.dc_huff_table_status(self.ctx, _ptr(tab), C.byref(mb))
        return st, mb.value

    def plan(self, tab, total=None):
        total = total if total is not None else self._t(1, torch.int64)
        check("dc_huff_plan", self.L.dc_huff_plan(self.ctx, _ptr(tab), _ptr(total)))
        self._last_total = total
        return total

    @property
    def fused_plan(self) -> bool:
        """Whether the library has dc_huff_encode_plan (hist + table + plan in one launch)."""
        return hasattr(self.L, "dc_huff_encode_plan")

    def encode_plan(self, x, n_ary: int, max_symbol_value: int = 258, hist=None, table=None, total=None,
                    max_bits=None):
        """hist -> table -> plan in one launch (dc_huff_encode_plan): the histogram kernel's
        last workgroup builds the table and the payload bit count. Returns (hist, table, total).
        With max_bits: dc_huff_encode_plan_limit, two launches, no code longer than max_bits bits."""
        hist = hist if hist is not None else self._t(256, torch.int64)
        table = table if table is not None else self._t(self.table_bytes)
        total = total if total is not None else self._t(1, torch.int64)
        if max_bits is not None:
            check("dc_huff_encode_plan_limit", self.L.dc_huff_encode_plan_limit(
                self.ctx, _ptr(x), x.numel(), max_symbol_value, n_ary, self.max_digits(n_ary, max_bits),
                _ptr(hist), _ptr(table), _ptr(total)))
            self._last_total = total
            return hist, table, total
        check("dc_huff_encode_plan", self.L.dc_huff_encode_plan(self.ctx, _ptr(x), x.numel(), max_symbol_value, n_ary,
                                                                _ptr(hist), _ptr(table), _ptr(total)))
        self._last_total = total
        return hist, table, total

    def table_plan(self, hist, n_ary: int, max_symbol_value: int = 258, out=None, total=None, max_bits=None):
        """table of `hist` + the plan of this context's last hist() under it, one launch
        (dc_huff_table_plan: a shard's encode after the all-reduce). Returns (table, total).
        With max_bits: dc_huff_table_plan_limit, no code longer than max_bits bits."""
        table = out if out is not None else self._t(self.table_bytes)
        total = total if total is not None else self._t(1, torch.int64)
        if max_bits is not None:
            check("dc_huff_table_plan_limit", self.L.dc_huff_table_plan_limit(
                self.ctx, _ptr(hist), max_symbol_value, n_ary, self.max_digits(n_ary, max_bits), _ptr(table),
                _ptr(total)))
            self._last_total = total
            return table, total
        check("dc_huff_table_plan", self.L.dc_huff_table_plan(self.ctx, _ptr(hist), max_symbol_value, n_ary,
                                                              _ptr(table), _ptr(total)))
        self._last_total = total
        return table, total

    def plan_total(self) -> int:
        return int(self._last_total.item())

    def words_needed(self, bit_base: int, total_bits: int) -> int:
        return int(self.L.dc_huff_words_needed(bit_base, total_bits))

    def sync_sizes(self, n: int, sync_syms: int):
        """(groups, chunks) of the sync index for n symbols."""
        return (int(self.L.dc_huff_sync_groups(n, sync_syms)), int(self.L.dc_huff_sync_chunks(n, sync_syms)))

    def alloc_sync(self, n: int, sync_syms: int):
        g, c = self.sync_sizes(n, sync_syms)   # (2 lengths of slack past the view: the kernels add into whole dwords)
        return (self._t(max(g, 1), torch.int64), self._t(max(c, 1) + 2, torch.int16)[: max(c, 1)])

    def pack(self, x, tab, bit_base, words, sync, sync_syms):
        base, lens = sync if sync is not None else (None, None)
        check("dc_huff_pack", self.L.dc_huff_pack(self.ctx, _ptr(x), x.numel(), _ptr(tab), bit_base, _ptr(words),
                                                  words.numel(), _ptr(base), _ptr(lens),
                                                  sync_syms if sync is not None else 0))

    def pack_async(self, x, tab, bit_base, words, sync, sync_syms):
        """bit_base: an int, or a one-element int64 device tensor read by the kernels
        (dc_huff_pack_async_dev: no host read of a gathered offset)."""
        base, lens = sync if sync is not None else (None, None)
        S = sync_syms if sync is not None else 0
        if hasattr(bit_base, "data_ptr"):
            check("dc_huff_pack_async_dev",
                  self.L.dc_huff_pack_async_dev(self.ctx, _ptr(x), x.numel(), _ptr(tab), _ptr(bit_base), _ptr(words),
                                                words.numel(), _ptr(base), _ptr(lens), S))
            return
        check("dc_huff_pack_async",
              self.L.dc_huff_pack_async(self.ctx, _ptr(x), x.numel(), _ptr(tab), bit_base, _ptr(words),
                                        words.numel(), _ptr(base), _ptr(lens), S))

    def pack_status(self, tab, gen=None):
        """Outcome of the last plan + pack (gen=None), or of the plan whose plan_gen() was gen."""
        if gen is None:
            return int(self.L.dc_huff_pack_status(self.ctx, _ptr(tab)))
        return int(self.L.dc_huff_pack_status_gen(self.ctx, _ptr(tab), gen))

    def plan_gen(self) -> int:
        """Identity of the last plan on this context (dc_huff_plan_gen), for pack_status(gen=)."""
        return int(self.L.dc_huff_plan_gen(self.ctx))

    def decode(self, words, bit_base, sync, sync_syms, n, tab, out):
        """bit_base: an int, or a one-element int64 device tensor (dc_huff_decode_dev)."""
        base, lens = sync
        if hasattr(bit_base, "data_ptr"):
            check("dc_huff_decode_dev", self.L.dc_huff_decode_dev(self.ctx, _ptr(words), _ptr(bit_base), words.numel(),
                                                                  _ptr(base), _ptr(lens), sync_syms, n, _ptr(tab),
                                                                  _ptr(out)))
            return
        check("dc_huff_decode", self.L.dc_huff_decode(self.ctx, _ptr(words), bit_base, words.numel(), _ptr(base),
                                                      _ptr(lens), sync_syms, n, _ptr(tab), _ptr(out)))

    def copy_probe(self, src, dst):
        """dc_copy_probe: a float4 device-to-device copy (the HBM reference rate of bench.py)."""
        check("dc_copy_probe", self.L.dc_copy_probe(self.ctx, _ptr(src), _ptr(dst), min(src.numel() * src.element_size(),
                                                                                       dst.numel() * dst.element_size())))

    def decode_status(self):
        return int(self.L.dc_huff_decode_status(self.ctx))

    def decode_redo_count(self) -> int:
        """Chunks of the last S = 64 decode that took the exact redo (diagnostic)."""
        v = C.c_uint64(0)
        check("dc_huff_decode_redo_count", self.L.dc_huff_decode_redo_count(self.ctx, C.byref(v)))
        return int(v.value)

    # ---- small front-end shard bodies (dist.ShardedSmall) --------------------
    def small_body(self, y, left_halo: bool, nelem: int, head: bytes = b"", out=None):
        """Front-end body of stream bytes y[1..nelem] (y[0]: left context; y[nelem+1], when
        present, the right halo) -> uint8 device tensor, after the bytes `head` (written in
        place, no copy of the body). out: optional buffer of >= nelem + len(head) bytes."""
        h = len(head)
        if out is None:
            out = self._t(max(nelem + h, 1))
        elif out.numel() < nelem + h or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("small_body output: contiguous uint8 of >= nelem + len(head) bytes")
        if h:
            out[:h] = torch.tensor(list(head), dtype=torch.uint8, device=out.device)
        n = C.c_uint64(0)
        check("dc_small_compress_body", self.L.dc_small_compress_body(self.ctx, _ptr(y), y.numel(), int(left_halo),
                                                                      nelem, _ptr(out) + h, C.byref(n)))
        return out[: h + n.value]

    def small_body_plan(self, y, left_halo: bool, nelem: int) -> int:
        """Length of small_body(y, left_halo, nelem) without writing it (dc_small_compress_body_plan);
        small_body_write then writes it wherever the caller places it."""
        n = C.c_uint64(0)
        check("dc_small_compress_body_plan", self.L.dc_small_compress_body_plan(self.ctx, _ptr(y), y.numel(),
                                                                                int(left_halo), nelem, C.byref(n)))
        return n.value

    def small_body_write(self, y, left_halo: bool, nelem: int, out, head: bytes = b""):
        """The planned body after `head`, into out (>= len(head) + planned bytes) -> view of out."""
        h = len(head)
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < h:
            raise ValueError("small_body_write output: contiguous uint8")
        if h:
            out[:h] = torch.tensor(list(head), dtype=torch.uint8, device=out.device)
        n = C.c_uint64(0)
        check("dc_small_compress_body_write", self.L.dc_small_compress_body_write(
            self.ctx, _ptr(y), y.numel(), int(left_halo), nelem, _ptr(out) + h, C.byref(n)))
        return out[: h + n.value]

    def _dec_out(self, seg, out):
        if out is None:
            return self._t(max(2 * seg.numel(), 1))
        if out.numel() < 2 * seg.numel() or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("front-end decode output: contiguous uint8 of >= 2 * input bytes")
        return out

    def small_decompress(self, seg, out=None):
        """A front-end stream that starts with its type byte (rank 0's segment). out: an
        optional preallocated buffer of >= 2 * seg.numel() bytes (the result is a view)."""
        out = self._dec_out(seg, out)
        n = C.c_uint64(0)
        check("dc_small_decompress", self.L.dc_small_decompress(self.ctx, _ptr(seg), seg.numel(), _ptr(out),
                                                                C.byref(n)))
        return out[: n.value]

    def small_decompress_body(self, seg, out=None):
        out = self._dec_out(seg, out)
        n = C.c_uint64(0)
        check("dc_small_decompress_body", self.L.dc_small_decompress_body(self.ctx, _ptr(seg), seg.numel(),
                                                                          _ptr(out), C.byref(n)))
        return out[: n.value]

    def small_compress(self, x, out=None):
        """dc_small_compress: the front-end stream of device bytes x (one stream, one host read
        of its length), into `out` when given: at least x.numel() + 64 bytes."""
        if out is None:
            out = self._t(x.numel() + 64)
        elif out.numel() < x.numel() + 64 or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("small_compress output: contiguous uint8 of >= x.numel() + 64 bytes")
        n = C.c_uint64(0)
        check("dc_small_compress", self.L.dc_small_compress(self.ctx, _ptr(x), x.numel(), _ptr(out), C.byref(n)))
        return out[: n.value]

    # ---- byte-stream batch v1: what the small and the nybble batch calls share (dc_gpu.h) ------
    @staticmethod
    def _block_offsets(x, block: int):
        """The offsets of x cut into blocks of `block` bytes (the last shorter), made on the device."""
        n = x.numel()
        off = torch.arange(0, n + block, block, dtype=torch.int64, device=x.device).clamp_(max=n)
        return off[: (n + block - 1) // block + 1].contiguous()

    def _stream_compress_batch(self, name, fn, bound, lead, x, offsets, out, out_cap):
        """fn(ctx, x, offsets, count, *lead, out, cap, out_off, status): the encode of either codec."""
        if x.dtype != torch.uint8 or not x.is_contiguous():
            raise ValueError(f"{name} input: contiguous uint8")
        offsets = self._i64(offsets, range(1, 1 << 62), f"{name} offsets")
        count = offsets.numel() - 1
        if out is None:
            out = self._t(max(bound(x.numel(), count), 1))
        buf = self._u8_out(out, name)
        cap = buf.numel() if out_cap is None else min(int(out_cap), buf.numel())
        out_off = self._t(count + 1, torch.int64) if count else torch.zeros(1, dtype=torch.int64, device=x.device)
        status = self._t(max(count, 1), torch.int32)[:count]
        check(fn.__name__, fn(self.ctx, _ptr(x), _ptr(offsets), count, *lead, _ptr(buf), cap, _ptr(out_off), _ptr(status)))
        return out, out_off, status

    def _stream_decompress_batch(self, name, fn, lead, data, offsets, out_off, out):
        """fn(ctx, data, offsets, count, *lead, out, out_off, cap, status): the decode of either codec."""
        if data.dtype != torch.uint8 or not data.is_contiguous():
            raise ValueError(f"{name} input: contiguous uint8")
        offsets = self._i64(offsets, range(1, 1 << 62), f"{name} offsets")
        count = offsets.numel() - 1
        out_off = self._i64(out_off, (count + 1,), f"{name} out_off")
        if out is None:
            out = self._t(max(int(out_off[-1]), 1))
        buf = self._u8_out(out, name)
        status = self._t(max(count, 1), torch.int32)[:count]
        check(fn.__name__, fn(self.ctx, _ptr(data), _ptr(offsets), count, *lead, _ptr(buf), _ptr(out_off), buf.numel(),
                              _ptr(status)))
        return out, status

    # ---- small batch v1: many buffers, one call each way (dc_gpu.h "small batch v1") -----------
    def small_batch_bound(self, total: int, count: int) -> int:
        """Bytes that always hold the streams of `count` buffers of `total` bytes in all
        (dc_small_batch_bound: total + count, exact)."""
        return int(self.L.dc_small_batch_bound(total, count))

    def small_compress_batch(self, x, offsets, out=None, out_cap: int | None = None):
        """dc_small_compress_batch: buffer i = x[offsets[i]:offsets[i+1]] (device uint8 x, int64
        offsets of count + 1 entries, any alignment, any length) coded as the front-end stream of
        that buffer alone (what small_compress gives for it), the streams back to back in `out`.
        Asynchronous, no host read; the launches do not depend on count or on the lengths.
        out: an optional preallocated uint8 buffer (else small_batch_bound(x.numel(), count)
        bytes); out_cap: a smaller capacity to hand to the kernels. Returns device tensors (out,
        out_off, status): out_off (int64, count + 1) always holds the true stream offsets, status
        (int32) each buffer's outcome; batch_status() gives the lowest failing buffer's."""
        return self._stream_compress_batch("small_compress_batch", self.L.dc_small_compress_batch,
                                           self.small_batch_bound, (), x, offsets, out, out_cap)

    def small_compress_blocks(self, x, block: int, **kw):
        """small_compress_batch of x cut into independent blocks of `block` bytes (the last
        shorter), the offsets made on the device."""
        if block <= 0:
            raise ValueError("small_compress_blocks: block > 0")
        return self.small_compress_batch(x, self._block_offsets(x, block), **kw)

    def small_decompress_batch_into(self, data, offsets, out_off, out=None):
        """dc_small_decompress_batch: stream i = data[offsets[i]:offsets[i+1]] decoded into
        out[out_off[i]:out_off[i+1]] (int64 device tensors or sequences of count + 1 entries; the
        length asked for must be the stream's). Asynchronous, one launch, no host read unless
        `out` is left to default, which reads out_off[-1] once to size it. Returns device tensors
        (out, status); a stream of any status but 0 writes no byte, and no byte outside the asked
        ranges is written. A damaged letter byte still decodes to its length with status 0:
        crc32_verify_batch(out, crc, status, offsets=out_off), with the crc32_batch of the inputs
        taken at encode, turns such a buffer into DC_E_CHECKSUM."""
        return self._stream_decompress_batch("small_decompress_batch_into", self.L.dc_small_decompress_batch, (), data,
                                             offsets, out_off, out)

    # ---- nybble codec, whole streams and shard bodies (dist.ShardedNybble) -----
    def nyb_compress(self, x, modify: bool, out=None):
        """compress_bytestring (nybble_compression.c:887-1038) of device bytes x (into `out`
        when given: at least x.numel() + 2 bytes)."""
        if out is None:
            out = self._t(x.numel() + 2)
        elif out.numel() < x.numel() + 2 or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("nyb_compress output: contiguous uint8 of >= n + 2 bytes")
        n = C.c_uint64(0)
        check("dc_nyb_compress", self.L.dc_nyb_compress(self.ctx, _ptr(x), x.numel(), int(modify), _ptr(out),
                                                        C.byref(n)))
        return out[: n.value]

    def nyb_decompress(self, comp, modify: bool, out=None):
        """decompress_bytestring (nybble_compression.c:734-817) of device bytes comp (into
        `out`, any alignment, when given: at least 2 * comp.numel() bytes)."""
        if out is None:
            out = self._t(max(2 * comp.numel(), 1))
        elif out.numel() < 2 * comp.numel():
            raise ValueError("out holds fewer than 2 * comp.numel() bytes")
        n = C.c_uint64(0)
        check("dc_nyb_decompress", self.L.dc_nyb_decompress(self.ctx, _ptr(comp), comp.numel(), int(modify),
                                                            _ptr(out), C.byref(n)))
        return out[: n.value]

    def nyb_compress_chunked(self, x, modify: bool, chunk: int = 1 << 16):
        """DCNK container: chunks of `chunk` bytes, each the reference stream of that chunk."""
        cap = int(self.L.dc_nyb_chunked_bound(x.numel(), chunk))
        out = self._t(cap)
        n = C.c_uint64(0)
        check("dc_nyb_compress_chunked", self.L.dc_nyb_compress_chunked(self.ctx, _ptr(x), x.numel(), int(modify),
                                                                        chunk, _ptr(out), cap, C.byref(n)))
        return out[: n.value]

    def nyb_decompress_chunked(self, comp):
        n, mod, K = C.c_uint64(0), C.c_int32(0), C.c_uint32(0)
        check("dc_nyb_chunked_info", self.L.dc_nyb_chunked_info(self.ctx, _ptr(comp), comp.numel(), C.byref(n),
                                                                C.byref(mod), C.byref(K)))
        out = self._t(max(n.value, 1))
        got = C.c_uint64(0)
        check("dc_nyb_decompress_chunked", self.L.dc_nyb_decompress_chunked(self.ctx, _ptr(comp), comp.numel(),
                                                                            _ptr(out), n.value, C.byref(got)))
        return out[: got.value]

    def nyb_decompress_batch(self, data, offsets, modify: bool, out_cap: int | None = None):
        """dc_nyb_decompress_batch: streams data[offsets[i]:offsets[i+1]] (device uint8 data,
        device int64 offsets, count + 1 entries) decoded one lane per stream. Returns
        (output bytes, output offsets), both device tensors."""
        count = offsets.numel() - 1
        out_off = self._t(count + 1, torch.int64)
        cap = out_cap if out_cap is not None else 2 * data.numel() + 16
        out = self._t(max(cap, 1))
        tot = C.c_uint64(0)
        check("dc_nyb_decompress_batch", self.L.dc_nyb_decompress_batch(self.ctx, _ptr(data), _ptr(offsets), count,
                                                                        int(modify), _ptr(out), cap, _ptr(out_off),
                                                                        C.byref(tot)))
        return out[: tot.value], out_off

    # ---- nybble batch v1: many buffers, one call each way (dc_gpu.h "nybble batch v1") ---------
    def nyb_batch_bound(self, total: int, count: int) -> int:
        """Bytes that always hold the streams of `count` buffers of `total` bytes in all
        (dc_nyb_batch_bound: total + count, exact)."""
        return int(self.L.dc_nyb_batch_bound(total, count))

    def nyb_compress_batch(self, x, offsets, modify: bool, out=None, out_cap: int | None = None):
        """dc_nyb_compress_batch: buffer i = x[offsets[i]:offsets[i+1]] (device uint8 x, int64
        offsets of count + 1 entries, any alignment, any length) coded as the reference stream of
        that buffer alone (what nyb_compress gives for it), the streams back to back in `out`.
        Asynchronous, no host read; the launches do not depend on count or on the lengths.
        out: an optional preallocated uint8 buffer (else nyb_batch_bound(x.numel(), count) bytes);
        out_cap: a smaller capacity to hand to the kernels. Returns device tensors (out, out_off,
        status): out_off (int64, count + 1) always holds the true stream offsets, status (int32)
        each buffer's outcome; batch_status() gives the lowest failing buffer's.
        The streams carry no checksum: keep crc32_batch(x, offsets=offsets)[0] beside them and
        hand it, with the decode's status, to crc32_verify_batch after nyb_decompress_batch_into."""
        return self._stream_compress_batch("nyb_compress_batch", self.L.dc_nyb_compress_batch, self.nyb_batch_bound,
                                           (int(bool(modify)),), x, offsets, out, out_cap)

    def nyb_compress_blocks(self, x, block: int, modify: bool, **kw):
        """nyb_compress_batch of x cut into independent blocks of `block` bytes (the last
        shorter), the offsets made on the device: the streams and offsets of a DCNK container of
        the same chunk size, without the container."""
        if block <= 0:
            raise ValueError("nyb_compress_blocks: block > 0")
        return self.nyb_compress_batch(x, self._block_offsets(x, block), modify, **kw)

    def nyb_decompress_batch_into(self, data, offsets, modify: bool, out_off, out=None):
        """dc_nyb_decompress_batch_async: stream i = data[offsets[i]:offsets[i+1]] decoded into
        out[out_off[i]:out_off[i+1]] (int64 device tensors or sequences of count + 1 entries; the
        length asked for must be the stream's). Asynchronous, one launch, no host read unless
        `out` is left to default, which reads out_off[-1] once to size it. Returns device tensors
        (out, status); a failed stream's own range holds unspecified bytes, and no byte outside
        the asked ranges is written. A damaged literal byte still decodes to its length with
        status 0: crc32_verify_batch(out, crc, status, offsets=out_off), with the crc32_batch of
        the inputs taken at encode, turns such a buffer into DC_E_CHECKSUM (and skips the streams
        that failed here)."""
        return self._stream_decompress_batch("nyb_decompress_batch_into", self.L.dc_nyb_decompress_batch_async,
                                             (int(bool(modify)),), data, offsets, out_off, out)

    def nyb_mtf_summary(self, y):
        """Move-to-front lists after elements y[1..] from empty lists: (lists[16][8], cnt[16])."""
        lists = np.zeros(128, np.uint8)
        cnt = np.zeros(16, np.uint8)
        check("dc_nyb_mtf_summary", self.L.dc_nyb_mtf_summary(self.ctx, _ptr(y), y.numel(), lists.ctypes.data,
                                                              cnt.ctypes.data))
        return lists.reshape(16, 8), cnt

    def nyb_body_plan(self, y, modify: bool, lists=None):
        """(c0, c1, s0, s1, last_rank) of the shard's elements y[1..] (dc_nyb_body_plan)."""
        plan = np.zeros(5, np.uint64)
        la = np.ascontiguousarray(lists, dtype=np.uint8) if modify else None
        check("dc_nyb_body_plan", self.L.dc_nyb_body_plan(self.ctx, _ptr(y), y.numel(), int(modify),
                                                          la.ctypes.data if modify else None, plan.ctypes.data))
        return [int(v) for v in plan]

    def _headed(self, cap, head):
        out = self._t(max(cap + len(head), 1))
        if head:
            out[: len(head)] = torch.tensor(list(head), dtype=torch.uint8, device=out.device)
        return out

    def nyb_body_write(self, y, modify: bool, pend_rank: int, is_last: bool, head: bytes = b""):
        """Body of the shard's elements y[1..] after the bytes `head` (written in place)."""
        h = len(head)
        out = self._headed(2 * y.numel(), head)
        n = C.c_uint64(0)
        st = C.c_int32(0)
        check("dc_nyb_body_write", self.L.dc_nyb_body_write(self.ctx, _ptr(y), y.numel(), int(modify), pend_rank,
                                                            int(is_last), _ptr(out) + h, C.byref(n), C.byref(st)))
        return out[: h + n.value]

    def nyb_dbody_plan(self, y, m: int):
        plan = np.zeros(4, np.uint64)
        check("dc_nyb_dbody_plan", self.L.dc_nyb_dbody_plan(self.ctx, _ptr(y), y.numel(), m, plan.ctypes.data))
        return [int(v) for v in plan]

    def nyb_dbody_write(self, y, m: int, s_in: int, head: bytes = b""):
        h = len(head)
        out = self._headed(2 * m, head)
        n = C.c_uint64(0)
        st = C.c_int32(0)
        check("dc_nyb_dbody_write", self.L.dc_nyb_dbody_write(self.ctx, _ptr(y), y.numel(), m, s_in, _ptr(out) + h,
                                                              C.byref(n), C.byref(st)))
        return out[: h + n.value]

    # ---- digit text: formats as dc_gpu.h DC_TEXT_* ------------------------
    TEXT_FORMATS = {"base64url": 0, "base16": 1, "digits": 2, "z85": 3, "trits5": 4}

    def text_bits(self, fmt, n_ary: int) -> int:
        """Bits per character of a text format (0: unsupported for this n)."""
        return int(self.L.dc_huff_text_bits(self.TEXT_FORMATS.get(fmt, fmt), n_ary))

    def text(self, words, bit_base: int, bits: int, fmt, n_ary: int):
        """Digit text of bits [bit_base, bit_base+bits) of `words` -> uint8 device tensor."""
        f = self.TEXT_FORMATS.get(fmt, fmt)
        b = self.text_bits(f, n_ary)
        if b == 0:
            raise ValueError(f"text format {fmt} does not support n={n_ary}")
        out = self._t(max((bits + b - 1) // b, 1))
        nc = C.c_uint64(0)
        check("dc_huff_text", self.L.dc_huff_text(self.ctx, _ptr(words), bit_base, bits, f, n_ary, _ptr(out),
                                                  C.byref(nc)))
        return out[: nc.value]

    def text_parse(self, text, fmt, n_ary: int, bits: int):
        """Inverse of text(): uint8 device tensor of characters -> int32 words holding the
        first `bits` bits. Raises DcError on an invalid character."""
        f = self.TEXT_FORMATS.get(fmt, fmt)
        words = self._t(max((bits + 31) // 32, 1), torch.int32)
        check("dc_huff_text_parse", self.L.dc_huff_text_parse(self.ctx, _ptr(text), text.numel(), f, n_ary, bits,
                                                              _ptr(words)))
        check("dc_huff_text_parse_status", self.L.dc_huff_text_parse_status(self.ctx))
        return words

    def default_sync(self, n: int) -> int:
        return int(self.L.dc_huff_default_sync(n))

    def choose_sync(self, n: int, total_bits: int) -> int:
        return int(self.L.dc_huff_choose_sync(n, total_bits))

    def encode(self, x, n_ary: int = 2, sync_syms: int | None = None, bit_base: int = 0, max_bits=None):
        """hist -> table -> plan -> pack on one device. Returns dict of device tensors.
        max_bits: no code longer than that many bits (encode_plan)."""
        n = x.numel()
        if max_bits is not None:
            hist, tab, total = self.encode_plan(x, n_ary, max_bits=max_bits)
        elif hasattr(self.L, "dc_huff_encode_plan"):
            hist, tab, total = self.encode_plan(x, n_ary)
        else:   # an older diagnostic library (tools/, DC_CORE_LIB): the three launches
            hist = self.hist(x)
            tab = self.table(hist, n_ary)
            total = self.plan(tab)
        bits = int(total.item())
        S = sync_syms or self.choose_sync(n, bits)
        words = self._t(self.words_needed(bit_base, bits), torch.int32)
        sync = self.alloc_sync(n, S)
        self.pack(x, tab, bit_base, words, sync, S)
        return {"hist": hist, "table": tab, "bits": bits, "words": words, "sync": sync, "S": S,
                "bit_base": bit_base, "n": n}

    def decode_into(self, enc, out):
        self.decode(enc["words"], enc["bit_base"], enc["sync"], enc["S"], enc["n"], enc["table"], out)

    # ---- random access by the sync index (dc_huff_decode_range / dc_huff_decode_ranges) ----------
    def _range_stream(self, enc):
        if hasattr(enc["bit_base"], "data_ptr"):
            raise ValueError("range decode needs the stream's bit_base as an int (it is device-resident here)")
        base, lens = enc["sync"]
        return (_ptr(enc["words"]), int(enc["bit_base"]), enc["words"].numel(), _ptr(base), _ptr(lens), enc["S"],
                enc["n"], _ptr(enc["table"]))

    @staticmethod
    def _u8_out(out, what):
        if out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError(f"{what} output: contiguous uint8")
        return out

    def _range_lists(self, what, lists, out, out_off):
        """The gather lists of decode_ranges / decode_batch_ranges: `lists` is (name, value) pairs
        ending with count, each an int64 device tensor or a Python sequence; out_off defaults to
        the exclusive cumulative sum of count (computed on the device), out to a new tensor that
        holds every range (sized with one host read unless count is a sequence and out_off the
        default). Returns (device tensors of lists, out_off, out, the buffer out is a view of)."""
        dev = f"cuda:{self.device}"

        def as_dev(v, name):
            if hasattr(v, "data_ptr"):
                if v.dtype != torch.int64 or not v.is_cuda or not v.is_contiguous():
                    raise ValueError(f"{what} {name}: a contiguous int64 device tensor")
                return v
            a = np.ascontiguousarray(v, dtype=np.int64).reshape(-1)
            if a.size and a.min() < 0:
                raise ValueError(f"{what} {name}: non-negative values")
            return torch.from_numpy(a).to(dev)

        names = [n for n, _ in lists]
        count = lists[-1][1]
        total = None   # bytes of a packed output, when the host knows the counts
        if out_off is None and not hasattr(count, "data_ptr"):
            total = int(np.asarray(count, dtype=np.int64).sum())
        tensors = [as_dev(v, n) for n, v in lists]
        count = tensors[-1]
        nr = count.numel()
        if any(t.numel() != nr for t in tensors):
            raise ValueError(f"{what}: {', '.join(names[:-1])} and {names[-1]} differ in length")
        if out_off is None:
            out_off = torch.cumsum(count, 0) - count
        else:
            out_off = as_dev(out_off, "out_off")
            if out_off.numel() != nr:
                raise ValueError(f"{what}: out_off and count differ in length")
        if out is None:
            if total is None:
                total = int((out_off + count).max().item()) if nr else 0
            buf = self._t(max(total, 1))
            out = buf[: max(total, 0)]
        else:
            buf = self._u8_out(out, what)
        return tensors, out_off, out, buf

    def decode_range(self, enc, first: int, count: int, out=None):
        """Symbols [first, first + count) of the stream enc (the dict of encode() /
        small_huff_encode()) -> a uint8 device tensor of count bytes (a view of `out` when
        given: any alignment, >= count bytes). Reads only the chunks the range touches.
        first + count > enc["n"] raises DcError (DC_E_ARG)."""
        stream = self._range_stream(enc)
        first, count = int(first), int(count)
        if first < 0 or count < 0:
            raise ValueError("decode_range: first and count are non-negative")
        if out is None:
            out = self._t(max(count, 1))
        elif self._u8_out(out, "decode_range").numel() < count:
            raise ValueError("decode_range output holds fewer than count bytes")
        check("dc_huff_decode_range", self.L.dc_huff_decode_range(self.ctx, *stream, first, count, _ptr(out)))
        return out[:count]

    def decode_ranges(self, enc, first, count, out=None, out_off=None):
        """Many ranges in one call: range r = symbols [first[r], first[r] + count[r]) of the
        stream enc -> out[out_off[r] ..). first / count / out_off: int64 device tensors (read by
        the kernels: a gather list computed on the GPU is used as it is) or Python sequences.
        out_off defaults to the exclusive cumulative sum of count, computed on the device (the
        ranges packed back to back); out defaults to a new tensor that holds every range (sized
        with one host read unless count is a Python sequence and out_off the default). Returns
        (out, out_off). A range past the stream or past out writes nothing and makes
        decode_status() DC_E_ARG (-1); the other ranges are decoded."""
        stream = self._range_stream(enc)
        (first, count), out_off, out, buf = self._range_lists(
            "decode_ranges", (("first", first), ("count", count)), out, out_off)
        nr = count.numel()
        check("dc_huff_decode_ranges", self.L.dc_huff_decode_ranges(self.ctx, *stream, _ptr(first), _ptr(count),
                                                                    _ptr(out_off), nr, _ptr(buf), out.numel()))
        return out, out_off

    # ---- batched codec: many small buffers, one table each (dc_gpu.h "Huffman batch v1") ---------
    SEG_MAX = 65536   # DC_BATCH_SEG_MAX

    def batch_bounds(self, total_bytes: int, count: int, sync_syms: int):
        """(payload bytes, u16 sync entries) that always hold a batch (dc_huff_batch_*_bound)."""
        return (int(self.L.dc_huff_batch_payload_bound(total_bytes, count)),
                int(self.L.dc_huff_batch_sync_bound(total_bytes, count, sync_syms)))

    @staticmethod
    def _hbatch(enc, payload_cap=None, sync_cap=None):
        from ._lib import HBatch
        pcap = enc["payload"].numel() if payload_cap is None else min(int(payload_cap), enc["payload"].numel())
        scap = enc["sync_len"].numel() if sync_cap is None else min(int(sync_cap), enc["sync_len"].numel())
        return HBatch(enc["count"], enc["n_ary"], enc["S"], _ptr(enc["lens"]), _ptr(enc["mode"]), _ptr(enc["bits"]),
                      _ptr(enc["pay_off"]), _ptr(enc["payload"]), pcap, _ptr(enc["sync_off"]), _ptr(enc["sync_len"]),
                      scap, _ptr(enc["status"]))

    def _i64(self, v, n, name):
        if not hasattr(v, "data_ptr"):
            v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64).reshape(-1)).to(f"cuda:{self.device}")
        if v.dtype != torch.int64 or not v.is_cuda or not v.is_contiguous() or v.numel() not in n:
            raise ValueError(f"{name}: a contiguous int64 device tensor of {' or '.join(map(str, n))} entries")
        return v

    def encode_batch(self, x, offsets, n_ary: int = 2, sync_syms: int = 64, payload=None, sync_len=None,
                     payload_cap=None, sync_cap=None, table=None, max_bits=None, checksum: bool = False, table_set=None):
        """dc_huff_encode_batch: segment i = x[offsets[i]:offsets[i+1]] (device uint8 x, int64
        offsets of count + 1 entries, any alignment, each segment <= 65536 bytes) coded under a
        table of its own, or stored when that is not smaller. Asynchronous, no host read; the
        launches do not depend on count. Returns a dict of device tensors: lens (count x 256
        u8), mode, bits, pay_off, payload, sync_off, sync_len, status (per segment; see
        batch_status()). payload / sync_len: optional preallocated buffers (else sized by
        batch_bounds); payload_cap / sync_cap: smaller caps to hand to the kernels.
        table: a device table (table(), table_lengths(), batch_table()) of the same n_ary that
        codes EVERY segment (dc_huff_encode_batch_shared): no table work per segment and no
        lens record; a segment holding a byte without a code under it is stored. The result
        then carries "table": table and "lens": None.
        max_bits (own tables only): no code of any segment's table longer than that many bits
        (dc_huff_encode_batch_limit); a segment with more distinct bytes than such codes is
        stored under a record of zeros. With table=, the cap belongs to batch_table(): a
        ValueError. The result carries "max_bits".
        checksum (any mode): the result also carries "crc", the CRC-32 of every input segment
        (crc32_batch over the same offsets: one more launch), for decode_batch(verify=True). A
        segment whose offsets decrease has crc 0 and fails the encode anyway. The default
        leaves the call and its result exactly as they are without it.
        table_set: a K x 256 uint8 device tensor of lens records (table_set(), batch_table_set()):
        every segment is coded under the record of the set that costs it the fewest bits among
        those with a code for each of its bytes, the lowest of equal ones
        (dc_huff_encode_batch_set), or stored when none has or none is smaller. No table work
        per segment beyond that choice and no lens record: the result carries "table_set":
        table_set, "tid" (uint8, count: the record of each segment) and "lens": None. Exclusive
        with table= and max_bits= (a ValueError): cap the records where they are made."""
        if x.dtype != torch.uint8 or not x.is_contiguous():
            raise ValueError("encode_batch input: contiguous uint8")
        if table_set is not None:
            if table is not None or max_bits is not None:
                raise ValueError("encode_batch: table_set excludes table= and max_bits= (cap the set's records in table())")
            self._table_set(table_set, "encode_batch")
        if table is not None and max_bits is not None:
            raise ValueError("encode_batch: max_bits caps the per-segment tables; cap a shared table in batch_table()")
        max_digits = self.max_digits(n_ary, max_bits)
        offsets = self._i64(offsets, range(1, 1 << 62), "encode_batch offsets")
        count = offsets.numel() - 1
        pb, sb = self.batch_bounds(x.numel(), count, sync_syms)
        payload = payload if payload is not None else self._t(max(pb, 16))
        sync_len = sync_len if sync_len is not None else self._t(max(sb, 1), torch.int16)
        enc = {"count": count, "n_ary": n_ary, "S": sync_syms, "offsets": offsets, "total": x.numel(),
               "lens": self._t(max(count, 1) * 256).view(max(count, 1), 256)[:count] if table is None and table_set is None else None,
               "mode": self._t(max(count, 1))[:count],
               "bits": self._t(max(count, 1), torch.int32)[:count], "pay_off": self._t(count + 1, torch.int64),
               "payload": payload, "sync_off": self._t(count + 1, torch.int64), "sync_len": sync_len,
               "status": self._t(max(count, 1), torch.int32)[:count], "max_bits": max_bits}
        b = self._hbatch(enc, payload_cap, sync_cap)
        enc["payload_cap"], enc["sync_cap"] = int(b.payload_cap), int(b.sync_cap)
        if checksum:   # (before the encode: batch_status() after the call is the encode's)
            enc["crc"] = self.crc32_batch(x, offsets=offsets)[0]
        if table_set is not None:
            enc["table_set"] = table_set
            enc["tid"] = self._t(max(count, 1))[:count]
            check("dc_huff_encode_batch_set",
                  self.L.dc_huff_encode_batch_set(self.ctx, _ptr(x), _ptr(offsets), count, _ptr(table_set),
                                                  table_set.shape[0], _ptr(enc["tid"]), C.byref(b)))
            return enc
        if table is not None:
            enc["table"] = table
            check("dc_huff_encode_batch_shared",
                  self.L.dc_huff_encode_batch_shared(self.ctx, _ptr(x), _ptr(offsets), count, _ptr(table), C.byref(b)))
            return enc
        if max_bits is not None:
            check("dc_huff_encode_batch_limit",
                  self.L.dc_huff_encode_batch_limit(self.ctx, _ptr(x), _ptr(offsets), count, max_digits, C.byref(b)))
            return enc
        check("dc_huff_encode_batch", self.L.dc_huff_encode_batch(self.ctx, _ptr(x), _ptr(offsets), count, C.byref(b)))
        return enc

    def encode_blocks(self, x, block: int = 65536, **kw):
        """encode_batch of x cut into independent blocks of `block` bytes (the last shorter),
        a table each: the reference's own block design (n_ary_huffman.c:1210-1255); with
        table=..., all under that one table; with table_set=..., each under the cheapest record
        of the set; with max_bits=..., each table capped; with checksum=True, the CRC-32 of every
        block in "crc"."""
        if not 0 < block <= self.SEG_MAX:
            raise ValueError("encode_blocks: 0 < block <= 65536")
        return self.encode_batch(x, self._block_offsets(x, block), **kw)

    def decode_batch(self, enc, out=None, out_off=None, verify: bool = False):
        """dc_huff_decode_batch of the dict encode_batch returned. out_off (int64 device tensor
        or sequence): count + 1 entries put segment i at out[out_off[i]:out_off[i+1]]; count
        entries give each segment's start alone (its length is the encoded segment's), so the
        outputs may lie anywhere in out (dc_huff_decode_batch_scatter). Default: the segments
        back to back from 0. Asynchronous; returns (out, out_off). Per-segment outcome in
        enc["status"], the first failure by batch_status(). A batch encoded under a shared
        table (enc["table"]) is decoded under it (dc_huff_decode_batch_shared), one encoded under a
        table set (enc["table_set"], enc["tid"]) under its records (dc_huff_decode_batch_set).
        verify: after the decode, the CRC-32 of every decoded segment against enc["crc"]
        (encode_batch(checksum=True); a ValueError without it), in either layout: a segment that
        decoded with DC_OK to other bytes than went in (a damaged stored segment, a code
        swapped for another of its length, a wrong table) becomes DC_E_CHECKSUM (-9) in
        enc["status"], and batch_status() answers for the decode and the verify together. One
        more launch (crc32_verify_batch); segments that failed the decode are not read."""
        if verify and enc.get("crc") is None:
            raise ValueError("decode_batch: verify=True needs enc[\"crc\"] (encode_batch(..., checksum=True))")
        count = enc["count"]
        if out_off is None:
            out_off = enc["offsets"] - enc["offsets"][:1]
        out_off = self._i64(out_off, (count, count + 1), "decode_batch out_off")
        if out is None:
            out = self._t(max(enc["total"], 1))[: enc["total"]] if out_off.numel() == count + 1 else None
            if out is None:
                raise ValueError("decode_batch: segment starts alone need an output buffer")
        buf = self._u8_out(out, "decode_batch")
        b = self._hbatch(enc, enc["payload_cap"], enc["sync_cap"])
        tab, mid = self._batch_table_args(enc)
        if out_off.numel() == count + 1:
            fn = "dc_huff_decode_batch" + mid
            check(fn, getattr(self.L, fn)(self.ctx, C.byref(b), *tab, _ptr(buf), _ptr(out_off), buf.numel()))
            if verify:
                self.crc32_verify_batch(buf, enc["crc"], enc["status"], offsets=out_off)
        else:
            end = out_off + (enc["offsets"][1:] - enc["offsets"][:-1])
            fn = "dc_huff_decode_batch" + mid + "_scatter"
            check(fn, getattr(self.L, fn)(self.ctx, C.byref(b), *tab, _ptr(buf), _ptr(out_off), _ptr(end), buf.numel()))
            if verify:
                self.crc32_verify_batch(buf, enc["crc"], enc["status"], beg=out_off, end=end)
        return out, out_off

    def decode_batch_ranges(self, enc, seg, first, count, out=None, out_off=None):
        """Byte ranges of segments in one call (dc_huff_decode_batch_ranges, or
        dc_huff_decode_batch_shared_ranges when enc has a "table", dc_huff_decode_batch_set_ranges
        when it has a "table_set"): range r = bytes [first[r],
        first[r] + count[r]) of segment seg[r] of the dict encode_batch returned -> out[out_off[r]
        ..). seg / first / count / out_off: int64 device tensors (read by the kernels: a gather
        list computed on the GPU is used as it is) or Python sequences. enc["offsets"] gives the
        segment lengths. out_off defaults to the exclusive cumulative sum of count, computed on
        the device (the ranges packed back to back); out defaults to a new tensor that holds every
        range (sized with one host read unless count is a Python sequence and out_off the
        default). Asynchronous, one launch. Returns (out, out_off, status): status[r] (int32,
        device) is range r's outcome, batch_status() the lowest failing range's. A failing range
        writes nothing and never stops the others. Only the chunks a range touches are read and
        verified. There is no checksum here: enc["crc"] is the CRC-32 of whole segments, and a
        part of a segment has none (decode_batch(verify=True) checks whole segments)."""
        (seg, first, count), out_off, out, buf = self._range_lists(
            "decode_batch_ranges", (("seg", seg), ("first", first), ("count", count)), out, out_off)
        nr = count.numel()
        status = self._t(max(nr, 1), torch.int32)[:nr]
        b = self._hbatch(enc, enc["payload_cap"], enc["sync_cap"])
        tab, mid = self._batch_table_args(enc)
        fn = "dc_huff_decode_batch" + mid + "_ranges"
        check(fn, getattr(self.L, fn)(self.ctx, C.byref(b), *tab, _ptr(enc["offsets"]), _ptr(seg), _ptr(first), _ptr(count),
                                      _ptr(out_off), nr, _ptr(buf), out.numel(), _ptr(status)))
        return out, out_off, status

    def batch_lens_pack(self, enc):
        """dc_huff_batch_lens_pack of enc["lens"] (an own-table batch): (lens4, status), a count x
        128 uint8 device tensor (byte j of a record = lens[2j] << 4 | lens[2j + 1]) and an int32
        one. A record holding a length above 15 is written as zeros with DC_E_CODE_TOO_LONG (-3)
        in its status and the lowest such index in batch_status(); none does when the batch was
        encoded under a cap of at most 15 digits. Asynchronous, one launch."""
        lens = enc["lens"]
        if lens is None:
            raise ValueError("batch_lens_pack: a batch under a shared table has no lens records")
        count = enc["count"]
        lens4 = self._t(max(count, 1) * 128).view(max(count, 1), 128)[:count]
        status = self._t(max(count, 1), torch.int32)[:count]
        check("dc_huff_batch_lens_pack",
              self.L.dc_huff_batch_lens_pack(self.ctx, _ptr(lens), count, _ptr(lens4), _ptr(status)))
        return lens4, status

    def batch_lens_unpack(self, lens4):
        """dc_huff_batch_lens_unpack: the count x 256 uint8 lens records of a count x 128 nybble
        tensor, to be put back as enc["lens"] before a decode. Asynchronous, one launch."""
        if lens4.dtype != torch.uint8 or not lens4.is_cuda or not lens4.is_contiguous() or lens4.dim() != 2 \
                or lens4.shape[1] != 128:
            raise ValueError("batch_lens_unpack: a contiguous count x 128 uint8 device tensor")
        count = lens4.shape[0]
        lens = self._t(max(count, 1) * 256).view(max(count, 1), 256)[:count]
        check("dc_huff_batch_lens_unpack", self.L.dc_huff_batch_lens_unpack(self.ctx, _ptr(lens4), count, _ptr(lens)))
        return lens

    def batch_table(self, x, n_ary: int = 2, max_bits=None, cover: bool = False):
        """The table of the whole input x (device uint8): hist plus table, for
        encode_batch(..., table=...). dc_huff_hist wants a 16-B aligned input: a misaligned x is
        cloned. max_bits: no code longer than that many bits (table()). cover: every one of the
        256 byte values gets a code, whether x holds it or not: the histogram's entries are
        raised to at least 1 on the device before the table (a sample then codes any later
        segment; it deepens the tree, so give max_bits with it)."""
        if x.dtype != torch.uint8 or not x.is_contiguous():
            raise ValueError("batch_table input: contiguous uint8")
        if x.data_ptr() & 15:
            x = x.clone()
        hist = self.hist(x)
        if cover:
            hist.clamp_(min=1)
        return self.table(hist, n_ary, max_bits=max_bits)

    # ---- table sets: K tables, each segment under its cheapest (dc_gpu.h "Huffman batch v1, table set") ----
    SET_MAX = 64   # DC_BATCH_SET_MAX

    def _table_set(self, ts, name):
        if not hasattr(ts, "data_ptr") or ts.dtype != torch.uint8 or not ts.is_cuda or not ts.is_contiguous() \
                or ts.dim() != 2 or ts.shape[1] != 256 or not 1 <= ts.shape[0] <= self.SET_MAX:
            raise ValueError(f"{name}: a table set is a contiguous K x 256 uint8 device tensor, 1 <= K <= {self.SET_MAX}")
        return ts

    @staticmethod
    def _batch_table_args(enc):
        """What a decode call takes between the batch and its output, and the part of its name
        that says so: nothing (own tables), the shared table, or the set, K and tid."""
        if enc.get("table_set") is not None:
            ts = enc["table_set"]
            return (_ptr(ts), ts.shape[0], _ptr(enc["tid"])), "_set"
        if enc.get("table") is not None:
            return (_ptr(enc["table"]),), "_shared"
        return (), ""

    def table_set(self, records, n_ary: int):
        """A table set for encode_batch(..., table_set=): the K x 256 uint8 device tensor of the K
        records, each either an array of code lengths in digits (its first 256 entries are used;
        what table_get_lengths returns, or a row of enc["lens"]) or a device table of that n_ary
        (read back through table_get_lengths). ValueError for K outside 1..64. A record that is
        no code at n_ary (dc_huff_batch_set_table_ok) is legal: no segment chooses it."""
        records = list(records)
        if not 1 <= len(records) <= self.SET_MAX:
            raise ValueError(f"table_set: 1 <= K <= {self.SET_MAX} records, not {len(records)}")
        if not 2 <= int(n_ary) <= 256:
            raise ValueError("table_set: 2 <= n_ary <= 256")
        rows = np.zeros((len(records), 256), np.uint8)
        for k, r in enumerate(records):
            if hasattr(r, "data_ptr") and r.is_cuda and r.dtype == torch.uint8 and r.numel() == self.table_bytes:
                r = self.table_get_lengths(r)
            elif hasattr(r, "data_ptr"):
                r = r.cpu().numpy()
            r = np.asarray(r).reshape(-1)[:256]
            if r.size and (r.min() < 0 or r.max() > 255):
                raise ValueError(f"table_set: record {k} holds a length outside 0..255")
            rows[k, : r.size] = r
        return torch.from_numpy(rows).to(f"cuda:{self.device}")

    def batch_set_select(self, x, offsets, ts, n_ary: int = 2):
        """dc_huff_batch_set_select: (tid, mode, bits, status), device tensors of count entries
        (uint8, uint8, int32, int32), exactly what encode_batch(x, offsets, n_ary, table_set=ts)
        puts in its result under those names, and nothing else: the plan alone, one launch,
        asynchronous. sum(ceil(bits / 8) rounded up to 16) sizes the payload before an encode."""
        if x.dtype != torch.uint8 or not x.is_contiguous():
            raise ValueError("batch_set_select input: contiguous uint8")
        self._table_set(ts, "batch_set_select")
        offsets = self._i64(offsets, range(1, 1 << 62), "batch_set_select offsets")
        count = offsets.numel() - 1
        tid, mode = self._t(max(count, 1))[:count], self._t(max(count, 1))[:count]
        bits, status = self._t(max(count, 1), torch.int32)[:count], self._t(max(count, 1), torch.int32)[:count]
        check("dc_huff_batch_set_select",
              self.L.dc_huff_batch_set_select(self.ctx, _ptr(x), _ptr(offsets), count, n_ary, _ptr(ts), ts.shape[0],
                                              _ptr(tid), _ptr(mode), _ptr(bits), _ptr(status)))
        return tid, mode, bits, status

    def batch_set_hist(self, x, offsets, tid, K: int):
        """dc_huff_batch_set_hist: the int64 K x 256 device tensor whose row k counts the bytes of
        the segments with tid[i] == k (tid: uint8 device tensor of count entries); segments with
        tid[i] >= K or bad offsets are skipped. One launch, asynchronous."""
        if x.dtype != torch.uint8 or not x.is_contiguous():
            raise ValueError("batch_set_hist input: contiguous uint8")
        if not 1 <= K <= self.SET_MAX:
            raise ValueError(f"batch_set_hist: 1 <= K <= {self.SET_MAX}")
        offsets = self._i64(offsets, range(1, 1 << 62), "batch_set_hist offsets")
        count = offsets.numel() - 1
        if tid.dtype != torch.uint8 or not tid.is_cuda or not tid.is_contiguous() or tid.numel() != count:
            raise ValueError("batch_set_hist tid: a contiguous uint8 device tensor of count entries")
        hist = self._t(K * 256, torch.int64).view(K, 256)
        check("dc_huff_batch_set_hist",
              self.L.dc_huff_batch_set_hist(self.ctx, _ptr(x), _ptr(offsets), count, _ptr(tid), K, _ptr(hist)))
        return hist

    def batch_table_set(self, x, offsets, k: int, n_ary: int = 2, max_bits=12, iters: int = 2):
        """Train a table set of k records on the segments x[offsets[i]:offsets[i+1]] (k-means on
        code cost): the K x 256 uint8 device tensor for encode_batch(..., table_set=). Reads the
        device between its steps: a call for set-up time, not for the hot path.
        Record 0 is batch_table(x, n_ary, max_bits, cover=True): it has a code for every byte
        value, is never replaced, and so makes every segment codable. Records 1..k-1 start from
        the histograms of k - 1 contiguous runs of segments (segment i in run i (k - 1) // count),
        then `iters` times: every segment selects its record (batch_set_select), the histogram of
        each record's segments is taken (batch_set_hist), and records 1..k-1 become the tables of
        theirs (table(hist, max_bits=)); a record no segment chose becomes 256 zeros.
        Guaranteed: with record 0 in the set, no segment takes more bits than under record 0
        alone, so the batch is never larger than encode_batch(table=record 0)'s, whatever the
        other records are. Not guaranteed: that a further round makes the batch smaller (a
        record is refitted to the segments that chose it, and bytes only the others hold lose
        their codes), or that k records beat k - 1. Deterministic: the same input gives the same set."""
        if not 1 <= k <= self.SET_MAX:
            raise ValueError(f"batch_table_set: 1 <= k <= {self.SET_MAX}")
        if x.dtype != torch.uint8 or not x.is_contiguous():
            raise ValueError("batch_table_set input: contiguous uint8")
        offsets = self._i64(offsets, range(1, 1 << 62), "batch_table_set offsets")
        count = offsets.numel() - 1
        rows = np.zeros((k, 256), np.uint8)
        rows[0] = self.table_get_lengths(self.batch_table(x, n_ary, max_bits, cover=True))[:256]
        if k == 1 or count == 0:
            return torch.from_numpy(rows).to(f"cuda:{self.device}")

        def refit(tid):   # records 1..k-1 from the histograms of their segments
            hist = self.batch_set_hist(x, offsets, tid, k)
            filled = (hist.sum(dim=1) > 0).cpu().numpy()
            for j in range(1, k):
                rows[j] = self.table_get_lengths(self.table(hist[j], n_ary, max_bits=max_bits))[:256] if filled[j] else 0
            return torch.from_numpy(rows).to(f"cuda:{self.device}")

        i = torch.arange(count, dtype=torch.int64, device=f"cuda:{self.device}")
        ts = refit((1 + i * (k - 1) // count).to(torch.uint8))
        for _ in range(iters):
            ts = refit(self.batch_set_select(x, offsets, ts, n_ary)[0])
        return ts

    def table_get_lengths(self, tab):
        """dc_huff_table_get_lengths: the table's lengths in digits, entries 0 ..
        max_symbol_value, as a numpy int32 array (what table_lengths takes back). Synchronising."""
        buf = np.zeros(1024, np.int32)   # DC_MAX_SYMS
        n = C.c_int(0)
        check("dc_huff_table_get_lengths", self.L.dc_huff_table_get_lengths(
            self.ctx, _ptr(tab), buf.ctypes.data_as(C.POINTER(C.c_int32)), buf.size, C.byref(n)))
        return buf[: n.value].copy()

    def batch_status(self) -> int:
        """0, or the status of the lowest-numbered failing segment of the last batch call on this
        codec (encode_batch with or without max_bits, batch_lens_pack, decode_batch,
        decode_batch_ranges, nyb_compress_batch,
        nyb_decompress_batch_into, small_compress_batch, small_decompress_batch_into, crc32_batch,
        crc32_verify_batch: after a verify, the carried-over decode failures included),
        synchronising."""
        return int(self.L.dc_huff_batch_status(self.ctx))

    # ---- the storable form of a batch (dc_gpu.h "Huffman batch v1: container DCHB") ---------------
    BLOB_OWN, BLOB_OWN4, BLOB_SHARED, BLOB_SET = 0, 1, 2, 3   # the header's kind
    BLOB_CRC = 1                                              # flag bit 0

    @staticmethod
    def _blob_kind(enc, lens4: bool = False):
        """(kind, flags, K, tables) of the dict encode_batch returned."""
        flags = Codec.BLOB_CRC if enc.get("crc") is not None else 0
        if enc.get("table_set") is not None:
            return Codec.BLOB_SET, flags, int(enc["table_set"].shape[0]), enc["table_set"]
        if enc.get("table") is not None:
            return Codec.BLOB_SHARED, flags, 1, enc["table"]
        return (Codec.BLOB_OWN4 if lens4 else Codec.BLOB_OWN), flags, 0, None

    def batch_blob_bound(self, total_bytes: int, count: int, sync_syms: int, kind: int = 0, flags: int = 0, K: int = 0) -> int:
        """dc_huff_batch_blob_bound: bytes that always hold a sealed batch. ValueError for
        arguments the format does not take."""
        b = int(self.L.dc_huff_batch_blob_bound(total_bytes, count, sync_syms, kind, flags, K))
        if b == 0:
            raise ValueError("batch_blob_bound: count, sync_syms, kind, flags or K outside the DCHB format")
        return b

    def batch_blob_layout(self, count: int, kind: int = 0, flags: int = 0, K: int = 0) -> dict:
        """dc_huff_batch_blob_layout: the section offsets the host knows before an encode
        (payload_off among them), as a dict of ints."""
        from ._lib import HBlobInfo
        info = HBlobInfo()
        check("dc_huff_batch_blob_layout", self.L.dc_huff_batch_blob_layout(count, kind, flags, K, C.byref(info)))
        return info.as_dict()

    def batch_seal(self, enc, out=None, lens4: bool = False):
        """dc_huff_batch_seal of the dict encode_batch returned: (blob, info, status). blob: a
        uint8 device tensor (out, or a new one of batch_blob_bound bytes) whose first info[0]
        bytes are the container; info: an int64 device tensor, (blob_bytes, container status: 0,
        DC_E_CAPACITY when out is too small, DC_E_ARG for a shared table that cannot be stored);
        status: int32 per segment (the encode's for a segment it failed, which is sealed empty;
        DC_E_CODE_TOO_LONG for a record that has no nybble form). The kind (own tables, shared
        table, table set), tid, crc and the table or set are taken from enc; lens4: own tables as
        128-byte nybble records. The payload is not copied when enc["payload"] already lies at
        out[payload_off:] (encode_batch_blob). Asynchronous, no host read."""
        kind, flags, K, tables = self._blob_kind(enc, lens4)
        count = enc["count"]
        if out is None:
            out = self._t(self.batch_blob_bound(enc["total"], count, enc["S"], kind, flags, K))
        if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.data_ptr() & 15:
            raise ValueError("batch_seal out: a contiguous, 16-B aligned uint8 device tensor")
        info = self._t(2, torch.int64)
        status = self._t(max(count, 1), torch.int32)[:count]
        b = self._hbatch(enc, enc["payload_cap"], enc["sync_cap"])
        check("dc_huff_batch_seal",
              self.L.dc_huff_batch_seal(self.ctx, C.byref(b), _ptr(enc["offsets"]), kind, flags, _ptr(tables), K,
                                        _ptr(enc.get("tid")), _ptr(enc.get("crc")), _ptr(out), out.numel(), _ptr(info),
                                        _ptr(status)))
        return out, info, status

    def encode_batch_blob(self, x, offsets, lens4: bool = False, **kw):
        """encode_batch(x, offsets, **kw) straight into a container: the blob is allocated at its
        bound, the encoder writes the payload at blob[payload_off:] (the offsets up to there depend
        on count and the mode alone), and batch_seal adds the directory, the sync index and the
        header: the payload is never copied. Returns batch_seal's (blob, info, status).
        Asynchronous, no host read."""
        offsets = self._i64(offsets, range(1, 1 << 62), "encode_batch_blob offsets")
        count = offsets.numel() - 1
        ts = kw.get("table_set")
        kind = self.BLOB_SET if ts is not None else self.BLOB_SHARED if kw.get("table") is not None else \
            self.BLOB_OWN4 if lens4 else self.BLOB_OWN
        flags = self.BLOB_CRC if kw.get("checksum") else 0
        K = int(ts.shape[0]) if kind == self.BLOB_SET else 1 if kind == self.BLOB_SHARED else 0
        S = kw.get("sync_syms", 64)
        blob = self._t(self.batch_blob_bound(x.numel(), count, S, kind, flags, K))
        at = self.batch_blob_layout(count, kind, flags, K)["payload_off"]
        pb = self.batch_bounds(x.numel(), count, S)[0]
        if flags and count and x.numel() == 0:
            # an input of no bytes has no address for crc32_batch to take; every segment it can hold
            # is empty, and the CRC-32 of no bytes is 0
            enc = self.encode_batch(x, offsets, payload=blob[at: at + pb], **dict(kw, checksum=False))
            enc["crc"] = self._t(count, torch.int32).zero_().view(torch.uint32)
        else:
            enc = self.encode_batch(x, offsets, payload=blob[at: at + pb], **kw)
        return self.batch_seal(enc, out=blob, lens4=lens4)

    def batch_info(self, blob) -> dict:
        """dc_huff_batch_blob_info of a container (device tensor, bytes or numpy): the header's
        fields and the section offsets as a dict of ints; a device tensor costs one 64-byte copy.
        DcError (DC_E_STREAM) for a header that breaks the rule of the format."""
        from ._lib import HBlobInfo
        if hasattr(blob, "data_ptr"):
            head, m = blob[:64].cpu().numpy().tobytes(), blob.numel()
        else:
            blob = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else \
                np.ascontiguousarray(blob, np.uint8).reshape(-1)
            head, m = blob[:64].tobytes(), blob.size
        info = HBlobInfo()
        buf = C.create_string_buffer(head, 64)
        check("dc_huff_batch_blob_info", self.L.dc_huff_batch_blob_info(C.cast(buf, C.c_void_p), m, C.byref(info)))
        return info.as_dict()

    def batch_open(self, blob):
        """dc_huff_batch_open: a container (a uint8 device tensor, or bytes / numpy, which are
        uploaded) as a dict that decode_batch, decode_batch_ranges and decode_batch(verify=True)
        accept as they accept encode_batch's: mode, bits, payload, sync_len (and lens of kind 0,
        tid and table_set of kind 3, crc) are views into the blob; pay_off, sync_off, offsets,
        status (and kind 1's unpacked lens, kind 2's rebuilt table) lie in one workspace tensor.
        Also "total", "info" (batch_info's dict) and "container_status" (an int32 device tensor of
        one entry: 0, or DC_E_STREAM when the directory's scans do not end at the header's totals;
        "status" has DC_E_STREAM for each segment that breaks its own rule). DcError (DC_E_STREAM)
        for a header that breaks the rule. One 64-byte read of a device blob, then asynchronous."""
        from ._lib import HBlobInfo, HBlobView
        if not hasattr(blob, "data_ptr"):
            host = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else \
                np.ascontiguousarray(blob, np.uint8).reshape(-1)
            dev = self._t(max(host.size, 1))[: host.size]
            dev.copy_(torch.from_numpy(host.copy()))
            head, blob = host[:64].tobytes(), dev
        else:
            if blob.dtype != torch.uint8 or not blob.is_cuda or not blob.is_contiguous():
                raise ValueError("batch_open: a contiguous uint8 device tensor, bytes or numpy")
            if blob.data_ptr() & 15:
                blob = blob.clone()
            head = blob[:64].cpu().numpy().tobytes()
        m = blob.numel()
        info = HBlobInfo()
        hbuf = C.create_string_buffer(head, 64)
        check("dc_huff_batch_blob_info", self.L.dc_huff_batch_blob_info(C.cast(hbuf, C.c_void_p), m, C.byref(info)))
        I = info.as_dict()
        work = self._t(max(I["work_bytes"], 256))
        view = HBlobView()
        check("dc_huff_batch_open",
              self.L.dc_huff_batch_open(self.ctx, _ptr(blob), m, C.byref(info), _ptr(work), work.numel(), C.byref(view)))
        n, kind = I["count"], I["kind"]

        def part(t, off, nbytes, dtype=None):
            v = t[off: off + nbytes]
            return v if dtype is None else v.view(dtype)

        enc = {"count": n, "n_ary": I["n_ary"], "S": I["sync_syms"], "total": I["total_bytes"], "max_bits": None,
               "offsets": part(work, I["w_seg_off"], 8 * (n + 1), torch.int64),
               "mode": part(blob, I["mode_off"], n), "bits": part(blob, I["bits_off"], 4 * n, torch.int32),
               "pay_off": part(work, I["w_pay_off"], 8 * (n + 1), torch.int64),
               "payload": part(blob, I["payload_off"], I["pay_total"]),
               "sync_off": part(work, I["w_sync_off"], 8 * (n + 1), torch.int64),
               "sync_len": part(blob, I["sync_off"], 2 * I["sync_total"], torch.int16),
               "status": part(work, I["w_status"], 4 * n, torch.int32),
               "container_status": part(work, I["w_cstatus"], 4, torch.int32),
               "payload_cap": I["pay_total"], "sync_cap": I["sync_total"], "lens": None,
               "info": I, "blob": blob, "work": work}
        if kind == self.BLOB_OWN:
            enc["lens"] = part(blob, I["rec_off"], 256 * n).view(n, 256)
        elif kind == self.BLOB_OWN4:
            enc["lens"] = part(work, I["w_lens"], 256 * n).view(n, 256)
        elif kind == self.BLOB_SHARED:
            enc["table"] = part(work, I["w_table"], self.table_bytes)
        else:
            enc["table_set"] = part(blob, I["rec_off"], 256 * I["K"]).view(I["K"], 256)
            enc["tid"] = part(blob, I["tid_off"], n)
        if I["flags"] & self.BLOB_CRC:
            enc["crc"] = part(blob, I["crc_off"], 4 * n, torch.uint32)
        return enc

    # ---- checksums: CRC-32 per buffer (dc_gpu.h "checksums") -----------------------------------
    CRC_TILE = 1024       # DC_CRC_TILE: the bytes a wave takes at a time
    CRC_PIECE = 131072    # DC_CRC_PIECE: dc_crc32's bytes per wave
    E_CHECKSUM = -9       # DC_E_CHECKSUM

    def _crc_in(self, x, name):
        if x.dtype != torch.uint8 or not x.is_cuda or not x.is_contiguous():
            raise ValueError(f"{name} input: a contiguous uint8 device tensor")
        return x

    def _crc_lists(self, name, offsets, beg, end):
        """(beg, end, count, keep): the two u64 device arrays of a buffer list, given as one
        offsets array of count + 1 entries (passed as off and off + 1) or as two of count."""
        if (offsets is None) == (beg is None and end is None) or (beg is None) != (end is None):
            raise ValueError(f"{name}: either offsets (count + 1 entries) or beg and end (count entries each)")
        if offsets is not None:
            off = self._i64(offsets, range(1, 1 << 62), f"{name} offsets")
            return off.data_ptr(), off.data_ptr() + 8, off.numel() - 1, (off,)
        beg = self._i64(beg, range(0, 1 << 62), f"{name} beg")
        end = self._i64(end, (beg.numel(),), f"{name} end")
        return beg.data_ptr(), end.data_ptr(), beg.numel(), (beg, end)

    def crc32(self, x):
        """dc_crc32: the CRC-32 (zlib's) of the device uint8 tensor x, any size and alignment,
        spread over the whole device. Returns a one-element uint32 device tensor. Asynchronous,
        no host read, two launches."""
        x = self._crc_in(x, "crc32")
        out = self._t(1, torch.uint32)
        check("dc_crc32", self.L.dc_crc32(self.ctx, _ptr(x), x.numel(), _ptr(out)))
        return out

    def crc32_batch(self, x, offsets=None, beg=None, end=None):
        """dc_crc32_batch: the CRC-32 of every buffer x[beg[i]:end[i]] (int64 device tensors or
        sequences of count entries each; any order, overlaps and gaps) or x[offsets[i]:
        offsets[i+1]] (count + 1 entries). Returns device tensors (crc, status): uint32 and
        int32, count entries each; a buffer with end < beg (DC_E_ARG) or end > x.numel()
        (DC_E_CAPACITY) is not read and has crc 0; batch_status() gives the lowest failing
        buffer's status. Asynchronous, one launch, no host read."""
        x = self._crc_in(x, "crc32_batch")
        pb, pe, count, keep = self._crc_lists("crc32_batch", offsets, beg, end)
        crc = self._t(max(count, 1), torch.uint32)[:count]
        status = self._t(max(count, 1), torch.int32)[:count]
        check("dc_crc32_batch", self.L.dc_crc32_batch(self.ctx, _ptr(x), x.numel(), pb, pe, count, _ptr(crc), _ptr(status)))
        return crc, status

    def crc32_verify_batch(self, x, expect, status=None, offsets=None, beg=None, end=None):
        """dc_crc32_verify_batch: the buffers of x (listed as in crc32_batch) against expect (a
        uint32 device tensor of count entries, e.g. what crc32_batch gave for the inputs before
        they were encoded). status (int32 device tensor, count entries) is in-out, so the
        status a decode call returned can be handed straight on: an entry that is nonzero keeps
        its value and its buffer is not read; an entry that is 0 becomes DC_E_ARG /
        DC_E_CAPACITY for a bad range and DC_E_CHECKSUM (-9) when the buffer's CRC-32 is not
        expect[i]. A fresh zero array is used when none is given. Returns status;
        batch_status() then answers for the decode and the verify together. Asynchronous, one
        launch, no host read."""
        x = self._crc_in(x, "crc32_verify_batch")
        pb, pe, count, keep = self._crc_lists("crc32_verify_batch", offsets, beg, end)
        if expect.dtype != torch.uint32 or not expect.is_cuda or not expect.is_contiguous() or expect.numel() != count:
            raise ValueError(f"crc32_verify_batch expect: a contiguous uint32 device tensor of {count} entries")
        if status is None:
            status = torch.zeros(count, dtype=torch.int32, device=x.device)
        elif status.dtype != torch.int32 or not status.is_cuda or not status.is_contiguous() or status.numel() != count:
            raise ValueError(f"crc32_verify_batch status: a contiguous int32 device tensor of {count} entries")
        check("dc_crc32_verify_batch", self.L.dc_crc32_verify_batch(self.ctx, _ptr(x), x.numel(), pb, pe, count,
                                                                    _ptr(expect), _ptr(status)))
        return status

    # ---- C5 fused front-end encode (small_compression.c front-end, then Huffman; one pass) -----
    def small_huff_plan(self, x, n_ary: int = 16, max_symbol_value: int = 258, hist=None, table=None, total=None):
        """dc_small_huff_plan: histogram of the front-end output of x (never written), table and
        plan total in one launch. Returns (hist, table, total); DcError DC_E_FALLBACK for n < 2."""
        hist = hist if hist is not None else self._t(256, torch.int64)
        table = table if table is not None else self._t(self.table_bytes)
        total = total if total is not None else self._t(1, torch.int64)
        check("dc_small_huff_plan", self.L.dc_small_huff_plan(self.ctx, _ptr(x), x.numel(), max_symbol_value, n_ary,
                                                              _ptr(hist), _ptr(table), _ptr(total)))
        self._last_total = total
        return hist, table, total

    def small_huff_pack_async(self, x, tab, bit_base, words, sync, sync_syms):
        base, lens = sync
        check("dc_small_huff_pack_async",
              self.L.dc_small_huff_pack_async(self.ctx, _ptr(x), x.numel(), _ptr(tab), bit_base, _ptr(words),
                                              words.numel(), _ptr(base), _ptr(lens), sync_syms))

    # ---- the same for one shard of the stream (dist.ShardedSmall at world > 1) -------------
    def small_shard_hist(self, x, shard, hist=None):
        """dc_small_huff_shard_hist: the histogram of the shard's front-end output; shard = the
        4 int64 of FeShard on the device (global bit, first symbol, byte before, byte after)."""
        hist = hist if hist is not None else self._t(256, torch.int64)
        check("dc_small_huff_shard_hist", self.L.dc_small_huff_shard_hist(self.ctx, _ptr(x), x.numel(), _ptr(shard),
                                                                          _ptr(hist)))
        return hist

    def small_shard_pack_async(self, x, tab, shard, words, sync, gsync, sync_syms):
        """dc_small_huff_shard_pack_async: codes at the global bit shard[0], the local sync index
        into sync, this shard's part of the stream's sync index into gsync."""
        base, lens = sync
        gbase, glens = gsync
        check("dc_small_huff_shard_pack_async",
              self.L.dc_small_huff_shard_pack_async(self.ctx, _ptr(x), x.numel(), _ptr(tab), _ptr(shard), _ptr(words),
                                                    words.numel(), _ptr(base), _ptr(lens), _ptr(gbase), _ptr(glens),
                                                    sync_syms))

    def small_huff_symbols(self) -> int:
        v = C.c_uint64(0)
        check("dc_small_huff_symbols", self.L.dc_small_huff_symbols(self.ctx, C.byref(v)))
        return int(v.value)

    def small_huff_encode(self, x, n_ary: int = 16, sync_syms: int = 64, bit_base: int = 0, words=None, sync=None):
        """The C5 encode of device bytes x: the front-end (small_compression.c:582-665) and the
        n-ary Huffman code of its output M in one pass over x, M never written. Returns the
        dict of encode() for M ("n" = symbols of M) with "fused": True, bit-identical to
        small_compress + encode. When the fused path does not apply (DC_E_FALLBACK: LITERAL
        output, every byte value present in M, an over-long block) the two stages run and
        "fused" is False. words / sync: optional preallocated buffers (sync for n + 1 symbols)."""
        n = x.numel()
        try:
            hist, tab, total = self.small_huff_plan(x, n_ary)
        except DcError as e:
            if e.rc != -8:
                raise
            return self._small_huff_two_stage(x, n_ary, sync_syms, bit_base)
        bits = int(total.item())
        need = self.words_needed(bit_base, bits)
        if words is None or words.numel() < need:
            words = self._t(need, torch.int32)
        sync = sync if sync is not None else self.alloc_sync(n + 1, sync_syms)
        self.small_huff_pack_async(x, tab, bit_base, words, sync, sync_syms)
        st = self.pack_status(tab)
        if st == -8:
            return self._small_huff_two_stage(x, n_ary, sync_syms, bit_base)
        check("dc_small_huff_pack_async", st)
        m = self.small_huff_symbols()
        ng, nch = self.sync_sizes(m, sync_syms)   # the index of m symbols (the buffers hold n + 1)
        return {"hist": hist, "table": tab, "bits": bits, "words": words, "S": sync_syms, "bit_base": bit_base,
                "sync": (sync[0][: max(ng, 1)], sync[1][: max(nch, 1)]), "n": m, "fused": True}

    def _small_huff_two_stage(self, x, n_ary, sync_syms, bit_base):
        fe = self._t(x.numel() + 64)
        m = C.c_uint64(0)
        check("dc_small_compress", self.L.dc_small_compress(self.ctx, _ptr(x), x.numel(), _ptr(fe), C.byref(m)))
        enc = self.encode(fe[: m.value], n_ary=n_ary, sync_syms=sync_syms, bit_base=bit_base)
        enc["fused"] = False
        return enc

    def small_huff_decode(self, enc, out=None, mbuf=None):
        """Huffman decode of M, then the front-end inverse (dc_small_huff_decode: the inverse
        takes the decoder's per-group counts instead of a counting pass of its own): the input
        bytes, a view of out (>= 2 * enc["n"] bytes) when given. mbuf: optional buffer for M."""
        m = enc["n"]
        mbuf = mbuf if mbuf is not None else self._t(max(m, 1) + 16)
        out = self._dec_out(mbuf[: m], out)
        n = C.c_uint64(0)
        base, lens = enc["sync"]
        bb = enc["bit_base"]
        if hasattr(bb, "data_ptr"):   # (device-resident offset: the two stages)
            self.decode(enc["words"], bb, enc["sync"], enc["S"], m, enc["table"], mbuf)
            return self.small_decompress(mbuf[: m], out=out)
        check("dc_small_huff_decode", self.L.dc_small_huff_decode(
            self.ctx, _ptr(enc["words"]), bb, enc["words"].numel(), _ptr(base), _ptr(lens), enc["S"], m,
            _ptr(enc["table"]), _ptr(mbuf), _ptr(out), C.byref(n)))
        return out[: n.value]

    # ---- allocation helpers (the engine interface used by dist.ShardedHuffman) -----------
    def alloc_words(self, bit_base: int, bits: int):
        return self._t(self.words_needed(bit_base, bits), torch.int32)

    def alloc_bytes(self, n: int):
        return self._t(max(n, 1))

    # ---- host helpers -------------------------------------------------------------------
    def histogram_host(self, x: np.ndarray, max_symbol_value: int = 258) -> np.ndarray:
        from ._lib import vp
        n = x.size
        d_in = C.c_void_p()
        d_h = C.c_void_p()
        check("dc_malloc", self.L.dc_malloc(C.byref(d_in), n + 64))
        check("dc_malloc", self.L.dc_malloc(C.byref(d_h), 256 * 8))
        try:
            if n:
                check("h2d", self.L.dc_memcpy_h2d(self.ctx, d_in, x.ctypes.data_as(vp), n))
            check("dc_huff_hist", self.L.dc_huff_hist(self.ctx, d_in, n, d_h))
            h = np.zeros(256, dtype=np.uint64)
            check("d2h", self.L.dc_memcpy_d2h(self.ctx, h.ctypes.data_as(vp), d_h, 256 * 8))
        finally:
            self.L.dc_free(d_in)
            self.L.dc_free(d_h)
        out = np.zeros(max_symbol_value + 1, dtype=np.int64)
        k = min(256, max_symbol_value + 1)
        out[:k] = h[:k].astype(np.int64)
        return out
