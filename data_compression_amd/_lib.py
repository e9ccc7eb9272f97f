"""Loading of the in-tree native libraries (data_compression_amd/lib/*.so).

The libraries link the HIP runtime by soname (libamdhip64.so.7). PyTorch-ROCm ships its
own copy; importing torch first makes every later dlopen resolve to that one copy, so
the kernels and torch share one runtime (device memory, streams, RCCL). Nothing here
falls back to Python or CPU compute: a missing library raises.
"""
from __future__ import annotations

import ctypes as C
import os

try:  # one HIP runtime per process: torch's, when torch is present
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the C-ABI itself
    torch = None

PKG = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(PKG, "lib")

_cache: dict[str, C.CDLL] = {}

vp = C.c_void_p
u8p = C.POINTER(C.c_uint8)
u64 = C.c_uint64
u32 = C.c_uint32
i32 = C.c_int


class HBatch(C.Structure):
    """dc_hbatch (dc_gpu.h): the device arrays of a Huffman batch."""
    _fields_ = [("count", u64), ("n_ary", C.c_int32), ("sync_syms", u32), ("d_lens", vp), ("d_mode", vp),
                ("d_bits", vp), ("d_pay_off", vp), ("d_payload", vp), ("payload_cap", u64), ("d_sync_off", vp),
                ("d_sync_len", vp), ("sync_cap", u64), ("d_status", vp)]


class HBlobInfo(C.Structure):
    """dc_hblob_info (dc_gpu.h "container DCHB"): the header's fields, the section offsets and
    the layout of open's workspace."""
    _fields_ = [(f, u32) for f in ("version", "kind", "flags", "K")] + [("n_ary", C.c_int32), ("sync_syms", u32)] + \
               [(f, u64) for f in ("count", "total_bytes", "sync_total", "pay_total", "blob_bytes", "len_off", "bits_off",
                                   "mode_off", "tid_off", "crc_off", "rec_off", "rec_bytes", "payload_off", "sync_off",
                                   "work_bytes", "w_items", "w_pay_off", "w_sync_off", "w_seg_off", "w_status",
                                   "w_cstatus", "w_lens", "w_lengths", "w_table")]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


class HBlobView(C.Structure):
    """dc_hblob_view: the batch of an opened container and what its decode calls take."""
    _fields_ = [("batch", HBatch), ("d_seg_off", vp), ("d_cstatus", vp), ("d_tid", vp), ("d_crc", vp), ("d_set", vp),
                ("K", u32), ("d_table", vp), ("total_bytes", u64)]


class DcError(RuntimeError):
    NAMES = {-1: "DC_E_ARG", -2: "DC_E_HIP", -3: "DC_E_CODE_TOO_LONG", -4: "DC_E_NOCODE",
             -5: "DC_E_STATE", -6: "DC_E_CAPACITY", -7: "DC_E_STREAM", -8: "DC_E_FALLBACK",
             -9: "DC_E_CHECKSUM"}

    def __init__(self, fn, rc):
        super().__init__(f"{fn} failed: {self.NAMES.get(rc, rc)}")
        self.rc = rc


def check(fn, rc):
    if rc != 0:
        raise DcError(fn, rc)
    return rc


def lib_path(name: str) -> str:
    if name == "libdc_core.so" and os.environ.get("DC_CORE_LIB"):   # diagnostic builds (tools/)
        return os.environ["DC_CORE_LIB"]
    return os.path.join(LIBDIR, name)


def load(name: str) -> C.CDLL:
    if name in _cache:
        return _cache[name]
    path = lib_path(name)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -m data_compression_amd.build` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(path)
    if name == "libdc_core.so":
        _declare_core(lib)
    _cache[name] = lib
    return lib


def core() -> C.CDLL:
    return load("libdc_core.so")


def _declare_core(L):
    P = vp
    sig = {
        "dc_ctx_create": ([C.POINTER(vp), i32, vp], i32),
        "dc_ctx_create_owned": ([C.POINTER(vp), i32], i32),
        "dc_ctx_destroy": ([vp], None),
        "dc_ctx_sync": ([vp], i32),
        "dc_ctx_stream": ([vp], vp),
        "dc_ctx_set_timing": ([vp, i32], i32),
        "dc_ctx_set_option": ([vp, i32, C.c_int64], i32),
        "dc_ctx_timings": ([vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32], i32),
        "dc_version": ([], C.c_char_p),
        "dc_dtable_size": ([], C.c_size_t),
        "dc_malloc": ([C.POINTER(vp), C.c_size_t], i32),
        "dc_free": ([vp], i32),
        "dc_memcpy_h2d": ([vp, vp, vp, C.c_size_t], i32),
        "dc_memcpy_d2h": ([vp, vp, vp, C.c_size_t], i32),
        "dc_memset": ([vp, vp, i32, C.c_size_t], i32),
        "dc_huff_hist": ([vp, P, u64, P], i32),
        "dc_huff_table": ([vp, P, i32, i32, P], i32),
        "dc_huff_table_freq": ([vp, P, i32, i32, P], i32),
        "dc_huff_table_lengths": ([vp, P, i32, i32, P], i32),
        "dc_huff_table_status": ([vp, P, C.POINTER(C.c_int32)], i32),
        "dc_huff_plan": ([vp, P, P], i32),
        "dc_huff_encode_plan": ([vp, P, u64, i32, i32, P, P, P], i32),
        "dc_huff_table_plan": ([vp, P, i32, i32, P, P], i32),
        "dc_huff_table_limit": ([vp, P, i32, i32, i32, P], i32),
        "dc_huff_table_freq_limit": ([vp, P, i32, i32, i32, P], i32),
        "dc_huff_table_plan_limit": ([vp, P, i32, i32, i32, P, P], i32),
        "dc_huff_encode_plan_limit": ([vp, P, u64, i32, i32, i32, P, P, P], i32),
        "dc_huff_limit_classes": ([i32, i32, C.POINTER(u32), u64], i32),
        "dc_small_huff_plan": ([vp, P, u64, i32, i32, P, P, P], i32),
        "dc_small_huff_pack_async": ([vp, P, u64, P, u64, P, u64, P, P, u32], i32),
        "dc_small_huff_symbols": ([vp, C.POINTER(u64)], i32),
        "dc_small_huff_shard_hist": ([vp, P, u64, P, P], i32),
        "dc_small_huff_shard_pack_async": ([vp, P, u64, P, P, P, u64, P, P, P, P, u32], i32),
        "dc_small_huff_decode": ([vp, P, u64, u64, P, P, u32, u64, P, P, P, C.POINTER(u64)], i32),
        "dc_copy_probe": ([vp, P, P, u64], i32),
        "dc_huff_pack": ([vp, P, u64, P, u64, P, u64, P, P, u32], i32),
        "dc_huff_sync_chunks": ([u64, u32], u64),
        "dc_huff_sync_groups": ([u64, u32], u64),
        "dc_huff_words_needed": ([u64, u64], u64),
        "dc_huff_pack_async": ([vp, P, u64, P, u64, P, u64, P, P, u32], i32),
        "dc_huff_pack_async_dev": ([vp, P, u64, P, P, P, u64, P, P, u32], i32),
        "dc_huff_pack_status": ([vp, P], i32),
        "dc_huff_plan_gen": ([vp], u32),
        "dc_huff_pack_status_gen": ([vp, P, u32], i32),
        "dc_huff_plan_offsets": ([vp, P, u64, C.POINTER(u64)], i32),
        "dc_huff_block_hist": ([vp, P, u64], i32),
        "dc_huff_decode": ([vp, P, u64, u64, P, P, u32, u64, P, P], i32),
        "dc_huff_decode_dev": ([vp, P, P, u64, P, P, u32, u64, P, P], i32),
        "dc_huff_decode_ranges": ([vp, P, u64, u64, P, P, u32, u64, P, P, P, P, u64, P, u64], i32),
        "dc_huff_decode_range": ([vp, P, u64, u64, P, P, u32, u64, P, u64, u64, P], i32),
        "dc_huff_decode_status": ([vp], i32),
        "dc_huff_batch_payload_bound": ([u64, u64], u64),
        "dc_huff_batch_sync_bound": ([u64, u64, u32], u64),
        "dc_huff_encode_batch": ([vp, P, P, u64, C.POINTER(HBatch)], i32),
        "dc_huff_encode_batch_limit": ([vp, P, P, u64, i32, C.POINTER(HBatch)], i32),
        "dc_huff_batch_lens_pack": ([vp, P, u64, P, P], i32),
        "dc_huff_batch_lens_unpack": ([vp, P, u64, P], i32),
        "dc_huff_decode_batch": ([vp, C.POINTER(HBatch), P, P, u64], i32),
        "dc_huff_decode_batch_scatter": ([vp, C.POINTER(HBatch), P, P, P, u64], i32),
        "dc_huff_batch_status": ([vp], i32),
        "dc_huff_encode_batch_shared": ([vp, P, P, u64, P, C.POINTER(HBatch)], i32),
        "dc_huff_decode_batch_shared": ([vp, C.POINTER(HBatch), P, P, P, u64], i32),
        "dc_huff_decode_batch_shared_scatter": ([vp, C.POINTER(HBatch), P, P, P, P, u64], i32),
        "dc_huff_table_get_lengths": ([vp, P, C.POINTER(C.c_int32), i32, C.POINTER(i32)], i32),
        "dc_huff_batch_range_chunks": ([u64, u64, u32, C.POINTER(u64), C.POINTER(u64)], i32),
        "dc_huff_batch_range_args": ([u64, u64, u64, u64, u64, u64], i32),
        "dc_huff_decode_batch_ranges": ([vp, C.POINTER(HBatch), P, P, P, P, P, u64, P, u64, P], i32),
        "dc_huff_decode_batch_shared_ranges": ([vp, C.POINTER(HBatch), P, P, P, P, P, P, u64, P, u64, P], i32),
        "dc_huff_batch_set_table_ok": ([P, i32], i32),
        "dc_huff_batch_set_select": ([vp, P, P, u64, i32, P, u32, P, P, P, P], i32),
        "dc_huff_encode_batch_set": ([vp, P, P, u64, P, u32, P, C.POINTER(HBatch)], i32),
        "dc_huff_decode_batch_set": ([vp, C.POINTER(HBatch), P, u32, P, P, P, u64], i32),
        "dc_huff_decode_batch_set_scatter": ([vp, C.POINTER(HBatch), P, u32, P, P, P, P, u64], i32),
        "dc_huff_decode_batch_set_ranges": ([vp, C.POINTER(HBatch), P, u32, P, P, P, P, P, P, u64, P, u64, P], i32),
        "dc_huff_batch_set_hist": ([vp, P, P, u64, P, u32, P], i32),
        "dc_huff_batch_blob_bound": ([u64, u64, u32, i32, i32, u32], u64),
        "dc_huff_batch_blob_layout": ([u64, i32, i32, u32, C.POINTER(HBlobInfo)], i32),
        "dc_huff_batch_blob_info": ([P, u64, C.POINTER(HBlobInfo)], i32),
        "dc_huff_batch_blob_check": ([P, u64], i32),
        "dc_huff_batch_seal": ([vp, C.POINTER(HBatch), P, i32, i32, P, u32, P, P, P, u64, P, P], i32),
        "dc_huff_batch_open": ([vp, P, u64, C.POINTER(HBlobInfo), P, u64, C.POINTER(HBlobView)], i32),
        "dc_huff_decode_redo_count": ([vp, C.POINTER(u64)], i32),
        "dc_huff_base64url": ([vp, P, u64, u64, P], i32),
        "dc_huff_text_bits": ([i32, i32], i32),
        "dc_huff_text": ([vp, P, u64, u64, i32, i32, P, C.POINTER(u64)], i32),
        "dc_huff_text_parse": ([vp, P, u64, i32, i32, u64, P], i32),
        "dc_huff_text_parse_status": ([vp], i32),
        "dc_huff_default_sync": ([u64], u32),
        "dc_huff_choose_sync": ([u64, u64], u32),
        "dc_nyb_compress": ([vp, P, u64, i32, P, C.POINTER(u64)], i32),
        "dc_nyb_decompress": ([vp, P, u64, i32, P, C.POINTER(u64)], i32),
        "dc_nyb_chunked_bound": ([u64, u32], u64),
        "dc_nyb_compress_chunked": ([vp, P, u64, i32, u32, P, u64, C.POINTER(u64)], i32),
        "dc_nyb_chunked_info": ([vp, P, u64, C.POINTER(u64), C.POINTER(i32), C.POINTER(u32)], i32),
        "dc_nyb_decompress_chunked": ([vp, P, u64, P, u64, C.POINTER(u64)], i32),
        "dc_nyb_decompress_batch": ([vp, P, P, u64, i32, P, u64, P, C.POINTER(u64)], i32),
        "dc_nyb_batch_bound": ([u64, u64], u64),
        "dc_nyb_compress_batch": ([vp, P, P, u64, i32, P, u64, P, P], i32),
        "dc_nyb_decompress_batch_async": ([vp, P, P, u64, i32, P, P, u64, P], i32),
        "dc_nyb_mtf_summary": ([vp, P, u64, P, P], i32),
        "dc_nyb_body_plan": ([vp, P, u64, i32, P, P], i32),
        "dc_nyb_body_write": ([vp, P, u64, i32, i32, i32, P, C.POINTER(u64), C.POINTER(i32)], i32),
        "dc_nyb_dbody_plan": ([vp, P, u64, u64, P], i32),
        "dc_nyb_dbody_write": ([vp, P, u64, u64, i32, P, C.POINTER(u64), C.POINTER(i32)], i32),
        "dc_small_compress": ([vp, P, u64, P, C.POINTER(u64)], i32),
        "dc_small_decompress": ([vp, P, u64, P, C.POINTER(u64)], i32),
        "dc_small_batch_bound": ([u64, u64], u64),
        "dc_small_compress_batch": ([vp, P, P, u64, P, u64, P, P], i32),
        "dc_small_decompress_batch": ([vp, P, P, u64, P, P, u64, P], i32),
        "dc_crc32_host": ([u32, vp, C.c_size_t], u32),
        "dc_crc32_combine": ([u32, u32, u64], u32),
        "dc_crc32": ([vp, P, u64, P], i32),
        "dc_crc32_batch": ([vp, P, u64, P, P, u64, P, P], i32),
        "dc_crc32_verify_batch": ([vp, P, u64, P, P, u64, P, P], i32),
        "dc_small_compress_body": ([vp, P, u64, i32, u64, P, C.POINTER(u64)], i32),
        "dc_small_compress_body_plan": ([vp, P, u64, i32, u64, C.POINTER(u64)], i32),
        "dc_small_compress_body_write": ([vp, P, u64, i32, u64, P, C.POINTER(u64)], i32),
        "dc_small_decompress_body": ([vp, P, u64, P, C.POINTER(u64)], i32),
        "dc_host_ctx": ([], vp),
        "dc_huff_compress_bound": ([u64, u32], u64),
        "dc_huff_compress_host": ([u8p, u64, i32, C.POINTER(C.c_int32), i32, u32, u8p, u64, C.POINTER(u64)], i32),
        "dc_huff_decompress_host": ([u8p, u64, u8p, u64, C.POINTER(u64)], i32),
        "dc_huff_netstring_bound": ([u64], u64),
        "dc_huff_compress_netstring": ([u8p, u64, i32, C.POINTER(C.c_int32), i32, u32, u8p, u64, C.POINTER(u64)], i32),
        "dc_huff_decompress_netstring": ([u8p, u64, u8p, u64, C.POINTER(u64)], i32),
        "dc_huff_netstring_info": ([u8p, u64, C.POINTER(u64)], i32),
        "dc_huff_container_info": ([u8p, u64, C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)], i32),
        "dc_huff_container_check": ([u8p, u64], i32),
        "dc_huff_range_span": ([u64, u32, C.POINTER(u64), u64, u64, u64, C.POINTER(u64)], i32),
        "dc_huff_decompress_range_host": ([u8p, u64, u64, u64, u8p, u64, C.POINTER(u64)], i32),
        "dc_huff_batch_compress_host": ([u8p, C.POINTER(u64), u64, i32, u32, i32, i32, i32, u8p, u32, u8p, u64,
                                         C.POINTER(u64)], i32),
        "dc_huff_batch_decompress_host": ([u8p, u64, u8p, u64, C.POINTER(u64), C.POINTER(u64)], i32),
        "dc_nyb_compress_host": ([u8p, u64, i32, u8p, u64, C.POINTER(u64)], i32),
        "dc_nyb_decompress_host": ([u8p, u64, i32, u8p, u64, C.POINTER(u64)], i32),
        "dc_small_compress_host": ([u8p, u64, u8p, u64, C.POINTER(u64)], i32),
        "dc_small_decompress_host": ([u8p, u64, u8p, u64, C.POINTER(u64)], i32),
    }
    for name, (args, res) in sig.items():
        if os.environ.get("DC_CORE_LIB") and not hasattr(L, name):   # older diagnostic build
            continue
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
