"""The "DCHB" container of a Huffman batch (dc_gpu.h "Huffman batch v1: container DCHB") without a
device: the model of tests/batch_blob_model.py round-trips its own containers; the library's pure
host calls (dc_huff_batch_blob_check / _info / _layout / _bound: csrc/dc_batch_blob.h as the
library compiles it) agree with the model over a catalogue of containers the device never wrote
(batch_body_model.hand_batch streams) and over each of them damaged field by field; the bound
holds every container; the entry points are exported and declared; and the header's own check
under the host sanitizers (tests/c/batch_blob_check.c) builds and passes.
container(), CPU_CATALOGUE and header_damage / directory_damage are shared with
tests/test_gpu_batch_blob.py."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import batch_blob_model as M
from tests import batch_body_model as BB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dc_huff_batch_blob_bound", "dc_huff_batch_blob_layout", "dc_huff_batch_blob_info",
                "dc_huff_batch_blob_check", "dc_huff_batch_seal", "dc_huff_batch_open",
                "dc_huff_batch_compress_host", "dc_huff_batch_decompress_host")
RECORDS = {2: ("b12", "b16"), 3: ("n3",), 16: ("n16",), 256: ("n256",)}
KINDS = (M.OWN, M.OWN4, M.SHARED, M.SET)


def _lib():
    from data_compression_amd._lib import core
    return core()


def records_of(kind, n_ary):
    """the records a container of this kind is coded under: one for kind 2, all of RECORDS[n_ary]
    otherwise (kind 1 wants lengths of at most 15 digits: b12 alone at n = 2)"""
    names = RECORDS[n_ary][:1] if kind in (M.SHARED, M.OWN4) else RECORDS[n_ary]
    return [BB.record(n) for n in names]


def container(kind, flags, n_ary, S, seg_lens, seed=0, stored_every=3):
    """A container the device never wrote: segment i of seg_lens[i] bytes, every stored_every-th one
    uniform random and stored, the others of a record's shortest codes and coded under it
    (hand_batch: coded up to bits == 8 len). Returns {"blob", "arrays", "seg_len", "segs", "records"
    (K x 256 u8, or None), "recs" (the record dicts), "crc", "kind", "flags", "n_ary", "S"}."""
    recs = records_of(kind, n_ary)
    rng = np.random.default_rng(seed)
    items = []
    for i, n in enumerate(seg_lens):
        if n == 0 or i % stored_every == stored_every - 1:
            items.append((rng.integers(0, 256, n, dtype=np.uint8), None))
        else:
            k = i % len(recs)
            items.append((BB.fill(recs[k], n, seed=seed + i), k))
    mode = "own" if kind in (M.OWN, M.OWN4) else "shared" if kind == M.SHARED else "set"
    arrays = BB.hand_batch(mode, items, n_ary, S, recs)
    segs = arrays["segs"]
    crc = np.array([zlib.crc32(s.tobytes()) for s in segs], np.uint32) if flags & M.CRC else None
    rows = None if kind in (M.OWN, M.OWN4) else np.stack([r["lens"] for r in recs]).astype(np.uint8)
    blob = M.write(arrays, [s.size for s in segs], kind, flags, n_ary, S, records=rows, crc=crc)
    return {"blob": blob, "arrays": arrays, "seg_len": np.array([s.size for s in segs], np.int64), "segs": segs,
            "records": rows, "recs": recs, "crc": crc, "kind": kind, "flags": flags, "n_ary": n_ary, "S": S}


def _cycle(count, S):
    edge = (0, 1, S - 1, S, S + 1, 100)
    return [edge[i % len(edge)] for i in range(count)]


def cpu_catalogue():
    """(name, kind, flags, n_ary, S, seg_lens): counts either side of 16 for every kind and flag,
    every arity and sync size once, the long lengths once, a count past the scan's 1024 threads"""
    out = []
    for kind in KINDS:
        for flags in (0, M.CRC):
            for count in (0, 1, 2, 15, 16, 17):
                out.append((f"k{kind}f{flags}c{count}", kind, flags, 2, 64, _cycle(count, 64)))
    for n_ary in (3, 16, 256):
        out.append((f"n{n_ary}", M.SET, M.CRC, n_ary, 16, _cycle(9, 16)))
    out.append(("S1024", M.OWN, 0, 2, 1024, _cycle(7, 1024)))
    out.append(("long", M.SHARED, M.CRC, 2, 64, [4095, 4096, 65536, 0, 65536]))
    out.append(("c1025", M.OWN4, 0, 2, 16, [i % 4 for i in range(1025)]))
    return out


CPU_CATALOGUE = cpu_catalogue()


@pytest.fixture(scope="module")
def built():
    return {name: container(kind, flags, n_ary, S, lens, seed=11) for name, kind, flags, n_ary, S, lens in CPU_CATALOGUE}


def lib_check(blob, m=None):
    b = bytes(blob)
    return _lib().dc_huff_batch_blob_check(C.cast(C.c_char_p(b), C.c_void_p), len(b) if m is None else m)


def lib_info(blob, m=None):
    from data_compression_amd._lib import HBlobInfo
    b = bytes(blob[:64])
    info = HBlobInfo()
    rc = _lib().dc_huff_batch_blob_info(C.cast(C.c_char_p(b), C.c_void_p), len(blob) if m is None else m, C.byref(info))
    return rc, info.as_dict()


def _set(blob, at, fmt, value, reseal=False):
    b = bytearray(blob)
    b[at: at + struct.calcsize(fmt)] = struct.pack(fmt, value)
    return M.reseal(b) if reseal else bytes(b)


def header_damage(c):
    """(name, blob, m) for every header field of the issue, each on the container c, the header CRC
    made right again except where the CRC itself is the damage"""
    blob, H = c["blob"], M.parse_header(c["blob"])
    m = len(blob)
    return [
        ("magic", _set(blob, 0, "<B", ord("E"), True), m),
        ("version2", _set(blob, 4, "<B", 2, True), m),
        ("kind4", _set(blob, 5, "<B", 4, True), m),
        ("flag_bit1", _set(blob, 6, "<B", H["flags"] | 2, True), m),
        ("K0", _set(blob, 7, "<B", 0 if H["kind"] >= M.SHARED else 1, True), m),   # (kinds 0 and 1: K must be 0)
        ("n_ary1", _set(blob, 8, "<H", 1, True), m),
        ("S48", _set(blob, 10, "<H", 48, True), m),
        ("count_max", _set(blob, 16, "<Q", M.COUNT_MAX + 1, True), m),
        ("pay_total+8", _set(blob, 40, "<Q", H["pay_total"] + 8, True), m),
        ("blob_bytes+1", _set(blob, 48, "<Q", H["blob_bytes"] + 1, True), m),
        ("blob_bytes-1", _set(blob, 48, "<Q", H["blob_bytes"] - 1, True), m),
        ("m-1", blob, m - 1),
        ("crc_bit", _set(blob, 60, "<I", H["crc"] ^ (1 << 9)), m),
    ]


def directory_damage(c, i):
    """(name, blob) for every directory field of the issue at segment i (a coded segment of len > 1)"""
    blob, P = c["blob"], M.parse(c["blob"])
    ln, bits = int(P["len"][i]), int(P["bits"][i])
    out = [("len+1", _set(blob, P["len_off"] + 4 * i, "<I", ln + 1)),
           ("len65537", _set(blob, P["len_off"] + 4 * i, "<I", 65537)),
           ("bits+1", _set(blob, P["bits_off"] + 4 * i, "<I", bits + 1)),
           ("bits-1", _set(blob, P["bits_off"] + 4 * i, "<I", bits - 1)),
           ("mode2", _set(blob, P["mode_off"] + i, "<B", 2))]
    if c["kind"] == M.SET:
        out.append(("tidK", _set(blob, P["tid_off"] + i, "<B", P["K"])))
    return out


def test_entry_points_are_exported_and_declared():
    L = _lib()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes is not None, name
    assert L.dc_huff_batch_blob_bound.restype is C.c_uint64 and len(L.dc_huff_batch_blob_bound.argtypes) == 6
    assert len(L.dc_huff_batch_seal.argtypes) == 13 and len(L.dc_huff_batch_open.argtypes) == 7
    from data_compression_amd import huffman
    from data_compression_amd.device import Codec
    for name in ("batch_blob_bound", "batch_seal", "encode_batch_blob", "batch_open"):
        assert callable(getattr(Codec, name)), name
    for name in ("compress_batch", "decompress_batch", "batch_info"):
        assert callable(getattr(huffman, name)), name


def test_seal_and_open_argument_errors_come_before_the_context():
    """The context is a host dummy: reading it, or a launch, would not return DC_E_ARG."""
    from data_compression_amd._lib import HBatch, HBlobInfo, HBlobView
    L = _lib()
    keep = C.create_string_buffer(4096)
    p = (C.addressof(keep) + 255) & ~255
    b = HBatch()
    b.count, b.n_ary, b.sync_syms = 0, 2, 64
    info, view = HBlobInfo(), HBlobView()
    assert L.dc_huff_batch_seal(None, C.byref(b), None, 0, 0, None, 0, None, None, p, 64, p + 512, None) == -1
    assert L.dc_huff_batch_seal(p, None, None, 0, 0, None, 0, None, None, p, 64, p + 512, None) == -1
    for kind, flags, K in ((4, 0, 0), (0, 2, 0), (0, 0, 1), (2, 0, 0), (3, 0, 0), (3, 0, 65), (-1, 0, 0)):
        assert L.dc_huff_batch_seal(p, C.byref(b), None, kind, flags, p + 1024, K, None, None, p, 64, p + 512, None) == -1
    assert L.dc_huff_batch_seal(p, C.byref(b), None, 0, 0, None, 0, None, None, p + 8, 64, p + 512, None) == -1   # blob off 16
    assert L.dc_huff_batch_seal(p, C.byref(b), None, 0, 0, None, 0, None, None, p, 64, None, None) == -1          # no d_info
    assert L.dc_huff_batch_seal(p, C.byref(b), None, 0, 0, None, 0, None, None, p, 64, p + 32, None) == -1        # d_info in the blob
    assert L.dc_huff_batch_blob_layout(0, 0, 0, 0, C.byref(info)) == 0
    info.n_ary, info.sync_syms, info.blob_bytes, info.sync_off = 2, 64, 64, 64
    assert L.dc_huff_batch_open(None, p, 64, C.byref(info), p + 1024, 2048, C.byref(view)) == -1
    assert L.dc_huff_batch_open(p, p + 8, 64, C.byref(info), p + 1024, 2048, C.byref(view)) == -1    # blob off 16
    assert L.dc_huff_batch_open(p, p, 63, C.byref(info), p + 1024, 2048, C.byref(view)) == -1        # blob_bytes > m
    assert L.dc_huff_batch_open(p, p, 64, C.byref(info), p + 1024, 16, C.byref(view)) == -1          # workspace too small
    assert L.dc_huff_batch_open(p, p, 64, C.byref(info), p, 2048, C.byref(view)) == -1               # workspace on the blob
    info.payload_off = 80
    assert L.dc_huff_batch_open(p, p, 4096, C.byref(info), p + 1024, 2048, C.byref(view)) == -1      # an offset that is not the layout's


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flags", (0, M.CRC))
def test_parse_of_write_is_the_identity(kind, flags):
    c = container(kind, flags, 2, 64, [0, 1, 63, 64, 65, 100, 4097, 17], seed=3)
    P, a = M.parse(c["blob"]), c["arrays"]
    n = len(c["segs"])
    assert (P["kind"], P["flags"], P["n_ary"], P["S"], P["count"]) == (kind, flags, 2, 64, n)
    assert P["blob_bytes"] == len(c["blob"]) and len(c["blob"]) % 16 == 0
    assert np.array_equal(P["len"], c["seg_len"]) and np.array_equal(P["bits"], a["bits"]) and np.array_equal(P["mode"], a["mode"])
    assert np.array_equal(P["payload"], a["payload"]) and np.array_equal(P["sync_len"], a["sync_len"])
    assert P["total_bytes"] == c["seg_len"].sum() and P["pay_total"] == a["pay_off"][n] and P["sync_total"] == a["sync_off"][n]
    if kind == M.OWN:
        assert np.array_equal(P["records"], a["lens"])
    elif kind == M.OWN4:
        assert np.array_equal(M.unpack4(P["records"]), a["lens"])
    else:
        assert np.array_equal(P["records"], c["records"]) and P["K"] == len(c["recs"])
    assert (P["tid"] is not None) == (kind == M.SET) and (kind != M.SET or np.array_equal(P["tid"], a["tid"]))
    assert (P["crcs"] is not None) == bool(flags) and (not flags or np.array_equal(P["crcs"], c["crc"]))
    off, po, so = M.derived(P["len"], P["bits"], 64)
    assert np.array_equal(po, a["pay_off"]) and np.array_equal(so, a["sync_off"])
    assert M.check(c["blob"]) == M.DC_OK and a["mode"].any() and not a["mode"].all()
    # writing the parsed sections again gives the same bytes
    again = {"mode": P["mode"], "bits": P["bits"], "payload": P["payload"], "pay_off": po, "sync_len": P["sync_len"],
             "sync_off": so, "lens": a.get("lens"), "tid": P["tid"]}
    assert M.write(again, P["len"], kind, flags, 2, 64, records=c["records"], crc=P["crcs"]) == c["blob"]


def test_nybble_records_that_do_not_pack_are_zeros():
    deep = BB._levels(2, 17)
    assert deep.max() > 15
    rec, ok = M.lens4(np.stack([BB.record("b12")["lens"], deep.astype(np.uint8)]))
    assert ok.tolist() == [True, False] and not rec[1].any() and rec[0].any()
    assert np.array_equal(M.unpack4(rec)[0], BB.record("b12")["lens"])


@pytest.mark.parametrize("name", [c[0] for c in CPU_CATALOGUE])
def test_library_agrees_with_the_model(built, name):
    from data_compression_amd._lib import HBlobInfo
    c, L = built[name], _lib()
    blob, n = c["blob"], len(c["segs"])
    assert M.check(blob) == M.DC_OK and lib_check(blob) == 0
    rc, I = lib_info(blob)
    H = M.header_ok(blob)
    assert rc == 0 and H is not None
    for lib_name, model_name in (("version", "version"), ("kind", "kind"), ("flags", "flags"), ("K", "K"), ("n_ary", "n_ary"),
                                 ("sync_syms", "S"), ("count", "count"), ("total_bytes", "total_bytes"),
                                 ("sync_total", "sync_total"), ("pay_total", "pay_total"), ("blob_bytes", "blob_bytes"),
                                 ("len_off", "len_off"), ("bits_off", "bits_off"), ("mode_off", "mode_off"),
                                 ("tid_off", "tid_off"), ("crc_off", "crc_off"), ("rec_off", "rec_off"),
                                 ("rec_bytes", "rec_bytes"), ("payload_off", "payload_off"), ("sync_off", "sync_off")):
        assert I[lib_name] == H[model_name], lib_name
    lay = HBlobInfo()
    assert L.dc_huff_batch_blob_layout(n, c["kind"], c["flags"], H["K"], C.byref(lay)) == 0
    want = M.layout(n, c["kind"], c["flags"], H["K"])
    assert {k: v for k, v in lay.as_dict().items() if k in want} == want
    assert lay.work_bytes == I["work_bytes"] and I["work_bytes"] >= 3 * 8 * n + 3 * 8 * (n + 1) + 4 * n + 4
    total = int(c["seg_len"].sum())
    bound = L.dc_huff_batch_blob_bound(total, n, c["S"], c["kind"], c["flags"], H["K"])
    assert bound == M.bound(total, n, c["S"], c["kind"], c["flags"], H["K"]) and bound >= len(blob)
    # more bytes at hand than the container takes are fine; fewer are not
    assert lib_check(blob + b"\x55" * 5) == 0 and M.check(blob + b"\x55" * 5) == 0
    assert lib_check(blob, len(blob) - 1) == M.DC_E_STREAM


@pytest.mark.parametrize("name", ("k0f0c17", "k1f1c16", "k2f1c15", "k3f1c17", "k3f0c0", "n256"))
def test_damaged_containers_are_refused_as_the_model_refuses_them(built, name):
    c = built[name]
    for what, blob, m in header_damage(c):
        assert M.check(blob, m) == M.DC_E_STREAM, what
        assert lib_check(blob, m) == M.DC_E_STREAM and lib_info(blob, m)[0] == M.DC_E_STREAM, what
    if not len(c["segs"]):
        return
    i = next(k for k in range(len(c["segs"])) if c["arrays"]["mode"][k] == 1 and c["seg_len"][k] > 1)
    for what, blob in directory_damage(c, i):
        # bits +- 1 passes the container rule where ceil(bits / 8) and the bound 8 len allow it: the
        # decode is what sees it then (tests/test_gpu_batch_blob.py)
        assert M.check(blob) == M.DC_E_STREAM or what.startswith("bits"), what
        assert lib_check(blob) == M.check(blob) and lib_info(blob)[0] == 0, what   # (the header alone is whole)


def test_the_bound_holds_every_container_and_is_tight_only_without_segments():
    """bound >= blob_bytes for every shape. The payload bound is dc_huff_batch_payload_bound's total +
    16 count, 16 bytes a segment more than a stored segment of a multiple of 16 bytes takes, so
    equality is reached at count 0 alone; for stored segments of multiples of 16 bytes the slack is
    exactly those 16 count bytes plus what the sync bound's `+ count` entries add after padding."""
    L = _lib()
    for kind in KINDS:
        K = {M.SHARED: 1, M.SET: 5}.get(kind, 0)
        for flags in (0, M.CRC):
            assert L.dc_huff_batch_blob_bound(0, 0, 64, kind, flags, K) == M.layout(0, kind, flags, K)["payload_off"]
    assert L.dc_huff_batch_blob_bound(0, 0, 64, M.OWN, 0, 0) == 64
    rng = np.random.default_rng(5)
    for S in (16, 64, 1024):
        for lens in ([16], [S], [16 * 7, S * 3, 16], [S * 8] * 9, [65536, 16, 4096]):
            segs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
            arrays = BB.hand_batch("own", [(s, None) for s in segs], 2, S, [])
            blob = M.write(arrays, lens, M.OWN, 0, 2, S)
            total, n = sum(lens), len(lens)
            chunks = sum(-(-v // S) for v in lens)
            bound = L.dc_huff_batch_blob_bound(total, n, S, M.OWN, 0, 0)
            assert bound - len(blob) == 16 * n + M.pad16(2 * (-(-total // S) + n)) - M.pad16(2 * chunks)
            assert lib_check(blob) == 0
    for args in ((0, 0, 48, 0, 0, 0), (0, M.COUNT_MAX + 1, 64, 0, 0, 0), (2**64 - 1, 1, 64, 0, 0, 0), (0, 0, 64, 4, 0, 0),
                 (0, 0, 64, 0, 2, 0), (0, 0, 64, 3, 0, 0), (0, 0, 64, 0, 0, 1)):
        assert L.dc_huff_batch_blob_bound(*args) == 0 == M.bound(*args), args


def test_blob_checker_builds_and_passes(tmp_path):
    """tests/c/batch_blob_check.c: the same header in a stand-alone C program, with the host
    sanitizers where the compiler has them."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc, "no C compiler"
    exe = str(tmp_path / "batch_blob_check")
    base = [cc, "-std=c11", "-g", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "data_compression_amd", "csrc"),
            os.path.join(REPO, "tests", "c", "batch_blob_check.c"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)   # (a compiler without the sanitizer runtimes)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "batch_blob_check: ok" in r.stdout, r.stdout + r.stderr
