"""Checksums (dc_gpu.h "checksums") without a device: the five entry points are exported and
declared; the device calls' host argument checks come before the first read of the context; the
host CRC (dc_crc32_host) is zlib.crc32 on every length 0..300 at every source alignment 0..15 and
in running form; dc_crc32_combine is zlib.crc32 of the concatenation, and at len_b = 2^32 + 5 a
pure-Python model of the product; the constants Python hands out are the header's. The header's
own check under the host sanitizers is tests/c/crc32_check.c."""
import ctypes as C
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_E_ARG = -1
RANGES_MAX = 1 << 28   # DC_RANGES_MAX
ENTRY_POINTS = ("dc_crc32_host", "dc_crc32_combine", "dc_crc32", "dc_crc32_batch", "dc_crc32_verify_batch")

POLY = 0xEDB88320
X0 = 0x80000000   # x^0 in reflected form; x^1 = 0x40000000


def model_mul(a, b):
    """a b mod P in reflected form: 32 shift-and-xor steps."""
    p = 0
    for k in range(32):
        if a & (X0 >> k):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def model_xpow(bits):
    """x^bits mod P by square and multiply over the bits of the exponent."""
    p, sq = X0, X0 >> 1
    while bits:
        if bits & 1:
            p = model_mul(p, sq)
        sq = model_mul(sq, sq)
        bits >>= 1
    return p


def model_combine(crc_a, crc_b, len_b):
    return model_mul(crc_a, model_xpow(8 * len_b)) ^ crc_b


def _lib():
    from data_compression_amd._lib import core
    return core()


def test_entry_points_are_exported_and_declared():
    L = _lib()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes is not None, name
    assert L.dc_crc32_host.restype is C.c_uint32 and len(L.dc_crc32_host.argtypes) == 3
    assert L.dc_crc32_combine.restype is C.c_uint32 and len(L.dc_crc32_combine.argtypes) == 3
    assert L.dc_crc32.restype is C.c_int and len(L.dc_crc32.argtypes) == 4
    assert L.dc_crc32_batch.restype is C.c_int and len(L.dc_crc32_batch.argtypes) == 8
    assert L.dc_crc32_verify_batch.restype is C.c_int and len(L.dc_crc32_verify_batch.argtypes) == 8
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(REPO, "data_compression_amd", "lib", "libdc_core.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(ENTRY_POINTS) <= exported


def test_constants_are_the_headers():
    from data_compression_amd._lib import DcError
    from data_compression_amd.device import Codec
    text = open(os.path.join(REPO, "include", "dc_gpu.h")).read()
    assert int(re.search(r"#define DC_CRC_TILE (\d+)u", text).group(1)) == Codec.CRC_TILE == 1024
    assert int(re.search(r"#define DC_CRC_PIECE (\d+)u", text).group(1)) == Codec.CRC_PIECE
    assert Codec.CRC_PIECE % Codec.CRC_TILE == 0
    assert int(re.search(r"DC_E_CHECKSUM = (-\d+)", text).group(1)) == Codec.E_CHECKSUM == -9
    assert DcError.NAMES[-9] == "DC_E_CHECKSUM"
    for v, name in DcError.NAMES.items():   # no existing value changed
        assert int(re.search(name + r" = (-\d+)", text).group(1)) == v


@pytest.fixture()
def dummies():
    keep = [C.create_string_buffer(64) for _ in range(6)]
    return [C.cast(k, C.c_void_p) for k in keep] + [keep]   # never read: a check fails first


def test_host_argument_checks(dummies):
    """Every failing test comes before the first read of the context, which is a host dummy here;
    count 0 returns DC_OK before it too."""
    L = _lib()
    ctx, d_in, beg, end, crc, st, _ = dummies
    for fn in (L.dc_crc32_batch, L.dc_crc32_verify_batch):
        assert fn(None, d_in, 64, beg, end, 1, crc, st) == DC_E_ARG
        assert fn(None, d_in, 64, beg, end, 0, crc, st) == DC_E_ARG
        assert fn(ctx, None, 64, beg, end, 1, crc, st) == DC_E_ARG
        assert fn(ctx, d_in, 64, None, end, 1, crc, st) == DC_E_ARG
        assert fn(ctx, d_in, 64, beg, None, 1, crc, st) == DC_E_ARG
        assert fn(ctx, d_in, 64, beg, end, 1, None, st) == DC_E_ARG
        assert fn(ctx, d_in, 64, beg, end, 1, crc, None) == DC_E_ARG
        assert fn(ctx, d_in, 64, beg, end, RANGES_MAX + 1, crc, st) == DC_E_ARG
        assert fn(ctx, d_in, 64, beg, end, 1 << 63, crc, st) == DC_E_ARG
        assert fn(ctx, None, 0, None, None, 0, None, None) == 0      # count 0: nothing to do, no launch
    assert L.dc_crc32(None, d_in, 5, crc) == DC_E_ARG
    assert L.dc_crc32(ctx, d_in, 5, None) == DC_E_ARG
    assert L.dc_crc32(ctx, None, 5, crc) == DC_E_ARG
    assert L.dc_crc32(None, None, 0, crc) == DC_E_ARG


def test_host_crc_is_zlibs_at_every_length_and_alignment():
    L = _lib()
    rng = np.random.default_rng(32)
    raw = (C.c_uint8 * (16 + 316))()
    base = C.addressof(raw)
    base += (-base) % 16
    data = rng.integers(0, 256, 316, dtype=np.uint8).tobytes()
    C.memmove(base, data, 316)
    for a in range(16):
        for n in range(301):
            assert L.dc_crc32_host(0, base + a, n) == zlib.crc32(data[a: a + n]), (a, n)
    assert L.dc_crc32_host(0, None, 0) == 0 and L.dc_crc32_host(77, base, 0) == 77
    assert L.dc_crc32_host(0, b"123456789", 9) == 0xCBF43926
    for n in (0, 1, 2, 3, 7, 100, 299, 316):     # the running form over three pieces
        p, q = n // 3, n - n // 4
        r = L.dc_crc32_host(0, base, p)
        r = L.dc_crc32_host(r, base + p, q - p)
        r = L.dc_crc32_host(r, base + q, n - q)
        assert r == zlib.crc32(data[:n]), n


def test_combine_is_the_crc_of_the_concatenation():
    L = _lib()
    rng = np.random.default_rng(33)
    for _ in range(200):
        n = int(rng.integers(0, 5000))
        k = int(rng.integers(0, n + 1))
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert L.dc_crc32_combine(zlib.crc32(d[:k]), zlib.crc32(d[k:]), n - k) == zlib.crc32(d), (n, k)
    d = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    assert L.dc_crc32_combine(zlib.crc32(d), 0, 0) == zlib.crc32(d)            # an empty B
    assert L.dc_crc32_combine(zlib.crc32(d[:39]), zlib.crc32(d[39:]), 1) == zlib.crc32(d)
    assert L.dc_crc32_combine(0, zlib.crc32(d), 40) == zlib.crc32(d)           # an empty A


def test_combine_at_large_lengths_is_the_model():
    L = _lib()
    assert model_mul(X0, 0xDEADBEEF) == 0xDEADBEEF
    d = bytes(range(50))
    assert model_combine(zlib.crc32(d[:20]), zlib.crc32(d[20:]), 30) == zlib.crc32(d)   # the model is zlib's too
    rng = np.random.default_rng(34)
    for len_b in ((1 << 32) + 5, 1 << 40, (1 << 61) + 1, (1 << 64) - 1):
        for _ in range(4):
            a, b = (int(v) for v in rng.integers(0, 1 << 32, 2))
            assert L.dc_crc32_combine(a, b, len_b) == model_combine(a, b, len_b), len_b


def test_crc_checker_builds_and_passes(tmp_path):
    """tests/c/crc32_check.c: the same header in a stand-alone C program, with the host sanitizers
    where the compiler has them."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc, "no C compiler"
    exe = str(tmp_path / "crc32_check")
    base = [cc, "-std=c11", "-g", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "data_compression_amd", "csrc"),
            os.path.join(REPO, "tests", "c", "crc32_check.c"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)   # (a compiler without the sanitizer runtimes)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "crc32_check: ok" in r.stdout, r.stdout + r.stderr
