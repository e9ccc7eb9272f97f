"""The batched nybble codec (dc_gpu.h "nybble batch v1") without a device: the bound function
(pure host arithmetic, csrc/dc_nyb_batch_bound.h), the host argument checks of the two entry
points, and the expected batch built from the CPU oracle alone. STREAM_INPUTS, pack_offsets and
oracle_streams are shared with tests/test_gpu_nyb_batch.py."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests.stream_batch_checks import pack_offsets

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_E_ARG = -1
RANGES_MAX = 1 << 28   # DC_RANGES_MAX
EDGE_LENGTHS = (127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 65_537)


def _inputs():
    from data_compression_amd import synth
    rng = np.random.default_rng(71)
    bufs = [synth.english_like(n, seed=n) for n in range(60)]
    bufs += [synth.english_like(n, seed=n) for n in EDGE_LENGTHS]
    bufs.append(rng.integers(1, 128, size=100, dtype=np.uint8))     # LITERAL
    bufs.append(rng.integers(1, 128, size=3000, dtype=np.uint8))    # long enough for the lists to pay
    bufs.append(np.concatenate([rng.integers(128, 256, size=500, dtype=np.uint8), synth.english_like(310, seed=310)]))
    for _ in range(300):
        bufs.append(synth.english_like(int(rng.integers(1, 2001)), seed=int(rng.integers(1 << 30))))
    return [np.ascontiguousarray(b, np.uint8) for b in bufs]


STREAM_INPUTS = _inputs()
I_RANDOM_100, I_RANDOM_3000, I_HIGH = 70, 71, 72   # their places in STREAM_INPUTS


@functools.lru_cache(maxsize=None)
def _oracle_inputs(modify):
    return tuple(orc.nybble_compress(b.tobytes(), modify) for b in STREAM_INPUTS)


def oracle_streams(bufs, modify):
    """The reference stream of every buffer, from oracle.oracle alone. Those of STREAM_INPUTS
    are computed once per mode: do not modify."""
    if bufs is STREAM_INPUTS:
        return _oracle_inputs(bool(modify))
    return tuple(orc.nybble_compress(b.tobytes(), bool(modify)) for b in bufs)


@pytest.mark.parametrize("count", (0, 1, 300))
@pytest.mark.parametrize("total", (0, 1, 65536, 2**33 + 5))
def test_bound_is_its_formula(total, count):
    from data_compression_amd._lib import core
    assert core().dc_nyb_batch_bound(total, count) == total + count


@pytest.mark.parametrize("modify", (False, True))
def test_bound_holds_the_oracle_batch(modify):
    from data_compression_amd._lib import core
    L = core()
    streams = oracle_streams(STREAM_INPUTS, modify)
    assert sum(map(len, streams)) <= L.dc_nyb_batch_bound(sum(b.size for b in STREAM_INPUTS), len(STREAM_INPUTS))
    for b, s in zip(STREAM_INPUTS, streams):   # and buffer by buffer, where it is exact for LITERAL
        assert len(s) <= L.dc_nyb_batch_bound(b.size, 1)
        assert s[0] in (0xAF, 0x20) and (s[0] == 0xAF or len(s) == b.size + 1)


def test_inputs_are_the_list_of_the_issue():
    sizes = [b.size for b in STREAM_INPUTS]
    assert sizes[:60] == list(range(60)) and tuple(sizes[60:70]) == EDGE_LENGTHS
    assert sizes[I_RANDOM_100] == 100 and sizes[I_RANDOM_3000] == 3000 and sizes[I_HIGH] == 810
    assert len(STREAM_INPUTS) == 373 and all(1 <= n <= 2000 for n in sizes[73:])
    assert sum(sizes) < 1 << 20
    assert (STREAM_INPUTS[I_HIGH][:500] >= 128).all() and (STREAM_INPUTS[I_HIGH][500:] < 128).all()
    assert all((b != 0).all() for b in STREAM_INPUTS)   # byte 0 is outside the reference's domain
    _, off = pack_offsets(STREAM_INPUTS)
    assert (off[1:-1] % 2 == 1).sum() >= len(STREAM_INPUTS) // 2   # packed back to back: odd offsets
    assert (off[1:-1] % 16 != 0).sum() >= len(STREAM_INPUTS) * 3 // 4   # and shared 16-B granules


@pytest.mark.parametrize("modify", (False, True))
def test_oracle_puts_both_forms_and_the_tightest_stream_in_the_list(modify):
    """What the device test relies on: LITERAL and nybble streams both occur, and a nybble stream
    of n - 1 bytes (the longest the nybble form may be) occurs. A change to synth that hollowed
    the list out would fail here."""
    streams = oracle_streams(STREAM_INPUTS, modify)
    form = lambda i: "literal" if streams[i][0] == 0x20 else "nybble"
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 10):
        assert form(n) == "literal" and len(streams[n]) == n + 1, n
    assert streams[0] == b" "
    for n in (6, 9):
        assert form(n) == "nybble" and len(streams[n]) == n - 1, n
    assert form(I_RANDOM_100) == "literal"
    assert form(I_RANDOM_3000) == "nybble"
    assert form(I_HIGH) == "nybble"
    forms = {form(i) for i in range(len(streams))}
    assert forms == {"literal", "nybble"}
    assert any(s[0] == 0xAF and len(s) == b.size - 1 for b, s in zip(STREAM_INPUTS, streams))
    for b, s in zip(STREAM_INPUTS[:80], streams[:80]):
        if (b < 128).all():   # (bytes >= 0x80 do not round-trip through the reference codec)
            assert orc.nybble_decompress(s, modify) == b.tobytes()


def test_entry_points_are_exported_and_declared():
    from data_compression_amd._lib import core
    L = core()
    assert L.dc_nyb_batch_bound.restype is C.c_uint64 and len(L.dc_nyb_batch_bound.argtypes) == 2
    for name in ("dc_nyb_compress_batch", "dc_nyb_decompress_batch_async"):
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == 9, name


@pytest.fixture()
def dummies():
    keep = [C.create_string_buffer(64) for _ in range(6)]
    return {"ptr": [C.cast(k, C.c_void_p) for k in keep], "keep": keep}   # never read: a check fails first


def _calls(L, ctx, p, count, cap=64):
    """(compress, decompress) return codes; p: d_in, d_in_off, d_out, d_out_off, d_status."""
    d_in, in_off, out, out_off, st = p
    return (L.dc_nyb_compress_batch(ctx, d_in, in_off, count, 1, out, cap, out_off, st),
            L.dc_nyb_decompress_batch_async(ctx, d_in, in_off, count, 1, out, out_off, cap, st))


def test_host_argument_checks(dummies):
    """The context is a host dummy: a launch, or any read of it, would not return these codes."""
    from data_compression_amd._lib import core
    L = core()
    ctx, p = dummies["ptr"][0], dummies["ptr"][1:]
    assert _calls(L, None, p, 1) == (DC_E_ARG, DC_E_ARG)
    assert _calls(L, None, p, 0) == (DC_E_ARG, DC_E_ARG)
    assert _calls(L, ctx, p, 0) == (0, 0)                      # no buffers: OK without a launch
    assert _calls(L, ctx, [None] * 5, 0) == (0, 0)
    for k in range(5):                                         # each pointer in turn
        q = list(p)
        q[k] = None
        assert _calls(L, ctx, q, 1) == (DC_E_ARG, DC_E_ARG), k
    for n in (RANGES_MAX + 1, 1 << 40, (1 << 64) - 1):
        assert _calls(L, ctx, p, n) == (DC_E_ARG, DC_E_ARG), n


def test_bound_checker_builds_and_passes(tmp_path):
    """tests/c/nyb_batch_bound_check.c: the same header in a stand-alone C program, with the host
    sanitizers where the compiler has them."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc, "no C compiler"
    exe = str(tmp_path / "nyb_batch_bound_check")
    base = [cc, "-std=c11", "-g", "-Wall", "-Werror", "-I" + os.path.join(REPO, "data_compression_amd", "csrc"),
            os.path.join(REPO, "tests", "c", "nyb_batch_bound_check.c"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)   # (a compiler without the sanitizer runtimes)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "nyb_batch_bound_check: ok" in r.stdout, r.stdout + r.stderr
