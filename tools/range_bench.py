"""Range decode (dc_huff_decode_range / dc_huff_decode_ranges, DCH1 range reads) on the 1 GiB
C2 stream of bench.py (synth.device_text, seed 0xC2, n = 2), one process, every comparison inside
the same run with the two sides alternating:
  whole   decode_range(0, n) against dc_huff_decode with decode_general = 1 (the kernel the range
          kernel is built on) and against the default fast decoder
  gather  2^18 random 4 KiB ranges, then 2^20 random 256-byte ranges: us per call and GB/s of
          output bytes, beside a full decode of the stream (the only way without range decode)
  host    huffman.decompress_range of 64 KiB out of a 256 MiB DCH1 container against
          decompress of the whole container
Device times are HIP events around `--steps` calls, the median of `--rounds` rounds; host times
are wall clock around calls that end in a copy to the host. Prints one JSON line per result.
    timeout 600 python tools/range_bench.py [--size BYTES] [--steps K] [--rounds R] [--only whole,gather,host]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from data_compression_amd import huffman, synth  # noqa: E402
from data_compression_amd._lib import core  # noqa: E402
from data_compression_amd.device import Codec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--host-size", type=int, default=256 << 20)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--only", default="whole,gather,host")
a = ap.parse_args()
assert torch.cuda.is_available(), "range_bench needs a GPU"
dev = "cuda:0"
c = Codec(0)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def ev_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(fns, steps, rounds):
    """{name: median ms per call}; the candidates take turns inside every round"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(ev_ms(fn, steps))
    return {k: statistics.median(v) for k, v in t.items()}, {k: (min(v), max(v)) for k, v in t.items()}


n = a.size
x = synth.device_text("C2", n, seed=0xC2, device=dev)
enc = c.encode(x, n_ary=2)
S = enc["S"]
emit(what="stream", n=n, bits=enc["bits"], S=S, bits_per_byte=round(enc["bits"] / n, 4))
full = torch.empty(n, dtype=torch.uint8, device=dev)


def dec_fast():
    c.decode_into(enc, full)


def dec_general():
    c.set_option("decode_general", 1)
    c.decode_into(enc, full)
    c.set_option("decode_general", 0)


if "whole" in a.only:
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    c.decode_range(enc, 0, n, out=out)
    assert c.decode_status() == 0 and torch.equal(out, x), "range decode of the whole stream differs"
    dec_general()
    assert c.decode_status() == 0 and torch.equal(full, x)
    med, spread = alternate({"range_0_n": lambda: c.decode_range(enc, 0, n, out=out), "general": dec_general,
                             "fast": dec_fast}, a.steps, a.rounds)
    emit(what="whole", ms=med, min_max_ms=spread, range_over_general=round(med["range_0_n"] / med["general"], 4),
         range_GBps=round(n / med["range_0_n"] / 1e6, 1))
    del out

if "gather" in a.only:
    for log_nr, size in ((18, 4096), (20, 256)):
        nr = 1 << log_nr
        g = torch.Generator(device=dev).manual_seed(7 + log_nr)
        first = torch.randint(0, n - size + 1, (nr,), generator=g, device=dev, dtype=torch.int64)
        count = torch.full((nr,), size, dtype=torch.int64, device=dev)
        out_off = torch.cumsum(count, 0) - count
        out = torch.empty(nr * size, dtype=torch.uint8, device=dev)
        c.decode_ranges(enc, first, count, out=out, out_off=out_off)
        assert c.decode_status() == 0
        pick = torch.arange(0, nr, nr // 2048, device=dev)   # 2048 of the ranges against the input
        idx = first[pick, None] + torch.arange(size, device=dev)[None, :]
        assert torch.equal(out.view(nr, size)[pick], x[idx]), "gathered bytes differ from the input"
        del idx
        med, spread = alternate({"ranges": lambda: c.decode_ranges(enc, first, count, out=out, out_off=out_off),
                                 "full_decode": dec_fast}, a.steps, a.rounds)
        emit(what="gather", ranges=nr, bytes_each=size, out_bytes=nr * size, us_per_call=round(med["ranges"] * 1e3, 1),
             out_GBps=round(nr * size / med["ranges"] / 1e6, 1), full_decode_us=round(med["full_decode"] * 1e3, 1),
             min_max_ms=spread)
        c.timing(True)
        c.decode_ranges(enc, first, count, out=out, out_off=out_off)
        emit(what="gather_kernels", ranges=nr, ms={k: round(v, 4) for k, v in c.timings()})
        c.timing(False)
        del out, first, count, out_off

if "host" in a.only:
    L = core()
    hn = min(a.host_size, n)
    xh = x[:hn].cpu().numpy()
    cap = int(L.dc_huff_compress_bound(hn, 0))
    buf = np.empty(cap, np.uint8)
    got = C.c_uint64(0)
    u8p = C.POINTER(C.c_uint8)
    rc = L.dc_huff_compress_host(xh.ctypes.data_as(u8p), hn, 2, None, 258, 0, buf.ctypes.data_as(u8p), cap, C.byref(got))
    assert rc == 0, rc
    blob = buf[: got.value].tobytes()
    del buf
    take = 64 << 10
    rng = np.random.default_rng(11)
    firsts = [int(v) for v in rng.integers(0, hn - take, 8)]

    def wall(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return statistics.median(ts) * 1e3

    for f in firsts:
        assert huffman.decompress_range(blob, f, take) == xh[f: f + take].tobytes()
    k = [0]

    def one_range():
        k[0] += 1
        huffman.decompress_range(blob, firsts[k[0] % len(firsts)], take)

    whole_out = np.empty(hn, np.uint8)
    inp = np.frombuffer(blob, np.uint8)

    def whole_c():   # dc_huff_decompress_host on buffers already in place (no Python copies)
        r = L.dc_huff_decompress_host(inp.ctypes.data_as(u8p), len(blob), whole_out.ctypes.data_as(u8p), hn, C.byref(got))
        assert r == 0 and got.value == hn

    whole_c()
    assert np.array_equal(whole_out, xh)
    emit(what="host", container_bytes=len(blob), n=hn, range_bytes=take,
         decompress_range_ms=round(wall(one_range, 20), 3),
         decompress_whole_c_ms=round(wall(whole_c, 3), 2),
         decompress_whole_python_ms=round(wall(lambda: huffman.decompress(blob, hn), 2), 2))
