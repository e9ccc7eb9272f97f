"""The batched small front-end (dc_small_compress_batch / dc_small_decompress_batch) on the first
256 MiB of bench.py's text (synth.device_text C1, seed 0xC1), one process:
  blocks  65 536 x 4 KiB: the batch encode and decode against dc_small_compress /
          dc_small_decompress of the same bytes as ONE stream (the only other way to run this codec
          on the device; it spreads one stream over the whole device and reads the length back);
          HIP events around each call, the two sides alternating, the median of `--rounds` rounds
          after a warm-up; the single-stream call against itself the same way gives the spread of
          such a comparison; and the per-kernel split of one call (dc_ctx_timings)
  loop    4096 x 4 KiB: one batch call each way against the loop of Codec.small_compress /
          small_decompress over the same buffers (all a caller could do before), wall clock around
          calls that end synchronised, alternating
  mixed   the same 256 MiB cut into lengths log-uniform in 64 B .. 64 KiB, once in drawn
          (shuffled) order and once sorted by length, against the single stream again: a wave per
          buffer in a fixed stride, so what the order costs is the uneven share of long buffers
          among the waves
Every output is checked for equality before it is timed. No time is a pass condition. One JSON
line per result, to stdout and appended to --log (default profiles/small_batch.log).
    timeout 900 python tools/small_batch_bench.py [--rounds R] [--only blocks,loop,mixed] [--log FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from data_compression_amd import synth  # noqa: E402
from data_compression_amd.device import Codec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256 << 20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--only", default="blocks,loop,mixed")
ap.add_argument("--log", default=os.path.join(REPO, "profiles", "small_batch.log"))
a = ap.parse_args()
assert a.rounds >= 5, "at least 5 repetitions"
assert torch.cuda.is_available(), "small_batch_bench needs a GPU"
dev = "cuda:0"
c = Codec(0)
K = 4096
log = open(a.log, "a")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def ev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(sides, rounds, timer=ev_ms):
    """sides: name -> fn. A warm-up call of each, then `rounds` rounds of one timed call of each
    in turn: name -> (median ms, [min, max])."""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            t[k].append(timer(fn))
    return {k: (round(statistics.median(v), 3), [round(min(v), 3), round(max(v), 3)]) for k, v in t.items()}


def stages(fn):
    c.timing(True)
    fn()
    ms = {k: round(v, 4) for k, v in c.timings()}
    c.timing(False)
    return ms


def gbps(nbytes, ms):
    return round(nbytes / ms / 1e6, 1)


n = a.size
x = synth.device_text("C1", 1 << 30, seed=0xC1, device=dev)[:n].clone()   # the first 256 MiB of the bench's text
one_out = torch.empty(n + 64, dtype=torch.uint8, device=dev)               # the single stream ...
one = c.small_compress(x, out=one_out).clone()
one_back = torch.empty(2 * one.numel(), dtype=torch.uint8, device=dev)     # ... and its decode
assert torch.equal(c.small_decompress(one, out=one_back), x), "the single stream does not round-trip"
torch.cuda.synchronize()


def single_encode():
    c.small_compress(x, out=one_out)


def single_decode():
    c.small_decompress(one, out=one_back)


def batch_sides(off, count, what, **tags):
    """One batch of `count` buffers at offsets `off`: checked, then timed against the single stream."""
    out = torch.empty(c.small_batch_bound(n, count), dtype=torch.uint8, device=dev)
    back = torch.zeros(n, dtype=torch.uint8, device=dev)
    _, oo, st = c.small_compress_batch(x, off, out=out)
    total = int(oo[-1])
    assert c.batch_status() == 0
    comp = out[:total].clone()
    c.small_decompress_batch_into(comp, oo, off, out=back)
    assert c.batch_status() == 0 and torch.equal(back, x), what + ": the round trip differs from the input"
    emit(what=what + "_size", count=count, bytes=n, compressed_bytes=total, single_stream_bytes=one.numel(), **tags)
    enc = alternate({"batch": lambda: c.small_compress_batch(x, off, out=out), "single": single_encode}, a.rounds)
    dec = alternate({"batch": lambda: c.small_decompress_batch_into(comp, oo, off, out=back), "single": single_decode},
                    a.rounds)
    for name, t in (("encode", enc), ("decode", dec)):
        emit(what=what + "_" + name, count=count, batch_ms=t["batch"][0], single_ms=t["single"][0],
             batch_GBps=gbps(n, t["batch"][0]), single_GBps=gbps(n, t["single"][0]),
             batch_over_single=round(t["batch"][0] / t["single"][0], 3), batch_min_max_ms=t["batch"][1],
             single_min_max_ms=t["single"][1], **tags)
    emit(what=what + "_stages", count=count, ms=stages(lambda: (
        c.small_compress_batch(x, off, out=out), single_encode(),
        c.small_decompress_batch_into(comp, oo, off, out=back), single_decode())), **tags)


if "blocks" in a.only:
    count = (n + K - 1) // K
    off = torch.arange(0, n + K, K, dtype=torch.int64, device=dev).clamp_(max=n)[: count + 1].contiguous()
    batch_sides(off, count, "blocks", block=K)
    self_ = alternate({"a": single_encode, "b": single_encode}, a.rounds)
    emit(what="single_vs_itself", encode_ms=[self_["a"][0], self_["b"][0]], min_max_ms=[self_["a"][1], self_["b"][1]],
         spread=round(abs(self_["a"][0] - self_["b"][0]) / min(self_["a"][0], self_["b"][0]), 4))

if "loop" in a.only:
    count = 4096
    m = count * K
    xs = x[:m]
    bufs = [xs[i * K: (i + 1) * K] for i in range(count)]
    off = torch.arange(0, m + K, K, dtype=torch.int64, device=dev)[: count + 1].contiguous()
    out = torch.empty(c.small_batch_bound(m, count), dtype=torch.uint8, device=dev)
    back = torch.empty(m, dtype=torch.uint8, device=dev)
    dec_out = torch.empty(2 * K + 16, dtype=torch.uint8, device=dev)
    state = {}

    def batch_encode():
        state["enc"] = c.small_compress_batch(xs, off, out=out)
        assert c.batch_status() == 0

    def batch_decode():
        c.small_decompress_batch_into(state["enc"][0], state["enc"][1], off, out=back)
        assert c.batch_status() == 0

    def loop_encode():
        state["streams"] = [c.small_compress(b) for b in bufs]   # (each call ends in its host read)

    def loop_decode():
        state["last"] = [c.small_decompress(s, out=dec_out) for s in state["streams"]][-1]

    batch_encode()
    loop_encode()
    o, oo, _ = state["enc"]
    assert torch.equal(torch.cat(state["streams"]), o[: int(oo[-1])]), "batch streams differ from the single calls'"
    batch_decode()
    assert torch.equal(back, xs)
    loop_decode()
    assert torch.equal(state["last"], bufs[-1])
    t = alternate({"batch_encode": batch_encode, "loop_encode": loop_encode, "batch_decode": batch_decode,
                   "loop_decode": loop_decode}, 5, timer=wall)
    emit(what="loop", count=count, block=K, wall_ms={k: v[0] for k, v in t.items()},
         min_max_ms={k: v[1] for k, v in t.items()},
         encode_speedup=round(t["loop_encode"][0] / t["batch_encode"][0], 1),
         decode_speedup=round(t["loop_decode"][0] / t["batch_decode"][0], 1))
    del out, back

if "mixed" in a.only:
    rng = np.random.default_rng(64)
    draw = np.exp(rng.uniform(math.log(64), math.log(65536), size=2 * n // 9000)).astype(np.int64)
    cut = int(np.searchsorted(np.cumsum(draw), n))
    lens = draw[:cut]
    lens = np.append(lens, n - int(lens.sum()))   # the rest of the text
    assert lens.sum() == n and lens.min() >= 1
    for order, ls in (("shuffled", lens), ("sorted", np.sort(lens))):
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(ls)]).astype(np.int64)).to(dev)
        batch_sides(off, int(lens.size), "mixed", order=order, min_len=int(ls.min()), max_len=int(ls.max()))
log.close()
