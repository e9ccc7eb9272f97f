"""The batched nybble codec (dc_nyb_compress_batch / dc_nyb_decompress_batch_async) on the first
256 MiB of bench.py's nybble text (synth.device_text C1, seed 0xC1), one process:
  blocks  65 536 x 4 KiB, static and adaptive: the batch encode against dc_nyb_compress_chunked at
          K = 4096 (the DCNK container of the same streams) and the asynchronous decode against
          dc_nyb_decompress_batch; HIP events around each call, the two sides alternating, the
          median of `--rounds` rounds after a warm-up; DCNK against itself the same way gives the
          spread of such a comparison; and the per-kernel split of one call (dc_ctx_timings)
  loop    4096 x 4 KiB: one batch call each way against the loop of Codec.nyb_compress /
          nyb_decompress over the same buffers (all a caller could do before), wall clock around
          calls that end synchronised, alternating; asserts that the batch calls are faster
  mixed   the same 256 MiB cut into lengths log-uniform in 64 B .. 64 KiB, once in drawn
          (shuffled) order and once sorted by length: what a wave's waiting for its longest
          buffer costs, and what sorting buys
Every output is checked for equality before it is timed. One JSON line per result, to stdout and
appended to --log (default profiles/nyb_batch.log).
    timeout 900 python tools/nyb_batch_bench.py [--rounds R] [--only blocks,loop,mixed] [--log FILE]
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
ap.add_argument("--log", default=os.path.join(REPO, "profiles", "nyb_batch.log"))
a = ap.parse_args()
assert a.rounds >= 5, "at least 5 repetitions"
assert torch.cuda.is_available(), "nyb_batch_bench needs a GPU"
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


def container_parts(box, nch):
    """(offsets int64 [nch + 1], payload) of a DCNK container (32-B header, u64 offsets, payload)."""
    return box[32: 32 + 8 * (nch + 1)].view(torch.int64).clone(), box[32 + 8 * (nch + 1):]


n = a.size
x = synth.device_text("C1", 1 << 30, seed=0xC1, device=dev)[:n].clone()   # the first 256 MiB of the bench's text
torch.cuda.synchronize()

if "blocks" in a.only:
    count = (n + K - 1) // K
    off = torch.arange(0, n + K, K, dtype=torch.int64, device=dev).clamp_(max=n)[: count + 1].contiguous()
    out = torch.empty(c.nyb_batch_bound(n, count), dtype=torch.uint8, device=dev)
    back = torch.empty(n, dtype=torch.uint8, device=dev)
    for modify in (False, True):
        mode = "adaptive" if modify else "static"
        box = c.nyb_compress_chunked(x, modify, K)
        c_off, payload = container_parts(box, count)
        _, oo, st = c.nyb_compress_batch(x, off, modify, out=out)
        total = int(oo[-1])
        assert c.batch_status() == 0 and torch.equal(oo, c_off) and torch.equal(out[:total], payload), \
            "the batch streams differ from the DCNK container's"
        comp = out[:total].clone()
        back.zero_()
        _, st = c.nyb_decompress_batch_into(comp, oo, modify, off, out=back)
        assert c.batch_status() == 0 and torch.equal(back, x), "the asynchronous decode differs from the input"
        old, old_off = c.nyb_decompress_batch(comp, oo, modify, out_cap=n)
        assert torch.equal(old, x) and torch.equal(old_off, off)
        del old, box
        emit(what="blocks_size", mode=mode, count=count, block=K, bytes=n, compressed_bytes=total)

        def dcnk():
            c.nyb_compress_chunked(x, modify, K)

        enc = alternate({"batch": lambda: c.nyb_compress_batch(x, off, modify, out=out), "dcnk": dcnk}, a.rounds)
        self_ = alternate({"dcnk_a": dcnk, "dcnk_b": dcnk}, a.rounds)
        spread = round(abs(self_["dcnk_a"][0] - self_["dcnk_b"][0]) / min(self_["dcnk_a"][0], self_["dcnk_b"][0]), 4)
        emit(what="blocks_encode", mode=mode, count=count, block=K, batch_ms=enc["batch"][0], dcnk_ms=enc["dcnk"][0],
             batch_GBps=round(n / enc["batch"][0] / 1e6, 1), dcnk_GBps=round(n / enc["dcnk"][0] / 1e6, 1),
             batch_over_dcnk=round(enc["batch"][0] / enc["dcnk"][0], 3), batch_min_max_ms=enc["batch"][1],
             dcnk_min_max_ms=enc["dcnk"][1], dcnk_vs_itself_ms=[self_["dcnk_a"][0], self_["dcnk_b"][0]],
             dcnk_vs_itself_min_max_ms=[self_["dcnk_a"][1], self_["dcnk_b"][1]], dcnk_vs_itself_spread=spread)
        dec = alternate({"async": lambda: c.nyb_decompress_batch_into(comp, oo, modify, off, out=back),
                         "sync": lambda: c.nyb_decompress_batch(comp, oo, modify, out_cap=n)}, a.rounds)
        emit(what="blocks_decode", mode=mode, count=count, block=K, async_ms=dec["async"][0], sync_ms=dec["sync"][0],
             async_GBps=round(n / dec["async"][0] / 1e6, 1), sync_GBps=round(n / dec["sync"][0] / 1e6, 1),
             async_over_sync=round(dec["async"][0] / dec["sync"][0], 3), async_min_max_ms=dec["async"][1],
             sync_min_max_ms=dec["sync"][1])

        def one_of_each():
            c.nyb_compress_batch(x, off, modify, out=out)
            c.nyb_compress_chunked(x, modify, K)
            c.nyb_decompress_batch_into(comp, oo, modify, off, out=back)
            c.nyb_decompress_batch(comp, oo, modify, out_cap=n)

        emit(what="blocks_stages", mode=mode, ms=stages(one_of_each))
        del comp
    del out, back

if "loop" in a.only:
    count = 4096
    m = count * K
    xs = x[:m]
    bufs = [xs[i * K: (i + 1) * K] for i in range(count)]
    off = torch.arange(0, m + K, K, dtype=torch.int64, device=dev)[: count + 1].contiguous()
    out = torch.empty(c.nyb_batch_bound(m, count), dtype=torch.uint8, device=dev)
    back = torch.empty(m, dtype=torch.uint8, device=dev)
    one_out = torch.empty(2 * K + 16, dtype=torch.uint8, device=dev)
    for modify in (False, True):
        state = {}

        def batch_encode():
            state["enc"] = c.nyb_compress_batch(xs, off, modify, out=out)
            assert c.batch_status() == 0

        def batch_decode():
            c.nyb_decompress_batch_into(state["enc"][0], state["enc"][1], modify, off, out=back)
            assert c.batch_status() == 0

        def loop_encode():
            state["streams"] = [c.nyb_compress(b, modify) for b in bufs]   # (each call ends in its host read)

        def loop_decode():
            state["last"] = [c.nyb_decompress(s, modify, out=one_out) for s in state["streams"]][-1]

        def wall(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

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
        emit(what="loop", mode="adaptive" if modify else "static", count=count, block=K,
             wall_ms={k: v[0] for k, v in t.items()}, min_max_ms={k: v[1] for k, v in t.items()},
             encode_speedup=round(t["loop_encode"][0] / t["batch_encode"][0], 1),
             decode_speedup=round(t["loop_decode"][0] / t["batch_decode"][0], 1))
        assert t["batch_encode"][0] < t["loop_encode"][0] and t["batch_decode"][0] < t["loop_decode"][0], \
            "the batch call is not faster than the loop of single-stream calls"
    del out, back

if "mixed" in a.only:
    rng = np.random.default_rng(64)
    draw = np.exp(rng.uniform(math.log(64), math.log(65536), size=2 * n // 9000)).astype(np.int64)
    cut = int(np.searchsorted(np.cumsum(draw), n))
    lens = draw[:cut]
    lens = np.append(lens, n - int(lens.sum()))   # the rest of the text
    assert lens.sum() == n and lens.min() >= 1
    count = lens.size
    out = torch.empty(c.nyb_batch_bound(n, count), dtype=torch.uint8, device=dev)
    back = torch.empty(n, dtype=torch.uint8, device=dev)
    for order, ls in (("shuffled", lens), ("sorted", np.sort(lens))):
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(ls)]).astype(np.int64)).to(dev)
        for modify in (False, True):
            _, oo, st = c.nyb_compress_batch(x, off, modify, out=out)
            total = int(oo[-1])
            assert c.batch_status() == 0
            comp = out[:total].clone()
            back.zero_()
            c.nyb_decompress_batch_into(comp, oo, modify, off, out=back)
            assert c.batch_status() == 0 and torch.equal(back, x), "mixed lengths: round trip differs from the input"
            t = alternate({"encode": lambda: c.nyb_compress_batch(x, off, modify, out=out),
                           "decode": lambda: c.nyb_decompress_batch_into(comp, oo, modify, off, out=back)}, a.rounds)
            emit(what="mixed", order=order, mode="adaptive" if modify else "static", count=int(count), bytes=n,
                 min_len=int(ls.min()), max_len=int(ls.max()), compressed_bytes=total, encode_ms=t["encode"][0],
                 decode_ms=t["decode"][0], encode_GBps=round(n / t["encode"][0] / 1e6, 1),
                 decode_GBps=round(n / t["decode"][0] / 1e6, 1), encode_min_max_ms=t["encode"][1],
                 decode_min_max_ms=t["decode"][1], stages_ms=stages(lambda: (
                     c.nyb_compress_batch(x, off, modify, out=out),
                     c.nyb_decompress_batch_into(comp, oo, modify, off, out=back))))
            del comp
log.close()
