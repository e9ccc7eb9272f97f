"""The batched Huffman codec (dc_huff_encode_batch / dc_huff_decode_batch) on the 1 GiB C2 text
of bench.py (synth.device_text, seed 0xC2, n = 2, S = 64), one process:
  blocks  the text as 16 384 x 64 KiB and as 262 144 x 4 KiB independent segments: encode and
          decode ms and GB/s (HIP events around `--steps` calls, the median of `--rounds` rounds),
          the per-stage split of one call (dc_ctx_timings), and the compressed size against the
          single-table stream of the same text
  loop    4096 x 4 KiB: the batch call against the loop of Codec.encode / decode_into over the
          same segments (all a caller could do before), wall clock around calls that end
          synchronised, the two sides alternating; asserts that the batch call is faster
  shared  the same blocks under ONE table of the whole text (Codec.batch_table, encode_blocks(...,
          table=)): encode and decode ms, the stage split, and the stored size (payload + u16
          index + 5 B per segment + the table's lengths once) beside the own-table size; then at
          4 KiB the own-table call against the shared call, alternating in this process; asserts
          that the shared encode and decode are each faster and that the shared form is smaller
Every result is checked against the input before it is timed. One JSON line per result.
    timeout 900 python tools/batch_bench.py [--size BYTES] [--steps K] [--rounds R] [--only blocks,loop,shared]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from data_compression_amd import synth  # noqa: E402
from data_compression_amd.device import Codec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", default="blocks,loop,shared")
a = ap.parse_args()
assert torch.cuda.is_available(), "batch_bench needs a GPU"
dev = "cuda:0"
c = Codec(0)
S = 64


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


def median_ms(fn, steps, rounds):
    fn()
    torch.cuda.synchronize()
    t = [ev_ms(fn, steps) for _ in range(rounds)]
    return statistics.median(t), (min(t), max(t))


n = a.size
x = synth.device_text("C2", n, seed=0xC2, device=dev)

if "blocks" in a.only:
    single = c.encode(x, n_ary=2, sync_syms=S)
    single_bytes = (single["bits"] + 7) // 8 + c.table_bytes + 2 * single["sync"][1].numel() + 8 * single["sync"][0].numel()
    emit(what="single_table_stream", n=n, payload_bytes=(single["bits"] + 7) // 8, with_table_and_index=single_bytes)
    del single
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    for block in (65536, 4096):
        count = (n + block - 1) // block
        pb, sb = c.batch_bounds(n, count, S)
        payload = torch.empty(pb, dtype=torch.uint8, device=dev)
        sync = torch.empty(sb, dtype=torch.int16, device=dev)
        enc = c.encode_blocks(x, block=block, n_ary=2, sync_syms=S, payload=payload, sync_len=sync)
        assert c.batch_status() == 0
        off = enc["offsets"]
        c.decode_batch(enc, out=out, out_off=off)
        assert c.batch_status() == 0 and torch.equal(out, x), "batch round trip differs from the input"
        pay = int(enc["pay_off"][-1])
        idx = int(enc["sync_off"][-1])
        # what a container would store per segment: lens (256), mode (1), bits (4), the payload, the u16 index
        stored = pay + 2 * idx + count * (256 + 1 + 4)
        emit(what="blocks_size", block=block, count=count, payload_bytes=pay, sync_entries=idx, with_records_and_index=stored,
             huffman_segments=int(enc["mode"].sum()), payload_bits_per_byte=round(8 * pay / n, 4))
        e_ms, e_mm = median_ms(lambda: c.encode_blocks(x, block=block, n_ary=2, sync_syms=S, payload=payload, sync_len=sync),
                               a.steps, a.rounds)
        d_ms, d_mm = median_ms(lambda: c.decode_batch(enc, out=out, out_off=off), a.steps, a.rounds)
        emit(what="blocks_time", block=block, count=count, encode_ms=round(e_ms, 3), encode_GBps=round(n / e_ms / 1e6, 1),
             decode_ms=round(d_ms, 3), decode_GBps=round(n / d_ms / 1e6, 1), encode_min_max_ms=e_mm, decode_min_max_ms=d_mm)
        c.timing(True)
        c.encode_blocks(x, block=block, n_ary=2, sync_syms=S, payload=payload, sync_len=sync)
        c.decode_batch(enc, out=out, out_off=off)
        emit(what="blocks_stages", block=block, ms={k: round(v, 4) for k, v in c.timings()})
        c.timing(False)
        del enc, payload, sync
    del out

if "loop" in a.only:
    count, block = 4096, 4096
    m = count * block
    xs = x[:m]
    segs = [xs[i * block: (i + 1) * block] for i in range(count)]
    out = torch.empty(m, dtype=torch.uint8, device=dev)
    outs = [out[i * block: (i + 1) * block] for i in range(count)]
    pb, sb = c.batch_bounds(m, count, S)
    payload = torch.empty(pb, dtype=torch.uint8, device=dev)
    sync = torch.empty(sb, dtype=torch.int16, device=dev)
    state = {}

    def batch_encode():
        state["enc"] = c.encode_blocks(xs, block=block, n_ary=2, sync_syms=S, payload=payload, sync_len=sync)
        assert c.batch_status() == 0

    def batch_decode():
        c.decode_batch(state["enc"], out=out, out_off=state["enc"]["offsets"])
        assert c.batch_status() == 0

    def loop_encode():
        state["encs"] = [c.encode(s, n_ary=2, sync_syms=S) for s in segs]
        torch.cuda.synchronize()

    def loop_decode():
        for e, o in zip(state["encs"], outs):
            c.decode_into(e, o)
        assert c.decode_status() == 0

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    batch_encode()
    batch_decode()
    assert torch.equal(out, xs)
    out.zero_()
    loop_encode()
    loop_decode()
    assert torch.equal(out, xs)
    t = {k: [] for k in ("batch_encode", "loop_encode", "batch_decode", "loop_decode")}
    for _ in range(3):
        t["batch_encode"].append(wall(batch_encode))
        t["loop_encode"].append(wall(loop_encode))
        t["batch_decode"].append(wall(batch_decode))
        t["loop_decode"].append(wall(loop_decode))
    med = {k: round(statistics.median(v), 3) for k, v in t.items()}
    emit(what="loop", count=count, block=block, wall_ms=med, all_ms={k: [round(v, 3) for v in vs] for k, vs in t.items()},
         encode_speedup=round(med["loop_encode"] / med["batch_encode"], 1),
         decode_speedup=round(med["loop_decode"] / med["batch_decode"], 1))
    assert med["batch_encode"] < med["loop_encode"] and med["batch_decode"] < med["loop_decode"], \
        "the batch call is not faster than the loop of single-stream calls"

if "shared" in a.only:
    tab = c.batch_table(x, n_ary=2)
    lengths = c.table_get_lengths(tab)
    assert lengths.max() <= 255   # a byte each in a container
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    for block in (65536, 4096):
        count = (n + block - 1) // block
        pb, sb = c.batch_bounds(n, count, S)
        bufs = {k: (torch.empty(pb, dtype=torch.uint8, device=dev), torch.empty(sb, dtype=torch.int16, device=dev))
                for k in ("own", "shared")}

        def encode(kind):
            return c.encode_blocks(x, block=block, n_ary=2, sync_syms=S, payload=bufs[kind][0], sync_len=bufs[kind][1],
                                   **({"table": tab} if kind == "shared" else {}))

        encs, size = {}, {}
        for kind in ("own", "shared"):
            enc = encs[kind] = encode(kind)
            assert c.batch_status() == 0
            out.zero_()
            c.decode_batch(enc, out=out, out_off=enc["offsets"])
            assert c.batch_status() == 0 and torch.equal(out, x), kind + ": batch round trip differs from the input"
            pay, idx = int(enc["pay_off"][-1]), int(enc["sync_off"][-1])
            # per segment: mode (1), bits (4), the payload, the u16 index; a lens record (256) each, or the lengths once
            size[kind] = pay + 2 * idx + count * 5 + (count * 256 if kind == "own" else lengths.size)
            emit(what="shared_size", table=kind, block=block, count=count, payload_bytes=pay, sync_entries=idx,
                 stored_bytes=size[kind], huffman_segments=int(enc["mode"].sum()), payload_bits_per_byte=round(8 * pay / n, 4))
        emit(what="shared_vs_own_size", block=block, own=size["own"], shared=size["shared"],
             shared_smaller_pct=round(100 * (1 - size["shared"] / size["own"]), 2))
        off = encs["shared"]["offsets"]
        e_ms, e_mm = median_ms(lambda: encode("shared"), a.steps, a.rounds)
        d_ms, d_mm = median_ms(lambda: c.decode_batch(encs["shared"], out=out, out_off=off), a.steps, a.rounds)
        emit(what="shared_time", block=block, count=count, encode_ms=round(e_ms, 3), encode_GBps=round(n / e_ms / 1e6, 1),
             decode_ms=round(d_ms, 3), decode_GBps=round(n / d_ms / 1e6, 1), encode_min_max_ms=e_mm, decode_min_max_ms=d_mm)
        c.timing(True)
        encode("shared")
        c.decode_batch(encs["shared"], out=out, out_off=off)
        emit(what="shared_stages", block=block, ms={k: round(v, 4) for k, v in c.timings()})
        c.timing(False)
        if block == 4096:   # the yardstick: the own-table call of this build, the two sides alternating
            fns = {"own_encode": lambda: encode("own"), "shared_encode": lambda: encode("shared"),
                   "own_decode": lambda: c.decode_batch(encs["own"], out=out, out_off=off),
                   "shared_decode": lambda: c.decode_batch(encs["shared"], out=out, out_off=off)}
            t = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    t[k].append(ev_ms(fn, a.steps))
            med = {k: round(statistics.median(v), 3) for k, v in t.items()}
            emit(what="shared_vs_own_time", block=block, count=count, ms=med,
                 min_max_ms={k: (round(min(v), 3), round(max(v), 3)) for k, v in t.items()},
                 encode_speedup=round(med["own_encode"] / med["shared_encode"], 2),
                 decode_speedup=round(med["own_decode"] / med["shared_decode"], 2))
            assert med["shared_encode"] < med["own_encode"], "the shared-table encode is not faster than the own-table encode"
            assert med["shared_decode"] < med["own_decode"], "the shared-table decode is not faster than the own-table decode"
            assert size["shared"] < size["own"], "the shared-table form is not smaller than the own-table form"
        del encs, bufs
    del out
