"""Length-limited tables (dc_huff_*_limit; DESIGN.md "Length-limited tables") on the 1 GiB C2 text of
bench.py (synth.device_text, seed 0xC2, n = 2), one process, the unlimited, 15-bit and 12-bit
tables alternating inside every round:
  table   the table launch alone (dc_huff_table against dc_huff_table_limit on the same histogram)
  stream  payload bytes, longest code, encode and decode ms of the whole stream at S = 64 (the fast
          decoder), the redo count of the decode, and the kernels' own times of one encode + decode
  batch   the text as 262 144 x 4 KiB segments under one shared table trained on its first 1/64:
          unlimited, 15 and 12 bits, each with and without cover: stored segments, payload bytes,
          encode and decode ms
Device times are HIP events around `--steps` calls, the median of `--rounds` rounds. Every decode is
compared with the input once. Prints one JSON line per result.
    timeout 600 python tools/limit_bench.py [--size BYTES] [--steps K] [--rounds R] [--only table,stream,batch]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from data_compression_amd import synth  # noqa: E402
from data_compression_amd.device import Codec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--only", default="table,stream,batch")
a = ap.parse_args()
assert torch.cuda.is_available(), "limit_bench needs a GPU"
dev = "cuda:0"
c = Codec(0)
CAPS = (None, 15, 12)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def name(cap, cover=False):
    return ("unlimited" if cap is None else f"{cap}bit") + ("+cover" if cover else "")


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
    return ({k: round(statistics.median(v), 4) for k, v in t.items()},
            {k: (round(min(v), 4), round(max(v), 4)) for k, v in t.items()})


n = a.size
x = synth.device_text("C2", n, seed=0xC2, device=dev)
out = torch.empty(n, dtype=torch.uint8, device=dev)

if "table" in a.only:
    hist = c.hist(x)
    tabs = {cap: c.alloc_table() for cap in CAPS}
    med, spread = alternate({name(cap): (lambda cap=cap: c.table(hist, 2, out=tabs[cap], max_bits=cap)) for cap in CAPS},
                            max(a.steps, 50), a.rounds)
    emit(what="table_launch", ms=med, min_max_ms=spread,
         longest_code={name(cap): c.table_status(tabs[cap])[1] for cap in CAPS})

if "stream" in a.only:
    S = 64
    encs = {cap: c.encode(x, n_ary=2, sync_syms=S, max_bits=cap) for cap in CAPS}
    for cap, enc in encs.items():
        out.zero_()
        c.decode_into(enc, out)
        assert c.decode_status() == 0 and torch.equal(out, x), f"{name(cap)}: the decode differs from the input"
        emit(what="stream", table=name(cap), n=n, S=S, payload_bytes=(enc["bits"] + 7) // 8,
             bits_per_byte=round(enc["bits"] / n, 5), longest_code=c.table_status(enc["table"])[1],
             redo_chunks=c.decode_redo_count(), chunks=(n + S - 1) // S,
             payload_vs_unlimited_pct=round(100 * (enc["bits"] / encs[None]["bits"] - 1), 4))
    fns = {}
    for cap in CAPS:
        fns["encode_" + name(cap)] = lambda cap=cap: c.encode(x, n_ary=2, sync_syms=S, max_bits=cap)
        fns["decode_" + name(cap)] = lambda cap=cap: c.decode_into(encs[cap], out)
    med, spread = alternate(fns, a.steps, a.rounds)
    emit(what="stream_time", ms=med, min_max_ms=spread,
         decode_15bit_over_unlimited=round(med["decode_15bit"] / med["decode_unlimited"], 4),
         decode_12bit_over_unlimited=round(med["decode_12bit"] / med["decode_unlimited"], 4))
    for cap in CAPS:   # the kernels' own times (events around each launch: slower end to end, so apart)
        c.timing(True)
        c.encode(x, n_ary=2, sync_syms=S, max_bits=cap)
        c.decode_into(encs[cap], out)
        emit(what="stream_kernels", table=name(cap), ms={k: round(v, 4) for k, v in c.timings()})
        c.timing(False)
    del encs

if "batch" in a.only:
    block, S = 4096, 64
    count = (n + block - 1) // block
    sample = x[: max(n >> 6, block)]
    pb, sb = c.batch_bounds(n, count, S)
    payload = torch.empty(pb, dtype=torch.uint8, device=dev)
    sync = torch.empty(sb, dtype=torch.int16, device=dev)
    encs, fns = {}, {}
    for cover in (False, True):
        for cap in CAPS:
            k = name(cap, cover)
            tab = c.batch_table(sample, n_ary=2, max_bits=cap, cover=cover)

            def encode(tab=tab):
                return c.encode_blocks(x, block, n_ary=2, sync_syms=S, payload=payload, sync_len=sync, table=tab)

            enc = encode()
            assert c.batch_status() == 0
            out.zero_()
            c.decode_batch(enc, out=out, out_off=enc["offsets"])
            assert c.batch_status() == 0 and torch.equal(out, x), f"{k}: the batch decode differs from the input"
            emit(what="batch", table=k, count=count, block=block, sample_bytes=sample.numel(),
                 longest_code=c.table_status(tab)[1], stored_segments=int((enc["mode"] == 0).sum().item()),
                 payload_bytes=int(enc["pay_off"][-1].item()))
            # each table keeps an encode of its own for the decode timing
            own = {"payload": torch.empty(pb, dtype=torch.uint8, device=dev), "sync": torch.empty(sb, dtype=torch.int16, device=dev)}
            encs[k] = c.encode_blocks(x, block, n_ary=2, sync_syms=S, payload=own["payload"], sync_len=own["sync"], table=tab)
            fns["encode_" + k] = encode
            fns["decode_" + k] = lambda k=k: c.decode_batch(encs[k], out=out, out_off=encs[k]["offsets"])
    med, spread = alternate(fns, a.steps, a.rounds)
    emit(what="batch_time", ms=med, min_max_ms=spread)
