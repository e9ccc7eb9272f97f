"""The checksum calls (dc_gpu.h "checksums") on the 1 GiB C2 text of bench.py (synth.device_text,
seed 0xC2), one process, HIP events, the sides of every comparison alternating inside each round:
  whole   dc_crc32 of the text (Codec.crc32) against the copy probe (Codec.copy_probe, the HBM
          reference rate of bench.py) on the same box
  batch   the text as 262 144 x 4 KiB and as 16 384 x 64 KiB buffers: crc32_batch and
          crc32_verify_batch of it against the shared-table decode_batch of the same batch (n = 2,
          S = 64, Codec.batch_table), and decode_batch(verify=True) against verify=False
Every value is checked before it is timed: the whole CRC against zlib.crc32 of the text on the
host, the batch CRCs against zlib on a sample and, folded with dc_crc32_combine, against the whole
CRC. Each timed window is at least 20 ms of calls; each figure is the median of `--rounds` rounds
with its (min, max). The usefulness bar (a check that costs more than the decode it follows will not
be switched on): verify_ms <= decode_ms at both shapes; the result line says whether it holds.
One JSON line per result, on stdout and in `--log` (default profiles/crc32.log).
    timeout 600 python tools/crc_bench.py [--size BYTES] [--rounds R] [--log PATH]
"""
import argparse
import json
import os
import statistics
import sys
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from data_compression_amd import synth  # noqa: E402
from data_compression_amd.device import Codec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--log", default=os.path.join(REPO, "profiles", "crc32.log"))
a = ap.parse_args()
assert torch.cuda.is_available(), "crc_bench needs a GPU"
dev = "cuda:0"
c = Codec(0)
S = 64
log = open(a.log, "w")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def ev_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def timed(fns):
    """{name: median ms}, {name: (min, max)}, {name: steps}: the sides alternating, windows of >= 20 ms."""
    steps = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        steps[k] = max(3, min(400, int(20.0 / max(ev_ms(fn, 2), 1e-3)) + 1))
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(ev_ms(fn, steps[k]))
    return ({k: round(statistics.median(v), 4) for k, v in t.items()},
            {k: (round(min(v), 4), round(max(v), 4)) for k, v in t.items()}, steps)


n = a.size
x = synth.device_text("C2", n, seed=0xC2, device=dev)
host = x.cpu().numpy()
whole = zlib.crc32(host)
out = torch.empty(n, dtype=torch.uint8, device=dev)

# ---- whole: one buffer over the whole device ----------------------------------------------------
got = int(c.crc32(x).cpu().numpy()[0])
assert got == whole, ("dc_crc32 differs from zlib.crc32", hex(got), hex(whole))
med, mm, steps = timed({"crc32": lambda: c.crc32(x), "copy_probe": lambda: c.copy_probe(x, out)})
emit(what="whole", n=n, crc=hex(whole), piece=Codec.CRC_PIECE, ms=med, min_max_ms=mm, steps=steps,
     crc32_read_GBps=round(n / med["crc32"] / 1e6, 1), copy_read_plus_write_GBps=round(2 * n / med["copy_probe"] / 1e6, 1),
     crc32_over_copy=round(med["crc32"] / med["copy_probe"], 3))

# ---- batch: the buffers a user stores and reads back --------------------------------------------
tab = c.batch_table(x, n_ary=2)
bar = {}
for block in (4096, 65536):
    count = (n + block - 1) // block
    enc = c.encode_blocks(x, block=block, n_ary=2, sync_syms=S, table=tab, checksum=True)
    assert c.batch_status() == 0
    off = enc["offsets"]
    crc_h = enc["crc"].cpu().numpy()
    for i in list(range(0, count, max(count // 64, 1))) + [count - 1]:
        assert int(crc_h[i]) == zlib.crc32(host[i * block: (i + 1) * block]), ("crc32_batch differs from zlib", block, i)
    fold = 0
    for i in range(count):
        fold = c.L.dc_crc32_combine(fold, int(crc_h[i]), min(block, n - i * block))
    assert fold == whole, ("the batch CRCs do not combine to the whole CRC", block)
    out.zero_()
    c.decode_batch(enc, out=out, out_off=off, verify=True)
    assert c.batch_status() == 0 and torch.equal(out, x), "verified round trip differs from the input"
    status = torch.zeros(count, dtype=torch.int32, device=dev)
    fns = {"crc32_batch": lambda: c.crc32_batch(x, offsets=off),
           "verify": lambda: c.crc32_verify_batch(out, enc["crc"], status, offsets=off),
           "decode": lambda: c.decode_batch(enc, out=out, out_off=off),
           "decode_verify": lambda: c.decode_batch(enc, out=out, out_off=off, verify=True)}
    med, mm, steps = timed(fns)
    assert c.batch_status() == 0
    bar[block] = med["verify"] <= med["decode"]
    emit(what="batch", block=block, count=count, table="shared", ms=med, min_max_ms=mm, steps=steps,
         crc32_batch_GBps=round(n / med["crc32_batch"] / 1e6, 1), verify_GBps=round(n / med["verify"] / 1e6, 1),
         verify_over_decode=round(med["verify"] / med["decode"], 3),
         decode_verify_over_decode=round(med["decode_verify"] / med["decode"], 3), verify_within_decode=bar[block])
    del enc
emit(what="bar", rule="verify_ms <= shared-table decode_ms at both shapes", holds=all(bar.values()), by_block=bar)
