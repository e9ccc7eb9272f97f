"""The "DCHB" container of a Huffman batch (dc_huff_batch_seal / dc_huff_batch_open) on the 1 GiB
C2 text of bench.py (synth.device_text, seed 0xC2, n = 2, S = 64) as 262 144 x 4 KiB and as
16 384 x 64 KiB segments, one process. The variants of a comparison alternate inside every round;
every figure is the median of `--rounds` rounds of HIP-event windows of `--steps` calls with its
(min, max), the spread a call shows against itself.
  encode  Codec.encode_batch_blob (payload in place, directory, sync copy, header) against
          Codec.encode_batch of the same arguments: the difference is the price of the container.
          The stage list of one in-place call (dc_ctx_timings) is printed, and the tool asserts
          that it holds no `hbb_payload` stage: the in-place form does not copy the payload.
  seal    Codec.batch_seal in its copying form against dc_copy_probe of blob_bytes, as a ratio.
  open    Codec.batch_open against the decode_batch that follows it, for kinds 0, 1, 2 and 3.
  decode  decode_batch of the opened container against decode_batch of the original enc (the same
          kernels on the same arrays), and the original against itself: a difference beyond that
          spread is a finding.
  size    stored bytes per kind against the sum of the arrays a caller keeps without a container
          (29 B of mode, bits, pay_off, sync_off and the caller's offset per segment, 256 B of
          lens per segment or the records once, the payload, the u16 index, 1 B of tid, 4 B of
          CRC): the directory saves 20 B a segment and kind 1 a further 128.
Every container is opened, decoded and compared with the input before anything is timed. One JSON
line per result.
    timeout 900 python tools/blob_bench.py [--size BYTES] [--steps K] [--rounds R] | tee profiles/batch_blob.log
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
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--blocks", default="4096,65536")
a = ap.parse_args()
assert torch.cuda.is_available(), "blob_bench needs a GPU"
dev = "cuda:0"
c = Codec(0)
S = 64
KINDS = ("own", "own4", "shared", "set")


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


def alternating(fns, steps, rounds):
    """{name: (median ms, (min, max))} of the named calls, one window of each per round in turn"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(ev_ms(fn, steps))
    return {k: (round(statistics.median(v), 4), (round(min(v), 4), round(max(v), 4))) for k, v in t.items()}


def mode_kw(kind, x, offsets):
    if kind == "own":
        return {}
    if kind == "own4":
        return {"max_bits": 15}
    if kind == "shared":
        return {"table": c.batch_table(x, 2)}
    return {"table_set": c.batch_table_set(x, offsets, 4, 2)}


n = a.size
x = synth.device_text("C2", n, seed=0xC2, device=dev)
out = torch.empty(n, dtype=torch.uint8, device=dev)

for block in (int(b) for b in a.blocks.split(",")):
    offsets = c._block_offsets(x, block)
    count = offsets.numel() - 1
    for kind in KINDS:
        kw = dict(n_ary=2, sync_syms=S, checksum=True, **mode_kw(kind, x, offsets))
        lens4 = kind == "own4"
        enc = c.encode_batch(x, offsets, **kw)
        blob, info, status = c.encode_batch_blob(x, offsets, lens4=lens4, **kw)
        nbytes, cst = (int(v) for v in info.cpu())
        assert cst == 0 and c.batch_status() == 0, "the seal failed"
        blob_c, info_c, _ = c.batch_seal(enc, lens4=lens4)
        assert int(info_c.cpu()[0]) == nbytes and torch.equal(blob_c[:nbytes], blob[:nbytes]), "in place and copied differ"
        sealed = blob[:nbytes].clone()
        op = c.batch_open(sealed)
        c.decode_batch(op, out=out, verify=True)
        assert c.batch_status() == 0 and int(op["container_status"].cpu()[0]) == 0 and torch.equal(out, x), \
            "the opened container does not decode to the input"

        # size: the container against the arrays a caller keeps today
        pay, idx = int(enc["pay_off"][-1]), int(enc["sync_off"][-1])
        recs = {"own": 256 * count, "own4": 256 * count, "shared": 4 * 259, "set": 256 * 4 + count}[kind]
        loose = pay + 2 * idx + 29 * count + 4 * count + recs
        emit(what="size", block=block, kind=kind, count=count, blob_bytes=nbytes, loose_arrays_bytes=loose,
             saved_per_segment=round((loose - nbytes) / count, 2), payload_bytes=pay, sync_entries=idx,
             blob_bits_per_byte=round(8 * nbytes / n, 4))

        # encode: the container's price, and no payload copy in place
        t = alternating({"encode_batch": lambda: c.encode_batch(x, offsets, **kw),
                         "encode_batch_blob": lambda: c.encode_batch_blob(x, offsets, lens4=lens4, **kw)}, a.steps, a.rounds)
        c.timing(True)
        c.encode_batch_blob(x, offsets, lens4=lens4, **kw)
        stages = c.timings()
        c.timing(False)
        names = [s for s, _ in stages]
        assert "hbb_header" in names and "hbb_payload" not in names, "the in-place form launched a payload copy"
        emit(what="encode", block=block, kind=kind, encode_batch_ms=t["encode_batch"], encode_batch_blob_ms=t["encode_batch_blob"],
             container_ms=round(t["encode_batch_blob"][0] - t["encode_batch"][0], 4),
             stages={s: round(ms, 4) for s, ms in stages if s.startswith("hbb_")})

        # seal, copying, against the copy probe of blob_bytes
        n16 = nbytes // 16 * 16
        dst = torch.empty(n16, dtype=torch.uint8, device=dev)
        t = alternating({"seal_copy": lambda: c.batch_seal(enc, out=blob_c, lens4=lens4),
                         "copy_probe": lambda: c.copy_probe(sealed[:n16], dst)}, a.steps, a.rounds)
        emit(what="seal", block=block, kind=kind, seal_copy_ms=t["seal_copy"], copy_probe_ms=t["copy_probe"],
             ratio=round(t["seal_copy"][0] / t["copy_probe"][0], 3))

        # open against the decode that follows; the opened container against the original
        off0, off1 = enc["offsets"], op["offsets"]   # (both given: the default out_off costs a torch kernel a call)
        t = alternating({"open": lambda: c.batch_open(sealed),
                         "decode_opened": lambda: c.decode_batch(op, out=out, out_off=off1),
                         "decode_enc": lambda: c.decode_batch(enc, out=out, out_off=off0),
                         "decode_enc_again": lambda: c.decode_batch(enc, out=out, out_off=off0)}, a.steps, a.rounds)
        emit(what="open", block=block, kind=kind, open_ms=t["open"], decode_opened_ms=t["decode_opened"],
             open_over_decode=round(t["open"][0] / t["decode_opened"][0], 4))
        emit(what="decode", block=block, kind=kind, decode_opened_ms=t["decode_opened"], decode_enc_ms=t["decode_enc"],
             decode_enc_again_ms=t["decode_enc_again"],
             opened_minus_enc_ms=round(t["decode_opened"][0] - t["decode_enc"][0], 4),
             enc_against_itself_ms=round(abs(t["decode_enc_again"][0] - t["decode_enc"][0]), 4))
        del enc, blob, blob_c, sealed, op, dst
