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
  ranges  (only on request) random 256-byte ranges of the blocks under the shared table, one
          decode_batch_ranges call against all a caller could do before: the whole-segment scatter
          decode of exactly the distinct segments the ranges touch (the others are skipped the
          one way the API has, an output range that ends before it starts: nothing of them is read,
          but each is visited and takes the failure path, a status store and an atomicMin on the
          call's first-failure word, which at 4 KiB blocks and few ranges is most of the time), then
          the wanted bytes sliced out by a precomputed index. The two sides alternate, the median of
          `--rounds` rounds of HIP-event windows of at least 20 ms; asserts that at 4096 ranges of
          the 64 KiB blocks the range call is faster. Then own tables at 65536 ranges, sorted by
          segment and not, and Codec.decode_ranges on the single stream of the same text.
  limit   (only on request) own tables capped per segment (encode_blocks(..., max_bits=)): the
          unlimited, 15-bit and 12-bit batches of both block sizes alternating inside every round.
          Per table: the whole encode and the decode (HIP-event windows), the plan and pack
          kernels' own times (dc_ctx_timings, one call a round), the payload bytes, how many
          segments the cap binds in (their unlimited record is deeper) and how many come out
          stored, the stored size with 256-byte and with 128-byte lens records, and the
          batch_lens_pack / batch_lens_unpack times. Every figure is the median of `--rounds`
          rounds with its (min, max): the spread a call shows against itself.
  set     (only on request) a table set (encode_blocks(..., table_set=)) between the two: on
          corpus (a), the C2 text, and on corpus (b), a mixed corpus of the same size in regions
          of 16 MiB (enwik-like, english-like, log-like, zipf bytes, hex digits, uniform bytes, in
          turn), both block sizes, four rows each: own tables, one shared table of the whole
          corpus, and sets of K = 4 and K = 16 trained by Codec.batch_table_set (its wall time is
          in the row). The four rows alternate inside every round. Per row: the whole encode and
          the decode (HIP-event windows), the plan and pack kernels' own times (dc_ctx_timings, one
          call a round), the payload bytes and the stored bytes (payload + u16 index + 5 B per
          segment, plus 256 B of lens per segment, or the table's lengths once, or 1 B of tid per
          segment and the K records once, 128 B each when they pack as nybbles); for a set, how
          many coded segments chose each record and how many were stored. Then per corpus and
          block size the set rows against the own-table and the shared-table rows.
Every result is checked against the input before it is timed. One JSON line per result.
    timeout 900 python tools/batch_bench.py [--size BYTES] [--steps K] [--rounds R] [--only blocks,loop,shared]
    timeout 900 python tools/batch_bench.py --only ranges
    timeout 900 python tools/batch_bench.py --only limit
    timeout 900 python tools/batch_bench.py --only set
"""
import argparse
import ctypes
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

if "limit" in a.only:
    CAPS = (None, 15, 12)
    cap_name = lambda cap: "unlimited" if cap is None else f"{cap}bit"
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    for block in (65536, 4096):
        count = (n + block - 1) // block
        pb, sb = c.batch_bounds(n, count, S)
        bufs = {cap: (torch.empty(pb, dtype=torch.uint8, device=dev), torch.empty(sb, dtype=torch.int16, device=dev))
                for cap in CAPS}

        def encode(cap):
            return c.encode_blocks(x, block=block, n_ary=2, sync_syms=S, payload=bufs[cap][0], sync_len=bufs[cap][1],
                                   max_bits=cap)

        encs, packed = {}, {}
        for cap in CAPS:
            enc = encs[cap] = encode(cap)
            assert c.batch_status() == 0
            lens4, st = c.batch_lens_pack(enc)
            packs = c.batch_status() == 0
            back = c.batch_lens_unpack(lens4)
            assert not packs or torch.equal(back, enc["lens"]), "the nybble records do not unpack to the lens records"
            assert packs or cap is None, "a record capped at 15 bits or fewer did not pack"
            out.zero_()
            c.decode_batch(dict(enc, lens=back) if packs else enc, out=out, out_off=enc["offsets"])   # from the stored form
            assert c.batch_status() == 0 and torch.equal(out, x), cap_name(cap) + ": batch round trip differs from the input"
            packed[cap] = lens4
            pay, idx = int(enc["pay_off"][-1]), int(enc["sync_off"][-1])
            depth = encs[None]["lens"].max(dim=1).values
            emit(what="limit_size", table=cap_name(cap), block=block, count=count, payload_bytes=pay,
                 payload_vs_unlimited_pct=round(100 * (pay / int(encs[None]["pay_off"][-1]) - 1), 4),
                 deepest_record=int(enc["lens"].max()), binding_segments=0 if cap is None else int((depth > cap).sum()),
                 stored_segments=int((enc["mode"] == 0).sum()), records_pack=packs,
                 unpackable_records=int((st != 0).sum()),
                 stored_bytes_lens256=pay + 2 * idx + count * (5 + 256), stored_bytes_lens128=pay + 2 * idx + count * (5 + 128))
        fns = {}
        for cap in CAPS:
            k = cap_name(cap)
            fns["encode_" + k] = lambda cap=cap: encode(cap)
            fns["decode_" + k] = lambda cap=cap: c.decode_batch(encs[cap], out=out, out_off=encs[cap]["offsets"])
            fns["lens_pack_" + k] = lambda cap=cap: c.batch_lens_pack(encs[cap])
            fns["lens_unpack_" + k] = lambda cap=cap: c.batch_lens_unpack(packed[cap])
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        stages = {cap_name(cap): {} for cap in CAPS}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(ev_ms(fn, a.steps))
            for cap in CAPS:   # the kernels' own times (events around each launch: slower end to end, so apart)
                c.timing(True)
                encode(cap)
                for name, ms in c.timings():
                    stages[cap_name(cap)].setdefault(name.replace("_limit", ""), []).append(ms)
                c.timing(False)
        med = {k: round(statistics.median(v), 4) for k, v in t.items()}
        emit(what="limit_time", block=block, count=count, ms=med,
             min_max_ms={k: (round(min(v), 4), round(max(v), 4)) for k, v in t.items()},
             decode_15bit_over_unlimited=round(med["decode_15bit"] / med["decode_unlimited"], 4),
             decode_12bit_over_unlimited=round(med["decode_12bit"] / med["decode_unlimited"], 4),
             encode_15bit_over_unlimited=round(med["encode_15bit"] / med["encode_unlimited"], 4),
             encode_12bit_over_unlimited=round(med["encode_12bit"] / med["encode_unlimited"], 4))
        emit(what="limit_stages", block=block, count=count,
             ms={k: {s: round(statistics.median(v), 4) for s, v in d.items()} for k, d in stages.items()},
             min_max_ms={k: {s: (round(min(v), 4), round(max(v), 4)) for s, v in d.items()} for k, d in stages.items()})
        del encs, bufs, packed
    del out

if "set" in a.only.split(","):
    REGION = 16 << 20

    def mixed(n):
        """Corpus (b): regions of REGION bytes of six kinds in turn, made on the device."""
        nreg = (n + REGION - 1) // REGION
        kinds = ("C2", "C1", "C5", "C4", "hex", "C3")
        per = (nreg + len(kinds) - 1) // len(kinds)
        out = torch.empty(nreg * REGION, dtype=torch.uint8, device=dev)
        digits = torch.tensor(list(b"0123456789abcdef"), dtype=torch.uint8, device=dev)
        for j, kind in enumerate(kinds):
            if kind == "hex":
                g = torch.Generator(device=dev).manual_seed(0xB6)
                src = digits[torch.randint(0, 16, (per * REGION,), generator=g, device=dev)]
            else:
                src = synth.device_text(kind, per * REGION, seed=0xB0 + j, device=dev)
            for r in range(j, nreg, len(kinds)):
                out[r * REGION: (r + 1) * REGION] = src[(r // len(kinds)) * REGION: (r // len(kinds) + 1) * REGION]
            del src
        return out[:n].contiguous()

    KINDS = ("own", "shared", "set4", "set16")
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    for corpus, xc in (("a_C2_text", x), ("b_mixed", mixed(n))):
        tab = c.batch_table(xc, n_ary=2)
        lengths = c.table_get_lengths(tab)
        for block in (65536, 4096):
            count = (n + block - 1) // block
            offsets = c._block_offsets(xc, block)
            pb, sb = c.batch_bounds(n, count, S)
            bufs = {k: (torch.empty(pb, dtype=torch.uint8, device=dev), torch.empty(sb, dtype=torch.int16, device=dev))
                    for k in KINDS}
            sets, train_ms = {}, {}
            for k in (4, 16):
                c.batch_table_set(xc[: 64 * block], offsets[:65] - offsets[:1], k)   # (allocations and first launches)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sets[f"set{k}"] = c.batch_table_set(xc, offsets, k, n_ary=2, max_bits=12, iters=2)
                torch.cuda.synchronize()
                train_ms[f"set{k}"] = round((time.perf_counter() - t0) * 1e3, 2)

            def encode(kind):
                kw = {"table": tab} if kind == "shared" else {"table_set": sets[kind]} if kind in sets else {}
                return c.encode_blocks(xc, block=block, n_ary=2, sync_syms=S, payload=bufs[kind][0], sync_len=bufs[kind][1], **kw)

            encs, size, rows = {}, {}, {}
            for kind in KINDS:
                enc = encs[kind] = encode(kind)
                assert c.batch_status() == 0
                out.zero_()
                c.decode_batch(enc, out=out, out_off=enc["offsets"])
                assert c.batch_status() == 0 and torch.equal(out, xc), kind + ": batch round trip differs from the input"
                pay, idx = int(enc["pay_off"][-1]), int(enc["sync_off"][-1])
                row = {"what": "set_size", "corpus": corpus, "table": kind, "block": block, "count": count, "payload_bytes": pay,
                       "sync_entries": idx, "huffman_segments": int(enc["mode"].sum()),
                       "payload_bits_per_byte": round(8 * pay / n, 4)}
                if kind == "own":
                    c.batch_lens_pack(enc)
                    rec = count * (128 if c.batch_status() == 0 else 256)
                    size[kind] = pay + 2 * idx + count * 5 + rec
                elif kind == "shared":
                    rec = int(lengths.size)
                    size[kind] = pay + 2 * idx + count * 5 + rec
                else:
                    K = sets[kind].shape[0]
                    c.batch_lens_pack({"lens": sets[kind], "count": K})
                    rec = K * (128 if c.batch_status() == 0 else 256)
                    size[kind] = pay + 2 * idx + count * 6 + rec
                    chose = torch.bincount(enc["tid"][enc["mode"] == 1].to(torch.int64), minlength=K)
                    row.update(K=K, train_ms=train_ms[kind], coded_segments_per_record=chose.cpu().tolist(),
                               stored_segments=int((enc["mode"] == 0).sum()))
                row.update(record_bytes=rec, stored_bytes=size[kind])
                rows[kind] = row
                emit(**row)
            fns = {}
            for kind in KINDS:
                fns["encode_" + kind] = lambda kind=kind: encode(kind)
                fns["decode_" + kind] = lambda kind=kind: c.decode_batch(encs[kind], out=out, out_off=offsets)
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
            t = {k: [] for k in fns}
            stages = {kind: {} for kind in KINDS}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    t[k].append(ev_ms(fn, a.steps))
                for kind in KINDS:   # the kernels' own times (events around each launch: slower end to end, so apart)
                    c.timing(True)
                    encode(kind)
                    c.decode_batch(encs[kind], out=out, out_off=offsets)
                    for name, ms in c.timings():   # hb_plan, hbs_plan, hbm_plan: "plan" in every row
                        stages[kind].setdefault(name.split("_", 1)[1], []).append(ms)
                    c.timing(False)
            med = {k: round(statistics.median(v), 4) for k, v in t.items()}
            emit(what="set_time", corpus=corpus, block=block, count=count, ms=med,
                 min_max_ms={k: (round(min(v), 4), round(max(v), 4)) for k, v in t.items()})
            emit(what="set_stages", corpus=corpus, block=block, count=count,
                 ms={k: {s_: round(statistics.median(v), 4) for s_, v in d.items()} for k, d in stages.items()},
                 min_max_ms={k: {s_: (round(min(v), 4), round(max(v), 4)) for s_, v in d.items()} for k, d in stages.items()})
            for kind in ("set4", "set16"):   # the comparison: the set against the two modes it lies between
                vs = {"what": "set_vs", "corpus": corpus, "block": block, "count": count, "table": kind}
                for other in ("own", "shared"):
                    vs[f"stored_bytes_over_{other}"] = round(size[kind] / size[other], 4)
                    for op in ("encode", "decode"):
                        vs[f"{op}_ms_over_{other}"] = round(med[f"{op}_{kind}"] / med[f"{op}_{other}"], 4)
                vs.update(stored_bytes={k: size[k] for k in ("own", "shared", kind)},
                          encode_ms={k: med["encode_" + k] for k in ("own", "shared", kind)},
                          decode_ms={k: med["decode_" + k] for k in ("own", "shared", kind)},
                          slower_than_own=[op for op in ("encode", "decode") if med[f"{op}_{kind}"] > med[f"{op}_own"]])
                emit(**vs)
            del encs, bufs, sets
        del tab
    del out

if "ranges" in a.only:
    RB = 256   # bytes per range
    tab = c.batch_table(x, n_ary=2)
    gen = torch.Generator(device=dev)
    lane = torch.arange(RB, dtype=torch.int64, device=dev)

    def timed_pair(fns):
        """{name: median ms}, {name: (min, max)}: the sides alternating, windows of >= 20 ms."""
        steps = {}
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            steps[k] = max(a.steps, min(400, int(20.0 / max(ev_ms(fn, 1), 1e-3)) + 1))
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(ev_ms(fn, steps[k]))
        return ({k: statistics.median(v) for k, v in t.items()}, {k: (round(min(v), 4), round(max(v), 4)) for k, v in t.items()},
                steps)

    def draw(count, block, nr, seed):
        gen.manual_seed(seed)
        seg = torch.randint(0, count, (nr,), generator=gen, device=dev, dtype=torch.int64)
        first = torch.randint(0, block - RB + 1, (nr,), generator=gen, device=dev, dtype=torch.int64)
        return seg, first

    def range_row(enc, block, nr, seg, first, table, order, baseline):
        count = enc["count"]
        cnt = torch.full((nr,), RB, dtype=torch.int64, device=dev)
        ooff = torch.arange(nr, dtype=torch.int64, device=dev) * RB
        want = torch.take(x, ((seg * block + first)[:, None] + lane).reshape(-1))
        out_r = torch.zeros(nr * RB, dtype=torch.uint8, device=dev)

        def ranges():
            c.decode_batch_ranges(enc, seg, first, cnt, out=out_r, out_off=ooff)

        ranges()
        assert c.batch_status() == 0 and torch.equal(out_r, want), "the range call differs from the input"
        fns = {"ranges": ranges}
        row = {"what": "ranges", "table": table, "order": order, "block": block, "count": count, "nranges": nr,
               "range_bytes": RB, "delivered_bytes": nr * RB}
        if baseline:
            touched = torch.unique(seg)
            nd = touched.numel()
            rank = torch.searchsorted(touched, seg)
            beg = torch.ones(count, dtype=torch.int64, device=dev)     # untouched: [1, 0), refused unread
            end = torch.zeros(count, dtype=torch.int64, device=dev)
            beg[touched] = torch.arange(nd, dtype=torch.int64, device=dev) * block
            end[touched] = beg[touched] + (enc["offsets"][1:] - enc["offsets"][:-1])[touched]
            buf = torch.zeros(nd * block, dtype=torch.uint8, device=dev)
            pick = ((rank * block + first)[:, None] + lane).reshape(-1)
            out_b = torch.zeros(nr * RB, dtype=torch.uint8, device=dev)
            hb = c._hbatch(enc, enc["payload_cap"], enc["sync_cap"])
            args = (c.ctx, ctypes.byref(hb)) + ((tab.data_ptr(),) if "table" in enc else ()) + \
                (buf.data_ptr(), beg.data_ptr(), end.data_ptr(), buf.numel())
            fn = c.L.dc_huff_decode_batch_shared_scatter if "table" in enc else c.L.dc_huff_decode_batch_scatter

            def whole():
                assert fn(*args) == 0
                torch.take(buf, pick, out=out_b)

            whole()
            st = enc["status"][touched]
            assert bool((st == 0).all()) and torch.equal(out_b, want), "the baseline differs from the input"
            fns["whole_segments"] = whole
            row.update(distinct_segments=nd, baseline_decoded_bytes=int((end - beg)[touched].sum()),
                       density_pct=round(100.0 * nr * RB / (nd * block), 2))
        med, mm, steps = timed_pair(fns)
        row.update(ranges_ms=round(med["ranges"], 4), ranges_delivered_GBps=round(nr * RB / med["ranges"] / 1e6, 2),
                   ranges_min_max_ms=mm["ranges"], steps=steps)
        if baseline:
            row.update(whole_ms=round(med["whole_segments"], 4), whole_delivered_GBps=round(nr * RB / med["whole_segments"] / 1e6, 2),
                       whole_min_max_ms=mm["whole_segments"], speedup=round(med["whole_segments"] / med["ranges"], 2))
        emit(**row)
        return row

    rows = {}
    for block in (65536, 4096):
        count = (n + block - 1) // block
        enc = c.encode_blocks(x, block=block, n_ary=2, sync_syms=S, table=tab)
        assert c.batch_status() == 0
        for lg in (12, 16, 18, 19, 20) + ((22,) if block == 4096 else ()):   # (2^22 x 256 B of 4 KiB blocks: every byte once on average)
            seg, first = draw(count, block, 1 << lg, 0xC2 + lg)
            rows[(block, lg)] = range_row(enc, block, 1 << lg, seg, first, "shared", "random", True)
        del enc
        enc = c.encode_blocks(x, block=block, n_ary=2, sync_syms=S)
        assert c.batch_status() == 0
        seg, first = draw(count, block, 1 << 16, 0xC2 + 16)
        range_row(enc, block, 1 << 16, seg, first, "own", "random", False)
        srt = torch.argsort(seg)
        range_row(enc, block, 1 << 16, seg[srt].contiguous(), first[srt].contiguous(), "own", "sorted by segment", False)
        del enc
    # for context: the same 65536 ranges of the single-table stream of the whole text (Codec.decode_ranges)
    single = c.encode(x, n_ary=2, sync_syms=S)
    nr = 1 << 16
    seg, first = draw(n // 65536, 65536, nr, 0xC2 + 16)
    pos = seg * 65536 + first
    cnt = torch.full((nr,), RB, dtype=torch.int64, device=dev)
    ooff = torch.arange(nr, dtype=torch.int64, device=dev) * RB
    out_s = torch.zeros(nr * RB, dtype=torch.uint8, device=dev)
    want = torch.take(x, (pos[:, None] + lane).reshape(-1))

    def single_ranges():
        c.decode_ranges(single, pos, cnt, out=out_s, out_off=ooff)

    single_ranges()
    assert c.decode_status() == 0 and torch.equal(out_s, want)
    med, mm, steps = timed_pair({"single": single_ranges})
    emit(what="ranges_single_stream", nranges=nr, range_bytes=RB, ms=round(med["single"], 4),
         delivered_GBps=round(nr * RB / med["single"] / 1e6, 2), min_max_ms=mm["single"], steps=steps)
    r = rows[(65536, 12)]
    assert r["ranges_ms"] < r["whole_ms"], "4096 ranges of 256 B from 64 KiB blocks are not faster than decoding their segments"
