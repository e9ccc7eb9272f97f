"""bench.py --dump-outputs and the plain / --full result lines.

dump_outputs (CPU): small arrays are written whole, large ones as a fixed sample + block sums,
every value exact, the same files from the same arrays, nothing past the size limit.
On the GPU: a plain run of a few MiB prints only the headline line and dumps what its last
timed step returned: the decoded bytes are the input, the payload and sync index are the
oracle's stream of that input, and a second run writes the same files. --full adds the rest.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"}
FULL_ONLY = {"ms_per_step_serial", "roofline", "encode_GBps", "decode_GBps", "ratio", "kernels", "roundtrip_ok"}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_small_arrays_whole_and_exact(tmp_path):
    arrays = {"u8": torch.arange(300, dtype=torch.int32).to(torch.uint8),
              "i16": torch.tensor([-32768, -1, 0, 32767], dtype=torch.int16),
              "i32": torch.tensor([-2**31, 2**31 - 1], dtype=torch.int32),
              "i64": torch.tensor([2**52 + 1, 7], dtype=torch.int64)}
    bench.dump_outputs(str(tmp_path), arrays, 0, 1)
    got = _load(tmp_path)
    assert sorted(got) == sorted(arrays)
    assert got["u8"].dtype == got["i16"].dtype == np.float32
    assert got["i32"].dtype == got["i64"].dtype == np.float64
    for k, t in arrays.items():
        assert np.array_equal(got[k].astype(np.int64), t.numpy().astype(np.int64)), k


def test_dump_large_array_sample_and_block_sums(tmp_path):
    n = bench.DUMP_CAP + 3 * bench.DUMP_BLOCK + 17   # past the cap, a partial last block
    t = torch.from_numpy(np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), {"x": t}, 0, 1)
    u = t.clone()
    u[n - 1] ^= 1   # one element differs: the block sums see it wherever the sample falls
    bench.dump_outputs(str(b), {"x": u}, 0, 1)
    ga, gb = _load(a), _load(b)
    assert sorted(ga) == ["x", "x_blocksum"]
    assert ga["x"].shape == (bench.DUMP_CAP,) and ga["x"].dtype == np.float32
    x = t.numpy().astype(np.int64)
    nb = -(-n // bench.DUMP_BLOCK)
    want = np.add.reduceat(x, np.arange(nb) * bench.DUMP_BLOCK)
    assert ga["x_blocksum"].dtype == np.float64 and np.array_equal(ga["x_blocksum"].astype(np.int64), want)
    idx = np.sort(np.random.default_rng(0xD0).integers(0, n, bench.DUMP_CAP))
    assert np.array_equal(ga["x"].astype(np.int64), x[idx])
    assert not np.array_equal(ga["x_blocksum"], gb["x_blocksum"])
    assert sum(v.nbytes for v in ga.values()) <= bench.DUMP_LIMIT


def test_dump_refuses_more_than_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1000)
    with pytest.raises(RuntimeError, match="limit"):
        bench.dump_outputs(str(tmp_path), {"x": torch.zeros(300, dtype=torch.uint8)}, 0, 1)
    assert os.listdir(tmp_path) == []


def test_dump_names_carry_the_rank(tmp_path):
    bench.dump_outputs(str(tmp_path), {"x": torch.zeros(3, dtype=torch.uint8)}, 2, 4)
    assert os.listdir(tmp_path) == ["x.rank2.npy"]


# ---------------------------------------------------------------- on the GPU
N = (3 << 20) + 4099   # odd; the decoded bytes are past DUMP_CAP (sampled), the ~0.54 N payload bytes below it


def _run(monkeypatch, capsys, *args):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--size", str(N), "--steps", "3", "--warmup", "1",
                                      "--prewarm", "2", *args])
    with torch.cuda.stream(torch.cuda.current_stream()):   # (--full leaves its codec's stream current)
        bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def oracle_stream():
    """(input, payload bytes, bits, group bases, chunk lengths at S) of the bench input, by the oracle."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import oracle as orc
    x = bench.bench_input("C2", N, bench.input_seed("C2", 0), torch.device("cuda", 0)).cpu().numpy()
    h = orc.histogram(x)
    el, ev = orc.canonical(orc.huffman_lengths(h, 2), 2)
    code, nb, _ = orc.bitcodes(el, ev, 2)

    def at(S):
        payload, bits, idx = orc.huff_pack(x, code, nb, sync_syms=S)
        base, lens = orc.sync_compact(idx, 0, bits)
        return payload, bits, base, lens
    return x, at


@pytest.mark.gpu
def test_plain_run_headline_only_and_dump(oracle_stream, monkeypatch, capsys, tmp_path):
    x, at = oracle_stream
    d1, d2 = tmp_path / "one", tmp_path / "two"
    res = _run(monkeypatch, capsys, "--dump-outputs", str(d1))
    assert HEADLINE <= set(res) and not FULL_ONLY & set(res) and "cpu_baseline" not in res
    assert res["steps"] == 3 and res["unit"] == "GB/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["value"] == pytest.approx(N / (res["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    got = _load(d1)
    assert sorted(got) == ["decoded", "decoded_blocksum", "payload", "payload_bits", "sync_bases", "sync_lens"]
    payload, bits, base, lens = at(res["config"]["sync_syms"])
    assert int(got["payload_bits"][0]) == bits
    assert np.array_equal(got["payload"].astype(np.uint8), payload)
    assert np.array_equal(got["sync_bases"].astype(np.uint64), base)
    assert np.array_equal(got["sync_lens"].astype(np.int16).view(np.uint16), lens)
    idx = np.sort(np.random.default_rng(0xD0).integers(0, N, bench.DUMP_CAP))
    assert np.array_equal(got["decoded"].astype(np.uint8), x[idx])
    nb = -(-N // bench.DUMP_BLOCK)
    assert np.array_equal(got["decoded_blocksum"].astype(np.int64),
                          np.add.reduceat(x.astype(np.int64), np.arange(nb) * bench.DUMP_BLOCK))
    _run(monkeypatch, capsys, "--dump-outputs", str(d2))   # the same arguments: the same files
    again = _load(d2)
    assert sorted(again) == sorted(got) and all(np.array_equal(again[k], got[k]) for k in got)


@pytest.mark.gpu
def test_full_run_adds_the_rest(oracle_stream, monkeypatch, capsys):
    res = _run(monkeypatch, capsys, "--full", "--cpu-sample", str(1 << 20), "--profile-steps", "2")
    assert HEADLINE | FULL_ONLY <= set(res)
    assert res["roundtrip_ok"] is True and res["cpu_baseline"]["value"] > 0
    assert res["roofline"]["encode_ms"] > 0 and res["roofline"]["decode_ms"] > 0
