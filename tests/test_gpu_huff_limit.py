"""Length-limited Huffman tables on the device (dc_gpu.h "Length-limited tables"): the four
*_limit calls against dc_huff_table_lengths on the lengths of tests/huff_limit_model.py, byte for
byte over the whole dc_dtable (both written into zeroed buffers: the table kernel writes every
field but the decoder tables, which no call here has built yet); then capped tables through the
real pack and decoders, the shared-table batch with a covering table, and the host containers."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import huff_limit_model as hm
from tests.test_batch_shared_cpu import oracle_shared_batch, outcome, table_codes
from tests.test_gpu_bigcount import DTable

pytestmark = pytest.mark.gpu

DC_OK, DC_E_ARG = 0, -1
N = 262144
CASES = hm.cases()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def codec(torch_cuda):
    from data_compression_amd.device import Codec
    return Codec(0)


@pytest.fixture(scope="module")
def model():
    """name -> (capped lengths or None, info), computed once."""
    return {name: hm.limit_lengths(f, n, D, M) for name, f, M, n, D in CASES}


@pytest.fixture(scope="module")
def skewed():
    """262 144 bytes: byte 65 + i with count 2^(17-i), i = 0 .. 17 (one more of the first), shuffled."""
    counts = np.array([1 << (17 - i) for i in range(18)], np.int64)
    counts[0] += 1
    x = np.repeat(np.arange(65, 83, dtype=np.uint8), counts)
    np.random.default_rng(3).shuffle(x)
    assert x.size == N
    return x


@pytest.fixture(scope="module")
def flat():
    return np.random.default_rng(4).integers(0, 256, N, dtype=np.uint8)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _zt(torch, codec):
    return torch.zeros(codec.table_bytes, dtype=torch.uint8, device="cuda")


def _fields(b):
    return DTable.from_buffer_copy(b[: C.sizeof(DTable)].tobytes())


def _diff(got, want):
    """The named fields in which two tables differ, or 'bytes past fixed8' (empty: equal)."""
    if np.array_equal(got, want):
        return []
    a, b = _fields(got), _fields(want)
    return [n for n, _ in DTable._fields_ if _raw(a, n) != _raw(b, n)] or ["bytes past fixed8"]


def _raw(s, name):
    v = getattr(s, name)
    return bytes(v) if hasattr(v, "_length_") else v


def _limit_call(codec, fn, src, M, n, D, out):
    rc = getattr(codec.L, fn)(codec.ctx, src.data_ptr(), M, n, D, out.data_ptr())
    assert rc == DC_OK, (fn, rc)
    return out.cpu().numpy()


def _codes(lengths, n, M=258):
    """(code, nb) of the first 256 symbols under `lengths`."""
    el, ev = orc.canonical(lengths, n, M)
    code, nb, mx = orc.bitcodes(el[:256].copy(), ev[:256].copy(), n)
    return code, nb


@pytest.mark.parametrize("call", ["dc_huff_table_freq_limit", "dc_huff_table_limit"])
def test_table_calls_equal_the_model(torch_cuda, codec, model, call):
    """Every case: the table equals dc_huff_table_lengths on the model's lengths; where no code
    exists its status is DC_E_ARG; with max_digits 0, or a cap that does not bind, it equals the
    unlimited call's table. (The histogram call takes the cases whose counts are byte counts.)"""
    torch = torch_cuda
    hist = call == "dc_huff_table_limit"
    unl_fn = codec.L.dc_huff_table if hist else codec.L.dc_huff_table_freq
    bad, ran, bound, infeasible = [], 0, 0, 0
    for name, f, M, n, D in CASES:
        if hist and (len(f) > 256 or M != 258):
            continue
        ran += 1
        fz = np.zeros(256 if hist else M + 1, np.int64)
        fz[: len(f)] = f.astype(np.int64)
        src = _dev(torch, fz)
        want_l, info = model[name]
        got = _limit_call(codec, call, src, M, n, D, _zt(torch, codec))
        unl_t = _zt(torch, codec)
        assert unl_fn(codec.ctx, src.data_ptr(), M, n, unl_t.data_ptr()) == DC_OK
        unl = unl_t.cpu().numpy()
        d0 = _limit_call(codec, call, src, M, n, 0, _zt(torch, codec))
        if not np.array_equal(d0, unl):
            bad.append((name, "max_digits 0", _diff(d0, unl)))
        if want_l is None:
            infeasible += 1
            if _fields(got).status != DC_E_ARG:
                bad.append((name, "status", _fields(got).status))
            continue
        ref = codec.table_lengths(_dev(torch, want_l.astype(np.int32)), n, M, out=_zt(torch, codec)).cpu().numpy()
        if _diff(got, ref):
            bad.append((name, "table_lengths(model)", _diff(got, ref)))
        t = _fields(got)
        if t.status != DC_OK or t.dec_ready != 0 or t.max_bits > D * hm.digit_bits(n):
            bad.append((name, "scalars", t.status, t.dec_ready, t.max_bits))
        if info["binding"]:
            bound += 1
            if np.array_equal(got, unl):
                bad.append((name, "a binding cap changed nothing"))
        elif not np.array_equal(got, unl):
            bad.append((name, "not binding", _diff(got, unl)))
    assert not bad, (len(bad), bad[:8])
    assert ran > 100 and bound > 40 and infeasible > (0 if hist else 10)


def test_flat_256_at_eight_bits_is_the_byte_map(torch_cuda, codec):
    """k = n^D: every length is 8, and the fixed8 / affine flags are set."""
    torch = torch_cuda
    h = _dev(torch, np.full(256, 1000, np.int64))
    got = _limit_call(codec, "dc_huff_table_limit", h, 258, 2, 8, _zt(torch, codec))
    t = _fields(got)
    assert t.status == DC_OK and t.fixed8 == 1 and t.max_bits == 8 and t.min_len == 8 and t.max_len == 8
    assert np.array_equal(np.frombuffer(bytes(t.nbits), np.uint32), np.full(256, 8))
    assert np.array_equal(np.frombuffer(bytes(t.code), np.uint32), np.arange(256))
    fixed8_affine, fixed8_lo, fixed8_count = np.frombuffer(
        got[DTable.fixed8.offset + 4: DTable.fixed8.offset + 16].tobytes(), np.int32)
    assert (fixed8_affine, fixed8_lo, fixed8_count) == (1, 0, 256)


def test_python_arguments(torch_cuda, codec):
    torch = torch_cuda
    from data_compression_amd._lib import DcError
    h = _dev(torch, np.full(256, 7, np.int64))
    with pytest.raises(ValueError):
        codec.table(h, 16, max_bits=3)        # not one 4-bit digit
    with pytest.raises(ValueError):
        codec.table(h, 2, max_bits=0)
    with pytest.raises(DcError):
        codec.table(h, 2, max_bits=33)
    with pytest.raises(DcError):
        codec.table_freq(h, 10, 255, max_bits=36)
    assert codec.max_digits(10, 15) == 3 and codec.max_digits(2, None) == 0 and codec.max_digits(256, 32) == 4
    assert codec.table_status(codec.table(h, 2, max_bits=7))[0] == DC_E_ARG     # 256 bytes, 128 codes
    assert codec.table_status(codec.table(h, 2, max_bits=8)) == (DC_OK, 8)


@pytest.mark.parametrize("n,bits", [(2, 15), (2, 12), (3, 12), (4, 8)])
def test_plan_calls(torch_cuda, codec, skewed, n, bits):
    """dc_huff_table_plan_limit and dc_huff_encode_plan_limit: the table as above, the total =
    sum h * nbits of the capped table (also under a table that is not the input's own)."""
    torch = torch_cuda
    D = bits // hm.digit_bits(n)
    xt = _dev(torch, skewed)
    hx = orc.histogram(skewed)
    geo = hm.histograms()["geo0.9"][0]
    for f in (hx, geo):
        want_l, info = hm.limit_lengths(f, n, D)
        assert info["binding"]
        code, nb = _codes(want_l, n)
        ref = codec.table_lengths(_dev(torch, want_l), n, out=_zt(torch, codec)).cpu().numpy()
        total = int((hx.astype(object) * nb.astype(object)).sum())
        codec.hist(xt)
        tab, tot = codec.table_plan(_dev(torch, f.astype(np.int64)), n, out=_zt(torch, codec), max_bits=bits)
        assert not _diff(tab.cpu().numpy(), ref), (n, bits, _diff(tab.cpu().numpy(), ref))
        assert int(tot.item()) == total
    # the fused call: this input's own table; f is the input's histogram again
    want_l, info = hm.limit_lengths(hx, n, D)
    code, nb = _codes(want_l, n)
    ref = codec.table_lengths(_dev(torch, want_l), n, out=_zt(torch, codec)).cpu().numpy()
    hist, tab, tot = codec.encode_plan(xt, n, table=_zt(torch, codec), max_bits=bits)
    assert np.array_equal(hist.cpu().numpy().astype(np.uint64), hx)
    assert not _diff(tab.cpu().numpy(), ref)
    assert int(tot.item()) == int((hx.astype(object) * nb.astype(object)).sum())
    # max_digits 0 is the fused twin
    t0, t1 = _zt(torch, codec), _zt(torch, codec)
    h0, h1 = (torch.zeros(256, dtype=torch.int64, device="cuda") for _ in range(2))
    b0, b1 = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    assert codec.L.dc_huff_encode_plan_limit(codec.ctx, xt.data_ptr(), N, 258, n, 0, h0.data_ptr(), t0.data_ptr(),
                                             b0.data_ptr()) == DC_OK
    assert codec.L.dc_huff_encode_plan(codec.ctx, xt.data_ptr(), N, 258, n, h1.data_ptr(), t1.data_ptr(),
                                       b1.data_ptr()) == DC_OK
    assert torch.equal(t0, t1) and torch.equal(h0, h1) and torch.equal(b0, b1)


def _off(bit_base):
    return (bit_base >> 3) - ((bit_base >> 5) << 2)   # words start at stream word bit_base / 32


def _assert_stream(enc, x, lengths, S, bit_base, tag):
    """The encode's payload and sync index are the oracle's pack under `lengths`."""
    code, nb = _codes(lengths, 2)
    payload, bits, idx = orc.huff_pack(x, code, nb, bit_base=bit_base, sync_syms=S)
    assert enc["bits"] == bits, tag
    got = enc["words"].cpu().numpy().view(np.uint8)
    off = _off(bit_base)
    assert np.array_equal(got[off: off + len(payload)], payload), tag
    assert not got[:off].any(), tag
    base, lens = orc.sync_compact(idx, bit_base, bits)
    assert np.array_equal(enc["sync"][0].cpu().numpy().astype(np.uint64)[: len(base)], base), tag
    assert np.array_equal(enc["sync"][1].cpu().numpy().view(np.uint16)[: len(lens)], lens), tag


def _decode(torch, codec, enc, x, tag):
    out = torch.empty(x.size + 16, dtype=torch.uint8, device="cuda")
    codec.decode_into(enc, out)
    assert codec.decode_status() == 0, tag
    redo = codec.decode_redo_count()
    assert np.array_equal(out[: x.size].cpu().numpy(), x), tag
    return redo


@pytest.mark.parametrize("bit_base", (0, 5))
@pytest.mark.parametrize("S", (64, 256))
@pytest.mark.parametrize("cap", (15, 12))
def test_round_trip_through_the_real_kernels(torch_cuda, codec, skewed, flat, cap, S, bit_base):
    torch = torch_cuda
    x = skewed
    hx = orc.histogram(x)
    want_l, info = hm.limit_lengths(hx, 2, cap)
    assert info["natural"] > 15 and info["binding"]
    tag = (cap, S, bit_base)
    enc = codec.encode(_dev(torch, x), 2, sync_syms=S, bit_base=bit_base, max_bits=cap)
    assert np.array_equal(codec.table_get_lengths(enc["table"]), want_l), tag
    _assert_stream(enc, x, want_l, S, bit_base, tag)
    redo = _decode(torch, codec, enc, x, tag)
    first, count = N // 3 + 7, 100001
    got = codec.decode_range(enc, first, count)
    assert codec.decode_status() == 0, tag
    assert np.array_equal(got.cpu().numpy(), x[first: first + count]), tag
    if cap == 15 and S == 64:
        # the structural redos alone (a flat input's table has no code past 9 bits), and fewer
        # than under the unlimited table, whose codes of 16 bits and more take the redo
        encf = codec.encode(_dev(torch, flat), 2, sync_syms=S, bit_base=bit_base, max_bits=cap)
        redo_flat = _decode(torch, codec, encf, flat, tag + ("flat",))
        encu = codec.encode(_dev(torch, x), 2, sync_syms=S, bit_base=bit_base)
        redo_unl = _decode(torch, codec, encu, x, tag + ("unlimited",))
        print(f"redo chunks at bit_base {bit_base}: capped {redo}, flat {redo_flat}, unlimited {redo_unl}")
        assert redo == redo_flat, tag
        assert redo < redo_unl, tag


@pytest.mark.parametrize("bit_base", (0, 5))
def test_unlimited_encodes_as_before(torch_cuda, codec, skewed, bit_base):
    torch = torch_cuda
    L = orc.huffman_lengths(orc.histogram(skewed), 2)
    assert L.max() > 15
    enc = codec.encode(_dev(torch, skewed), 2, sync_syms=64, bit_base=bit_base)
    assert np.array_equal(codec.table_get_lengths(enc["table"]), L)
    _assert_stream(enc, skewed, L, 64, bit_base, ("unlimited", bit_base))
    _decode(torch, codec, enc, skewed, ("unlimited", bit_base))


def test_shared_batch_with_a_covering_table(torch_cuda, codec):
    """A table trained on a sample that lacks 16 byte values, applied to 64 segments of 1 KiB that
    hold them: stored without cover; with cover=True, max_bits=12 every segment that gets smaller
    is coded, decodes exactly, and so does one range of each."""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    p = 0.98 ** np.arange(256)
    perm = rng.permutation(256)
    missing = perm[100:116]                      # mid-rank values: they would be frequent enough to matter
    ps = p.copy()
    ps[100:116] = 0
    sample = perm[rng.choice(256, 65536, p=ps / ps.sum())].astype(np.uint8)
    assert set(range(256)) - set(sample.tolist()) == set(missing.tolist())
    segs = [perm[rng.choice(256, 1024, p=p / p.sum())].astype(np.uint8) for _ in range(63)]
    segs.append(rng.integers(0, 256, 1024, dtype=np.uint8))   # flat: not smaller under any table
    for s in segs:
        s[5] = missing[0]
    x = np.concatenate(segs)
    off = np.arange(65) * 1024
    xt, offt = _dev(torch, x), _dev(torch, off.astype(np.int64))
    # without cover: every segment holds a byte without a code
    tab = codec.batch_table(_dev(torch, sample))
    enc = codec.encode_batch(xt, offt, table=tab)
    assert codec.batch_status() == 0
    assert not enc["mode"].cpu().numpy().any()
    # with cover and a 12-bit cap
    hs = np.maximum(orc.histogram(sample), 1)
    want_l, info = hm.limit_lengths(hs, 2, 12)
    assert info["binding"] and (want_l[:256] > 0).all() and want_l.max() <= 12
    tab = codec.batch_table(_dev(torch, sample), max_bits=12, cover=True)
    assert np.array_equal(codec.table_get_lengths(tab), want_l)
    code, nb = table_codes(want_l, 2)
    kinds = [outcome(s, nb) for s in segs]
    assert kinds.count("coded") >= 60 and kinds[-1] == "notsmaller"
    exp = oracle_shared_batch(segs, code, nb, 64)
    enc = codec.encode_batch(xt, offt, table=tab)
    assert codec.batch_status() == 0
    assert np.array_equal(enc["mode"].cpu().numpy(), exp["mode"])
    assert np.array_equal(enc["bits"].cpu().numpy(), exp["bits"])
    end = int(exp["pay_off"][-1])
    assert np.array_equal(enc["payload"].cpu().numpy()[:end], exp["payload"])
    out, _ = codec.decode_batch(enc)
    assert codec.batch_status() == 0
    assert np.array_equal(out.cpu().numpy(), x)
    seg = np.arange(64)
    first = (seg * 13) % 900
    count = 100 + (seg * 7) % 24
    got, got_off, st = codec.decode_batch_ranges(enc, seg, first, count)
    assert codec.batch_status() == 0 and not st.cpu().numpy().any()
    g, o = got.cpu().numpy(), got_off.cpu().numpy()
    for r in range(64):
        assert np.array_equal(g[o[r]: o[r] + count[r]], segs[r][first[r]: first[r] + count[r]]), r


def test_host_containers_take_capped_lengths(torch_cuda, skewed):
    """huffman.compress(..., lengths=capped) and a DCH1 container of the same lengths both
    decompress to the input."""
    from data_compression_amd import huffman as H
    from data_compression_amd._lib import core
    data = skewed[:70001].tobytes()
    want_l, info = hm.limit_lengths(orc.histogram(skewed[:70001]), 2, 12)
    assert info["binding"]
    assert H.decompress(H.compress(data, 2, lengths=want_l)) == data
    n = len(data)
    cap = int(core().dc_huff_compress_bound(n, 64))
    out = (C.c_uint8 * cap)()
    got = C.c_uint64(0)
    src = (C.c_uint8 * n).from_buffer_copy(data)
    L = np.ascontiguousarray(want_l, np.int32)
    rc = core().dc_huff_compress_host(src, n, 2, L.ctypes.data_as(C.POINTER(C.c_int32)), 258, 64, out, cap, C.byref(got))
    assert rc == 0
    blob = bytes(out[: got.value])
    assert blob[:4] == b"DCH1"
    assert H.decompress(blob) == data
