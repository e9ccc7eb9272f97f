"""The model of the two Huffman containers (tests/container_model.py) and the host rule for a
container that was read (csrc/dc_container_check.h, dc_huff_container_check), without a device.

The model is pinned: its raw form is the reference's own compress() output (tests/golden/
container.npz), parse(write(x)) == x over the catalogue, and the catalogue reaches every edge it
claims (computed from the model: the character counts of the frame edges are not assumed).

The rule: dc_huff_container_check and the model's dch1_ok / netstring_ok, written independently,
agree on every container of the catalogues, valid, reader-only and malformed; the host-only info
calls give the model's sizes; and every DCH1 entry the rule rejects, the wild ones included (bits
of 2^64 - 1, a base of 2^63, a length of 0xFFFF), comes back as DC_E_STREAM from
dc_huff_decompress_host and dc_huff_decompress_range_host themselves. Where there is no device a
call that reached its first device call returns DC_E_HIP, so DC_E_STREAM shows that the rejection
comes first; with a device the same statuses hold, and the output buffer is untouched either way.

Two malformed entries pass the rule, and the test says so: one symbol fewer than the index was
built for, and two lengths of one group swapped. Every count and sum holds in them and every chunk
still starts inside the payload, which is all the rule is for: the decode is safe. What it gives
is the decoder's business: the input less its last symbol in the first case; in the second, wrong
bytes in the chunks between the two, with DC_E_STREAM only where a bit pattern is no code (a
complete code has none: a CRC-32 of the output, dc_crc32, is what sees that). They are handed to
no reader here.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import container_model as cm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")


def _lib():
    from data_compression_amd._lib import core
    return core()


def _buf(blob):
    return (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0")


def _check(blob):
    return _lib().dc_huff_container_check(_buf(blob), len(blob))


def _valid_containers():
    """(name, container, is DCH1) of everything valid the model writes"""
    out = []
    for c in cm.catalogue():
        if c.dch1 and c.dch1_model()[0] == cm.OK:
            out.append((c.name + "/dch1", c.dch1_model()[1], True))
        if c.ns:
            out.append((c.name + "/ns", c.ns_model()[0], False))
    out += [(name, blob, False) for name, blob, _ in cm.reader_inputs()]
    return out


# ---- the model is pinned ---------------------------------------------------------------------
def test_raw_form_is_the_reference_compress_output():
    d = np.load(os.path.join(G, "container.npz"), allow_pickle=False)
    for i in range(int(d["n_inputs"][0])):
        x = d[f"in_{i}"]
        assert cm.raw_bytes(x.tobytes()) == d[f"comp_{i}"].tobytes(), i
        assert len(cm.raw_bytes(x.tobytes())) == cm.len_raw(x.size)
        assert cm.decode_netstring(d[f"comp_{i}"].tobytes()) == x.tobytes()


def test_parse_of_write_is_the_input():
    for c in cm.catalogue():
        x = c.x.tobytes()
        st, blob = c.dch1_model()
        if st == cm.OK:
            assert cm.decode_dch1(blob) == x and cm.dch1_ok(blob), c
            p = cm.parse_dch1(blob)
            assert len(blob) == cm.HEADER + cm.index_bytes(len(x), p["S"]) + (p["bits"] + 7) // 8
            assert len(blob) <= cm.compress_bound(len(x), c.S), c
        blob, why = c.ns_model()
        assert cm.decode_netstring(blob) == x, c
        assert len(blob) <= cm.len_raw(len(x)) <= cm.netstring_bound(len(x)), c
        assert (len(blob) < cm.len_raw(len(x))) == (why == "huffman"), c
    for name, blob, want in cm.reader_inputs():
        assert cm.decode_netstring(blob) == want, name


def _texts(blob):
    """per Huffman segment: ([characters per #dcidx block], [characters per Z block])"""
    out = []
    for typ, payload, _ in cm.ns_blocks(blob):
        if typ == "#" and payload[:4] == b"dc1 ":
            out.append(([], []))
        elif typ == "#" and payload[:6] == b"dcidx:":
            out[-1][0].append(len(payload) - 6)
        elif typ == "Z":
            out[-1][1].append(len(payload))
    return out


def test_catalogue_reaches_its_size_and_arity_edges():
    for S in cm.SIZES_S:
        want = {0: (0, 0, 0), 1: (1, 1, 1), S - 1: (1, 1, S - 1), S: (1, 1, 0), S + 1: (2, 1, 1),
                64 * S - 1: (64, 1, S - 1), 64 * S: (64, 1, 0), 64 * S + 1: (65, 2, 1)}
        for n, (nc, ng, part) in want.items():
            c = cm.case("size-S%d-n%d" % (S, n))
            assert (cm.chunks(n, S), cm.groups(n, S), n % S) == (nc, ng, part)
            p = cm.parse_dch1(c.dch1_model()[1])
            assert (p["n"], p["S"], p["bases"].size, p["lens"].size) == (n, S, ng, nc)
        assert cm.case("size-S%d-n%d" % (S, 64 * S + 1)).ns_model()[1] == "huffman"
    # the writer's own sync size: 32 above 8.2 bits per symbol, else 64
    dense, sparse = cm.case("size-S0-dense"), cm.case("size-S0-sparse")
    pd, ps = cm.parse_dch1(dense.dch1_model()[1]), cm.parse_dch1(sparse.dch1_model()[1])
    assert pd["S"] == 32 and pd["bits"] / pd["n"] > 8.21 and ps["S"] == 64 and ps["bits"] / ps["n"] < 8
    assert cm.parse_dch1(cm.case("size-S0-n0").dch1_model()[1])["S"] == 64
    assert cm.parse_netstring(sparse.ns_model()[0])[0][1]["S"] == 64
    assert cm.choose_sync(1000, 8203) == 64 and cm.choose_sync(1000, 8204) == 32
    widths = {2: 1, 3: 2, 4: 2, 9: 4, 16: 4, 17: 5, 256: 8}
    for a, w in widths.items():
        c = cm.case("arity-%d" % a)
        assert cm.digit_bits(a) == w
        st, blob = c.dch1_model()
        if a <= 16:
            assert st == cm.OK and cm.parse_dch1(blob)["w"] == w and c.ns_model()[1] == "huffman"
        else:
            assert st == cm.E_ARG
    assert cm.case("arity-17").ns_model()[1] == "huffman" and cm.case("arity-256").ns_model()[1] == "notsmaller"


def test_catalogue_reaches_its_length_edges():
    def xblock(c):
        return [p for t, p, _ in cm.ns_blocks(c.ns_model()[0]) if t == "X"][0]

    c = cm.case("M255")
    assert c.ns_model()[1] == "huffman" and xblock(c).startswith(b"255:") and len(xblock(c)) == 4 + 256
    assert c.x.max() == 254 and c.dch1_model()[0] == cm.OK
    c = cm.case("M100")
    assert c.ns_model()[1] == "huffman" and xblock(c).startswith(b"100:") and len(xblock(c)) == 4 + 101
    assert c.x.max() == 100 and c.lengths[100] > 0 and c.dch1_model()[0] == cm.OK      # the byte M itself is coded
    c = cm.case("letters")
    assert c.ns_model()[1] == "huffman" and set(xblock(c)[4:]) >= set(cm.LEN_CHARS[1:33].encode())
    assert cm.LEN_CHARS[10] == "A" and cm.LEN_CHARS[32] == "W" and cm.LEN_CHARS[35] == "Z"
    assert cm.code_of(c.x, 2, c.lengths)["max_bits"] == 32 and c.dch1_model()[0] == cm.OK
    assert (cm.case("len33").ns_model()[1], cm.case("len33").dch1_model()[0]) == ("maxbits", cm.E_CODE_TOO_LONG)
    assert (cm.case("len36").ns_model()[1], cm.case("len36").dch1_model()[0]) == ("maxbits", cm.E_CODE_TOO_LONG)
    c = cm.case("len36-sym257")
    assert c.ns_model()[1] == "len35" and c.dch1_model()[0] == cm.OK and cm.code_of(c.x, 2, c.lengths)["max_bits"] == 20
    c = cm.case("nocode")
    t = cm.code_of(c.x, 2, c.lengths)
    assert (c.ns_model()[1], c.dch1_model()[0]) == ("nocode", cm.E_NOCODE) and t["nocode"]
    assert cm.huffman_size(c.x.size, 2, t["bits"], 64, 258) < cm.len_raw(c.x.size)     # so it is not "notsmaller"


def test_catalogue_reaches_its_frame_edges():
    for n, nblocks in zip(cm.RAW_SIZES, (1, 1, 2, 3)):
        blob, why = cm.case("raw-%d" % n).ns_model()
        assert why == "notsmaller" and [t for t, _, _ in cm.ns_blocks(blob)] == ["\n"] * nblocks
    C = cm.NS_MAX - 2
    for n, zblocks in zip(cm.Z_EDGES, ([C], [C, 1], [C, C])):
        c = cm.case("zedge-%d" % n)
        blob, why = c.ns_model()
        seg = cm.parse_netstring(blob)[0][1]
        assert why == "huffman" and seg["bits"] == 4 * n and len(seg["ztext"]) == -(-4 * n // 6) == sum(zblocks)
        assert _texts(blob)[0][1] == zblocks
    CI = cm.NS_MAX - 8
    for n, ib, iblocks in zip(cm.IDX_EDGES, (24570, 24572), ([CI], [CI, 3])):
        blob, why = cm.case("idxedge-%d" % n).ns_model()
        nc = -(-n // 16)
        assert why == "huffman" and 8 * (-(-nc // 64)) + 2 * nc == ib == cm.index_bytes(n, 16)   # the header comment's ib
        assert -(-8 * ib // 6) == sum(iblocks) and _texts(blob)[0][0] == iblocks


def test_reader_inputs_reach_their_edges():
    R = {name: blob for name, blob, _ in cm.reader_inputs()}
    for k in (1, 15, 16, 17):       # where the Huffman segment's output starts: 16 alone is 16-B aligned
        segs = cm.parse_netstring(R["raw%d-then-huffman" % k])
        assert [s[0] for s in segs] == ["raw", "huff"] and len(segs[0][1]) == k
    assert [s[0] for s in cm.parse_netstring(R["huffman-raw-huffman"])] == ["huff", "raw", "huff"]
    types = [t + p[:5].decode("latin-1") for t, p, _ in cm.ns_blocks(R["other-between-Z"])]
    assert any(a[0] == "Z" and b == "#other" and c[0] == "Z" for a, b, c in zip(types, types[1:], types[2:]))
    types = [t + p[:5].decode("latin-1") for t, p, _ in cm.ns_blocks(R["other-between-dcidx"])]
    assert any(a == "#dcidx" and b == "#other" and c == "#dcidx" for a, b, c in zip(types, types[1:], types[2:]))
    assert R["hex-lengths"].count(b"0x") >= 4 and b"0X" in R["hex-lengths"]
    assert re.match(rb"0\d+:\n#dc1", R["octal-lengths"]) and R["plus-lengths"].startswith(b"+")
    assert b"+" in R["plus-slash-text"] and b"/" in R["plus-slash-text"]
    assert b"-" not in R["plus-slash-text"] and b"_" not in R["plus-slash-text"]
    assert set(_texts(R["Z-split-1"])[0][1]) == {1} and set(_texts(R["Z-split-2"])[0][1][:-1]) == {2}
    assert _texts(R["Z-split-32766"])[0][1][0] == 32766 and len(_texts(R["Z-split-32766"])[0][1]) == 2
    assert R["whitespace"][:1] == b" " and R["whitespace"][-1:] == b"\n" and b",\r\n \t" in R["whitespace"]
    assert b"\0" in R["nul-after-last"] and b"M=" not in R["no-M"]
    assert b"M=258" in R["raw1-then-huffman"]


# ---- the rule ----------------------------------------------------------------------------------
def test_check_is_exported_and_declared():
    L = _lib()
    assert L.dc_huff_container_check.restype is C.c_int and len(L.dc_huff_container_check.argtypes) == 2
    text = open(os.path.join(REPO, "include", "dc_host.h")).read()
    assert "int dc_huff_container_check(const uint8_t *in, uint64_t m);" in text
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(REPO, "data_compression_amd", "lib", "libdc_core.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "dc_huff_container_check" in {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_check_and_model_agree_on_valid_containers():
    for name, blob, is_dch1 in _valid_containers():
        assert (cm.dch1_ok(blob) if is_dch1 else cm.netstring_ok(blob)), name
        assert _check(blob) == cm.OK, name
        assert (blob[:4] == cm.MAGIC) == is_dch1
    assert _lib().dc_huff_container_check(None, 0) == cm.E_STREAM
    assert _check(b"") == cm.OK and cm.netstring_ok(b"") and cm.decode_netstring(b"") == b""   # no block: no bytes


def test_check_and_model_agree_on_malformed_containers():
    names = [e[0] for e in cm.malformed_dch1()]
    for want in ("version-2", "n_ary-0", "n_ary-1", "n_ary-17", "wrong-w", "flags-1", "S-0", "S-8", "S-48", "S-2048",
                 "n-plus-1", "n-minus-1", "bits-2^64-1", "bits-2^64-7", "bits-2^63", "bits-plus-1", "cut-1-at-header",
                 "cut-1-at-bases", "cut-1-at-lens", "cut-1-at-payload", "bases0-1", "bases1-plus-1", "bases1-minus-1",
                 "bases1-2^63", "bases1-bits-plus-1", "bases-descending", "len-plus-1", "len-minus-1", "len-0xFFFF",
                 "lens-swapped-in-group"):
        assert want in names
    for name, blob, valid, _ in cm.malformed_dch1():
        assert cm.dch1_ok(blob) == valid, name
        assert _check(blob) == (cm.OK if valid else cm.E_STREAM), name
    # the two the rule cannot see (module docstring)
    assert [e[0] for e in cm.malformed_dch1() if e[2]] == ["valid", "n-minus-1", "lens-swapped-in-group"]
    for name, blob, valid in cm.malformed_netstring():
        assert cm.netstring_ok(blob) == valid, name
        assert _check(blob) == (cm.OK if valid else cm.E_STREAM), name
    # a shifted index is text the host does not parse: the host check passes it, the model's decode
    # (the index rule on the parsed index) does not
    for delta in (1, -1, 64, -64):
        for what in ("base", "len"):
            blob, _ = cm.shifted_index(delta, what)
            assert _check(blob) == cm.OK and cm.netstring_ok(blob)
            with pytest.raises(cm.Malformed):
                cm.decode_netstring(blob)


def test_index_rule_cases():
    x, P = cm.malformed_base()
    n, bits, bases, lens = P["n"], P["bits"], P["bases"], P["lens"]
    assert cm.index_ok(n, 16, bases, lens, bits)
    assert not cm.index_ok(n, 16, bases, lens, bits, bit_base=1)
    assert cm.index_ok(n, 16, bases + np.uint64(77), lens, bits, bit_base=77)
    assert not cm.index_ok(n, 16, bases[:-1], lens, bits) and not cm.index_ok(n, 16, bases, lens[:-1], bits)
    assert not cm.index_ok(n, 32, bases, lens, bits) and not cm.index_ok(n, 24, bases, lens, bits)
    assert cm.index_ok(0, 64, [], [], 0) and not cm.index_ok(0, 64, [], [], 1)
    # a chunk of k symbols holds at most 32 k bits, the last partial chunk with its own k
    assert cm.index_ok(17, 16, [0], [512, 32], 544) and not cm.index_ok(17, 16, [0], [511, 33], 544)
    assert not cm.index_ok(17, 16, [0], [513, 31], 544)


def test_info_calls_give_the_models_sizes():
    L = _lib()
    for name, blob, is_dch1 in _valid_containers():
        n, a, bits = C.c_uint64(7), C.c_int(7), C.c_uint64(7)
        assert L.dc_huff_container_info(_buf(blob), len(blob), C.byref(n), C.byref(a), C.byref(bits)) == 0, name
        if is_dch1:
            p = cm.parse_dch1(blob)
            assert (n.value, a.value, bits.value) == (p["n"], p["n_ary"], p["bits"]), name
        else:
            assert (n.value, a.value, bits.value) == (cm.netstring_size(blob), 0, 0), name
            v = C.c_uint64(7)
            assert L.dc_huff_netstring_info(_buf(blob), len(blob), C.byref(v)) == 0 and v.value == n.value, name
    wraps = dict((e[0], e[1]) for e in cm.malformed_netstring())["syms-sum-wraps"]
    assert wraps.count(b"syms=%d " % 2 ** 63) == 2
    assert L.dc_huff_netstring_info(_buf(wraps), len(wraps), C.byref(C.c_uint64(0))) == cm.E_STREAM
    half = wraps[: len(wraps) // 2]                      # one such segment alone: a size, not a wrap
    v = C.c_uint64(0)
    assert L.dc_huff_netstring_info(_buf(half), len(half), C.byref(v)) == 0 and v.value == 2 ** 63


def test_rejected_containers_are_refused_before_the_first_device_call():
    """DC_E_STREAM, never DC_E_HIP, and nothing written: from both DCH1 readers for every DCH1
    entry the rule rejects, and from the netstring reader for every netstring entry it rejects."""
    L = _lib()
    x, P = cm.malformed_base()
    seen = 0
    for name, blob, valid, wild in cm.malformed_dch1():
        if valid:
            continue
        seen += wild
        for ranged in (False, True):
            out = (C.c_uint8 * 8192)(*([0xA5] * 8192))
            got = C.c_uint64(0xA5A5)
            if ranged:     # symbols 1000..1099 at S = 16: groups 0 and 1, where the index entries are damaged
                rc = L.dc_huff_decompress_range_host(_buf(blob), len(blob), 1000, 100, out, 8192, C.byref(got))
            else:
                rc = L.dc_huff_decompress_host(_buf(blob), len(blob), out, 8192, C.byref(got))
            assert rc == cm.E_STREAM, (name, ranged, rc)
            # (the range read clears *out_len once the header and the range have passed)
            assert bytes(out) == b"\xa5" * 8192 and got.value in ((0, 0xA5A5) if ranged else (0xA5A5,)), (name, ranged)
    assert seen == 7
    for name, blob, valid in cm.malformed_netstring():
        if valid:
            continue
        out = (C.c_uint8 * 8192)(*([0xA5] * 8192))
        got = C.c_uint64(0xA5A5)
        for fn in (L.dc_huff_decompress_netstring, L.dc_huff_decompress_host):
            assert fn(_buf(blob), len(blob), out, 8192, C.byref(got)) == cm.E_STREAM, name
        assert bytes(out) == b"\xa5" * 8192 and got.value == 0xA5A5, name


def test_container_checker_builds_and_passes(tmp_path):
    """tests/c/container_check.c: the same header in a stand-alone C program, with the host
    sanitizers where the compiler has them."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc, "no C compiler"
    exe = str(tmp_path / "container_check")
    base = [cc, "-std=c11", "-g", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "data_compression_amd", "csrc"),
            os.path.join(REPO, "tests", "c", "container_check.c"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)   # (a compiler without the sanitizer runtimes)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "container_check: ok" in r.stdout, r.stdout + r.stderr
