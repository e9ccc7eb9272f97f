"""Length-limited Huffman tables (dc_gpu.h "Length-limited tables") without a device: the exported
entry points and their host argument checks; the repair of the length counts as the library
compiles it (dc_huff_limit_classes, csrc/dc_huff_limit.h) against the numpy model's steps 3 to 5 on
every case; the model's own properties (Kraft, 1 <= len <= D, monotone in the count, the unlimited
lengths when they fit, never below a package-merge optimum at n = 2); and the measured cost of the
rule over that optimum, held to what was measured. The header's exhaustive check under the host
sanitizers is tests/c/huff_limit_check.c."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import huff_limit_model as hm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_E_ARG = -1
ENTRY_POINTS = ("dc_huff_table_limit", "dc_huff_table_freq_limit", "dc_huff_table_plan_limit",
                "dc_huff_encode_plan_limit", "dc_huff_limit_classes")
CASES = hm.cases()
IDS = [c[0] for c in CASES]


def _lib():
    from data_compression_amd._lib import core
    return core()


def test_entry_points_are_exported_and_declared():
    L = _lib()
    for name in ENTRY_POINTS:
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is C.c_int, name
    assert len(L.dc_huff_table_limit.argtypes) == 6
    assert len(L.dc_huff_table_freq_limit.argtypes) == 6
    assert len(L.dc_huff_table_plan_limit.argtypes) == 7
    assert len(L.dc_huff_encode_plan_limit.argtypes) == 9
    assert len(L.dc_huff_limit_classes.argtypes) == 4


@pytest.fixture()
def dummies():
    keep = [C.create_string_buffer(64) for _ in range(5)]
    return [C.cast(k, C.c_void_p) for k in keep] + [keep]   # never read: a check fails first


def _four(L, ctx, src, hist, tab, total, M, n, D):
    """The four calls' return codes; src: the histogram / frequency array / input."""
    return (L.dc_huff_table_limit(ctx, src, M, n, D, tab),
            L.dc_huff_table_freq_limit(ctx, src, M, n, D, tab),
            L.dc_huff_table_plan_limit(ctx, src, M, n, D, tab, total),
            L.dc_huff_encode_plan_limit(ctx, src, 64, M, n, D, hist, tab, total))


def test_host_argument_checks(dummies):
    """Every failing test comes before the first read of the context, which is a host dummy here."""
    L = _lib()
    ctx, src, hist, tab, total, _ = dummies
    bad = (DC_E_ARG,) * 4
    # a cap the packed code cannot hold: past DC_MAX_DIGITS, or max_digits * w > 32; negative
    for n, D in ((2, 33), (2, 129), (2, 1 << 20), (3, 17), (4, 17), (9, 9), (10, 9), (16, 9), (17, 7), (256, 5),
                 (2, -1), (16, -8)):
        assert not hm.cap_valid(n, D)
        assert _four(L, ctx, src, hist, tab, total, 258, n, D) == bad, (n, D)
    # the twins' own tests, with a valid cap and with none (max_digits 0 goes to the twin)
    for D in (0, 8):
        assert _four(L, None, src, hist, tab, total, 258, 2, D) == bad
        assert _four(L, ctx, src, hist, None, total, 258, 2, D) == bad
        for M, n in ((-1, 2), (1024, 2), (258, 1), (258, 257)):
            assert _four(L, ctx, src, hist, tab, total, M, n, D) == bad, (M, n, D)
        assert L.dc_huff_table_limit(ctx, None, 258, 2, D, tab) == DC_E_ARG
        assert L.dc_huff_table_freq_limit(ctx, None, 258, 2, D, tab) == DC_E_ARG
        assert L.dc_huff_table_plan_limit(ctx, None, 258, 2, D, tab, total) == DC_E_ARG
        assert L.dc_huff_table_plan_limit(ctx, src, 258, 2, D, tab, None) == DC_E_ARG
        assert L.dc_huff_encode_plan_limit(ctx, src, 64, 258, 2, D, hist, tab, None) == DC_E_ARG


def _lib_classes(n, D, cnt, k):
    a = (C.c_uint32 * (D + 1))(*[int(c) for c in cnt])
    rc = _lib().dc_huff_limit_classes(n, D, a, k)
    return rc, list(a)


def test_classes_argument_checks():
    L = _lib()
    a = (C.c_uint32 * 9)(0, 0, 0, 0, 0, 0, 0, 0, 3)
    assert L.dc_huff_limit_classes(2, 8, None, 3) == DC_E_ARG
    for n, D in ((2, 0), (2, 33), (1, 4), (257, 2), (16, 9), (3, 17)):
        assert L.dc_huff_limit_classes(n, D, a, 3) == DC_E_ARG, (n, D)
    assert L.dc_huff_limit_classes(2, 8, a, 4) == DC_E_ARG      # sum cnt != k
    assert L.dc_huff_limit_classes(2, 8, a, 3) == 0 and list(a) == [0, 1, 2, 0, 0, 0, 0, 0, 0]   # 1/2 + 1/4 + 1/4 = 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_classes_equal_the_model(case):
    """dc_huff_limit_classes on the case's length counts = the model's steps 1, 4 and 5; cnt is
    unchanged where no code exists."""
    name, f, M, n, D = case
    l = hm.limit_lengths(f, n, D, M)[1]["unlimited"]
    fz = np.zeros(M + 1, np.uint64)
    fz[: len(f)] = f
    cnt = hm.classes(l, fz, D)
    k = int((fz > 0).sum())
    want = hm.repair(n, D, cnt, k)
    rc, got = _lib_classes(n, D, cnt, k)
    if want is None:
        assert rc == DC_E_ARG and got == cnt.tolist()
    else:
        assert rc == 0 and got[1:] == want[0][1:]


# cost / package-merge optimum of every n = 2 case the cap binds on, as measured with this model
# (rounded up at the sixth decimal); the test allows a tenth of the excess more
MEASURED = {
    "flat256-n2-D8": 1.000000,
    "pow2_18-n2-D8": 1.007576,
    "pow2_18-n2-D12": 1.000122,
    "pow2_18-n2-D15": 1.000000,
    "fib40-n2-D8": 1.005987,
    "fib40-n2-D12": 1.000067,
    "fib40-n2-D15": 1.000000,
    "geo0.8-n2-D8": 1.000000,
    "geo0.8-n2-D12": 1.035718,      # natural depth 44
    "geo0.8-n2-D15": 1.004367,
    "geo0.8-n2-D32": 1.000001,
    "geo0.9-n2-D8": 1.000000,
    "geo0.9-n2-D12": 1.011008,
    "geo0.9-n2-D15": 1.001469,
    "geo0.9-n2-D32": 1.000001,
    "near2^33-n2-D8": 1.000000,
    "near2^33-n2-D12": 1.002550,
    "near2^33-n2-D15": 1.000001,
    "m1023-n2-D12": 1.138169,       # 1000 symbols in 4096 codes: the worst of the list
    "m1023-n2-D15": 1.003343,
    "depth=D+1-n2-D8": 1.000000,
    "depth=D+1-n2-D12": 1.000000,
    "depth=D+1-n2-D15": 1.000000,
}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_properties(case):
    name, f, M, n, D = case
    l, info = hm.limit_lengths(f, n, D, M)
    fz = np.zeros(M + 1, np.uint64)
    fz[: len(f)] = f
    present = fz > 0
    k = int(present.sum())
    if n ** D < k:
        assert l is None
        return
    assert l is not None
    assert np.all(l[~present] == 0)
    lp = l[present].astype(object)
    assert lp.min() >= 1 and lp.max() <= D
    assert sum(n ** (D - int(x)) for x in lp) <= n ** D          # Kraft
    shortest_below = D + 1                                         # a higher count never a longer code:
    for c in np.unique(fz[present]):                               # counts ascending
        lc = l[fz == c]
        assert lc.max() <= shortest_below, (name, int(c))
        shortest_below = min(shortest_below, int(lc.min()))
    if info["natural"] <= D:
        assert not info["binding"] and np.array_equal(l, info["unlimited"])
    else:
        assert info["binding"] and not np.array_equal(l, info["unlimited"])
    if n == 2 and k >= 2:
        c, opt = hm.cost(fz, l), hm.package_merge_cost(fz, D)
        ratio = c / opt
        print(f"{name}: cost / optimum = {ratio:.6f} (demotions {info['demotions']}, promotions {info['promotions']})")
        assert c >= opt
        if info["binding"]:
            assert name in MEASURED, name
            assert ratio <= 1 + 1.1 * (MEASURED[name] - 1), (name, ratio)


def test_the_case_list_covers_the_rule():
    infos = {c[0]: hm.limit_lengths(c[1], c[3], c[4], c[2]) for c in CASES}
    assert any(i["promotions"] > 0 for _, i in infos.values())            # step 5 promotes
    assert any(i["levels"] >= 2 for _, i in infos.values())               # demotion through two or more levels
    assert any(l is None for l, _ in infos.values())                      # no such code
    assert infos["flat256+256-n2-D8"][0] is None
    l, i = infos["flat256-n2-D8"]                                         # k = n^D: every length is D
    assert i["k"] == 256 and np.all(l[:256] == 8) and np.all(l[256:] == 0)
    for D in (8, 12, 15):
        assert infos[f"depth=D-n2-D{D}"][1]["natural"] == D and not infos[f"depth=D-n2-D{D}"][1]["binding"]
        assert infos[f"depth=D+1-n2-D{D}"][1]["natural"] == D + 1 and infos[f"depth=D+1-n2-D{D}"][1]["binding"]
    assert {c[3] for c in CASES} == set(hm.ARITIES)


def test_package_merge_is_huffman_without_a_cap():
    """The optimum the costs are held against: with a cap of 32 it is plain Huffman's cost (a heap
    Huffman here, no phantom dummy), and with 2^D = k it is k leaves at D."""
    import heapq
    rng = np.random.default_rng(5)
    for k in (2, 3, 17, 100):
        f = rng.integers(1, 1000, k)
        h = [int(x) for x in f]
        heapq.heapify(h)
        tot = 0
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h)
            tot += a + b
            heapq.heappush(h, a + b)
        assert hm.package_merge_cost(f, 32) == tot
    assert hm.package_merge_cost(np.arange(1, 17), 4) == 4 * sum(range(1, 17))


def test_limit_checker_builds_and_passes(tmp_path):
    """tests/c/huff_limit_check.c: the same header in a stand-alone C program, with the host
    sanitizers where the compiler has them."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc, "no C compiler"
    exe = str(tmp_path / "huff_limit_check")
    base = [cc, "-std=c11", "-g", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "data_compression_amd", "csrc"),
            os.path.join(REPO, "tests", "c", "huff_limit_check.c"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)   # (a compiler without the sanitizer runtimes)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "huff_limit_check: ok" in r.stdout, r.stdout + r.stderr
