"""Length-limited Huffman tables (dc_gpu.h "Length-limited tables") in numpy, on the oracle's
huffman() lengths: the rule's steps 1 to 6, the cases both test files run, and a package-merge
optimum for n = 2 to hold the rule's cost against. Shared by tests/test_huff_limit_cpu.py and
tests/test_gpu_huff_limit.py."""
import numpy as np

from oracle import oracle as orc

DC_MAX_DIGITS = 128


def digit_bits(n):
    """w = ceil(log2 n)."""
    return max(n - 1, 1).bit_length()


def cap_valid(n, D):
    """The host's test of a cap (0, "no cap", is not one)."""
    return 1 <= D <= DC_MAX_DIGITS and D * digit_bits(n) <= 32


def classes(l, f, D):
    """Step 3: cnt[d] = the present symbols of length min(l, D), d = 0 .. D (cnt[0] = 0)."""
    l, f = np.asarray(l), np.asarray(f)
    return np.bincount(np.minimum(l[f > 0], D), minlength=D + 1).astype(np.int64)


def repair(n, D, cnt, k):
    """Steps 1, 4 and 5 on cnt (a list of D + 1 Python ints): (cnt, demotions, promotions, the
    number of levels a demotion started from), or None when n^D < k."""
    cnt = [int(c) for c in cnt]
    B = n ** D
    if B < k:
        return None
    K = sum(cnt[d] * n ** (D - d) for d in range(1, D + 1))
    dem = pro = 0
    levels = set()
    while K > B:
        d = max(d for d in range(1, D) if cnt[d] > 0)
        cnt[d] -= 1
        cnt[d + 1] += 1
        K -= (n - 1) * n ** (D - d - 1)
        dem += 1
        levels.add(d)
    for d in range(D, 1, -1):
        c = (n - 1) * n ** (D - d)
        while cnt[d] > 0 and K + c <= B:
            cnt[d] -= 1
            cnt[d - 1] += 1
            K += c
            pro += 1
    return cnt, dem, pro, len(levels)


def limit_lengths(freq, n, D, M=258):
    """The capped lengths of the counts freq[0 ..] among symbols 0 .. M (steps 1 to 6) as an int32
    array of M + 1, or None when no such code exists; and a dict of what the rule did: k, the
    natural depth, whether the cap binds, the demotions, the promotions, the number of levels
    demoted from, and the unlimited lengths."""
    f = np.zeros(M + 1, np.uint64)
    f[: len(freq)] = np.asarray(freq, np.uint64)
    l = orc.huffman_lengths(f, n, M).astype(np.int32)
    present = np.flatnonzero(f > 0)
    k = present.size
    info = {"k": k, "natural": int(l.max()) if k else 0, "binding": False, "demotions": 0, "promotions": 0,
            "levels": 0, "unlimited": l}
    if n ** D < k:
        return None, info
    if k == 0 or l.max() <= D:
        return l, info
    cnt, dem, pro, lev = repair(n, D, classes(l, f, D), k)
    info.update(binding=True, demotions=dem, promotions=pro, levels=lev)
    # step 6: count descending, the higher symbol value first among equal counts
    order = sorted(present.tolist(), key=lambda s: (-int(f[s]), -s))
    out = np.zeros(M + 1, np.int32)
    at = 0
    for d in range(1, D + 1):
        for s in order[at: at + cnt[d]]:
            out[s] = d
        at += cnt[d]
    assert at == k
    return out, info


def cost(f, l):
    """sum f * l in Python ints (counts near 2^33 times lengths stay exact anyway)."""
    return sum(int(a) * int(b) for a, b in zip(np.asarray(f).tolist(), np.asarray(l).tolist()))


def package_merge_cost(freq, D):
    """The least sum f * l over binary prefix codes of the present symbols with every l <= D
    (Larmore and Hirschberg's package-merge), k >= 2 and 2^D >= k."""
    w = sorted(int(x) for x in np.asarray(freq).tolist() if int(x) > 0)
    k = len(w)
    assert k >= 2 and (1 << D) >= k
    leaves = [(x, 1) for x in w]   # (weight, leaves inside); the cost needs only the weights' sum
    cur = list(leaves)
    for _ in range(D - 1):
        packs = [(cur[i][0] + cur[i + 1][0], 0) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + packs, key=lambda p: p[0])
    # the 2k - 2 cheapest items of the last list: each leaf inside an item adds one to its length,
    # so the cost is the sum of the chosen items' weights
    return sum(p[0] for p in cur[: 2 * k - 2])


def _geometric(r, m=256):
    return np.maximum(np.round(1e12 * r ** np.arange(m)), 1).astype(np.uint64)


def _fib(m):
    a = [1, 1]
    while len(a) < m:
        a.append(a[-1] + a[-2])
    return np.array(a[:m], np.uint64)


def _depth_case(depth):
    """Counts 2^(depth-1-i), i < depth, and one more of count 1: natural depth = depth at n = 2."""
    return np.array([1 << (depth - 1 - i) for i in range(depth)] + [1], np.uint64)


def histograms():
    """name -> (counts, M)."""
    rng = np.random.default_rng(11)
    flat = np.ones(256, np.uint64) * 1000
    flat257 = np.zeros(257, np.uint64)
    flat257[:] = 1000
    big = (np.uint64(1) << np.uint64(33)) - rng.integers(0, 1000, 200).astype(np.uint64)
    big[:40] = _fib(40)   # a deep tail under counts near 2^33
    h = {
        "k1": (np.array([0, 0, 7], np.uint64), 258),
        "k2": (np.array([5, 0, 0, 9], np.uint64), 258),
        "flat256": (flat, 258),
        "flat256+256": (flat257, 258),
        "pow2_18": (np.array([1 << (17 - i) for i in range(18)], np.uint64), 258),
        "fib40": (_fib(40), 258),
        "geo0.8": (_geometric(0.8), 258),
        "geo0.9": (_geometric(0.9), 258),
        "equal200": (np.full(200, 3, np.uint64), 258),
        "near2^33": (big, 258),
        "m1023": (np.concatenate([_fib(30), rng.integers(1, 50, 970).astype(np.uint64)]), 1023),
    }
    return h


CAP_BITS = (8, 12, 15, 32)
ARITIES = (2, 3, 4, 9, 10, 16)


def cases():
    """(name, counts, M, n, D) of every case: each histogram at every arity and every cap of
    CAP_BITS bits that holds a digit; flat256 at n = 2, D = 8 (k = n^D) and flat256+256 there
    (infeasible) are among them; and the two "natural depth" cases at n = 2: a tree whose depth is
    D exactly (the cap does not bind) and D + 1 (it binds by one)."""
    out = []
    for name, (f, M) in histograms().items():
        for n in ARITIES:
            for D in sorted({b // digit_bits(n) for b in CAP_BITS}):
                if D >= 1:
                    out.append((f"{name}-n{n}-D{D}", f, M, n, D))
    for D in (8, 12, 15):
        out.append((f"depth=D-n2-D{D}", _depth_case(D), 258, 2, D))
        out.append((f"depth=D+1-n2-D{D}", _depth_case(D + 1), 258, 2, D))
    return out
