"""The model of the batch Huffman bodies (tests/batch_body_model.py) without a device: pinned to
the oracle (every expected stream decodes through orc.huff_unpack, expected_batch of SEGMENTS is
the three existing oracles' batch), and one test_<family>_reach_* per row of DESIGN.md section 6
"The batch Huffman bodies at their own edges" that asserts FROM THE MODEL'S GEOMETRY that the
catalogue plants what the row says. tests/test_gpu_batch_edges.py runs the same catalogue on the
device."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import batch_body_model as M
from tests.test_batch_cpu import SEGMENTS, oracle_batch
from tests.test_batch_set_cpu import oracle_set_batch, set_records
from tests.test_batch_shared_cpu import oracle_text_batch, text_table

ARRAYS = ("mode", "bits", "pay_off", "payload", "sync_off", "sync_len")


def _enc(fam):
    return [c for c in M.family(fam) if c.kind == "enc"]


def _dec(fam):
    return [c for c in M.family(fam) if c.kind == "dec"]


def _coded_items(case):
    """(segment index, bytes, record) of the coded segments of a decode case"""
    return [(i, s, case.records[k]) for i, (s, k) in enumerate(case.items) if k is not None and len(s)]


# ---- the model is the oracle's -------------------------------------------------------------------
@pytest.mark.parametrize("fam", M.FAMILIES)
def test_every_hand_stream_decodes_through_the_oracle(fam):
    for case in _dec(fam):
        if case.damage is not None:
            continue
        b = M.hand_batch(case.mode, case.items, case.n_ary, case.S, case.records)
        assert (b["pay_off"] % 16 == 0).all()
        for i, s, rec in _coded_items(case):
            m, bits, pay, sl = M.segment_view(b, i)
            assert m == 1 and bits <= 8 * len(s) and pay.size == M.pad16((bits + 7) // 8), (case, i)
            assert int(sl.astype(np.int64).sum()) == bits and sl.size == -(-len(s) // case.S)
            assert not pay[(bits + 7) // 8:].any() and (bits % 8 == 0 or pay[bits // 8] & (0xFF >> (bits % 8)) == 0)
            got = orc.huff_unpack(pay, bits, len(s), rec["enc_len"], rec["enc_val"], case.n_ary)
            assert np.array_equal(got, s), (case, i)


def test_model_decode_agrees_with_the_oracle_on_undamaged_streams():
    for name in M.RECORD_NAMES:
        case = M.case(f"codes-{name}-own-dec")
        b = case.batch()
        for i, s, rec in _coded_items(case):
            st, out = M.model_decode(rec, *M.segment_view(b, i), len(s), case.S)
            assert st == M.DC_OK and np.array_equal(out, s), (name, i)


@pytest.mark.parametrize("name", ("window-shared-dec", "codes-b32-shared-dec", "codes-n17-shared-dec", "codes-n3-shared-dec",
                                  "chunks-S16-shared-dec", "chunks-S1024-b32-shared-dec"))
def test_decode_geometry_is_model_decodes_trace(name):
    """the closed forms of decode_geometry (wbits before the refill test, the refill, the code found,
    the highest word index of a chunk) against what model_decode does symbol by symbol"""
    case = M.case(name)
    b = case.batch()
    for i, s, rec in _coded_items(case)[:24]:
        trace = []
        assert M.model_decode(rec, *M.segment_view(b, i), len(s), case.S, trace=trace)[0] == M.DC_OK
        g = M.decode_geometry(rec, s, case.S, 64)
        assert [c * case.S + j for c, j, *_ in trace] == g["sym"].tolist()
        assert [pre for _, _, pre, _, _ in trace] == g["wpre"].tolist(), (name, i)
        assert [nb for _, _, _, nb, _ in trace] == g["n"].tolist()
        assert [pre < 32 for _, _, pre, _, _ in trace] == g["refill"].tolist()
        last = {}
        for c, _, _, _, k in trace:
            last[c] = k - 1
        assert [last[c] for c in range(g["nch"])] == g["word_max"].tolist(), (name, i)
        assert g["nw"] == M.segment_view(b, i)[2].size // 4


def test_expected_batch_is_the_existing_oracles():
    own = M.expected_batch("own", SEGMENTS, 2, 64)
    ref = oracle_batch(SEGMENTS, 2, 64)
    for k in ARRAYS + ("lens",):
        assert np.array_equal(own[k], ref[k]), k
    rec = M.make_record(text_table(2)[:256], 2)
    sh = M.expected_batch("shared", SEGMENTS, 2, 64, [rec])
    ref = oracle_text_batch(2, 64)
    for k in ARRAYS:
        assert np.array_equal(sh[k], ref[k]), k
    recs = [M.make_record(np.asarray(r)[:256], 2) for r in set_records(2)]
    st = M.expected_batch("set", SEGMENTS, 2, 64, recs)
    ref = oracle_set_batch(SEGMENTS, set_records(2), 2, 64)
    for k in ARRAYS + ("tid",):
        assert np.array_equal(st[k], ref[k]), k


def test_the_catalogue_is_small_and_named():
    cs = M.catalogue()
    assert len({c.name for c in cs}) == len(cs) and {c.family for c in cs} == set(M.FAMILIES)
    for c in cs:
        segs = c.segs if c.kind == "enc" else [s for s, _ in c.items]
        assert all(len(s) <= M.SEG_MAX for s in segs) and len(segs) <= 300, c


# ---- codes ---------------------------------------------------------------------------------------
def test_codes_reach_every_length_both_sides_of_the_lut():
    want = {"n16": (12, 16), "n17": (10, 15), "n256": (8, 16), "b13": (12, 13), "b12": (12, None)}
    for name in M.RECORD_NAMES:
        rec = M.record(name)
        lengths = {b for b in rec["by"] if b <= 32}
        for mode in ("own", "shared", "set"):
            case = M.case(f"codes-{name}-{mode}-dec")
            used = set()
            for i, s, r in _coded_items(case):
                assert r is rec
                used |= set(rec["nbits"][s].tolist())
            if name == "n256":   # a 16-bit code never fits 8 len bits: reached by the damage family alone
                assert used == {8} and 16 in lengths
                continue
            assert used == lengths, (name, mode)
        if name in want:
            inside, beyond = want[name]
            assert inside in lengths and inside <= M.HB_LUT_BITS and (beyond is None or (beyond in lengths and beyond > M.HB_LUT_BITS))
    assert max(M.record("n17")["by"]) == 30 and max(M.record("b32")["by"]) == 32
    for name in ("n3", "n5"):   # incomplete: a window with no code exists
        rec = M.record(name)
        assert any(M.lookup(rec, w << 24)[1] == 0 for w in range(256)), name
    assert not M.record_valid(np.ones(256), 2) and M.record_valid(M.record("n3")["lens"], 3)


def test_codes_reach_the_longest_code_at_chunk_edges():
    for name in M.RECORD_NAMES:
        if name in ("f8", "n256"):
            continue
        rec = M.record(name)
        top = max(b for b in rec["by"] if b <= 32)
        case = M.case(f"codes-{name}-shared-dec")
        x = case.items[0][0]
        nb = rec["nbits"][x]
        assert nb[64] == top and nb[127] == top and nb[700 - 1] == top, name     # first and last of a chunk
        assert rec["nbits"][case.items[3][0]][0] == top                         # reversed: first of the segment
        g = M.decode_geometry(rec, x, 64, 64)
        assert g["slow"].any() == (top > M.HB_LUT_BITS)
    # the encode of the same bytes, through shared and set
    assert {c.mode for c in _enc("codes")} == {"shared", "set"}
    exp = M.case("codes-n17-shared-enc").expected()
    assert exp["mode"].tolist() == [1, 1, 1]


# ---- window --------------------------------------------------------------------------------------
def test_window_reach_32_bit_codes_at_every_position():
    rec = M.record("b32")
    case = M.case("window-shared-dec")
    nacc32, wpre = set(), set()
    runs4 = False
    for s, _ in case.items:
        g = M.pack_geometry(rec, s)
        long = g["n"] == 32
        nacc32 |= set(g["nacc"][long].tolist())
        assert (g["shift"] >= 0).all() and (g["shift"] + g["n"] <= 64).all()
        runs4 = runs4 or (np.convolve(long.astype(int), np.ones(4, int), "valid") == 4).any()
        d = M.decode_geometry(rec, s, 64, 64)
        wpre |= set(d["wpre"][d["n"] == 32].tolist())
    assert {0, 1, 31} <= nacc32 and runs4
    assert {32, 31} <= wpre           # a 32-bit lookup with exactly 32 bits (no refill) and with 31 (refill)
    ones = case.items[6][0]
    assert (rec["nbits"][ones] == 1).all() and ones.size > 64 * 5


def test_window_reach_the_end_of_the_payload():
    rec = M.record("b32")
    case = M.case("window-shared-dec")
    mod128, mod32, past = set(), set(), set()
    for s, _ in case.items:
        g = M.pack_geometry(rec, s)
        if g["n"][-1] == 32:
            mod128.add(g["bits"] % 128)
            mod32.add(g["bits"] % 32)
        d = M.decode_geometry(rec, s, 64, 64)
        past |= set((d["word_max"] - d["nw"]).tolist())
        assert g["psize"] == M.pad16(-(-g["bits"] // 8)) and g["words"] * 4 <= g["psize"]
    assert {0, 1, 127} <= mod128 and {0, 1, 31} <= mod32
    # HB_WORD(k + 1) and the refill's word at nw (zero) and inside; a valid stream never asks for a word
    # past nw (a chunk that starts in the last word ends in it)
    assert 0 in past and any(p < 0 for p in past) and max(past) == 0


# ---- units ---------------------------------------------------------------------------------------
def test_units_reach_every_cut_of_the_pack():
    case = M.case("units-shared-lead0-after00")
    lens = [len(s) for s in case.segs]
    assert set(M.UNIT_LENS) <= set(lens) and lens[-1] == 65536 and len(set(case.segs[-1].tolist())) == 1
    rec = case.records[0]
    units = {M.pack_geometry(rec, s)["units"] for s in case.segs}
    assert {1, 2, 255, 256, 257, 17, 16 * 255 + 1, 4096} <= units      # 16 t + 1 units: t = 1, 255
    rounds = {M.pack_geometry(rec, s)["rounds"] for s in case.segs}
    assert {1, 2, 16} <= rounds
    g = M.pack_geometry(rec, case.segs[lens.index(65536)])
    assert g["scan_threads"] == 256 and g["units_last_thread"] == 16
    assert M.pack_geometry(rec, case.segs[lens.index(17)])["units_last_thread"] == 2
    g = M.pack_geometry(rec, case.segs[lens.index(16 * 16 + 1)])
    assert (g["scan_threads"], g["units_last_thread"]) == (2, 1)
    g = M.pack_geometry(rec, case.segs[lens.index(16 * 16 * 255 + 1)])
    assert (g["scan_threads"], g["units_last_thread"], g["rounds"]) == (256, 1, 16)


def test_units_reach_every_alignment_and_the_guarded_dwords():
    a_seen, mis_seen, short_head = set(), set(), False
    after = set()
    for case in _enc("units"):
        after.add(case.after)
        at = case.lead
        for s in case.segs:
            g = M.load_geometry(len(s), at)
            a_seen |= set(g["a"].tolist())
            mis_seen.add(g["mis"])
            short_head = short_head or (0 < len(s) < g["mis"])
            # the guard drops a dword only when all of it lies past the end
            assert g["past"][:, 0].sum() == 0
            at += len(s)
    assert a_seen == {0, 1, 2, 3} and mis_seen == {0, 1, 2, 3} and short_head
    assert after == {0x00, 0xFF, 0xEE}
    hole = M.case("units-shared-lead3-afteree").records[0]
    assert hole["nbits"][0xEE] == 0 and hole["nbits"][0xFF] > 0
    assert {c.lead for c in _enc("units") if "align" in c.name} == set(range(16))
    # what follows the segments never changes what is expected
    a, b = M.case("units-own-lead3-after00").expected(), M.case("units-own-lead3-afterff").expected()
    assert all(np.array_equal(a[k], b[k]) for k in ARRAYS)


# ---- chunks --------------------------------------------------------------------------------------
def test_chunks_reach_every_round_of_both_scans():
    for S in (16, 64, 1024):
        case = M.case(f"chunks-S{S}-shared-dec")
        lens = [len(s) for s, _ in case.items]
        nch = [-(-n // S) for n in lens]
        want = [c for c in M.CHUNK_COUNTS if (c - 1) * S + 1 <= M.SEG_MAX]
        assert set(want) <= set(nch), S
        deal = M.deal_shared(lens)
        wave = {c for j, c in enumerate(nch) if deal[j // 4][0] == "wave"}
        wg = {c for j, c in enumerate(nch) if deal[j // 4][0] == "wg"}
        if S == 64:
            assert {1, 63, 64, 65} <= wave and {255, 256, 257, 513} <= wg
        if S == 16:
            assert 512 in wave and 4096 in wg and {255, 256, 257, 513} & wg
        assert {n % S for n in lens} >= {1, S - 1}
    rec = M.record("b16")
    x = M.case("chunks-S64-shared-dec").items[4][0]
    g = M.geometry(rec, x, 64)["decode"]
    assert g["nch"] == 64 and g["rounds"] == 1
    assert M.decode_geometry(rec, M.case("chunks-S64-shared-dec").items[6][0], 64, 64)["rounds"] == 2
    x = next(s for s, _ in M.case("chunks-S64-shared-dec").items if -(-len(s) // 64) == 257)
    assert M.decode_geometry(rec, x, 64, 256)["rounds"] == 2


def test_chunks_reach_a_chunk_of_32768_bits():
    case = M.case("chunks-S1024-b32-shared-dec")
    rec = case.records[0]
    g = M.decode_geometry(rec, case.items[0][0], 1024, 64)
    assert 32768 in g["clen"].tolist() and g["clen"].max() <= 65535
    assert M.case("chunks-S1024-b32-enc").expected()["mode"].tolist() == [1]


# ---- phase ---------------------------------------------------------------------------------------
PHASE_INSTANCES = (("phase-wave-mode1-shared", "wave"), ("phase-wave-mode0-shared", "wave"), ("phase-wave-mode1-set", "wave"),
                   ("phase-wave-mode0-set", "wave"), ("phase-wg-mode1-shared", "wg"), ("phase-wg-mode0-shared", "wg"),
                   ("phase-wg-mode1-set", "wg"), ("phase-wg-mode0-set", "wg"), ("phase-wg-mode1-own", None), ("phase-wg-mode0-own", None))
PHASE_PAIRS = {(n, ph) for n in M.PHASE_SIZES for ph in range(16)}


@pytest.mark.parametrize("name,path", PHASE_INSTANCES)
def test_phase_reach_every_phase_times_every_size(name, path):
    seen = set()
    for half, sizes in M.PHASE_HALVES:
        case = M.case(f"{name}-{half}")
        lens = [len(s) for s, _ in case.items]
        assert {int(m) for m in case.batch()["mode"]} == {int(name[name.index("mode") + 4])}
        if path:   # every group of four takes the instance the case is named for
            assert {d[0] for d in M.deal_shared(lens)} == {path}, name
        seen |= {(n, ph) for n, ph in zip(lens, case.phases) if n in sizes}
    assert len(PHASE_PAIRS) == 16 * 20 and seen == PHASE_PAIRS, name
    geo = {pair: M.write_geometry(pair[1], pair[0]) for pair in seen}
    assert geo[(3, 1)]["below_head"] and geo[(14, 1)]["below_head"] and not geo[(15, 1)]["below_head"]
    # the last byte at 127, 128 and 129 of the stage: either side of the first 128-byte pad
    assert not geo[(127, 1)]["crosses_pad"] and geo[(128, 1)]["crosses_pad"] and geo[(127, 2)]["crosses_pad"]
    assert not geo[(128, 0)]["crosses_pad"] and geo[(129, 0)]["crosses_pad"] and geo[(8192, 15)]["crosses_pad"]
    assert any(g["head"] and g["nbody"] and g["tail"] for g in geo.values()) and any(g["nbody"] == 0 for g in geo.values())
    assert M.oidx(127) + 5 == M.oidx(128)


def test_phase_reach_ranges_with_partial_chunks():
    for mode in ("shared", "set", "own"):
        case = M.case(f"phase-ranges-{mode}")
        rec, x = case.records[0], case.items[0][0]
        assert len(case.rows()) == len(case.range_phases) == 16 * 20
        for (i, f, c), ph in zip(case.rows(), case.range_phases):
            g = M.decode_geometry(rec, x, 64, 64, phase=ph, first=f, count=c)
            assert g["first_partial"] and g["last_partial"] and g["row_negative"] and g["phase"] == ph
        assert {(c, ph) for (_, _, c), ph in zip(case.rows(), case.range_phases)} == PHASE_PAIRS


# ---- mode ----------------------------------------------------------------------------------------
def test_mode_reach_equality_in_every_plan():
    t89 = M.record("t89")
    case = M.case("mode-t89-shared")
    cost = [int(t89["nbits"][s].sum()) - 8 * len(s) for s in case.segs]
    assert cost == [-1, 0, 1, -1, 0, 1]
    assert case.expected()["mode"].tolist() == [1, 0, 0, 1, 0, 0]
    exp = M.case("mode-hole-shared").expected()
    assert exp["mode"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0]          # a byte without a code: first, last, only
    assert not M.case("mode-f8-shared").expected()["mode"].any()
    case = M.case("mode-set")
    exp = case.expected()
    assert not M.record_valid(case.records[0]["lens"], 2)              # the invalid record is cheapest, and never taken
    assert exp["tid"].tolist() == [2, 1, 1, 2, 1, 1, 2, 2, 1] and exp["mode"].tolist() == [1, 0, 0, 1, 0, 0, 1, 1, 0]
    exp = M.case("mode-set-hole-first").expected()
    assert exp["tid"].tolist()[:6] == [0] * 6 and exp["tid"].tolist()[6:] == [1, 1, 1] and exp["mode"].tolist()[6:] == [1, 1, 0]
    own = M.case("mode-own-equality")
    exp = own.expected()
    L = orc.huffman_lengths(orc.histogram(own.segs[0]), 2)[:256]
    assert int((np.bincount(own.segs[0], minlength=256) * L).sum()) == 8 * len(own.segs[0])
    assert exp["mode"][0] == 0 and exp["bits"][0] == 8 * len(own.segs[0])


def test_depth_weight_bound_holds_for_the_oracle():
    """the bound that "not reachable" rests on, against orc.huffman_lengths: on the chain family it
    is within the family's own weight, and no drawn histogram is lighter than it for its depth"""
    rng = np.random.default_rng(1)
    for n_ary in (2, 3, 5, 17):
        for levels in range(2, 9):
            c = M.chain_counts(n_ary, levels)
            if c.size <= 256:
                assert int(M.lengths_of_counts(c, n_ary).max()) == levels, (n_ary, levels)
                assert M.depth_weight_bound(n_ary, levels) <= int(c.sum())
        for _ in range(200):
            cnt = np.maximum(1, (rng.pareto(0.6, int(rng.integers(1, 257))) * 3).astype(np.int64))
            depth = int(M.lengths_of_counts(cnt, n_ary).max())
            assert int(cnt.sum()) >= M.depth_weight_bound(n_ary, depth), (n_ary, cnt.tolist())


@pytest.mark.parametrize("n_ary", (2, 3, 17))
def test_mode_own_tables_never_pass_32_bits(n_ary):
    """NOT REACHABLE at n = 2, 3, 17: `maxbits <= 32` of k_hb_plan is never false for a segment of at
    most 65536 bytes. depth_weight_bound (the argument is in its docstring) of the first depth
    that passes 32 bits is more than a segment holds: 9227464, 174761 and 110433 bytes."""
    need = M.over_32_digits(n_ary)
    assert need * M.digit_bits(n_ary) > 32 >= (need - 1) * M.digit_bits(n_ary)
    assert M.depth_weight_bound(n_ary, need) == {2: 9227464, 3: 174761, 17: 110433}[n_ary] > M.SEG_MAX
    assert M.own_over_32(n_ary) is None


def test_mode_reach_an_own_table_over_32_bits_at_n5():
    """REACHABLE at n = 5: 44 byte values, 57248 bytes, codes of 11 digits = 33 bits"""
    counts = M.own_over_32(5)
    assert counts is not None and counts.size == 44 and int(counts.sum()) == 57248 <= M.SEG_MAX
    assert M.depth_weight_bound(5, 11) <= 57248
    case = M.case("mode-own-over32-n5")
    below, big = case.segs[0], case.segs[1]
    L = orc.huffman_lengths(orc.histogram(big), 5)[:256]
    assert int(L.max()) == 11 and not M.own_usable(L, 5)
    assert orc.bitcodes(*orc.canonical(L, 5), 5)[2] == -1                # the oracle has no bit code for it
    Lb = orc.huffman_lengths(orc.histogram(below), 5)[:256]
    assert int(Lb.max()) == 10 and M.own_usable(Lb, 5)                   # one digit below: 30 bits, coded
    exp = case.expected()
    assert exp["mode"].tolist() == [1, 0, 1, 0] and exp["bits"][1] == 8 * len(big)
    assert np.array_equal(exp["lens"][1], L) and np.array_equal(exp["lens"][3], L) and exp["lens"][1].max() == 11
    s0, s1 = int(exp["pay_off"][1]), int(exp["pay_off"][2])
    assert np.array_equal(exp["payload"][s0: s0 + len(big)], big) and s1 - s0 == M.pad16(len(big))
    # the decoder: the stored segment under that record is taken, one that claims to be coded under it refused
    stored, as_coded = M.case("mode-own-over32-n5-stored-dec"), M.case("mode-own-over32-n5-coded-dec")
    for c in (stored, as_coded):
        assert np.array_equal(c.batch()["lens"][1], L) and c.batch()["lens"][0].max() == 10
    assert stored.batch()["mode"].tolist() == [1, 0, 1] and stored.outcome()[0] == [M.DC_OK] * 3
    assert np.array_equal(stored.outcome()[1][1], big)
    assert as_coded.batch()["mode"].tolist() == [1, 1, 1] and as_coded.outcome()[0] == [M.DC_OK, M.DC_E_STREAM, M.DC_OK]
    assert {M.range_outcome(as_coded, r)[0] for r in as_coded.rows() if r[0] == 1} == {M.DC_E_STREAM}
    assert {M.range_outcome(stored, r)[0] for r in stored.rows()} == {M.DC_OK}


# ---- deal ----------------------------------------------------------------------------------------
def test_deal_reach_every_count_and_path():
    counts = {len(c.items) for c in _dec("deal") if "count" in c.name}
    assert counts == {1, 2, 3, 4, 5, 7, 8}
    assert {c.grid for c in _dec("deal")} == {0, 1, 2}
    case = M.case("deal-groups-shared-grid0")
    paths = [p for p, _ in M.deal_shared([len(s) for s, _ in case.items])]
    assert "wave" in paths and "wg" in paths
    assert any(len(s) == 0 for s, _ in case.items) and any(len(s) == 8193 for s, _ in case.items)


def test_deal_reach_have_kept_rebuilt_and_reset():
    seen = set()
    for grid in (1, 2, 0):
        for name in (f"deal-groups-set-grid{grid}", f"deal-badtid-set-grid{grid}"):
            case = M.case(name)
            b = case.batch()
            lens = [len(s) for s, _ in case.items]
            tr = M.deal_set(lens, b["mode"].tolist(), b["tid"].tolist(), case.records, 2, grid)
            assert len(tr) == 6 and {t["wg"] for t in tr} == set(range(M.grid_of(6, grid)))
            for t in tr:
                seen |= {(grid, t["path"], e) for e in t["events"]}
            if "badtid" in name:
                st, _ = case.outcome()
                assert [i for i, v in enumerate(st) if v] == [2, 14] and st[2] == M.DC_E_STREAM
                assert b["tid"][17] == 255 and b["mode"][17] == 0
    # grid 1: one workgroup keeps, rebuilds and loses its table; the default grid: a workgroup a group
    assert {(1, "wave", "kept"), (1, "wg", "kept"), (1, "wg", "built"), (1, "wg", "reset"), (1, "wave", "built"),
            (2, "wg", "built"), (0, "wave", "built")} <= seen, seen
    tr = M.deal_set([len(s) for s, _ in M.case("deal-groups-set-grid1").items], M.case("deal-groups-set-grid1").batch()["mode"].tolist(),
                    M.case("deal-groups-set-grid1").batch()["tid"].tolist(), M.case("deal-groups-set-grid1").records, 2, 1)
    assert [t["path"] for t in tr] == ["wave", "wg", "wave", "wg", "wave", "wave"]


# ---- damage --------------------------------------------------------------------------------------
def test_damage_reach_both_outcomes_and_stays_inside_the_payload():
    outcomes = set()
    for mode in ("own", "shared", "set"):   # all bad, then all good
        names = [c.name for c in _dec("damage")]
        assert names.index(f"damage-b16-all-good-{mode}") == names.index(f"damage-b16-all-bad-{mode}") + 1
        assert M.case(f"damage-b16-all-bad-{mode}").outcome()[0] == [M.DC_E_STREAM] * 8
        assert M.case(f"damage-b16-all-good-{mode}").outcome()[0] == [M.DC_OK] * 8
    for case in _dec("damage"):
        if "-all-" in case.name:
            continue
        clean = M.hand_batch(case.mode, case.items, case.n_ary, case.S, case.records)
        b = case.batch()
        for k in ("pay_off", "sync_off", "mode"):          # the damage is in payload bits, sync entries and bits alone
            assert np.array_equal(clean[k], b[k]), (case, k)
        changed = [i for i in range(len(case.items)) if any(
            not np.array_equal(x, y) for x, y in zip(M.segment_view(clean, i)[1:], M.segment_view(b, i)[1:]))]
        assert len(changed) == 1, case
        i = changed[0]
        st, out = case.outcome()
        assert all(v == M.DC_OK for j, v in enumerate(st) if j != i)
        if st[i] == M.DC_OK:
            assert out[i] is not None
            outcomes.add("ok-same" if np.array_equal(out[i], case.items[i][0]) else "ok-other")
        else:
            assert st[i] == M.DC_E_STREAM and out[i] is None
            outcomes.add("stream")
        # every word read lies in the segment's padded payload or is past nw, where HB_WORD gives zero
        rec, (m, bits, pay, sl) = case.records[-1], M.segment_view(b, i)
        # (a trace entry's k: the indices read so far are below it)
        trace = []
        M.model_decode(rec, m, bits, pay, sl, len(case.items[i][0]), case.S, trace=trace)
        nw = pay.size // 4
        assert pay.size == int(b["pay_off"][i + 1] - b["pay_off"][i]) and pay.size % 16 == 0   # index < nw: the segment's own bytes
        pos = np.concatenate(([0], np.cumsum(sl.astype(np.int64))))
        assert trace and int(pos[-1]) <= 8 * pay.size
        for c, j, pre, nb, k in trace:
            # a chunk starts inside the payload, reads two words and at most one more a symbol: no
            # index is past the chunk's first word + 1 + the symbols decoded so far
            assert int(pos[c]) >> 5 < nw or int(pos[c]) == 8 * pay.size, (case, c)
            assert 2 <= k <= (int(pos[c]) >> 5) + 2 + j + 1 and 0 <= nb <= 32, (case, c, j)
        top = max(k for *_, k in trace) - 1
        assert top <= nw                                        # in this catalogue: the one zero word at nw at the most
        clean_trace = []
        assert M.model_decode(rec, *M.segment_view(clean, i), len(case.items[i][0]), case.S, trace=clean_trace)[0] == M.DC_OK
        assert max(k for *_, k in clean_trace) - 1 <= nw         # the valid stream: index nw at the most
        if top == nw:
            outcomes.add("at nw")
        # a range that does not touch the damaged chunk is exact
        rows = [r for r in case.rows() if r[0] == i and r[2]]
        got = {M.range_outcome(case, r)[0] for r in rows}
        assert M.DC_OK in got or "bits" in case.name, case
    assert {"stream", "ok-other", "at nw"} <= outcomes, outcomes
    two = M.case("damage-n256-two-digit-own")
    trace = []
    M.model_decode(two.records[-1], *M.segment_view(two.batch(), 1), len(two.items[1][0]), 64, trace=trace)
    assert 16 in {nb for _, _, _, nb, _ in trace}          # the two-digit code of n = 256 is read, and refused
    assert two.outcome()[0][1] == M.DC_E_STREAM
