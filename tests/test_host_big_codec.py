"""The table of tests/big_codec.py without a GPU.

At the small crossing point FAR = 2^16 (the codec's chunk of 16 384 samples allows no smaller one) every closed form is
compared with brute force on the dense channels -- np.bincount for the histograms, the CPU oracle for what mh_measure and
mh_encode compute from them, a loop over the segments for the compaction -- and shown to differ from what an index cut
modulo FAR would give.  At full length, without building anything of that size: the plan of case A through
tests/planner_check.cpp (directory, workgroup tasks, histogram and calibration tiles) against the oracle's directory and
a Python restatement, with the first entry of each that passes 2^32; the work lists of the range and re-bin calls; the
launch numbers of k_rebin3 behind its grid cap; the no-fault rule for every large buffer; the bit rate of the drifted
filling."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import big_codec as bc
from tests import helpers
from tests.test_host_launch_geometry import YMAX, _ints, _rebin
from tests.test_host_launch_geometry import _run as geometry
from tests.test_host_worklist import _run as worklists
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

OC = oracle.c
SMALL, FULL = 1 << 16, 1 << 32
TABS = helpers.sclv_tables()
FILLS = list(bc.FILLINGS)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def small():
    return {name: make(SMALL) for name, (_S, make) in bc.FILLINGS.items()}


def _plan_line(S, h, window, lens, sc=2):
    tab = TABS[S]
    return "%d %d %d 1 %d %d %d  %s  %s" % (len(lens), S, h, window, len(tab), sc, " ".join(map(str, lens)),
                                           " ".join(str(int(v)) for v in tab.ravel()))


def test_the_table():
    assert [c.id for c in bc.CASES] == ["A-measure", "A-codec", "A-compact", "A-range", "A-decode-rebin", "A-rebin", "A-sweep", "B-compact",
                                        "C-layout", "C-packed", "C-stream"]
    assert bc.T_LONG == 6_442_455_043 == bc.t_long(FULL) and FULL % bc.P == 2304 and SMALL % bc.P != 0
    assert bc.D < bc.P < SMALL // 2 and bc.LEAD == 1 << 31 and bc.CHUNK == OC.CHUNK and bc.HDR_WORDS == OC.HDR_WORDS
    for n in (1, 63, 16383, 16384, 16385, 32768, 12345):
        for maxlen in (2, 9):
            assert bc.slot_words(n, maxlen) == OC.slot_words(n, maxlen)


# ---- at 2^16: closed form = brute force, true != cut ---------------------------------------------------------------------
@pytest.mark.parametrize("name", FILLS)
def test_a_the_histograms_are_the_brute_force_counts(small, name):
    S = bc.FILLINGS[name][0]
    rng = np.random.RandomState(3)
    for ch in small[name]:
        x = ch.dense()
        assert np.array_equal(ch.at(np.arange(ch.n)), x)
        cuts = [0, 1, 63, 64, 65, bc.D, bc.D + 1, bc.P, SMALL - 1, SMALL, SMALL + 1, ch.n - 1, ch.n]
        cuts = sorted(set(min(c, ch.n) for c in cuts) | set(int(v) for v in rng.randint(0, ch.n + 1, size=12)))
        for a in cuts[::3] + [0]:
            for b in cuts:
                if b < a:
                    continue
                for lim in (S, 10, 256):
                    want = np.bincount(np.minimum(x[a:b], lim - 1), minlength=lim)
                    assert np.array_equal(ch.hist(a, b, lim), want), (name, a, b, lim)
    long_ = small[name][1]
    assert bc.decoys_tell(long_, SMALL) and bc.decoys_tell(bc.FILLINGS[name][1](FULL)[1], FULL)
    cut = long_.cut(SMALL)
    assert not np.array_equal(np.bincount(np.minimum(cut, S - 1), minlength=S), long_.hist(0, long_.n, S))
    # ... and a cut read differs from the true one exactly behind FAR, at every planted sample there
    diff = np.flatnonzero(cut != long_.dense())
    assert diff.min() >= SMALL and {i for i, _v in long_.planted if i >= SMALL} <= set(diff.tolist())


@pytest.mark.parametrize("h,win", [(6, OC.WIN_FULL), (12, OC.WIN_AFTER_CAL), (30, OC.WIN_AFTER_CAL)])
@pytest.mark.parametrize("name", FILLS)
def test_a_the_measure_restatement_is_the_oracle(small, name, h, win):
    """peak = the first maximum, enc = the first minimum of table . rank-ordered counts, the histograms in rank order, bits"""
    S = bc.FILLINGS[name][0]
    chs, tab = small[name], TABS[S]
    data, off, ln = OC.flatten([c.dense() for c in chs])
    om = OC.measure(data, off, ln, OC.Params(S, h, 1, win, tab))
    for c, m in enumerate(bc.expect_measure(chs, S, h, win == OC.WIN_AFTER_CAL, tab, OC.approx_sort_rule)):
        assert (m["cutoff"], m["peak"], m["enc"], m["bits"]) == (int(om["cutoff"][c]), int(om["peak"][c]), int(om["enc"][c]), int(om["bits"][c]))
        assert np.array_equal(m["cal_hist"], om["cal_sorted"][c]) and np.array_equal(m["post_hist"], om["post_mapped"][c])
        assert om["skipped"][c] == 0


@pytest.mark.parametrize("name", FILLS)
def test_a_ch_bits_and_the_round_trip_of_the_oracle(small, name):
    """ch_bits = sum over the symbols of count x code length; the oracle decodes its own stream to min(x, S - 1); the
    segments the GPU test takes to the oracle are one-segment channels there"""
    S = bc.FILLINGS[name][0]
    chs, tab = small[name], TABS[S]
    data, off, ln = OC.flatten([c.dense() for c in chs])
    p = OC.Params(S, 6, 1, OC.WIN_FULL, tab, seg_chunks=2)
    e = OC.encode(data, off, ln, p)
    want = bc.expect_measure(chs, S, 6, False, tab, OC.approx_sort_rule)
    for c, m in enumerate(want):
        assert int(e["ch_bits"][c]) == int((chs[c].hist(0, chs[c].n, S) * m["lens"]).sum()) == m["bits"]
        assert (int(e["peak"][c]), int(e["enc"][c])) == (m["peak"], m["enc"])
    got = OC.decode(e["payload"], off, ln, p, e["peak"], e["enc"], data.size)
    for c, ch in enumerate(chs):
        assert np.array_equal(got[int(off[c]):int(off[c]) + ch.n], np.minimum(ch.dense(), S - 1))
    # the long channel's segments one by one under its (peak, enc): the same words as in the whole stream
    long_, T = chs[1], chs[1].n
    ids = np.flatnonzero(e["seg"]["ch"] == 1)
    assert [(int(e["seg"]["first"][s]), int(e["seg"]["n"][s])) for s in ids] == bc.segments_of(T)
    p1 = OC.Params(S, 0, 1, OC.WIN_FULL, tab, seg_chunks=2)
    for k in bc.oracle_segments(SMALL, T):
        first, n = bc.segments_of(T)[k]
        x = long_.at(np.arange(first, first + n))
        one = OC.encode_preset(np.concatenate([x, np.zeros(64, np.uint8)]), np.zeros(1, np.uint64), np.array([n], np.uint64), p1,
                               want[1]["peak"], want[1]["enc"])
        s = ids[k]
        o, w = int(e["seg"]["off"][s]), int(e["seg_words"][s])
        assert int(one["seg_words"][0]) == w and np.array_equal(one["payload"][:w], e["payload"][o:o + w]), k


def test_the_drifted_filling_costs_more_than_5_4_bits_a_sample():
    """a dense stream passes byte 2^32 inside one channel of T_LONG samples above 5.33 bits a sample"""
    tab = TABS[10]
    chs = bc.drifted_channels(FULL)
    m = bc.expect_measure(chs, 10, 6, False, tab, OC.approx_sort_rule)[1]
    assert (m["peak"], chs[1].hist(0, 64, 10)[0]) == (0, 64)
    x = np.ascontiguousarray(chs[1].period)
    p = OC.Params(10, 0, 1, OC.WIN_FULL, tab, seg_chunks=2)
    e = OC.encode_preset(np.concatenate([x, np.zeros(64, np.uint8)]), np.zeros(1, np.uint64), np.array([bc.P], np.uint64), p, m["peak"], m["enc"])
    assert int(e["ch_bits"][0]) / bc.P > 5.4
    assert m["bits"] / bc.T_LONG > 5.4 and m["bits"] > FULL and m["bits"] // 8 > FULL
    for name in ("sparse-S3", "sparse-S10"):           # the sparse fillings: a count and a bit total above 2^32 all the same
        S = bc.FILLINGS[name][0]
        ms = bc.expect_measure(bc.FILLINGS[name][1](FULL), S, 6, False, TABS[S], OC.approx_sort_rule)[1]
        assert ms["post_hist"].max() > FULL and ms["bits"] > FULL


def test_the_compaction_model_and_its_cut():
    b = bc.case_b(SMALL)
    payload = bc.payload_word(np.arange(b["payload_words"]))
    dense, off = bc.compact_model(payload, b["slot_off"], b["seg_words"])
    assert np.array_equal(off, b["dense_off"]) and dense.size == b["total"] and (dense >= 0).all()
    # the word at dense index j, as the GPU test forms it: the segment by search, then its slot
    j = np.arange(b["total"])
    seg = np.searchsorted(np.cumsum(b["seg_words"]), j, side="right")
    assert np.array_equal(dense, bc.payload_word(b["slot_off"][seg] + j - off[seg]))
    cut, _ = bc.compact_model(payload, b["slot_off"], b["seg_words"], far=SMALL)
    assert not np.array_equal(cut, dense) and (cut[SMALL:] == -1).all()
    # source offsets cut modulo FAR read other words: the payload is not cyclic in FAR ... nor in 2^32
    assert not np.array_equal(bc.payload_word(j[-8:] % SMALL), bc.payload_word(j[-8:]))
    assert not np.array_equal(bc.payload_word(np.arange(FULL, FULL + 8)), bc.payload_word(np.arange(8)))
    assert b["slot_off"][-1] > SMALL and off[-1] > SMALL and b["seg_words"][b["cross"] - 1] == 0 == b["seg_words"][b["cross"] + 1]


def test_images_of_a_cut_index_differ(small):
    """what the GPU test compares as images of the input -- decoded bytes, re-bin sums, transposes -- differs under a cut
    sample index, at the planted samples behind FAR"""
    long_ = small["drifted-S10"][1]
    x, cut = np.minimum(long_.dense(), 9), np.minimum(long_.cut(SMALL), 9)
    assert not np.array_equal(x, cut)
    for r in (2, 7, 17, 68, 100):
        s = lambda v: np.add.reduceat(v.astype(np.int64), np.arange(0, v.size, r))          # noqa: E731
        assert not np.array_equal(s(x), s(cut)), r
        # a bin index cut modulo FAR / r stores the last bins over the first ones
        nb = -(-x.size // r)
        assert nb > SMALL // r
    c = bc.case_c(SMALL)
    tm = np.stack([ch.dense() for ch in c["chs"]], 1)
    tm_cut = tm[np.arange(c["T"]) % SMALL]
    assert not np.array_equal(tm, tm_cut) and all(bc.decoys_tell(ch, SMALL) for ch in c["chs"])


# ---- at full length -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FILLS)
def test_no_access_of_case_a_leaves_its_allocation(name):
    S = bc.FILLINGS[name][0]
    a = bc.case_a(name, FULL, int(TABS[S].max()))
    assert bc.no_fault(a["accesses"]) > 0
    assert a["off"][2] > FULL and a["lens"] == [70001, bc.T_LONG, 40000] and a["peak"] < 40 * 10 ** 9
    if name == "drifted-S10":
        assert 4 * a["cap"] > 7.2e9 and a["cap"] < 1 << 31         # 7.3 GB of slots; a word offset stays below 2^31


def test_no_access_of_cases_b_and_c_leaves_its_allocation():
    b = bc.case_b(FULL)
    assert bc.no_fault(b["accesses"]) > 0
    assert b["C"] == 512 and b["nseg"] == 512 * b["per"] and 470_000 < b["nseg"] < 480_000 and 3.0e7 < b["T"] < 3.1e7
    assert b["payload_words"] > FULL + (1 << 26) and b["total"] > FULL + (1 << 24) and 90 <= b["n_zero"] <= 110
    assert b["slot_off"][b["cross"]] > b["dense_off"][b["cross"]] >= FULL - bc.slot_words(bc.SEG, 9)
    assert (b["dense_off"] >= 1 << 30).any() and (b["slot_off"] >= FULL).any() and (b["dense_off"] >= FULL).any()
    assert b["peak"] < 62 * 10 ** 9
    c = bc.case_c(FULL)
    assert bc.no_fault(c["accesses"]) > 0 and c["T"] == FULL + 4099 and c["peak"] < 50 * 10 ** 9


@pytest.mark.parametrize("S,h,window", [(3, 6, 3), (10, 6, 3), (10, 30, 2)])
def test_the_plan_of_case_a_at_full_length(exe, S, h, window):  # noqa: F811
    """directory, workgroup tasks and tiles of channels of 70 001, T_LONG and 40 000 samples: the oracle's directory, a Python
    restatement, and where each first passes 2^32 (the program itself checks every task against the directory in 64 bits)"""
    lens = [70001, bc.T_LONG, 40000]
    line = _plan_line(S, h, window, lens) + "\n"
    r = subprocess.run([exe], input=line, capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.splitlines()
    nseg, cap, sc, wave, _tickets = (int(v) for v in out[0].split())
    got = {k: np.array(out[1 + i].split(), dtype=np.uint64) for i, k in enumerate(("ch", "first", "n", "off"))}
    want = OC.plan_segments(np.array(lens, np.uint64), OC.Params(S, h, 1, window, TABS[S], seg_chunks=2))
    assert (sc, wave) == (2, 0) and cap == want["cap_words"] + 4
    for k in got:
        assert np.array_equal(got[k], want[k].astype(np.uint64)), k
    maxlen = int(TABS[S].max())
    win = [bc.window(T, h, window == 2) for T in lens]
    mine = [(c, f, n) for c, (_cut, w0, w1) in enumerate(win) for f, n in bc.segments_of(w1 - w0)]
    assert [(int(c), int(f), int(n)) for c, f, n in zip(got["ch"], got["first"], got["n"])] == mine and nseg == len(mine)
    slots = np.array([bc.slot_words(n, maxlen) for _c, _f, n in mine], np.int64)
    assert np.array_equal(got["off"].astype(np.int64), np.cumsum(slots) - slots)
    assert got["first"].max() >= FULL
    if S == 10:
        assert got["off"].max() >= 1 << 30                          # a slot behind byte 2^32 of the payload
    # tasks and tiles
    t = subprocess.run([exe, "--tasks"], input=line, capture_output=True, text=True, timeout=600, env=ENV)
    assert t.returncode == 0, t.stderr[-3000:]
    rows = [ln.split() for ln in t.stdout.splitlines()]
    ntask, ntile, ncal, stride, slot_full = (int(v) for v in rows[0][1:])
    assert (stride, slot_full) == (bc.SEG, bc.slot_words(bc.SEG, maxlen))
    G = np.array([r_[1:] for r_ in rows if r_[0] == "G"], dtype=np.int64)
    H = np.array([r_[1:] for r_ in rows if r_[0] == "H"], dtype=np.int64)
    Pc = np.array([r_[1:] for r_ in rows if r_[0] == "P"], dtype=np.int64).reshape(-1, 3)
    assert (len(G), len(H), len(Pc)) == (ntask, ntile, ncal)
    ch_off = np.cumsum([0] + [bc.up(T, 16) for T in lens])          # the program's channel offsets
    seg0 = [s for c in range(3) for s in range(sum(1 for m in mine if m[0] < c), sum(1 for m in mine if m[0] <= c), 4)]
    assert list(G[:, 4]) == seg0
    for src, dst, n_last, c, s0, cnt in G[::max(1, len(G) // 64)].tolist() + G[-3:].tolist():
        assert src == ch_off[c] + win[c][1] + mine[s0][1] and dst == int(got["off"][s0]) and n_last == mine[s0 + cnt - 1][2]
    assert G[:, 0].max() >= FULL
    tiles = [(c, w0 + f, min(bc.HIST_TILE, w1 - w0 - f)) for c, (_cut, w0, w1) in enumerate(win) for f in range(0, max(w1 - w0, 1), bc.HIST_TILE)]
    assert [tuple(v) for v in H.tolist()] == tiles and H[:, 1].max() >= FULL
    cal = [(c, f, min(bc.HIST_TILE, cut - f)) for c, (cut, _w0, _w1) in enumerate(win) for f in range(0, cut, bc.HIST_TILE)] if h > 12 else []
    assert [tuple(v) for v in Pc.tolist()] == cal
    if h == 30:
        assert win[1] == (1 << 30, 1 << 30, bc.T_LONG) and len(cal) == 8192 + 2     # the tiled calibration path, 2^30 samples of it


def test_the_work_lists_of_the_range_and_rebin_calls(exe):  # noqa: F811
    T, lo = bc.T_LONG, FULL - 20000
    t7 = lo // 7 * 7
    qs = ["1 1 0 %d 0 %d" % (T, T),                          # (a) one row longer than 2^32 bytes
          "3 1 0 2 %d %d 0 %d" % (lo, lo + 40000, 40013),    # (b) rows 0 and 2 are zero fill
          "1 1 %d %d 0 3" % (T - 3, T),                      # (c) three samples that end at T_LONG
          "1 1 0 %d 100 %d" % (T, -(-T // 100)),
          "1 1 0 %d 96 %d" % (T, -(-T // 96)),
          "1 1 %d %d 7 %d" % (t7, t7 + 40000, -(-40000 // 7))]
    (seg, lists), = worklists(exe, [(_plan_line(10, 6, 3, [70001, T, 40000]), qs)])
    ids = np.flatnonzero(seg["ch"] == 1)
    (ha, a), (hb, b), (hc, c), (h100, r100), (h96, r96), (h7, r7) = lists
    # (a): a task per segment, each whole, written at its first sample
    assert len(a["T"]) == len(ids) and np.array_equal(a["T"][:, 1], ids) and np.array_equal(a["T"][:, 0], seg["first"][ids])
    assert a["T"][:, 0].max() >= FULL and (a["T"][:, 2] == 0).all() and np.array_equal(a["T"][:, 4], seg["n"][ids]) and len(a["F"]) == 0
    assert (a["T"][:, 5] == 0).all() and np.array_equal(a["T"][:, 6], seg["n"][ids])
    # (b): the two segments around 2^32 in row 0; rows 1 and 2 (channels 0 and 2) are one fill record each
    assert sorted(b["F"].tolist()) == [[40013, 40000], [2 * 40013, 40000]]
    k = FULL // bc.SEG
    # (20000 samples reach back into the first chunk of the segment in front of 2^32: nothing is skipped)
    assert b["T"][:, 1].tolist() == [int(ids[k - 1]), int(ids[k])] and b["T"][:, 0].tolist() == [20000 - bc.SEG, 20000]
    assert b["T"][:, 2].tolist() == [0, 0] and b["T"][:, 5].tolist() == [bc.SEG - 20000, 0] and b["T"][:, 6].tolist() == [bc.SEG, 20000]
    # (c): the last three samples of the last, partial segment
    n_last = T % bc.SEG
    assert c["T"][:, 1].tolist() == [int(ids[-1])] and c["T"][0, 6] - c["T"][0, 5] == 3 and c["T"][0, 2] == (n_last - 1) // bc.CHUNK
    assert c["T"][0, 0] + c["T"][0, 5] == 0 and c["T"][0, 6] == n_last - c["T"][0, 2] * bc.CHUNK
    # re-bin (T: dst seg skip n lo hi ph jfirst jlast head tail): r = 100 has 64 424 551 bins, r = 96 more than 2^26; a bin
    # that two segments share is summed in a side slot and fixed
    for r, (_h, rec) in ((100, (h100, r100)), (96, (h96, r96))):
        R = rec["T"]
        first = seg["first"][ids]
        assert len(R) == len(ids) and np.array_equal(R[:, 0] + R[:, 7], first // r) and np.array_equal(R[:, 6], first % r)
        assert R[-1, 0] + R[-1, 8] == -(-T // r) - 1 and len(rec["F"]) == 0 and len(rec["X"]) == int((first[1:] % r != 0).sum())
    assert -(-T // 100) == 64_424_551 < 1 << 26 <= (r96["T"][:, 0] + r96["T"][:, 8]).max()
    # r = 7 from the multiple of 7 below 2^32 - 20000
    T7 = r7["T"]
    assert T7[:, 1].tolist() == [int(ids[k - 1]), int(ids[k])] and t7 % 7 == 0 and lo - 7 < t7 <= lo
    assert T7[-1, 0] + T7[-1, 8] == -(-40000 // 7) - 1 and len(r7["X"]) == int(FULL % 7 != 0)


def test_rebin3_runs_past_its_grid_cap(exe):  # noqa: F811
    """r = 17, 34, 68: u = 17 dwords, 256 units and 17 408 bytes a tile, so 65535 x 4 tiles are 4 563 333 120 bytes -- and the
    long channel needs 370 086 tiles; r = 2 (k_rebin2, 4096 tiles in x) wraps as well, r = 100 (u = 25) stays below the cap"""
    T = bc.T_LONG
    shapes = [(T, 3, r) for r in (17, 34, 68, 100, 2)]
    got = [_ints(rec, "rebin") for rec in geometry(exe, ["rebin %d %d %d" % s for s in shapes])]
    for s, g in zip(shapes, got):
        assert g == _rebin(*s), s
    for g in got[:3]:
        assert g == [YMAX, 3, g[2], 17, 256, 4] and g[3] * g[4] * 4 == 17408
    assert [g[2] for g in got[:3]] == [4, 2, 1]
    assert YMAX * 4 * 17408 == 4_563_333_120 < T and -(-T // 17408) == 370_086 > 4 * YMAX == 262_140
    # r = 100: 25 dwords a unit, tiles of 25 600 bytes -- 62 915 workgroups in x, below the cap
    assert got[3][:1] + got[3][3:] == [-(-(-(-T // 25600)) // 4), 25, 256, 4] and got[3][0] == 62915 < YMAX
    assert got[4] == [4096, 3] and -(-T // 2) >= 1 << 31 and -(-(-(-T // 2)) // 16384) > 4096
