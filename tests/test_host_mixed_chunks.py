"""The mixed-segment scenarios (tests/mixed_chunks.py) without a GPU: that they are what they claim to be, that the
library's own selection puts them on the kernels they are meant for, that together they reach every (rung, transition)
pair a kernel can reach, and that the host code -- the stream validators and the work lists of the range decoders --
is right on them, so that a failure of tests/test_gpu_mixed_chunks.py can be pinned on a kernel.

  premises    the CPU oracle's stream, walked header by header (mixed_chunks.chunk_words), gives every chunk the size
              its token claims, and with it the route: staged or oversize per decoder rung (payload words + 3 against
              64 * NR, NR read from the cell symbols of tests/kernel_cells.py), fast or slow in an LC >= 2 encoder
              (longest sub-stream against 1024 bits)
  placement   planner_check --cells (the route of tests/test_host_kernel_cells.py) names the intended instance for
              every scenario: byte and 4-bit packed encoder and decoder, k_decode_range, k_decode_rebin
  accounting  the transitions each scenario's segments drive through each instance, computed from the chunk sizes by a
              restatement of the control flow of decode_segment, decode_segment_dual and the encoders; every pair that
              arithmetic does not rule out is there
"""
import numpy as np
import pytest

import muahuff
from muahuff import container_io as cio
from tests import kernel_cells as kc
from tests import mixed_chunks as mc
from tests import standins
from tests.test_host_kernel_cells import _line, planned
from tests.test_host_worklist import _execute_range, _execute_rebin, _run
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

CH = mc.CHUNK
RS = (1, 7, 50, 4096)


def _args(symbol):
    return [a.strip() for a in symbol[:-1].split("<")[1].split(",")]


def _nr(symbol):
    """NR of a decoder instance: the third template argument"""
    return int(_args(symbol)[2])


def _dual(symbol):
    return "k_decode2w<" in symbol and _args(symbol)[5] == "true"


def _lc(symbol):
    return int(_args(symbol)[0])


def _cell(cells, scn, input_bits, decoder):
    """the cell of tests/kernel_cells.py a scenario is meant for: task form, input / output width, and the code -- the
    encoders by the row itself, the decoders by its longest codeword (a cell's cases span the lengths it serves)"""
    hit = []
    for c in cells:
        if c.wave != scn.wave or c.input_bits != input_bits:
            continue
        lens = [k.maxlen for k in c.cases]
        if decoder and min(lens) <= scn.maxlen <= max(lens):
            hit.append(c)
        if not decoder and any(k.rows == (scn.row,) for k in c.cases):
            hit.append(c)
    assert len(hit) == 1, (scn.name, input_bits, decoder, [c.symbol for c in hit])
    return hit[0]


def intended(scn):
    """{role: symbol} from the cell table"""
    return dict(enc=_cell(kc.ENCODER_CELLS, scn, 8, False).symbol, dec=_cell(kc.DECODER_CELLS, scn, 8, True).symbol,
                enc4=_cell(kc.ENCODER_CELLS, scn, 4, False).symbol, dec4=_cell(kc.PACKED_DECODER_CELLS, scn, 4, True).symbol)


@pytest.fixture(scope="module")
def picks(exe):  # noqa: F811
    """the library's selection for every scenario, byte and 4-bit packed plans, once for the module"""
    rows = {s.name: (s.row,) for s in mc.SCENARIOS}
    lines = [_line(s.lens(), s.S, 0, 0, rows[s.name], s.sc, bits) for s in mc.SCENARIOS for bits in (8, 4)]
    got = planned(exe, lines)
    out = {}
    for i, s in enumerate(mc.SCENARIOS):
        (ml, wave, _W, p8), (ml4, wave4, _W4, p4) = got[2 * i], got[2 * i + 1]
        assert ml == ml4 == s.maxlen and wave == wave4, s.name
        assert len(p8) == 4 and len(p4) == 2, s.name
        out[s.name] = dict(wave=bool(wave), enc=p8[0][0], dec=p8[1][0], range=p8[2][0], rebin=p8[3][0], enc4=p4[0][0],
                           dec4=p4[1][0])
    return out


def test_scenario_table_is_well_formed_and_small():
    assert len({s.name for s in mc.SCENARIOS}) == len(mc.SCENARIOS)
    assert {s.sc for s in mc.SCENARIOS if s.row_key == "10_9"} == {2, 3, 4}
    for s in mc.SCENARIOS:
        mc.check_shape(s)
        assert sum(s.lens()) < 2_100_000, s.name
        nseg = [len(c) for c in s.channels]
        if s.wave:
            assert max(nseg) <= 4, s.name
        else:     # multiples of 4; the one-chunk channel is the exception the planner's rule has room for
            assert all(n % 4 == 0 or c == (mc.SINGLE,) for n, c in zip(nseg, s.channels)), s.name
    # the two layouts of a (row, seg_chunks) hold the same segments
    for a in mc.WG_SCENARIOS:
        b, = [s for s in mc.WAVE_SCENARIOS if (s.row_key, s.sc) == (a.row_key, a.sc)]
        assert {seg for c in a.channels for seg in c} == {seg for c in b.channels for seg in c}, a.name


def test_required_segments_are_in_the_table():
    segs = {(s.row_key, seg) for s in mc.SCENARIOS for c in s.channels for seg in c}
    for seg in ("Q L", "L Q", "Q L Q Q", "L Q L L", "Q Q Q L", "s L", "L s", "s s+ s", "M M", "Q M", "M Q M"):
        assert ("10_9", seg) in segs, seg
    for b in ("b31", "b36"):
        for side in "-+":
            assert ("10_9", "%s%s Q" % (b, side)) in segs and ("10_9", "Q %s%s" % (b, side)) in segs, (b, side)
    for side in "-+":
        assert ("10_4", "b32%s Q" % side) in segs and ("10_4", "Q b32%s" % side) in segs, side
    for key in ("10_9", "10_4", "6_5", "9_8"):
        # an oversize, a staged and a short quiet partial chunk behind a quiet and behind a loud chunk
        for first in "QL":
            assert (key, first + " l") in segs and (key, first + " m") in segs, (key, first)
            assert any(k == key and seg.split()[-2:-1] == [first] and seg.split()[-1] in ("q100", "q15")
                       for k, seg in segs), (key, first)
    for s in mc.SCENARIOS:       # one channel that is a single partial oversize chunk, in both task forms
        if s.sc == 2:
            assert (mc.SINGLE,) in s.channels, s.name
    assert ("6_5", "Q L") in segs and ("10_4", "Q L") in segs


@pytest.mark.parametrize("scn", mc.SCENARIOS, ids=lambda s: s.name)
def test_premises_every_chunk_is_what_its_token_claims(scn, picks):
    """chunk sizes from the oracle's stream; for every rung the scenario runs on (byte / packed decoder, range, re-bin)
    the token's side of `nw + 3 <= 64 * NR`, for the dual rung the pair sums, for the encoder the side of 1024 bits"""
    ref = mc.reference(scn.name)
    kl = mc.CLASSES[scn.row_key]
    seg = ref.enc["seg"]
    toks = [s.split() for c in scn.channels for s in c]
    assert len(toks) == len(ref.chunks) == len(seg["ch"])
    assert not ref.enc["peak"].any() and not ref.enc["enc"].any() and not ref.enc["skipped"].any()
    pk = picks[scn.name]
    want = intended(scn)
    # NR of the codec kernels from the cell table; the range kernels have no cells: from the selection
    nrs = {_nr(want["dec"]), _nr(want["dec4"]), _nr(pk["range"]), _nr(pk["rebin"])}
    # which tokens the scenario's rungs must find oversize: stated here, not derived from the stream
    oversize = {31: {"L", "l", "b31+", "b36-", "b36+"}, 36: {"L", "l", "b36+"}, 32: {"L", "l", "b32+"}}
    slow = {"L", "l", "s+", "b36-", "b36+"} if scn.maxlen >= 5 else set()
    for s, (tk, cw) in enumerate(zip(toks, ref.chunks)):
        assert len(tk) == len(cw) == (int(seg["n"][s]) + CH - 1) // CH, (scn.name, s)
        assert int(seg["n"][s]) == sum(kl[t].n for t in tk), (scn.name, s)
        for t, (hw, nw, longest) in zip(tk, cw):
            k = kl[t]
            assert k.nw[0] <= nw <= k.nw[1], (scn.name, s, t, nw)
            assert 1 <= hw <= 25
            if k.longest >= 0:
                assert longest == k.longest, (scn.name, s, t, longest)
            for NR in nrs:
                assert (nw + 3 > 64 * NR) == (t in oversize[NR]), (scn.name, s, t, nw, NR)
            assert (longest > mc.ENC_STAGE_BITS) == (t in slow), (scn.name, s, t, longest)
        if _dual(want["dec"]):     # the pair sums the dual rung tests: payload A + chunk B + 3 words of read-ahead
            cap = 64 * _nr(want["dec"])
            for j in range(0, int(seg["n"][s]) // CH - 1, 2):
                total = cw[j][1] + cw[j + 1][0] + cw[j + 1][1] + 3
                pair = tuple(tk[j:j + 2])
                fits = pair in (("Q", "Q"), ("Q", "M"), ("M", "Q"), ("s", "s+"), ("s+", "s"), ("Q", "s"), ("s", "Q"),
                                ("s+", "Q"))
                assert (total <= cap) == fits, (scn.name, s, pair, total)
                if pair == ("M", "M"):
                    assert cw[j][1] + 3 <= cap and cw[j + 1][1] + 3 <= cap < total


def test_the_class_table_of_the_long_code_row_in_numbers():
    """the word counts the scenario table is built on, as the oracle's stream has them"""
    ref = mc.reference("10_9-sc2-wg")
    toks = [s.split() for c in ref.scn.channels for s in c]
    seen = {}
    for tk, cw in zip(toks, ref.chunks):
        for t, (hw, nw, longest) in zip(tk, cw):
            seen.setdefault(t, set()).add((nw, longest if t in ("s", "s+", "M", "L") else None))
    assert seen["M"] == {(1280, 640)} and seen["L"] == {(4608, 2304)}
    assert seen["s"] == {(536, 1024)} and seen["s+"] == {(537, 1025)}
    assert seen["b31-"] == {(1981, None)} and seen["b31+"] == {(1982, None)}
    assert seen["b36-"] == {(2301, None)} and seen["b36+"] == {(2302, None)}
    assert seen["l"] == {(2532, None)} and seen["m"] == {(1407, None)}
    assert 1981 + 3 == 64 * 31 and 2301 + 3 == 64 * 36 and 2045 + 3 == 64 * 32
    q = [cw[0] for tk, cws in zip(toks, ref.chunks) for t, cw in zip(tk, cws) if t == "Q"]
    assert set(q) == {11}           # a quiet chunk's header: 11 words


def test_placement_every_scenario_lands_on_the_intended_instances(picks):
    for s in mc.SCENARIOS:
        want, got = intended(s), picks[s.name]
        assert got["wave"] == s.wave, s.name
        for role in ("enc", "dec", "enc4", "dec4"):
            assert got[role] == want[role], (s.name, role, got[role], want[role])
        # the range kernels are workgroup-form kernels on the plan's own table width: the byte decoder's rung, but the
        # hybrid pair table (NR = 31) where that is the wave-only one-symbol rung (csrc/mh_select.hpp, dec_pick)
        rung = ["2", "2", "31", "2", "true"] if _dual(want["dec"]) else _args(want["dec"])[:5]
        for role, head in (("range", "mh::k_decode_range<"), ("rebin", "mh::k_decode_rebin<")):
            assert got[role].startswith(head), (s.name, got[role])
            assert _args(got[role])[:5] == rung, (s.name, role, got[role], rung)
    # rungs the scenario sets run on
    assert {(_nr(picks[s.name]["dec"]), s.wave) for s in mc.SCENARIOS} == {(31, False), (32, False), (32, True), (36, True)}
    assert {_lc(picks[s.name]["enc"]) for s in mc.SCENARIOS} == {1, 2, 3}


def _worst_fits(maxlen, NR):
    """a full chunk of the longest code of the rung's plans still stages: no route but the pipeline"""
    return CH * maxlen // 32 + 3 <= 64 * NR


def _accounting(picks):
    dec, enc = {}, {}
    for s in mc.SCENARIOS:
        ref = mc.reference(s.name)
        pk = picks[s.name]
        for n, cw in zip(ref.enc["seg"]["n"], ref.chunks):
            for role in ("dec", "dec4", "range", "rebin"):
                sym = pk[role]
                dec.setdefault(sym, set()).update(mc.decoder_transitions(cw, int(n), _nr(sym), _dual(sym)))
            for role in ("enc", "enc4"):
                enc.setdefault(pk[role], set()).update(mc.encoder_transitions(cw) if _lc(pk[role]) >= 2 else set())
    return dec, enc


def test_accounting_every_reachable_rung_and_transition_is_driven(picks):
    dec, enc = _accounting(picks)
    left_out = 0
    # decoders: every shipped byte / packed-output instance, and the range and re-bin instances of the same rungs
    for cell in kc.DECODER_CELLS + kc.PACKED_DECODER_CELLS:
        NR = _nr(cell.symbol)
        maxlen = max(k.maxlen for k in cell.cases)
        if _worst_fits(maxlen, NR):         # NR = 17 with maxlen <= 2, NR = 25 with maxlen 3
            assert (NR, maxlen) in ((17, 2), (25, 3)), cell.symbol
            assert cell.symbol not in dec or not dec[cell.symbol], cell.symbol
            continue
        if cell.input_bits == 2:
            continue                        # 2-bit pieces: S <= 4, maxlen <= 3 (ruled out above)
        want = set(mc.DEC_TRANSITIONS) | ({mc.PAIR_TRANSITION} if _dual(cell.symbol) else set())
        missing = want - dec.get(cell.symbol, set())
        left_out += len(missing)
        assert not missing, (cell.symbol, sorted(missing))
    for role in ("range", "rebin"):
        syms = {picks[s.name][role] for s in mc.SCENARIOS}
        assert {_nr(x) for x in syms} == {31, 32}, syms
        for sym in syms:
            missing = set(mc.DEC_TRANSITIONS) - dec[sym]
            left_out += len(missing)
            assert not missing, (sym, sorted(missing))
    # encoders: code class LC >= 2 can overflow its staging (LC <= 1: 8 * maxlen dwords hold a chunk's worst case):
    # every such instance, byte input and 4-bit pieces, both task forms
    for cell in kc.ENCODER_CELLS:
        if cell.input_bits == 2:
            continue                        # S <= 4: maxlen <= 3, LC <= 1
        lc = _lc(cell.symbol)
        if lc <= 1:
            # 256 codewords per sub-stream against its staging: 16 dwords for maxlen <= 2, else 32 (enc_stage_dw)
            assert all(256 * k.maxlen <= 32 * (16 if k.maxlen <= 2 else 32) for k in cell.cases), cell.symbol
            assert not enc.get(cell.symbol), cell.symbol
            continue
        missing = set(mc.ENC_TRANSITIONS) - enc.get(cell.symbol, set())
        left_out += len(missing)
        assert not missing, (cell.symbol, sorted(missing))
    assert sum(_lc(c.symbol) >= 2 for c in kc.ENCODER_CELLS) == 10
    assert left_out == 0


def _dense(ref):
    e = ref.enc
    return standins.dense_words(e["payload"], e["seg"]["off"], e["seg_words"])


@pytest.mark.parametrize("scn", mc.SCENARIOS, ids=lambda s: s.name)
def test_validators_accept_every_dense_scenario_stream(scn):
    ref = mc.reference(scn.name)
    e = ref.enc
    dense = np.ascontiguousarray(_dense(ref))
    sw = np.ascontiguousarray(e["seg_words"], np.uint64)
    ln = np.ascontiguousarray(ref.ln, np.uint64)
    L = muahuff._lib.lib()
    head = (ln.ctypes.data, len(ln), scn.S, 0, 0, muahuff.WIN_FULL, ref.rows.ctypes.data, 1, scn.sc)
    rc = L.mh_validate_stream(*head, dense.ctypes.data, dense.size, sw.ctypes.data, sw.size, e["peak"].ctypes.data,
                              e["enc"].ctypes.data)
    assert rc == 0, L.mh_last_error()
    off = np.concatenate([[0], np.cumsum(sw)[:-1]]).astype(np.uint64)
    idx = np.arange(sw.size, dtype=np.uint64)
    rc = L.mh_validate_segments(*head, dense.ctypes.data, dense.size, off.ctypes.data, sw.ctypes.data, sw.size,
                                idx.ctypes.data, idx.size, e["peak"].ctypes.data, e["enc"].ctypes.data)
    assert rc == 0, L.mh_last_error()
    # and in the slotted layout the encoders write, every other segment
    slots = np.ascontiguousarray(e["seg"]["off"], np.uint64)
    pay = np.ascontiguousarray(e["payload"])
    rc = L.mh_validate_segments(*head, pay.ctypes.data, pay.size, slots.ctypes.data, sw.ctypes.data, sw.size,
                                idx[::2].copy().ctypes.data, idx[::2].size, e["peak"].ctypes.data, e["enc"].ctypes.data)
    assert rc == 0, L.mh_last_error()


WORKLIST_SCENARIO = "10_9-sc3-wg"


def test_work_lists_of_the_gpu_tests_ranges_execute_to_the_oracles_slices(exe):  # noqa: F811
    """the ranges tests/test_gpu_mixed_chunks.py asks for, on one scenario: each work list, executed in NumPy on the
    oracle's decode, gives the slice and its bin sums"""
    ref = mc.reference(WORKLIST_SCENARIO)
    scn = ref.scn
    lens = scn.lens()
    case = "%d %d 0 0 3 1 %d  %s  %s" % (len(lens), scn.S, scn.sc, " ".join(map(str, lens)), " ".join(map(str, scn.row)))
    qs, info = [], []
    for i, (c, a, b) in enumerate(mc.query_ranges(scn)):
        for r in (0,) + RS:
            t0 = a - a % r if r else a
            row = (b - t0 + r - 1) // r if r else b - t0
            pitch = row + 13 if i % 2 else row
            qs.append("1 %d %d %d %d %d" % (c, t0, b, r, pitch))
            info.append(([c], t0, b, r, pitch))
    (seg, lists), = _run(exe, [(case, qs)])
    assert np.array_equal(seg["n"], ref.enc["seg"]["n"].astype(np.int64))
    w0, w1 = cio.window_bounds(lens, 0, 3)
    assert not w0.any() and np.array_equal(w1, lens)
    for (head, rec), (sel, t0, t1, r, pitch) in zip(lists, info):
        if r == 0:
            _execute_range(head, rec, seg, ref.full, w0, w1, sel, t0, t1, pitch)
        else:
            assert _execute_rebin(head, rec, seg, ref.full, w0, w1, sel, t0, t1, r, pitch) <= 2
