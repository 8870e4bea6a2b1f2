"""The byte-misaligned scenarios (tests/misaligned.py) without a GPU: every codec scenario lands on its cell's kernel
instance (planner_check --cells with the scenario's window rule and h), the scenarios of a cell reach the address
residues they are for, every measure scenario is in the launch form it claims (planner_check --forms), and the CPU
oracle -- the reference side of tests/test_gpu_misaligned.py -- gives on the misaligned layouts what a few lines of
NumPy say it must, whatever the offsets."""
import subprocess
import zlib

import numpy as np
import pytest

import oracle
from tests import kernel_cells as kc
from tests import misaligned as ma
from tests.test_host_kernel_cells import _line, planned
from tests.test_planner_sanitized import exe  # noqa: F401  (fixture: planner_check built under the sanitizers)

OC = oracle.c
IDS = [c.key.replace("mh::", "").replace(" ", "") for c in ma.CODEC_CELLS]


def test_the_scenarios_cover_the_20_byte_layout_cells():
    assert len(ma.CODEC_CELLS) == 20
    assert sum(c.decoder for c in ma.CODEC_CELLS) == 8 and all(c.input_bits == 8 for c in ma.CODEC_CELLS)
    assert {c.symbol for c in ma.CODEC_CELLS} == {c.symbol for c in kc.ENCODER_CELLS + kc.DECODER_CELLS
                                                  if c.input_bits == 8}
    for form in (ma.WAVE, ma.WG):
        assert {0, 1, 2} == {rule for _w, _sc, _h, rule, _s in form}, "MH_WIN_REF_HALF in every task form"
        assert {0, 1, 2, 3} == {h for _w, _sc, h, _rule, _s in form}
        assert {1, 7, 8, 15} <= {s % 16 for _w, _sc, _h, _rule, s in form}
    assert 0 in ma.GAPS and max(ma.GAPS) >= 113 and sum(0 < g < 16 and g % 2 for g in ma.GAPS) >= 2


def test_layout_builder():
    chans = [np.full(n, 9, np.uint8) for n in (5, 1, 300, 16, 7)]
    data, off, ln = ma.layout(chans, 256 + 7)
    assert off.tolist() == [263, 268, 272, 689, 706] and ln.tolist() == [5, 1, 300, 16, 7]
    assert len(data) == 706 + 7 + ma.GUARD
    mask = np.zeros(len(data), bool)
    for o, n in zip(off, ln):
        assert not mask[int(o):int(o + n)].any()
        mask[int(o):int(o + n)] = True
    assert np.all(data[mask] == 9) and np.array_equal(data[~mask], np.resize(ma.PAD, len(data))[~mask])
    with pytest.raises(AssertionError):
        ma.offsets([5, 5], 255)


def test_every_codec_scenario_lands_on_its_cell(exe):  # noqa: F811
    want = [(c, s) for c in ma.CODEC_CELLS for s in ma.codec_scenarios(c)]
    lines = [_line(s.lens, s.case.S, s.h, s.mode, s.case.rows, s.seg_chunks, 8, window=s.window) for _c, s in want]
    for (c, s), (maxlen, wave, W, picks) in zip(want, planned(exe, lines)):
        tag = (c.symbol, s)
        assert maxlen == s.case.maxlen and wave == int(c.wave) and len(picks) == 4, tag
        if c.decoder:
            assert W == s.case.W and picks[1][0] == c.symbol, tag
        else:
            assert picks[0][0] == c.symbol, tag


@pytest.mark.parametrize("cell", ma.CODEC_CELLS, ids=IDS)
def test_codec_scenarios_reach_the_residues(cell):
    """Window start addresses 1, 8 and 15 mod 16 and one in the last 15 bytes of a 128-byte line (a 16-byte access
    there straddles two lines); an odd end address; a REF_HALF_TRUNC window that ends inside its channel off a 16-byte
    boundary with at least 16 live samples behind it; touching neighbours in every scenario; every case of the cell,
    MH_WIN_AFTER_CAL and MH_WIN_REF_HALF_TRUNC; under MH_WIN_REF_HALF channels that the rule skips, one of them
    touching the end of a coded neighbour, and no skipped channel under any other rule."""
    scen = ma.codec_scenarios(cell)
    starts, ends, cut, skips, skips_touching = [], [], 0, 0, 0
    for s in scen:
        assert 0 <= s.h <= 3 and s.shift >= ma.GUARD
        off = s.offsets()
        if len(s.lens) > 1:
            assert any(int(off[i]) + s.lens[i] == int(off[i + 1]) for i in range(len(s.lens) - 1)), s
        for i, (o, T) in enumerate(zip(off, s.lens)):
            w0, w1, skip = ma.window(T, s.h, s.window)
            assert not skip or (s.window == ma.WIN_REF_HALF and w0 == w1)
            skips += skip
            if skip and i and int(off[i - 1]) + s.lens[i - 1] == int(o):
                before = ma.window(s.lens[i - 1], s.h, s.window)
                skips_touching += before[1] > before[0]
            if w1 > w0:
                assert w0 == 1 << s.h
                starts.append(int(o) + w0)
                ends.append(int(o) + w1)
                cut += s.window == ma.WIN_REF_HALF_TRUNC and (int(o) + w1) % 16 != 0 and T - w1 >= 16
    assert {1, 8, 15} <= {a % 16 for a in starts}, sorted({a % 16 for a in starts})
    assert any(a % 128 >= 113 for a in starts)
    assert any(a % 16 % 2 for a in ends)
    assert cut >= 1
    assert skips >= 2 and skips_touching >= 1
    assert {ma.WIN_AFTER_CAL, ma.WIN_REF_HALF_TRUNC} <= {s.window for s in scen}
    assert {s.case for s in scen} == set(cell.cases)


def _rank_order(S, mode, peak):
    """idx[rank] = symbol: the peak, then its neighbours below and above in turn (APPROX); the identity (NOSORT)"""
    if not mode:
        return np.arange(S)
    both = [peak] + [v for d in range(1, S) for v in (peak - d, peak + d)]
    return np.array([v for v in both if 0 <= v < S])


def _np_measure(x, S, h, mode, rule, sclv):
    w0, w1, skipped = ma.window(len(x), h, rule)
    y = np.minimum(x, S - 1)
    cal, post = np.bincount(y[:w0], minlength=S), np.bincount(y[w0:w1], minlength=S)
    peak = int(np.argmax(cal)) if mode else 0
    idx = _rank_order(S, mode, peak)
    enc = int(np.argmin(sclv.astype(np.int64) @ cal[idx]))
    return w0, cal[idx], peak, enc, post[idx], int(sclv[enc].astype(np.int64) @ post[idx]), skipped


def _same_measure(om, chans, S, h, mode, rule, sclv, tag):
    for c, x in enumerate(chans):
        cut, cal, peak, enc, post, bits, skipped = _np_measure(x, S, h, mode, rule, sclv)
        got = (int(om["cutoff"][c]), om["cal_sorted"][c].tolist(), int(om["peak"][c]), int(om["enc"][c]),
               om["post_mapped"][c].tolist(), int(om["bits"][c]), int(om["skipped"][c]))
        assert got == (cut, cal.tolist(), peak, enc, post.tolist(), bits, skipped), tag + (c,)


@pytest.mark.parametrize("cell", ma.CODEC_CELLS, ids=IDS)
def test_oracle_is_indifferent_to_the_offsets_codec(cell):
    """decode(encode(x)) is min(x, S - 1) on the windows and leaves every other byte as it was; measure is the NumPy
    restatement -- on the misaligned layout, and the stream is the one the 16-byte-padded layout gives"""
    rng = np.random.RandomState(zlib.crc32(cell.key.encode()))
    for s in ma.codec_scenarios(cell):
        S, rows = s.case.S, np.array(s.case.rows, np.uint8)
        chans = ma.codec_channels(rng, s.lens)
        data, off, ln = ma.layout(chans, s.shift)
        p = OC.Params(S, s.h, s.mode, s.window, rows, seg_chunks=s.seg_chunks)
        oe = OC.encode(data, off, ln, p)
        od = OC.decode(oe["payload"], off, ln, p, oe["peak"], oe["enc"], len(data))
        want = np.zeros(len(data), np.uint8)
        for x, o in zip(chans, off):
            w0, w1, _skip = ma.window(len(x), s.h, s.window)
            want[int(o) + w0:int(o) + w1] = np.minimum(x[w0:w1], S - 1)
        assert np.array_equal(od, want), (cell.symbol, s)
        assert oe["skipped"].tolist() == [ma.window(T, s.h, s.window)[2] for T in s.lens], (cell.symbol, s)
        _same_measure(OC.measure(data, off, ln, p), chans, S, s.h, s.mode, s.window, rows, (cell.symbol, s))
        flat, foff, fln = OC.flatten(chans)
        fe = OC.encode(flat, foff, fln, p)
        for k in ("payload", "seg_words", "ch_bits", "peak", "enc", "skipped"):
            assert np.array_equal(oe[k], fe[k]), (cell.symbol, s, k)


MEASURE = ma.measure_scenarios()


def test_measure_scenarios_are_in_the_form_they_claim(exe):  # noqa: F811
    """planner_check --forms: one launch or separate launches, and calibration tiles exactly in the separate form;
    S = 2, 3, 5, 8, 9, 10 x both mappers x MH_WIN_REF_HALF, MH_WIN_AFTER_CAL x both forms"""
    assert len(MEASURE) == 48 and len({m.ident for m in MEASURE}) == 48
    assert {(m.S, m.mode, m.window, m.fused) for m in MEASURE} == {
        (S, mode, w, f) for S in (2, 3, 5, 8, 9, 10) for mode in (0, 1) for w in (ma.WIN_REF_HALF, ma.WIN_AFTER_CAL)
        for f in (False, True)}
    assert {1, 7, 8, 15} <= {m.shift % 16 for m in MEASURE}
    text = "\n".join(_line(m.lens()[0], m.S, m.h, m.mode, ma.MEASURE_ROWS[m.S], 0, 8, window=m.window)
                     for m in MEASURE) + "\n"
    r = subprocess.run([exe, "--forms"], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    forms = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(forms) == len(MEASURE)
    for m, (_wave, fused, _fc, _tickets, cal_tiles, _heads, skipped, shorter) in zip(MEASURE, forms):
        lens = m.lens()[0]
        assert (m.h <= 12) == m.fused and bool(fused) == m.fused, m
        assert cal_tiles == (0 if m.fused else len(lens)), m      # one calibration tile per channel: k_hist2<4>
        assert shorter >= 1 and (skipped >= 1) == (m.window == ma.WIN_REF_HALF), m
    # the tile geometry the scenarios are built on is the planner's: its constants, and its window tiles one by one
    t = subprocess.run([exe, "--tiles"], input=text, capture_output=True, text=True, timeout=600)
    assert t.returncode == 0, t.stderr[-3000:]
    lines = t.stdout.splitlines()
    assert len(lines) == 2 * len(MEASURE)
    for i, m in enumerate(MEASURE):
        tile, cal_direct, n_tiles, n_cal = (int(v) for v in lines[2 * i].split())
        assert tile == ma.TILE and ((1 << m.h) > cal_direct) == (not m.fused), m
        want = []
        for T in m.lens()[0]:
            w0, w1, _skip = ma.window(T, m.h, m.window)
            want += [min(ma.TILE, w1 - w0 - first) for first in range(0, w1 - w0, ma.TILE)] or [0]
        assert [int(v) for v in lines[2 * i + 1].split()] == want and n_tiles == len(want), m
        assert n_cal == (0 if m.fused else len(m.lens()[0])), m


@pytest.mark.parametrize("m", MEASURE, ids=lambda m: m.ident)
def test_measure_scenarios_reach_every_peel(m):
    """Per scenario, by the arithmetic of the kernels (k_hist / k_hist2: head = (16 - address % 16) % 16, cut to the
    tile; vectors; tail): window tiles shorter than their head, head only, head and tail without a vector, one vector
    with and without a tail, odd heads and odd tails, whole tiles and a second tile of one sample; touching channels,
    odd gaps and one of more than a line; in the separate form a calibration tile shorter than its head and odd ones."""
    lens, gaps, kinds = m.lens()
    off = m.offsets()
    assert kinds.count("one") == 2 and 20 <= len(lens) <= 48 and max(lens) <= 320000
    assert 0 in gaps and max(gaps) >= 113 and any(0 < g < 16 and g % 2 for g in gaps)
    assert set(kinds) >= {"head", "tile", "bit", "one", "short", "skip", "full"} - ({"short"} if m.h <= 1 else set())
    seen = set()
    for o, T, kind in zip(off, lens, kinds):
        w0, w1, _skip = ma.window(T, m.h, m.window)
        if kind in ("one", "short", "skip"):
            assert T <= 1 << m.h and w0 == w1 == T
        for first in range(0, w1 - w0, ma.TILE):
            n, H = min(ma.TILE, w1 - w0 - first), ma.head(int(o) + w0 + first)
            hd = min(H, n)
            nvec, tail = (n - hd) // 16, (n - hd) % 16
            if kind == "head":
                assert H >= 2
            seen.add(("short of head", n < H))
            seen.add(("head only", n == H and H > 0))
            seen.add(("head, tail", hd == H and nvec == 0 and tail > 0 and H > 0))
            seen.add(("head, vector", H > 0 and nvec == 1 and tail == 0))
            seen.add(("head, vector, tail", H > 0 and nvec == 1 and tail > 0))
            seen.add(("odd head", hd % 2 == 1))
            seen.add(("odd tail", tail % 2 == 1))
            seen.add(("whole tile", n == ma.TILE))
            seen.add(("tile of one", first > 0 and n == 1 and H > 1))
            seen.add(("more than one trip", nvec > 256 * 4))
        if not m.fused:    # calibration tiles start at the channel's first byte
            n, H = min(T, 1 << m.h), ma.head(int(o))
            seen.add(("cal short of head", n < H))
            seen.add(("cal odd head", min(n, H) % 2 == 1))
            seen.add(("cal odd tail", (n - min(n, H)) % 16 % 2 == 1))
    want = ["short of head", "head only", "head, tail", "head, vector", "head, vector, tail", "odd head", "odd tail",
            "whole tile", "tile of one", "more than one trip"]
    if m.window == ma.WIN_REF_HALF and m.h > 3:   # a REF_HALF window is at least 2^h samples: hundreds of vectors
        want = want[5:]
    if not m.fused:
        want += ["cal odd head", "cal odd tail", "cal short of head"]
    assert not [w for w in want if (w, True) not in seen], m


def test_oracle_is_indifferent_to_the_offsets_measure():
    for m in MEASURE:
        rows = np.array(ma.MEASURE_ROWS[m.S], np.uint8)
        chans = ma.measure_channels(m.h, m.window, m.shift)
        lens, gaps, kinds = m.lens()
        assert tuple(len(x) for x in chans) == lens
        assert all(np.all(x == 255) for x, k in zip(chans, kinds) if k == "full")
        assert any(np.mean(x >= m.S) > 0.05 for x in chans) and max(int(x.max()) for x in chans) == 255
        data, off, ln = ma.layout(chans, m.shift, gaps)
        assert np.array_equal(off, m.offsets())
        om = OC.measure(data, off, ln, OC.Params(m.S, m.h, m.mode, m.window, rows))
        _same_measure(om, chans, m.S, m.h, m.mode, m.window, rows, (m,))
