"""Fused decode + re-bin on the GPU (mh_decode_rebin, codec.Plan.decode_rebin, container_io.decompress_binned,
api.decompress with bin=): every row equals the CPU oracle's decode of the whole channel, sliced, zero-extended and
re-binned by the oracle (rebin_u8 / rebin_u32) -- exactly, for every bin factor of the list, both output forms, every
window rule, both format revisions, every decoder rung, ranges cut on every kind of boundary; nothing outside the rows
is written; corrupt input is flagged or rejected; full size matches mh_decode + a torch reshape-sum."""
import numpy as np
import pytest

import muahuff
from muahuff import container_io as cio
from tests import helpers, kernel_cells as kc, standins

pytestmark = pytest.mark.gpu
CH = muahuff.CHUNK
RS = (1, 2, 3, 5, 7, 10, 16, 20, 50, 100, 128, 1000, 4096)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    return torch


def _container(lens, S, h, window, sc, rev=3, seed=0, tab=None, rate=0.9):
    """oracle.c.encode -> dense container (as _oracle_container of tests/test_host_range_decode.py, with the SCLV rows
    and the Poisson rate as arguments) and the oracle's decode of it, per channel"""
    import oracle
    OC = oracle.c
    rng = np.random.RandomState(seed)
    tab = helpers.sclv_tables()[S] if tab is None else tab
    chans = [np.minimum(rng.poisson(rate, size=T), 255).astype(np.uint8) for T in lens]
    data, off, ln = OC.flatten(chans)
    p = OC.Params(S, h, 1, window | (OC.WIN_REV2_SEGMENTS if rev == 2 else 0), tab, seg_chunks=sc)
    e = OC.encode(data, off, ln, p)
    dense = standins.dense_words(e["payload"], e["seg"]["off"], e["seg_words"])
    hdr = cio.make_header(S, h, 1, window, sc, tab)
    hdr["format_revision"] = rev
    C = len(lens)
    c = cio.Compressed(hdr, np.array(lens, np.uint64), e["peak"].astype(np.uint8), e["enc"].astype(np.uint8),
                       np.zeros(C, np.uint8), np.zeros(C, np.uint64), e["seg_words"].astype(np.uint64), dense)
    full = OC.decode(e["payload"], off, ln, p, e["peak"], e["enc"], len(data))
    return c, [full[int(o):int(o) + int(n)] for o, n in zip(off, ln)]


def _want(full, sel, start, stop, r, saturate):
    """the oracle's expectation: decoded channel, sliced and zero-extended to [start, stop), re-binned by the oracle"""
    import oracle
    nb = (stop - start + r - 1) // r
    rows = np.zeros((len(sel), nb), np.uint8 if saturate else np.uint32)
    for i, ch in enumerate(sel):
        y = np.zeros(stop - start, np.uint8)
        x = full[ch][start:stop]
        y[:len(x)] = x
        if nb:
            rows[i] = oracle.c.rebin_u8(y, r) if saturate else oracle.c.rebin_u32(y, r)
    return rows


def _got(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint32)


# shorter than the calibration window (h = 6: 64) / than r; last chunks of 1..3 samples; >= 16 chunks (head segment)
LENS = [16 * CH + 1000, 50000, 20 * CH + 3, 5, 70001, CH + 1, 3 * CH + 2, 300000, 40, 17 * CH]
CASES = [(S, h, window, rev) for S in (5, 7) for window in (0, 1, 2, 3) for rev in (2, 3) for h in (2, 6)]


@pytest.mark.parametrize("S,h,window,rev", CASES)
def test_binned_rows_equal_the_oracle(gpu, S, h, window, rev):
    sc = 1 + (S + window + rev + h // 6) % 2
    c, full = _container(LENS, S, h, window, sc, rev, seed=S * 7 + window)
    T, C = max(LENS), len(LENS)
    sat_seen = False
    for r in RS:
        for saturate in (True, False):
            got = _got(cio.decompress_binned(c, r, saturate=saturate))
            want = _want(full, range(C), 0, T, r, saturate)
            assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (S, h, window, rev, r, saturate)
            if r >= 1000:
                if saturate:
                    sat_seen |= bool((want == 255).any())
                else:
                    assert want.max() > 255
        if r == 1:
            assert np.array_equal(got, cio.decompress_range(c, 0, T).cpu().numpy())
    assert sat_seen


def test_a_skipped_ref_half_channel_bins_to_zero(gpu):
    """WIN_REF_HALF skips a channel whose window would be empty or whose calibration fails: its row is all zero"""
    lens = [3 * CH, 70, 2 * CH + 9]
    c, full = _container(lens, 5, 6, 0, 1, seed=4)
    for r in (5, 50):
        got = _got(cio.decompress_binned(c, r, saturate=False))
        assert np.array_equal(got, _want(full, range(3), 0, max(lens), r, False))
    assert not full[1].any()


def _ranges(lens, h, window, sc, rng):
    w0, w1 = cio.window_bounds(lens, h, window)
    T = max(lens)
    r = [(0, 0), (7, 7), (0, 1), (T - 1, T), (0, T), (3, 13), (5, 37), (1000, 3100), (CH - 5, CH + 21),
         (2 * CH - 1, 2 * CH + 1), (sc * CH - 100, sc * CH + 100), (1, 2 * sc * CH + 777)]
    for c in range(len(lens)):
        a = int(w0[c])
        r += [(max(a - 3, 0), min(a + 50, T)), (a + 1024 - 2, min(a + 1024 + 3, T)), (max(int(w1[c]) - 9, 0), T),
              (min(lens[c] - 5, T), T)]
    for _ in range(6):
        a, b = sorted(int(x) for x in rng.randint(0, T + 1, size=2))
        r.append((a, b))
    return [(a, b) for a, b in r if 0 <= a <= b <= T]


@pytest.mark.parametrize("S,h,window,rev", [(3, 6, 2, 3), (5, 2, 0, 2), (7, 6, 1, 3), (10, 3, 3, 2), (4, 6, 2, 2)])
def test_ranges_cut_on_every_boundary(gpu, S, h, window, rev):
    sc = 1 + (S + window) % 2
    c, full = _container(LENS, S, h, window, sc, rev, seed=S + window)
    rng = np.random.RandomState(S + 10 * window + rev)
    C = len(LENS)
    sels = [None, [2, 0, 7], list(range(C))[::-1], [4, 4, 1, 4]]
    for k, (a, b) in enumerate(_ranges(LENS, h, window, sc, rng)):
        sel = sels[k % len(sels)]
        r = RS[k % len(RS)]
        a -= a % r
        saturate = bool(k & 1)
        got = _got(cio.decompress_binned(c, r, a, b, channels=sel, saturate=saturate))
        want = _want(full, list(range(C)) if sel is None else sel, a, b, r, saturate)
        assert got.shape == want.shape and np.array_equal(got, want), (S, h, window, rev, a, b, r, sel)


def _ident(cell):
    return cell.key


@pytest.mark.parametrize("cell", kc.DECODER_CELLS, ids=_ident)
def test_every_decoder_rung(gpu, cell):
    """one case per decoder cell: its SCLV rows and layouts (whole-channel windows) decide the rung mh_decode_rebin takes"""
    for j, case in enumerate(cell.cases):
        lens, sc = cell.layouts[j % len(cell.layouts)]
        lens = [int(x) for x in lens]
        c, full = _container(lens, case.S, 0, 3, sc, 3, seed=j + case.S, tab=np.array(case.rows, np.uint8), rate=1.2)
        T = max(lens)
        for r, saturate in ((7, True), (50, False), (1000, True)):
            got = _got(cio.decompress_binned(c, r, saturate=saturate))
            assert np.array_equal(got, _want(full, range(len(lens)), 0, T, r, saturate)), (cell.key, case.S, r)
        a, b = (T // 3) - (T // 3) % 20, T - 1
        got = _got(cio.decompress_binned(c, 20, a, b, saturate=False))
        assert np.array_equal(got, _want(full, range(len(lens)), a, b, 20, False)), (cell.key, case.S)


def test_every_S_is_covered():
    """the decoder cells' cases and the parametrised cases above together run S = 2..10"""
    cells = {case.S for cell in kc.DECODER_CELLS for case in cell.cases}
    assert cells | {S for S, *_ in CASES} >= set(range(2, 11))


def _plan_and_stream(torch, c):
    from muahuff import codec
    hd = c.header
    plan = codec.Plan(np.zeros(len(c.ch_len), np.uint64), c.ch_len, hd["S"], hd["h"], hd["mode"], cio.plan_window(hd),
                      np.array(hd["sclv"], np.uint8), seg_chunks=hd["seg_chunks"])
    pay = torch.zeros(c.payload.size + 4, dtype=torch.int32, device="cuda")
    pay[:c.payload.size] = torch.from_numpy(c.payload.view(np.int32)).cuda()
    dense_off = np.concatenate([[0], np.cumsum(c.seg_words)[:-1]]).astype(np.int64)
    return plan, pay, torch.from_numpy(dense_off).cuda(), torch.from_numpy(c.peak.copy()).cuda(), torch.from_numpy(c.enc.copy()).cuda()


def test_guards_pitch_determinism_and_list_reuse(gpu):
    torch = gpu
    c, full = _container(LENS, 5, 6, 2, 2, 3, seed=1)
    plan, pay, seg_off, peak, enc = _plan_and_stream(torch, c)
    for (a, b, r, lead) in ((CH - 34, 3 * CH + 5, 50, 7), (0, max(LENS), 100, 0), (65, 65 + 16, 5, 13), (300, 299 + 2 * CH, 3, 1)):
        sel = [6, 0, 2, 2, 7]
        nb = (b - a + r - 1) // r
        for saturate in (True, False):
            dt = torch.uint8 if saturate else torch.int32
            canary = 0xA5 if saturate else 0x5A5A5A5A
            outs = []
            for _ in range(2):
                buf = torch.full((len(sel) + 2, nb + lead + 45), canary, dtype=dt, device="cuda")
                view = buf[1:-1, lead:lead + nb]
                out = plan.decode_rebin(pay, seg_off, peak, enc, sel, a, b, r, saturate, out=view)
                assert plan.decode_ok() and out.data_ptr() == view.data_ptr()
                host = buf.cpu().numpy()
                assert (host[1:-1, :lead] == canary).all() and (host[1:-1, lead + nb:] == canary).all(), (a, b, r)
                assert (host[0] == canary).all() and (host[-1] == canary).all()
                outs.append(_got(out))
            assert np.array_equal(outs[0], outs[1])
            assert np.array_equal(outs[0], _want(full, sel, a, b, r, saturate)), (a, b, r, saturate)
    # a repeated query reuses the plan's work list (same selection values in another array): same answer
    sel = np.array([1, 4], np.int64)
    one = _got(plan.decode_rebin(pay, seg_off, peak, enc, sel, 0, 50000, 50)).copy()
    two = _got(plan.decode_rebin(pay, seg_off, peak, enc, sel.copy(), 0, 50000, 50))
    assert np.array_equal(one, two) and np.array_equal(one, _want(full, [1, 4], 0, 50000, 50, True))
    # argument errors of the binding and of the C call
    with pytest.raises(ValueError):
        plan.decode_rebin(pay, seg_off, peak, enc, [0], 5, 4, 5)
    with pytest.raises(ValueError):
        plan.decode_rebin(pay, seg_off, peak, enc, [0], 7, 70, 5)
    with pytest.raises(IndexError):
        plan.decode_rebin(pay, seg_off, peak, enc, [len(LENS)], 0, 4, 2)
    L = muahuff._lib.lib()
    s32 = np.array([0, 1], np.uint32)
    o = torch.zeros(64, dtype=torch.uint8, device="cuda")
    from muahuff.codec import _ptr
    for (t0, t1, r, pitch) in ((0, 100, 0, 100), (0, 100, 4097, 100), (3, 100, 5, 100), (10, 5, 5, 100),
                               (0, max(LENS) + 1, 5, 1 << 30), (0, 100, 5, 19)):
        rc = L.mh_decode_rebin(plan._h, _ptr(pay), pay.numel(), _ptr(seg_off), s32.ctypes.data, 2, t0, t1, r, 1, _ptr(peak),
                               _ptr(enc), _ptr(o), pitch, None)
        assert rc == muahuff._lib.ERR_ARG and L.mh_last_error(), (t0, t1, r, pitch)
    s32[1] = len(LENS)
    assert L.mh_decode_rebin(plan._h, _ptr(pay), pay.numel(), _ptr(seg_off), s32.ctypes.data, 2, 0, 100, 5, 1, _ptr(peak),
                             _ptr(enc), _ptr(o), 20, None) == muahuff._lib.ERR_ARG
    plan.close()


def test_range_and_rebin_lists_of_one_plan_do_not_disturb_each_other(gpu):
    """mh_decode_range and mh_decode_rebin keep a work list each in the plan, in caches of one type: interleaved calls
    -- the same query under both, a list reused after the other call rebuilt its own -- all give the oracle's answer"""
    torch = gpu
    c, full = _container(LENS, 5, 6, 2, 2, 3, seed=2)
    plan, pay, seg_off, peak, enc = _plan_and_stream(torch, c)
    q1 = ([6, 0, 2, 2, 7], CH - 34, 3 * CH + 5)
    q2 = ([4, 1], 7 * 900, 5 * CH + 11)
    for sel, a, b, r in (q1 + (0,), q1 + (50,), q1 + (0,), q2 + (7,), q1 + (0,), q1 + (50,)):
        if r:
            got = _got(plan.decode_rebin(pay, seg_off, peak, enc, sel, a, b, r, saturate=False))
            want = _want(full, sel, a, b, r, False)
        else:
            got = _got(plan.decode_range(pay, seg_off, peak, enc, sel, a, b))
            want = _want(full, sel, a, b, 1, True)     # bins of one sample: the slice itself
        assert plan.decode_ok()
        assert got.shape == want.shape and np.array_equal(got, want), (sel, a, b, r)
    plan.close()


def test_packed_plan_is_refused(gpu):
    torch = gpu
    from muahuff import MODE_APPROX, WIN_FULL, codec, sclv
    lens = np.array([3 * CH, 2 * CH], np.uint64)
    plan = codec.Plan(np.array([0, 3 * CH // 4], np.uint64), lens, 3, 0, MODE_APPROX, WIN_FULL, sclv.table(3),
                      input_bits=2)
    z = torch.zeros(16, dtype=torch.int32, device="cuda")
    o = torch.zeros(8, dtype=torch.int64, device="cuda")
    b = torch.zeros(8, dtype=torch.uint8, device="cuda")
    with pytest.raises(muahuff.MuaHuffError) as e:
        plan.decode_rebin(z, o, b, b, [0], 0, 4, 2)
    assert e.value.code == muahuff._lib.ERR_ARG
    plan.close()


def test_untrusted_input_is_flagged_or_rejected(gpu):
    """malformed INPUTS to a memory-safe decoder: truncated, all-ones-sprinkled, all-zero-header and wild-offset streams"""
    torch = gpu
    c, full = _container(LENS, 5, 6, 2, 2, 3, seed=3)
    a, b, sel, r = CH - 34, 5 * CH + 100, [0, 2, 7], 50
    pay, seg_off, segs = cio.gather_range(c, a, b, np.array(sel))
    bad = c.payload.copy()
    dense_off = np.concatenate([[0], np.cumsum(c.seg_words)[:-1]]).astype(np.int64)
    for s in segs:
        bad[int(dense_off[int(s)])] ^= 0xFFF
    cb = cio.Compressed(c.header, c.ch_len, c.peak, c.enc, c.skipped, c.ch_bits, c.seg_words, bad)
    with pytest.raises(ValueError):
        cio.decompress_binned(cb, r, a, b, channels=sel)
    plan, _, _, peak, enc = _plan_and_stream(torch, c)
    nb = (b - a + r - 1) // r
    wild = seg_off.copy()
    wild[[int(s) for s in segs]] = np.uint64(1) << np.uint64(62)
    streams = [(pay[:len(pay) // 3], seg_off, True),
               (np.where(np.arange(len(pay)) % 97 == 0, np.uint32(0xFFFFFFFF), pay).astype(np.uint32), seg_off, False),
               (np.zeros_like(pay), seg_off, True),
               (pay, wild, True)]
    for payload, off, must_flag in streams:
        d_pay = torch.from_numpy(payload.view(np.int32).copy()).cuda()
        for saturate in (True, False):
            canary = 0xA5 if saturate else 0x5A5A5A5A
            buf = torch.full((len(sel) + 2, nb + 64), canary, dtype=torch.uint8 if saturate else torch.int32, device="cuda")
            plan.decode_rebin(d_pay, torch.from_numpy(off.view(np.int64)).cuda(), peak, enc, sel, a, b, r, saturate,
                              out=buf[1:-1, 32:32 + nb])
            flagged = not plan.decode_ok()
            host = buf.cpu().numpy()
            assert (host[1:-1, :32] == canary).all() and (host[1:-1, 32 + nb:] == canary).all()
            assert (host[0] == canary).all() and (host[-1] == canary).all()
            assert flagged or not must_flag
    plan.close()


def test_files_and_the_api(gpu, tmp_path):
    lens = [16 * CH + 1000, 50000, 20 * CH + 3]
    c, full = _container(lens, 3, 6, 2, 2, 3, seed=9, rate=1.1)
    fn = str(tmp_path / "a.muahuff")
    cio.save(fn, c)
    import oracle
    got = muahuff.decompress(fn, bin=50)
    assert len(got) == 3
    for g, x in zip(got, full):
        assert g.dtype == np.uint8 and np.array_equal(g, oracle.c.rebin_u8(x, 50))
    got = muahuff.decompress(c, channels=[2, 0], bin=7)
    assert all(np.array_equal(g, oracle.c.rebin_u8(full[ch], 7)) for g, ch in zip(got, (2, 0)))
    for (a, b, sel) in ((CH + 16, CH + 16 + 16384, [2, 0]), (40000, 60001, [1, 1]), (0, max(lens), None)):
        sel_ = list(range(3)) if sel is None else sel
        api = muahuff.decompress(fn, channels=sel, start=a, stop=b, bin=50)
        want = _want(full, sel_, a, b, 50, True)
        assert len(api) == len(sel_) and all(np.array_equal(x, y) for x, y in zip(api, want)), (a, b)
        with cio.open(fn) as f:
            cio.decompress_range(f, a, b, channels=sel)
            plain = f.bytes_read
        with cio.open(fn) as f:
            g = _got(cio.decompress_binned(f, 50, a, b, channels=sel, saturate=False))
            assert f.bytes_read <= plain
        assert np.array_equal(g, _want(full, sel_, a, b, 50, False))


def test_full_size_equals_decode_plus_reshape_sum(gpu):
    """1024 x 1e7, S = 3, r = 50, both forms, against mh_decode (pinned at this size by test_gpu_fullsize) + torch's sum"""
    torch = gpu
    from muahuff import MODE_APPROX, WIN_AFTER_CAL, codec, sclv, synth
    C, T, r = 1024, 10_000_000, 50
    cs = synth.generate(C, T, seed=3)
    plan = codec.Plan(cs.ch_off, cs.ch_len, 3, 6, MODE_APPROX, WIN_AFTER_CAL, sclv.table(3))
    e = plan.encode(cs.data)
    ref = torch.zeros_like(cs.data)
    plan.decode(e, ref)
    seg_off = torch.from_numpy(plan.segments()["off"].astype(np.int64)).cuda()
    del cs
    pitch = int(plan.ch_off[1] - plan.ch_off[0])
    assert np.all(np.diff(plan.ch_off.astype(np.int64)) == pitch)
    mat = ref.as_strided((C, T), (pitch, 1), int(plan.ch_off[0]))
    want = torch.empty((C, T // r), dtype=torch.int32, device="cuda")
    for i in range(0, C, 64):
        want[i:i + 64] = mat[i:i + 64].reshape(64, T // r, r).sum(dim=2, dtype=torch.int32)
    got = plan.decode_rebin(e.payload, seg_off, e.peak, e.enc, None, 0, T, r, saturate=False)
    assert plan.decode_ok() and torch.equal(got, want)
    got8 = plan.decode_rebin(e.payload, seg_off, e.peak, e.enc, None, 0, T, r, saturate=True)
    assert plan.decode_ok() and torch.equal(got8, want.clamp(max=255).to(torch.uint8))
    plan.close()
