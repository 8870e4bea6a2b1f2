"""The codec where ONE channel, or its payload, passes 2^32: the cases of tests/big_codec.py on the device.
tests/test_host_big_codec.py shows without a GPU that every closed form used here is the brute-force result, that an index
cut to 32 bits gives another one, and that no true, cut or sign-extended index leaves an allocation.

  Wrong, never a fault.  Every index starts at its buffer's first element and every large buffer of a direct call begins
  2^31 bytes (2^31 words in case B) inside its allocation, canary in front: a narrowed kernel reads a decoy or leaves canary.
  (StreamEncoder / StreamDecoder allocate their own buffers: an unsigned cut stays inside those as well.)
  References.  Closed forms from the period and the planted entries for the counts and bit totals; plain torch on the device,
  in slabs, for everything that is an image of the input (clamp, ==, sums over a [-1, r] view, transposes, cumsum); the CPU
  oracle on four 32 768-sample segments of the long channel.  Nothing expected comes from the library.
  Memory.  Each filling asserts its computed peak against the free memory before it allocates; the long input, and the
  drifted stream, are built once per filling and shared by the tests of that filling, which run one filling after another.

Every comparison is exact.  Each test prints its wall time (pytest -s)."""
import ctypes as ct
import gc
import time

import numpy as np
import pytest
import torch

import oracle
from tests import big_codec as bc
from tests import helpers
from tests.test_gpu_fullsize import _pack_ref

pytestmark = pytest.mark.gpu

OC = oracle.c
FAR = 1 << 32
SLAB = 1 << 28
LIM = 14                 # the fillings hold 0 .. 12 and 255
TABS = helpers.sclv_tables()


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec, container, stream, sweep  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    yield muahuff
    _drop()
    _drop_time_major()


@pytest.fixture(autouse=True)
def timed(request):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\n[big-codec] %s: %.2f s, peak %.2f GB allocated" % (request.node.name, time.perf_counter() - t0,
                                                               torch.cuda.max_memory_allocated() / 1e9))


def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _need(nbytes, what):
    _free()
    free, _total = torch.cuda.mem_get_info()
    assert nbytes < free, "%s needs ~%.1f GB of free HBM; %.1f GB free" % (what, nbytes / 1e9, free / 1e9)


def _led(body_bytes, fill=bc.CANARY, lead=bc.LEAD):
    """(allocation, body): the body begins `lead` bytes inside the allocation, canary in front of it"""
    whole = torch.empty(lead + body_bytes, dtype=torch.uint8, device="cuda")
    whole[:lead] = bc.CANARY
    whole[lead:] = fill
    return whole, whole[lead:]


def _lead_intact(whole, lead=bc.LEAD):
    return all(bool((whole[a:min(a + (1 << 30), lead)].view(torch.int64) == bc.CAN64).all()) for a in range(0, lead, 1 << 30))


def _all(t, value):
    """every element of the 1-D tensor equals value (in slabs)"""
    return all(bool((t[a:a + SLAB] == value).all()) for a in range(0, max(t.numel(), 1), SLAB))


def _i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda")


def _p(t):
    return ct.c_void_p(t.data_ptr())


def _put(row, ch):
    """expand a big_codec.Channel into its bytes `row` on the device"""
    n, pt = ch.n, torch.from_numpy(ch.period).cuda()
    reps = n // bc.P
    row[:reps * bc.P].view(reps, bc.P).copy_(pt.expand(reps, bc.P))
    row[reps * bc.P:n] = pt[:n - reps * bc.P]
    if ch.head[0]:
        row[:ch.head[0]] = ch.head[1]
    if ch.planted:
        row[_i64([i for i, _v in ch.planted])] = torch.tensor([v for _i, v in ch.planted], dtype=torch.uint8, device="cuda")


def _counts(row, a, b, lim):
    """int64 [lim] counts of min(x, lim - 1) over row[a:b]: torch, in slabs"""
    h = torch.zeros(lim, dtype=torch.int64, device="cuda")
    for s in range(a, b, SLAB):
        xc = torch.clamp(row[s:min(b, s + SLAB)], max=lim - 1)
        for v in range(lim):
            h[v] += (xc == v).sum()
    return h.cpu().numpy()


def _same_clipped(got, x, S, what):
    """got == min(x, S - 1), two 1-D tensors (any strides), in slabs"""
    assert got.numel() == x.numel()
    for a in range(0, x.numel(), SLAB):
        assert torch.equal(got[a:a + SLAB], torch.clamp(x[a:a + SLAB], max=S - 1)), (what, a)


def _bin_sums(row, r, lo, hi):
    """int32 sums of row (1-D uint8) in bins of r samples, bins [lo, hi); a cut last bin is kept"""
    n = row.numel()
    a, b = lo * r, min(hi * r, n)
    whole = (b - a) // r
    out = row[a:a + whole * r].view(whole, r).sum(1, dtype=torch.int32)
    if a + whole * r < b:
        out = torch.cat([out, row[a + whole * r:b].sum(dtype=torch.int32).view(1)])
    assert out.numel() == hi - lo
    return out


# ---- the long input, one filling at a time -----------------------------------------------------------------------------
class _Held:
    name = None


H = _Held()


def _drop():
    for k in list(vars(H)):
        delattr(H, k)
    _free()


def _filling(mh, name):
    """the three channels of the filling on the device (built once; the previous filling is freed first)"""
    if H.name == name:
        return H
    _drop()
    _drop_time_major()
    S = bc.FILLINGS[name][0]
    tab = TABS[S]
    a = bc.case_a(name, FAR, int(tab.max()))
    if name == "drifted-S10":
        # before anything is built: the oracle's bits a sample on one period, under the word that 64 zeros calibrate --
        # above 5.33 the dense stream of the long channel passes byte 2^32
        w = bc.expect_measure(a["chs"], S, 6, False, tab, OC.approx_sort_rule)[1]
        one = OC.encode_preset(np.concatenate([a["chs"][1].period, np.zeros(64, np.uint8)]), np.zeros(1, np.uint64),
                               np.array([bc.P], np.uint64), OC.Params(S, 0, 1, OC.WIN_FULL, tab, seg_chunks=2), w["peak"], w["enc"])
        assert int(one["ch_bits"][0]) / bc.P > 5.4
    _need(a["peak"], "case A, " + name)
    H.name, H.S, H.tab, H.a, H.chs, H.off = name, S, tab, a, a["chs"], a["off"]
    H.whole, H.x = _led(a["body"])
    for c, ch in enumerate(H.chs):
        _put(H.x[H.off[c]:H.off[c] + ch.n], ch)
    H.rows = [H.x[H.off[c]:H.off[c] + ch.n] for c, ch in enumerate(H.chs)]
    # the input itself against its closed form: the counts of every channel, the planted samples and their aliases
    H.counts = [_counts(H.rows[c], 0, ch.n, LIM) for c, ch in enumerate(H.chs)]          # (255 counts as LIM - 1)
    for c, ch in enumerate(H.chs):
        assert np.array_equal(H.counts[c], ch.hist(0, ch.n, LIM)), c
    t = np.array(sorted({j for i, _v in H.chs[1].planted for j in (i, i - FAR, i + 1, i - 1) if 0 <= j < H.chs[1].n}))
    assert np.array_equal(H.rows[1][torch.from_numpy(t).cuda()].cpu().numpy(), H.chs[1].at(t))
    H.want = bc.expect_measure(H.chs, S, 6, False, tab, OC.approx_sort_rule)
    return H


def _plan(mh, h, window):
    return mh.codec.Plan(np.array(H.off, np.uint64), np.array([c.n for c in H.chs], np.uint64), H.S, h, mh.MODE_APPROX, window, H.tab,
                         seg_chunks=2)


def _same_image(out, what):
    """a decoded buffer laid out like x: every channel min(x, S - 1), canary between and behind the channels"""
    end = 0
    for c, ch in enumerate(H.chs):
        assert _all(out[end:H.off[c]], bc.CANARY), (what, "gap in front of channel", c)
        _same_clipped(out[H.off[c]:H.off[c] + ch.n], H.rows[c], H.S, (what, c))
        end = H.off[c] + ch.n
    assert _all(out[end:], bc.CANARY), (what, "tail")


def _encode(mh, plan):
    a = H.a
    assert plan.payload_cap_words == a["cap"] and plan.n_segments == a["nseg"]
    whole, body = _led(4 * a["cap"])
    e = mh.codec.Encoded(body.view(torch.int32), torch.zeros(a["nseg"], dtype=torch.int64, device="cuda"),
                         torch.zeros(3, dtype=torch.int64, device="cuda"), *(torch.zeros(3, dtype=torch.uint8, device="cuda") for _ in range(3)))
    plan.encode(H.x, out=e)
    torch.cuda.synchronize()
    return whole, e


def _stream(mh):
    """the drifted filling encoded (h = 6, whole-channel windows) and compacted: shared by the tests that read it"""
    _filling(mh, "drifted-S10")
    if not hasattr(H, "e"):
        H.plan = _plan(mh, 6, mh.WIN_FULL)
        H.pay_whole, H.e = _encode(mh, H.plan)
    return H


def _dense(mh):
    _stream(mh)
    if not hasattr(H, "dense"):
        cap, nseg = H.a["cap"], H.a["nseg"]
        H.dense_whole, body = _led(4 * cap)
        H.d_off = torch.full((nseg,), -1, dtype=torch.int64, device="cuda")
        H.d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        H.dense, _tot = H.plan.compact(H.e, dense=body.view(torch.int32), off=H.d_off, tot=H.d_tot)
        torch.cuda.synchronize()
    return H


# ---- case A ---------------------------------------------------------------------------------------------------------------
def _measure(mh, name):
    """mh_measure at h = 6 over whole channels (k_hist / k_hist2): a count and a bit total above 2^32.  Then h = 30 with the
    window behind the calibration: cutoff 2^30, the tiled calibration with its 32-bit counters on 2^30 samples, peak = the
    first maximum of torch's counts, enc = the first minimum of table . rank-ordered counts, the window [2^30, T_LONG)."""
    _filling(mh, name)
    S, tab = H.S, H.tab
    for h, window in ((6, mh.WIN_FULL), (30, mh.WIN_AFTER_CAL)):
        want = bc.expect_measure(H.chs, S, h, window == mh.WIN_AFTER_CAL, tab, OC.approx_sort_rule)
        plan = _plan(mh, h, window)
        m = plan.measure(H.x)
        torch.cuda.synchronize()
        got = {k: getattr(m, k).cpu().numpy() for k in ("cutoff", "cal_hist", "peak", "enc", "post_hist", "bits", "skipped")}
        plan.close()
        for c, w in enumerate(want):
            for k in ("cutoff", "peak", "enc", "bits"):
                assert int(got[k][c]) == w[k], (h, c, k, int(got[k][c]), w[k])
            assert np.array_equal(got["cal_hist"][c], w["cal_hist"]) and np.array_equal(got["post_hist"][c], w["post_hist"]), (h, c)
            assert got["skipped"][c] == 0
        assert got["bits"][1] > FAR and (h == 30 or got["post_hist"][1].max() > FAR)
        if h == 30:
            # the calibration window of the long channel once more, from torch's counts of its first 2^30 samples
            cal = _counts(H.rows[1], 0, 1 << 30, S)
            peak = int(np.argmax(cal))
            idx = OC.approx_sort_rule(S, peak)
            assert got["cutoff"][1] == 1 << 30 and got["peak"][1] == peak and np.array_equal(got["cal_hist"][1], cal[idx])
            assert got["enc"][1] == int(np.argmin(tab.astype(np.int64) @ cal[idx]))
            post = _counts(H.rows[1], 1 << 30, bc.T_LONG, S)
            assert np.array_equal(got["post_hist"][1], post[idx]) and want[1]["w0"] == 1 << 30 and want[1]["w1"] == bc.T_LONG
            assert got["cutoff"][0] == 70001 and got["post_hist"][0].sum() == 0          # a short channel: all calibration


def _check_oracle_segments(plan, e, seg_off, what):
    """four segments of the long channel: the oracle's words under (peak, enc) are the GPU's, its decoder reads the GPU's"""
    S, T = H.S, H.chs[1].n
    seg = plan.segments()
    ids = np.flatnonzero(seg["ch"] == 1)
    assert [(int(seg["first"][s]), int(seg["n"][s])) for s in ids[:3]] == bc.segments_of(T)[:3]
    p1 = OC.Params(S, 0, 1, OC.WIN_FULL, H.tab, seg_chunks=2)
    peak, enc = int(e.peak[1]), int(e.enc[1])
    zero, sw = np.zeros(1, np.uint64), e.seg_words.cpu().numpy()
    for k in bc.oracle_segments(FAR, T):
        s = int(ids[k])
        first, n = int(seg["first"][s]), int(seg["n"][s])
        assert (first, n) == (k * bc.SEG, min(bc.SEG, T - k * bc.SEG))
        x = np.concatenate([H.rows[1][first:first + n].cpu().numpy(), np.zeros(64, np.uint8)])
        one = OC.encode_preset(x, zero, np.array([n], np.uint64), p1, peak, enc)
        o, w = int(seg_off[s]), int(sw[s])
        words = e.payload[o:o + w].cpu().numpy().view(np.uint32)
        assert int(one["seg_words"][0]) == w and np.array_equal(one["payload"][:w], words), (what, k)
        pay = np.zeros(one["seg"]["cap_words"] + 4, np.uint32)
        pay[:w] = words
        got = OC.decode(pay, zero, np.array([n], np.uint64), p1, [peak], [enc], n)
        assert np.array_equal(got, np.minimum(x[:n], S - 1)), (what, k)
    return seg


def _encode_decode(mh, name):
    """mh_encode into the plan's slots and mh_decode from them: ch_bits in closed form (above 2^32), the sizes consistent,
    the round trip min(x, S - 1) over the whole buffer with the canary between the channels, four segments against the
    oracle.  A seg_first >= 2^32; with S = 10 a slot behind word 2^30."""
    _filling(mh, name)
    S, a = H.S, H.a
    if name == "drifted-S10":
        _stream(mh)
        plan, pay_whole, e = H.plan, H.pay_whole, H.e
    else:
        plan = _plan(mh, 6, mh.WIN_FULL)
        pay_whole, e = _encode(mh, plan)
    seg = plan.segments()
    assert seg["first"].max() >= FAR and (S != 10 or seg["off"].max() >= 1 << 30)
    for c, w in enumerate(H.want):
        assert (int(e.peak[c]), int(e.enc[c]), int(e.ch_bits[c])) == (w["peak"], w["enc"], w["bits"]), c
        cnt = np.append(H.counts[c][:S - 1], H.counts[c][S - 1:].sum())          # torch's counts of the input, clipped at S - 1
        assert w["bits"] == int((cnt * w["lens"]).sum())
    assert int(e.ch_bits[1]) > FAR and int(e.skipped.sum()) == 0
    if name == "drifted-S10":
        assert (int(e.peak[1]), int(e.ch_bits[1]) / bc.T_LONG > 5.4) == (0, True)
    # sizes: a segment holds its code bits and its chunk headers, and fits its slot
    sw = e.seg_words.cpu().numpy()
    slots = np.diff(np.append(seg["off"].astype(np.int64), a["cap"] - 4))
    assert (sw > 0).all() and (sw <= slots).all()
    for c in range(3):
        mine = seg["ch"] == c
        chunks = int(np.ceil(seg["n"][mine].astype(np.int64) / bc.CHUNK).sum())
        words = int(sw[mine].sum())
        assert 32 * words >= int(e.ch_bits[c]) + 32 * chunks, c          # (a chunk header is at least one word)
    assert _lead_intact(pay_whole)
    _check_oracle_segments(plan, e, seg["off"], name)
    out_whole, out = _led(a["body"])
    plan.decode(e, out)
    assert plan.decode_ok()
    _same_image(out, name)
    assert _lead_intact(out_whole)
    del out, out_whole
    if name != "drifted-S10":
        plan.close()
        del e, pay_whole
    _free()


def _long_calibration(mh):
    """the h = 30 plan of the sparse S = 10 filling: windows [2^30, T_LONG) and nothing of the short channels; the bytes in
    front of the window keep the canary"""
    _filling(mh, "sparse-S10")
    S, T = H.S, bc.T_LONG
    want = bc.expect_measure(H.chs, S, 30, True, H.tab, OC.approx_sort_rule)
    plan = _plan(mh, 30, mh.WIN_AFTER_CAL)
    nseg, cap = plan.n_segments, plan.payload_cap_words
    assert nseg == -(-(T - (1 << 30)) // bc.SEG) and plan.window_samples == T - (1 << 30)
    pay_whole, body = _led(4 * cap)
    e = mh.codec.Encoded(body.view(torch.int32), torch.zeros(nseg, dtype=torch.int64, device="cuda"),
                         torch.zeros(3, dtype=torch.int64, device="cuda"), *(torch.zeros(3, dtype=torch.uint8, device="cuda") for _ in range(3)))
    plan.encode(H.x, out=e)
    torch.cuda.synchronize()
    for c, w in enumerate(want):
        assert (int(e.peak[c]), int(e.enc[c]), int(e.ch_bits[c])) == (w["peak"], w["enc"], w["bits"]), c
    assert int(e.ch_bits[1]) > FAR and plan.segments()["first"].max() + (1 << 30) >= FAR
    out_whole, out = _led(H.a["body"])
    plan.decode(e, out)
    assert plan.decode_ok()
    o1 = H.off[1]
    assert _all(out[:o1 + (1 << 30)], bc.CANARY) and _all(out[o1 + T:], bc.CANARY)
    _same_clipped(out[o1 + (1 << 30):o1 + T], H.rows[1][1 << 30:], S, "h=30")
    assert _lead_intact(out_whole) and _lead_intact(pay_whole)
    plan.close()
    del out, out_whole, e, pay_whole, body
    _free()


def _compact_dense(mh):
    """mh_compact of the drifted stream: dense_off is the exclusive cumsum of seg_words and passes word 2^30 (byte 2^32) inside
    the long channel; every dense word is its slot's; canary behind `total`; mh_decode from the dense offsets"""
    _dense(mh)
    nseg, sw = H.a["nseg"], H.e.seg_words
    want_off = torch.cumsum(sw, 0) - sw
    total = int(sw.sum())
    assert int(H.d_tot[0]) == total and torch.equal(H.d_off, want_off)
    seg = H.plan.segments()
    inside = np.flatnonzero(seg["ch"] == 1)
    assert int(want_off[int(inside[-1])]) >= 1 << 30 and 4 * total > FAR + (1 << 31)
    slot_off = torch.from_numpy(seg["off"].astype(np.int64)).cuda()
    ends = want_off + sw
    for a in range(0, total, 1 << 26):
        j = torch.arange(a, min(a + (1 << 26), total), dtype=torch.int64, device="cuda")
        s = torch.searchsorted(ends, j, right=True)
        assert torch.equal(H.dense.payload[a:a + j.numel()], H.e.payload[slot_off[s] + j - want_off[s]]), a
        del j, s
    assert _all(H.dense.payload[total:], bc.CAN32) and _lead_intact(H.dense_whole)
    assert nseg == sw.numel()
    _check_oracle_segments(H.plan, H.dense, H.d_off.cpu().numpy(), "dense")
    out_whole, out = _led(H.a["body"])
    H.plan.decode(H.dense, out)
    assert H.plan.decode_ok()
    _same_image(out, "dense")
    assert _lead_intact(out_whole)
    del out, out_whole
    _free()


def _decode_range(mh):
    """mh_decode_range on the dense stream: (a) one row longer than 2^32 bytes, (b) three rows around 2^32 on an odd pitch,
    two of them zero fill, (c) the last three samples"""
    _dense(mh)
    S, T, d = H.S, bc.T_LONG, H.dense
    whole, body = _led(T + 128)
    H.plan.decode_range(d.payload, d.seg_off, d.peak, d.enc, [1], 0, T, out=body[:T].view(1, T))
    assert H.plan.decode_ok()
    _same_clipped(body[:T], H.rows[1], S, "range a")
    assert _all(body[T:], bc.CANARY) and _lead_intact(whole)
    del whole, body
    _free()
    lo, n, pitch = FAR - 20000, 40000, 40013
    buf = torch.full((3 * pitch + 64,), bc.CANARY, dtype=torch.uint8, device="cuda")
    H.plan.decode_range(d.payload, d.seg_off, d.peak, d.enc, [1, 0, 2], lo, lo + n, out=buf.as_strided((3, n), (pitch, 1)))
    assert H.plan.decode_ok()
    want = torch.full_like(buf, bc.CANARY)
    rows = want.as_strided((3, n), (pitch, 1))
    rows[0] = torch.clamp(H.rows[1][lo:lo + n], max=S - 1)
    rows[1:] = 0
    assert torch.equal(buf, want)
    buf = torch.full((64,), bc.CANARY, dtype=torch.uint8, device="cuda")
    H.plan.decode_range(d.payload, d.seg_off, d.peak, d.enc, [1], T - 3, T, out=buf[16:19].view(1, 3))
    assert H.plan.decode_ok()
    want = torch.full_like(buf, bc.CANARY)
    want[16:19] = torch.clamp(H.rows[1][T - 3:], max=S - 1)
    assert torch.equal(buf, want) and int(want[18]) == 9 == H.chs[1].planted[-1][1]


def _decode_rebin(mh):
    """mh_decode_rebin on the dense stream: r = 100 and r = 96 (more than 2^26 bins) over the whole channel, exact sums with
    the cut last bin; r = 7 from the multiple of 7 below 2^32 - 20000, 40 000 samples, both output forms"""
    _dense(mh)
    S, T, d = H.S, bc.T_LONG, H.dense
    clipped = lambda a, b: torch.clamp(H.rows[1][a:b], max=S - 1)          # noqa: E731
    for r in (100, 96):
        nb = -(-T // r)
        assert (r == 100 or nb >= 1 << 26) and T % r
        buf = torch.full((4 * (nb + 16),), bc.CANARY, dtype=torch.uint8, device="cuda").view(torch.int32)
        H.plan.decode_rebin(d.payload, d.seg_off, d.peak, d.enc, [1], 0, T, r, saturate=False, out=buf[:nb].view(1, nb))
        assert H.plan.decode_ok()
        step = 1 << 21
        for b0 in range(0, nb, step):
            b1 = min(nb, b0 + step)
            assert torch.equal(buf[b0:b1], _bin_sums(clipped(b0 * r, min(b1 * r, T)), r, 0, b1 - b0)), (r, b0)
        assert _all(buf[nb:], bc.CAN32)
        del buf
    t0, n, r = (FAR - 20000) // 7 * 7, 40000, 7
    nb = -(-n // r)
    ref = _bin_sums(clipped(t0, t0 + n), r, 0, nb)
    for sat in (True, False):
        dt = torch.uint8 if sat else torch.int32
        buf = torch.full(((nb + 16) * (1 if sat else 4),), bc.CANARY, dtype=torch.uint8, device="cuda").view(dt)
        H.plan.decode_rebin(d.payload, d.seg_off, d.peak, d.enc, [1], t0, t0 + n, r, saturate=sat, out=buf[:nb].view(1, nb))
        assert H.plan.decode_ok()
        assert torch.equal(buf[:nb], torch.clamp(ref, max=255).to(dt)) and _all(buf[nb:], bc.CANARY if sat else bc.CAN32), sat
    assert int(ref.max()) > 9 and t0 < FAR < t0 + n
    _free()


def _rebin(mh, r, sat):
    """mh_rebin on the raw bytes of the sparse S = 10 filling: r = 2 behind k_rebin2's tile clamp with b0 >= 2^31 bins; r = 17
    and 68 behind the 65535-workgroup cap of k_rebin3 (370 086 tiles against 262 140 a pass); r = 100.  The cut last bin of
    every channel, canary between the channels' bins."""
    _filling(mh, "sparse-S10")
    lens = np.array([c.n for c in H.chs], np.int64)
    nb = -(-lens // r)
    assert lens[1] % r and (r != 2 or nb[1] >= 1 << 31)
    out_off = 64 + np.cumsum(nb + 48) - nb - 48
    size = int(out_off[-1] + nb[-1]) + 64
    elem = 1 if sat else 4
    whole, body = _led(size * elem)
    out = body if sat else body.view(torch.int32)
    d_off, d_len, d_ooff = _i64(H.off), _i64(lens), _i64(out_off)
    mh._lib.check(mh._lib.lib().mh_rebin(_p(H.x), _p(d_off), _p(d_len), 3, int(lens.max()), r, sat, _p(out), _p(d_ooff), None))
    torch.cuda.synchronize()
    can = bc.CANARY if sat else bc.CAN32
    end = 0
    step = max(1, (1 << 27) // r)
    for c in range(3):
        o, n = int(out_off[c]), int(nb[c])
        assert _all(out[end:o], can), ("gap", c)
        for b0 in range(0, n, step):
            b1 = min(n, b0 + step)
            ref = _bin_sums(H.rows[c], r, b0, b1)
            assert torch.equal(out[o + b0:o + b1], torch.clamp(ref, max=255).to(torch.uint8) if sat else ref), (c, b0)
        end = o + n
    assert _all(out[end:], can) and _lead_intact(whole)
    if sat and r > 2:
        assert int(_bin_sums(H.rows[1], r, (FAR - 1) // r, (FAR - 1) // r + 1)) > 255          # the planted 255s saturate a bin
    del whole, body, out
    _free()


def _sweep(mh):
    """mh_sweep_create / mh_sweep_run with hist_bits = (6, 30) on the sparse S = 10 filling: the bounds are the restated
    breakpoints, the last one T_LONG, and every interval's histogram is torch's count between its bounds"""
    _filling(mh, "sparse-S10")
    lens = [c.n for c in H.chs]
    sw = mh.sweep.SweepHist(np.array(H.off, np.uint64), np.array(lens, np.uint64), (6, 30))
    bounds = np.array([sorted([0, T] + [b for h in (6, 30) for b in (min(2 ** h, T), min(min(2 ** h, T) + T // 2, T))]) for T in lens])
    assert sw.n_intervals == 5 and np.array_equal(sw.bounds.astype(np.int64), bounds) and bounds[1, -1] == bc.T_LONG >= FAR
    assert bounds[1].tolist() == [0, 64, 1 << 30, 64 + bc.T_LONG // 2, (1 << 30) + bc.T_LONG // 2, bc.T_LONG]
    sw.run(H.x)
    hist = np.diff(sw.cum, axis=1)
    sw.close()
    for c, ch in enumerate(H.chs):
        for j in range(5):
            lo, hi = int(bounds[c, j]), int(bounds[c, j + 1])
            assert np.array_equal(hist[c, j], _counts(H.rows[c], lo, hi, 10)), (c, j)
            assert np.array_equal(hist[c, j], ch.hist(lo, hi, 10)), (c, j)
    assert hist[1].sum() == bc.T_LONG and hist[1, :, 0].sum() > FAR // 2


# the tests of case A, one filling after another (each filling is built once)
def test_sparse_s3_measure(mh):
    _measure(mh, "sparse-S3")


def test_sparse_s3_encode_decode(mh):
    _encode_decode(mh, "sparse-S3")


def test_sparse_s10_measure(mh):
    _measure(mh, "sparse-S10")


def test_sparse_s10_encode_decode(mh):
    _encode_decode(mh, "sparse-S10")


def test_sparse_s10_encode_decode_behind_a_long_calibration(mh):
    _long_calibration(mh)


@pytest.mark.parametrize("r,sat", [(2, 1), (17, 0), (17, 1), (68, 0), (68, 1), (100, 0)])
def test_sparse_s10_rebin(mh, r, sat):
    _rebin(mh, r, sat)


def test_sparse_s10_sweep_histograms(mh):
    _sweep(mh)


def test_drifted_s10_encode_decode(mh):
    _encode_decode(mh, "drifted-S10")


def test_drifted_s10_compact_and_decode_the_dense_stream(mh):
    _compact_dense(mh)


def test_drifted_s10_decode_range(mh):
    _decode_range(mh)


def test_drifted_s10_decode_rebin(mh):
    _decode_rebin(mh)


# ---- case B: mh_compact past 2^32 words -------------------------------------------------------------------------------------
def test_compact_past_2_to_32_words(mh):
    """A plan only: 512 channels of 919 segments, 17.5 GB of slots.  The source offsets seg_off[seg] pass word 2^32, the
    destinations pass word 2^30 (byte 2^32) and word 2^32; seg_words with zeros next to the crossing.  dense_off against
    cumsum, `total`, every dense word against the payload's formula at its slot, the lead and the canary behind `total`."""
    _drop()
    _drop_time_major()
    b = bc.case_b(FAR)
    _need(b["peak"], "case B")
    tab = TABS[10]
    assert int(tab.max()) == bc.B_MAXLEN
    from muahuff.container import layout
    off, ln, _total = layout([b["T"]] * b["C"])
    plan = mh.codec.Plan(off, ln, 10, 0, mh.MODE_APPROX, mh.WIN_FULL, tab, seg_chunks=2)
    seg = plan.segments()
    assert plan.n_segments == b["nseg"] and plan.payload_cap_words == b["payload_words"]
    assert np.array_equal(seg["off"].astype(np.int64), b["slot_off"])
    lead = 4 * bc.LEAD
    pay_whole, pay = _led(4 * b["payload_words"], lead=lead)
    payload = pay.view(torch.int32)
    for a in range(0, b["payload_words"], 1 << 27):
        i = torch.arange(a, min(a + (1 << 27), b["payload_words"]), dtype=torch.int64, device="cuda")
        v = (i * 40503 + (i >> 20)) & 0xFFFFFFFF
        payload[a:a + i.numel()] = (((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)).to(torch.int32)
        del i, v
    probe = np.array([0, 1, (1 << 31) - 1, 1 << 31, FAR - 1, FAR, FAR + 5, b["payload_words"] - 1])
    assert np.array_equal(payload[torch.from_numpy(probe).cuda()].cpu().numpy().view(np.uint32), bc.payload_word(probe).astype(np.uint32))
    d_sw = torch.from_numpy(b["seg_words"]).cuda()
    total = b["total"]
    assert total > FAR + (1 << 24) and (b["slot_off"] >= FAR).any() and (b["dense_off"] >= FAR).any()
    dense_whole, dbody = _led(4 * (total + 64), lead=lead)
    dense = dbody.view(torch.int32)
    d_off = torch.full((b["nseg"],), -1, dtype=torch.int64, device="cuda")
    d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    e = mh.codec.Encoded(payload, d_sw, None, None, None, None)
    d, tot = plan.compact(e, dense=dense, off=d_off, tot=d_tot)
    torch.cuda.synchronize()
    want_off = torch.cumsum(d_sw, 0) - d_sw
    assert int(tot[0]) == total and torch.equal(d.seg_off, want_off)
    assert np.array_equal(want_off.cpu().numpy(), b["dense_off"])
    slot_off, ends = torch.from_numpy(b["slot_off"]).cuda(), want_off + d_sw
    for a in range(0, total, 1 << 26):
        j = torch.arange(a, min(a + (1 << 26), total), dtype=torch.int64, device="cuda")
        s = torch.searchsorted(ends, j, right=True)
        src = slot_off[s] + j - want_off[s]
        v = (src * 40503 + (src >> 20)) & 0xFFFFFFFF
        want = (((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)).to(torch.int32)
        assert torch.equal(dense[a:a + j.numel()], want), a
        del j, s, src, v, want
    assert _all(dense[total:], bc.CAN32) and _lead_intact(dense_whole, lead) and _lead_intact(pay_whole, lead)
    plan.close()
    del payload, pay, pay_whole, dense, dbody, dense_whole, e, d
    _free()


# ---- case C: the layout calls and the stream path with T >= 2^32 ------------------------------------------------------------
class _TimeMajor:
    pass


TM = _TimeMajor()


def _time_major(mh):
    """x [T, 3] time-major, T = 2^32 + 4099, behind a lead (built once for the tests of case C)"""
    if hasattr(TM, "x"):
        return TM
    _drop()
    c = bc.case_c(FAR)
    _need(c["peak"] + (18 << 30), "case C")
    TM.c, TM.T, TM.chs = c, c["T"], c["chs"]
    TM.whole, body = _led(bc.C_CH * c["T"])
    TM.x = body.view(c["T"], bc.C_CH)
    for k, ch in enumerate(TM.chs):
        _put(TM.x[:, k], ch)
    t = np.array([0, bc.D, FAR - 1, FAR, FAR + bc.D, c["T"] - 1])
    for k, ch in enumerate(TM.chs):
        assert np.array_equal(TM.x[torch.from_numpy(t).cuda(), k].cpu().numpy(), ch.at(t))
    return TM


def _drop_time_major():
    for k in list(vars(TM)):
        delattr(TM, k)
    _free()


def test_deinterleave_and_interleave_past_2_to_32_steps(mh):
    """mh_deinterleave of [2^32 + 4099, 3] into channels with canary behind each, then mh_interleave back: both against torch's
    strided views of x, in slabs"""
    _time_major(mh)
    T, pitch = TM.T, TM.c["pitch"]
    cm_whole, cm = _led(bc.C_CH * pitch)
    d_off = _i64([k * pitch for k in range(bc.C_CH)])
    lib = mh._lib.lib()
    mh._lib.check(lib.mh_deinterleave(_p(TM.x), T, bc.C_CH, _p(cm), _p(d_off), None))
    torch.cuda.synchronize()
    for k in range(bc.C_CH):
        row = cm[k * pitch:(k + 1) * pitch]
        for a in range(0, T, SLAB):
            assert torch.equal(row[a:min(a + SLAB, T)], TM.x[a:a + SLAB, k]), (k, a)
        assert _all(row[T:], bc.CANARY), k
    assert _lead_intact(cm_whole)
    tm_whole, tm = _led(bc.C_CH * T + 128)
    mh._lib.check(lib.mh_interleave(_p(cm), _p(d_off), T, bc.C_CH, _p(tm), None))
    torch.cuda.synchronize()
    flat = TM.x.view(-1)
    for a in range(0, flat.numel(), SLAB):
        assert torch.equal(tm[a:min(a + SLAB, flat.numel())], flat[a:a + SLAB]), a
    assert _all(tm[flat.numel():], bc.CANARY) and _lead_intact(tm_whole)
    del cm, cm_whole, tm, tm_whole
    _free()


@pytest.mark.parametrize("bits,blocked", [(2, False), (2, True), (4, False), (4, True)])
def test_packed_layout_calls_past_2_to_32_steps(mh, bits, blocked):
    """mh_deinterleave_packed against _pack_ref (tests/test_gpu_fullsize.py), contiguous and chunk-blocked -- blocked at 4 bits
    chunk 2^18 of every channel lies behind byte 2^32 -- then mh_interleave_packed back to min(x, 2^bits - 1)"""
    _time_major(mh)
    T, C = TM.T, bc.C_CH
    pb, npiece = 2 * bits, (T + 15) // 16
    cb, nch = 1024 * pb, (T + 16383) // 16384
    lib = mh._lib.lib()
    if blocked:
        stride, size = C * cb, nch * C * cb
        offs = [k * cb for k in range(C)]
        assert nch > 1 << 18 and (bits != 4 or (1 << 18) * stride > FAR)
    else:
        pitch = (npiece * pb + 15) // 16 * 16 + 128
        stride, size = 0, C * pitch
        offs = [k * pitch for k in range(C)]
    whole, out = _led(size + 256)
    d_off = _i64(offs)
    mh._lib.check(lib.mh_deinterleave_packed(_p(TM.x), T, C, bits, _p(out), _p(d_off), stride, None))
    torch.cuda.synchronize()
    slab_chunks = 4096
    for j0 in range(0, nch, slab_chunks):
        j1 = min(nch, j0 + slab_chunks)
        ref = _pack_ref(TM.x[j0 * 16384:j1 * 16384], bits)                      # [C, pieces of the slab * pb]
        if blocked:
            # whole 16-byte items: zeros behind the last piece up to the next 16 bytes, the rest of the last chunk is canary
            want = torch.full((C, (j1 - j0) * cb), bc.CANARY, dtype=torch.uint8, device="cuda")
            want[:, :(ref.shape[1] + 15) // 16 * 16] = 0
            want[:, :ref.shape[1]] = ref
            got = out[j0 * stride:j1 * stride].view(j1 - j0, C, cb).permute(1, 0, 2).reshape(C, -1)
            assert torch.equal(got, want), (bits, "chunks", j0)
        else:
            rows = out[:size].view(C, -1)
            p0 = j0 * cb
            assert torch.equal(rows[:, p0:p0 + ref.shape[1]], ref), (bits, j0)
        del ref
    if not blocked:
        rows = out[:size].view(C, -1)
        used = (npiece * pb + 15) // 16 * 16
        assert bool((rows[:, npiece * pb:used] == 0).all()) and bool((rows[:, used:] == bc.CANARY).all())
    assert _all(out[size:], bc.CANARY) and _lead_intact(whole)
    tm_whole, tm = _led(C * T + 128)
    mh._lib.check(lib.mh_interleave_packed(_p(out), _p(d_off), T, C, bits, stride, _p(tm), None))
    torch.cuda.synchronize()
    _same_clipped(tm[:C * T], TM.x.view(-1), 1 << bits, ("interleave_packed", bits, blocked))
    assert _all(tm[C * T:], bc.CANARY) and _lead_intact(tm_whole)
    del out, whole, tm, tm_whole
    _free()


@pytest.mark.parametrize("S", [3, 10])
def test_stream_path_past_2_to_32_steps(mh, S):
    """StreamEncoder.encode_block_device (packed chunk-blocked plan, mh_encode_preset, the compaction) and StreamDecoder back
    to time-major (mh_decode_packed, mh_interleave_packed) on a block of 2^32 + 4099 steps: min(x, S - 1), ch_bits in closed
    form, two segments of channel 1 around t = 2^32 against the oracle"""
    _time_major(mh)
    T, C, tab = TM.T, bc.C_CH, TABS[S]
    want = bc.expect_measure(TM.chs, S, 6, False, tab, OC.approx_sort_rule)
    se = mh.stream.StreamEncoder(C, S, 6, tab)
    peak, enc = se.calibrate(TM.x[:64].contiguous())
    assert peak.cpu().tolist() == [w["peak"] for w in want] and enc.cpu().tolist() == [w["enc"] for w in want]
    dense, tot, slot = se.encode_block_device(TM.x)
    torch.cuda.synchronize()
    plan = slot["plan"]
    nseg, per = plan.n_segments, -(-T // bc.SEG)
    assert plan.input_bits == (2 if S <= 4 else 4) and nseg == C * per
    assert S <= 4 or plan.chunk_stride * (-(-T // bc.CHUNK) - 1) > FAR          # the last chunks lie behind byte 2^32 of the pieces
    sw = dense.seg_words[:nseg]
    assert int(tot[0]) == int(sw.sum()) and torch.equal(dense.seg_off[:nseg], torch.cumsum(sw, 0) - sw)
    assert dense.ch_bits.cpu().tolist() == [w["bits"] for w in want]
    p1 = OC.Params(S, 0, 1, OC.WIN_FULL, tab, seg_chunks=2)
    zero = np.zeros(1, np.uint64)
    for k in (FAR // bc.SEG - 1, FAR // bc.SEG):
        s, n = per + k, min(bc.SEG, T - k * bc.SEG)                    # (the one behind 2^32 is the last: 4099 samples)
        x = np.concatenate([TM.x[k * bc.SEG:k * bc.SEG + n, 1].cpu().numpy(), np.zeros(64, np.uint8)])
        one = OC.encode_preset(x, zero, np.array([n], np.uint64), p1, want[1]["peak"], want[1]["enc"])
        o, w = int(dense.seg_off[s]), int(sw[s])
        assert int(one["seg_words"][0]) == w and np.array_equal(one["payload"][:w], dense.payload[o:o + w].cpu().numpy().view(np.uint32)), k
    pay, seg_words, seg_off = dense.payload, sw.clone(), dense.seg_off[:nseg].clone()
    del dense, slot, plan, sw
    se.close()
    del se
    _free()
    sd = mh.stream.StreamDecoder(C, S, tab)
    out = sd.decode_block_device(pay, seg_words, peak, enc, T, seg_off=seg_off)
    assert sd.ok()
    _same_clipped(out.view(-1), TM.x.view(-1), S, ("stream", S))
    sd.close()
    del sd, out, pay
    _free()


RUNS = {"A-measure": (test_sparse_s3_measure, test_sparse_s10_measure),
        "A-codec": (test_sparse_s3_encode_decode, test_sparse_s10_encode_decode, test_sparse_s10_encode_decode_behind_a_long_calibration,
                    test_drifted_s10_encode_decode),
        "A-compact": (test_drifted_s10_compact_and_decode_the_dense_stream,), "A-range": (test_drifted_s10_decode_range,),
        "A-decode-rebin": (test_drifted_s10_decode_rebin,), "A-rebin": (test_sparse_s10_rebin,), "A-sweep": (test_sparse_s10_sweep_histograms,),
        "B-compact": (test_compact_past_2_to_32_words,), "C-layout": (test_deinterleave_and_interleave_past_2_to_32_steps,),
        "C-packed": (test_packed_layout_calls_past_2_to_32_steps,), "C-stream": (test_stream_path_past_2_to_32_steps,)}


def test_every_case_of_the_table_is_run():
    assert set(RUNS) == {c.id for c in bc.CASES}
