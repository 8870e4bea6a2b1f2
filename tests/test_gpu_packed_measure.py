"""mh_measure on packed plans (mh_plan_create_packed, 2- and 4-bit pieces) and the drift tracking StreamEncoder builds on
it.  Every expectation comes from the CPU oracle on the unpacked samples min(x, 2^bits - 1); the pieces are built on the
host from the bit layout include/muahuff.h documents (sample i in bits [i * bits, (i + 1) * bits) of the channel's
little-endian stream, 16 samples per piece, chunk j of a chunk-blocked channel at ch_off + j * chunk_stride)."""
import numpy as np
import pytest
import torch

import oracle
from tests import async_table as at
from tests import helpers

pytestmark = pytest.mark.gpu

OC = oracle.c
CH = at.CHUNK
CANARY = 0xA5
NT = 16
FIELDS = ("cutoff", "cal_hist", "peak", "enc", "post_hist", "bits", "skipped")
ORACLE_KEY = dict(cutoff="cutoff", cal_hist="cal_sorted", peak="peak", enc="enc", post_hist="post_mapped", bits="bits",
                  skipped="skipped")
# (piece bits, S): every S the issue lists for each piece width
WIDTHS = ((2, 2), (2, 3), (2, 4), (4, 3), (4, 5), (4, 8), (4, 10))
LENS = (7, 1000, CH, CH + 1, 40000, 3 * CH)


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec, stream  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    return muahuff


def _pack(x, bits, rng=None):
    """one channel -> its pieces (uint8): min(x, 2^bits - 1), 16 samples per piece; the fields behind the last sample
    are zero, or non-zero garbage when rng is given"""
    T = len(x)
    top = (1 << bits) - 1
    s = np.zeros((T + 15) // 16 * 16, np.uint8)
    s[:T] = np.minimum(x, top)
    if rng is not None:
        s[T:] = rng.randint(1, top + 1, size=len(s) - T)
    per = 8 // bits
    g = s.reshape(-1, per).astype(np.uint32)
    by = np.zeros(len(g), np.uint32)
    for f in range(per):
        by |= g[:, f] << (bits * f)
    return by.astype(np.uint8)


def _place(chans, bits, blocked, rng=None):
    """-> (buffer, ch_off, chunk_stride): canary bytes everywhere but in the pieces"""
    cb = CH * bits // 8
    C = len(chans)
    pieces = [_pack(x, bits, rng) for x in chans]
    if blocked:
        nch = max((len(x) + CH - 1) // CH for x in chans)
        buf = np.full(nch * C * cb, CANARY, np.uint8)
        for c, pk in enumerate(pieces):
            for j in range(0, len(pk), cb):
                a = c * cb + (j // cb) * C * cb
                buf[a:a + len(pk[j:j + cb])] = pk[j:j + cb]
        return buf, np.arange(C, dtype=np.uint64) * np.uint64(cb), C * cb
    sz = [(len(pk) + 15) // 16 * 16 + 16 for pk in pieces]
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
    buf = np.full(int(sum(sz)), CANARY, np.uint8)
    for pk, o in zip(pieces, off):
        buf[int(o):int(o) + len(pk)] = pk
    return buf, off, 0


def _channels(rng, lens):
    """spike-count like channels with different rates (some reach above 15), one all-zero and one all-250"""
    out = []
    for i, T in enumerate(lens):
        lam = (0.15, 0.8, 2.5, 6.0, 13.0)[i % 5]
        out.append(np.minimum(rng.poisson(lam, size=T), 255).astype(np.uint8))
    return out


def _oracle(chans, bits, S, h, mode, rows):
    un = [np.minimum(x, (1 << bits) - 1) for x in chans]
    data, off, ln = OC.flatten(un)
    return OC.measure(data, off, ln, OC.Params(S, h, mode, 3, rows), nthreads=NT), un


def _check(m, want, tag):
    torch.cuda.synchronize()
    for f in FIELDS:
        got = getattr(m, f).cpu().numpy()
        exp = want[ORACLE_KEY[f]]
        assert np.array_equal(got.astype(np.uint64), exp.astype(np.uint64)), (tag, f, np.argwhere(got.astype(np.uint64) != exp.astype(np.uint64))[:4])


def _check_np(m, un, S, h, mode, tag):
    """peak and the rank-ordered calibration histogram against the NumPy restatement of approx_sort"""
    peak = m.peak.cpu().numpy()
    cal = m.cal_hist.cpu().numpy()
    for c, x in enumerate(un):
        hist = oracle.np_.hist_clipped(x[:min(1 << h, len(x))], S)
        idx = oracle.np_.approx_sort_idx(hist) if mode == 1 else np.arange(S)
        assert int(peak[c]) == (int(idx[0]) if mode == 1 else 0), (tag, c)
        assert np.array_equal(cal[c].astype(np.int64), hist[idx]), (tag, c)


def _measure_packed(mh, chans, bits, S, h, mode, rows, blocked, rng=None):
    buf, off, stride = _place(chans, bits, blocked, rng)
    ln = np.array([len(x) for x in chans], np.uint64)
    plan = mh.codec.Plan(off, ln, S, h, mode, mh.WIN_FULL, rows, seg_chunks=1, input_bits=bits, chunk_stride=stride)
    m = plan.measure(torch.from_numpy(buf).cuda())
    torch.cuda.synchronize()
    plan.close()
    return m


@pytest.mark.parametrize("blocked", (False, True), ids=("contiguous", "chunk-blocked"))
@pytest.mark.parametrize("h", (2, 6, 13))
@pytest.mark.parametrize("bits,S", WIDTHS)
def test_packed_measure_equals_the_oracle(mh, bits, S, h, blocked):
    """All seven outputs, both mapper modes, K = 1 and the full SCLV table.  Lengths 7 and 1000 are shorter than 2^13
    (7 also than 2^6) and not multiples of 16 or of a piece; the contiguous layout carries non-zero garbage in the
    padding fields of every cut last piece."""
    rng = np.random.RandomState(1000 * bits + 100 * S + 10 * h + int(blocked))
    chans = _channels(rng, LENS) + [np.zeros(20001, np.uint8), np.full(CH + 9, 250, np.uint8)]
    table = helpers.sclv_tables()[S]
    for mode in (0, 1):
        for rows in (table[-1:], table):
            tag = (bits, S, h, blocked, mode, len(rows))
            want, un = _oracle(chans, bits, S, h, mode, rows)
            m = _measure_packed(mh, chans, bits, S, h, mode, rows, blocked, None if blocked else rng)
            _check(m, want, tag)
            _check_np(m, un, S, h, mode, tag)


@pytest.mark.parametrize("bits,S,h,blocked", ((2, 3, 6, True), (4, 5, 13, False), (4, 10, 6, True), (2, 4, 13, False)))
def test_packed_measure_on_long_channels(mh, bits, S, h, blocked):
    """70 channels x 147 461 steps: nine chunks and five samples, so two tiles per channel and a cut last piece"""
    rng = np.random.RandomState(7 * bits + S + h)
    chans = _channels(rng, (147461,) * 70)
    rows = helpers.sclv_tables()[S]
    want, un = _oracle(chans, bits, S, h, 1, rows)
    m = _measure_packed(mh, chans, bits, S, h, 1, rows, blocked, rng)
    _check(m, want, (bits, S, h, blocked))
    _check_np(m, un, S, h, 1, (bits, S, h, blocked))


def test_packed_measure_above_the_fused_channel_limit(mh):
    """layout "b" of tests/async_table.py: more than 4096 channels of four chunks each (the byte plan's non-fused form)"""
    L = at.BY_NAME["b"]
    rng = np.random.RandomState(4100)
    flat = rng.randint(0, 6, size=(len(L.lens), L.lens[0])).astype(np.uint8)
    flat[::3] = np.minimum(flat[::3], 1)
    chans = list(flat)
    rows = helpers.sclv_tables()[L.S]
    want, _un = _oracle(chans, 2, L.S, L.h, L.mode, rows)
    for blocked in (True, False):
        m = _measure_packed(mh, chans, 2, L.S, L.h, L.mode, rows, blocked)
        _check(m, want, ("b", blocked))


@pytest.mark.parametrize("h", (6, 13))
@pytest.mark.parametrize("bits,S", WIDTHS)
def test_packed_measure_is_bit_identical_to_the_byte_path(mh, bits, S, h):
    rng = np.random.RandomState(50 * bits + S + h)
    chans = _channels(rng, LENS + (100003,))
    rows = helpers.sclv_tables()[S]
    un = [np.minimum(x, (1 << bits) - 1) for x in chans]
    data, off, ln = OC.flatten(un)
    plan = mh.codec.Plan(off, ln, S, h, 1, mh.WIN_FULL, rows, seg_chunks=1)
    mb = plan.measure(torch.from_numpy(data).cuda())
    mp = _measure_packed(mh, chans, bits, S, h, 1, rows, True)
    torch.cuda.synchronize()
    plan.close()
    for f in FIELDS:
        assert torch.equal(getattr(mb, f), getattr(mp, f)), (bits, S, h, f)


@pytest.mark.parametrize("bits,S", ((2, 3), (4, 5)))
def test_packed_measure_keeps_the_asynchronous_contract(mh, bits, S):
    """Stream order on a non-blocking side stream, a captured measure replayed on changed input, and
    measure / preset encode / measure on the same buffers (the process keeps its default of at least 4 queues)."""
    h, mode = 6, 1
    rows = helpers.sclv_tables()[S]
    wants, images = [], []
    # the same lengths in every dataset (one plan): rotate the RATES, not the lengths
    sets = [[np.minimum(np.random.RandomState(17 * k + i).poisson((0.2, 1.0, 3.0)[(i + k) % 3], size=T), 255).astype(np.uint8)
             for i, T in enumerate(LENS)] for k in range(3)]
    for chans in sets:
        buf, off, stride = _place(chans, bits, True)
        images.append(torch.from_numpy(buf).pin_memory())
        wants.append(_oracle(chans, bits, S, h, mode, rows)[0])
    ln = np.array(LENS, np.uint64)
    plan = mh.codec.Plan(off, ln, S, h, mode, mh.WIN_FULL, rows, seg_chunks=1, input_bits=bits, chunk_stride=stride)
    dev = torch.zeros(len(images[0]), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        # stream order: dataset 0 dirties every scratch word, dataset 1 follows on the same buffers without a sync
        dev.copy_(images[0], non_blocking=True)
        m = plan.measure(dev)
        dev.copy_(images[1], non_blocking=True)
        plan.measure(dev, out=m)
    side.synchronize()
    _check(m, wants[1], "stream order")
    # graph capture: one measure, replayed on two other inputs
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.measure(dev, out=m)
    for k in (2, 0):
        with torch.cuda.stream(side):
            dev.copy_(images[k], non_blocking=True)
            for f in FIELDS:
                getattr(m, f).fill_(77)
            g.replay()
        side.synchronize()
        _check(m, wants[k], ("replay", k))
    # measure, preset encode, measure: the plan's scratch is shared and must come back clean
    with torch.cuda.stream(side):
        m1 = plan.measure(dev)
        e = plan.encode(dev, preset=(m1.peak, m1.enc))
        m2 = plan.measure(dev)
        m3 = plan.measure(dev)
    side.synchronize()
    for mm in (m1, m2, m3):
        _check(mm, wants[0], "mixed sequence")
    un = [np.minimum(x, (1 << bits) - 1) for x in sets[0]]
    data, o8, l8 = OC.flatten(un)
    ref = OC.encode_preset(data, o8, l8, OC.Params(S, h, mode, 3, rows, 1), wants[0]["peak"], wants[0]["enc"], nthreads=NT)
    assert np.array_equal(e.ch_bits.cpu().numpy().astype(np.uint64), ref["ch_bits"])
    assert np.array_equal(e.ch_bits.cpu().numpy().astype(np.uint64), wants[0]["bits"])  # the word is the window's own
    plan.close()


def _stream_blocks(S, C, Tb, seed):
    """Calibration block, a block of the same statistics, one whose rates are swapped on `swapped`, and a later block of
    the swapped statistics.  Quiet channels peak at 0, busy ones at 2; the swap exchanges the two kinds."""
    rng = np.random.RandomState(seed)
    lam = np.where(np.arange(C) % 2 == 0, 0.2, 2.6)
    swapped = np.array([1, 2, C - 1])
    lam2 = lam.copy()
    lam2[swapped] = np.where(lam[swapped] < 1, 2.6, 0.2)
    draw = lambda l: np.minimum(rng.poisson(l, size=(Tb, C)), 255).astype(np.uint8)  # noqa: E731
    return draw(lam), draw(lam), draw(lam2), draw(lam2), swapped


def _oracle_tm(block, S, h, mode, rows, sc, word=None):
    """oracle over a time-major block: measure (fresh calibration) or encode_preset under `word`"""
    chans = [np.ascontiguousarray(block[:, c]) for c in range(block.shape[1])]
    data, off, ln = OC.flatten(chans)
    p = OC.Params(S, h, mode, 3, rows, sc)
    if word is None:
        return OC.measure(data, off, ln, p, nthreads=NT)
    return OC.encode_preset(data, off, ln, p, word[0], word[1], nthreads=NT)


@pytest.mark.parametrize("S", (3, 5))
def test_stream_encoder_tracks_drift_and_adopts(mh, S):
    C, Tb, h, sc = 10, 40000, 6, 2
    rows = helpers.sclv_tables()[S]
    cal, same, drifted, later, swapped = _stream_blocks(S, C, Tb, 300 + S)
    se = mh.stream.StreamEncoder(C, S, h, rows, seg_chunks=sc)
    plain = mh.stream.StreamEncoder(C, S, h, rows, seg_chunks=sc)   # never tracks
    se.calibrate(cal)
    plain.calibrate(cal)
    stale = (se.peak.cpu().numpy().copy(), se.enc.cpu().numpy().copy())

    def snapshot(enc_, block, **kw):
        dense, tot, slot = enc_.encode_block_device(block, **kw)
        torch.cuda.synchronize()
        n = int(tot.item())
        e = slot["enc"]
        return (dense.payload[:n].cpu().numpy().copy(), e.seg_words.cpu().numpy().copy(), e.ch_bits.cpu().numpy().copy(),
                e.payload.cpu().numpy().copy(), slot)

    # track=False is the old path: byte-identical to an encoder that never tracks; so is the stream of a tracked block
    for block, kw in ((same, {}), (drifted, dict(track=True))):
        a, b = snapshot(se, block, **kw), snapshot(plain, block)
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x, y)
    slot = a[4]
    ch_bits = a[2]
    fresh = slot["fresh"]
    # the fresh word is what a new calibration on this block gives
    again = mh.stream.StreamEncoder(C, S, h, rows, seg_chunks=sc)
    pk, en = again.calibrate(drifted)
    assert torch.equal(fresh.peak, pk) and torch.equal(fresh.enc, en)
    want = _oracle_tm(drifted, S, h, 1, rows, sc)
    assert np.array_equal(fresh.peak.cpu().numpy(), want["peak"]) and np.array_equal(fresh.enc.cpu().numpy(), want["enc"])
    assert np.array_equal(ch_bits.astype(np.uint64), _oracle_tm(drifted, S, h, 1, rows, sc, stale)["ch_bits"])
    drift = se.drift(slot).cpu().numpy()
    assert np.array_equal(drift, ch_bits.astype(np.int64) - want["bits"].astype(np.int64))
    print("drift per channel:", drift.tolist())
    assert (drift[swapped] > 0).all(), drift
    # adopt: on the device, in place, from the next block on
    peak_t, enc_t = se.peak, se.enc
    take = se.adopt(slot)
    torch.cuda.synchronize()
    take = take.cpu().numpy()
    assert np.array_equal(take, drift >= 1) and take[swapped].all()
    assert se.peak is peak_t and se.enc is enc_t
    word = (np.where(take, want["peak"], stale[0]).astype(np.uint8), np.where(take, want["enc"], stale[1]).astype(np.uint8))
    assert np.array_equal(se.peak.cpu().numpy(), word[0]) and np.array_equal(se.enc.cpu().numpy(), word[1])
    a, b = snapshot(se, later), snapshot(plain, later)
    ref = _oracle_tm(later, S, h, 1, rows, sc, word)
    assert np.array_equal(a[2].astype(np.uint64), ref["ch_bits"])
    assert np.array_equal(a[2][take].astype(np.uint64), _oracle_tm(later, S, h, 1, rows, sc, (want["peak"], want["enc"]))["ch_bits"][take])
    seg = a[4]["plan"].segments()
    for s in range(len(seg["ch"])):   # untouched channels: the same words in the same slots as without tracking
        if not take[seg["ch"][s]]:
            o, n = int(seg["off"][s]), int(a[1][s])
            assert n == int(b[1][s]) and np.array_equal(a[3][o:o + n], b[3][o:o + n]), s
    assert np.array_equal(a[2][~take], b[2][~take])
    # and the block round-trips on the receiving end with the word it ships
    c = se.encode_block(later)
    assert np.array_equal(c.peak, word[0]) and np.array_equal(c.enc, word[1])
    dec = mh.stream.StreamDecoder(C, S, rows, seg_chunks=sc)
    assert np.array_equal(dec.decode_block(c), np.minimum(later, S - 1))
    for x in (se, plain, again, dec):
        x.close()
