"""The time-major stream path, the packed de-interleave and the dense compaction at the sizes the project runs at,
against references that do not go through the kernels under test: plain torch ops on the device (clamp, ==, sum,
cumsum, shifts and ors, transposes) and the CPU oracle on a few whole channels copied to the host.  Inputs may come
from libmuahuff (synth.generate, pinned to the oracle by test_synth_matches_oracle); expected values never do."""
import ctypes as ct

import numpy as np
import pytest
import torch

import oracle
from tests import helpers

pytestmark = pytest.mark.gpu

OC = oracle.c
GiB = 1 << 30


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import codec, container, stream, synth  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    info = muahuff.device_info(0)
    assert "gfx950" in info["arch"], info
    return muahuff


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _need(nbytes, what):
    _free()
    free, _total = torch.cuda.mem_get_info()
    assert nbytes < free, "%s needs ~%.1f GB of free HBM; %.1f GB free" % (what, nbytes / 1e9, free / 1e9)


def _counts(x, T, C, lim, step=1 << 20):
    """[T, C] time-major counts -> int64 [C, lim] histogram of min(x, lim - 1) per channel (torch, in time slabs)"""
    h = torch.zeros((C, lim), dtype=torch.int64, device=x.device)
    for t0 in range(0, T, step):
        xc = torch.clamp(x[t0:t0 + step], max=lim - 1)
        for s in range(lim):
            h[:, s] += (xc == s).sum(0)
    return h


def _sprinkle(x, seed, frac=1e-3):
    """overwrite a sparse, seeded set of samples with counts up to 255 (far above every field and symbol range)"""
    g = torch.Generator(device=x.device).manual_seed(seed)
    n = max(1, int(x.numel() * frac))
    idx = torch.randint(0, x.numel(), (n,), generator=g, device=x.device)
    x.view(-1)[idx] = torch.randint(0, 256, (n,), generator=g, device=x.device, dtype=torch.uint8)
    x[0, :] = 255                                  # every channel sees a clipped count in its first time steps


# ------------------------------------------------------------------------------------------------------------------
# A. mh_deinterleave_packed on both sides of the cached / non-temporal store switch
# ------------------------------------------------------------------------------------------------------------------
# mh_deinterleave_packed (csrc/muahuff.hip) stores its pieces with plain stores while
#     (double)T * C * bits / 8.0 <= 192.0 * 1048576.0
# and with non-temporal stores above that (k_deinterleave_p, csrc/mh_layout.hpp).
SWITCH_BYTES = 192 * (1 << 20)


def _pack_ref(xs, bits):
    """[t, C] time-major counts -> [C, ceil(t/16) * 2 * bits] packed pieces as include/muahuff.h documents them:
    min(x, 2^bits - 1), 16 samples per piece, sample i of a piece in bits [i * bits, (i + 1) * bits) little-endian,
    the last piece zero-padded.  Torch on the device; the NumPy form is _bitpack in test_gpu_parity.py."""
    t, C = xs.shape
    npc = (t + 15) // 16
    s = torch.zeros((C, npc * 16), dtype=torch.uint8, device=xs.device)
    s[:, :t] = torch.clamp(xs, max=(1 << bits) - 1).t()
    per = 8 // bits
    g = s.view(C, npc * 16 // per, per)
    by = g[..., 0].clone()
    for f in range(1, per):
        by |= g[..., f] << (bits * f)
    return by


def _deinterleave_packed(mh, x, bits, out, off, stride):
    T, C = x.shape
    d_off = torch.from_numpy(np.asarray(off, np.int64)).to(x.device)
    mh._lib.check(mh._lib.lib().mh_deinterleave_packed(ct.c_void_p(x.data_ptr()), T, C, bits, ct.c_void_p(out.data_ptr()),
                                                       ct.c_void_p(d_off.data_ptr()), stride, None))
    torch.cuda.synchronize()


def _check_packed(mh, x, bits, blocked, slab_chunks=64):
    """Run mh_deinterleave_packed over a canary-filled buffer and compare every byte with _pack_ref, slab by slab."""
    T, C = x.shape
    pb, npiece = 2 * bits, (T + 15) // 16
    CANARY, tail = 0xEE, 256
    if blocked:                                  # chunk j of channel c at c * cb + j * C * cb (StreamEncoder._slot)
        cb = 1024 * pb
        nch = (T + 16383) // 16384
        stride = C * cb
        out = torch.full((nch * stride + tail,), CANARY, dtype=torch.uint8, device=x.device)
        _deinterleave_packed(mh, x, bits, out, np.arange(C) * cb, stride)
        blocks = out[:nch * stride].view(nch, C, cb)
        for j0 in range(0, nch, slab_chunks):
            j1 = min(nch, j0 + slab_chunks)
            ref = _pack_ref(x[j0 * 16384:j1 * 16384], bits)                  # [C, pieces of the slab * pb]
            # the kernel stores whole 16-byte items: zeros behind the last piece up to the next 16 bytes, then
            # nothing -- the rest of the last chunk keeps the canary
            want = torch.full((C, (j1 - j0) * cb), CANARY, dtype=torch.uint8, device=x.device)
            r16 = (ref.shape[1] + 15) // 16 * 16
            want[:, :r16] = 0
            want[:, :ref.shape[1]] = ref
            got = blocks[j0:j1].permute(1, 0, 2).reshape(C, -1)
            assert torch.equal(got, want), (T, C, bits, "chunks", j0, j1)
        end = nch * stride
    else:                                        # contiguous: channel c at c * pitch, pitch = its pieces on 16 bytes
        pitch = (npiece * pb + 15) // 16 * 16
        out = torch.full((C * pitch + tail,), CANARY, dtype=torch.uint8, device=x.device)
        _deinterleave_packed(mh, x, bits, out, np.arange(C) * pitch, 0)
        rows = out[:C * pitch].view(C, pitch)
        step = slab_chunks * 16384
        for t0 in range(0, T, step):
            ref = _pack_ref(x[t0:t0 + step], bits)
            p0 = t0 // 16 * pb
            assert torch.equal(rows[:, p0:p0 + ref.shape[1]], ref), (T, C, bits, t0)
        assert bool((rows[:, npiece * pb:] == 0).all()), (T, C, bits)    # the last item's zero padding
        end = C * pitch
    # the last piece's 16-byte store leaves the bytes behind it untouched
    assert bool((out[end:] == CANARY).all()), (T, C, bits, blocked)
    del out
    _free()


def _switch_cases():
    out = []
    for bits in (2, 4):
        C = 192                                   # 1.5 strips of 128 channels: a partial last strip
        T_at = SWITCH_BYTES * 8 // (bits * C)     # T * C * bits / 8 == the switch exactly
        assert T_at * C * bits // 8 == SWITCH_BYTES and (T_at * C * bits) % 8 == 0
        for T, side in ((T_at - 1, "below"), (T_at, "at"), (T_at + 1, "above")):
            for blocked in (False, True):
                out.append(pytest.param(bits, T, C, blocked, side, id="%db-%s-%s" % (bits, side, "blocked" if blocked else "contig")))
    return out


@pytest.mark.parametrize("bits,T,C,blocked,side", _switch_cases())
def test_packed_deinterleave_at_the_store_switch(mh, bits, T, C, blocked, side):
    """Every byte of the pieces, both packings and both layouts, with T * C * bits / 8 just below, exactly at and
    just above the size where the stores turn non-temporal (ragged T below and above: T % 16 != 0)."""
    size = T * C * bits / 8.0
    assert {"below": size < SWITCH_BYTES, "at": size == SWITCH_BYTES, "above": size > SWITCH_BYTES}[side]
    assert abs(size - SWITCH_BYTES) <= C * bits / 8 and C % 128 != 0
    assert side == "at" or T % 16 != 0
    g = torch.Generator(device="cuda").manual_seed(1000 * bits + T % 1000)
    x = torch.randint(0, 1 << bits, (T, C), generator=g, device="cuda", dtype=torch.uint8)
    _sprinkle(x, seed=bits + T % 97, frac=0.02)
    _check_packed(mh, x, bits, blocked)


def test_packed_deinterleave_chunk_blocked_above_4_gib(mh):
    """4-bit pieces, chunk-blocked, more than 4 GiB of them (1000 channels x 9 000 011 steps: 4.5 GB of pieces from
    9 GB of input): the 64-bit piece addressing of the stores, checked byte for byte against _pack_ref."""
    C, T, bits = 1000, 9_000_011, 4
    pieces = ((T + 16383) // 16384) * C * 1024 * 2 * bits
    assert pieces > 4 * GiB and C % 128 != 0 and T % 16 != 0
    _need(T * C + pieces + 3 * GiB, "the > 4 GiB de-interleave")
    g = torch.Generator(device="cuda").manual_seed(77)
    x = torch.randint(0, 16, (T, C), generator=g, device="cuda", dtype=torch.uint8)
    _sprinkle(x, seed=78)
    _check_packed(mh, x, bits, True, slab_chunks=32)
    del x
    _free()


# ------------------------------------------------------------------------------------------------------------------
# B. the stream path (calibrate, de-interleave to packed pieces, preset encode, compaction) at its headline shape
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,T", [(3, 1024, 10_000_000), (5, 1024, 10_000_000), (10, 1000, 5_000_011)],
                         ids=["S3-2bit-1024x1e7", "S5-4bit-1024x1e7", "S10-4bit-1000x5000011"])
def test_stream_path_at_full_size(mh, S, C, T):
    from muahuff import MODE_APPROX, WIN_FULL, codec, stream, synth
    from muahuff.container import ChannelSet
    bits = 2 if S <= 4 else 4
    tab = helpers.sclv_tables()[S]
    maxlen = int(tab.max())
    # x, then the encoder's slot (pieces, slotted payload, dense copy); later x + decoded set + interleaved copy
    _need(T * C * max(1 + bits / 8 + 2 * maxlen / 8 + 0.25, 3.25) + 4 * GiB, "the full-size stream block")
    cs = synth.generate(C, T, seed=S)
    x = cs.matrix().t().contiguous()                                   # [T, C] time-major
    del cs
    _free()
    _sprinkle(x, seed=100 + S)
    assert x.shape == (T, C) and x.numel() > 4 * GiB
    # --- calibration: the RAM word equals the oracle's on the same 64 steps
    se = stream.StreamEncoder(C, S, 6, tab)
    peak, enc = (t.cpu().numpy() for t in se.calibrate(x[:64]))
    first = x[:64].cpu().numpy()
    data, off, ln = OC.flatten([first[:, c].copy() for c in range(C)])
    om = OC.measure(data, off, ln, OC.Params(S, 6, 1, OC.WIN_FULL, tab))
    assert np.array_equal(peak, om["peak"]) and np.array_equal(enc, om["enc"])
    # --- the block
    dense, tot, slot = se.encode_block_device(x)
    torch.cuda.synchronize()
    plan_p = slot["plan"]
    nseg = plan_p.n_segments
    seg_p = plan_p.segments()
    assert plan_p.input_bits == bits
    # the encoder's own slot offsets: with 4-bit pieces the slotted payload is longer than 4 GiB and the last segments'
    # slots begin behind byte 2^32 (word 2^30).  With S = 3 -- at most 2 bits a sample -- it is 0.61 of that: no crossing
    if bits == 4:
        assert int(seg_p["off"][-1]) >= 1 << 30 and plan_p.payload_cap_words * 4 > 1 << 32
    sw = dense.seg_words[:nseg]
    assert int(tot[0]) == int(sw.sum())
    assert torch.equal(dense.seg_off[:nseg], torch.cumsum(sw, 0) - sw)
    # --- bits: ch_bits[c] == sum_s count_c(s) * tab[enc[c]][rank_c(s)], every channel
    counts = _counts(x, T, C, S).cpu().numpy()
    assert int(counts.sum()) == T * C
    lens = np.zeros((C, S), np.int64)
    for c in range(C):
        rank_of = np.argsort(OC.approx_sort_rule(S, int(peak[c])))
        lens[c] = tab[enc[c]][rank_of]
    assert np.array_equal(dense.ch_bits.cpu().numpy(), (counts * lens).sum(1))
    seg_words = sw.clone()
    ch_bits, skipped = dense.ch_bits.clone(), dense.skipped.clone()
    dense_pay, dense_off = dense.payload, dense.seg_off[:nseg].clone()
    total = int(tot[0])
    del dense, tot, slot, sw
    se.close()                                                          # frees the pieces and the slotted payload
    _free()
    # --- the dense stream decoded on the device with a plain byte-layout plan (as container_io.decompress does)
    out = ChannelSet.empty([T] * C)
    plan_d = codec.Plan(out.ch_off, out.ch_len, S, 0, MODE_APPROX, WIN_FULL, tab, seg_chunks=plan_p.seg_chunks)
    assert plan_d.n_segments == nseg
    seg_d = plan_d.segments()
    for k in ("ch", "first", "n"):
        assert np.array_equal(seg_d[k], seg_p[k]), k
    plan_p.close()
    e = codec.Encoded(dense_pay, seg_words, ch_bits, torch.from_numpy(peak).cuda(), torch.from_numpy(enc).cuda(),
                      skipped, dense_off, True)
    plan_d.decode(e, out.data)
    assert plan_d.decode_ok()
    step = 1 << 20
    mat = out.matrix()
    for t0 in range(0, T, step):
        assert torch.equal(mat[:, t0:t0 + step], torch.clamp(x[t0:t0 + step], max=S - 1).t()), t0
    # --- the oracle's decoder on the GPU's bytes: channels 0, C/2, C-1 moved into the oracle's slot layout
    p1 = OC.Params(S, 0, 1, OC.WIN_FULL, tab, seg_chunks=plan_p.seg_chunks)
    seg1 = OC.plan_segments(np.array([T], np.uint64), p1)
    cap1 = np.diff(np.append(seg1["off"], np.uint64(seg1["cap_words"]))).astype(np.int64)
    doff, dsw = dense_off.cpu().numpy(), seg_words.cpu().numpy()
    for c in (0, C // 2, C - 1):
        idx = np.nonzero(seg_p["ch"] == c)[0]
        assert len(idx) == len(seg1["ch"]) and np.array_equal(seg_p["n"][idx], seg1["n"])
        pay = np.zeros(seg1["cap_words"] + 4, np.uint32)
        lo, hi = int(doff[idx[0]]), int(doff[idx[-1]] + dsw[idx[-1]])
        words = dense_pay[lo:hi].cpu().numpy().view(np.uint32)
        for k, s in enumerate(idx):
            o, n = int(doff[s]) - lo, int(dsw[s])
            assert n <= cap1[k], (c, k)
            pay[int(seg1["off"][k]):int(seg1["off"][k]) + n] = words[o:o + n]
        got = OC.decode(pay, np.zeros(1, np.uint64), np.array([T], np.uint64), p1, peak[c:c + 1], enc[c:c + 1], T)
        assert np.array_equal(got, np.minimum(x[:, c].cpu().numpy(), S - 1)), c
    assert total == int(dsw.sum())
    plan_d.close()
    del e, dense_pay, mat
    _free()
    # --- back to time-major (mh_interleave, above 4 GiB of output for the 1e7-step blocks)
    tm = out.to_time_major()
    for t0 in range(0, T, step):
        assert torch.equal(tm[t0:t0 + step], torch.clamp(x[t0:t0 + step], max=S - 1)), t0
    del tm, out, x
    _free()


# ------------------------------------------------------------------------------------------------------------------
# D. mh_compact in all three of its scan regimes
# ------------------------------------------------------------------------------------------------------------------
# csrc/muahuff.hip mh_compact: <= kScanBlock (2048) segments -> one self-scanning launch; more -> block sums,
# k_scan_top over the block sums (one per thread up to 1024 blocks = 2048 * 1024 segments, several per thread above)
# and the in-block scan.
@pytest.mark.parametrize("nseg", [1500, 2048, 2049, 300_000, 2048 * 1024, 2048 * 1024 + 1, 2_200_000])
def test_compaction_scan_regimes(mh, nseg):
    from muahuff import MODE_APPROX, WIN_FULL, codec
    from muahuff.container import layout
    S, T = 3, 16                                  # one 16-sample segment per channel
    tab = helpers.sclv_tables()[S]
    off, ln, _total = layout([T] * nseg)
    plan = codec.Plan(off, ln, S, 0, MODE_APPROX, WIN_FULL, tab, seg_chunks=1)
    assert plan.n_segments == nseg
    seg = plan.segments()
    cap = np.diff(np.append(seg["off"], np.uint64(plan.payload_cap_words - 4))).astype(np.int64)
    assert cap.min() > 0
    rng = np.random.RandomState(nseg % 100003)
    sw = rng.randint(0, cap + 1).astype(np.int64)           # anything up to the slot's capacity, zeros included
    sw[:3] = cap[:3]
    sw[-1] = cap[-1]
    g = torch.Generator(device="cuda").manual_seed(nseg)
    payload = torch.randint(-2 ** 31, 2 ** 31 - 1, (plan.payload_cap_words,), generator=g, device="cuda", dtype=torch.int32)
    d_sw = torch.from_numpy(sw).cuda()
    want_off = torch.cumsum(d_sw, 0) - d_sw
    total = int(sw.sum())
    CANARY = -0x11111112
    dense = torch.full((total + 64,), CANARY, dtype=torch.int32, device="cuda")
    d_off = torch.full((nseg,), -1, dtype=torch.int64, device="cuda")
    d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    e = codec.Encoded(payload, d_sw, None, None, None, None)
    d, tot = plan.compact(e, dense=dense, off=d_off, tot=d_tot)
    torch.cuda.synchronize()
    assert int(tot[0]) == total
    assert torch.equal(d.seg_off, want_off)
    # every word of every segment, from torch slices of the payload
    seg_id = torch.repeat_interleave(torch.arange(nseg, device="cuda"), d_sw)
    slot_off = torch.from_numpy(seg["off"].astype(np.int64)).cuda()
    src = slot_off[seg_id] + torch.arange(total, device="cuda") - want_off[seg_id]
    assert torch.equal(dense[:total], payload[src])
    assert bool((dense[total:] == CANARY).all())
    plan.close()
    del payload, dense, seg_id, src
    _free()
