"""Indices of the codec (libmuahuff) that pass 2^32 because ONE channel, or its payload, is that long -- tests/far_offsets.py
crosses 2^32 in offset and stride arguments, tests/big_inputs.py in the ingest kernels; here a per-channel count, a bit total,
a seg_first, a tile_start, a sample index t, a re-bin bin, a RangeTask::dst and a dense offset the scan computed.  One
table, two users: tests/test_host_big_codec.py (no GPU: the closed forms at a small crossing point against brute-force
NumPy and the CPU oracle, the plans and work lists at full length through tests/planner_check.cpp, the no-fault rule) and
tests/test_gpu_big_codec.py (the calls themselves).

The rules, as in big_inputs.py:

  pattern   every long input is a pattern of period P = 4099 (prime; FAR mod P != 0 for FAR = 2^16 and 2^32, so sample t and
            sample t - FAR sit at different phases), expanded on the device, with a few planted values on top: at FAR - 1,
            FAR, FAR + D and the last sample, and a decoy at the alias (index - FAR) of each
  expect    closed forms from the period and the planted entries (Channel.hist); everything that is an image of the input
            (decoded bytes, re-bin sums, transposes) is compared with plain torch on the device instead
  cut       Channel.cut(far): the channel as reads at index mod FAR see it
  accesses  the large buffers with their true far indices, for the no-fault rule: a true index, its unsigned cut and its
            sign-extended cut (of the index, of the byte offset and of the whole sum) lie inside the allocation; every
            large buffer starts LEAD = 2^31 bytes (2^31 words where it is indexed in words past 2^31) inside its
            allocation, canary in front

Nothing here calls the library under test."""
from collections import namedtuple

import numpy as np

CANARY = 0xA5
CAN32 = int(np.frombuffer(bytes([CANARY]) * 4, np.int32)[0])
CAN64 = int(np.frombuffer(bytes([CANARY]) * 8, np.int64)[0])
LEAD = 1 << 31
P = 4099
D = 1037
CHUNK = 16384                # MH_CHUNK
SEG = 2 * CHUNK              # seg_chunks = 2 throughout
HDR_WORDS = 32               # MH_HDR_WORDS
HIST_TILE = 256 * 16 * 32    # mh_planner.hpp: kHistTileBytes
FULL = 1 << 32
T_LONG = 3 * (1 << 31) + P   # 6 442 455 043

Access = namedtuple("Access", "buf elem lead body base idx")       # lead, body, base in bytes; idx: element indices from `base`


def up(x, a):
    return (x + a - 1) // a * a


def t_long(far):
    return far + far // 2 + P


def slot_words(n, maxlen):
    """mh_planner.hpp slot_words, restated"""
    full, rem = divmod(n, CHUNK)
    words = (full + (1 if rem else 0)) * HDR_WORDS + full * ((CHUNK * maxlen + 31) // 32)
    if rem:
        words += (rem * maxlen + 31) // 32
    return up(words, 32)


# ---- the channels ---------------------------------------------------------------------------------------------------------
def sparse_pattern(S):
    """at least 70 % zeros, the rest spread over 1 .. S + 2 (so S - 1, S, S + 1 and S + 2 all clip to S - 1)"""
    rng = np.random.RandomState(100 + S)
    pat = np.zeros(P, np.uint8)
    k = rng.rand(P) >= 0.75
    pat[k] = rng.randint(1, S + 3, size=int(k.sum()))
    assert (pat == 0).mean() >= 0.7 and set(range(S + 3)) <= set(pat.tolist())
    return pat


def drifted_pattern():
    """symbols 6 .. 9 only, with a few 0s and 255s: far from what 64 leading zeros calibrate for (S = 10)"""
    rng = np.random.RandomState(77)
    pat = rng.randint(6, 10, size=P).astype(np.uint8)
    pat[rng.choice(P, 12, replace=False)] = 0
    pat[rng.choice(P, 7, replace=False)] = 255
    return pat


class Channel:
    """x[t] = planted[t], else head value for t < head count, else period[t % P]; 0 <= t < n"""

    def __init__(self, n, period, head=(0, 0), planted=()):
        self.n, self.period, self.head, self.planted = int(n), np.ascontiguousarray(period, np.uint8), head, sorted(planted)
        assert self.period.size == P and len({i for i, _v in self.planted}) == len(self.planted)
        assert all(head[0] <= i < self.n for i, _v in self.planted)
        onehot = np.zeros((P + 1, 256), np.int64)
        onehot[np.arange(1, P + 1), self.period] = 1
        self._cum = np.cumsum(onehot, 0)                         # _cum[k] = counts of period[:k]

    def _pattern_counts(self, a, b):
        at = lambda x: (x // P) * self._cum[P] + self._cum[x % P]          # noqa: E731
        return at(b) - at(a)

    def at(self, t):
        """the values at the indices t (any shape)"""
        t = np.asarray(t, np.int64)
        out = np.where(t < self.head[0], self.head[1], self.period[t % P]).astype(np.uint8)
        for i, v in self.planted:
            out = np.where(t == i, v, out).astype(np.uint8)
        return out

    def hist(self, a, b, lim=256):
        """int64 [lim] counts of min(x, lim - 1) over a <= t < b, in closed form"""
        a, b = min(a, self.n), min(b, self.n)
        h = np.zeros(256, np.int64)
        if b > a:
            h += self._pattern_counts(a, b)
            hb = min(b, self.head[0])
            if hb > a:
                h -= self._pattern_counts(a, hb)
                h[self.head[1]] += hb - a
            for i, v in self.planted:
                if a <= i < b:
                    h[int(self.period[i % P])] -= 1
                    h[v] += 1
        out = h[:lim].copy()
        out[lim - 1] += h[lim:].sum()
        return out

    def dense(self):
        """brute force: the whole channel (host tests, small n)"""
        x = self.period[np.arange(self.n) % P].copy()
        x[:self.head[0]] = self.head[1]
        for i, v in self.planted:
            x[i] = v
        return x

    def cut(self, far):
        """the channel as reads at t mod FAR see it (small n)"""
        x = self.dense()
        return x[np.arange(self.n) % far]


def planted(far, n, values):
    """(index, value): FAR - 1, FAR, FAR + D, the last sample, one in the middle, and a decoy at the alias of each but
    FAR's own (index 0 belongs to the calibration head) -- `values` in that order, 8 of them"""
    idx = [far - 1, far, far + D, n - 1, far // 2 + 11, D, n - 1 - far, 2 * D]
    assert len(set(idx)) == 8 and far + D < n - 1 and 64 <= n - 1 - far < far - 1 and len(values) == 8
    return list(zip(idx, values))


def sparse_channels(S, far):
    """three channels: 70 001 samples, the long one, 40 000 -- the short ones are the same pattern at other phases"""
    pat = sparse_pattern(S)
    n = t_long(far)
    long_ = Channel(n, pat, planted=planted(far, n, [255, S + 1, 1, S, 255, 255, 0, S - 1]))
    return [Channel(70001, np.roll(pat, -17)), long_, Channel(40000, np.roll(pat, -34), planted=[(39999, 255)])]


def drifted_channels(far):
    """the long channel: 64 zeros (calibration at h = 6 picks peak 0), then symbols 6 .. 9 with a few 0s and 255s"""
    n = t_long(far)
    pat = sparse_pattern(10)
    long_ = Channel(n, drifted_pattern(), head=(64, 0), planted=planted(far, n, [255, 6, 3, 9, 255, 5, 255, 0]))
    return [Channel(70001, np.roll(pat, -17)), long_, Channel(40000, np.roll(pat, -34), planted=[(39999, 255)])]


FILLINGS = {"sparse-S3": (3, lambda far: sparse_channels(3, far)), "sparse-S10": (10, lambda far: sparse_channels(10, far)),
            "drifted-S10": (10, drifted_channels)}


def decoys_tell(ch, far):
    """every planted sample behind FAR differs from the sample at its alias"""
    return all(v != int(ch.at(i - far)) for i, v in ch.planted if i >= far)


def layout_a(chs):
    """byte offsets of the three channels in one buffer: 128-byte aligned, at least 128 canary bytes between them, and
    the body size (canary behind the last one too)"""
    off, cur = [], 0
    for c in chs:
        off.append(cur)
        cur = up(cur + c.n + 128, 128)
    return off, cur


# ---- what mh_measure computes, restated -------------------------------------------------------------------------------------
def window(T, h, win_after_cal):
    """(cutoff, w0, w1) of mh_planner.hpp channel_window for MH_WIN_FULL / MH_WIN_AFTER_CAL"""
    cut = min(T, 1 << h)
    return (cut, cut, T) if win_after_cal else (cut, 0, T)


def measure_ref(cal_counts, win_counts, tab, rule):
    """cal_counts, win_counts: int64 [S] counts of min(x, S - 1) over the calibration window and the coding window;
    tab: uint8 [K, S]; rule(S, peak) -> the symbol at each rank (oracle approx_sort_rule).
    -> peak (the first maximum), enc (the first minimum of table . rank-ordered counts), the two histograms in rank order,
    bits, and the code length of each SYMBOL"""
    S = len(cal_counts)
    peak = int(np.argmax(cal_counts))
    idx = np.asarray(rule(S, peak), np.int64)
    cal_sorted, post = np.asarray(cal_counts, np.int64)[idx], np.asarray(win_counts, np.int64)[idx]
    cost = tab.astype(np.int64) @ cal_sorted
    enc = int(np.argmin(cost))
    lens = np.zeros(S, np.int64)
    lens[idx] = tab[enc]
    return dict(peak=peak, enc=enc, cal_hist=cal_sorted, post_hist=post, bits=int(tab[enc].astype(np.int64) @ post), lens=lens)


def expect_measure(chs, S, h, win_after_cal, tab, rule):
    out = []
    for c in chs:
        cut, w0, w1 = window(c.n, h, win_after_cal)
        m = measure_ref(c.hist(0, cut, S), c.hist(w0, w1, S), tab, rule)
        m.update(cutoff=cut, w0=w0, w1=w1)
        out.append(m)
    return out


def segments_of(T):
    """(first, n) of a channel's segments under a whole-channel window that starts on a 128-sample boundary"""
    return [(f, min(SEG, T - f)) for f in range(0, T, SEG)]


def oracle_segments(far, T):
    """the segments the CPU oracle runs on: the first, the one that ends at FAR (it holds the planted FAR - 1), the one that
    starts there, and the last (a partial one)"""
    nseg = -(-T // SEG)
    assert far % SEG == 0 and T % SEG != 0
    return [0, far // SEG - 1, far // SEG, nseg - 1]


# ---- case A: memory, accesses -----------------------------------------------------------------------------------------------
def case_a(name, far, maxlen):
    S, make = FILLINGS[name]
    chs = make(far)
    off, body = layout_a(chs)
    T = chs[1].n
    nseg = sum(-(-c.n // SEG) for c in chs)
    cap = sum(slot_words(n, maxlen) for c in chs for _f, n in segments_of(c.n)) + 4
    slot1 = sum(slot_words(n, maxlen) for _f, n in segments_of(chs[0].n))        # the long channel's first slot
    last_slot = cap - 4 - sum(slot_words(n, maxlen) for _f, n in segments_of(chs[2].n)) - slot_words(T % SEG, maxlen)
    far_t = [far - 1, far, far + D, T - 1]
    acc = [Access("x", 1, LEAD, body, off[1], far_t), Access("x third channel", 1, LEAD, body, off[2], [0, chs[2].n - 1]),
           Access("decoded", 1, LEAD, body, off[1], far_t), Access("decoded third channel", 1, LEAD, body, off[2], [0, chs[2].n - 1]),
           Access("slotted payload", 4, LEAD, 4 * cap, 0, [slot1, last_slot, cap - 5]),
           Access("dense payload", 4, LEAD, 4 * cap, 0, [slot1, last_slot, cap - 5]),     # (dense offsets are below the slots')
           Access("range row", 1, LEAD, T + 128, 0, far_t)]
    for r, elem in ((2, 1), (17, 4), (17, 1), (68, 4), (68, 1), (100, 4)):
        nb = -(-T // r)
        acc.append(Access("rebin r=%d out, %d-byte" % (r, elem), elem, LEAD, elem * (nb + 64), 0, [(far - 1) // r, far // r, nb - 1]))
    # x + slotted payload + dense copy + decoded image, each behind its lead, + slabs of the torch references
    peak = 4 * LEAD + 2 * body + 2 * 4 * cap + (3 << 30)
    return dict(S=S, chs=chs, off=off, body=body, T=T, nseg=nseg, cap=cap, accesses=acc, peak=peak, lens=[c.n for c in chs])


# ---- case B: mh_compact past 2^32 words -------------------------------------------------------------------------------------
B_MAXLEN, B_TAIL = 9, 12345


def case_b(far):
    """A plan only: C channels of nfull whole segments and one of B_TAIL samples, S = 10 (maxlen 9), so that the slotted
    payload exceeds FAR + FAR / 64 words; seg_words = capacity - randint(0, 32), the first three and the last at capacity,
    about a hundred zeros, two of them next to the crossing of the destinations"""
    C = 512 if far == FULL else 4
    full, tail = slot_words(SEG, B_MAXLEN), slot_words(B_TAIL, B_MAXLEN)
    nfull = 1
    while C * (nfull * full + tail) <= far + (far // 64 if far == FULL else far // 2):     # (a few segments behind the small crossing)
        nfull += 1
    per = nfull + 1
    T = nfull * SEG + B_TAIL
    cap = np.tile(np.array([full] * nfull + [tail], np.int64), C)
    nseg = cap.size
    slot_off = np.cumsum(cap) - cap
    rng = np.random.RandomState(5)
    sw = cap - rng.randint(0, 33, size=nseg)
    sw[:3], sw[-1] = cap[:3], cap[-1]
    zeros = rng.choice(np.arange(3, nseg - 1), min(100, nseg // 8), replace=False)
    sw[zeros] = 0
    while True:                                              # zeros on both sides of the segment whose words straddle
        k = int(np.searchsorted(np.cumsum(sw), far, side="right"))      # destination word FAR (a zero in front moves it)
        assert 3 < k < nseg - 2
        if sw[k - 1] == 0 and sw[k + 1] == 0:
            break
        sw[k - 1] = sw[k + 1] = 0
    dense_off = np.cumsum(sw) - sw
    total = int(sw.sum())
    payload_words = int(cap.sum()) + 4
    assert payload_words - 4 > far + far // 64 and total > far + far // 256
    acc = [Access("slotted payload", 4, 4 * LEAD, 4 * payload_words, 0, [0, int(slot_off[k]), int(slot_off[-1]), payload_words - 5]),
           Access("dense", 4, 4 * LEAD, 4 * (total + 64), 0, [0, far // 4, far - 1, far, total - 1])]
    peak = 8 * LEAD + 4 * payload_words + 4 * (total + 64) + 16 * nseg * 4 + (6 << 30)
    return dict(C=C, T=T, nfull=nfull, per=per, nseg=nseg, cap=cap, slot_off=slot_off, seg_words=sw, dense_off=dense_off, total=total,
                payload_words=payload_words, cross=k, accesses=acc, peak=peak, n_zero=int((sw == 0).sum()))


def payload_word(i):
    """the word at payload index i (int64 array) as an unsigned value: not cyclic in 2^32 -- word i + 2^32 is word i + 4096"""
    i = np.asarray(i, np.int64)
    return (i * 40503 + (i >> 20)) & 0xFFFFFFFF


def compact_model(payload, slot_off, seg_words, far=None):
    """brute force mh_compact: (dense, dense_off); with `far` the destinations are taken modulo FAR (the later store wins)"""
    dense_off = np.cumsum(seg_words) - seg_words
    total = int(seg_words.sum())
    out = np.full(total, -1, np.int64)
    for s in range(len(seg_words)):
        n, d0 = int(seg_words[s]), int(dense_off[s])
        dst = d0 + np.arange(n)
        out[dst % far if far else dst] = payload[int(slot_off[s]):int(slot_off[s]) + n]
    return out, dense_off


# ---- case C: the layout calls with T >= 2^32 --------------------------------------------------------------------------------
C_CH = 3


def case_c(far):
    """time-major [T, 3], T = FAR + P: x[t, c] = pattern[(t + 17 c) mod P] with planted rows"""
    T = far + P
    pat = sparse_pattern(10)
    chs = []
    for c in range(C_CH):
        per = np.roll(pat, -17 * c)
        at_far = 11 if per[0] != 11 else 12                  # sample FAR differs from sample 0, its alias
        chs.append(Channel(T, per, planted=planted(far, T, [255, at_far, 1 + c, 10, 255, 255 - c, 0, 9])))
    pitch = up(T + 128, 128)
    far_t = [far - 1, far, far + D, T - 1]
    acc = [Access("x", 1, LEAD, C_CH * T, c, [C_CH * t for t in far_t]) for c in range(C_CH)]
    acc += [Access("channel-major", 1, LEAD, C_CH * pitch, c * pitch, far_t) for c in range(C_CH)]
    acc += [Access("time-major again", 1, LEAD, C_CH * T, c, [C_CH * t for t in far_t]) for c in range(C_CH)]
    peak = 3 * LEAD + 2 * C_CH * T + C_CH * pitch + (3 << 30)
    return dict(T=T, chs=chs, pitch=pitch, accesses=acc, peak=peak)


def no_fault(accesses):
    """the rule of the module docstring; -> the number of true byte addresses at or behind 2^32"""
    sext = lambda v: v % FULL - (FULL if v % FULL >= 1 << 31 else 0)          # noqa: E731
    far = 0
    for a in accesses:
        for i in a.idx:
            at = a.base + i * a.elem
            cuts = {at, a.base + (i % FULL) * a.elem, a.base + sext(i) * a.elem, a.base + (i * a.elem) % FULL,
                    a.base + sext(i * a.elem), at % FULL, sext(at)}
            for c in cuts:
                assert -a.lead <= c and c + a.elem <= a.body, (a.buf, i, c)
            far += at >= FULL
    return far


Case = namedtuple("Case", "id entry crosses shape")
CASES = [
    Case("A-measure", "mh_measure (k_hist, k_hist2, the tiled calibration)", "a histogram count, `bits`, tile_start; h = 30",
         "channels of 70 001, 3 * 2^31 + 4099 and 40 000 samples; sparse S = 3 and S = 10"),
    Case("A-codec", "mh_encode, mh_decode", "ch_bits, seg_first, the slot offsets, the sample index of the stores",
         "the same; sparse S = 3, S = 10 and the drifted S = 10 filling (7.3 GB of slots)"),
    Case("A-compact", "mh_compact, mh_decode from dense offsets", "a dense offset >= 2^30 words out of k_scan_apply", "drifted S = 10"),
    Case("A-range", "mh_decode_range", "RangeTask::dst, a row longer than 2^32 bytes", "drifted S = 10, dense offsets"),
    Case("A-decode-rebin", "mh_decode_rebin", "the bin index (>= 2^26 bins), t0 next to 2^32", "drifted S = 10; r = 100 and r = 7"),
    Case("A-rebin", "mh_rebin", "b0 >= 2^31 bins (k_rebin2), the 65535-workgroup cap of k_rebin3", "the sparse S = 10 bytes; r = 2, 17, 68, 100"),
    Case("A-sweep", "mh_sweep_create, mh_sweep_run", "bounds up to T_LONG", "the sparse S = 10 bytes; hist_bits = (6, 30)"),
    Case("B-compact", "mh_compact", "seg_off[seg] and dense_off past word 2^32", "512 channels of 919 segments, 17.5 GB of slots"),
    Case("C-layout", "mh_deinterleave, mh_interleave", "the time index t >= 2^32", "[2^32 + 4099, 3] time-major"),
    Case("C-packed", "mh_deinterleave_packed, mh_interleave_packed", "t >= 2^32; j * chunk_stride past byte 2^32", "the same; 2 and 4 bits, contiguous and blocked"),
    Case("C-stream", "StreamEncoder.encode_block_device, StreamDecoder", "the packed plan, mh_encode_preset, mh_decode_packed at t >= 2^32",
         "the same; S = 3 and S = 10"),
]
