"""Segments that mix staged and oversize chunks (a plain module, not a conftest): the data of
tests/test_host_mixed_chunks.py and tests/test_gpu_mixed_chunks.py.

Every codec kernel has two routes per 16384-sample chunk.  The encoders stage codewords in LDS and carry a tail of up
to 63 words (`pend`) to the next chunk, unless a sub-stream outgrows the staging (32 dwords = 1024 bits, code class
LC >= 2 only): that chunk takes the global two-pass routine, after the carried tail has been written with plain stores,
and leaves the output pointer off its 256-byte grid.  The decoders pipeline chunks through LDS while payload words + 3
fit 64 * NR words; the first chunk that does not ends the pipeline and the rest of the segment, chunks that would have
fitted included, goes symbol by symbol.  The one-symbol wave rung (NR = 36) decodes chunks in pairs and falls back to
single chunks when a pair does not fit.  The scenarios here put both routes into ONE segment, on every side of every
switch.

Settings of every scenario: MH_MODE_NOSORT, one SCLV row (K = 1), MH_WIN_FULL, h = 0.  The code length of a sample is
then row[min(x, S - 1)] whatever the calibration yields, and chunk c of a channel is its samples [c * 16384, ...).

A chunk is written as a token, a segment as tokens separated by blanks, a channel as a tuple of segments:

  Q     quiet: rng.random_sample(n) < 0.1
  M     1, 2 alternating (two of them exceed the pair budget of NR = 36, one alone stages)
  L     loud: the last symbol everywhere -- oversize for every rung that can overflow
  s     zeros, sub-stream 5 (samples with (i >> 4) & 63 == 5) all 3: the longest sub-stream is 1024 bits, the last
        chunk an LC >= 2 encoder stages
  s+    as s, one of those samples 4: 1025 bits, the first chunk such an encoder sends down its slow path
  bNR-  payload words + 3 == 64 * NR: the last chunk the rung NR stages
  bNR+  one word more
  l m   tails of loud samples: an oversize and a staged partial chunk
  q100 q15   quiet tails of 100 and of 15 samples

CLASSES gives, per row, what each token claims: payload words (nw, exact or a range), the longest sub-stream in bits
where the encoder's switch depends on it, and its length when it is a tail.  Nothing here is computed by the code
under test: tests/test_host_mixed_chunks.py checks the claims on the CPU oracle's stream with chunk_words().
"""
import functools
import types
import zlib
from dataclasses import dataclass

import numpy as np

from tests import kernel_cells as kc

CHUNK = kc.CHUNK
ENC_STAGE_BITS = 1024        # enc_stage_dw(maxlen >= 3) = 32 dwords per sub-stream (csrc/mh_select.hpp)

ROWS = {
    "10_9": kc.R[(10, 9)][0],     # [1,2,3,4,5,6,7,8,9,9]: hybrid workgroup rung NR = 31, one-symbol wave rung NR = 36, LC 3
    "10_4": kc.R[(10, 4)][0],     # [2,2,4,4,4,4,4,4,4,4]: NR = 32 in both task forms, LC 1 (never overflows)
    "6_5": kc.R[(6, 5)][0],       # [1,2,3,4,5,5]: non-hybrid workgroup rung NR = 32 (wave: NR = 36), LC 2
    "9_8": kc.R[(9, 8)][0],       # [1,2,3,4,5,6,7,8,8]: the decoders of 10_9; the LC 2 encoder with 4-bit pair indices (S = 9)
}


@dataclass(frozen=True)
class Klass:
    nw: tuple            # (lo, hi) payload words the token claims, inclusive
    longest: int = -1    # longest sub-stream in bits, -1: not claimed (any value on the staged side of the encoder)
    n: int = CHUNK       # samples (a tail when < CHUNK)


def _k(nw, longest=-1, n=CHUNK):
    return Klass((nw, nw) if isinstance(nw, int) else nw, longest, n)


CLASSES = {
    "10_9": {
        "Q": _k((520, 620)), "M": _k(1280, 640), "L": _k(4608, 2304), "s": _k(536, 1024), "s+": _k(537, 1025),
        "b31-": _k(1981), "b31+": _k(1982), "b36-": _k(2301), "b36+": _k(2302),
        "l": _k(2532, n=9000), "m": _k(1407, n=5000), "q100": _k((4, 8), n=100), "q15": _k((1, 2), n=15),
    },
    "10_4": {
        "Q": _k(1024, 512), "L": _k(2048, 1024), "b32-": _k(2045), "b32+": _k(2046),
        # a tail of 4-bit codes is oversize for NR = 32 only from 16361 samples on: (2045 * 32 + 1) / 4
        "l": _k(2048, n=16380), "m": _k(625, n=5000), "q100": _k(7, n=100), "q15": _k(1, n=15),
    },
    "6_5": {
        "Q": _k((520, 620)), "L": _k(2560, 1280), "s": _k(536, 1024), "s+": _k(537, 1025),
        "l": _k(2500, n=16000), "m": _k(782, n=5000), "q100": _k((4, 8), n=100), "q15": _k((1, 2), n=15),
    },
    "9_8": {
        "Q": _k((520, 620)), "L": _k(4096, 2048), "s": _k(536, 1024), "s+": _k(537, 1025),
        # 9000 samples of 8 bits would still stage at NR = 36 (2250 + 3 <= 2304)
        "l": _k(2325, n=9300), "m": _k(1250, n=5000), "q100": _k((4, 8), n=100), "q15": _k((1, 2), n=15),
    },
}

_SET_TO = {"b31": (2, 3, 14240), "b36": (3, 4, 8096), "b32": (9, 0, 48)}   # base value, other value, count on the '-' side


def chunk_samples(token, row_key, rng):
    """the samples of one chunk of class `token` under row `row_key`"""
    S = len(ROWS[row_key])
    n = CLASSES[row_key][token].n
    i = np.arange(n)
    if token in ("Q", "q100", "q15"):
        return (rng.random_sample(n) < 0.1).astype(np.uint8)
    if token == "M":
        return np.where(i & 1, 2, 1).astype(np.uint8)
    if token in ("L", "l", "m"):
        return np.full(n, S - 1, np.uint8)
    if token in ("s", "s+"):
        x = np.where((i >> 4) & 63 == 5, 3, 0).astype(np.uint8)
        if token == "s+":
            x[rng.choice(np.flatnonzero(x))] = 4
        return x
    base, other, count = _SET_TO[token[:3]]
    if token[3] == "+":      # one more long code (b31, b36) resp. one short code fewer (b32): one word more
        count += 1 if other > base else -1
    x = np.full(n, base, np.uint8)
    x[rng.choice(n, size=count, replace=False)] = other
    return x


def chunk_words(payload, seg_off, seg_words, seg_n):
    """Per chunk of one segment (hw, nw, longest sub-stream in bits), read from the chunk headers as include/muahuff.h
    describes them: a 12-bit minimum sub-stream length, a 4-bit field width w, 64 w-bit (length - minimum) fields from
    bit 16 on; hw = ceil((16 + 64 w) / 32) header words, then ceil(sum of lengths / 32) payload words.  The chunks of
    a segment follow one another; they must add up to seg_words."""
    pos, out = int(seg_off), []
    for _ in range((int(seg_n) + CHUNK - 1) // CHUNK):
        w0 = int(payload[pos])
        mn, w = w0 & 0xFFF, (w0 >> 12) & 15
        hw = (16 + 64 * w + 31) // 32
        bits = 0
        for k in range(hw):
            bits |= int(payload[pos + k]) << (32 * k)
        lens = [mn + ((bits >> (16 + j * w)) & ((1 << w) - 1)) for j in range(64)]
        nw = (sum(lens) + 31) // 32
        out.append((hw, nw, max(lens)))
        pos += hw + nw
    assert pos - int(seg_off) == int(seg_words), (pos, int(seg_off), int(seg_words))
    return out


# ---- patterns: full segments and last segments (with a tail) per row and seg_chunks --------------------------------
_P10_9 = {
    2: (("Q L", "L Q", "s L", "L s", "M M", "Q M", "M Q", "b31- Q", "Q b31-", "b31+ Q", "Q b31+", "b36- Q", "Q b36-",
         "b36+ Q", "Q b36+", "s s+", "s+ s", "L L"),
        ("Q l", "L l", "Q m", "L m", "Q q100", "L q15")),
    3: (("s s+ s", "M Q M", "Q L Q", "L Q L", "Q Q L", "M M Q", "Q M M", "b31+ Q b31-", "b36+ Q b36-", "Q b36- M",
         "s+ Q s+"),
        ("Q L l", "L Q m", "Q Q q15", "L l", "Q m")),
    4: (("Q L Q Q", "L Q L L", "Q Q Q L", "M M M M", "Q M M Q", "s s+ s L", "M M Q L", "Q M Q L", "Q Q L Q",
         "Q b36- b31+ Q"),
        ("Q Q L l", "L L Q q100", "Q M M m", "Q l")),
}
_P10_4 = {
    2: (("Q L", "L Q", "b32- Q", "Q b32-", "b32+ Q", "Q b32+", "L L", "Q Q"),
        ("Q l", "L l", "Q m", "L m", "Q q100", "L q15")),
    4: (("Q L Q Q", "L Q L L", "Q Q Q L", "Q b32- b32+ Q"),
        ("Q Q L l", "L q15")),
}
_P6_5 = {
    2: (("Q L", "L Q", "s L", "L s", "s s+", "s+ s", "Q Q", "L L"),
        ("Q l", "L l", "Q m", "L m", "Q q100", "L q15")),
    3: (("s s+ s", "Q L Q", "L Q L", "Q Q L"),
        ("Q L l", "L Q m")),
}
PATTERNS = {"10_9": _P10_9, "10_4": _P10_4, "6_5": _P6_5, "9_8": {2: _P6_5[2]}}
SINGLE = "l"     # one channel that is a single partial chunk (seg_chunks 2 only: see _wg_channels)


def _wg_channels(full, tails, single):
    """Workgroup tasks: every channel has a multiple of 4 segments (three full ones in front of each tail, the rest in
    fours, the list repeated from its start where a four is short).  The single-chunk channel leaves three waves of
    its task idle, which the planner's rule (at most one idle wave in 16) allows from 45 segments on."""
    chans = []
    it = 0

    def take(k):
        nonlocal it
        got = tuple(full[(it + j) % len(full)] for j in range(k))
        it += k
        return got
    for t in tails:
        chans.append(take(3) + (t,))
    while it < len(full) or (single and sum(len(c) for c in chans) < 45):
        chans.append(take(4))
    if single:
        chans.append((SINGLE,))
    return tuple(chans)


def _wave_channels(full, tails, single):
    """Wave tasks: at most 3 segments per channel, so a workgroup task would idle one wave in four."""
    chans = [(full[j % len(full)], t) for j, t in enumerate(tails)]
    rest = full[len(tails):] if len(full) > len(tails) else ()
    chans += [tuple(rest[j:j + 3]) for j in range(0, len(rest), 3)]
    if single:
        chans.append((SINGLE,))
    return tuple(chans)


@dataclass(frozen=True)
class Scenario:
    row_key: str
    sc: int              # seg_chunks
    wave: bool           # the task form the layout puts the plan on
    channels: tuple      # per channel: its segments, each a string of tokens

    @property
    def name(self):
        return "%s-sc%d-%s" % (self.row_key, self.sc, "wave" if self.wave else "wg")

    @property
    def row(self):
        return ROWS[self.row_key]

    @property
    def S(self):
        return len(self.row)

    @property
    def maxlen(self):
        return max(self.row)

    def tokens(self):
        """[(channel, segment within the channel, chunk within the segment, token)] in stream order"""
        return [(c, s, k, tok) for c, segs in enumerate(self.channels) for s, seg in enumerate(segs)
                for k, tok in enumerate(seg.split())]

    def lens(self):
        kl = CLASSES[self.row_key]
        return [sum(kl[tok].n for seg in segs for tok in seg.split()) for segs in self.channels]

    def build(self):
        """-> the channels' samples (uint8 arrays); the same for every caller"""
        rng = np.random.RandomState(zlib.crc32(self.name.encode()))
        chans = []
        for segs in self.channels:
            parts = [chunk_samples(tok, self.row_key, rng) for seg in segs for tok in seg.split()]
            chans.append(np.concatenate(parts))
        return chans

    def chunk_starts(self):
        """{(channel, segment, chunk): first sample of that chunk in its channel}"""
        out = {}
        for c, segs in enumerate(self.channels):
            for s, seg in enumerate(segs):
                for k in range(len(seg.split())):
                    out[(c, s, k)] = (s * self.sc + k) * CHUNK
        return out


def _scenarios():
    out = []
    for row_key, by_sc in PATTERNS.items():
        for sc, (full, tails) in sorted(by_sc.items()):
            single = sc == 2
            out.append(Scenario(row_key, sc, False, _wg_channels(full, tails, single)))
            out.append(Scenario(row_key, sc, True, _wave_channels(full, tails, single)))
    return tuple(out)


SCENARIOS = _scenarios()
WG_SCENARIOS = tuple(s for s in SCENARIOS if not s.wave)      # segment counts per channel multiples of 4
WAVE_SCENARIOS = tuple(s for s in SCENARIOS if s.wave)        # at most 4 segments per channel


def check_shape(scn):
    """a scenario is well formed: every full segment has seg_chunks whole chunks, a tail only ends a channel"""
    kl = CLASSES[scn.row_key]
    for segs in scn.channels:
        for s, seg in enumerate(segs):
            toks = seg.split()
            last = s == len(segs) - 1
            assert 1 <= len(toks) <= scn.sc
            assert all(kl[t].n == CHUNK for t in toks[:-1]), seg
            if not last:
                assert len(toks) == scn.sc and kl[toks[-1]].n == CHUNK, seg
            else:
                assert len(toks) == scn.sc or kl[toks[-1]].n < CHUNK, seg


# ---- the routes a segment takes, from its chunk sizes alone ----------------------------------------------------------
DEC_TRANSITIONS = ("staged->oversize", "oversize->staged-size", "first chunk oversize with more to come",
                   "oversize partial", "fits by 0 words", "exceeds by 1 word")
PAIR_TRANSITION = "pair too large / singles fit"
ENC_TRANSITIONS = ("fast->slow with pend > 0", "slow->fast", "sp == cap", "sp == cap + 1")


def decoder_transitions(chunks, n, NR, dual):
    """What decode_segment / decode_segment_dual (csrc/mh_codec2.hpp) meet on a segment of n samples whose chunks are
    `chunks` [(hw, nw, longest)]: the set of transition names.  A size test counts only where the code makes it: the
    pipeline tests the first chunk and then each next one until one fails; the per-symbol loop tests nothing."""
    cap = 64 * NR
    nfull = n // CHUNK
    seen = set()

    def sized(nw):
        if nw + 3 == cap:
            seen.add("fits by 0 words")
        if nw + 3 == cap + 1:
            seen.add("exceeds by 1 word")
        return nw + 3 <= cap
    c = 0
    if dual:
        while c + 2 <= nfull:
            (_ha, nwa, _), (hwb, nwb, _) = chunks[c], chunks[c + 1]
            if nwa + hwb + nwb + 3 > cap:
                if nwa + 3 <= cap and nwb + 3 <= cap:
                    seen.add(PAIR_TRANSITION)
                break
            c += 2
    first = c
    if c < nfull:
        if sized(chunks[c][1]):
            c += 1
            while c < nfull and sized(chunks[c][1]):
                c += 1
            if c < nfull:
                seen.add("staged->oversize")
        elif nfull - first > 1 or n % CHUNK:
            seen.add("first chunk oversize with more to come")
        slow_from = c
        for k in range(slow_from + 1, nfull):
            if chunks[k][1] + 3 <= cap:
                seen.add("oversize->staged-size")
    if n % CHUNK and not sized(chunks[nfull][1]):
        seen.add("oversize partial")
    return seen


def encoder_transitions(chunks):
    """What an LC >= 2 encoder (encode_full_chunk / encode_partial_chunk) meets on a segment: `pend` is the words
    carried so far modulo 64 (merge_and_flush), 0 behind a slow chunk (overflow_chunk), which leaves the output pointer
    where its own words end: "slow->fast" counts a staged chunk that starts off the 64-word grid for that reason."""
    seen = set()
    pend, words, off_grid = 0, 0, False
    for hw, nw, longest in chunks:
        sp = (longest + 31) // 32
        if longest == ENC_STAGE_BITS:
            assert sp == ENC_STAGE_BITS // 32
            seen.add("sp == cap")
        if longest == ENC_STAGE_BITS + 1:
            assert sp == ENC_STAGE_BITS // 32 + 1
            seen.add("sp == cap + 1")
        if longest > ENC_STAGE_BITS:
            if pend:
                seen.add("fast->slow with pend > 0")
            pend = 0
            off_grid = (words + hw + nw) % 64 != 0
        else:
            if off_grid:
                seen.add("slow->fast")
            pend = (pend + hw + nw) % 64
        words += hw + nw
    return seen


# ---- the oracle's side of a scenario, computed once and shared ---------------------------------------------------------
BY_NAME = {s.name: s for s in SCENARIOS}
OVERSIZE_TOKENS = ("L", "l", "b31+", "b36+", "b32+")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The CPU oracle on scenario `name`: channels, flat data, the encode (slotted stream), its decode, and per segment
    the chunk sizes read from the stream's headers.  Callers must not modify any of it."""
    import oracle
    OC = oracle.c
    scn = BY_NAME[name]
    chans = scn.build()
    data, off, ln = OC.flatten(chans)
    rows = np.array([scn.row], np.uint8)
    p = OC.Params(scn.S, 0, OC.MODE_NOSORT, OC.WIN_FULL, rows, seg_chunks=scn.sc)
    e = OC.encode(data, off, ln, p)
    dec = OC.decode(e["payload"], off, ln, p, e["peak"], e["enc"], len(data))
    seg = e["seg"]
    chunks = [chunk_words(e["payload"], seg["off"][s], e["seg_words"][s], seg["n"][s]) for s in range(len(seg["ch"]))]
    for a in (data, off, ln, dec, e["payload"], e["seg_words"], e["ch_bits"], e["peak"], e["enc"]) + tuple(chans):
        a.setflags(write=False)
    return types.SimpleNamespace(scn=scn, chans=chans, data=data, off=off, ln=ln, rows=rows, params=p, enc=e, dec=dec,
                                 chunks=chunks, full=[dec[int(o):int(o) + int(n)] for o, n in zip(off, ln)])


def query_ranges(scn):
    """[(channel, t0, t1)] of the range tests: the whole of every channel, and around every oversize chunk (first
    sample p of its channel) a range cut inside it on both sides, one over its first and one over its last sample, one
    that only passes over it, and one that starts in the chunk behind it in the same segment."""
    lens = scn.lens()
    out = [(c, 0, T) for c, T in enumerate(lens)]
    toks = {(c, s, k): t for c, s, k, t in scn.tokens()}
    for (c, s, k), p in sorted(scn.chunk_starts().items()):
        if toks[(c, s, k)] not in OVERSIZE_TOKENS:
            continue
        T = lens[c]
        cand = [(p + 5, p + CHUNK - 7), (p - 3, p + 40), (p + CHUNK - 40, p + CHUNK + 3), (p + CHUNK, T)]
        if (c, s, k + 1) in toks:
            cand.append((p + CHUNK + 100, p + CHUNK + 900))
        for a, b in cand:
            a, b = max(a, 0), min(b, T)
            if a < b:
                out.append((c, a, b))
    return out
