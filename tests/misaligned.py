"""Byte-misaligned channel layouts for every byte-layout codec cell and every histogram kernel (a plain module, not a
conftest).

mh_plan_create takes channel i as the bytes [ch_off[i], ch_off[i] + ch_len[i]) of the buffer, at any address, and the
window rules move the coded range on: MH_WIN_REF_HALF, _TRUNC and _AFTER_CAL start c = min(2^h, T) samples in, and the
two REF_HALF rules end inside the channel with live samples behind the end.  The layouts of tests/kernel_cells.py come
from oracle.c.flatten (offsets padded to 16 bytes, whole-channel windows), so there every 16-byte row load and store is
aligned and only zeros follow a window.  Here:

  layout()           channels at ch_off[0] = shift, ch_off[i + 1] = ch_off[i] + len[i] + gap[i % len(gap)]: touching
                     neighbours (gap 0), small odd gaps and one of more than a cache line; GUARD bytes in front of the
                     first channel and behind the last.  With the buffer itself on a 128-byte boundary (the GPU tests
                     assert it) an offset IS the address residue.  Guards and gaps hold the PAD pattern of countable
                     symbols, not zeros: a kernel that reads one as a sample changes a histogram bin or a codeword
  codec_scenarios()  per byte-layout cell of kernel_cells.ENCODER_CELLS (12) and DECODER_CELLS (8): the cell layouts'
                     lengths as WINDOW lengths under MH_WIN_AFTER_CAL, _REF_HALF_TRUNC and _REF_HALF with h = 0..3 (the
                     window starts 1, 2, 4 or 8 samples into its channel), which keeps the cell's task form
  measure_scenarios()  S = 2, 3, 5, 8, 9, 10 (k_hist<1>, k_hist<2>, two each for k_hist2<3> and k_hist2<4>), both
                     mappers, MH_WIN_REF_HALF and _AFTER_CAL, as one launch (h <= 12) and as separate launches (h = 13, whose
                     calibration window also goes through the tiled k_hist2<4>); window lengths follow from the tile
                     geometry (measure_lens)

tests/test_host_misaligned.py checks without a GPU that every scenario lands on its cell's kernel and in the form it
claims, that the scenarios reach the address residues they are for, and that the oracle is indifferent to the offsets;
tests/test_gpu_misaligned.py runs them against the oracle.  Every comparison is exact."""
import functools
import itertools
import zlib
from dataclasses import dataclass

import numpy as np

from tests import kernel_cells as kc

CHUNK = kc.CHUNK
GUARD = 256                     # bytes in front of the first channel and behind the last (at least)
TILE = 256 * 16 * 32            # kHistTileBytes (csrc/mh_planner.hpp): samples of one histogram tile
WIN_REF_HALF, WIN_REF_HALF_TRUNC, WIN_AFTER_CAL = 0, 1, 2
GAPS = (0, 3, 117, 1)           # bytes between neighbouring channels, in turn
PAD = np.array([0, 1, 2, 255], np.uint8)   # what guards and gaps hold, repeated


def window(T, h, rule):
    """(w0, w1, skipped) of a channel of T samples: include/muahuff.h, MH_WIN_*"""
    c = min(1 << h, T)
    e = c + T // 2
    if rule == WIN_REF_HALF:
        return (c, c, 1) if e > T else (c, e, 0)
    if rule == WIN_REF_HALF_TRUNC:
        return c, min(e, T), 0
    if rule == WIN_AFTER_CAL:
        return c, T, 0
    return 0, T, 0


def offsets(lens, shift, gaps=GAPS):
    assert shift >= GUARD
    off = [shift]
    for i, T in enumerate(lens[:-1]):
        off.append(off[-1] + T + gaps[i % len(gaps)])
    return np.array(off, np.uint64)


def layout(chans, shift, gaps=GAPS):
    """list of 1-D uint8 arrays -> (data, ch_off, ch_len)"""
    lens = [len(x) for x in chans]
    off = offsets(lens, shift, gaps)
    data = np.resize(PAD, int(off[-1]) + lens[-1] + GUARD)
    for x, o in zip(chans, off):
        data[int(o):int(o) + len(x)] = x
    return data, off, np.array(lens, np.uint64)


def head(addr):
    """bytes a histogram tile at this address peels before its first aligned 16-byte vector"""
    return (16 - addr % 16) % 16


# ------------------------------------------------------------------------------------------
# codec
# ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Scenario:
    case: kc.Case
    lens: tuple          # channel lengths
    seg_chunks: int
    h: int
    window: int
    mode: int
    shift: int

    def offsets(self):
        return offsets(self.lens, self.shift)


def _after(h, wins):
    """channel lengths whose MH_WIN_AFTER_CAL windows [c, T) have the lengths `wins`"""
    return tuple(n + (1 << h) for n in wins)


def _half(wins):
    """channel lengths whose REF_HALF windows [c, c + T // 2) have the lengths `wins`, T = 2 n + 1 (n >= c - 1)"""
    return tuple(2 * n + 1 for n in wins)


# (channel lengths, seg_chunks, h, rule, shift) per task form: the layouts of kernel_cells -- lengths below 16, off
# multiples of 16, whole chunks and one past -- as windows.  The shifts are 1, 7, 8 and 15 mod 16 in either form and
# chosen so that the windows of a form start at 1, 8 and 15 mod 16 and in the last 15 bytes of a 128-byte line
# (tests/test_host_misaligned.py computes it).  The window of 16 chunks starts with a head segment.
# The MH_WIN_REF_HALF templates (h = 2: c = 4) hold channels the rule SKIPS -- c + T // 2 > T, T = 2, 3 and 5: no
# segments, nothing decoded over them, in a wave-task plan a calibrate-only record -- touching the end of a coded
# neighbour (gap 0 in front of the second and the last channel) and between odd gaps.
_W, _G = [l[0] for l in kc.WAVE_LAYOUTS], [l[0] for l in kc.WG_LAYOUTS]
WAVE = (
    (_after(0, _W[0]), 1, 0, WIN_AFTER_CAL, 256 + 7),
    (_half(_W[1]), 2, 3, WIN_REF_HALF_TRUNC, 384 + 8),
    (_half(_W[2][1:2]) + (5,) + _half(_W[2][2:3]) + (3,) + _half(_W[2][3:]) + (2,), 3, 2, WIN_REF_HALF, 256 + 15),
    (_after(1, _W[3]), 4, 1, WIN_AFTER_CAL, 512 + 1),
    (_half(_W[4]), 1, 3, WIN_REF_HALF_TRUNC, 256 + 6),
)
WG = (
    (_half(_G[0]), 1, 3, WIN_REF_HALF_TRUNC, 256 + 1),
    (_after(0, _G[1]), 2, 0, WIN_AFTER_CAL, 384 + 7),
    (_half(_G[2][:1]) + (5,) + _half(_G[2][1:]) + (3, 2), 3, 2, WIN_REF_HALF, 256 + 8),
    (_after(1, _G[3]), 4, 1, WIN_AFTER_CAL, 512 + 15),
    (_half(_G[5]), 1, 2, WIN_REF_HALF_TRUNC, 256 + 2),
)

CODEC_CELLS = tuple(c for c in kc.ENCODER_CELLS if c.input_bits == 8) + kc.DECODER_CELLS


def codec_scenarios(cell):
    """the cell's cases in turn over the templates of its task form, NOSORT / APPROX alternating from cell.mode"""
    return tuple(Scenario(cell.cases[i % len(cell.cases)], lens, sc, h, rule, (cell.mode + i) % 2, shift)
                 for i, (lens, sc, h, rule, shift) in enumerate(WAVE if cell.wave else WG))


def codec_channels(rng, lens):
    """Poisson counts at mixed rates, as the pattern `matched` of tests/test_gpu_kernel_cells.py has them"""
    return [np.minimum(rng.poisson(float(np.exp(rng.uniform(np.log(0.05), np.log(6.0)))), size=T), 255).astype(np.uint8)
            for T in lens]


# ------------------------------------------------------------------------------------------
# measure
# ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class MeasureScenario:
    S: int
    mode: int
    window: int
    h: int
    fused: bool          # mh_measure as one launch (csrc/mh_planner.hpp: measure_fused)
    shift: int

    @property
    def ident(self):
        return "S%d-%s-%s-h%d" % (self.S, ("nosort", "approx")[self.mode], ("half", "trunc", "after")[self.window],
                                  self.h)

    def lens(self):
        return measure_lens(self.h, self.window, self.shift)

    def offsets(self):
        lens, gaps, _kinds = self.lens()
        return offsets(lens, self.shift, gaps)


@functools.lru_cache(maxsize=None)
def measure_lens(h, rule, shift):
    """-> (channel lengths, the gap in front of every channel but the first, what each channel is for).

    Write H for the head of a channel's tiles, head(address of its window).  Every tile of a window starts a multiple
    of 16 from it, so all of them peel H bytes, and the last one the tail.  Window lengths:
      "head"   H - 1 (the tile is shorter than its head), H (head only), H + 1 (head and tail, no vector), H + 15,
               H + 16, H + 17 (one vector; without a tail, with one of 1 sample), three times over with different H.  The gaps
               are GAPS in turn; where a gap would give one of these, a "tile" or a "bit" channel H < 2, the next one
               is taken instead (place).
      "tile"   one whole tile, one sample less and one more (a second tile of 1 sample, shorter than its head)
      "bit"    one and a bit tiles, the bit odd
      "one"    a channel of one sample: the first channel, and one whose own address is 2..15 bytes short of a 16-byte
               boundary (a calibration tile shorter than its head)
      "short"  a channel that ends inside its calibration window (empty window)
      "skip"   a channel of exactly 2^h samples: empty window, skipped under MH_WIN_REF_HALF
      "full"   every sample 255
    MH_WIN_REF_HALF codes [c, c + T // 2) and skips a channel whose window would run past its end, so a window is at
    least c samples: with c > 8 the "head" lengths stand on top of c (a multiple of 16: the same head and tail), with
    c <= 8 the heads are kept above c."""
    c = 1 << h
    base = c if rule == WIN_REF_HALF and c > 8 else 0
    hmin = c + 1 if rule == WIN_REF_HALF and not base else 2
    assert 2 <= hmin <= 9
    lens, gaps, kinds = [], [], []
    cycle = itertools.cycle(GAPS)

    def place(ok):
        """the address of the next channel: behind the next gap of the cycle for which ok(address) holds"""
        if not lens:
            return shift
        end = shift + sum(lens) + sum(gaps)
        gaps.append(next(g for g in cycle if ok(end + g)))
        return end + gaps[-1]

    def channel(kind, T):
        lens.append(T)
        kinds.append(kind)

    def windowed(kind, n):
        """a channel whose window has n samples ("head": H + n on top of `base`); its tiles' head is at least hmin"""
        at = place(lambda a: head(a + c) >= hmin)
        if kind == "head":
            n += base + head(at + c)
        T = c + n if rule == WIN_AFTER_CAL else 2 * n
        assert window(T, h, rule)[:2] == (c, c + n), (T, h, rule, n)
        channel(kind, T)

    place(lambda a: True)
    channel("one", 1)
    for rep in range(3):
        for d in (-1, 0, 1, 15, 16, 17):
            windowed("head", d)
        if rep == 0:
            windowed("tile", TILE)
            place(lambda a: head(a) >= 2)     # its calibration tile, where it has one, is shorter than its head
            channel("one", 1)
        elif rep == 1:
            windowed("tile", TILE - 1)
            windowed("bit", TILE + 20001)
        else:
            windowed("tile", TILE + 1)
            place(lambda a: True)
            if c > 2:
                channel("short", c - 1)
                place(lambda a: True)
            channel("skip", c)
    windowed("full", base + 4097)
    return tuple(lens), tuple(gaps), tuple(kinds)


MEASURE_S = (2, 3, 5, 8, 9, 10)
# candidate encoders per S: every row kernel_cells has for it (first argmin over more than one row from S = 5 on)
MEASURE_ROWS = {S: sum((kc.R[k] for k in sorted(kc.R) if k[0] == S), ()) for S in MEASURE_S}
# (window, h, one launch); the shift follows S and the mapper below
MEASURE_FORMS = ((WIN_REF_HALF, 1, True), (WIN_AFTER_CAL, 12, True), (WIN_REF_HALF, 13, False),
                 (WIN_AFTER_CAL, 13, False))
_MEASURE_SHIFTS = (1, 7, 8, 15, 9, 3)


def measure_scenarios():
    out = []
    for rule, h, fused in MEASURE_FORMS:
        for i, S in enumerate(MEASURE_S):
            for mode in (0, 1):
                shift = 256 + _MEASURE_SHIFTS[(i + 3 * mode) % 6]
                out.append(MeasureScenario(S, mode, rule, h, fused, shift))
    return tuple(out)


@functools.lru_cache(maxsize=8)
def measure_channels(h, rule, shift):
    """Poisson counts at mixed rates, one sample in eight uniform in 0..255 (so every S clips, in the head and tail
    loops and in the vectors); the "full" channel is all 255"""
    lens, _gaps, kinds = measure_lens(h, rule, shift)
    rng = np.random.RandomState(zlib.crc32(repr((h, rule, shift)).encode()))
    chans = []
    for T, kind in zip(lens, kinds):
        x = rng.poisson(float(np.exp(rng.uniform(np.log(0.05), np.log(6.0)))), size=T)
        x = np.where(rng.random_sample(T) < 0.125, rng.randint(0, 256, size=T), x)
        chans.append(np.full(T, 255, np.uint8) if kind == "full" else np.minimum(x, 255).astype(np.uint8))
    return tuple(chans)
