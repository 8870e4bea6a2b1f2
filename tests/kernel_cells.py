"""The codec kernels the production library ships, one cell per instance (a plain module, not a conftest).

libmuahuff.so compiles a fixed set of k_encode2 / k_encode2w / k_decode2 / k_decode2w template instances, and
enc_pick and dec_pick (csrc/mh_select.hpp) choose among them from the plan: maxlen L (the longest codeword of the
plan's SCLV rows), S <= 8 (3-bit pair packing) or not, input_bits (8, or packed 4 / 2), the planner's wave-task rule
(csrc/mh_planner.hpp) and, for the decoder, the output (bytes for mh_decode, 2- / 4-bit pieces for mh_decode_packed:
input_bits of the packed cells) and the table width W.  Every CELL names one instance and the plans that land on it:

  cases    (S, SCLV rows) pairs -- each row Kraft-complete and non-decreasing -- with the maxlen they give; decoder
           cells also give the table width W for that case
  layouts  (channel lengths, seg_chunks): whole-channel windows (MH_WIN_FULL) that put the plan in the cell's task
           form -- wave tasks when the workgroup tasks (<= 4 segments of one channel) would leave more than one
           wave in 16 idle, workgroup tasks otherwise

tests/test_host_kernel_cells.py checks without a GPU that the cells and the shipped symbols are the same set and
that the library's own selection puts every case and layout on its cell's instance; tests/test_gpu_kernel_cells.py
(encoders, byte decoders) and tests/test_gpu_stream_decode.py (packed decoders) run them against the CPU oracle.

  mixed    the layouts here keep every channel on ONE route per chunk (all staged or all oversize); transitions within
           a segment -- staged and oversize chunks side by side -- are tests/mixed_chunks.py, run by
           tests/test_host_mixed_chunks.py and tests/test_gpu_mixed_chunks.py
  aligned  the layouts here are flattened by oracle.c.flatten -- channel offsets padded to 16 bytes -- and coded whole
           (MH_WIN_FULL), so every 16-byte row load and store is aligned and only padding follows a window; the
           byte-layout cells at odd addresses, with touching channels and windows that start 1..8 samples into a
           channel and end inside it, are tests/misaligned.py, run by tests/test_host_misaligned.py and
           tests/test_gpu_misaligned.py
"""
from dataclasses import dataclass

CHUNK = 16384


@dataclass(frozen=True)
class Case:
    S: int
    rows: tuple          # K rows of S code lengths
    maxlen: int
    W: int = 0           # decoder cells: index bits of the decode table


@dataclass(frozen=True)
class Cell:
    symbol: str          # demangled kernel name as the code object lists it, "mh::k_encode2<1, 4, 0>"
    wave: bool           # wave-task form (k_*2w) or workgroup-task form (k_*2)
    input_bits: int      # 8 = byte input; 4 / 2 = packed pieces (mh_plan_create_packed)
    mode: int            # mapper the placement is checked with (the GPU tests run both)
    cases: tuple
    layouts: tuple

    @property
    def decoder(self):
        return "k_decode2" in self.symbol

    @property
    def key(self):
        """Name of the cell's GPU tests and seed of their data.  It keeps the symbol's form from when the table was
        written, before k_encode2 lost its ablation level (always 0, before PK), k_decode2 its DUAL flag (always
        false) and the decoders gained PO: the byte decoders (PO = 0) keep the names without it, the packed ones
        (PO = 2 / 4) the names of their former kernels k_decpk / k_decpkw.  So every cell keeps its test ids and its
        data across those renames."""
        head, args = self.symbol[:-1].split("<")
        if head == "mh::k_encode2":
            lc, pb, pk = args.split(", ")
            return "%s<%s, %s, 0, %s>" % (head, lc, pb, pk)
        if self.decoder:
            rest, po = args.rsplit(", ", 1)
            if po != "0":
                return "%s<%s, %s>" % (head.replace("k_decode2", "k_decpk"), rest, po)
            return "%s<%s, false>" % (head, rest) if head == "mh::k_decode2" else "%s<%s>" % (head, rest)
        return self.symbol


def _row(*lens):
    return (tuple(lens),)


# rows by (S, L)
R = {
    (2, 1): _row(1, 1),
    (3, 2): _row(1, 2, 2),
    (4, 2): _row(2, 2, 2, 2),
    (4, 3): _row(1, 2, 3, 3),
    (5, 3): _row(2, 2, 2, 3, 3),    # the shortest code a 4-bit packed decoder can have
    (5, 4): _row(1, 2, 3, 4, 4),
    (8, 3): _row(*[3] * 8),
    (8, 4): _row(2, 2, 3, 3, 4, 4, 4, 4),
    (9, 4): _row(2, 2, 3, 4, 4, 4, 4, 4, 4),
    (10, 4): _row(2, 2, 4, 4, 4, 4, 4, 4, 4, 4),
    (6, 5): _row(1, 2, 3, 4, 5, 5),
    (8, 5): _row(2, 2, 2, 4, 4, 4, 5, 5),
    (9, 5): _row(2, 2, 2, 4, 4, 5, 5, 5, 5),
    (7, 6): _row(1, 2, 3, 4, 5, 6, 6),
    (8, 7): _row(1, 2, 3, 4, 5, 6, 7, 7),
    (9, 8): _row(1, 2, 3, 4, 5, 6, 7, 8, 8),
    (10, 9): _row(1, 2, 3, 4, 5, 6, 7, 8, 9, 9),
}
# two candidate encoders, the longest code in the one a quiet calibration picks
R2_10_9 = R[(10, 9)] + R[(10, 4)]


def _c(S, L, rows=None, **dec):
    return Case(S, rows or R[(S, L)], L, **dec)


# Task forms.  Wave: every channel has at most 4 segments, so each workgroup task idles waves.  Workgroup: segment
# counts are multiples of 4 -- a channel of 5 samples next to 44 full segments is exactly at the rule's edge
# (48 padded waves * 15 == 45 segments * 16).  Lengths below 16, off multiples of 16, whole chunks and one past; the
# equal-length layouts are also packed by the device de-interleaver.
WAVE_LAYOUTS = (
    ((7, 1000, CHUNK, CHUNK + 1, 40000, 3 * CHUNK), 1),
    ((15, 16, 17, 2 * CHUNK + 1, 4 * CHUNK, 100000), 2),
    ((1, 3 * CHUNK, 3 * CHUNK + 1, 120000), 3),
    ((3, 4 * CHUNK + 1, 200000, 130000), 4),
    ((CHUNK + 1,) * 6, 1),
)
WG_LAYOUTS = (
    ((4 * CHUNK, 3 * CHUNK + 1, 8 * CHUNK - 5, 7 * CHUNK + 16), 1),
    ((8 * CHUNK, 6 * CHUNK + 1, 115687), 2),
    ((12 * CHUNK, 9 * CHUNK + 1), 3),
    ((16 * CHUNK, 13 * CHUNK + 7), 4),
    ((44 * CHUNK, 5), 1),
    ((4 * CHUNK - 3,) * 3, 1),
)


def _pair(wg_symbol, wave_symbol, input_bits, cases, mode=1):
    return [Cell(wg_symbol, False, input_bits, mode, tuple(cases), WG_LAYOUTS),
            Cell(wave_symbol, True, input_bits, 1 - mode, tuple(cases), WAVE_LAYOUTS)]


ENCODER_CELLS = tuple(
    # byte input: LC = code class of L (<= 2, <= 4, <= 8, 9), PB = 3-bit pairs (S <= 8) or 4-bit pairs
    _pair("mh::k_encode2<0, 3, 0>", "mh::k_encode2w<0, 3, 0>", 8, [_c(3, 2), _c(2, 1), _c(4, 2)])
    + _pair("mh::k_encode2<1, 3, 0>", "mh::k_encode2w<1, 3, 0>", 8, [_c(8, 3), _c(4, 3), _c(8, 4)])
    + _pair("mh::k_encode2<1, 4, 0>", "mh::k_encode2w<1, 4, 0>", 8, [_c(9, 4), _c(10, 4)])
    + _pair("mh::k_encode2<2, 3, 0>", "mh::k_encode2w<2, 3, 0>", 8, [_c(8, 7), _c(6, 5), _c(8, 5)])
    + _pair("mh::k_encode2<2, 4, 0>", "mh::k_encode2w<2, 4, 0>", 8, [_c(9, 8), _c(9, 5)])
    + _pair("mh::k_encode2<3, 4, 0>", "mh::k_encode2w<3, 4, 0>", 8, [_c(10, 9), _c(10, 9, R2_10_9)])
    # 2-bit pieces (S <= 4): the four-symbol table
    + _pair("mh::k_encode2<0, 4, 2>", "mh::k_encode2w<0, 4, 2>", 2, [_c(3, 2), _c(4, 2), _c(2, 1)])
    + _pair("mh::k_encode2<1, 4, 2>", "mh::k_encode2w<1, 4, 2>", 2, [_c(4, 3)])
    # 4-bit pieces: a byte of the stream is the PB = 4 pair index
    + _pair("mh::k_encode2<0, 4, 4>", "mh::k_encode2w<0, 4, 4>", 4, [_c(3, 2), _c(4, 2)])
    + _pair("mh::k_encode2<1, 4, 4>", "mh::k_encode2w<1, 4, 4>", 4, [_c(4, 3), _c(5, 4), _c(9, 4), _c(10, 4)])
    + _pair("mh::k_encode2<2, 4, 4>", "mh::k_encode2w<2, 4, 4>", 4, [_c(6, 5), _c(8, 7), _c(9, 8)])
    + _pair("mh::k_encode2<3, 4, 4>", "mh::k_encode2w<3, 4, 4>", 4, [_c(10, 9)])
)

DECODER_CELLS = (
    # byte output; workgroup form: shared tables of up to 10 index bits
    Cell("mh::k_decode2<4, 4, 17, 1, false, 0>", False, 8, 1,
         (_c(3, 2, W=8), _c(2, 1, W=4)), WG_LAYOUTS),
    Cell("mh::k_decode2<2, 2, 25, 2, false, 0>", False, 8, 0,
         (_c(8, 3, W=6), _c(4, 3, W=6)), WG_LAYOUTS),
    Cell("mh::k_decode2<2, 2, 32, 0, false, 0>", False, 8, 1,      # L = 5 is the last with W = 2L
         (_c(9, 4, W=8), _c(6, 5, W=10), _c(8, 5, W=10)),
         WG_LAYOUTS),
    Cell("mh::k_decode2<2, 2, 31, 2, true, 0>", False, 8, 0,       # L = 6 is the first hybrid one
         (_c(7, 6, W=10), _c(10, 9, W=10), _c(9, 8, W=10)),
         WG_LAYOUTS),
    # wave form: per-wave tables of up to 8 index bits
    Cell("mh::k_decode2w<4, 4, 17, 1, false, false, 0>", True, 8, 0,
         (_c(3, 2, W=8), _c(4, 2, W=8)), WAVE_LAYOUTS),
    Cell("mh::k_decode2w<2, 2, 25, 2, false, false, 0>", True, 8, 1,
         (_c(8, 3, W=6), _c(4, 3, W=6)), WAVE_LAYOUTS),
    Cell("mh::k_decode2w<2, 2, 32, 0, false, false, 0>", True, 8, 0,      # L = 4 is the last with W = 2L
         (_c(9, 4, W=8), _c(8, 4, W=8)), WAVE_LAYOUTS),
    Cell("mh::k_decode2w<1, 2, 36, 2, false, true, 0>", True, 8, 1,       # L = 5 is the first one-symbol one
         (_c(6, 5, W=8), _c(9, 5, W=8), _c(10, 9, W=9)),               # (W >= L: an entry holds its first code)
         WAVE_LAYOUTS),
)

# packed output (mh_decode_packed), 2 / 4 bits per symbol (input_bits): the byte decoders' choice, restricted to what S
# allows.  Planned like StreamDecoder's blocks: no calibration window (h = 0), mode 1.
PACKED_DECODER_CELLS = (
    # 2-bit pieces (S <= 4): the four-symbol table for L <= 2, the pair table for L = 3
    Cell("mh::k_decode2<4, 4, 17, 1, false, 2>", False, 2, 1,
         (_c(3, 2, W=8), _c(2, 1, W=4), _c(4, 2, W=8)),
         WG_LAYOUTS),
    Cell("mh::k_decode2<2, 2, 25, 2, false, 2>", False, 2, 1, (_c(4, 3, W=6),), WG_LAYOUTS),
    Cell("mh::k_decode2w<4, 4, 17, 1, false, false, 2>", True, 2, 1,
         (_c(3, 2, W=8), _c(2, 1, W=4), _c(4, 2, W=8)),
         WAVE_LAYOUTS),
    Cell("mh::k_decode2w<2, 2, 25, 2, false, false, 2>", True, 2, 1, (_c(4, 3, W=6),), WAVE_LAYOUTS),
    # 4-bit pieces (S >= 5)
    Cell("mh::k_decode2<2, 2, 25, 2, false, 4>", False, 4, 1,
         (_c(5, 3, W=6), _c(8, 3, W=6)), WG_LAYOUTS),
    Cell("mh::k_decode2<2, 2, 32, 0, false, 4>", False, 4, 1,     # L = 5 is the last with W = 2L
         (_c(5, 4, W=8), _c(9, 4, W=8), _c(6, 5, W=10)),
         WG_LAYOUTS),
    Cell("mh::k_decode2<2, 2, 31, 2, true, 4>", False, 4, 1,      # hybrid pair table from L = 6
         (_c(7, 6, W=10), _c(10, 9, W=10)), WG_LAYOUTS),
    Cell("mh::k_decode2w<2, 2, 25, 2, false, false, 4>", True, 4, 1,
         (_c(5, 3, W=6), _c(8, 3, W=6)), WAVE_LAYOUTS),
    Cell("mh::k_decode2w<2, 2, 32, 0, false, false, 4>", True, 4, 1,  # L = 4 is the last with W = 2L
         (_c(5, 4, W=8), _c(10, 4, W=8)), WAVE_LAYOUTS),
    Cell("mh::k_decode2w<1, 2, 36, 2, false, true, 4>", True, 4, 1,   # one-symbol pairs from L = 5
         (_c(6, 5, W=8), _c(10, 9, W=9)), WAVE_LAYOUTS),
)

CELLS = ENCODER_CELLS + DECODER_CELLS + PACKED_DECODER_CELLS

