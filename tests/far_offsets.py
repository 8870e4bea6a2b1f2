"""Offsets, pitches and strides beyond 4 GiB for every entry point that takes one (a plain module, not a conftest).

Both C ABIs (include/muahuff.h, include/muahuff_ingest.h) take 64-bit offsets and strides from the caller.  A parameter
narrowed to 32 bits, or one product formed in 32 bits, passes every test whose addresses stay within a few hundred MiB of
the base pointer.  The cases here put a few KiB of real data at the far end of an allocation that is never touched as a
whole:

  arena    one device uint8 buffer of ARENA_BYTES = 2^32 + SLACK bytes (SLACK = 2^28), from torch.empty.  A far address
           is 2^32 + d with d + size < SLACK; its ALIAS is d, where the access lands when the offset -- or a product that
           forms it -- is cut to 32 bits.  d < 2^31, so a signed and an unsigned cut agree.  A wrong kernel therefore
           reads or writes inside the same allocation: no case can fault.
  arena W  int32 words, ARENA_W_WORDS = 2^32 + 2^26 of them: the three cases whose seg_off is >= 2^32 WORDS.
  far value    an offset or stride that is itself >= 2^32 (catches a narrowed parameter)
  far product  a stride below 2^32 whose product with a small index crosses it (catches a 32-bit multiply)

A far INPUT has a decoy of the same size at its alias (the complement for counts, other ticks for time stamps, zero words
for a payload); a far OUTPUT has canary there.  Every case is a Setup: an Image of the arena before the call (`pre`: the
windows around every true region and every alias), the Image after it (`post`: the yardstick's result inside canary at the
true place, the alias untouched), the list of accesses the call forms (base + sum of index * stride * scale, in bytes)
and the argument rules of the entry point.  The yardsticks (NumPy, zlib, oracle.c) see the channels rebased to offset 0;
no host array of arena size is ever built.

tests/test_host_far_offsets.py checks every Setup without a GPU: what crosses 2^32, that every address -- with each term
in full and with each term cut modulo 2^32 -- lies inside the arena AND inside a window that is compared, that a region
and its alias differ, and the argument rules.  tests/test_gpu_far_offsets.py uploads the windows, makes the call and
compares every window whole.

Where the arena bounds a shape of the table: an index i >= 2 times a stride >= 2^32 lies behind the arena, so far VALUES
come with index 1 (2 rows, 2 draws, 2 output slots) and three rows / draws / elements come with far PRODUCTS.  For the
same reason the mirror store of mhi_gram's symmetric form, at j * gram_row_stride, is not in the table: it happens only
between different tiles, i.e. for a row index >= 128, and 128 times a far stride lies behind the arena (its pitch is
checked near the base by tests/test_gpu_gram_tiles.py)."""
import zlib
from dataclasses import dataclass, field

import numpy as np

FAR = 1 << 32
SLACK = 1 << 28
ARENA_BYTES = FAR + SLACK
ARENA_W_WORDS = FAR + (1 << 26)
ARENA_W_BYTES = 4 * ARENA_W_WORDS
HEADROOM = 2 << 30                 # free HBM asked for on top of an arena: the small tensors of a case
CANARY = 0xA5
PAD = 256                          # canary in front of and behind every region of a window
CHUNK = 16384
STRIDE_VALUE = FAR                 # far value: FAR + a few bytes
STRIDE_PRODUCT = 1 << 31           # far product: 2^31 + a few KiB, times 2


def ceil_div(a, b):
    return -(-a // b)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# ---- the sparse image of an arena ------------------------------------------------------------------------------------
class Image:
    """Windows [lo, lo + n) of an arena of `size` bytes, each a host array that starts as canary; `mark` tells which bytes
    were put.  Windows that would overlap are merged."""

    def __init__(self, size=ARENA_BYTES):
        self.size = size
        self.wins = []             # [lo, bytes, mark]

    def _find(self, a, n):
        for w in self.wins:
            if w[0] <= a and a + n <= w[0] + w[1].size:
                return w
        return None

    def ensure(self, a, n):
        assert 0 <= a and a + n <= self.size, (a, n, self.size)
        if self._find(a, n) is not None:
            return
        lo, hi = max(0, a - PAD) & ~15, min(self.size, (a + n + PAD + 15) & ~15)
        hit = [w for w in self.wins if w[0] < hi and lo < w[0] + w[1].size]
        for w in hit:
            lo, hi = min(lo, w[0]), max(hi, w[0] + w[1].size)
        buf, mark = np.full(hi - lo, CANARY, np.uint8), np.zeros(hi - lo, bool)
        for w in hit:
            buf[w[0] - lo:w[0] - lo + w[1].size] = w[1]
            mark[w[0] - lo:w[0] - lo + w[1].size] = w[2]
            self.wins.remove(w)
        self.wins.append([lo, buf, mark])

    def put(self, a, data):
        d = as_bytes(data)
        self.ensure(a, d.size)
        w = self._find(a, d.size)
        w[1][a - w[0]:a - w[0] + d.size] = d
        w[2][a - w[0]:a - w[0] + d.size] = True

    def get(self, a, n):
        w = self._find(a, n)
        return None if w is None else w[1][a - w[0]:a - w[0] + n]

    def marked(self, a, n):
        w = self._find(a, n)
        return None if w is None else w[2][a - w[0]:a - w[0] + n]

    def copy(self):
        im = Image(self.size)
        im.wins = [[lo, b.copy(), m.copy()] for lo, b, m in self.wins]
        return im

    def nbytes(self):
        return sum(w[1].size for w in self.wins)


@dataclass(frozen=True)
class Term:
    """index * stride * scale bytes; scale = the element size of an element-indexed argument"""
    index: int
    stride: int
    scale: int = 1

    @property
    def value(self):
        return self.index * self.stride * self.scale

    def cuts(self):
        """what a kernel forms when the stride, the product or the byte product is taken modulo 2^32"""
        return {self.scale * self.index * (self.stride % FAR), self.scale * ((self.index * self.stride) % FAR),
                (self.scale * self.index * self.stride) % FAR}


@dataclass(frozen=True)
class Access:
    """a region a call reads (`role` "in") or writes ("out"): `nbytes` at base + sum of the terms; `arg` names the
    argument of the entry point that a term comes from"""
    arg: str
    role: str
    terms: tuple
    nbytes: int
    base: int = 0

    @property
    def full(self):
        return self.base + sum(t.value for t in self.terms)

    def aliases(self):
        """the addresses with one term cut, or the whole sum cut -- without the true one"""
        full, out = self.full, set()
        for t in self.terms:
            out |= {full - t.value + c for c in t.cuts()}
        out.add(self.base + (full - self.base) % FAR)
        out.discard(full)
        return sorted(out)


@dataclass
class Setup:
    arena: str                               # "A" or "W"
    pre: Image
    post: Image = None
    accesses: list = field(default_factory=list)
    crossing: list = field(default_factory=list)     # (what, value, unit): must be >= 2^32 of that unit
    rules: list = field(default_factory=list)        # (rule of the entry point, holds)
    run: object = None                               # run(ctx): the device call and the checks of its small outputs
    decoys: list = field(default_factory=list)       # (access, what its aliases hold): placed by seal()

    def read(self, arg, terms, data, decoy=None, base=0):
        """a far or near input: `data` at its true place; at every alias that nothing else occupies, the decoy"""
        d = as_bytes(data)
        acc = Access(arg, "in", tuple(terms), d.size, base)
        self.accesses.append(acc)
        self.pre.put(acc.full, d)
        self.decoys.append((acc, as_bytes(decoy) if decoy is not None else ~d))
        return acc

    def write(self, arg, terms, nbytes, base=0, initial=None):
        """an output region: canary (or `initial`, for calls that add to what is there) at its true place and its aliases"""
        acc = Access(arg, "out", tuple(terms), int(nbytes), base)
        self.accesses.append(acc)
        self.pre.ensure(acc.full, acc.nbytes)
        if initial is not None:
            self.pre.put(acc.full, initial)
        return acc

    def seal(self):
        """decoys and alias windows, once every true region is placed; then `post` starts as a copy of `pre`"""
        for acc in self.accesses:
            for a in acc.aliases():
                self.pre.ensure(a, acc.nbytes)
        for acc, dec in self.decoys:
            for a in acc.aliases():
                free = ~self.pre.marked(a, acc.nbytes)
                w = self.pre._find(a, acc.nbytes)
                s = slice(a - w[0], a - w[0] + acc.nbytes)
                w[1][s] = np.where(free, dec, w[1][s])
        self.post = self.pre.copy()

    def expect(self, acc, data):
        d = as_bytes(data)
        assert d.size == acc.nbytes, (acc.arg, d.size, acc.nbytes)
        self.post.put(acc.full, d)


@dataclass(frozen=True)
class Case:
    id: str
    row: str                  # the row of the table (one parametrised GPU test each)
    entry: str                # entry point(s)
    far: str                  # which argument is far
    kind: str                 # "value", "product" or "offset" (a far entry of an offset table)
    shape: str
    build: object
    args: tuple = ()
    arena: str = "A"

    def setup(self):
        return self.build(*self.args)


CASES = []


def _case(row, entry, far, kind, shape, build, *args, arena="A"):
    cid = "-".join([row if arena == "A" else row + "W"] + [str(a) for a in args])
    CASES.append(Case(cid, row, entry, far, kind, shape, build, args, arena))


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _counts(rng, n, rate=1.5):
    """counts with values on both sides of every clip and saturation"""
    x = np.minimum(rng.poisson(rate, size=n), 255).astype(np.uint8)
    x[rng.rand(n) < 0.05] = 255
    x[rng.rand(n) < 0.05] = rng.randint(3, 200)
    return x


def _off(d, far):
    return d + (FAR if far else 0)


def _table_terms(v, scale=1):
    return (Term(1, int(v), scale),)


# =====================================================================================================================
# mh_rebin
# =====================================================================================================================
REBIN_LENS = (1, 101, 32769, 100003)
REBIN_R = (2, 3, 5, 7)                 # k_rebin2, k_rebin2, k_rebin3<., 5>, k_rebin3<., 0>


def build_rebin(which, r, sat):
    """channel 0 low, the others far: their input (which = "in") or their bins (which = "out"; uint32: >= 2^30 elements)"""
    rng = _rng("rebin", which, r, sat)
    s = Setup("A", Image())
    C, e = len(REBIN_LENS), 1 if sat else 4
    chans = [_counts(rng, T, 3.0) for T in REBIN_LENS]
    in_off = [_off(0x100000 * (c + 1), which == "in" and c > 0) for c in range(C)]
    nb = [ceil_div(T, r) for T in REBIN_LENS]
    out_byte = [_off(0x800000 + 0x100000 * c + 4 * c, which == "out" and c > 0) for c in range(C)]
    out_off = [b // e for b in out_byte]
    for c in range(C):
        s.read("in_off", _table_terms(in_off[c]), chans[c])
    outs = [s.write("out_off", _table_terms(out_off[c], e), nb[c] * e) for c in range(C)]
    s.seal()
    for c in range(C):
        sums = np.add.reduceat(chans[c].astype(np.uint32), np.arange(0, REBIN_LENS[c], r))
        s.expect(outs[c], np.minimum(sums, 255).astype(np.uint8) if sat else sums.astype("<u4"))
    far = in_off if which == "in" else out_byte
    s.crossing = [("%s_off[%d] in bytes" % (which, c), far[c], "bytes") for c in range(1, C)]
    if which == "out" and not sat:
        s.rules.append(("uint32 out_off >= 2^30 elements", all(o >= 1 << 30 for o in out_off[1:])))
    s.rules.append(("out byte addresses fit the element size", all(b % e == 0 for b in out_byte)))

    def run(ctx):
        rc = ctx.lib.mh_rebin(ctx.at(0), ctx.p(ctx.u64(in_off)), ctx.p(ctx.u64(REBIN_LENS)), C, max(REBIN_LENS), r, int(sat), ctx.at(0),
                              ctx.p(ctx.u64(out_off)), None)
        assert rc == 0, ctx.lib.mh_last_error()
    s.run = run
    return s


for _which in ("in", "out"):
    for _r in REBIN_R:
        for _sat in (1, 0):
            _case("rebin", "mh_rebin", _which + "_off", "offset", "lens %r, r = %d" % (REBIN_LENS, _r), build_rebin, _which, _r, _sat)


# =====================================================================================================================
# mh_deinterleave, mh_interleave
# =====================================================================================================================
TR_T, TR_C, TR_SLOT = 300, 130, 320


def build_transpose(entry):
    """T = 300, C = 130 (two strips of 128, one cut): odd channels far, even ones low; channel c owns slot c of a block of
    320-byte slots, so the alias of an odd channel is its own, otherwise unused, slot of the low block"""
    rng = _rng(entry)
    s = Setup("A", Image())
    x = rng.randint(0, 256, size=(TR_T, TR_C)).astype(np.uint8)
    off = [_off(0x200000 + c * TR_SLOT, c % 2 == 1) for c in range(TR_C)]
    tm = 0x100000 + 1
    if entry == "mh_deinterleave":
        s.read("in", (), x, base=tm)
        outs = [s.write("out_off", _table_terms(off[c]), TR_T) for c in range(TR_C)]
        s.seal()
        for c in range(TR_C):
            s.expect(outs[c], x[:, c])
    else:
        for c in range(TR_C):
            s.read("in_off", _table_terms(off[c]), x[:, c])
        out = s.write("out", (), TR_T * TR_C, base=tm)
        s.seal()
        s.expect(out, x)
    s.crossing = [("off[%d]" % c, off[c], "bytes") for c in range(1, TR_C, 2)]

    def run(ctx):
        if entry == "mh_deinterleave":
            rc = ctx.lib.mh_deinterleave(ctx.at(tm), TR_T, TR_C, ctx.at(0), ctx.p(ctx.u64(off)), None)
        else:
            rc = ctx.lib.mh_interleave(ctx.at(0), ctx.p(ctx.u64(off)), TR_T, TR_C, ctx.at(tm), None)
        assert rc == 0, ctx.lib.mh_last_error()
    s.run = run
    return s


_case("transpose", "mh_deinterleave", "out_off", "offset", "T = 300, C = 130", build_transpose, "mh_deinterleave")
_case("transpose", "mh_interleave", "in_off", "offset", "T = 300, C = 130", build_transpose, "mh_interleave")


# =====================================================================================================================
# mh_synth_poisson
# =====================================================================================================================
SYNTH_LENS = (1, 4097, 70000)


def build_synth():
    import oracle
    rng = _rng("synth")
    s = Setup("A", Image())
    C = len(SYNTH_LENS)
    near = [0x100000 * (c + 1) + 16 for c in range(C)]
    off = [_off(near[c], c > 0) for c in range(C)]
    thr = np.sort(rng.randint(0, 65536, size=(C, 15)), axis=1).astype(np.uint32).reshape(-1)
    seed = 77
    outs = [s.write("ch_off", _table_terms(off[c]), SYNTH_LENS[c]) for c in range(C)]
    s.seal()
    want = oracle.c.synth(np.array(near, np.uint64), np.array(SYNTH_LENS, np.uint64), thr, seed)     # rebased offsets
    for c in range(C):
        s.expect(outs[c], want[near[c]:near[c] + SYNTH_LENS[c]])
    s.crossing = [("ch_off[%d]" % c, off[c], "bytes") for c in range(1, C)]
    s.rules.append(("the samples are not all alike", len(set(want[near[2]:near[2] + 70000].tolist())) > 3))

    def run(ctx):
        rc = ctx.lib.mh_synth_poisson(ctx.at(0), ctx.p(ctx.u64(off)), ctx.p(ctx.u64(SYNTH_LENS)), C, max(SYNTH_LENS),
                                      ctx.p(ctx.dev(thr.view(np.int32))), seed, None)
        assert rc == 0, ctx.lib.mh_last_error()
    s.run = run
    return s


_case("synth", "mh_synth_poisson", "ch_off", "offset", "lens %r" % (SYNTH_LENS,), build_synth)


# =====================================================================================================================
# mh_reduce_rows, mh_power_draws
# =====================================================================================================================
REDUCE_LENS = (7, 129, 1000)


def build_reduce_rows():
    """row_off counts doubles: >= 2^29 of them puts the bytes past 2^32"""
    rng = _rng("reduce")
    s = Setup("A", Image())
    first = (1 << 29) + 0x1003
    row_off = np.concatenate([[0], np.cumsum(REDUCE_LENS)]).astype(np.int64) + first
    rows = [rng.standard_normal(n) * 10.0 ** rng.randint(-3, 6, size=n) for n in REDUCE_LENS]
    for i, v in enumerate(rows):
        s.read("row_off", _table_terms(row_off[i], 8), v.astype("<f8"), decoy=(1.0 - v).astype("<f8"))
    s.seal()
    s.crossing = [("8 * row_off[%d]" % i, 8 * int(row_off[i]), "bytes") for i in range(len(rows))]
    s.rules.append(("row_off >= 2^29 doubles", int(row_off[0]) >= 1 << 29))

    def run(ctx):
        sm, mx = ctx.canary(len(rows) + 2, np.float64), ctx.canary(len(rows) + 2, np.float64)
        rc = ctx.lib.mh_reduce_rows(ctx.at(0), ctx.p(ctx.u64(row_off)), len(rows), ctx.p(sm, 1), ctx.p(mx, 1), None)
        assert rc == 0, ctx.lib.mh_last_error()
        ctx.framed(sm, 1, np.array([np.sum(v) for v in rows]), "sum")
        ctx.framed(mx, 1, np.array([np.max(v) for v in rows]), "max")
    s.run = run
    return s


_case("analysis", "mh_reduce_rows", "row_off", "offset", "rows of %r doubles" % (REDUCE_LENS,), build_reduce_rows)

DRAWS_Z, DRAWS_NBR = 290, 61


def build_power_draws(kind):
    """x_stride counts doubles.  value: 2^29 + 5 with 2 draws (a third would lie behind the arena); product: 2^28 + 3 with
    3 draws, the third at element 2^29 + 6"""
    rng = _rng("draws", kind)
    s = Setup("A", Image())
    stride, nd = ((1 << 29) + 5, 2) if kind == "value" else ((1 << 28) + 3, 3)
    br = rng.uniform(100.0, 3000.0, DRAWS_NBR)
    idx = rng.randint(0, DRAWS_NBR, size=(DRAWS_Z, nd)).astype(np.int32)      # [Z][draw]
    ce, pc, sp = 20e-9, DRAWS_Z * 0.96e-6, 0.1618e-3
    x0 = rng.uniform(0.0, 1e-3, nd)
    base = 0x30008
    outs = [s.write("x_stride", (Term(d, stride, 8),), 8, base=base, initial=np.array([x0[d]], "<f8")) for d in range(nd)]
    s.seal()
    for d in range(nd):
        temp = ce * np.sum(br[idx[:, d]]) + pc + sp            # left to right, as the reference's line evaluates
        s.expect(outs[d], np.array([x0[d] + temp], "<f8"))
    s.crossing = [("8 * %d * x_stride" % (nd - 1), 8 * (nd - 1) * stride, "bytes")]
    s.rules.append(("the last draw's element index >= 2^29", (nd - 1) * stride >= 1 << 29))
    if kind == "product":
        s.rules.append(("8 * x_stride itself is below 2^32", 8 * stride < FAR))

    def run(ctx):
        rc = ctx.lib.mh_power_draws(ctx.p(ctx.dev(br)), DRAWS_NBR, ctx.p(ctx.dev(idx)), DRAWS_Z, nd, ce, pc, sp, ctx.at(base), stride, None)
        assert rc == 0, ctx.lib.mh_last_error()
    s.run = run
    return s


for _k in ("value", "product"):
    _case("analysis", "mh_power_draws", "x_stride", _k, "Z = 290, %d draws" % (2 if _k == "value" else 3), build_power_draws, _k)


# =====================================================================================================================
# mh_sweep_create / mh_sweep_run
# =====================================================================================================================
SWEEP_LENS = (5, 1025, 131072 + 77)


def build_sweep():
    rng = _rng("sweep")
    s = Setup("A", Image())
    C = len(SWEEP_LENS)
    chans = [_counts(rng, T, float(np.exp(rng.uniform(-2, 2)))) for T in SWEEP_LENS]
    near = [0x100000 * (c + 1) for c in range(C)]
    off = [_off(near[c], c > 0) for c in range(C)]
    for c in range(C):
        s.read("ch_off", _table_terms(off[c]), chans[c])
    s.seal()
    s.crossing = [("ch_off[%d]" % c, off[c], "bytes") for c in range(1, C)]

    def run(ctx):
        import oracle
        from muahuff import sclv, sweep
        sw = sweep.SweepHist(np.array(off, np.uint64), np.array(SWEEP_LENS, np.uint64)).run(ctx.arena)
        idx = np.arange(C)
        data, o0, ln = oracle.c.flatten(chans)                   # the yardstick's channels, rebased
        for S in (10, 3):
            tab = sclv.table(S)
            want = np.stack([np.bincount(np.minimum(x, S - 1), minlength=S) for x in chans])
            assert np.array_equal(sw.train_hist(idx, S), want), S
            for h in (2, 6, 10):
                for approx in (True, False):
                    v = sw.validation(idx, S, h, approx)
                    om = oracle.c.measure(data, o0, ln, oracle.c.Params(S, h, int(approx), 0, tab))
                    assert np.array_equal(v["post"].astype(np.uint64), om["post_mapped"]), (S, h, approx)
                    assert np.array_equal(v["cal"].astype(np.uint32), om["cal_sorted"]), (S, h, approx)
                    assert np.array_equal(v["skipped"], om["skipped"]) and np.array_equal(v["cutoff"].astype(np.uint64), om["cutoff"])
        sw.close()
    s.run = run
    return s


_case("sweep", "mh_sweep_create / mh_sweep_run", "ch_off", "offset", "lens %r" % (SWEEP_LENS,), build_sweep)


# =====================================================================================================================
# mhi_seg_crc32 (byte-far; the word-far case is with arena W below)
# =====================================================================================================================
CRC_WORDS = (0, 1, 255, 256, 2051)


def _crc_layout(first_word):
    """segments at any word: gaps of 1, 0, 3, 2 words between them"""
    off, at = [], first_word
    for n, gap in zip(CRC_WORDS, (1, 0, 3, 2, 0)):
        off.append(at)
        at += n + gap
    return off


def build_crc(form, arena="A"):
    rng = _rng("crc", form, arena)
    size = ARENA_BYTES if arena == "A" else ARENA_W_BYTES
    s = Setup(arena, Image(size))
    off = _crc_layout((1 << 30) + 0x4001 if arena == "A" else FAR + 0x4001)
    segs = [rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype("<u4") for n in CRC_WORDS]
    for i, w in enumerate(segs):
        if w.size:
            s.read("seg_off", _table_terms(off[i], 4), w)
    s.seal()
    want = np.array([zlib.crc32(w.tobytes()) if w.size else 0 for w in segs], np.uint32)
    listed = [4, 0, 2] if form == "seg_idx" else list(range(len(segs)))
    s.crossing = [("4 * seg_off[%d]" % i, 4 * off[i], "bytes") for i in range(len(segs))]
    if arena == "W":
        s.crossing += [("seg_off[%d]" % i, off[i], "words") for i in range(len(segs))]
    s.rules.append(("the payload is 4-byte aligned and holds every segment", all(4 * (o + n) <= size for o, n in zip(off, CRC_WORDS))))

    def run(ctx):
        n = len(segs)
        crc = ctx.canary(n + 2, np.uint32)
        bad = ctx.dev(np.array([0, -1], np.int64))
        d_idx = ctx.u64(listed) if form == "seg_idx" else None
        args = (ctx.at(0), size // 4, ctx.p(ctx.u64(off)), ctx.p(ctx.u64(CRC_WORDS)), n, ctx.p(d_idx),
                len(listed) if form == "seg_idx" else 0)
        rc = ctx.ilib.mhi_seg_crc32(*args, ctx.p(crc, 1), None, None, None)
        assert rc == 0, ctx.ilib.mhi_last_error()
        got = ctx.host(crc)
        exp = np.full(n + 2, got.dtype.type(0xA5A5A5A5))
        exp[1 + np.array(listed)] = want[listed]
        assert np.array_equal(got, exp), (got, exp)
        rc = ctx.ilib.mhi_seg_crc32(*args, None, ctx.p(ctx.dev(want.view(np.int32))), ctx.p(bad), None)      # the verify form
        assert rc == 0, ctx.ilib.mhi_last_error()
        assert ctx.host(bad).tolist() == [0, -1]
    s.run = run
    return s


for _f in ("all", "seg_idx"):
    _case("crc", "mhi_seg_crc32", "seg_off (bytes)", "offset", "segments of %r words" % (CRC_WORDS,), build_crc, _f)


# =====================================================================================================================
# mhi_excess_apply
# =====================================================================================================================
def apply_ref(base, pos, val, first, last, start, stop, r, lead, bits):
    """int64 [n_rows, elements]: row i takes the entries [first[i], last[i])"""
    out = base.astype(np.int64).copy()
    for i in range(out.shape[0]):
        for k in range(first[i], last[i]):
            if start <= pos[k] < stop:
                out[i, (pos[k] - start + lead) // r] += val[k]
    return np.minimum(out, 255) if bits == 8 else out


def build_apply(kind, r, bits):
    """row_value: 2 rows, row_stride = 2^32 + 36.  row_product: 3 rows, row_stride = 2^31 + 4100.  col_product: a
    time-major target of 2 rows and 3 elements, col_stride = 2^31 + 4, row_stride = one element"""
    rng = _rng("apply", kind, r, bits)
    s = Setup("A", Image())
    e = bits // 8
    if kind == "col_product":
        n_rows, rs, cs = 2, e, STRIDE_PRODUCT + 4
        start, stop, lead = (10, 12, 1) if r == 1 else (10, 21, 2)
    else:
        n_rows, rs, cs = (2, STRIDE_VALUE + 36, e) if kind == "row_value" else (3, STRIDE_PRODUCT + 4100, e)
        start, stop, lead = 10, 50, 3
    E = ceil_div(stop - start + lead, r)
    pos, val, first, last = [], [], [], []
    for i in range(n_rows):                    # a handful of entries per row, ascending, two of them outside [start, stop)
        inside = np.sort(rng.choice(np.arange(start, stop), size=min(6, stop - start), replace=False))
        p = np.concatenate([[start - 3], inside, [stop + 1]])
        first.append(len(pos))
        pos += p.tolist()
        val += [17, 254] + rng.randint(1, 255, size=p.size - 2).tolist()      # the first entry inside takes an element past 255
        last.append(len(pos))
    base0 = rng.randint(2, 60, size=(n_rows, E))
    want = apply_ref(base0, pos, val, first, last, start, stop, r, lead, bits)
    at = 0x40000
    dt = np.uint8 if e == 1 else "<u4"
    outs = []
    for i in range(n_rows):
        if kind == "col_product":
            outs.append([s.write("col_stride", (Term(i, rs), Term(b, cs)), e, base=at, initial=np.array([base0[i, b]], dt))
                         for b in range(E)])
        else:
            outs.append([s.write("row_stride", (Term(i, rs),), E * e, base=at, initial=base0[i].astype(dt))])
    s.seal()
    for i in range(n_rows):
        if kind == "col_product":
            for b in range(E):
                s.expect(outs[i][b], np.array([want[i, b]], dt))
        else:
            s.expect(outs[i][0], want[i].astype(dt))
    if kind == "col_product":
        s.crossing = [("(elements - 1) * col_stride", (E - 1) * cs, "bytes")]
        s.rules += [("3 elements", E == 3), ("col_stride itself is below 2^32", cs < FAR)]
    else:
        s.crossing = [("(n_rows - 1) * row_stride", (n_rows - 1) * rs, "bytes")]
        s.rules.append(("far value: row_stride >= 2^32" if kind == "row_value" else "far product: row_stride < 2^32",
                        (rs >= FAR) == (kind == "row_value")))
    s.rules += [("32-bit strides are multiples of 4", e == 1 or (rs % 4 == 0 and cs % 4 == 0 and at % 4 == 0)),
                ("the call changes something", not np.array_equal(want, base0)),
                ("8 bits saturate", bits != 8 or (apply_ref(base0, pos, val, first, last, start, stop, r, lead, 32) > 255).any())]

    def run(ctx):
        rc = ctx.ilib.mhi_excess_apply(ctx.p(ctx.dev(np.array(pos, np.uint32).view(np.int32))), ctx.p(ctx.dev(np.array(val, np.uint8))),
                                       len(pos), ctx.p(ctx.u64(first)), ctx.p(ctx.u64(last)), n_rows, start, stop, r, lead, ctx.at(at),
                                       bits, rs, cs, None)
        assert rc == 0, ctx.ilib.mhi_last_error()
    s.run = run
    return s


for _k in ("row_value", "row_product", "col_product"):
    for _r in (1, 5):
        for _b in (8, 32):
            _case("apply", "mhi_excess_apply", _k.split("_")[0] + "_stride", _k.split("_")[1], "r = %d, %d bits" % (_r, _b),
                  build_apply, _k, _r, _b)


# =====================================================================================================================
# mhi_windows
# =====================================================================================================================
WIN_COLS, WIN_N = 5000, 9
WIN_FORMS = ((100, 1), (100, 7), (330, 100))           # a lane per 16 samples, a staged tile, a wave per bin


def windows_ref(rec, offs, W, r):
    """int64 [n, rows, nb]: bin b of window k = sum of rec[:, offs[k] + b*r : offs[k] + min(b*r + r, W)]"""
    nb = ceil_div(W, r)
    g = rec[:, np.asarray(offs, np.int64)[:, None] + np.arange(W)]
    g = np.concatenate([g, np.zeros(g.shape[:2] + (nb * r - W,), np.uint8)], axis=2)
    return g.reshape(g.shape[0], g.shape[1], nb, r).sum(axis=3, dtype=np.int64).transpose(1, 0, 2)


def _win_strides(kind):
    """(rows, input row_stride, a 32-bit output stride, a 64-bit output stride)"""
    if kind == "value":
        return 2, STRIDE_VALUE + 37, STRIDE_VALUE + 36, STRIDE_VALUE + 40
    return 3, STRIDE_PRODUCT + 4099, STRIDE_PRODUCT + 4100, STRIDE_PRODUCT + 4104


def _win_input(s, rng, kind):
    rows, rs, _o4, _o8 = _win_strides(kind)
    rec = _counts(rng, rows * WIN_COLS, 0.8).reshape(rows, WIN_COLS)
    at = 0x10001                                           # an odd first byte
    for i in range(rows):
        s.read("row_stride", (Term(i, rs),), rec[i], base=at)
    offs = rng.randint(0, WIN_COLS - 400, size=WIN_N).astype(np.int64)
    offs = offs - offs % 16 + np.arange(WIN_N) % 16
    offs[1] = offs[0]
    return rec, at, rows, rs, offs


def build_windows(mode, far, kind, W, r):
    """The input rows are far in every case.  far names the output stride that crosses as well:
    stack / out_row_stride  9 windows through a permuting win_idx, 8 and 32 bits (two calls, two targets)
    stack / out_win_stride  slots 0 .. rows - 1 only (slot * out_win_stride must stay inside the arena): as many windows
                            as rows, permuted; 8 and 32 bits
    sum / out_row_stride + sq_row_stride   9 windows, with the squares"""
    rng = _rng("windows", mode, far, kind, W, r)
    s = Setup("A", Image())
    rec, at, rows, rs, offs = _win_input(s, rng, kind)
    _rows, _rs, o4, o8 = _win_strides(kind)
    nb = ceil_div(W, r)
    if mode == "stack":
        n = WIN_N if far == "out_row_stride" else rows
        offs = offs[:n]
        perm = rng.permutation(n)
        want = windows_ref(rec, offs, W, r)                   # [n, rows, nb]
        targets = []
        for bits, tb in ((8, 0x2000000), (32, 0x4000000)):
            e = bits // 8
            stride = o4 if e == 4 else o4 + 1                 # the 8-bit target takes an odd stride
            if far == "out_row_stride":
                ws, ors = nb * e + 4 * 5, stride              # the slots of one row side by side
            else:
                ws, ors = stride, nb * e + 4 * 3
            acc = [[s.write(far, (Term(sl, ws), Term(i, ors)), nb * e, base=tb) for i in range(rows)] for sl in range(n)]
            targets.append((bits, tb, ws, ors, acc))
        s.seal()
        for bits, tb, ws, ors, acc in targets:
            for k in range(n):
                for i in range(rows):
                    v = want[k, i]
                    s.expect(acc[perm[k]][i], np.minimum(v, 255).astype(np.uint8) if bits == 8 else v.astype("<u4"))
        top = (rows - 1) * max(t[3] for t in targets) if far == "out_row_stride" else (n - 1) * max(t[2] for t in targets)
        s.crossing = [("(rows - 1) * row_stride", (rows - 1) * rs, "bytes"), ("the last index * %s" % far, top, "bytes")]
        s.rules.append(("32-bit strides are multiples of 4",
                        all(t[2] % 4 == 0 and t[3] % 4 == 0 and t[1] % 4 == 0 for t in targets if t[0] == 32)))
    else:
        n = WIN_N
        want = windows_ref(rec, offs, W, r)
        tot, sq = want.sum(axis=0), (want * want).sum(axis=0)
        ta, tq = 0x2000000, 0x4000000
        a_out = [s.write("out_row_stride", (Term(i, o4),), 4 * nb, base=ta) for i in range(rows)]
        a_sq = [s.write("sq_row_stride", (Term(i, o8),), 8 * nb, base=tq) for i in range(rows)]
        s.seal()
        for i in range(rows):
            s.expect(a_out[i], tot[i].astype("<u4"))
            s.expect(a_sq[i], sq[i].astype("<u8"))
        s.crossing = [("(rows - 1) * row_stride", (rows - 1) * rs, "bytes"), ("(rows - 1) * out_row_stride", (rows - 1) * o4, "bytes"),
                      ("(rows - 1) * sq_row_stride", (rows - 1) * o8, "bytes")]
        s.rules += [("out_row_stride % 4, sq_row_stride % 8", o4 % 4 == 0 and o8 % 8 == 0 and ta % 4 == 0 and tq % 8 == 0),
                    ("n_win * 255 * min(r, W) < 2^32", n * 255 * min(r, W) < FAR)]
    s.rules += [("row_stride >= cols", rs >= WIN_COLS), ("every window lies inside the rows", int(offs.max()) + W <= WIN_COLS),
                ("far value" if kind == "value" else "far product", (rs >= FAR) == (kind == "value"))]

    def run(ctx):
        d_off = ctx.u64(offs)
        if mode == "stack":
            for bits, tb, ws, ors, _acc in targets:
                bad = ctx.dev(np.array([0, -1], np.int64))
                rc = ctx.ilib.mhi_windows(ctx.at(at), rs, rows, WIN_COLS, ctx.p(d_off), ctx.p(ctx.u64(perm)), n, n, W, r, 0, ctx.at(tb),
                                          bits, ws, ors, None, 0, 0, ctx.p(bad), None)
                assert rc == 0, ctx.ilib.mhi_last_error()
                assert ctx.host(bad).tolist() == [0, -1]
        else:
            bad = ctx.dev(np.array([0, -1], np.int64))
            rc = ctx.ilib.mhi_windows(ctx.at(at), rs, rows, WIN_COLS, ctx.p(d_off), None, n, 0, W, r, 1, ctx.at(ta), 32, 0, o4,
                                      ctx.at(tq), o8, 0, ctx.p(bad), None)
            assert rc == 0, ctx.ilib.mhi_last_error()
            assert ctx.host(bad).tolist() == [0, -1]
    s.run = run
    return s


for _W, _r in WIN_FORMS:
    for _k in ("value", "product"):
        _case("windows", "mhi_windows", "row_stride + out_row_stride (STACK)", _k, "W = %d, r = %d" % (_W, _r), build_windows,
              "stack", "out_row_stride", _k, _W, _r)
        _case("windows", "mhi_windows", "row_stride + out_win_stride (STACK)", _k, "W = %d, r = %d" % (_W, _r), build_windows,
              "stack", "out_win_stride", _k, _W, _r)
        _case("windows", "mhi_windows", "row_stride + out_row_stride + sq_row_stride (SUM)", _k, "W = %d, r = %d" % (_W, _r),
              build_windows, "sum", "out_row_stride", _k, _W, _r)


def build_windows_public(kind):
    """windows.gather / windows.psth on an as_strided view of the arena: the public route to a far row_stride"""
    rng = _rng("windows public", kind)
    s = Setup("A", Image())
    rec, at, rows, rs, offs = _win_input(s, rng, kind)
    s.seal()
    s.crossing = [("(rows - 1) * row_stride", (rows - 1) * rs, "bytes")]
    s.rules.append(("row_stride >= cols", rs >= WIN_COLS))

    def run(ctx):
        from muahuff import windows
        view = ctx.arena.as_strided((rows, WIN_COLS), (rs, 1), at)
        for W, r in WIN_FORMS:
            want = windows_ref(rec, offs, W, r)
            assert np.array_equal(windows.gather(view, offs, W, r, saturate=False).cpu().numpy(), want), (W, r)
            assert np.array_equal(windows.gather(view, offs, W, r).cpu().numpy(), np.minimum(want, 255)), (W, r)
            t, q = windows.psth(view, offs, W, r, moments=2)
            assert np.array_equal(t.cpu().numpy(), want.sum(axis=0)) and np.array_equal(q.cpu().numpy(), (want * want).sum(axis=0)), (W, r)
    s.run = run
    return s


for _k in ("value", "product"):
    _case("windows", "windows.gather / windows.psth", "row_stride", _k, "every form", build_windows_public, _k)


# =====================================================================================================================
# mhi_gram
# =====================================================================================================================
GRAM_COLS, GRAM_NEAR = 333, 5
GRAM_A, GRAM_B, GRAM_G = 0x10001, 0x40003, 0x80000         # the first byte of a and of b (odd), of gram (8-byte aligned)
GRAM_FAR_D = 0xC0008                                       # a far base pointer is 2^32 + this


def _gram_strides(kind):
    """(rows of the far operand, its row stride in bytes, the far gram_row_stride)"""
    if kind == "value":
        return 2, STRIDE_VALUE + 5, STRIDE_VALUE + 40
    return 3, STRIDE_PRODUCT + 4096 + 3, STRIDE_PRODUCT + 4104


def build_gram(far, kind, form, accumulate):
    """cols = 333; the near operand has 5 rows, the far one 2 (far value) or 3 (far product); a and b begin at an odd
    byte and near rows are an even number of bytes apart, so each begins at an odd byte; the far strides are odd, so far
    rows take both parities, none on a 16-byte boundary.
    a_row_stride / b_row_stride  the rows of that operand are far; "sym": b NULL, so a_row_stride strides both operands
    gram_row_stride              the result's rows are far: accumulate = 0 zeroes them through the 2-D memset whose pitch
                                 is the far stride (canary before the call), accumulate = 1 adds to `initial` values
    sum_a / sum_b / gram         (kind "offset") that base pointer is 2^32 + GRAM_FAR_D, canary at GRAM_FAR_D
    The mirror store of the symmetric form, gram + j * gram_row_stride + 8 i, happens only off the diagonal TILE, i.e. for
    i >= 128: times a far stride that lies behind the arena, as an index >= 2 times a far value does.  The symmetric
    cases here are one tile: their far rows are written by the i * gram_row_stride store alone."""
    rng = _rng("gram", far, kind, form, accumulate)
    s = Setup("A", Image())
    n, in_far, g_far = _gram_strides(kind) if kind != "offset" else (3, None, None)
    ra, rb = (GRAM_NEAR, n) if far == "b_row_stride" else (n, n if form == "sym" else GRAM_NEAR)
    sym = form == "sym"
    a_rs = in_far if far == "a_row_stride" else GRAM_COLS + 5
    b_rs = a_rs if sym else in_far if far == "b_row_stride" else GRAM_COLS + 9
    g_rs = g_far if far == "gram_row_stride" else 8 * (rb + 1)
    x = _counts(rng, ra * GRAM_COLS).reshape(ra, GRAM_COLS)
    y = x if sym else _counts(rng, rb * GRAM_COLS).reshape(rb, GRAM_COLS)
    for i in range(ra):
        s.read("a_row_stride", (Term(i, a_rs),), x[i], base=GRAM_A)
    if not sym:
        for j in range(rb):
            s.read("b_row_stride", (Term(j, b_rs),), y[j], base=GRAM_B)
    g0 = rng.randint(1, 1 << 40, size=(ra, rb)).astype("<i8")
    s0 = rng.randint(1, 1 << 40, size=(2, max(ra, rb))).astype("<i8")
    lead = (Term(1, FAR + GRAM_G),) if far == "gram" else ()
    g_at = 0 if far == "gram" else GRAM_G
    outs = [s.write("gram" if far == "gram" else "gram_row_stride", lead + (Term(i, g_rs),), 8 * rb, base=g_at,
                    initial=g0[i] if accumulate else None) for i in range(ra)]
    far_sum = None
    if far in ("sum_a", "sum_b"):
        k = ra if far == "sum_a" else rb
        far_sum = s.write(far, _table_terms(FAR + GRAM_FAR_D), 8 * k, initial=s0[int(far == "sum_b"), :k] if accumulate else None)
    s.seal()
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    G, sa, sb = xi @ yi.T, xi.sum(1), yi.sum(1)
    if accumulate:
        G, sa, sb = G + g0, sa + s0[0, :ra], sb + s0[1, :rb]
    for i in range(ra):
        s.expect(outs[i], G[i].astype("<i8"))
    if far_sum is not None:
        s.expect(far_sum, (sa if far == "sum_a" else sb).astype("<i8"))
    top = {"a_row_stride": ("(a_rows - 1) * a_row_stride", (ra - 1) * a_rs), "b_row_stride": ("(b_rows - 1) * b_row_stride", (rb - 1) * b_rs),
           "gram_row_stride": ("(a_rows - 1) * gram_row_stride", (ra - 1) * g_rs), "gram": ("gram - base", FAR + GRAM_G),
           "sum_a": ("sum_a - base", FAR + GRAM_FAR_D), "sum_b": ("sum_b - base", FAR + GRAM_FAR_D)}[far]
    s.crossing = [top + ("bytes",)]
    far_rs = {"a_row_stride": a_rs, "b_row_stride": b_rs, "gram_row_stride": g_rs}.get(far)
    s.rules += [("a_rows, b_rows, cols >= 1; cols < 2^40", min(ra, rb, GRAM_COLS) >= 1 and GRAM_COLS < 1 << 40),
                ("a_row_stride >= cols, b_row_stride >= cols", a_rs >= GRAM_COLS and b_rs >= GRAM_COLS),
                ("gram and gram_row_stride are multiples of 8", GRAM_G % 8 == 0 and FAR % 8 == 0 and g_rs % 8 == 0),
                ("gram_row_stride >= 8 * b_rows", g_rs >= 8 * rb), ("sum_a and sum_b are multiples of 8", GRAM_FAR_D % 8 == 0),
                ("accumulate is 0 or 1", accumulate in (0, 1)),
                ("a and b begin at an odd byte, no row on a 16-byte boundary, every near row at an odd byte",
                 GRAM_A % 2 == 1 and GRAM_B % 2 == 1 and all((GRAM_A + i * a_rs) % 16 for i in range(ra))
                 and all((GRAM_B + j * b_rs) % 16 for j in range(rb))
                 and (far == "a_row_stride" or all((GRAM_A + i * a_rs) % 2 for i in range(ra)))
                 and (far == "b_row_stride" or sym or all((GRAM_B + j * b_rs) % 2 for j in range(rb)))),
                ("one tile: no mirror store", max(ra, rb) <= 128),
                ("a pitched result: an overwrite call zeroes it with the 2-D memset", ra > 1 and g_rs != 8 * rb),
                ("far value" if kind == "value" else "far product" if kind == "product" else "a far base pointer",
                 far_rs is None if kind == "offset" else (far_rs >= FAR) == (kind == "value"))]

    def run(ctx):
        def small(k, init, skip):
            if skip:
                return None
            t = ctx.canary(k + 2, np.int64)
            if accumulate:
                t[1:1 + k] = ctx.dev(init[:k])
            return t
        d_sa, d_sb = small(ra, s0[0], far == "sum_a"), small(rb, s0[1], far == "sum_b")
        p_sa = ctx.at(FAR + GRAM_FAR_D) if far == "sum_a" else ctx.p(d_sa, 1)
        p_sb = ctx.at(FAR + GRAM_FAR_D) if far == "sum_b" else ctx.p(d_sb, 1)
        rc = ctx.ilib.mhi_gram(ctx.at(GRAM_A), a_rs, ra, None if sym else ctx.at(GRAM_B), 0 if sym else b_rs, 0 if sym else rb, GRAM_COLS,
                               ctx.at(FAR + GRAM_G if far == "gram" else GRAM_G), g_rs, p_sa, p_sb, accumulate, None)
        assert rc == 0, ctx.ilib.mhi_last_error()
        ctx.sync()
        if d_sa is not None:
            ctx.framed(d_sa, 1, sa.astype("<i8"), "sum_a")
        if d_sb is not None:
            ctx.framed(d_sb, 1, sb.astype("<i8"), "sum_b")
    s.run = run
    return s


for _k in ("value", "product"):
    _case("gram", "mhi_gram", "a_row_stride", _k, "%d x 5 rows, cols = 333" % (2 if _k == "value" else 3), build_gram, "a_row_stride", _k, "cross", 0)
    _case("gram", "mhi_gram", "b_row_stride", _k, "5 x %d rows, cols = 333" % (2 if _k == "value" else 3), build_gram, "b_row_stride", _k, "cross", 0)
    for _acc in (0, 1):
        _case("gram", "mhi_gram", "gram_row_stride", _k, "%d x 5 rows, cols = 333, accumulate = %d" % (2 if _k == "value" else 3, _acc),
              build_gram, "gram_row_stride", _k, "cross", _acc)
_case("gram", "mhi_gram", "a_row_stride (symmetric)", "product", "3 rows, cols = 333", build_gram, "a_row_stride", "product", "sym", 0)
_case("gram", "mhi_gram", "gram_row_stride (symmetric)", "product", "3 rows, cols = 333", build_gram, "gram_row_stride", "product", "sym", 0)
for _far in ("sum_a", "sum_b", "gram"):
    for _acc in (0, 1):
        _case("gram", "mhi_gram", _far, "offset", "3 x 5 rows, cols = 333, accumulate = %d" % _acc, build_gram, _far, "offset", "cross", _acc)


# =====================================================================================================================
# mhi_unbin_count / mhi_unbin_emit (CSR) and mhi_excess_count / mhi_excess_emit (ROWS): row_off far
# =====================================================================================================================
ROWS3, ROW_COLS = 3, CHUNK + 5
ROW_STARTS = (1, 3, 7)                                  # odd first bytes


def _row_input(s, rng, rate, frame):
    """3 rows of 16384 + 5 columns, row 0 low and the others far, framed by `frame` bytes (what a read outside a row finds)"""
    x = np.minimum(rng.poisson(rate, size=(ROWS3, ROW_COLS)), 255).astype(np.uint8)
    x[:, 0], x[:, -1], x[:, CHUNK - 1], x[:, CHUNK] = 255, 9, 3, 4      # the first and last byte of every row and tile
    near = [0x100000 * (i + 1) + ROW_STARTS[i] for i in range(ROWS3)]
    off = [_off(near[i], i > 0) for i in range(ROWS3)]
    for i in range(ROWS3):
        s.pre.put(off[i] - 64, np.full(ROW_COLS + 128, frame, np.uint8))
        s.read("row_off", _table_terms(off[i]), x[i])
    s.crossing = [("row_off[%d]" % i, off[i], "bytes") for i in range(1, ROWS3)]
    return x, off


def build_unbin():
    rng = _rng("unbin")
    s = Setup("A", Image())
    x, off = _row_input(s, rng, 0.02, 255)
    s.seal()
    origin, period, phase = 1 << 40, 30, 7

    def run(ctx):
        from tests import test_gpu_unbin as ub
        want, ev = ub.csr_oracle(x, origin, period, phase)
        o = ub.Out(ctx.mh, ub.CSR, ROWS3, ROW_COLS, want.size)
        o.call(ctx.mh, ctx.arena, ctx.u64(off), origin, period, phase)
        ctx.sync()
        o.check(want, ev, tag="far row_off")
    s.run = run
    return s


def build_excess():
    rng = _rng("excess")
    s = Setup("A", Image())
    x, off = _row_input(s, rng, 1.2, 255)
    s.seal()
    thr = 2
    lo, hi = np.array([0, 5, CHUNK - 1]), np.array([ROW_COLS, CHUNK + 1, ROW_COLS + 9])

    def run(ctx):
        from tests import test_gpu_excess as ex
        want = ex.oracle(list(x), thr, lo, hi)
        o = ex.Out(ctx.mh, ex.ROWS, ROWS3, ROW_COLS, len(want[1]))
        o.call(ctx.mh, ctx.arena, ctx.u64(off), ctx.u64(lo), ctx.u64(hi), thr)
        ctx.sync()
        o.check(want, tag="far row_off")
        assert len(want[1]) > 1000
    s.run = run
    return s


_case("unbin", "mhi_unbin_count / mhi_unbin_emit (CSR)", "row_off", "offset", "3 rows of 16384 + 5 columns", build_unbin)
_case("excess", "mhi_excess_count / mhi_excess_emit (ROWS)", "row_off", "offset", "3 rows of 16384 + 5 columns, threshold 2", build_excess)


# =====================================================================================================================
# mhi_bin_events, bits = 8: ev_off >= 2^29 ticks (ticks = the arena's base) and out_off far
# =====================================================================================================================
BIN_C, BIN_T = 3, CHUNK + 7


def _events(rng, C, T, origin, period, per_channel):
    """sorted ticks per channel with duplicates, some before the origin and some behind the last bin -> (ticks per
    channel, counts int64 [C, T])"""
    ticks, counts = [], np.zeros((C, T), np.int64)
    for c in range(C):
        t = rng.randint(origin - 5 * period, origin + (T + 5) * period, size=per_channel)
        t = np.sort(np.concatenate([t, t[:per_channel // 4], [origin, origin + T * period - 1, origin + T * period]])).astype(np.uint64)
        ticks.append(t)
        b = (t.astype(np.int64) - origin) // period
        keep = (t.astype(np.int64) >= origin) & (b < T)
        np.add.at(counts[c], b[keep], 1)
    return ticks, counts


def build_bin8():
    rng = _rng("bin8")
    s = Setup("A", Image())
    origin, period = 1000, 30
    ticks, counts = _events(rng, BIN_C, BIN_T, origin, period, 150)
    ev_off = np.concatenate([[0], np.cumsum([t.size for t in ticks])]).astype(np.int64) + (1 << 29) + 0x1001
    for c in range(BIN_C):
        other = np.sort(rng.randint(origin, origin + BIN_T * period, size=ticks[c].size)).astype("<u8")
        s.read("ev_off", _table_terms(ev_off[c], 8), ticks[c].astype("<u8"), decoy=other)
    out_off = [_off(0x2000000 + 0x100000 * c + 3, c > 0) for c in range(BIN_C)]
    outs = [s.write("out_off", _table_terms(out_off[c]), BIN_T) for c in range(BIN_C)]
    s.seal()
    for c in range(BIN_C):
        s.expect(outs[c], np.minimum(counts[c], 255).astype(np.uint8))
    s.crossing = [("8 * ev_off[%d]" % c, 8 * int(ev_off[c]), "bytes") for c in range(BIN_C)] + \
                 [("out_off[%d]" % c, out_off[c], "bytes") for c in range(1, BIN_C)]
    s.rules += [("ev_off >= 2^29 ticks", int(ev_off[0]) >= 1 << 29), ("bins with several events", counts.max() >= 2),
                ("ticks are 8-byte aligned", True)]

    def run(ctx):
        rc = ctx.ilib.mhi_bin_events(ctx.at(0), ctx.p(ctx.u64(ev_off)), BIN_C, origin, period, BIN_T, 8, ctx.at(0), ctx.p(ctx.u64(out_off)),
                                     0, None)
        assert rc == 0, ctx.ilib.mhi_last_error()
    s.run = run
    return s


_case("bin8", "mhi_bin_events (bits = 8)", "ev_off + out_off", "offset", "C = 3, T = 16384 + 7", build_bin8)


# =====================================================================================================================
# packed plans: mh_deinterleave_packed, mh_measure, mh_encode_preset, mh_interleave_packed, mh_decode_packed,
# mhi_bin_events at bits 4 / 2 -- contiguous pieces at far offsets, and chunk-blocked with chunk_stride = 2^31 + 4096
# =====================================================================================================================
PK_C, PK_T = 5, 2 * CHUNK + 5
PK_H, PK_MODE, PK_SC = 6, 1, 2
ROWS_S = {3: (1, 2, 2), 8: (1, 2, 3, 4, 5, 6, 7, 7)}
PK_S = {2: 3, 4: 8}                                       # bits -> S


def bitpack(s, bits):
    """samples (a multiple of 16 of them, each below 2^bits) -> bytes: sample i in bits [i * bits, (i + 1) * bits)"""
    per = 8 // bits
    g = np.asarray(s, np.uint32).reshape(-1, per)
    by = np.zeros(g.shape[0], np.uint32)
    for f in range(per):
        by |= g[:, f] << (bits * f)
    return by.astype(np.uint8)


def _packed_layout(bits, layout):
    """-> (ch_off, chunk_stride, [[(chunk j, byte address, pieces)] per channel])"""
    pb = 2 * bits
    cb = 1024 * pb
    npiece = ceil_div(PK_T, 16)
    if layout == "blocked":
        stride = STRIDE_PRODUCT + 4096
        off = [0x100000 + c * cb for c in range(PK_C)]
        parts = [[(j, off[c] + j * stride, min(1024, npiece - 1024 * j)) for j in range(ceil_div(npiece, 1024))] for c in range(PK_C)]
    else:
        stride = 0
        off = [_off(0x100000 * (c + 1), c > 0) for c in range(PK_C)]
        parts = [[(0, off[c], npiece)] for c in range(PK_C)]
    return off, stride, parts


def _packed_terms(off_c, j, stride):
    return (Term(1, off_c), Term(j, stride)) if stride else (Term(1, off_c),)


def _pieces(x, bits):
    """one channel's counts -> its packed pieces (the cut last piece zero-padded)"""
    n = ceil_div(x.size, 16) * 16
    v = np.zeros(n, np.uint32)
    v[:x.size] = np.minimum(x, (1 << bits) - 1)
    return bitpack(v, bits)


def _packed_crossing(s, bits, layout, off, stride, parts):
    if layout == "blocked":
        s.crossing = [("2 * chunk_stride", 2 * stride, "bytes")]
        s.rules += [("chunk_stride is a multiple of 16 and at least one packed chunk", stride % 16 == 0 and stride >= 1024 * 2 * bits),
                    ("chunk_stride itself is below 2^32", stride < FAR),
                    ("a channel of 2 chunks + 5 samples", len(parts[0]) == 3 and parts[0][2][2] == 1)]
    else:
        s.crossing = [("off[%d]" % c, off[c], "bytes") for c in range(1, PK_C)]
    s.rules.append(("off % 16 == 0", all(o % 16 == 0 for o in off)))


def build_packed(what, bits, layout):
    import oracle
    OC = oracle.c
    rng = _rng("packed", what, bits, layout)
    s = Setup("A", Image())
    S, pb = PK_S[bits], 2 * bits
    rows = np.array([ROWS_S[S]], np.uint8)
    off, stride, parts = _packed_layout(bits, layout)
    x = np.stack([_counts(rng, PK_T, float(np.exp(rng.uniform(-2, 1.5)))) for _ in range(PK_C)], axis=1)       # [T, C]
    chans = [np.ascontiguousarray(x[:, c]) for c in range(PK_C)]
    ln = np.full(PK_C, PK_T, np.uint64)
    tm = 0x8000000 + 1
    origin, period = 1000, 30
    if what in ("deinterleave", "decode", "bin"):
        if what == "deinterleave":
            s.read("in", (), x, base=tm)
        if what == "bin":
            ticks, counts = _events(rng, PK_C, PK_T, origin, period, 3000)
            chans = [np.minimum(counts[c], 255).astype(np.uint8) for c in range(PK_C)]
        clip = S - 1 if what == "decode" else 255
        outs = []
        for c in range(PK_C):
            by = _pieces(np.minimum(chans[c], clip), bits)
            for j, _addr, n in parts[c]:
                # mh_deinterleave_packed stores 16 bytes at a time: zeros up to the next multiple of 16 behind the last piece
                size = n * pb if what != "deinterleave" else (n * pb + 15) // 16 * 16
                piece = np.zeros(size, np.uint8)
                piece[:n * pb] = by[1024 * j * pb:(1024 * j + n) * pb]
                outs.append((s.write("chunk_stride" if stride else "out_off", _packed_terms(off[c], j, stride), size), piece))
        s.seal()
        for acc, piece in outs:
            s.expect(acc, piece)
    else:                                    # "encode": measure, encode_preset and interleave_packed read the pieces
        for c in range(PK_C):
            by = _pieces(chans[c], bits)
            for j, _addr, n in parts[c]:
                s.read("chunk_stride" if stride else "ch_off", _packed_terms(off[c], j, stride), by[1024 * j * pb:(1024 * j + n) * pb])
        out = s.write("out", (), PK_T * PK_C, base=tm)
        s.seal()
        s.expect(out, np.minimum(x, (1 << bits) - 1).astype(np.uint8))
    _packed_crossing(s, bits, layout, off, stride, parts)
    data, o0, _ln = OC.flatten(chans)                    # the yardstick's channels, rebased
    p = OC.Params(S, PK_H, PK_MODE, OC.WIN_FULL, rows, seg_chunks=PK_SC)

    def run(ctx):
        import torch
        d_off = ctx.u64(off)
        if what == "deinterleave":
            rc = ctx.lib.mh_deinterleave_packed(ctx.at(tm), PK_T, PK_C, bits, ctx.at(0), ctx.p(d_off), stride, None)
            assert rc == 0, ctx.lib.mh_last_error()
            return
        if what == "bin":
            ev = np.concatenate([[0], np.cumsum([t.size for t in ticks])])
            rc = ctx.ilib.mhi_bin_events(ctx.p(ctx.dev(np.concatenate(ticks))), ctx.p(ctx.u64(ev)), PK_C, origin, period, PK_T, bits,
                                         ctx.at(0), ctx.p(d_off), stride, None)
            assert rc == 0, ctx.ilib.mhi_last_error()
            return
        plan = ctx.mh.codec.Plan(np.array(off, np.uint64), ln, S, PK_H, PK_MODE, ctx.mh.WIN_FULL, rows, seg_chunks=PK_SC,
                                 input_bits=bits, chunk_stride=stride)
        om = OC.measure(data, o0, ln, p)
        oe = OC.encode_preset(data, o0, ln, p, om["peak"], om["enc"])
        pk, en = ctx.dev(om["peak"]), ctx.dev(om["enc"])
        try:
            if what == "decode":
                from muahuff.codec import Encoded
                pay = ctx.dev(oe["payload"])
                enc = Encoded(pay, None, None, pk, en, None)
                plan.decode_packed(enc, ctx.bytes)
                assert plan.decode_ok()
                return
            m = plan.measure(ctx.bytes)
            for got, want in ((m.cutoff, om["cutoff"]), (m.cal_hist, om["cal_sorted"]), (m.peak, om["peak"]), (m.enc, om["enc"]),
                              (m.post_hist, om["post_mapped"]), (m.bits, om["bits"]), (m.skipped, om["skipped"])):
                assert np.array_equal(got.cpu().numpy().astype(np.int64), want.astype(np.int64)), "mh_measure"
            e = plan.encode(ctx.bytes, preset=(pk, en))
            nseg = plan.n_segments
            assert np.array_equal(plan.segments()["off"], oe["seg"]["off"]) and plan.payload_cap_words == oe["payload"].size
            sw = e.seg_words.cpu().numpy().astype(np.uint64)[:nseg]
            assert np.array_equal(sw, oe["seg_words"]) and np.array_equal(e.ch_bits.cpu().numpy().astype(np.uint64), oe["ch_bits"])
            pay = e.payload.cpu().numpy().view(np.uint32)
            for k in range(nseg):
                o, n = int(oe["seg"]["off"][k]), int(sw[k])
                assert np.array_equal(pay[o:o + n], oe["payload"][o:o + n]), ("segment", k)
            rc = ctx.lib.mh_interleave_packed(ctx.at(0), ctx.p(d_off), PK_T, PK_C, bits, stride, ctx.at(tm), None)
            assert rc == 0, ctx.lib.mh_last_error()
            torch.cuda.synchronize()
        finally:
            plan.close()
    s.run = run
    return s


for _bits in (2, 4):
    for _lay in ("contiguous", "blocked"):
        _kind = "product" if _lay == "blocked" else "offset"
        _far = "chunk_stride" if _lay == "blocked" else "out_off / ch_off"
        _case("packed", "mh_deinterleave_packed", _far, _kind, "C = 5, T = 2 * 16384 + 5", build_packed, "deinterleave", _bits, _lay)
        _case("packed", "mh_measure, mh_encode_preset, mh_interleave_packed", _far, _kind, "C = 5, T = 2 * 16384 + 5", build_packed,
              "encode", _bits, _lay)
        _case("packed", "mh_decode_packed", _far, _kind, "C = 5, T = 2 * 16384 + 5", build_packed, "decode", _bits, _lay)
        _case("packed", "mhi_bin_events (bits = %d)" % _bits, _far, _kind, "C = 5, T = 2 * 16384 + 5", build_packed, "bin", _bits, _lay)


# =====================================================================================================================
# the byte-layout codec: mh_measure, mh_encode, mh_encode_preset read far channels; mh_decode writes them, from a
# payload whose seg_off is far in bytes (arena A) or in words (arena W)
# =====================================================================================================================
CODEC_H = 6
CODEC_LAYOUTS = {"wave": ((7, 1000, CHUNK, CHUNK + 1, 40000, 3 * CHUNK), 1),        # kernel_cells.WAVE_LAYOUTS[0]
                 "wg": ((16 * CHUNK, 13 * CHUNK + 7), 4),                          # kernel_cells.WG_LAYOUTS[3]
                 # MH_WIN_AFTER_CAL at h = 6 leaves the 16-chunk channel a window of 16 * CHUNK - 64 samples, just below
                 # MH_HEAD_MIN_WINDOW: no head segment.  One more chunk and the window begins with a revision-3 head segment
                 "wg_head": ((17 * CHUNK, 13 * CHUNK + 7), 4)}
PAYLOAD_D = 0x4000000              # the payload's bytes sit at 2^32 + PAYLOAD_D (4 * 2^32 + PAYLOAD_D in arena W)


def _codec_channels(rng, lens, S):
    chans = [_counts(rng, T, float(np.exp(rng.uniform(-2, np.log(S))))) for T in lens]
    near = [0x100000 * (c + 1) for c in range(len(lens))]
    return chans, near


def _payload_words(arena):
    return ((FAR + PAYLOAD_D) // 4) if arena == "A" else FAR + PAYLOAD_D // 4


def build_codec(what, layout, S, arena="A"):
    import oracle
    OC = oracle.c
    rng = _rng("codec", layout, S)
    size = ARENA_BYTES if arena == "A" else ARENA_W_BYTES
    s = Setup(arena, Image(size))
    lens, sc = CODEC_LAYOUTS[layout]
    C = len(lens)
    rows = np.array([ROWS_S[S]], np.uint8)
    chans, near = _codec_channels(rng, lens, S)
    off = [_off(near[c], c > 0) for c in range(C)]
    data, o0, ln = OC.flatten(chans)                      # the yardstick's channels, rebased
    mode = OC.MODE_APPROX
    p = OC.Params(S, CODEC_H, mode, OC.WIN_AFTER_CAL, rows, seg_chunks=sc)
    oe = OC.encode(data, o0, ln, p)
    s.crossing = [("ch_off[%d]" % c, off[c], "bytes") for c in range(1, C)]
    if what == "encode":
        for c in range(C):
            s.read("ch_off", _table_terms(off[c]), chans[c])
        s.seal()
    else:
        first = _payload_words(arena)
        s.read("seg_off", _table_terms(first, 4), oe["payload"].astype("<u4"), decoy=np.zeros(oe["payload"].size, "<u4"))
        outs = [s.write("ch_off", _table_terms(off[c]), lens[c]) for c in range(C)]
        s.seal()
        od = OC.decode(oe["payload"], o0, ln, p, oe["peak"], oe["enc"], len(data))
        for c in range(C):
            w0 = min(1 << CODEC_H, lens[c])               # MH_WIN_AFTER_CAL: [c, T); the bytes in front of it stay as they are
            img = np.full(lens[c], CANARY, np.uint8)
            img[w0:] = od[int(o0[c]) + w0:int(o0[c]) + lens[c]]
            s.rules.append(("decoded bytes == clip", np.array_equal(img[w0:], np.minimum(chans[c][w0:], S - 1))))
            s.expect(outs[c], img)
        s.crossing.append(("4 * seg_off[0]", 4 * first, "bytes"))
        if arena == "W":
            s.crossing.append(("seg_off[0]", first, "words"))
    if layout == "wg_head":
        s.rules.append(("a revision-3 head segment", bool((oe["seg"]["n"][oe["seg"]["ch"] == 0][0] == 128 - (1 << CODEC_H)))))

    def run(ctx):
        plan = ctx.mh.codec.Plan(np.array(off, np.uint64), ln, S, CODEC_H, mode, ctx.mh.WIN_AFTER_CAL, rows, seg_chunks=sc)
        try:
            nseg = plan.n_segments
            assert np.array_equal(plan.segments()["off"], oe["seg"]["off"]) and plan.payload_cap_words == oe["payload"].size
            if what == "decode":
                seg_off = ctx.u64(first + oe["seg"]["off"].astype(np.int64))
                rc = ctx.lib.mh_decode(plan._h, ctx.at(0), size // 4, ctx.p(seg_off), ctx.p(ctx.dev(oe["peak"])), ctx.p(ctx.dev(oe["enc"])),
                                       ctx.at(0), None)
                assert rc == 0, ctx.lib.mh_last_error()
                assert plan.decode_ok()
                return
            om = OC.measure(data, o0, ln, p)
            m = plan.measure(ctx.bytes)
            for got, want in ((m.cutoff, om["cutoff"]), (m.cal_hist, om["cal_sorted"]), (m.peak, om["peak"]), (m.enc, om["enc"]),
                              (m.post_hist, om["post_mapped"]), (m.bits, om["bits"]), (m.skipped, om["skipped"])):
                assert np.array_equal(got.cpu().numpy().astype(np.int64), want.astype(np.int64)), "mh_measure"
            word = (ctx.dev(np.where(om["peak"] > 0, om["peak"] - 1, 1).astype(np.uint8)), ctx.dev(om["enc"]))       # another word
            op = OC.encode_preset(data, o0, ln, p, word[0].cpu().numpy(), word[1].cpu().numpy())
            for e, want in ((plan.encode(ctx.bytes), oe), (plan.encode(ctx.bytes, preset=word), op)):
                assert np.array_equal(e.peak.cpu().numpy(), want["peak"]) and np.array_equal(e.enc.cpu().numpy(), want["enc"])
                sw = e.seg_words.cpu().numpy().astype(np.uint64)[:nseg]
                assert np.array_equal(sw, want["seg_words"]) and np.array_equal(e.ch_bits.cpu().numpy().astype(np.uint64), want["ch_bits"])
                pay = e.payload.cpu().numpy().view(np.uint32)
                for k in range(nseg):
                    o, n = int(want["seg"]["off"][k]), int(sw[k])
                    assert np.array_equal(pay[o:o + n], want["payload"][o:o + n]), ("segment", k)
        finally:
            plan.close()
    s.run = run
    return s


for _lay in ("wave", "wg", "wg_head"):
    for _S in (3, 8):
        _case("codec", "mh_measure, mh_encode, mh_encode_preset", "ch_off", "offset", "%s layout, S = %d" % (_lay, _S), build_codec,
              "encode", _lay, _S)
        _case("codec", "mh_decode", "ch_off + seg_off (bytes)", "offset", "%s layout, S = %d" % (_lay, _S), build_codec, "decode", _lay, _S)
_case("codec", "mh_decode", "ch_off + seg_off (words)", "offset", "wg layout, S = 8", build_codec, "decode", "wg", 8, "W", arena="W")


# =====================================================================================================================
# mh_decode_range, mh_decode_rebin: out_pitch as far value (2 rows) and far product (3 rows), seg_off far
# =====================================================================================================================
RANGE_R = 7
RANGE_T0 = (13 * CHUNK - 700) // RANGE_R * RANGE_R
RANGE_T1 = 13 * CHUNK + 7 + 901            # cuts a chunk at both ends and reaches 900 samples past the short channel


def build_range(what, kind, arena="A"):
    """what: "range", "rebin8" or "rebin32" (out_pitch in ELEMENTS: the uint32 form crosses in bytes from 2^30 elements)"""
    import oracle
    OC = oracle.c
    rng = _rng("range")
    size = ARENA_BYTES if arena == "A" else ARENA_W_BYTES
    s = Setup(arena, Image(size))
    lens, sc = CODEC_LAYOUTS["wg"]
    S = 8
    rows = np.array([ROWS_S[S]], np.uint8)
    chans, _near = _codec_channels(rng, lens, S)
    data, o0, ln = OC.flatten(chans)
    p = OC.Params(S, CODEC_H, OC.MODE_APPROX, OC.WIN_FULL, rows, seg_chunks=sc)
    oe = OC.encode(data, o0, ln, p)
    first = _payload_words(arena)
    s.read("seg_off", _table_terms(first, 4), oe["payload"].astype("<u4"), decoy=np.zeros(oe["payload"].size, "<u4"))
    e = 4 if what == "rebin32" else 1
    if kind == "value":
        sel, pitch = [1, 0], (STRIDE_VALUE + 36) // e + (1 if e == 1 else 0)
    else:
        sel, pitch = [0, 1, 0], (STRIDE_PRODUCT + 4100) // e - (1 if e == 1 else 0)
    t0, t1 = RANGE_T0, RANGE_T1
    y = np.zeros((len(sel), t1 - t0), np.uint8)
    for i, c in enumerate(sel):
        b = min(t1, lens[c])
        y[i, :b - t0] = np.minimum(chans[c][t0:b], S - 1)
    if what == "range":
        want = y
    else:
        sums = np.add.reduceat(y.astype(np.uint32), np.arange(0, t1 - t0, RANGE_R), axis=1)
        want = np.minimum(sums, 255).astype(np.uint8) if what == "rebin8" else sums.astype("<u4")
    n = want.shape[1]
    at = 0x3000000 + (4 if e == 4 else 7)
    outs = [s.write("out_pitch", (Term(i, pitch, e),), n * e, base=at) for i in range(len(sel))]
    s.seal()
    for i in range(len(sel)):
        s.expect(outs[i], want[i])
    s.crossing = [("%d * (n_sel - 1) * out_pitch" % e, e * (len(sel) - 1) * pitch, "bytes"), ("4 * seg_off[0]", 4 * first, "bytes")]
    if arena == "W":
        s.crossing.append(("seg_off[0]", first, "words"))
    s.rules += [("out_pitch >= n", pitch >= n), ("t0 % r == 0", t0 % RANGE_R == 0), ("a zero fill", t1 > lens[1] > t0),
                ("both ends cut a chunk", t0 % CHUNK != 0 and t1 % CHUNK != 0 and t0 // CHUNK != t1 // CHUNK),
                ("far value" if kind == "value" else "far product", (e * pitch >= FAR) == (kind == "value")),
                ("a cut last bin", what == "range" or (t1 - t0) % RANGE_R != 0)]

    def run(ctx):
        import torch
        plan = ctx.mh.codec.Plan(o0, ln, S, CODEC_H, OC.MODE_APPROX, ctx.mh.WIN_FULL, rows, seg_chunks=sc)
        try:
            seg_off = ctx.u64(first + oe["seg"]["off"].astype(np.int64))
            pk, en = ctx.dev(oe["peak"]), ctx.dev(oe["enc"])
            if what == "range":
                view = ctx.bytes.as_strided((len(sel), n), (pitch, 1), at)
                plan.decode_range(ctx.words, seg_off, pk, en, sel, t0, t1, out=view)
            else:
                src = ctx.bytes if e == 1 else ctx.words
                view = src.as_strided((len(sel), n), (pitch, 1), at // e)
                plan.decode_rebin(ctx.words, seg_off, pk, en, sel, t0, t1, RANGE_R, saturate=(e == 1), out=view)
            assert plan.decode_ok()
            torch.cuda.synchronize()
        finally:
            plan.close()
    s.run = run
    return s


for _what in ("range", "rebin8", "rebin32"):
    for _k in ("value", "product"):
        _case("range", "mh_decode_range" if _what == "range" else "mh_decode_rebin", "out_pitch + seg_off (bytes)", _k,
              "wg layout, S = 8, r = 7", build_range, _what, _k)
_case("range", "mh_decode_range", "out_pitch + seg_off (words)", "value", "wg layout, S = 8", build_range, "range", "value", "W", arena="W")
_case("crc", "mhi_seg_crc32", "seg_off (words)", "offset", "segments of %r words" % (CRC_WORDS,), build_crc, "all", "W", arena="W")
