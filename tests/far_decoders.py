"""Row strides and columns beyond 4 GiB for the five decoder libraries (a plain module, not a conftest): the case table of
tests/test_host_far_decoders.py and tests/test_gpu_far_decoders.py, on the machinery of tests/far_offsets.py -- the same
arena of 2^32 + 2^28 bytes that is never touched as a whole, the same sparse Image of it, the same Access / Term list that
says where a call reads and writes and where it would if a term were cut to 32 bits.

include/muahuff_wiener.h, _cascade.h, _smooth.h, _sweep.h and _kalman.h take 64-bit row strides and up to 2^40 - 1 columns
of float32 or float64, so the byte offset of a column passes 2^32 at column 2^30 or 2^29.  Three kinds of case:

  far value    a row stride of 2^32 + a few KiB, two rows (index 1): a stride parameter narrowed to 32 bits
  far product  a row stride of 2^31 + a few KiB, three rows (index 2): a j * stride formed in 32 bits
  far column   the calls that take ranges (mhc_moments, mhq_xty_clips, mhk_scan) on views of the arena with cols just under
               its element count and ranges that start past column 2^30 (float32) or 2^29 (float64): a 4 * t, an 8 * t or a
               column index formed in 32 bits.  Only the far windows and their aliases are touched.

The calls that always walk [0, cols) get their far column over the whole length of the arena; those five fill and compare
it on the device and live in tests/test_gpu_far_decoders.py, with their shapes (WHOLE) stated here.

A far input has a decoy at every alias, a far output has canary there and around every row.  Every expected value is exact:
integer weights and inputs below 2^24 (mhw_fir, mhc_polyval, mhs_box_f32), dyadic covariates (mhw_xty, mhq_xty_clips),
small integers (mhc_moments), integers (mhs_box, mhq_gram_clips), one dyadic m per channel (mhk_project); the yardsticks are
the oracles of the feature tests on the rows rebased to offset 0.  mhk_scan is the exception: the host image holds
kalman_oracle.serial_scan, the device test first makes the same call on the same data in a compact tensor at column 0,
holds that against the oracle within 64 * D_SCAN of the largest state, and then expects ITS bits in the arena -- the header
fixes tiles and gains relative to a range's own start, so where the columns lie must not show.

An operand that the header forbids to overlap another as a byte range lies below it: a far operand spans [base, base +
index * stride + row), so the near one sits under its base."""
import numpy as np

from tests import box_oracle as bo
from tests import cascade_oracle as co
from tests import kalman_oracle as ko
from tests import sweep_oracle as so
from tests import wiener_oracle as wo
from tests.far_offsets import (ARENA_BYTES, CANARY, FAR, PAD, SLACK, STRIDE_PRODUCT, STRIDE_VALUE, Access, Case, Image,  # noqa: F401
                               Setup, Term, _rng)

ARENA_F32 = ARENA_BYTES // 4           # the arena as float32: a column's byte offset passes 2^32 at column 2^30
ARENA_F64 = ARENA_BYTES // 8           # ... as float64: at column 2^29
ARENA2_BYTES = 2 * ARENA_BYTES         # two rows of the arena's length: the far column of mhk_scan with k = 2
NEAR, NEAR2, FAR_BASE = 0x10000, 0x80000, 0x400000      # where a near operand, a second one and a far one begin
# mh_wiener_layout.hpp, mh_cascade_layout.hpp, mh_smooth_layout.hpp, mh_kalman_layout.hpp (the host tests hold the same)
XTY_RUN, FIR_TILE, MOM_RUN, POLY_TILE, BOX_TILE, BOXF_TILE, PROJ_TILE, SCAN_TILE = 32768, 512, 16384, 1024, 3824, 256, 1024, 512

# what a far stride adds to 2^32 or 2^31: more than the longest row of any case, so that the alias of the last row lies behind
# row 0, and of the alignment the operand asks for (a byte row at any address: odd)
EX1, EX4, EX8, EX16 = 0x10003, 0x10004, 0x10008, 0x10010

CASES = []


def _case(row, entry, far, kind, shape, build, *args, arena="A"):
    CASES.append(Case("-".join([row] + [str(a) for a in args]), row, entry, far, kind, shape, build, args, arena))


def _stride(kind, extra, align=1):
    """(rows, stride): far value -- 2^32 + extra, index 1; far product -- 2^31 + extra, index 2"""
    stride = (STRIDE_VALUE if kind == "value" else STRIDE_PRODUCT) + extra
    assert stride % align == 0
    return (2 if kind == "value" else 3), stride


def _kind_rules(s, kind, what, n, stride, scale=1):
    s.crossing.append(("(%d - 1) * %s" % (n, what), scale * (n - 1) * stride, "bytes"))
    s.rules.append(("far value: the stride itself is >= 2^32" if kind == "value" else "far product: the stride itself is below 2^32",
                    (scale * stride >= FAR) == (kind == "value")))


def _counts(rng, rows, cols):
    """counts on both sides of every clip the cases use"""
    x = np.minimum(rng.poisson(1.5, size=(rows, cols)), 255).astype(np.uint8)
    x[rng.rand(rows, cols) < 0.05] = 255
    x[rng.rand(rows, cols) < 0.1] = rng.randint(2, 9)
    return x


def _dyadic(rng, k, cols):
    """(yi, y): y = yi / 64 in float32, multiples of 2^-6 with |y| <= 64 -- every product with a count and every sum exact"""
    yi = rng.randint(-4096, 4097, (k, cols)).astype(np.int64)
    y = (yi / 64.0).astype("<f4")
    assert np.array_equal(y.astype(np.float64) * 64, yi)
    return yi, y


def _out64(ctx, n):
    """a contiguous float64 / int64 result of n elements between two canary elements"""
    return ctx.canary(n + 2, np.float64)


def _scratch(ctx, nbytes):
    return ctx.canary(max(int(nbytes), 8), np.uint8)


def _host_u64(values):
    import ctypes as ct
    flat = [int(v) for v in values]
    return (ct.c_uint64 * max(len(flat), 1))(*flat)


# =====================================================================================================================
# mhw_xty: c * x_row_stride, j * y_row_stride + 4 * t
# =====================================================================================================================
XTY_COLS, XTY_LAGS, XTY_CLIP = 300, 3, 4


def build_xty(far, kind):
    rng = _rng("xty", far, kind)
    s = Setup("A", Image())
    far_x = far == "x_row_stride"
    n, stride = _stride(kind, EX1 if far_x else EX4, 1 if far_x else 4)
    rows, k = (n, 2) if far_x else (2, n)
    width = XTY_COLS + XTY_LAGS - 1
    xs, ys = (stride, 4 * XTY_COLS + 36) if far_x else (width + 37, stride)
    xb, yb = (FAR_BASE + 1, NEAR) if far_x else (NEAR + 1, FAR_BASE)
    x = _counts(rng, rows, width)
    _yi, y = _dyadic(rng, k, XTY_COLS)
    _di, ydec = _dyadic(rng, k, XTY_COLS)
    for c in range(rows):
        s.read("x_row_stride", (Term(c, xs),), x[c], base=xb)
    for j in range(k):
        s.read("y_row_stride", (Term(j, ys),), y[j], decoy=ydec[j], base=yb)
    s.seal()
    want = wo.xty(x, y, XTY_LAGS, XTY_CLIP)[0]                  # [lags, rows, k], exact: dyadic covariates
    other = wo.xty(np.concatenate([x[:1], 255 - x[1:]]), y, XTY_LAGS, XTY_CLIP)[0] if far_x else \
        wo.xty(x, np.concatenate([y[:1], ydec[1:]]), XTY_LAGS, XTY_CLIP)[0]
    _kind_rules(s, kind, far, n, stride)
    s.rules += [("the decoy rows give another result", not np.array_equal(want[:, n - 1] if far_x else want[:, :, n - 1],
                                                                          other[:, n - 1] if far_x else other[:, :, n - 1])),
                ("y and y_row_stride are multiples of 4", yb % 4 == 0 and ys % 4 == 0),
                ("x_row_stride >= cols + lags - 1, y_row_stride >= 4 * cols", xs >= width and ys >= 4 * XTY_COLS),
                ("x begins at an odd byte", xb % 2 == 1)]

    def run(ctx):
        lib = ctx.wlib
        import ctypes as ct
        need = ct.c_uint64(0)
        assert lib.mhw_xty_scratch_bytes(rows, XTY_COLS, XTY_LAGS, k, ct.byref(need)) == 0
        out, scratch = _out64(ctx, want.size), _scratch(ctx, need.value)
        rc = lib.mhw_xty(ctx.at(xb), xs, rows, XTY_COLS, XTY_LAGS, XTY_CLIP, ctx.at(yb), ys, k, ctx.p(out, 1), 0, ctx.p(scratch),
                         scratch.numel(), None)
        assert rc == 0, lib.mhw_last_error()
        ctx.sync()
        ctx.framed(out, 1, want, "mhw_xty")
    s.run = run
    return s


for _k in ("value", "product"):
    for _far in ("x_row_stride", "y_row_stride"):
        _case("xty", "mhw_xty", _far, _k, "cols = 300, lags = 3", build_xty, _far, _k)


# =====================================================================================================================
# mhw_fir: c * x_row_stride, j * out_row_stride
# =====================================================================================================================
FIR_COLS, FIR_LAGS, FIR_CLIP = 2 * (FIR_TILE - 2) + 9, 3, 5        # two workgroup tiles of 512 - (lags - 1) outputs and a cut one


def build_fir(far, kind):
    rng = _rng("fir", far, kind)
    s = Setup("A", Image())
    far_x = far == "x_row_stride"
    n, stride = _stride(kind, EX1 if far_x else EX4, 1 if far_x else 4)
    rows, k = (n, 2) if far_x else (2, n)
    width = FIR_COLS + FIR_LAGS - 1
    xs, os_ = (stride, 4 * FIR_COLS + 36) if far_x else (width + 37, stride)
    xb, ob = (FAR_BASE + 1, NEAR) if far_x else (NEAR + 1, FAR_BASE)        # out must not overlap x: the near one lies below
    x = _counts(rng, rows, width)
    w = rng.randint(-9, 10, (k, FIR_LAGS, rows)).astype(np.int64)
    bias = rng.randint(-100, 101, (k,)).astype(np.int64)
    for c in range(rows):
        s.read("x_row_stride", (Term(c, xs),), x[c], base=xb)
    outs = [s.write("out_row_stride", (Term(j, os_),), 4 * FIR_COLS, base=ob) for j in range(k)]
    s.seal()
    want, mag = wo.fir(x, w, bias, FIR_LAGS, FIR_CLIP)
    for j in range(k):
        s.expect(outs[j], want[j].astype("<f4"))
    _kind_rules(s, kind, far, n, stride)
    other = wo.fir(np.concatenate([x[:1], 255 - x[1:]]), w, bias, FIR_LAGS, FIR_CLIP)[0]
    s.rules += [("every partial sum is below 2^24", int(mag.max()) < 1 << 24),
                ("the decoy rows give another result", not far_x or not np.array_equal(want, other)),
                ("out and out_row_stride are multiples of 4", ob % 4 == 0 and os_ % 4 == 0),
                ("x_row_stride >= cols + lags - 1, out_row_stride >= 4 * cols", xs >= width and os_ >= 4 * FIR_COLS),
                ("more than two workgroup tiles", FIR_COLS > 2 * (FIR_TILE - (FIR_LAGS - 1)))]

    def run(ctx):
        lib = ctx.wlib
        rc = lib.mhw_fir(ctx.at(xb), xs, rows, FIR_COLS, FIR_LAGS, FIR_CLIP, ctx.p(ctx.dev(w.astype("<f4"))), ctx.p(ctx.dev(bias.astype("<f4"))),
                         k, ctx.at(ob), os_, None)
        assert rc == 0, lib.mhw_last_error()
    s.run = run
    return s


for _k in ("value", "product"):
    for _far in ("x_row_stride", "out_row_stride"):
        _case("fir", "mhw_fir", _far, _k, "cols = %d, lags = 3" % FIR_COLS, build_fir, _far, _k)


# =====================================================================================================================
# mhc_moments: j * p_row_stride, j * y_row_stride, + t
# =====================================================================================================================
MOM_DEGREE = 2


def _mom_data(rng, k, cols):
    """small integers: p even with |p| <= 6, y with |y| <= 3, center even, inv_scale 0.5 -- u and every term are integers"""
    p = (2 * rng.randint(-3, 4, (k, cols))).astype("<f4")
    y = rng.randint(-3, 4, (k, cols)).astype("<f4")
    return p, y


def _mom_call(ctx, pa, ps, ya, ys, k, cols, ranges, center, inv, want):
    import ctypes as ct
    lib = ctx.clib
    need = ct.c_uint64(0)
    assert lib.mhc_moments_scratch_bytes(cols, k, MOM_DEGREE, len(ranges), ct.byref(need)) == 0
    out, scratch = _out64(ctx, want.size), _scratch(ctx, need.value)
    host = _host_u64([v for ab in ranges for v in ab])
    rc = lib.mhc_moments(ctx.at(pa), ps, ctx.at(ya), ys, k, cols, ct.cast(host, ct.c_void_p), len(ranges), MOM_DEGREE,
                         ctx.p(ctx.dev(center)), ctx.p(ctx.dev(inv)), ctx.p(out, 1), 0, ctx.p(scratch), scratch.numel(), None)
    assert rc == 0, lib.mhc_last_error()
    ctx.sync()
    ctx.framed(out, 1, want, "mhc_moments")


def build_moments(far, kind):
    rng = _rng("moments", far, kind)
    s = Setup("A", Image())
    k, stride = _stride(kind, EX4, 4)
    cols = MOM_RUN // 8 + 5
    far_p = far == "p_row_stride"
    ps, ys = (stride, 4 * cols + 36) if far_p else (4 * cols + 44, stride)
    pb, yb = (FAR_BASE, NEAR) if far_p else (NEAR, FAR_BASE)
    p, y = _mom_data(rng, k, cols)
    dp, dy = _mom_data(rng, k, cols)
    center, inv = (2 * rng.randint(-1, 2, (k,))).astype(np.float64), np.full((k,), 0.5)
    for j in range(k):
        s.read("p_row_stride", (Term(j, ps),), p[j], decoy=dp[j], base=pb)
        s.read("y_row_stride", (Term(j, ys),), y[j], decoy=dy[j], base=yb)
    s.seal()
    ranges = [(3, 1000), (1000, cols)]
    terms = co.moment_terms(p, y, MOM_DEGREE, center, inv)
    want = np.stack([terms[:, :, a:b].sum(2) for a, b in ranges])
    t2 = co.moment_terms(dp if far_p else p, y if far_p else dy, MOM_DEGREE, center, inv)
    _kind_rules(s, kind, far, k, stride)
    s.rules += [("every term is an integer and every sum exact", bool((terms == np.rint(terms)).all()) and cols * np.abs(terms).max() < 2.0 ** 53),
                ("the decoy rows give another result", not np.array_equal(terms[k - 1, 1:].sum(1), t2[k - 1, 1:].sum(1))),
                ("p, y and their strides are multiples of 4", pb % 4 == 0 and yb % 4 == 0 and ps % 4 == 0 and ys % 4 == 0),
                ("the strides are at least 4 * cols", min(ps, ys) >= 4 * cols)]
    s.run = lambda ctx: _mom_call(ctx, pb, ps, yb, ys, k, cols, ranges, center, inv, want)
    return s


def build_moments_column():
    """k = 1, p and y views of the arena (y a few KiB in), cols just under its float count; two ranges past column 2^30,
    the second of two runs and a ragged one, so that run numbering starts at a nonzero value"""
    rng = _rng("moments", "column")
    s = Setup("A", Image())
    pb, yb = 0, 0x100000                                 # (the aliases of p end below y's)
    cols = ARENA_F32 - yb // 4
    a0 = (1 << 30) + 0x1003
    ranges = [(a0, a0 + 301), (a0 + 0x2000, a0 + 0x2000 + 2 * MOM_RUN + 77)]
    center, inv = np.array([2.0]), np.array([0.5])
    data, want = [], []
    for a, b in ranges:
        p, y = _mom_data(rng, 1, b - a)
        dp, dy = _mom_data(rng, 1, b - a)
        s.read("ranges (p)", (Term(a, 1, 4),), p[0], decoy=dp[0], base=pb)
        s.read("ranges (y)", (Term(a, 1, 4),), y[0], decoy=dy[0], base=yb)
        terms = co.moment_terms(p, y, MOM_DEGREE, center, inv)
        data.append((terms, co.moment_terms(dp, y, MOM_DEGREE, center, inv), co.moment_terms(p, dy, MOM_DEGREE, center, inv)))
        want.append(terms.sum(2))
    s.seal()
    want = np.stack(want)
    s.crossing = [("4 * ranges[%d]" % (2 * r), 4 * a, "bytes") for r, (a, _b) in enumerate(ranges)]
    s.rules += [("every term is an integer and every sum exact", all(bool((t == np.rint(t)).all()) for t, _p, _y in data)),
                ("the decoys of p and of y give another result",
                 all(not np.array_equal(t[0, 1:].sum(1), o[0, 1:].sum(1)) for t, dp_, dy_ in data for o in (dp_, dy_))),
                ("the ranges start past column 2^30 and lie inside cols", ranges[0][0] >= 1 << 30 and ranges[-1][1] <= cols),
                ("cols is just under the arena's float count and both rows fit", ARENA_F32 - cols <= 1 << 18 and yb // 4 + cols <= ARENA_F32),
                ("the second range is two runs and a ragged one", ranges[1][1] - ranges[1][0] == 2 * MOM_RUN + 77)]
    s.run = lambda ctx: _mom_call(ctx, pb, 0, yb, 0, 1, cols, ranges, center, inv, want)
    return s


for _k in ("value", "product"):
    for _far in ("p_row_stride", "y_row_stride"):
        _case("moments", "mhc_moments", _far, _k, "cols = 2053, degree 2, 2 ranges", build_moments, _far, _k)
_case("moments", "mhc_moments", "ranges", "column", "k = 1, cols = 2^30 + 2^26 - 2^18, 2 ranges", build_moments_column)


# =====================================================================================================================
# mhc_polyval: j * p_row_stride, j * out_row_stride
# =====================================================================================================================
POLY_COLS = POLY_TILE + 5


def _poly_data(rng, k):
    p = rng.randint(-9, 10, (k, POLY_COLS)).astype("<f4")
    coef = rng.randint(-5, 6, (k, 3)).astype("<f4")
    coef[:, 0] = rng.choice([-3, -2, 2, 3], k)
    center, inv = rng.randint(-2, 3, (k,)).astype("<f4"), np.full((k,), 2.0, "<f4")
    return p, coef, center, inv


def build_polyval(far, kind):
    """far p_row_stride or out_row_stride with the other operand near, or both far and the call in place (out == p)"""
    rng = _rng("polyval", far, kind)
    s = Setup("A", Image())
    k, stride = _stride(kind, EX4, 4)
    p, coef, center, inv = _poly_data(rng, k)
    dp = _poly_data(rng, k)[0]
    inplace = far == "in place"
    far_p = far == "p_row_stride"
    ps, os_ = (stride, stride) if inplace else (stride, 4 * POLY_COLS + 36) if far_p else (4 * POLY_COLS + 44, stride)
    pb, ob = (FAR_BASE, FAR_BASE) if inplace else (FAR_BASE, NEAR) if far_p else (NEAR, FAR_BASE)
    for j in range(k):
        s.read("p_row_stride", (Term(j, ps),), p[j], decoy=dp[j], base=pb)
    outs = [s.write("out_row_stride", (Term(j, os_),), 4 * POLY_COLS, base=ob) for j in range(k)]
    s.seal()
    want, mag = co.polyval(p, coef, center, inv)
    for j in range(k):
        s.expect(outs[j], want[j].astype("<f4"))
    _kind_rules(s, kind, "the stride", k, stride)
    s.rules += [("every intermediate is an integer below 2^24", float(mag.max()) < 2 ** 24 and bool((want == np.rint(want)).all())),
                ("the decoy rows give another result", not np.array_equal(want, co.polyval(dp, coef, center, inv)[0])),
                ("the result differs from the input", not np.array_equal(want, p.astype(np.float64))),
                ("pointers and strides are multiples of 4, strides at least 4 * cols", pb % 4 == 0 and ob % 4 == 0 and ps % 4 == 0
                 and os_ % 4 == 0 and min(ps, os_) >= 4 * POLY_COLS),
                ("out is p itself or does not overlap it: the near operand lies below the far one's base", inplace or min(pb, ob) + 4 * POLY_COLS * k + 64 * k <= FAR_BASE)]

    def run(ctx):
        lib = ctx.clib
        rc = lib.mhc_polyval(ctx.at(pb), ps, k, POLY_COLS, ctx.p(ctx.dev(coef)), 2, ctx.p(ctx.dev(center)), ctx.p(ctx.dev(inv)), ctx.at(ob), os_, None)
        assert rc == 0, lib.mhc_last_error()
    s.run = run
    return s


for _k in ("value", "product"):
    for _far in ("p_row_stride", "out_row_stride", "in place"):
        _case("polyval", "mhc_polyval", _far, _k, "cols = 1029, degree 2", build_polyval, _far, _k)


# =====================================================================================================================
# mhs_box_f32: j * in_row_stride, j * out_row_stride
# =====================================================================================================================
BOXF_COLS, BOXF_WINDOW = 2 * BOXF_TILE + 5, 7


def build_box_f32(far, kind):
    rng = _rng("box_f32", far, kind)
    s = Setup("A", Image())
    k, stride = _stride(kind, EX4, 4)
    far_in = far == "in_row_stride"
    is_, os_ = (stride, 4 * BOXF_COLS + 36) if far_in else (4 * BOXF_COLS + 44, stride)
    ib, ob = (FAR_BASE, NEAR) if far_in else (NEAR, FAR_BASE)
    p = rng.randint(-30000, 30001, (k, BOXF_COLS)).astype(np.int64)
    dp = rng.randint(-30000, 30001, (k, BOXF_COLS)).astype(np.int64)
    bias = rng.randint(-1000, 1001, (k,)).astype(np.int64)
    for j in range(k):
        s.read("in_row_stride", (Term(j, is_),), p[j].astype("<f4"), decoy=dp[j].astype("<f4"), base=ib)
    outs = [s.write("out_row_stride", (Term(j, os_),), 4 * BOXF_COLS, base=ob) for j in range(k)]
    s.seal()
    want, mag = bo.box_f32(p, BOXF_WINDOW, bias)
    for j in range(k):
        s.expect(outs[j], want[j].astype("<f4"))
    _kind_rules(s, kind, far, k, stride)
    s.rules += [("every partial sum is below 2^24", int(mag.max()) < 1 << 24),
                ("the decoy rows give another result", not np.array_equal(want, bo.box_f32(dp, BOXF_WINDOW, bias)[0])),
                ("pointers and strides are multiples of 4, strides at least 4 * cols and below 2^48",
                 ib % 4 == 0 and ob % 4 == 0 and is_ % 4 == 0 and os_ % 4 == 0 and 4 * BOXF_COLS <= min(is_, os_) and max(is_, os_) < 1 << 48),
                ("out does not overlap in: the near operand lies below the far one's base", NEAR + (4 * BOXF_COLS + 44) * k <= FAR_BASE)]

    def run(ctx):
        lib = ctx.slib
        rc = lib.mhs_box_f32(ctx.at(ib), is_, k, BOXF_COLS, BOXF_WINDOW, ctx.p(ctx.dev(bias.astype("<f4"))), ctx.at(ob), os_, None)
        assert rc == 0, lib.mhs_last_error()
    s.run = run
    return s


for _k in ("value", "product"):
    for _far in ("in_row_stride", "out_row_stride"):
        _case("box_f32", "mhs_box_f32", _far, _k, "cols = 517, window 7", build_box_f32, _far, _k)


# =====================================================================================================================
# mhs_box: the far product (tests/test_gpu_box.py has the far values)
# =====================================================================================================================
BOX_COLS, BOX_WINDOW, BOX_CLIP = BOX_TILE + 70, 50, 39


def build_box(far):
    rng = _rng("box", far)
    s = Setup("A", Image())
    far_x = far == "x_row_stride"
    rows, stride = _stride("product", EX1 if far_x else EX16, 1 if far_x else 16)
    width = BOX_COLS + BOX_WINDOW - 1
    xs, os_ = (stride, (BOX_COLS + 15) // 16 * 16 + 32) if far_x else (width + 37, stride)
    # lo and hi must not overlap x as byte ranges: the near side lies below the far one's base; far planes interleave
    xb, lob, hib = (FAR_BASE + 1, NEAR, NEAR2) if far_x else (NEAR + 1, FAR_BASE, FAR_BASE + 0x100000)
    x = _counts(rng, rows, width)
    for c in range(rows):
        s.pre.put(xb + c * xs - 16, np.full(width + 32, 255, np.uint8))      # what the dwords at a row's ragged ends hold
        s.read("x_row_stride", (Term(c, xs),), x[c], base=xb)
    lo = [s.write("out_row_stride (lo)", (Term(c, os_),), BOX_COLS, base=lob) for c in range(rows)]
    hi = [s.write("out_row_stride (hi)", (Term(c, os_),), BOX_COLS, base=hib) for c in range(rows)]
    s.seal()
    wl, wh = bo.planes(x, BOX_WINDOW, BOX_CLIP)
    for c in range(rows):
        s.expect(lo[c], wl[c])
        s.expect(hi[c], wh[c])
    _kind_rules(s, "product", far, rows, stride)
    s.rules += [("lo, hi and out_row_stride are multiples of 16", lob % 16 == 0 and hib % 16 == 0 and os_ % 16 == 0),
                ("the strides hold a row and are below 2^48", xs >= width and os_ >= BOX_COLS and max(xs, os_) < 1 << 48),
                ("two planes: sums above 255", int(wh.max()) > 0),
                ("the decoy rows give another result", not far_x or not np.array_equal(wl[2], bo.planes(255 - x[2:], BOX_WINDOW, BOX_CLIP)[0][0])),
                ("more than one tile", BOX_COLS > BOX_TILE)]

    def run(ctx):
        lib = ctx.slib
        rc = lib.mhs_box(ctx.at(xb), xs, rows, BOX_COLS, BOX_WINDOW, BOX_CLIP, ctx.at(lob), ctx.at(hib), os_, None)
        assert rc == 0, lib.mhs_last_error()
    s.run = run
    return s


for _far in ("x_row_stride", "out_row_stride"):
    _case("box", "mhs_box", _far, "product", "3 rows, cols = %d, window 50" % BOX_COLS, build_box, _far)


# =====================================================================================================================
# mhq_gram_clips: the far product (tests/test_gpu_sweep.py has the far value)
# =====================================================================================================================
def build_gram_clips():
    rng = _rng("gram_clips")
    s = Setup("A", Image())
    rows, stride = _stride("product", EX1)
    cols, lags, clips = 300, 3, (2, 39)
    xb = FAR_BASE + 13
    x = _counts(rng, rows, cols)
    for c in range(rows):
        s.read("x_row_stride", (Term(c, stride),), x[c], base=xb)
    s.seal()
    ranges = [(2, 150), (150, cols)]
    want = so.gram_clips_fast(x, ranges, clips, lags)
    other = so.gram_clips_fast(np.concatenate([x[:2], 255 - x[2:]]), ranges, clips, lags)
    _kind_rules(s, "product", "x_row_stride", rows, stride)
    s.rules += [("the decoy row gives other sums", not np.array_equal(want[1], other[1])), ("x_row_stride >= cols", stride >= cols)]

    def run(ctx):
        import ctypes as ct
        lib = ctx.qlib
        gram, sums = ctx.dev(np.zeros(want[0].size + 2, np.int64)), ctx.dev(np.zeros(want[1].size + 2, np.int64))
        hc = (ct.c_uint32 * len(clips))(*clips)
        rc = lib.mhq_gram_clips(ctx.at(xb), stride, rows, cols, ct.cast(_host_u64([v for ab in ranges for v in ab]), ct.c_void_p), len(ranges),
                                ct.cast(hc, ct.c_void_p), len(clips), lags, ctx.p(gram, 1), ctx.p(sums, 1), None)
        assert rc == 0, lib.mhq_last_error()
        ctx.sync()
        for got, exp in ((gram, want[0]), (sums, want[1])):          # the call adds to the zeros it was given; the frame stays zero
            g = ctx.host(got)
            assert g[0] == 0 and g[-1] == 0 and np.array_equal(g[1:-1], exp.ravel()), ("mhq_gram_clips", g[1:-1], exp.ravel())
    s.run = run
    return s


_case("gram_clips", "mhq_gram_clips", "x_row_stride", "product", "3 rows, cols = 300, lags = 3", build_gram_clips)


# =====================================================================================================================
# mhq_xty_clips: c * x_row_stride + first, 4 * (first + lead) + j * y_row_stride + 4 * t
# =====================================================================================================================
XC_LAGS, XC_LEAD, XC_CLIPS = 3, 2, (2, 39)


def _xty_clips_call(ctx, xa, xs, rows, cols, ranges, ya, ys, k, want):
    import ctypes as ct
    lib = ctx.qlib
    need = ct.c_uint64(0)
    assert lib.mhq_xty_clips_scratch_bytes(rows, cols, XC_LAGS, k, len(ranges), len(XC_CLIPS), ct.byref(need)) == 0
    out, scratch = _out64(ctx, want.size), _scratch(ctx, need.value)
    hc = (ct.c_uint32 * len(XC_CLIPS))(*XC_CLIPS)
    rc = lib.mhq_xty_clips(ctx.at(xa), xs, rows, cols, ct.cast(_host_u64([v for ab in ranges for v in ab]), ct.c_void_p), len(ranges),
                           ct.cast(hc, ct.c_void_p), len(XC_CLIPS), XC_LAGS, XC_LEAD, ctx.at(ya), ys, k, ctx.p(out, 1), ctx.p(scratch),
                           scratch.numel(), None)
    assert rc == 0, lib.mhq_last_error()
    ctx.sync()
    ctx.framed(out, 1, want, "mhq_xty_clips")


def build_xty_clips(far, kind):
    rng = _rng("xty_clips", far, kind)
    s = Setup("A", Image())
    far_x = far == "x_row_stride"
    n, stride = _stride(kind, EX1 if far_x else EX4, 1 if far_x else 4)
    rows, k = (n, 2) if far_x else (2, n)
    cols = 400
    xs, ys = (stride, 4 * cols + 36) if far_x else (cols + 37, stride)
    xb, yb = (FAR_BASE + 1, NEAR) if far_x else (NEAR + 1, FAR_BASE)
    x = _counts(rng, rows, cols)
    _yi, y = _dyadic(rng, k, cols)
    _di, ydec = _dyadic(rng, k, cols)
    for c in range(rows):
        s.read("x_row_stride", (Term(c, xs),), x[c], base=xb)
    for j in range(k):
        s.read("y_row_stride", (Term(j, ys),), y[j], decoy=ydec[j], base=yb)
    s.seal()
    ranges = [(XC_LAGS - 1, 150), (150, 150), (190, cols - XC_LEAD)]
    want = so.xty_clips(x, y, ranges, XC_CLIPS, XC_LAGS, XC_LEAD)[0]
    other = so.xty_clips(np.concatenate([x[:1], 255 - x[1:]]), y, ranges, XC_CLIPS, XC_LAGS, XC_LEAD)[0] if far_x else \
        so.xty_clips(x, np.concatenate([y[:1], ydec[1:]]), ranges, XC_CLIPS, XC_LAGS, XC_LEAD)[0]
    _kind_rules(s, kind, far, n, stride)
    s.rules += [("the decoy rows give another result", not np.array_equal(want[0], other[0]) and not np.array_equal(want[2], other[2])),
                ("y and y_row_stride are multiples of 4", yb % 4 == 0 and ys % 4 == 0),
                ("x_row_stride >= cols, y_row_stride >= 4 * cols", xs >= cols and ys >= 4 * cols)]
    s.run = lambda ctx: _xty_clips_call(ctx, xb, xs, rows, cols, ranges, yb, ys, k, want)
    return s


def build_xty_clips_column():
    """rows = 1, k = 1; x a byte view and y a float view of the arena, cols just under its float count; two ranges past
    column 2^30, the second of a run and a ragged one"""
    rng = _rng("xty_clips", "column")
    s = Setup("A", Image())
    xb, yb = 0x1001, 0
    cols = ARENA_F32 - 0x2000
    a0 = (1 << 30) + 0x5003
    ranges = [(a0, a0 + 301), (a0 + 0x4000, a0 + 0x4000 + XTY_RUN + 77)]
    want, diff = [], []
    for a, b in ranges:
        n = b - a
        x = _counts(rng, 1, n + XC_LAGS - 1)                    # the columns [a - (lags - 1), b)
        _yi, y = _dyadic(rng, 1, n)                             # the columns [a + lead, b + lead)
        _di, ydec = _dyadic(rng, 1, n)
        s.read("ranges (x)", (Term(a - (XC_LAGS - 1), 1),), x[0], base=xb)
        s.read("ranges (y)", (Term(a + XC_LEAD, 1, 4),), y[0], decoy=ydec[0], base=yb)
        # rebased: the range is the design rows [lags - 1, lags - 1 + n) of x against y shifted by lead
        pad = np.zeros((1, n + XC_LAGS - 1 + XC_LEAD), np.float32)
        xpad = np.concatenate([x, np.zeros((1, XC_LEAD), np.uint8)], axis=1)      # (the oracle wants as many columns of x as of y)
        one = [(XC_LAGS - 1, XC_LAGS - 1 + n)]
        for src, dst in ((y, want), (ydec, diff)):
            pad[0, XC_LAGS - 1 + XC_LEAD:] = src[0]
            dst.append(so.xty_clips(xpad, pad, one, XC_CLIPS, XC_LAGS, XC_LEAD)[0][0])
    s.seal()
    want = np.stack(want)
    s.crossing = [("4 * (ranges[%d] + lead)" % (2 * r), 4 * (a + XC_LEAD), "bytes") for r, (a, _b) in enumerate(ranges)]
    s.rules += [("the decoys give another result", all(not np.array_equal(w, d) for w, d in zip(want, diff))),
                ("the ranges start past column 2^30 and end at or before cols - lead", ranges[0][0] >= 1 << 30 and ranges[-1][1] <= cols - XC_LEAD),
                ("cols is just under the arena's float count and x fits the arena", ARENA_F32 - cols <= 0x2000 and xb + cols <= ARENA_BYTES),
                ("the second range is a run and a ragged one", ranges[1][1] - ranges[1][0] == XTY_RUN + 77)]
    s.run = lambda ctx: _xty_clips_call(ctx, xb, 0, 1, cols, ranges, yb, 0, 1, want)
    return s


for _k in ("value", "product"):
    for _far in ("x_row_stride", "y_row_stride"):
        _case("xty_clips", "mhq_xty_clips", _far, _k, "cols = 400, lags = 3, lead = 2, 3 ranges, 2 clips", build_xty_clips, _far, _k)
_case("xty_clips", "mhq_xty_clips", "ranges", "column", "rows = k = 1, cols = 2^30 + 2^26 - 8192, 2 ranges", build_xty_clips_column)


# =====================================================================================================================
# mhk_project: c * x_row_stride, j * v_row_stride
# =====================================================================================================================
PROJ_COLS, PROJ_CLIP = PROJ_TILE + 5, 4


def build_project(far, kind):
    rng = _rng("project", far, kind)
    s = Setup("A", Image())
    far_x = far == "x_row_stride"
    n, stride = _stride(kind, EX1 if far_x else EX8, 1 if far_x else 8)
    rows, k = (n, 2) if far_x else (2, n)
    xs, vs = (stride, 8 * PROJ_COLS + 40) if far_x else (PROJ_COLS + 37, stride)
    xb, vb = (FAR_BASE + 1, NEAR) if far_x else (NEAR + 1, FAR_BASE)       # v must not overlap x: the near one lies below
    x = _counts(rng, rows, PROJ_COLS)
    mi, m0i = rng.randint(-40, 41, (k, rows)).astype(np.int64), rng.randint(-9, 10, (k,)).astype(np.int64)
    mi[mi == 0] = 3
    for c in range(rows):
        s.read("x_row_stride", (Term(c, xs),), x[c], base=xb)
    outs = [s.write("v_row_stride", (Term(j, vs),), 8 * PROJ_COLS, base=vb) for j in range(k)]
    s.seal()
    # m = mi / 8, m0 = m0i / 4: dyadic, every product and sum exact
    ref = lambda xx: (2 * m0i[:, None] + mi @ np.minimum(xx, PROJ_CLIP).astype(np.int64)) / 8.0      # noqa: E731
    want = ref(x)
    for j in range(k):
        s.expect(outs[j], want[j].astype("<f8"))
    _kind_rules(s, kind, far, n, stride)
    s.rules += [("the decoy rows give another result", not far_x or not np.array_equal(want, ref(np.concatenate([x[:1], 255 - x[1:]])))),
                ("v and v_row_stride are multiples of 8", vb % 8 == 0 and vs % 8 == 0),
                ("x_row_stride >= cols, v_row_stride >= 8 * cols, both below 2^48", xs >= PROJ_COLS and vs >= 8 * PROJ_COLS and max(xs, vs) < 1 << 48),
                ("more than one tile", PROJ_COLS > PROJ_TILE)]

    def run(ctx):
        lib = ctx.klib
        rc = lib.mhk_project(ctx.at(xb), xs, rows, PROJ_COLS, PROJ_CLIP, ctx.p(ctx.dev(mi / 8.0)), ctx.p(ctx.dev(m0i / 4.0)), k, ctx.at(vb), vs, None)
        assert rc == 0, lib.mhk_last_error()
    s.run = run
    return s


for _k in ("value", "product"):
    for _far in ("x_row_stride", "v_row_stride"):
        _case("project", "mhk_project", _far, _k, "cols = 1029", build_project, _far, _k)


# =====================================================================================================================
# mhk_scan: j * v_row_stride, j * out_row_stride, [t] in all three kernels
# =====================================================================================================================
SCAN_GAINS = 5                                     # the gain index moves (steps 0..3) and saturates (from step 4 on)
SCAN_STEPS = 3 * SCAN_TILE + 9                     # three tiles and a ragged one


def _scan_expect(s, ctx, k, v_of, ranges, F, B, init, where):
    """The compact call: the columns [ranges[0][0], ranges[-1][1]) in a contiguous tensor at column 0.  Its result is held
    against the serial oracle within 64 * D_SCAN of the largest state, and its bits become what the arena must hold.
    v_of: float64 [k, span]; where(j, a, b) -> the Access of row j, columns [a, b)"""
    import ctypes as ct

    import torch

    from tests.test_host_kalman import D_SCAN
    lib = ctx.klib
    a0, span = ranges[0][0], ranges[-1][1] - ranges[0][0]
    rebased = [(a - a0, b - a0) for a, b in ranges]
    vc = ctx.dev(v_of)
    need = ct.c_uint64(0)
    assert lib.mhk_scan_scratch_bytes(span, k, len(ranges), ct.byref(need)) == 0
    scratch = _scratch(ctx, need.value)
    rc = lib.mhk_scan(ctx.p(vc), 8 * span, k, span, ct.cast(_host_u64([u for ab in rebased for u in ab]), ct.c_void_p), len(ranges),
                      ctx.p(ctx.dev(F)), ctx.p(ctx.dev(B)), SCAN_GAINS, ctx.p(ctx.dev(init)), ctx.p(vc), 8 * span, ctx.p(scratch), scratch.numel(), None)
    assert rc == 0, lib.mhk_last_error()
    torch.cuda.synchronize()
    compact = vc.cpu().numpy()
    ref = ko.serial_scan(v_of, rebased, F, B, init, out=v_of.copy())
    err, scale = np.abs(compact - ref).max(), np.abs(ref).max()
    print("\nthe compact scan (k %d): error %.3g of the largest state, bound %.3g" % (k, err / scale, 64 * D_SCAN))
    assert err <= 64 * D_SCAN * scale
    for r, (a, b) in enumerate(rebased):
        assert np.array_equal(compact[:, a], init[r])
        for j in range(k):
            s.expect(where(j, ranges[r][0], ranges[r][1]), compact[j, a:b].astype("<f8"))
    return compact


def _scan_call(ctx, va, vs, oa, os_, k, cols, ranges, F, B, init):
    import ctypes as ct
    lib = ctx.klib
    need = ct.c_uint64(0)
    assert lib.mhk_scan_scratch_bytes(cols, k, len(ranges), ct.byref(need)) == 0
    scratch = _scratch(ctx, need.value)
    rc = lib.mhk_scan(ctx.at(va), vs, k, cols, ct.cast(_host_u64([u for ab in ranges for u in ab]), ct.c_void_p), len(ranges), ctx.p(ctx.dev(F)),
                      ctx.p(ctx.dev(B)), SCAN_GAINS, ctx.p(ctx.dev(init)), ctx.at(oa), os_, ctx.p(scratch), scratch.numel(), None)
    assert rc == 0, lib.mhk_last_error()


def build_scan(far, kind):
    """far v_row_stride or out_row_stride with the other operand near, or both far and the call in place; one range of three
    tiles and a ragged one behind a short one"""
    rng = _rng("scan", far, kind)
    s = Setup("A", Image())
    k, stride = _stride(kind, EX8, 8)
    cols = 40 + SCAN_STEPS + 1 + 7
    ranges = [(2, 40), (40, 40 + SCAN_STEPS + 1)]
    inplace, far_v = far == "in place", far == "v_row_stride"
    vs, os_ = (stride, stride) if inplace else (stride, 8 * cols + 40) if far_v else (8 * cols + 40, stride)
    vb, ob = (FAR_BASE, FAR_BASE) if inplace else (FAR_BASE, NEAR) if far_v else (NEAR, FAR_BASE)
    F, B = ko.contractive(k, SCAN_GAINS, 0.98, 11)
    v, dv, init = rng.randn(k, cols), rng.randn(k, cols), rng.randn(len(ranges), k)
    for j in range(k):
        s.read("v_row_stride", (Term(j, vs),), v[j].astype("<f8"), decoy=dv[j].astype("<f8"), base=vb)
    # what is written: the columns of the ranges; in place the other columns keep v, otherwise canary
    outs = {(j, a): s.write("out_row_stride", (Term(j, os_),), 8 * (b - a), base=ob + 8 * a) for j in range(k) for a, b in ranges}
    s.seal()
    ref = ko.serial_scan(v, ranges, F, B, init)
    for j in range(k):
        for a, b in ranges:
            s.expect(outs[(j, a)], ref[j, a:b].astype("<f8"))     # the oracle; the device test puts the compact call's bits here
    _kind_rules(s, kind, "the stride", k, stride)
    s.rules += [("pointers and strides are multiples of 8, strides at least 8 * cols and below 2^48",
                 vb % 8 == 0 and ob % 8 == 0 and vs % 8 == 0 and os_ % 8 == 0 and 8 * cols <= min(vs, os_) and max(vs, os_) < 1 << 48),
                ("the decoy rows give another result", not np.array_equal(ref[k - 1, 41:50], ko.serial_scan(np.concatenate([v[:k - 1], dv[k - 1:]]), ranges, F, B, init)[k - 1, 41:50])),
                ("three tiles and a ragged one, behind a range with a tile of its own", ranges[1][1] - ranges[1][0] - 1 == 3 * SCAN_TILE + 9 and ranges[0][1] - ranges[0][0] > 1),
                ("the gain index moves and saturates", 1 < SCAN_GAINS < 40),
                ("out is v itself or does not overlap it: the near operand lies below the far one's base", inplace or NEAR + (8 * cols + 40) * k <= FAR_BASE)]

    def run(ctx):
        a0, b1 = ranges[0][0], ranges[-1][1]
        _scan_expect(s, ctx, k, np.ascontiguousarray(v[:, a0:b1]), ranges, F, B, init, lambda j, a, b: outs[(j, a)])
        _scan_call(ctx, vb, vs, ob, os_, k, cols, ranges, F, B, init)
    s.run = run
    return s


def build_scan_column(k):
    """in place on a view of the arena with cols just under its float64 count; two ranges past column 2^29, the second of
    three tiles and a ragged one.  k = 2 needs a second row at least 8 * cols bytes behind the first, which no arena of
    2^32 + 2^28 bytes holds: that case takes one of twice the length, its rows one arena apart."""
    rng = _rng("scan", "column", k)
    size = ARENA_BYTES if k == 1 else ARENA2_BYTES
    s = Setup("A" if k == 1 else "A2", Image(size))
    cols = ARENA_F64 - 16
    stride = 0 if k == 1 else ARENA_BYTES
    a0 = (1 << 29) + 0x803
    ranges = [(a0, a0 + 40), (a0 + 0x1000, a0 + 0x1000 + SCAN_STEPS + 1)]
    lo, hi = ranges[0][0] - 5, ranges[-1][1] + 5           # the columns that hold data: a little more than the ranges
    F, B = ko.contractive(k, SCAN_GAINS, 0.98, 12 + k)
    v, dv, init = rng.randn(k, hi - lo), rng.randn(k, hi - lo), rng.randn(len(ranges), k)
    outs = {}
    for j in range(k):
        s.read("ranges (v)", (Term(j, stride), Term(lo, 1, 8)), v[j].astype("<f8"), decoy=dv[j].astype("<f8"))
        for a, b in ranges:
            outs[(j, a)] = s.write("ranges (out)", (Term(j, stride), Term(a, 1, 8)), 8 * (b - a))
    s.seal()
    rebased = [(a - lo, b - lo) for a, b in ranges]
    ref = ko.serial_scan(v, rebased, F, B, init, out=v.copy())
    for j in range(k):
        for (a, b), (ra, rb) in zip(ranges, rebased):
            s.expect(outs[(j, a)], ref[j, ra:rb].astype("<f8"))
    s.crossing = [("8 * ranges[%d]" % (2 * r), 8 * a, "bytes") for r, (a, _b) in enumerate(ranges)]
    s.rules += [("the ranges start past column 2^29 and lie inside cols", ranges[0][0] >= 1 << 29 and ranges[-1][1] <= cols),
                ("cols is just under the arena's float64 count", ARENA_F64 - cols == 16),
                ("k rows fit: row stride at least 8 * cols, a multiple of 8, the last row inside the arena",
                 k == 1 or (stride >= 8 * cols and stride % 8 == 0 and (k - 1) * stride + 8 * cols <= size)),
                ("k = 2 does not fit the arena of 2^32 + 2^28 bytes", 2 * 8 * (1 << 29) > ARENA_BYTES),
                ("three tiles and a ragged one, behind a range with a tile of its own", ranges[1][1] - ranges[1][0] - 1 == 3 * SCAN_TILE + 9),
                ("the decoys give another result", not np.array_equal(ref[:, rebased[1][0] + 1:rebased[1][0] + 9],
                                                                      ko.serial_scan(dv, rebased, F, B, init, out=dv.copy())[:, rebased[1][0] + 1:rebased[1][0] + 9]))]

    def run(ctx):
        a_first, b_last = ranges[0][0], ranges[-1][1]
        _scan_expect(s, ctx, k, np.ascontiguousarray(v[:, a_first - lo:b_last - lo]), ranges, F, B, init, lambda j, a, b: outs[(j, a)])
        _scan_call(ctx, 0, stride, 0, stride, k, cols, ranges, F, B, init)
    s.run = run
    return s


for _k in ("value", "product"):
    for _far in ("v_row_stride", "out_row_stride", "in place"):
        _case("scan", "mhk_scan", _far, _k, "%d steps behind a short range, n_gain 5" % SCAN_STEPS, build_scan, _far, _k)
_case("scan", "mhk_scan", "ranges", "column", "k = 1, in place, cols = 2^29 + 2^25 - 16", build_scan_column, 1)
_case("scan2", "mhk_scan", "ranges", "column", "k = 2, in place, cols = 2^29 + 2^25 - 16, rows one arena apart", build_scan_column, 2, arena="A2")


# =====================================================================================================================
# the far column over the whole length: the calls that always walk [0, cols).  One row, one output; the far operand IS the
# arena, filled and compared on the device in chunks (tests/test_gpu_far_decoders.py).  cols = the column where the byte
# offset passes 2^32, a little more than one tile or run of the kernel, and a ragged end.
# =====================================================================================================================
GIB = 1 << 30
WHOLE_CHUNK = 1 << 26                   # columns filled or compared at a time
WHOLE = {
    # entry: (cols, element size of the far operand, free HBM asked for, what else is allocated)
    "mhw_xty": ((1 << 30) + XTY_RUN + 77, 4, ARENA_BYTES + 6 * GIB, "x of cols + 1 bytes, chunk temporaries"),
    "mhw_fir": ((1 << 30) + (FIR_TILE - 1) + 79, 4, ARENA_BYTES + 6 * GIB, "x of cols + 1 bytes, chunk temporaries"),
    "mhc_polyval": ((1 << 30) + POLY_TILE + 5, 4, ARENA_BYTES + 5 * GIB, "chunk temporaries"),
    "mhs_box_f32": ((1 << 30) + BOXF_TILE + 5, 4, 2 * ARENA_BYTES + 5 * GIB, "the input, a second buffer of the arena's size; chunk temporaries"),
    "mhk_project": ((1 << 29) + PROJ_TILE + 5, 8, ARENA_BYTES + 6 * GIB, "x of cols bytes, chunk temporaries"),
}
