"""The moving-average window on the GPU (include/muahuff_smooth.h, csrc/mh_smooth.hpp, smooth.py, wiener.stats(window=)).
mhs_box against NumPy's integer box sums -- equal, both planes, nothing around the rows written -- over every byte
alignment of x, tiles, halos, windows and clips, past the grid cap and with row strides beyond 2^32; mhs_box_f32 against
the integer result on integer input -- equal -- and within its float64 chain's bound on general floats; wiener.stats with
a window against the explicit smoothed design matrix; WienerFilter and cascade.cross_validate against the oracle's; and
the contract: graph capture and replay, and return before the stream drains."""
import time

import numpy as np
import pytest
import torch

import muahuff
from muahuff import _smooth, cascade, smooth, wiener
from tests import box_oracle as bo
from tests import cascade_oracle as co
from tests import wiener_oracle as wo
from tests.test_gpu_cascade import CV_REF
from tests.test_gpu_wiener import _counts, _dev, _devf, _gamma
from tests.test_host_box import D_BOX, D_BOX_W, MAX_BLOCKS, TILE_COLS, box_data
from tests.test_host_cascade import nonlinear_data
from tests.test_host_wiener import D_REF, D_REF_W

pytestmark = pytest.mark.gpu

F32_TILE = 256                                                     # mh_smooth_layout.hpp: kBoxfTile


def _planes(rows, cols, two=True, extra=16):
    """(lo, hi): pitched uint8 device views [rows, cols] as mhs_box takes them -- first byte and pitch multiples of 16 --
    with 255 in every byte around the rows; hi None for one plane"""
    pitch = (cols + 15) // 16 * 16 + extra
    out = []
    for _ in range(2 if two else 1):
        buf = torch.full((rows * pitch + 64,), 255, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        out.append(buf.as_strided((rows, cols), (pitch, 1), 32))
    return out[0], (out[1] if two else None)


def _untouched(view, rows, cols):
    """every byte of the view's buffer outside its rows is still 255"""
    flat = view._base.cpu().numpy()
    around = np.ones(flat.size, bool)
    around[(32 + np.arange(rows)[:, None] * view.stride(0) + np.arange(cols)[None, :]).ravel()] = False
    return bool((flat[around] == 255).all())


def _box(xv, cols, window, clip, two=True):
    """one mhs_box on the view xv [rows, cols + window - 1] -> (lo, hi) device views"""
    rows = xv.shape[0]
    lo, hi = _planes(rows, cols, two)
    _smooth.box(xv.data_ptr(), xv.stride(0) if rows > 1 else 0, rows, cols, window, clip, lo, hi)
    return lo, hi


def _same(lo, hi, want):
    got = lo.cpu().numpy().astype(np.int64) + (256 * hi.cpu().numpy().astype(np.int64) if hi is not None else 0)
    return np.array_equal(got, want)


COLS = (1, 63, TILE_COLS + 1, 3 * TILE_COLS + 5)
WINDOWS = (1, 2, 5, 200, 256)
CLIPS = (1, 2, 39, 255)


@pytest.mark.parametrize("rows", [1, 5, 70])
def test_box_equals_numpy_on_both_planes(rows):
    """every (cols, window, clip) of the three axes; the first byte of x cycles through the offsets 0..15"""
    i = 0
    for cols in COLS:
        x = _counts(rows, cols + 255, 10 * rows + cols % 7)
        wide = np.random.RandomState(rows + cols).randint(0, 256, x.shape).astype(np.uint8)
        x[:, ::3] = wide[:, ::3]                                   # counts on both sides of every clip
        for window in WINDOWS:
            xs = x[:, :cols + window - 1]
            xv = _dev(xs, lead=(i * 5 + rows) % 16, extra=37 + i % 3)
            for clip in CLIPS:
                want = bo.box(xs, window, clip)
                lo, hi = _box(xv, cols, window, clip)
                assert _same(lo, hi, want), (rows, cols, window, clip)
                assert _untouched(lo, rows, cols) and _untouched(hi, rows, cols)
                if window * clip <= 255:                           # one plane where it is enough
                    one, _none = _box(xv, cols, window, clip, two=False)
                    assert _same(one, None, want) and _untouched(one, rows, cols) and not hi.any()
                if i % 7 == 0:                                     # two calls give identical bytes
                    lo2, hi2 = _box(xv, cols, window, clip)
                    assert torch.equal(lo, lo2) and torch.equal(hi, hi2)
                i += 1


@pytest.mark.parametrize("window,clip", [(5, 39), (256, 255), (1, 2)])
def test_box_with_the_first_byte_of_x_at_every_offset(window, clip):
    rows, cols = 3, TILE_COLS + 1
    x = _counts(rows, cols + window - 1, window)
    want = bo.box(x, window, clip)
    for lead in range(16):
        lo, hi = _box(_dev(x, lead=lead, extra=1 + lead % 4), cols, window, clip)
        assert _same(lo, hi, want), lead
        assert _untouched(lo, rows, cols) and _untouched(hi, rows, cols)


def test_box_where_one_plane_ends_and_two_begin():
    """window * clip = 255: hi may be NULL; 256: it may not, and with hi given the 256s come out as lo 0, hi 1"""
    for window, clip in ((5, 51), (255, 1), (1, 255), (3, 85)):
        x = np.full((2, 400 + window - 1), 255, np.uint8)
        x[:, 7::300] = 0                                           # (at least one whole window between two of them)
        lo, _none = _box(_dev(x, lead=3), 400, window, clip, two=False)
        got = lo.cpu().numpy()
        assert np.array_equal(got, bo.box(x, window, clip)) and got.max() == 255
    for window, clip in ((4, 64), (256, 1), (16, 16)):
        x = np.full((2, 400 + window - 1), 255, np.uint8)
        x[:, 7::300] = 0                                           # (at least one whole window between two of them)
        xv = _dev(x, lead=5)
        lo, hi = _box(xv, 400, window, clip)
        want = bo.box(x, window, clip)
        assert want.max() == 256 and _same(lo, hi, want)
        one, _none = _planes(2, 400, two=False)
        with pytest.raises(muahuff.MuaHuffError, match="hi is NULL"):
            _smooth.box(xv.data_ptr(), xv.stride(0), 2, 400, window, clip, one, None)
        assert (one == 255).all()                                  # refused before any device work
    with pytest.raises(ValueError):
        smooth.box_sum(_dev(x), 257)


def test_box_of_all_255_at_the_widest_window_is_65280_everywhere():
    rows, cols = 5, TILE_COLS + 1
    xv = _dev(np.full((rows, cols + 255), 255, np.uint8), lead=9)
    lo, hi = _box(xv, cols, 256, 255)
    assert (lo == 0).all() and (hi == 255).all()                   # 65280 = 255 * 256
    lo, hi = smooth.box_sum(xv, 256)
    assert tuple(lo.shape) == (rows, cols) and (lo == 0).all() and (hi == 255).all()
    ma = smooth.moving_average(xv, 256)
    assert ma.dtype == torch.float32 and (ma == 255.0).all()
    lo, hi = smooth.box_sum(xv, 5, clip=51)
    assert hi is None and (lo == 255).all()


def test_box_past_the_grid_cap():
    """one row, a column more than the capped grid has tiles: the stride loop's second trip"""
    cols, window = MAX_BLOCKS * TILE_COLS + 1, 2
    x = _counts(1, cols + window - 1, 3)
    lo, hi = _box(_dev(x, lead=1), cols, window, 255)
    assert _same(lo, hi, bo.box(x, window))
    assert _untouched(lo, 1, cols) and _untouched(hi, 1, cols)


# ---- strides beyond 2^32 --------------------------------------------------------------------------------------------------
ARENA_BYTES = (1 << 32) + (1 << 28)


@pytest.fixture(scope="module")
def arena():
    """2^32 + 2^28 bytes, never touched as a whole"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    if free < ARENA_BYTES + (2 << 30):
        pytest.skip("the arena of 2^32 + 2^28 bytes (+ 2 GiB for the small tensors) needs more free HBM than %.1f GB" % (free / 1e9))
    a = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


def test_box_with_an_input_row_stride_beyond_2_to_the_32(arena):
    """two rows 2^32 + 4099 bytes apart; where a 32-bit row offset would look for the second row lies a decoy"""
    cols, window, clip = TILE_COLS + 70, 50, 39
    n = cols + window - 1
    stride, first = (1 << 32) + 4099, 13
    x = _counts(2, n, 61)
    decoy = 255 - x[1]
    assert first + stride + n <= ARENA_BYTES and first + n < first + 4099
    for off, row in ((first, x[0]), (first + 4099, decoy), (first + stride, x[1])):
        arena[off - 8:off + n + 8] = 255
        arena[off:off + n] = torch.from_numpy(row).cuda()
    lo, hi = _planes(2, cols)
    _smooth.box(arena.data_ptr() + first, stride, 2, cols, window, clip, lo, hi)
    assert _same(lo, hi, bo.box(x, window, clip))
    assert not np.array_equal(bo.box(x, window, clip)[1], bo.box(decoy[None, :], window, clip)[0])


def test_box_with_an_output_row_stride_beyond_2_to_the_32(arena):
    """the planes' second rows lie 2^32 + 65536 bytes behind the first; where a 32-bit offset would write them lie canaries"""
    cols, window, clip = 4001, 200, 39
    stride, at_lo, at_hi = (1 << 32) + 65536, 256, (1 << 20) + 256
    assert arena.data_ptr() % 16 == 0 and at_hi + stride + cols <= ARENA_BYTES
    x = _counts(2, cols + window - 1, 62)
    for at in (at_lo, at_hi):
        for off in (at, at + 65536, at + stride):
            arena[off - 16:off + cols + 16] = 0xA5
    lo, hi = arena.as_strided((2, cols), (stride, 1), at_lo), arena.as_strided((2, cols), (stride, 1), at_hi)
    xv = _dev(x, lead=7)
    _smooth.box(xv.data_ptr(), xv.stride(0), 2, cols, window, clip, lo, hi)
    torch.cuda.synchronize()
    want = bo.box(x, window, clip)
    for r in range(2):
        got = arena[at_lo + r * stride:at_lo + r * stride + cols].cpu().numpy().astype(np.int64) \
            + 256 * arena[at_hi + r * stride:at_hi + r * stride + cols].cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want[r]), r
    for at in (at_lo, at_hi):
        assert (arena[at + 65536 - 16:at + 65536 + cols + 16] == 0xA5).all()                    # the 32-bit alias of row 1
        for off in (at, at + stride):
            assert (arena[off - 16:off] == 0xA5).all() and (arena[off + cols:off + cols + 16] == 0xA5).all()


# ---- mhs_box_f32 ----------------------------------------------------------------------------------------------------------
def _box_f32(p, window, bias, lead=2, extra=3):
    """one mhs_box_f32 on p [k, cols] (NumPy) -> a pitched device view with nan around its rows"""
    pv = _devf(np.ascontiguousarray(p, np.float32), lead=1, extra=7)
    out = _devf(np.full(p.shape, np.nan, np.float32), lead, extra)
    _smooth.box_f32(pv, window, torch.from_numpy(np.ascontiguousarray(bias, np.float32)).cuda(), out)
    return out


@pytest.mark.parametrize("window", [1, 2, 50, 256])
def test_box_f32_equals_the_integer_result(window):
    """integer input whose every partial sum stays below 2^24: the float64 chain and the float32 result are exact"""
    for k in (1, 3, 8):
        for cols in sorted({1, max(window - 1, 1), window, 3 * F32_TILE + 5}):
            rng = np.random.RandomState(1000 * window + 10 * k + cols % 9)
            p = rng.randint(-30000, 30001, (k, cols)).astype(np.int64)
            bias = rng.randint(-1000, 1001, (k,)).astype(np.int64)
            want, mag = bo.box_f32(p, window, bias)
            assert mag.max() < 2 ** 24
            out = _box_f32(p, window, bias, lead=1 + k % 3)
            again = _box_f32(p, window, bias, lead=1 + k % 3)
            got = out.cpu().numpy()
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want), (k, cols)
            assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32))
            flat = out._base.cpu().numpy()
            assert np.isnan(flat).sum() == flat.size - k * cols     # nothing around the rows was written


def test_box_f32_past_the_grid_cap():
    """more (tile, output) items than the capped grid has workgroups"""
    k, cols, window = 8, (4096 // 8) * F32_TILE + 300, 3
    p = np.random.RandomState(7).randint(-1000, 1001, (k, cols)).astype(np.int64)
    bias = np.arange(k).astype(np.int64)
    assert -(-cols // F32_TILE) * k > 4096
    got = _box_f32(p, window, bias).cpu().numpy()
    assert np.array_equal(got.astype(np.int64), bo.box_f32(p, window, bias)[0])


def test_box_f32_on_general_floats_is_within_the_chain_bound():
    """|got - ref| <= window * 2^-53 * (|bias| + sum |in|) + 2^-24 * |out|: at most `window` float64 additions, each within
    2^-53 of the magnitudes added so far, and one rounding to float32"""
    k, cols = 3, 3 * F32_TILE + 5
    rng = np.random.RandomState(8)
    p = (rng.randn(k, cols) * 50).astype(np.float32)
    bias = rng.randn(k).astype(np.float32)
    for window in (2, 50, 256):
        ref, mag = bo.box_f32(p, window, bias)
        a, b = _box_f32(p, window, bias).cpu().numpy(), _box_f32(p, window, bias).cpu().numpy()
        bound = window * 2.0 ** -53 * mag + 2.0 ** -24 * np.abs(ref)
        err = np.abs(a.astype(np.longdouble) - ref)
        print("\nbox_f32 general floats, window %d: worst error / bound = %.3g" % (window, float((err / bound).max())))
        assert (err <= bound).all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- stats, fit, predict, score ----------------------------------------------------------------------------------------
C, L, K, T, LEAD = 7, 5, 2, 4000, 3


@pytest.fixture(scope="module")
def world():
    x, y = box_data()
    return x, y, _dev(x, lead=1), _devf(y, lead=2)


def _xty_close(got, r):
    """2 n * 2^-53 * sum |x y|, elementwise: the order-free float64 bound of the per-plane sums (n * 2^-53 each way of
    summing exact products) plus one rounding per batch, per warm-up piece and for the combine, fewer than n in all"""
    return (np.abs(got - r["xty"]) <= 2 * r["n"] * 2.0 ** -53 * r["abs_xty"]).all()


@pytest.mark.parametrize("w,clip", [(4, 2), (50, None)])
def test_window_stats_equal_the_explicit_smoothed_design(world, w, clip):
    x, y, xv, yv = world
    s = wiener.stats(xv, yv, L, LEAD, clip, window=w)[0]
    r = bo.stats(x, y, L, LEAD, clip, w)
    assert s.n == r["n"] == T - LEAD - (L - 1) and (s.lags, s.lead, s.clip, s.channels, s.window) == (L, LEAD, clip or 255, C, w)
    assert s.gram.dtype == torch.int64 and np.array_equal(s.gram.cpu().numpy(), r["gram"])
    assert s.sum_x.dtype == torch.int64 and np.array_equal(s.sum_x.cpu().numpy(), r["sum_x"])
    assert s.xty.dtype == torch.float64 and _xty_close(s.xty.cpu().numpy(), r)
    assert np.allclose(s.sum_y.cpu().numpy(), r["sum_y"], rtol=1e-12, atol=1e-9) and np.allclose(s.sum_yy.cpu().numpy(), r["sum_yy"], rtol=1e-12)
    # ranges that tile the rows: the first lies wholly inside the warm-up, the second is cut by its end, one is empty;
    # batches of 300 bins, so every batch carries its halo of L-1 + w-1 columns
    end = L - 1 + w - 1
    rs = [(L - 1, L - 1 + max(w // 2, 1)), (L - 1 + max(w // 2, 1), end + 11), (end + 11, end + 11), (end + 11, 2501), (2501, T - LEAD)]
    assert rs[0][1] < end < rs[1][1]
    parts = wiener.stats(xv, yv, L, LEAD, clip, ranges=rs, max_bytes=C * 300, window=w)
    for (a, b), p in zip(rs, parts):
        rr = bo.stats(x, y, L, LEAD, clip, w, a, b)
        assert p.n == rr["n"] == b - a and p.window == w
        assert np.array_equal(p.gram.cpu().numpy(), rr["gram"]) and np.array_equal(p.sum_x.cpu().numpy(), rr["sum_x"]), (a, b)
        assert _xty_close(p.xty.cpu().numpy(), rr)
    tot = sum(parts)
    assert tot.n == s.n and tot.window == w and torch.equal(tot.gram, s.gram) and torch.equal(tot.sum_x, s.sum_x)
    assert _xty_close(tot.xty.cpu().numpy(), r)
    with pytest.raises(ValueError):
        parts[0] + wiener.stats(xv, yv, L, LEAD, clip, ranges=[rs[1]])[0]       # no window
    for bad in (0, 257, -3):                                       # stats' own check of the window, on device operands
        with pytest.raises(ValueError, match="window"):
            wiener.stats(xv, yv, L, LEAD, clip, window=bad)
    # window 1 is the route without a window, bit for bit
    a, b = wiener.stats(xv, yv, L, LEAD, clip, window=1)[0], wiener.stats(xv, yv, L, LEAD, clip)[0]
    assert a.window == 1 and torch.equal(a.gram, b.gram) and torch.equal(a.xty, b.xty)


@pytest.mark.parametrize("w,clip", [(4, 2), (50, None), (200, 39)])
def test_the_window_filter_fits_predicts_and_scores_as_the_oracle(world, w, clip):
    x, y, xv, yv = world
    s = wiener.stats(xv, yv, L, LEAD, clip, window=w)[0]
    f = wiener.WienerFilter(1e-2).fit(s)
    h = s.to("cpu")
    wt, b = wo.fit_from_stats(h.n, h.sum_x.numpy(), h.gram.numpy(), h.xty.numpy(), h.sum_y.numpy(), 1e-2, L, C)
    scale = np.abs(wt).max()
    gw, gb = f.weights.cpu().numpy(), f.bias.cpu().numpy()
    print("\nwindow %d fit: weights differ by %.3g, bias by %.3g of the largest weight" % (w, np.abs(gw - wt).max() / scale, np.abs(gb - b).max() / scale))
    assert f.window == w and f.weights.is_cuda and gw.shape == (K, L, C)
    assert np.abs(gw - wt).max() <= 64 * D_BOX_W[w] * scale and np.abs(gb - b).max() <= 64 * D_BOX[w] * scale
    # predict: the box sum of the float64 filter output with the filter's own weights; each of the (at most w) summed
    # columns carries mhw_fir's chain bound and the cast of its weights, the sum itself mhs_box_f32's bound
    pred = f.predict(xv)
    p = pred.cpu().numpy()
    assert p.dtype == np.float32 and p.shape == (K, T - L + 1)
    zero = np.zeros(K)
    fir, mag = wo.fir(x, gw, zero, L, clip)
    ref, in_mag = bo.box_f32(fir, w, gb)
    boxed_mag, _m = bo.box_f32(mag, w, zero)
    bound = (_gamma(C + L + 1) + 2.0 ** -24) * boxed_mag + w * 2.0 ** -53 * in_mag + 2.0 ** -24 * np.abs(ref)
    err = np.abs(p.astype(np.longdouble) - ref)
    print("window %d predict: worst error / bound = %.3g" % (w, float((err / bound).max())))
    assert (err <= bound).all()
    # column i is design row L-1 + i: the features of the explicit smoothed design times the weights
    X, _Y = bo.design(x, y, L, LEAD, clip, w)
    lin = X.astype(np.float64) @ gw.reshape(K, L * C).T + gb
    assert np.allclose(p[:, :len(X)].T, lin, rtol=0, atol=1e-4 * np.abs(lin).max())
    # score: over the columns whose target exists
    rmse, cc = f.score(xv, yv)
    n = T - L + 1 - LEAD
    ytrue, ypred = y[:, L - 1 + LEAD:].T.astype(np.float64), p[:, :n].T.astype(np.float64)
    assert np.allclose(rmse.cpu().numpy(), wo.rmse(ytrue, ypred), rtol=1e-6, atol=0)
    assert np.allclose(cc.cpu().numpy(), wo.pearson(ytrue, ypred), rtol=1e-6, atol=0)


def test_cross_validate_with_a_window_gives_the_arrays_of_the_oracles_loop():
    """the loop of tests/cascade_oracle.py on the explicit smoothed design of tests/box_oracle.py.  The tolerance is that of
    tests/test_gpu_cascade.py for the unsmoothed case, 64 * CV_REF, widened by the ratio of this window's recorded D_BOX
    constants to D_REF (the larger of the weights' and the bias's ratio): the smoothed lags are that much closer to
    collinear, and every difference between two solvers grows with it."""
    w, F, alphas, degrees = 50, 5, (1e-2,), (None, 3)
    x, y = nonlinear_data()
    xv, yv = _dev(x, lead=1), _devf(y, lead=2)
    got = cascade.cross_validate(xv, yv, L, LEAD, None, alphas, degrees, F, window=w)
    X, Y = bo.design(x, y, L, LEAD, None, w)
    allowed = 64 * CV_REF * max(D_BOX_W[w] / D_REF_W, D_BOX[w] / D_REF)
    worst = 0.0
    for i, (tr, va, te) in enumerate(wo.split_index(len(X), F)):
        for a in alphas:
            for d in degrees:
                wt, b, coefs = co.cascade_fit(X[tr], Y[tr], a, d)
                for name, idx in (("valid", va), ("test", te)):
                    pred = co.cascade_predict(X[idx], wt, b, coefs)
                    for kind, want in (("rmse_", wo.rmse(Y[idx], pred)), ("cc_", wo.pearson(Y[idx], pred))):
                        g = got[(a, d)][kind + name]
                        assert g.dtype == torch.float64 and tuple(g.shape) == (F, K)
                        rel = np.abs(g[i].cpu().numpy() - want) / np.abs(want)
                        worst = max(worst, rel.max())
                        assert (rel <= allowed).all(), (i, a, d, kind + name, rel.max())
    print("\ncross_validate, window %d: worst relative difference from the oracle's loop %.3g (allowed %.3g)" % (w, worst, allowed))


# ---- the contract -------------------------------------------------------------------------------------------------------
DELAY_BYTES, DELAY_PASSES = 512 << 20, 24     # as tests/test_gpu_async_contract.py: tens of milliseconds on the device


def _pair(xv, cols, window, clip, lo, hi, pv, bias, out):
    _smooth.box(xv.data_ptr(), xv.stride(0), xv.shape[0], cols, window, clip, lo, hi)
    _smooth.box_f32(pv, window, bias, out)


def test_the_pair_is_captured_replayed_and_returns_before_the_stream_drains():
    rows, cols, window, clip, k = 5, TILE_COLS + 3, 50, 39, 2
    x = _counts(rows, cols + window - 1, 31)
    pi = np.random.RandomState(32).randint(-30000, 30001, (k, cols)).astype(np.int64)
    bi = np.array([5, -7], np.int64)
    xv, pv = _dev(x), _devf(pi.astype(np.float32))
    bias = torch.from_numpy(bi.astype(np.float32)).cuda()
    want_box, want_f32 = bo.box(x, window, clip), bo.box_f32(pi, window, bi)[0].astype(np.float32)
    lo, hi = _planes(rows, cols)
    out = torch.zeros((k, cols), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _pair(xv, cols, window, clip, lo, hi, pv, bias, out)           # eager, and the warm-up
    side.synchronize()
    assert _same(lo, hi, want_box) and np.array_equal(out.cpu().numpy(), want_f32)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _pair(xv, cols, window, clip, lo, hi, pv, bias, out)
    lo.fill_(7), hi.fill_(7), out.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert _same(lo, hi, want_box) and np.array_equal(out.cpu().numpy(), want_f32)
    # behind a delay on the stream: both calls return while the delay is still running
    lo.fill_(7), hi.fill_(7), out.fill_(-1)
    delay = torch.zeros(DELAY_BYTES // 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(side):
        for _ in range(DELAY_PASSES):
            delay.add_(1)
        ev.record()
        t0 = time.perf_counter()
        _pair(xv, cols, window, clip, lo, hi, pv, bias, out)
        t1 = time.perf_counter()
        pending = not ev.query()
    side.synchronize()
    assert pending, "the delay had completed when the calls returned (host enqueue %.3f ms)" % (1e3 * (t1 - t0))
    assert _same(lo, hi, want_box) and np.array_equal(out.cpu().numpy(), want_f32)
