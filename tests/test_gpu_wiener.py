"""The Wiener filter on the GPU (include/muahuff_wiener.h, csrc/mh_wiener.hpp, wiener.py).  mhw_xty against NumPy's int64
product on dyadic covariates -- equal, not close -- over every byte alignment of x, runs, lag blocks and clips, and within
the order-free float64 bound on general floats; mhw_fir against the int64 result on integer weights -- equal: a wrong lane
map, M-tile or halo shows -- and within the f32 chain's bound on general floats; wiener.stats against the explicit design
matrix; WienerFilter against the oracle's solve, product and scores; folds; and the contract: graph capture and replay,
and return before the stream drains."""
import time

import numpy as np
import pytest
import torch

from muahuff import _wiener, wiener
from tests import wiener_oracle as wo
from tests.test_host_wiener import D_REF, D_REF_W, FIR_MAX_BLOCKS, RUN, TILE_COLS, data, layout
from tests.test_host_wiener import MAX_BLOCKS as XTY_MAX_BLOCKS

pytestmark = pytest.mark.gpu


def _dev(x, lead=1, extra=37):
    """the matrix as a pitched device view whose first byte sits at `lead` mod 128, every byte around the rows 255"""
    rows, cols = x.shape
    pitch = cols + extra
    buf = torch.full((rows * pitch + lead + 256,), 255, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 128 == 0
    view = buf.as_strided((rows, cols), (pitch, 1), lead)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    return view


def _devf(y, lead=3, extra=5, fill=float("nan")):
    """a float32 matrix as a pitched device view (odd pitch, `lead` floats in), nan around the rows"""
    rows, cols = y.shape
    pitch = cols + extra
    buf = torch.full((rows * pitch + lead + 64,), fill, dtype=torch.float32, device="cuda")
    view = buf.as_strided((rows, cols), (pitch, 1), lead)
    view.copy_(torch.from_numpy(np.ascontiguousarray(y)).cuda())
    return view


def _counts(rows, cols, seed):
    rng = np.random.RandomState(seed)
    x = np.minimum(rng.poisson(0.8, size=(rows, cols)), 255).astype(np.uint8)
    x[rng.rand(rows, cols) < 0.05] = 255
    x[rng.rand(rows, cols) < 0.05] = 2
    return x


def _xty(xv, yv, lags, clip, out=None, accumulate=False):
    """one mhw_xty on views xv [rows, cols + lags - 1] and yv [k, cols] -> the device result [lags, rows, k]"""
    rows, k, cols = xv.shape[0], yv.shape[0], yv.shape[1]
    if out is None:
        out = torch.full((lags, rows, k), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.full((_wiener.xty_scratch_bytes(rows, cols, lags, k),), 0xFF, dtype=torch.uint8, device="cuda")
    _wiener.xty(xv.data_ptr(), xv.stride(0) if rows > 1 else 0, rows, cols, lags, clip, yv.data_ptr(),
                4 * yv.stride(0) if k > 1 else 0, k, out, scratch, accumulate)
    return out


def _fir(xv, w, bias, lags, clip, lead=2, extra=3):
    """one mhw_fir on the view xv [rows, cols + lags - 1] with w [k, lags, rows], bias [k] (NumPy) -> out [k, cols], a
    pitched device view with nan around its rows"""
    rows, k, cols = xv.shape[0], w.shape[0], xv.shape[1] - lags + 1
    out = _devf(np.full((k, cols), np.nan, np.float32), lead, extra)
    wd = torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda()
    bd = torch.from_numpy(np.ascontiguousarray(bias, np.float32)).cuda()
    _wiener.fir(xv.data_ptr(), xv.stride(0) if rows > 1 else 0, rows, cols, lags, clip, wd, bd, k, out)
    return out


# (rows, lags, k, cols, clip): every value of every axis the exactness can depend on, each byte alignment of x (the
# first-byte offset cycles 0..3 and lags - 1 - l shifts it), one run, a run and a bit, three and a bit
XTY_SHAPES = [(1, 1, 1, 1, 255), (5, 4, 2, 63, 2), (70, 5, 8, RUN + 3, 1), (70, 32, 2, 3 * RUN + 5, 255), (5, 32, 8, 63, 255),
              (1, 4, 1, 3 * RUN + 5, 2), (70, 1, 2, 1, 255), (5, 5, 1, RUN + 3, 255), (1, 32, 8, 1, 1), (70, 4, 8, 63, 255),
              (5, 1, 2, 3 * RUN + 5, 2), (1, 5, 2, RUN + 3, 1)]


@pytest.mark.parametrize("i,shape", list(enumerate(XTY_SHAPES)), ids=["%dx%d-L%d-K%d-q%d" % (s[0], s[3], s[1], s[2], s[4]) for s in XTY_SHAPES])
def test_xty_equals_the_integer_product_on_dyadic_covariates(i, shape):
    rows, lags, k, cols, clip = shape
    rng = np.random.RandomState(100 + i)
    x = _counts(rows, cols + lags - 1, i)
    yi = rng.randint(-4096, 4097, (k, cols)).astype(np.int64)          # y = yi / 64: multiples of 2^-6, |y| <= 64
    y = (yi / 64.0).astype(np.float32)
    assert np.array_equal(y.astype(np.float64) * 64, yi) and ((x == 255).any() or x.size < 200)
    xq = np.minimum(x, clip).astype(np.int64)
    want = np.stack([xq[:, lags - 1 - l:lags - 1 - l + cols] @ yi.T for l in range(lags)]).astype(np.float64) / 64.0
    xv, yv = _dev(x, lead=i % 4, extra=37), _devf(y, lead=1 + i % 3)
    out = _xty(xv, yv, lags, clip)
    again = _xty(xv, yv, lags, clip)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(again.cpu().numpy().view(np.uint64), got.view(np.uint64))    # identical bits
    _xty(xv, yv, lags, clip, out=out, accumulate=True)                                 # accumulate: twice the result
    assert np.array_equal(out.cpu().numpy(), 2 * want)
    _xty(xv, yv, lags, clip, out=out, accumulate=False)                                # ... and overwrite
    assert np.array_equal(out.cpu().numpy(), want)


def test_xty_every_first_byte_offset_and_every_lag_block():
    """lags = 9, 16, 17: one lag past a block of 8, two whole blocks, one past two; the first byte at 0..3 mod 4"""
    for lead in range(4):
        for lags in (9, 16, 17):
            rows, k, cols = 3, 3, 1000 + lead
            x = _counts(rows, cols + lags - 1, 7 * lead + lags)
            yi = np.random.RandomState(lags).randint(-4096, 4097, (k, cols)).astype(np.int64)
            want = np.stack([x.astype(np.int64)[:, lags - 1 - l:lags - 1 - l + cols] @ yi.T for l in range(lags)]) / 64.0
            got = _xty(_dev(x, lead=lead, extra=1), _devf((yi / 64.0).astype(np.float32)), lags, 255).cpu().numpy()
            assert np.array_equal(got, want), (lead, lags)


def test_xty_past_both_grid_caps():
    """4100 channels are more (run, channel) items than the first kernel's capped grid has workgroups, and 4100 x 32 x 8
    elements more than the second's has threads: the second trip of both stride loops"""
    rows, lags, k, cols = 4100, 32, 8, 63
    lay = layout(rows, cols, lags, k)
    assert lay[1] > lay[4] == XTY_MAX_BLOCKS and lay[5] > lay[6] * 256 and lay[6] == XTY_MAX_BLOCKS
    rng = np.random.RandomState(5)
    x = rng.randint(0, 4, (rows, cols + lags - 1)).astype(np.uint8)
    x[rng.rand(*x.shape) < 0.01] = 255
    yi = rng.randint(-4096, 4097, (k, cols)).astype(np.int64)
    xq = x.astype(np.int64)
    want = np.stack([xq[:, lags - 1 - l:lags - 1 - l + cols] @ yi.T for l in range(lags)]) / 64.0
    got = _xty(_dev(x, lead=2, extra=3), _devf((yi / 64.0).astype(np.float32)), lags, 255).cpu().numpy()
    assert np.array_equal(got, want)


def test_xty_on_general_floats_is_within_the_order_free_float64_bound():
    """|got - ref| <= cols * 2^-53 * sum |x y|: any order of summing exact products in float64 stays inside it"""
    rows, lags, k, cols = 70, 15, 2, 3 * RUN + 5
    x = _counts(rows, cols + lags - 1, 11)
    y = (np.random.RandomState(12).randn(k, cols) * 3).astype(np.float32)
    ref, mag = wo.xty(x, y, lags, 255)
    xv, yv = _dev(x, lead=3), _devf(y)
    a, b = _xty(xv, yv, lags, 255).cpu().numpy(), _xty(xv, yv, lags, 255).cpu().numpy()
    err = np.abs(a - ref)
    print("\nxty general floats: worst error / bound = %.3g" % (err / (cols * 2.0 ** -53 * mag)).max())
    assert (err <= cols * 2.0 ** -53 * mag).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _tile(lags):
    return TILE_COLS - (lags - 1)


# (rows, lags, k, cols, clip): one, two (a pair), three (a pair and an odd one) and 70 channels; k = 3 at 15 lags needs
# two M-tiles, k = 8 at 32 lags eight; one column, 127, a workgroup tile and one, three tiles and five
FIR_SHAPES = [(70, 15, 2, 3 * _tile(15) + 5, 255), (70, 15, 3, _tile(15) + 1, 2), (70, 32, 8, _tile(32) + 1, 255), (1, 1, 1, 1, 255),
              (2, 5, 2, 127, 1), (3, 5, 3, 3 * _tile(5) + 5, 255), (3, 32, 1, 127, 2), (1, 15, 8, _tile(15) + 1, 255),
              (2, 1, 2, _tile(1) + 1, 255), (70, 5, 8, 127, 255), (70, 1, 3, 3 * _tile(1) + 5, 2), (3, 15, 3, 1, 255),
              (2, 32, 8, 3 * _tile(32) + 5, 1), (1, 5, 1, 1, 1)]


def _int_filter(rows, lags, k, seed):
    rng = np.random.RandomState(seed)
    w = rng.randint(-7, 8, (k, lags, rows)).astype(np.int64)
    # every (output, lag, channel) distinguishable: a swapped row of the M-tile or channel of the pair changes the sums
    return w, rng.randint(-100, 101, (k,)).astype(np.int64)


@pytest.mark.parametrize("i,shape", list(enumerate(FIR_SHAPES)), ids=["%dx%d-L%d-K%d-q%d" % (s[0], s[3], s[1], s[2], s[4]) for s in FIR_SHAPES])
def test_fir_equals_the_integer_result_on_integer_weights(i, shape):
    rows, lags, k, cols, clip = shape
    x = _counts(rows, cols + lags - 1, 50 + i)
    w, bias = _int_filter(rows, lags, k, 70 + i)
    want, mag = wo.fir(x, w, bias, lags, clip)
    assert mag.max() < 2 ** 24                                           # every partial sum is an exact float32
    xv = _dev(x, lead=i % 4, extra=37 + i % 2)
    out = _fir(xv, w, bias, lags, clip)
    again = _fir(xv, w, bias, lags, clip)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32))
    base = out._base if out._base is not None else out                    # nothing around the rows was written
    flat = base.cpu().numpy()
    assert np.isnan(flat).sum() == flat.size - k * cols


def test_fir_past_the_grid_cap():
    """one channel, one lag, one output, a column more than the capped grid has tiles: the stride loop's second trip"""
    cols = FIR_MAX_BLOCKS * TILE_COLS + 1
    assert layout(1, cols, 1, 1)[11:] == [FIR_MAX_BLOCKS + 1, FIR_MAX_BLOCKS]
    x = _counts(1, cols, 3)
    w, bias = np.array([[[3]]], np.int64), np.array([-5], np.int64)
    got = _fir(_dev(x, lead=1), w, bias, 1, 255).cpu().numpy()
    assert np.array_equal(got.astype(np.int64), 3 * x.astype(np.int64) - 5)


def _gamma(n):
    return n * 2.0 ** -24 / (1 - n * 2.0 ** -24)


def test_fir_on_general_floats_is_within_the_chain_bound():
    """|got - ref| <= gamma_n (|b| + sum |w| x), n = rows + lags + 1: the length of the longest chain an output can be"""
    rows, lags, k, cols = 70, 15, 2, 3 * _tile(15) + 5
    rng = np.random.RandomState(21)
    x = _counts(rows, cols + lags - 1, 22)
    w = rng.randn(k, lags, rows).astype(np.float32)
    bias = rng.randn(k).astype(np.float32)
    ref, mag = wo.fir(x, w.astype(np.float64), bias.astype(np.float64), lags, 255)
    xv = _dev(x, lead=1)
    a, b = _fir(xv, w, bias, lags, 255).cpu().numpy(), _fir(xv, w, bias, lags, 255).cpu().numpy()
    bound = _gamma(rows + lags + 1) * mag
    err = np.abs(a.astype(np.float64) - ref)
    print("\nfir general floats: worst error / bound = %.3g" % (err / bound).max())
    assert (err <= bound).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- stats, fit, predict, score ----------------------------------------------------------------------------------------
C, L, K, T, LEAD = 7, 5, 2, 4000, 3


@pytest.fixture(scope="module")
def world():
    x, y = data(C, L, K, T)
    return x, y, _dev(x, lead=1), _devf(y, lead=2)


def _xty_close(got, r):
    """the mhw_xty bound on the statistics: n * 2^-53 * sum |x y|, elementwise"""
    return (np.abs(got - r["xty"]) <= r["n"] * 2.0 ** -53 * r["abs_xty"]).all()


@pytest.mark.parametrize("clip", [None, 2])
def test_stats_equal_the_explicit_design_matrix(world, clip):
    x, y, xv, yv = world
    s = wiener.stats(xv, yv, L, LEAD, clip)[0]
    r = wo.stats(x, y, L, LEAD, clip)
    assert s.n == r["n"] == T - LEAD - (L - 1) and (s.lags, s.lead, s.clip, s.channels) == (L, LEAD, clip or 255, C)
    assert s.gram.dtype == torch.int64 and np.array_equal(s.gram.cpu().numpy(), r["gram"])
    assert s.sum_x.dtype == torch.int64 and np.array_equal(s.sum_x.cpu().numpy(), r["sum_x"])
    assert s.xty.dtype == torch.float64 and _xty_close(s.xty.cpu().numpy(), r)
    assert np.allclose(s.sum_y.cpu().numpy(), r["sum_y"], rtol=1e-12, atol=1e-9) and np.allclose(s.sum_yy.cpu().numpy(), r["sum_yy"], rtol=1e-12)
    # three ranges that tile the rows, the first from L - 1, the last to T - lead; the clamped copy in batches of 300 bins
    rs = [(L - 1, 1000), (1000, 2501), (2501, T - LEAD)]
    parts = wiener.stats(xv, yv, L, LEAD, clip, ranges=rs, max_bytes=C * 300)
    for (a, b), p in zip(rs, parts):
        rr = wo.stats(x, y, L, LEAD, clip, a, b)
        assert p.n == rr["n"] and np.array_equal(p.gram.cpu().numpy(), rr["gram"]) and np.array_equal(p.sum_x.cpu().numpy(), rr["sum_x"])
        assert _xty_close(p.xty.cpu().numpy(), rr)
    tot = parts[0] + parts[1] + parts[2]
    assert tot.n == s.n and torch.equal(tot.gram, s.gram) and torch.equal(tot.sum_x, s.sum_x)
    assert _xty_close(tot.xty.cpu().numpy(), r)
    assert wiener.stats(xv, yv, L, LEAD, clip, ranges=[(10, 10)])[0].n == 0


@pytest.mark.parametrize("clip", [None, 2])
def test_the_filter_fits_predicts_and_scores_as_the_oracle(world, clip):
    x, y, xv, yv = world
    s = wiener.stats(xv, yv, L, LEAD, clip)[0]
    f = wiener.WienerFilter(1e-2).fit(s)
    h = s.to("cpu")
    w, b = wo.fit_from_stats(h.n, h.sum_x.numpy(), h.gram.numpy(), h.xty.numpy(), h.sum_y.numpy(), 1e-2, L, C)
    scale = np.abs(w).max()
    gw, gb = f.weights.cpu().numpy(), f.bias.cpu().numpy()
    print("\nfit: weights differ by %.3g, bias by %.3g of the largest weight" % (np.abs(gw - w).max() / scale, np.abs(gb - b).max() / scale))
    assert f.weights.is_cuda and f.weights.dtype == torch.float64 and gw.shape == (K, L, C) and (gw[:, :, 3] == 0).all()
    assert np.abs(gw - w).max() <= 64 * D_REF_W * scale and np.abs(gb - b).max() <= 64 * D_REF * scale
    # predict: the float64 product with the filter's own weights, within the f32 chain's bound plus the cast of the weights
    pred = f.predict(xv)
    p = pred.cpu().numpy()
    assert p.dtype == np.float32 and p.shape == (K, T - L + 1)
    ref, mag = wo.fir(x, gw, gb, L, clip)
    bound = (_gamma(C + L + 1) + 2.0 ** -24) * mag
    err = np.abs(p.astype(np.float64) - ref)
    print("predict: worst error / bound = %.3g" % (err / bound).max())
    assert (err <= bound).all()
    # score: over the columns whose target exists
    rmse, cc = f.score(xv, yv)
    n = T - L + 1 - LEAD
    ytrue, ypred = y[:, L - 1 + LEAD:].T.astype(np.float64), p[:, :n].T.astype(np.float64)
    assert np.allclose(rmse.cpu().numpy(), wo.rmse(ytrue, ypred), rtol=1e-6, atol=0)
    assert np.allclose(cc.cpu().numpy(), wo.pearson(ytrue, ypred), rtol=1e-6, atol=0)
    # the covariates do depend on the counts: unrelated series of n bins correlate at about 1 / sqrt(n) = 0.016 (without a
    # clip the 255s among the counts, which the covariates see as 4, cost most of the correlation)
    assert (cc.cpu().numpy() > 0.1).all()


def test_cross_validation_from_fold_statistics(world):
    x, y, xv, yv = world
    splits = wiener.folds(xv, 5, lags=L, lead=LEAD)
    n = T - LEAD - (L - 1)
    want = wo.split_index(n, 5)
    every = {r: st for r, st in zip(wiener.fold_ranges(n, 5, L - 1), wiener.stats(xv, yv, L, LEAD, ranges=wiener.fold_ranges(n, 5, L - 1)))}
    for (train, valid, test), (itr, iva, ite) in zip(splits, want):
        assert np.array_equal(np.concatenate([np.arange(a, b) for a, b in train]), itr + L - 1)
        assert np.array_equal(np.arange(*valid), iva + L - 1) and np.array_equal(np.arange(*test), ite + L - 1)
    train = splits[1][0]
    assert len(train) == 3
    tot = sum(every[r] for r in train)
    X, Y = wo.design(x, y, L, LEAD)
    rows = np.concatenate([np.arange(a, b) for a, b in train]) - (L - 1)
    Xt, Yt = X[rows], Y[rows]
    assert tot.n == len(rows) and np.array_equal(tot.gram.cpu().numpy(), Xt.T @ Xt) and np.array_equal(tot.sum_x.cpu().numpy(), Xt.sum(0))
    assert (np.abs(tot.xty.cpu().numpy() - Xt.T.astype(np.float64) @ Yt) <= len(rows) * 2.0 ** -53 * (Xt.T.astype(np.float64) @ np.abs(Yt))).all()
    f = wiener.WienerFilter(1.0).fit(tot)
    w, b = wo.fit_lstsq(Xt, Yt, 1.0)
    scale = np.abs(w).max()
    assert np.abs(f.weights.cpu().numpy().reshape(K, L * C).T - w).max() <= 64 * D_REF_W * scale


# ---- the contract -------------------------------------------------------------------------------------------------------
DELAY_BYTES, DELAY_PASSES = 512 << 20, 24     # as tests/test_gpu_async_contract.py: tens of milliseconds on the device


def _pair(xv, yv, w, b, lags, out_xty, out_fir, scratch):
    rows, k, cols = xv.shape[0], yv.shape[0], yv.shape[1]
    _wiener.xty(xv.data_ptr(), xv.stride(0), rows, cols, lags, 255, yv.data_ptr(), 4 * yv.stride(0), k, out_xty, scratch)
    _wiener.fir(xv.data_ptr(), xv.stride(0), rows, cols, lags, 255, w, b, k, out_fir)


def test_the_pair_is_captured_replayed_and_returns_before_the_stream_drains():
    rows, lags, k, cols = 5, 4, 2, RUN + 3
    x = _counts(rows, cols + lags - 1, 31)
    yi = np.random.RandomState(32).randint(-4096, 4097, (k, cols)).astype(np.int64)
    wi, bi = _int_filter(rows, lags, k, 33)
    xv, yv = _dev(x), _devf((yi / 64.0).astype(np.float32))
    w, b = torch.from_numpy(wi.astype(np.float32)).cuda(), torch.from_numpy(bi.astype(np.float32)).cuda()
    want_xty = np.stack([x.astype(np.int64)[:, lags - 1 - l:lags - 1 - l + cols] @ yi.T for l in range(lags)]) / 64.0
    want_fir = wo.fir(x, wi, bi, lags)[0].astype(np.float32)
    out_xty = torch.zeros((lags, rows, k), dtype=torch.float64, device="cuda")
    out_fir = torch.zeros((k, cols), dtype=torch.float32, device="cuda")
    scratch = torch.zeros((_wiener.xty_scratch_bytes(rows, cols, lags, k),), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _pair(xv, yv, w, b, lags, out_xty, out_fir, scratch)                 # eager, and the warm-up
    side.synchronize()
    assert np.array_equal(out_xty.cpu().numpy(), want_xty) and np.array_equal(out_fir.cpu().numpy(), want_fir)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _pair(xv, yv, w, b, lags, out_xty, out_fir, scratch)
    out_xty.fill_(-1), out_fir.fill_(-1), scratch.fill_(0xFF)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out_xty.cpu().numpy(), want_xty) and np.array_equal(out_fir.cpu().numpy(), want_fir)
    # behind a delay on the stream: both calls return while the delay is still running
    out_xty.fill_(-1), out_fir.fill_(-1)
    delay = torch.zeros(DELAY_BYTES // 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(side):
        for _ in range(DELAY_PASSES):
            delay.add_(1)
        ev.record()
        t0 = time.perf_counter()
        _pair(xv, yv, w, b, lags, out_xty, out_fir, scratch)
        t1 = time.perf_counter()
        pending = not ev.query()
    side.synchronize()
    assert pending, "the delay had completed when the calls returned (host enqueue %.3f ms)" % (1e3 * (t1 - t0))
    assert np.array_equal(out_xty.cpu().numpy(), want_xty) and np.array_equal(out_fir.cpu().numpy(), want_fir)
