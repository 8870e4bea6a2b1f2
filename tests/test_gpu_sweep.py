"""The dynamic-range sweep on the GPU (include/muahuff_sweep.h, csrc/mh_sweep.hpp, wiener.iter_stats_clips,
cascade.sweep_clips).  mhq_gram_clips against NumPy's int64 products -- equal, not close -- over the tile, lag, clip and
range edges, every byte alignment of x, the int32 bound of a full run, the stride loop past the grid cap and a row stride
beyond 2^32; mhq_xty_clips against mhw_xty on every (range, clip) -- the same bits -- and within mhw_xty's own bound of
the oracle; wiener.stats_clips against wiener.stats(clip=q) and cascade.sweep_clips against the loop of
cross_validate(clip=q), field by field under torch.equal; and the contract: graph capture and replay, and return before
the stream drains."""
import time

import numpy as np
import pytest
import torch

from muahuff import _sweep, _wiener, cascade, wiener
from tests import sweep_oracle as so
from tests.test_gpu_box import ARENA_BYTES, arena  # noqa: F401  (the fixture)
from tests.test_gpu_wiener import DELAY_BYTES, DELAY_PASSES, _dev, _devf, _xty_close
from tests.test_host_cascade import nonlinear_data
from tests.test_host_sweep import GRAM_RUN, MAX_BLOCKS, XTY_MAX_BLOCKS, XTY_RUN, layout
from tests.test_host_wiener import data

pytestmark = pytest.mark.gpu


def _edge_counts(rows, cols, clips, seed):
    """counts that hold 0, 255 and the values on either side of every clip, at random places"""
    rng = np.random.RandomState(seed)
    marks = sorted({0, 255} | {min(max(q + s, 0), 255) for q in clips for s in (-1, 0, 1)})
    x = np.minimum(rng.poisson(1.5, size=(rows, cols)), 255).astype(np.uint8)
    pick = rng.rand(rows, cols) < 0.5
    x[pick] = np.asarray(marks, np.uint8)[rng.randint(0, len(marks), int(pick.sum()))]
    if x.size >= 4 * len(marks):
        x.flat[rng.choice(x.size, len(marks), replace=False)] = marks         # every one of them at least once
    return x


def _gram(xv, ranges, clips, lags, gram=None, sums=None):
    """one mhq_gram_clips on the view xv [rows, cols] onto zeroed buffers -> (gram [R, n, lags, rows, rows], sums [R, n, rows])"""
    rows, cols = xv.shape
    if gram is None:
        gram = torch.zeros((len(ranges), len(clips), lags, rows, rows), dtype=torch.int64, device="cuda")
        sums = torch.zeros((len(ranges), len(clips), rows), dtype=torch.int64, device="cuda")
    _sweep.gram_clips(xv.data_ptr(), xv.stride(0) if rows > 1 else 0, rows, cols, ranges, clips, lags, gram, sums)
    return gram, sums


def _same(got, want):
    return all(g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


# ---- mhq_gram_clips -------------------------------------------------------------------------------------------------------
CLIPS = [(1,), (1, 2, 39, 255), (127, 128), tuple(range(2, 66))]


@pytest.mark.parametrize("lags", [1, 2, 15, 32])
@pytest.mark.parametrize("rows", [1, 17, 128, 129])
def test_gram_clips_equals_numpy_int64(rows, lags):
    """one range of 1, 63 and 64 + 15 columns -- and of a full run and 65 with few rows --, and five ranges: adjacent ones, an
    empty one, the first starting exactly at lags - 1; every clip list with the single ranges, the four-clip list with the
    five; both clamp forms (clips up to 127 and above) in one launch wherever the list holds both"""
    L1 = lags - 1
    five = [(L1, L1 + 70), (L1 + 70, L1 + 70), (L1 + 70, L1 + 200), (L1 + 200, L1 + 263), (L1 + 333, L1 + 600)]
    cases = [([(L1 + off, L1 + off + n)], c) for c in CLIPS for off, n in ((0, 1), (3, 63), (0, 64 + 15))]
    cases.append((five, CLIPS[1]))
    if rows <= 17:
        cases += [([(L1 + 5, L1 + 5 + GRAM_RUN + 65)], (39, 255))]
    for i, (ranges, clips) in enumerate(cases):
        cols = ranges[-1][1] + (i % 3)
        x = _edge_counts(rows, cols, clips, 1000 * rows + 10 * lags + i)
        xv = _dev(x, lead=(rows + lags + i) % 16, extra=36 + i % 2)
        got = _gram(xv, ranges, clips, lags)
        want = so.gram_clips_fast(x, ranges, clips, lags)
        assert _same(got, want), (ranges, clips)
        if i % 5 == 0:                                              # added to what is there: twice the result, and identical bits
            again = _gram(xv, ranges, clips, lags)
            assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
            _gram(xv, ranges, clips, lags, *got)
            assert _same(got, (2 * want[0], 2 * want[1]))


def test_gram_clips_with_the_first_byte_of_x_at_every_offset_and_an_odd_row_stride():
    rows, lags, clips = 17, 15, (3, 200)
    ranges = [(14, 90), (100, 100 + 64 + 15 + 2)]
    x = _edge_counts(rows, 190, clips, 5)
    want = so.gram_clips_fast(x, ranges, clips, lags)
    for off in range(16):
        xv = _dev(x, lead=off, extra=37)
        assert xv.stride(0) % 2 == 1 and xv.data_ptr() % 16 == off
        assert _same(_gram(xv, ranges, clips, lags), want), off


def test_gram_clips_on_a_full_run_of_255_is_at_the_int32_bound():
    """all counts 255, one run of 65536 columns: clip 255 (the XOR form: 128 * 128 * 65536 = 2^30 per accumulator, the
    fix-up brings 255^2 n) and clip 127 (the direct form: 127^2 * 65536 just under 2^30)"""
    rows, lags, n = 17, 2, GRAM_RUN
    xv = _dev(np.full((rows, n + 1), 255, np.uint8), lead=3, extra=5)
    gram, sums = _gram(xv, [(1, n + 1)], (127, 255), lags)
    for i, q in enumerate((127, 255)):
        assert bool((gram[0, i] == q * q * n).all()) and bool((sums[0, i] == q * n).all())
    assert 255 * 255 * n > 2 ** 31 > 128 * 128 * n                # the sum is past int32, the accumulator of the XOR form is not


def test_gram_clips_past_the_grid_cap():
    """5 ranges of 70 000 columns (two runs each) x 38 clips x 15 lag differences x 1 tile = 5 700 items on 2 048 workgroups:
    the stride loop's second and third trips"""
    rows, lags, clips = 5, 15, tuple(range(2, 40))
    ranges = [(14 + 70000 * i, 14 + 70000 * (i + 1)) for i in range(5)]
    lay = layout(rows, lags, 1, ranges, clips)
    assert lay[1] == 5700 > 2 * lay[2] and lay[2] == MAX_BLOCKS
    x = _edge_counts(rows, ranges[-1][1], (2, 20, 39), 9)
    assert _same(_gram(_dev(x, lead=7, extra=1), ranges, clips, lags), so.gram_clips_fast(x, ranges, clips, lags))


def test_gram_clips_with_a_row_stride_beyond_2_to_the_32(arena):  # noqa: F811
    """two rows 2^32 + 4099 bytes apart; where a 32-bit row offset would look for the second row lies a decoy"""
    cols, lags, clips = 300, 3, (2, 39)
    stride, first = (1 << 32) + 4099, 13
    x = _edge_counts(2, cols, clips, 61)
    decoy = 255 - x[1]
    assert first + stride + cols <= ARENA_BYTES and first + cols < first + 4099
    for off, row in ((first, x[0]), (first + 4099, decoy), (first + stride, x[1])):
        arena[off - 8:off + cols + 8] = 255
        arena[off:off + cols] = torch.from_numpy(row).cuda()
    ranges = [(2, 150), (150, cols)]
    gram = torch.zeros((2, 2, lags, 2, 2), dtype=torch.int64, device="cuda")
    sums = torch.zeros((2, 2, 2), dtype=torch.int64, device="cuda")
    _sweep.gram_clips(arena.data_ptr() + first, stride, 2, cols, ranges, clips, lags, gram, sums)
    want = so.gram_clips_fast(x, ranges, clips, lags)
    assert _same((gram, sums), want)
    assert not np.array_equal(want[1], so.gram_clips_fast(np.stack([x[0], decoy]), ranges, clips, lags)[1])


# ---- mhq_xty_clips ----------------------------------------------------------------------------------------------------------
def _xty_clips(xv, yv, ranges, clips, lags, lead):
    rows, cols, k = xv.shape[0], xv.shape[1], yv.shape[0]
    out = torch.full((len(ranges), len(clips), lags, rows, k), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.full((_sweep.xty_clips_scratch_bytes(rows, cols, lags, k, len(ranges), len(clips)),), 0xFF, dtype=torch.uint8, device="cuda")
    _sweep.xty_clips(xv.data_ptr(), xv.stride(0) if rows > 1 else 0, rows, cols, ranges, clips, lags, lead, yv.data_ptr(),
                     4 * yv.stride(0) if k > 1 else 0, k, out, scratch)
    return out


@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("k", [1, 2, 8])
def test_xty_clips_is_mhw_xty_bit_for_bit_on_every_range_and_clip(k, lead):
    """a range of two runs and a bit, an empty one, a short one and one that ends with the last column that has a target;
    9 lags are one past a lag block.  Every (range, clip) slice against the mhw_xty call wiener._range_stats makes, and
    against the oracle within the bound tests/test_gpu_wiener.py has for mhw_xty."""
    rows, lags, clips = 5, 9, (1, 3, 127, 255)
    cols = 2 * XTY_RUN + 700
    ranges = [(lags - 1, lags - 1 + 2 * XTY_RUN + 100), (2 * XTY_RUN + 150, 2 * XTY_RUN + 150), (2 * XTY_RUN + 150, 2 * XTY_RUN + 213),
              (2 * XTY_RUN + 300, cols - lead)]
    x = _edge_counts(rows, cols, clips, 40 + k + lead)
    y = (np.random.RandomState(50 + k).randn(k, cols) * 3).astype(np.float32)
    xv, yv = _dev(x, lead=5), _devf(y, lead=1 + lead)
    got = _xty_clips(xv, yv, ranges, clips, lags, lead)
    again = _xty_clips(xv, yv, ranges, clips, lags, lead)
    assert torch.equal(got, again) and not bool(torch.isnan(got).any())
    ref, mag, n = so.xty_clips(x, y, ranges, clips, lags, lead)
    for r, (a, b) in enumerate(ranges):
        for i, q in enumerate(clips):
            if a == b:
                assert bool((got[r, i] == 0).all())
                continue
            one = torch.full((lags, rows, k), float("nan"), dtype=torch.float64, device="cuda")
            scratch = torch.empty((_wiener.xty_scratch_bytes(rows, b - a, lags, k),), dtype=torch.uint8, device="cuda")
            _wiener.xty(xv.data_ptr() + a - (lags - 1), xv.stride(0), rows, b - a, lags, q, yv.data_ptr() + 4 * (a + lead),
                        4 * yv.stride(0) if k > 1 else 4 * (b - a), k, one, scratch)
            assert torch.equal(got[r, i], one), (r, q)
            assert _xty_close(got[r, i].cpu().numpy(), dict(xty=ref[r, i], n=int(n[r]), abs_xty=mag[r, i])), (r, q)


def test_xty_clips_past_both_grid_caps():
    """70 channels x 64 clips x 2 runs are more (run, clip, channel) items than the first kernel's capped grid has
    workgroups, and 2 x 64 x 70 x 32 x 8 elements more than the second's has threads: the second trip of both stride
    loops.  Dyadic covariates: the sums are exact, equal to the oracle's"""
    rows, lags, k, lead, clips = 70, 32, 8, 1, tuple(range(2, 66))
    ranges = [(31, 94), (94, 150)]
    lay = layout(rows, lags, k, ranges, clips)
    assert lay[4] > lay[5] == XTY_MAX_BLOCKS and lay[6] > 256 * lay[7] and lay[7] == XTY_MAX_BLOCKS
    x = _edge_counts(rows, 151, (2, 30, 65), 77)
    yi = np.random.RandomState(78).randint(-4096, 4097, (k, 151)).astype(np.int64)
    got = _xty_clips(_dev(x, lead=2, extra=3), _devf((yi / 64.0).astype(np.float32)), ranges, clips, lags, lead)
    assert np.array_equal(got.cpu().numpy(), so.xty_clips(x, yi.astype(np.float64), ranges, clips, lags, lead)[0] / 64.0)


# ---- wiener.stats_clips, cascade.sweep_clips ----------------------------------------------------------------------------------
C, L, K, T, LEAD = 7, 5, 2, 4000, 3
FIELDS = ("gram", "sum_x", "xty", "sum_y", "sum_yy")


def test_stats_clips_equal_stats_clip_by_clip():
    """clips 2..39, 7 channels x 4000 bins, the five folds; max_bytes holds the count products of 13 clips: three groups"""
    x, y = data(C, L, K, T)
    xv, yv = _dev(x, lead=1), _devf(y, lead=2)
    fr = wiener.fold_ranges(T - LEAD - (L - 1), 5, L - 1)
    clips = list(range(2, 40))
    max_bytes = 13 * 5 * L * C * C * 8
    assert [len(g) for g in wiener._clip_groups(clips, 5, L, C, max_bytes)] == [13, 13, 12]
    got = wiener.stats_clips(xv, yv, L, LEAD, clips, ranges=fr, max_bytes=max_bytes)
    assert [q for q, _s in got] == clips
    for q, parts in got:
        want = wiener.stats(xv, yv, L, LEAD, clip=q, ranges=fr)
        assert len(parts) == len(want) == 5
        for s, w in zip(parts, want):
            assert (s.n, s.lags, s.lead, s.clip, s.channels, s.window) == (w.n, w.lags, w.lead, w.clip, w.channels, w.window) == (w.n, L, LEAD, q, C, 1)
            for f in FIELDS:
                a, b = getattr(s, f), getattr(w, f)
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (q, f)
    # the default route: one group, all design rows as the one range, an unclipped entry
    one = wiener.stats_clips(xv, yv, L, LEAD, (2, 255))
    for (q, parts), clip in zip(one, (2, None)):
        w = wiener.stats(xv, yv, L, LEAD, clip)[0]
        assert len(parts) == 1 and parts[0].n == w.n and all(torch.equal(getattr(parts[0], f), getattr(w, f)) for f in FIELDS)
    with pytest.raises(ValueError, match="ascending"):
        wiener.iter_stats_clips(xv, yv, L, LEAD, (2, 3), ranges=[(100, 200), (150, 300)])


@pytest.mark.parametrize("window,clips", [(1, (2, 3, 39)), (4, (2, 39))])
def test_sweep_clips_equals_the_loop_of_cross_validate(window, clips):
    """all four arrays of every (alpha, degree) under torch.equal; window 4 takes the per-clip route inside sweep_clips"""
    x, y = nonlinear_data()
    xv, yv = _dev(x, lead=1), _devf(y, lead=2)
    alphas, degrees = (1e-4, 1e-2), (None, 2, 4)
    got = cascade.sweep_clips(xv, yv, L, LEAD, clips, alphas, degrees, 5, window)
    assert list(got) == list(clips)
    for q in clips:
        want = cascade.cross_validate(xv, yv, L, LEAD, q, alphas, degrees, 5, window)
        assert set(got[q]) == set(want) == {(a, d) for a in alphas for d in degrees}
        for key, arrays in want.items():
            for name, w in arrays.items():
                g = got[q][key][name]
                assert g.dtype == torch.float64 and tuple(g.shape) == (5, K) and torch.equal(g, w), (q, key, name)


# ---- the contract -------------------------------------------------------------------------------------------------------
def _pair(xv, yv, ranges, clips, lags, lead, gram, sums, out, scratch):
    rows, cols, k = xv.shape[0], xv.shape[1], yv.shape[0]
    _sweep.gram_clips(xv.data_ptr(), xv.stride(0), rows, cols, ranges, clips, lags, gram, sums)
    _sweep.xty_clips(xv.data_ptr(), xv.stride(0), rows, cols, ranges, clips, lags, lead, yv.data_ptr(), 4 * yv.stride(0), k, out, scratch)


def test_the_pair_is_captured_replayed_and_returns_before_the_stream_drains():
    rows, lags, lead, k, clips = 5, 4, 2, 2, (2, 200)
    cols = XTY_RUN + 300
    ranges = [(3, 3 + XTY_RUN + 3), (XTY_RUN + 50, cols - lead)]
    x = _edge_counts(rows, cols, clips, 31)
    yi = np.random.RandomState(32).randint(-4096, 4097, (k, cols)).astype(np.int64)          # y = yi / 64: the sums are exact
    xv, yv = _dev(x), _devf((yi / 64.0).astype(np.float32))
    want_gram = so.gram_clips_fast(x, ranges, clips, lags)
    want_xty = so.xty_clips(x, yi.astype(np.float64), ranges, clips, lags, lead)[0] / 64.0
    gram = torch.zeros((2, 2, lags, rows, rows), dtype=torch.int64, device="cuda")
    sums = torch.zeros((2, 2, rows), dtype=torch.int64, device="cuda")
    out = torch.zeros((2, 2, lags, rows, k), dtype=torch.float64, device="cuda")
    scratch = torch.zeros((_sweep.xty_clips_scratch_bytes(rows, cols, lags, k, 2, 2),), dtype=torch.uint8, device="cuda")
    args = (xv, yv, ranges, clips, lags, lead, gram, sums, out, scratch)
    good = lambda: _same((gram, sums), want_gram) and np.array_equal(out.cpu().numpy(), want_xty)   # noqa: E731
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _pair(*args)                                                          # eager, and the warm-up
    side.synchronize()
    assert good()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _pair(*args)
    for _ in range(2):                                                        # replayed twice, each time onto zeroed buffers
        gram.zero_(), sums.zero_(), out.fill_(-1), scratch.fill_(0xFF)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert good()
    # behind a delay on the stream: both calls return while the delay is still running
    gram.zero_(), sums.zero_(), out.fill_(-1)
    delay = torch.zeros(DELAY_BYTES // 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(side):
        for _ in range(DELAY_PASSES):
            delay.add_(1)
        ev.record()
        t0 = time.perf_counter()
        _pair(*args)
        t1 = time.perf_counter()
        pending = not ev.query()
    side.synchronize()
    assert pending, "the delay had completed when the calls returned (host enqueue %.3f ms)" % (1e3 * (t1 - t0))
    assert good()
