"""The Kalman filter decoder on the device (include/muahuff_kalman.h, muahuff.kalman): mhk_project against the float64 sum
in channel order within the derived bound, mhk_scan against the oracle's serial recurrence within 64 x the host's
tiled-against-serial figure, both with identical bits on a second call, next to other data and past their grid caps; then
stats, fit, predict, score and cross_validate against the reference's algorithm restated in tests/kalman_oracle.py.

As measured on an MI355X (every test prints its figure before it asserts): mhk_project at most 0.25 of its bound; mhk_scan
1.8e-16 .. 1.1e-15 of the largest state (bound 64 D_SCAN = 2.9e-14); the fit 1e-15 .. 1.4e-14 of a matrix's largest entry
(bound 64 D_REF_W = 5.8e-13); predict 3.2e-14 .. 1.3e-13 of a state's standard deviation (bound 64 D_KALMAN = 7.7e-13)."""
import numpy as np
import pytest
import torch

from muahuff import _kalman, kalman, wiener
from tests import kalman_oracle as ko
from tests import wiener_oracle as wo
from tests.test_host_kalman import (D_KALMAN, D_SCAN, PROJECT_PAST_CAP, SCAN_CASES, SCAN_PAST_CAP, TILE, scan_inputs, scan_reference)
from tests.test_host_wiener import D_REF_W

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


def _devd(y, lead=3, extra=5, fill=float("nan")):
    """a float64 matrix as a pitched device view (odd pitch, `lead` values in), nan around the rows -> (view, buffer)"""
    rows, cols = y.shape
    pitch = cols + extra
    buf = torch.full((rows * pitch + lead + 64,), fill, dtype=torch.float64, device="cuda")
    view = buf.as_strided((rows, cols), (pitch, 1), lead)
    view.copy_(torch.from_numpy(np.ascontiguousarray(y)).cuda())
    return view, buf


def _counts(rows, cols, seed):
    rng = np.random.RandomState(seed)
    x = np.minimum(rng.poisson(0.8, size=(rows, cols)), 255).astype(np.uint8)
    x[rng.rand(rows, cols) < 0.05] = 255
    x[rng.rand(rows, cols) < 0.05] = 2
    return x


def _bits(t):
    return t.contiguous().view(torch.int64)


# ---- mhk_project ---------------------------------------------------------------------------------------------------------
def _project(xv, m, m0, clip, pitched=True):
    rows, cols = xv.shape
    k = m.shape[0]
    md = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    m0d = None if m0 is None else torch.from_numpy(np.ascontiguousarray(m0)).cuda()
    if pitched:
        v, buf = _devd(np.full((k, cols), np.nan))
    else:
        v = buf = torch.full((k, cols), float("nan"), dtype=torch.float64, device="cuda")
    before = buf.clone()
    _kalman.project(xv.data_ptr(), xv.stride(0) if rows > 1 else 0, rows, cols, clip, md, m0d, v)
    torch.cuda.synchronize()
    # nothing but the k x cols values was written
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask.as_strided(v.shape, v.stride(), v.storage_offset() - buf.storage_offset()).fill_(False)
    assert torch.equal(_bits(buf[mask]), _bits(before[mask]))
    return v


def _project_reference(x, m, m0, clip):
    """the float64 sum in channel order, and the magnitude |m0| + sum |m| min(x, clip) of the bound"""
    k, rows = m.shape
    xq = np.minimum(x, clip).astype(np.float64)
    ref = np.repeat((np.zeros(k) if m0 is None else m0)[:, None], x.shape[1], 1).astype(np.float64)
    mag = np.abs(ref)
    for c in range(rows):
        ref += m[:, c:c + 1] * xq[c:c + 1]
        mag += np.abs(m[:, c:c + 1]) * xq[c:c + 1]
    return ref, mag


# (rows, cols, k, clip, m0, first-byte offset): every value of every axis, every byte alignment of x
PROJECT_SHAPES = [(1, 1, 1, 255, True, 0), (7, 63, 2, 2, True, 1), (65, 1025, 3, 255, False, 2), (300, 1025, 8, 2, True, 3), (7, 1, 8, 255, False, 1),
                  (65, 63, 1, 2, True, 3), (300, 63, 2, 255, True, 2), (1, 1025, 3, 2, False, 1), (8, 5, 2, 255, True, 3), (9, 2 * 1024 + 3, 2, 255, True, 1)]


@pytest.mark.parametrize("i,shape", list(enumerate(PROJECT_SHAPES)), ids=["%dx%d-K%d-q%d-%s-o%d" % (s[0], s[1], s[2], s[3], "m0" if s[4] else "null", s[5]) for s in PROJECT_SHAPES])
def test_project_is_within_the_channel_order_bound(i, shape):
    """|got - ref| <= rows * 2^-53 * (|m0| + sum |m| min(x, clip)): any float64 evaluation of the rows + 1 terms stays inside it"""
    rows, cols, k, clip, with_m0, lead = shape
    rng = np.random.RandomState(200 + i)
    x = _counts(rows, cols, 300 + i)
    m, m0 = rng.randn(k, rows), (rng.randn(k) if with_m0 else None)
    xv = _dev(x, lead=lead)
    got = _project(xv, m, m0, clip)
    ref, mag = _project_reference(x, m, m0, clip)
    err, bound = np.abs(got.cpu().numpy() - ref), rows * 2.0 ** -53 * mag
    print("\nproject %s: worst error / bound = %.3g" % (shape, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    # a second call, and every column inside a longer matrix at another alignment: identical bits
    assert torch.equal(_bits(_project(xv, m, m0, clip)), _bits(got))
    wide = np.concatenate([_counts(rows, 7, 1), x, _counts(rows, 9, 2)], 1)
    inside = _project(_dev(wide, lead=(lead + 2) % 4), m, m0, clip, pitched=False)
    assert torch.equal(_bits(inside[:, 7:7 + cols]), _bits(got))


def test_project_past_the_grid_cap():
    """one channel, one output, a column more than the capped grid has tiles: the stride loop's second trip"""
    cols = PROJECT_PAST_CAP
    x = _counts(1, cols, 5)
    m, m0 = np.array([[1.5]]), np.array([-0.25])
    got = _project(_dev(x, lead=3), m, m0, 255, pitched=False).cpu().numpy()
    assert np.array_equal(got, 1.5 * x.astype(np.float64) - 0.25)          # (exact: one product of small dyadic numbers)


# ---- mhk_scan ----------------------------------------------------------------------------------------------------------------
def _scan(v, ranges, F, B, init, inplace=False, pitched=False, poison=float("nan")):
    """one mhk_scan of NumPy inputs -> out as a device view; the scratch holds 0xFF bytes before the call"""
    k, cols = v.shape
    vd = _devd(v, fill=poison)[0] if pitched else torch.from_numpy(np.ascontiguousarray(v)).cuda()
    if inplace:
        out = vd
    else:
        out = _devd(np.full((k, cols), poison), lead=5, extra=3, fill=poison)[0] if pitched else torch.full((k, cols), poison, dtype=torch.float64, device="cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    scratch = torch.full((max(_kalman.scan_scratch_bytes(cols, k, len(ranges)), 8),), 0xFF, dtype=torch.uint8, device="cuda")
    _kalman.scan(vd, ranges, t(F), t(B), t(init), out, scratch)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("i", range(len(SCAN_CASES)))
def test_scan_is_the_serial_recurrence(i):
    k, cols, ranges, n_gain, radius, inplace, pitched = SCAN_CASES[i]
    v, F, B, init = scan_inputs(i)
    ref = scan_reference(i)
    inside = np.isfinite(ref[0])
    out = _scan(v, ranges, F, B, init, inplace, pitched)
    got = out.cpu().numpy()
    scale = np.abs(ref[:, inside]).max()
    err = np.abs(got[:, inside] - ref[:, inside]).max()
    print("\nscan case %d (k %d, %d ranges, n_gain %d, radius %g): error %.3g of the largest state, bound %.3g" % (i, k, len(ranges), n_gain, radius, err / scale, 64 * D_SCAN))
    assert err <= 64 * D_SCAN * scale
    for r, (a, b) in enumerate(ranges):
        if b > a:
            assert np.array_equal(got[:, a], init[r])                        # the first column is init, bit for bit
    # columns outside every range are as they were: the poison, or in place the projection
    assert np.array_equal(got[:, ~inside], v[:, ~inside]) if inplace else np.isnan(got[:, ~inside]).all()
    # a second call: identical bits
    again = _scan(v, ranges, F, B, init, inplace, pitched)
    assert torch.equal(_bits(again), _bits(out))
    # every range alone (not in place, another pitch): the bits it has among the others
    for r, (a, b) in enumerate(ranges):
        if b - a < 2 or (len(ranges) > 3 and r % 5):
            continue
        alone = _scan(v, [(a, b)], F, B, init[r:r + 1], False, not pitched)
        assert torch.equal(_bits(alone[:, a:b]), _bits(out[:, a:b])), (r, a, b)


def test_scan_past_the_grid_cap():
    """16 ranges whose tiles together are more than the capped grid has threads, each of them under the cap alone: the same
    bits together and alone, and the oracle's recurrence at the start of the first and of the last"""
    ranges, cols = SCAN_PAST_CAP, SCAN_PAST_CAP[-1][1]
    assert sum(-(-(b - a - 1) // TILE) for a, b in ranges) > _kalman.SCAN_MAX_BLOCKS * _kalman.SCAN_THREADS
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((1, cols), dtype=torch.float64, device="cuda", generator=g)
    F, B = ko.contractive(1, 5, 0.98, 9)
    init = np.linspace(-1, 1, 16).reshape(16, 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    Fd, Bd, initd = t(F), t(B), t(init)
    scratch = torch.empty((_kalman.scan_scratch_bytes(cols, 1, 16),), dtype=torch.uint8, device="cuda")
    out = torch.full((1, cols), float("nan"), dtype=torch.float64, device="cuda")
    _kalman.scan(v, ranges, Fd, Bd, initd, out, scratch)
    alone = torch.full((1, cols), float("nan"), dtype=torch.float64, device="cuda")
    for r, ab in enumerate(ranges):
        _kalman.scan(v, [ab], Fd, Bd, initd[r:r + 1], alone, scratch)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(alone))
    covered = torch.zeros((cols,), dtype=torch.bool, device="cuda")
    for a, b in ranges:
        covered[a:b] = True
    assert bool(torch.isfinite(out[0, covered]).all()) and bool(torch.isnan(out[0, ~covered]).all()) and int((~covered).sum()) == sum(r % 3 for r in range(16))
    for r in (0, 15):
        a, n = ranges[r][0], 3 * TILE + 5
        ref = ko.serial_scan(v[:, a:a + n].cpu().numpy(), [(0, n)], F, B, init[r:r + 1])
        assert np.abs(out[:, a:a + n].cpu().numpy() - ref).max() <= 64 * D_SCAN * np.abs(ref).max()
    # the last tiles of the last range, from the device's own state in front of them
    a, b = ranges[15]
    s = b - 2 * TILE
    ref = ko.serial_scan(v[:, s:b].cpu().numpy(), [(0, b - s)], F[-1:], B[-1:], out[:, s].cpu().numpy().reshape(1, 1))
    assert np.abs(out[:, s:b].cpu().numpy() - ref).max() <= 64 * D_SCAN * np.abs(ref).max()


def test_the_pair_is_captured_into_a_graph_and_replayed():
    """mhk_project then mhk_scan on a side stream, eager and as a captured graph (four kernels in a chain): the same bits,
    with the buffers poisoned in between -- neither call synchronises, allocates or copies"""
    rows, cols, k = 9, 3 * TILE + 11, 2
    rng = np.random.RandomState(71)
    xv = _dev(_counts(rows, cols, 72), lead=3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    m, m0 = t(rng.randn(k, rows)), t(rng.randn(k))
    F, B = (t(a) for a in ko.contractive(k, 5, 0.98, 73))
    ranges = [(0, 700), (700, cols)]
    init = t(rng.randn(2, k))
    v = torch.zeros((k, cols), dtype=torch.float64, device="cuda")
    out = torch.zeros((k, cols), dtype=torch.float64, device="cuda")
    scratch = torch.zeros((_kalman.scan_scratch_bytes(cols, k, 2),), dtype=torch.uint8, device="cuda")

    def pair():
        _kalman.project(xv.data_ptr(), xv.stride(0), rows, cols, 3, m, m0, v)
        _kalman.scan(v, ranges, F, B, init, out, scratch)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pair()                                                                 # eager, and the warm-up
    side.synchronize()
    want = out.clone()
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pair()
    v.fill_(float("nan")), out.fill_(float("nan")), scratch.fill_(0xFF)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))


# ---- stats, fit, predict, score, cross_validate ----------------------------------------------------------------------------
WORLDS = {(7, 4000): 1, (33, 3000): 1}


@pytest.fixture(scope="module")
def worlds():
    out = {}
    for (C, T), seed in WORLDS.items():
        x, y = ko.data(C, 2, T, seed)
        yd = torch.from_numpy(y).cuda()
        out[(C, T)] = (x, y, _dev(x, lead=1), yd)
    return out


@pytest.mark.parametrize("C,T,lead,clip", [(7, 4000, 0, 4), (33, 3000, 2, None)])
def test_stats_and_fit_from_the_device_are_the_reference_fit(worlds, C, T, lead, clip):
    x, y, xv, yv = worlds[(C, T)]
    s = kalman.stats(xv, yv, lead, clip)[0]
    r = ko.stats(x, y, lead, clip)
    assert s.w.n == r["n"] == T - lead and s.n_pairs == r["n_pairs"] == T - lead - 1 and (s.w.lags, s.w.lead, s.w.clip) == (1, lead, clip or 255)
    assert np.array_equal(s.w.gram.cpu().numpy(), r["gram"]) and np.array_equal(s.w.sum_x.cpu().numpy(), r["sum_x"])
    for name in ("sum_a", "sum_b", "aa", "bb", "ab", "sum_d", "dd", "ad"):
        assert np.allclose(getattr(s, name).cpu().numpy(), r[name], rtol=1e-12, atol=1e-9), name
    # three ranges add to the whole but for the two junction pairs
    cut = [(0, 1000), (1000, 2501), (2501, T - lead)]
    parts = kalman.stats(xv, yv, lead, clip, cut)
    tot = sum(parts)
    assert tot.w.n == s.w.n and tot.n_pairs == s.n_pairs - 2 and torch.equal(tot.w.gram, s.w.gram)
    assert [p.n_pairs for p in parts] == [b - a - 1 for a, b in cut]
    p = ko.prepare(x, y, lead, clip)
    for alpha in (0.0, 1e-2):
        f = kalman.KalmanFilter(alpha).fit(s)
        model = ko.reference_fit(p["Z"], p["Y"], alpha)
        for name, ref in zip("AWHQ", model):
            got = getattr(f, name)
            d = np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max()
            print("\n%d x %d alpha %g: %s differs by %.2e of its largest entry" % (C, T, alpha, name, d))
            assert got.is_cuda and got.dtype == torch.float64 and d <= 64 * D_REF_W
        assert (f.lead, f.clip, f.channels) == (lead, clip or 255, C) and (f.m[:, min(3, C - 1)] == 0).all()


# (C, T, lead, clip, alpha, three ranges, y0 given)
PREDICT_CASES = [(7, 4000, 0, None, 0.0, False, True), (7, 4000, 2, 3, 1e-2, True, False), (33, 3000, 2, None, 0.0, True, True),
                 (33, 3000, 0, 3, 1e-2, False, False), (7, 4000, 0, 3, 0.0, True, True), (33, 3000, 2, None, 1e-2, False, False)]


@pytest.mark.parametrize("C,T,lead,clip,alpha,three,given", PREDICT_CASES)
def test_predict_is_the_reference_loop(worlds, C, T, lead, clip, alpha, three, given):
    """fit and predict on the device against reference_fit and reference_predict on the explicit z-scored data, every range
    restarted, within 64 x D_KALMAN of the state's standard deviation"""
    x, y, xv, yv = worlds[(C, T)]
    n = T - lead
    f = kalman.KalmanFilter(alpha).fit(kalman.stats(xv, yv, lead, clip))
    p = ko.prepare(x, y, lead, clip)
    model = ko.reference_fit(p["Z"], p["Y"], alpha)
    # (one range: the default, the whole recording, where every bin has its target; otherwise the bins that have one)
    ranges = [(5, 700), (700, 700 + 2 * TILE + 9), (2000, n)] if three else None if lead == 0 else [(0, n)]
    rs = ranges or [(0, T)]
    y0 = np.stack([p["Y"][a] + p["ybar"] for a, _b in rs]) if given else None
    pred = f.predict(xv, None if y0 is None else torch.from_numpy(y0).cuda(), ranges)
    assert pred.dtype == torch.float64 and tuple(pred.shape) == (2, T)
    got = pred.cpu().numpy()
    std = p["Y"][:n].std(0)
    worst = 0.0
    inside = np.zeros(T, bool)
    for r, (a, b) in enumerate(rs):
        inside[a:b] = True
        ref = ko.reference_predict(model, p["Z"][a:b], (y0[r] - p["ybar"]) if given else np.zeros(2))
        worst = max(worst, (np.abs(got[:, a:b].T - p["ybar"] - ref).max(0) / std).max())
    print("\npredict %s: %.3g of the state's standard deviation, bound %.3g" % ((C, T, lead, clip, alpha, three, given), worst, 64 * D_KALMAN))
    assert worst <= 64 * D_KALMAN
    assert np.isnan(got[:, ~inside]).all()
    assert torch.equal(_bits(f.predict(xv, None if y0 is None else torch.from_numpy(y0).cuda(), ranges)[:, inside]), _bits(pred[:, inside]))


def _scores(x, y, lead, clip, alpha, train, held):
    """the reference's loop with the oracle: z-score and fit on the concatenated training folds (without the junction
    pairs), predict every held-out fold from its true first state, score all its columns -> [(rmse, cc)] per fold"""
    parts = [wo.design(x, y, 1, lead, clip, a, b) for a, b in train]
    X, Y = np.concatenate([p[0] for p in parts]).astype(np.float64), np.concatenate([p[1] for p in parts])
    mean, std, ybar = X.mean(0), X.std(0), Y.mean(0)
    keep = np.flatnonzero(std > 0)
    model = ko.reference_fit((X[:, keep] - mean[keep]) / std[keep], Y - ybar, alpha, [len(p[0]) for p in parts])
    out = []
    for a, b in held:
        h = ko.prepare(x, y, lead, clip, a, b, dict(mean=mean, std=std, keep=keep, ybar=ybar))
        pred = ko.reference_predict(model, h["Z"], h["Y"][0])
        out.append((wo.rmse(h["Y"], pred), wo.pearson(h["Y"], pred)))
    return out


def test_score_and_cross_validate_are_the_reference_loop(worlds):
    C, T, lead, clip, folds = 7, 4000, 2, 3, 5
    x, y, xv, yv = worlds[(C, T)]
    fr = wiener.fold_ranges(T - lead, folds)
    assert [(tr, v, t) for tr, v, t in wiener.folds(xv, folds, 1, lead)][0][1] == fr[0]
    alphas = (0.0, 1e-2)
    res = kalman.cross_validate(xv, yv, lead, clip, alphas, folds)
    std = y.astype(np.float64).std(1)
    for j, alpha in enumerate(alphas):
        for i in (0, folds - 1):                                                # the first split and the one whose test fold wraps around
            v, t = i, (i + 1) % folds
            (rv, cv), (rt, ct) = _scores(x, y, lead, clip, alpha, [fr[k] for k in range(folds) if k not in (v, t)], [fr[v], fr[t]])
            # With every prediction within e = 64 D_KALMAN of a state's standard deviation s of the reference's, an rmse
            # moves by at most e s (the training folds' s may differ from the recording's: a factor of 2 for that) and r,
            # whose numerator and denominator each move by about e relative to themselves, by 4 e.
            for name, ref in (("rmse_valid", rv), ("rmse_test", rt), ("cc_valid", cv), ("cc_test", ct)):
                got = res[name][j, i].cpu().numpy()
                d = np.abs(got - ref) / (2 * std if name.startswith("rmse") else 4.0)
                print("\nalpha %g split %d %s: %s against %s, %.3g" % (alpha, i, name, got, ref, d.max()))
                assert (d <= 64 * D_KALMAN).all()
    assert all(tuple(res[k].shape) == (2, folds, 2) and res[k].dtype == torch.float64 for k in res)
    assert float(res["cc_test"].min()) > 0.5
    # score on one range is cross_validate's number for it
    tot = sum(kalman.stats(xv, yv, lead, clip, [fr[2], fr[3], fr[4]]))
    rmse, cc = kalman.KalmanFilter(0.0).fit(tot).score(xv, yv, [fr[0], fr[1]])
    assert torch.equal(rmse[0], res["rmse_valid"][0, 0]) and torch.equal(cc[1], res["cc_test"][0, 0])
