"""The decoders' file routes on the GPU: lagged Gram matrices, Wiener statistics (one clip and a list), predictions, the
cascade's and the Kalman filter's cross-validation from a gram.BinSource over an archive or a container, walked in
batches that carry a halo -- against the in-memory function on what read() returns for the same bins.  Every case runs
at a budget that gives one batch, one that gives several batches longer than the halo and one whose batches are SHORTER
than the halo (the halo then moves over itself), and asserts the number of batches, so a silent single batch cannot
pass.  Bounds: integers are equal; a float64 sum taken batch by batch and the same sum taken at once are each within
gamma_n = n 2^-53 of the exact sum, so they differ by at most n 2^-52 times the sum of the terms' magnitudes."""
import numpy as np
import pytest
import torch

import muahuff
from muahuff import archive, cascade, gram, kalman, wiener
from muahuff import container_io as cio
from tests import cascade_oracle as co
from tests import kalman_oracle as ko
from tests import wiener_oracle as wo
from tests.test_gpu_cascade import CV_REF
from tests.test_gpu_kalman import _scores
from tests.test_gpu_wiener import _gamma
from tests.test_host_cascade import nonlinear_data
from tests.test_host_kalman import D_KALMAN
from tests.test_host_wiener import data

pytestmark = pytest.mark.gpu

C, S, K = 12, 3, 2
TB = [2 * muahuff.CHUNK + 700, 20000, 3 * muahuff.CHUNK + 5]       # three blocks of unequal length, a few chunks each
T = sum(TB)
B1, B2 = TB[0], TB[0] + TB[1]
RANGE = (B1 - 5000, B2 + 7003)         # from inside block 1, across block 2, into block 3
SUBSET = [7, 0, 11, 7]
TINY = 300                             # bins of the range the one-bin batches walk: it straddles the first block boundary
# (lags, lead, clip, window); the last is the two-plane route (50 * 39 > 255) with a warm-up of 49 rows
SETTINGS = [(5, 0, None, 1), (15, 3, 3, 1), (5, 3, 3, 4), (5, 0, 39, 50)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("file_decoders")
    rng = np.random.RandomState(33)
    rec = np.minimum(rng.poisson(0.3 + 0.08 * np.arange(C), size=(T, C)), 255).astype(np.uint8)
    rec[rng.rand(T, C) < 0.001] = 255
    out = {}
    for name, kw in (("plain", {}), ("exact", dict(exact=True))):
        fn = str(d / (name + ".mua"))
        with archive.create(fn, C, S=S, hist_bits=6, seg_chunks=2, **kw) as w:
            t = 0
            for Tb in TB:
                w.append(rec[t:t + Tb])
                t += Tb
        out[name] = fn
    c = muahuff.compress([np.ascontiguousarray(rec[:, i]) for i in range(C)], S=S, hist_bits=6)
    out["container"] = str(d / "c.mh")
    cio.save(out["container"], c)
    out["compressed"] = c
    return out


class _File:
    """one way to the same two things for an archive and a container: read() and bins()"""

    def __init__(self, files, kind):
        self.kind, self.files = kind, files
        self.rd = archive.open(files[kind]) if kind != "container" else None

    def read(self, start, stop, channels=None, bin=None):  # noqa: A002
        if self.rd is not None:
            return self.rd.read(start, stop, channels, bin=bin)
        c = self.files["compressed"]
        return cio.decompress_range(c, start, stop, channels) if bin is None else cio.decompress_binned(c, bin, start, stop, channels)

    def bins(self, start, stop, channels=None, bin=None, max_bytes=None):  # noqa: A002
        if self.rd is not None:
            return self.rd.bins(start, stop, channels, bin=bin, max_bytes=max_bytes)
        return cio.bins(self.files["container"], start, stop, channels, bin=bin, max_bytes=max_bytes)

    def close(self):
        if self.rd is not None:
            self.rd.close()


def _span(bin_, tiny=False):
    """-> (start, stop, n): RANGE on the bin grid, or TINY bins of it around the first block boundary"""
    r = bin_ or 1
    a, b = RANGE if not tiny else (B1 - (TINY // 2) * r, B1 + (TINY // 2) * r + r // 2)
    a -= a % r
    return a, b, (b - a) // r


def _resident(f, bin_, channels, tiny=False):
    a, b, n = _span(bin_, tiny)
    x = f.read(a, a + n * (bin_ or 1), channels, bin_)[:, :n]
    assert x.dtype == torch.uint8 and tuple(x.shape) == (C if channels is None else len(channels), n)
    return x


def _covariates(x, seed=5):
    """K smooth functions of a few channels, two bins late, plus noise: float32 on the bin grid"""
    rng = np.random.RandomState(seed)
    h = np.minimum(x.cpu().numpy(), 4).astype(np.float64)
    mix = np.zeros((K, h.shape[0]))
    mix[:, :3] = rng.randn(K, 3)
    y = mix @ np.roll(h, 2, axis=1) + 0.5 * rng.randn(K, h.shape[1])
    return torch.from_numpy(y.astype(np.float32)).cuda()


def _budgets(rows, n, halo):
    """-> [(max_bytes, check of the plan)]: one batch; at least three batches longer than the halo"""
    many = rows * (n // 3 - 11)
    plan = gram.halo_plan(n, rows, halo, many)
    assert sum(nb > halo for _b0, nb in plan) >= 3
    assert len(gram.halo_plan(n, rows, halo, 1 << 30)) == 1
    return [None, many]


def _tiny_budget(rows, n, halo):
    """batches shorter than the halo: eight bins in the scratch, fewer under a halo that short"""
    cap = min(8, halo - 1)
    plan = gram.halo_plan(n, rows, halo, rows * cap)
    assert cap >= 1 and len(plan) > n - 9 and all(nb < halo for _b0, nb in plan)
    return rows * cap


# ---- the walker alone ------------------------------------------------------------------------------------------------------
def test_the_walker_reproduces_a_resident_matrix_at_every_budget():
    rows, n, halo = 12, 1000, 14
    x = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (rows, n)).astype(np.uint8)).cuda()
    budgets = _budgets(rows, n, halo) + [_tiny_budget(rows, n, halo), rows * (halo + 3), rows * (2 * halo - 1)]
    for mb in budgets:
        src = gram.BinSource.of(x, mb)
        assert (src.rows, src.n) == (rows, n)
        plan = gram.halo_plan(n, rows, halo, src.max_bytes)
        seen = []
        for b0, nb, h, view in gram.walk(src, halo):
            assert h == min(halo, b0) and tuple(view.shape) == (rows, h + nb) and view.numel() <= max(src.max_bytes, rows * (h + 1))
            assert torch.equal(view, x[:, b0 - h:b0 + nb]), (mb, b0, nb, h)
            seen.append((b0, nb))
        assert seen == plan
    # a part of the bins: the halo starts at the first bin read
    src = gram.BinSource.of(x, rows * 8)
    got = list((b0, nb, h) for b0, nb, h, view in gram.walk(src, halo, 100, 140) if torch.equal(view, x[:, b0 - h:b0 + nb]))
    assert got[0] == (100, 8, 0) and got[1] == (108, 1, 8) and got[-1][0] + got[-1][1] == 140 and got[-1][2] == halo
    assert list(gram.walk(src, halo, 7, 7)) == []
    with pytest.raises(ValueError):
        list(gram.walk(src, halo, 0, n + 1))


# ---- Gram matrices ---------------------------------------------------------------------------------------------------------
def _same_gram(got, want):
    assert isinstance(got, gram.Gram) and got.n == want.n and got.symmetric == want.symmetric
    for name in ("gram", "sum_a", "sum_b"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == torch.int64 and a.shape == b.shape and torch.equal(a, b), name


@pytest.mark.parametrize("kind,bin_,channels", [("plain", None, None), ("exact", 5, SUBSET), ("container", None, SUBSET),
                                                ("container", 5, None), ("exact", None, None)])
def test_lagged_gram_from_a_file_equals_gram_of_what_read_returns(files, kind, bin_, channels):
    f = _File(files, kind)
    try:
        for tiny in (False, True):
            a, b, n = _span(bin_, tiny)
            x = _resident(f, bin_, channels, tiny)
            rows = int(x.shape[0])
            budgets = [_tiny_budget(rows, n, 14)] if tiny else _budgets(rows, n, 14)
            for lag in (0, 3, [0, 1, 14]):
                want = gram.gram(x, lag=lag)
                for mb in budgets:
                    if kind == "container":
                        got = cio.decompress_gram(files["container"], a, b, channels, bin=bin_, max_bytes=mb, lag=lag)
                    else:
                        got = f.rd.read_gram(a, b, channels, bin=bin_, max_bytes=mb, lag=lag)
                    _same_gram(got, want)
    finally:
        f.close()


# ---- Wiener statistics -----------------------------------------------------------------------------------------------------
def _fmax(clip, window):
    return window * min(clip or 255, 255)


def _same_stats(got, want, y, rs, lead, fmax):
    yabs = y.double().abs()
    for s, r, (a, b) in zip(got, want, rs):
        assert (s.n, s.lags, s.lead, s.clip, s.channels, s.window) == (r.n, r.lags, r.lead, r.clip, r.channels, r.window) and s.n == b - a
        assert s.gram.dtype == torch.int64 and torch.equal(s.gram, r.gram) and torch.equal(s.sum_x, r.sum_x)
        ya = yabs[:, a + lead:b + lead]
        eps = max(s.n, 1) * 2.0 ** -52
        assert bool(((s.xty - r.xty).abs() <= eps * fmax * ya.sum(1).unsqueeze(0)).all())
        assert bool(((s.sum_y - r.sum_y).abs() <= eps * ya.sum(1)).all())
        assert bool(((s.sum_yy - r.sum_yy).abs() <= eps * (ya @ ya.t())).all())


@pytest.mark.parametrize("lags,lead,clip,window", SETTINGS)
@pytest.mark.parametrize("bin_,channels", [(None, None), (5, SUBSET)])
def test_stats_from_a_file_equal_stats_of_what_read_returns(files, bin_, channels, lags, lead, clip, window):
    f = _File(files, "exact")
    halo = lags - 1 + window - 1
    try:
        for tiny in (False, True):
            a, b, n = _span(bin_, tiny)
            x = _resident(f, bin_, channels, tiny)
            y = _covariates(x)
            rows = int(x.shape[0])
            fr = wiener.fold_ranges(n - lead - (lags - 1), 5, lags - 1)       # edges inside batches, the first at the warm-up
            want = wiener.stats(x, y, lags, lead, clip, ranges=fr, window=window)
            for mb in ([_tiny_budget(rows, n, halo)] if tiny else _budgets(rows, n, halo)):
                src = f.bins(a, b, channels, bin_, mb)
                assert (src.rows, src.n) == (rows, n)
                _same_stats(wiener.stats_from(src, y, lags, lead, clip, ranges=fr, window=window), want, y, fr, lead, _fmax(clip, window))
            if not tiny:                                                     # no ranges: the one range of all design rows
                src = f.bins(a, b, channels, bin_, rows * (n // 3 - 11))
                whole = wiener.stats(x, y, lags, lead, clip, window=window)
                _same_stats(wiener.stats_from(src, y, lags, lead, clip, window=window), whole, y, [(lags - 1, n - lead)], lead,
                            _fmax(clip, window))
    finally:
        f.close()


@pytest.mark.parametrize("kind,bin_,channels", [("plain", None, None), ("plain", 5, SUBSET), ("container", None, SUBSET), ("container", 5, None)])
def test_stats_and_predictions_from_a_plain_archive_and_a_container(files, kind, bin_, channels):
    """the sources that copy what they decoded into the view (container_io.bins) and the archive without exact lists,
    under a halo: the clamped route, the two-plane window, the clip list, the FIR and the Kalman projection"""
    f = _File(files, kind)
    try:
        for tiny in (False, True):
            a, b, n = _span(bin_, tiny)
            x = _resident(f, bin_, channels, tiny)
            y = _covariates(x)
            rows = int(x.shape[0])
            for lags, lead, clip, window in (SETTINGS[1], SETTINGS[3]):
                halo = lags - 1 + window - 1
                fr = wiener.fold_ranges(n - lead - (lags - 1), 5, lags - 1)
                want = wiener.stats(x, y, lags, lead, clip, ranges=fr, window=window)
                mb = _tiny_budget(rows, n, halo) if tiny else _budgets(rows, n, halo)[1]
                with f.bins(a, b, channels, bin_, mb) as src:
                    _same_stats(wiener.stats_from(src, y, lags, lead, clip, ranges=fr, window=window), want, y, fr, lead, _fmax(clip, window))
            lags, lead = 5, 3
            fr = wiener.fold_ranges(n - lead - (lags - 1), 5, lags - 1)
            mb = _tiny_budget(rows, n, lags - 1) if tiny else _budgets(rows, n, lags - 1)[1]
            with f.bins(a, b, channels, bin_, mb) as src:
                for q, st in wiener.stats_clips_from(src, y, lags, lead, (1, 2), fr):
                    _same_stats(st, wiener.stats(x, y, lags, lead, q, ranges=fr), y, fr, lead, q)
                flt = wiener.WienerFilter(1e-2).fit(wiener.stats(x, y, lags, lead, 2))
                got, want = flt.predict_from(src), flt.predict(x)
                assert float((got.double() - want.double()).abs().max()) <= 2 * _gamma(lags * rows) * float(flt.weights.abs().sum(dim=(1, 2)).max()) * 2
                if channels is not None:                            # a repeated channel leaves no positive definite Q
                    continue
                kf = kalman.KalmanFilter(1e-2).fit(kalman.stats_from(src, y, lead, 2))
                rs = [(3, n // 2), (n // 2 + 7, n - lead)]
                p, pw = kf.predict_from(src, None, rs), kf.predict(x, None, rs)
                inside = ~torch.isnan(pw[0])
                assert torch.equal(torch.isnan(p), torch.isnan(pw))
                assert float((p[:, inside] - pw[:, inside]).abs().max()) <= 2 * 64 * D_KALMAN * float(y.double().std(1).max())
    finally:
        f.close()


def test_the_cascades_internal_entries_take_the_prediction_of_the_file_route(nonlinear):
    from tests.test_host_cascade import L, LEAD
    x, y, fn = nonlinear
    xv, yv = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    rs = [(L - 1, 1000), (2501, x.shape[1] - LEAD)]
    with archive.open(fn) as rd:
        src = rd.bins(0, x.shape[1], max_bytes=x.shape[0] * 1300)
        st = sum(wiener.stats_from(src, yv, L, LEAD, 2, ranges=rs))
        want = cascade.WienerCascade(1e-2, 3).fit(sum(wiener.stats(xv, yv, L, LEAD, 2, ranges=rs)), xv, yv, rs)
        c = cascade.WienerCascade(1e-2, 3)
        c.linear.fit(st)
        c._fit_stage(st, c.linear.predict_from(src), yv, rs)
        # the same integers; xty summed in another order moves the weights by its own rounding, far below the float32 prediction's
        assert torch.allclose(c.coef, want.coef, rtol=1e-6, atol=1e-6 * float(want.coef.abs().max()))
        for a, b in zip(c._score_stage(c.linear.predict_from(src), yv, rs), want.score(xv, yv, rs)):
            assert torch.allclose(a, b, rtol=1e-6, atol=0)


def test_a_single_fold_reads_less_than_the_range(files):
    lags, lead = 15, 3
    a, b, n = _span(None)
    fr = wiener.fold_ranges(n - lead - (lags - 1), 5, lags - 1)
    read = []
    for ranges in (fr, [fr[2]]):
        with archive.open(files["exact"]) as rd:
            x = rd.read(a, b)
            y = _covariates(x)
            before = rd.bytes_read
            src = rd.bins(a, b, max_bytes=C * (n // 16))
            got = wiener.stats_from(src, y, lags, lead, 3, ranges=ranges)
            read.append(rd.bytes_read - before)
            want = wiener.stats(x, y, lags, lead, 3, ranges=ranges)
            _same_stats(got, want, y, ranges, lead, 3)
    print("\nbytes read for five folds %d, for the third alone %d" % tuple(read))
    assert 0 < read[1] < read[0] // 2


def test_the_small_case_against_the_explicit_design_matrix(tmp_path):
    Cs, L, Ts, lead = 7, 5, 4000, 3
    x, y = data(Cs, L, K, Ts)
    fn = str(tmp_path / "small.mua")
    with archive.create(fn, Cs, S=S, hist_bits=6, seg_chunks=2, exact=True) as w:
        w.append(np.ascontiguousarray(x.T))
    yv = torch.from_numpy(y).cuda()
    with archive.open(fn) as rd:
        assert np.array_equal(rd.read(0, Ts).cpu().numpy(), x)
        for clip in (None, 2):
            r = wo.stats(x, y, L, lead, clip)
            mb = Cs * (Ts // 3 - 11)
            assert len(gram.halo_plan(Ts, Cs, L - 1, mb)) >= 3
            s = wiener.stats_from(rd.bins(0, Ts, max_bytes=mb), yv, L, lead, clip)[0]
            assert s.n == r["n"] and np.array_equal(s.gram.cpu().numpy(), r["gram"]) and np.array_equal(s.sum_x.cpu().numpy(), r["sum_x"])
            # the device's batched sum and the oracle's product are each within gamma_n of the exact sum
            assert (np.abs(s.xty.cpu().numpy() - r["xty"]) <= r["n"] * 2.0 ** -52 * r["abs_xty"]).all()


def test_stats_of_a_clip_list_equal_stats_from_clip_by_clip(files):
    lags, lead, clips = 5, 3, (2, 3, 39)
    f = _File(files, "exact")
    try:
        for tiny in (False, True):
            a, b, n = _span(5, tiny)
            x = _resident(f, 5, SUBSET, tiny)
            y = _covariates(x)
            fr = wiener.fold_ranges(n - lead - (lags - 1), 5, lags - 1)
            mb = _tiny_budget(4, n, lags - 1) if tiny else _budgets(4, n, lags - 1)[1]
            got = wiener.stats_clips_from(f.bins(a, b, SUBSET, 5, mb), y, lags, lead, clips, fr)
            assert [q for q, _s in got] == list(clips)
            for q, st in got:
                _same_stats(st, wiener.stats_from(f.bins(a, b, SUBSET, 5, mb), y, lags, lead, q, ranges=fr), y, fr, lead, q)
                _same_stats(st, wiener.stats(x, y, lags, lead, q, ranges=fr), y, fr, lead, q)
    finally:
        f.close()


# ---- predictions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 4])
def test_predict_from_a_file_is_predict_on_what_read_returns(files, window):
    lags, lead, clip = 15, 3, 3
    f = _File(files, "exact")
    try:
        for tiny in (False, True):
            a, b, n = _span(5, tiny)
            x = _resident(f, 5, SUBSET, tiny)
            y = _covariates(x)
            rows = int(x.shape[0])
            flt = wiener.WienerFilter(1e-2).fit(wiener.stats(x, y, lags, lead, clip, window=window))
            other = wiener.WienerFilter(1.0).fit(wiener.stats(x, y, 5, 0, None))
            want, want_other = flt.predict(x), other.predict(x)
            # both routes run float32 chains of L * C products: each is within gamma32 of the exact value
            bound = 2 * _gamma(lags * rows) * float(flt.weights.abs().sum(dim=(1, 2)).max()) * _fmax(clip, window)
            for mb in ([_tiny_budget(rows, n, lags - 1)] if tiny else _budgets(rows, n, lags - 1)):
                got = flt.predict_from(f.bins(a, b, SUBSET, 5, mb))
                assert got.dtype == torch.float32 and got.shape == want.shape == (K, n - lags + 1)
                err = float((got.double() - want.double()).abs().max())
                print("\nwindow %d, max_bytes %s: predict_from and predict differ by %.3g (bound %.3g), bit-identical: %s"
                      % (window, mb, err, bound, torch.equal(got, want)))
                assert err <= bound
                both = wiener.predict_many_from(f.bins(a, b, SUBSET, 5, mb), [other, flt])
                assert both[0].shape == want_other.shape and torch.equal(both[1], got)
                assert float((both[0].double() - want_other.double()).abs().max()) <= 2 * _gamma(5 * rows) * float(other.weights.abs().sum(dim=(1, 2)).max()) * 255
            rmse, cc = flt.score_from(f.bins(a, b, SUBSET, 5, None), y)
            r2, c2 = flt._score(got, y)
            assert torch.allclose(rmse, r2, rtol=1e-6) and torch.allclose(cc, c2, rtol=1e-6) and torch.allclose(rmse, flt.score(x, y)[0], rtol=1e-6)
    finally:
        f.close()


def test_predict_many_from_passes_once_per_group_that_fits(files):
    a, b, n = _span(5)
    with archive.open(files["exact"]) as rd:
        x = rd.read(a, a + n * 5, bin=5)
        y = _covariates(x)
        fs = [wiener.WienerFilter(al).fit(wiener.stats(x, y, 5, 0, 3)) for al in (0.0, 1e-2, 1.0)]
        want = [flt.predict(x) for flt in fs]
        one = 4 * K * (n - 4)                                                # the bytes of one prediction
        for mb, passes in ((1 << 30, 1), (2 * one, 2), (one, 3)):
            reads = []
            base = rd.bins(a, b, bin=5, max_bytes=mb)
            src = gram.BinSource(base.rows, base.n, base.device, mb, lambda b0, nb, view: (reads.append(b0), base.read_bins(b0, nb, view)))
            got = wiener.predict_many_from(src, fs)
            assert reads.count(0) == passes
            for flt, g_, w_ in zip(fs, got, want):
                assert float((g_.double() - w_.double()).abs().max()) <= 2 * _gamma(5 * C) * float(flt.weights.abs().sum(dim=(1, 2)).max()) * 3


def test_kalman_predict_from_a_file_is_predict_on_what_read_returns(files):
    lead, clip = 2, 3
    f = _File(files, "exact")
    try:
        a, b, n = _span(5)
        x = _resident(f, 5, None)
        y = _covariates(x)
        mb = _budgets(C, n, 0)[1]
        ks = kalman.stats(x, y, lead, clip)
        got = kalman.stats_from(f.bins(a, b, None, 5, mb), y, lead, clip)
        _same_stats([g_.w for g_ in got], [k_.w for k_ in ks], y, [(0, n - lead)], lead, clip)
        for name in ("sum_a", "sum_b", "aa", "bb", "ab", "sum_d", "dd", "ad"):
            assert torch.allclose(getattr(got[0], name), getattr(ks[0], name), rtol=1e-13, atol=0), name
        assert got[0].n_pairs == ks[0].n_pairs
        flt = kalman.KalmanFilter(1e-2).fit(ks)
        ranges = [(5, 700), (700, 2300), (4000, n - lead)]
        y0 = torch.stack([y[:, s + lead] for s, _e in ranges]).double()
        # each route is within 64 D_KALMAN of the state's spread of the reference's loop (tests/test_gpu_kalman.py)
        bound = 2 * 64 * D_KALMAN * float(y.double().std(1).max())
        for rs, first in ((None, None), (ranges, None), (ranges, y0)):
            want = flt.predict(x, first, rs)
            for budget in (None, mb):
                p = flt.predict_from(f.bins(a, b, None, 5, budget), first, rs)
                assert p.dtype == torch.float64 and p.shape == want.shape == (K, n)
                inside = ~torch.isnan(want[0])
                assert torch.equal(torch.isnan(p), torch.isnan(want))
                err = float((p[:, inside] - want[:, inside]).abs().max())
                print("\nkalman predict_from, ranges %s, y0 %s, max_bytes %s: differs by %.3g (bound %.3g), bit-identical: %s"
                      % (rs is not None, first is not None, budget, err, bound, torch.equal(p[:, inside], want[:, inside])))
                assert err <= bound
        rmse, cc = flt.score_from(f.bins(a, b, None, 5, mb), y, ranges[:2])
        r2, c2 = flt.score(x, y, ranges[:2])
        assert torch.allclose(rmse, r2, rtol=1e-9) and torch.allclose(cc, c2, rtol=1e-9)
    finally:
        f.close()


# ---- cross-validation ------------------------------------------------------------------------------------------------------
def _stored(tmp, name, x, lens):
    """x [channels, bins] in an exact archive of blocks of `lens` bins"""
    fn = str(tmp / name)
    with archive.create(fn, x.shape[0], S=S, hist_bits=6, seg_chunks=2, exact=True) as w:
        t = 0
        for n in lens:
            w.append(np.ascontiguousarray(x[:, t:t + n].T))
            t += n
    assert t == x.shape[1]
    return fn


@pytest.fixture(scope="module")
def nonlinear(tmp_path_factory):
    x, y = nonlinear_data()
    return x, y, _stored(tmp_path_factory.mktemp("cv"), "nonlinear.mua", x, (1500, 1200, 1300))


@pytest.mark.parametrize("clip", [None, 2])
def test_cascade_cross_validate_from_a_file_gives_the_oracles_arrays(nonlinear, clip):
    from tests.test_host_cascade import L, LEAD
    x, y, fn = nonlinear
    Cn, Tn = x.shape
    alphas, degrees, F = (0.0, 1e-2), (None, 2, 4), 5
    want = co.cross_validate(x, y, L, LEAD, clip, alphas, degrees, F)
    yv = torch.from_numpy(y).cuda()
    with archive.open(fn) as rd:
        assert np.array_equal(rd.read(0, Tn).cpu().numpy(), x)
        mb = Cn * (Tn // 3 - 11)
        assert len(gram.halo_plan(Tn, Cn, L - 1, mb)) >= 3
        routes = {"cross_validate_from": cascade.cross_validate_from(rd.bins(0, Tn, max_bytes=mb), yv, L, LEAD, clip, alphas, degrees, F),
                  "sweep_clips_from": cascade.sweep_clips_from(rd.bins(0, Tn, max_bytes=mb), yv, L, LEAD, (clip or 255,), alphas, degrees, F)[clip or 255]}
    for route, got in routes.items():
        assert set(got) == set(want)
        worst = 0.0
        for key in want:
            for name, w in want[key].items():
                g = got[key][name]
                assert g.dtype == torch.float64 and tuple(g.shape) == (F, K)
                rel = np.abs(g.cpu().numpy() - w) / np.abs(w)
                worst = max(worst, rel.max())
                assert (rel <= 64 * CV_REF).all(), (route, key, name, rel.max())
        print("\n%s, clip %s: worst relative difference from the oracle's loop %.3g (allowed %.3g)" % (route, clip, worst, 64 * CV_REF))


def test_kalman_cross_validate_from_a_file_is_the_reference_loop(tmp_path):
    Ck, Tk, lead, clip, folds = 7, 4000, 2, 3, 5
    x, y = ko.data(Ck, 2, Tk, 1)
    fn = _stored(tmp_path, "kalman.mua", x, (1500, 1200, 1300))
    fr = wiener.fold_ranges(Tk - lead, folds)
    alphas = (0.0, 1e-2)
    with archive.open(fn) as rd:
        assert np.array_equal(rd.read(0, Tk).cpu().numpy(), x)
        mb = Ck * (Tk // 3 - 11)
        res = kalman.cross_validate_from(rd.bins(0, Tk, max_bytes=mb), torch.from_numpy(y).cuda(), lead, clip, alphas, folds)
    std = y.astype(np.float64).std(1)
    for j, alpha in enumerate(alphas):
        for i in (0, folds - 1):
            v, t = i, (i + 1) % folds
            (rv, cv), (rt, ct) = _scores(x, y, lead, clip, alpha, [fr[k] for k in range(folds) if k not in (v, t)], [fr[v], fr[t]])
            for name, ref in (("rmse_valid", rv), ("rmse_test", rt), ("cc_valid", cv), ("cc_test", ct)):
                got = res[name][j, i].cpu().numpy()
                d = np.abs(got - ref) / (2 * std if name.startswith("rmse") else 4.0)   # as tests/test_gpu_kalman.py weighs them
                print("\nalpha %g split %d %s: %.3g (allowed %.3g)" % (alpha, i, name, d.max(), 64 * D_KALMAN))
                assert (d <= 64 * D_KALMAN).all()
    assert all(tuple(res[k].shape) == (2, folds, 2) and res[k].dtype == torch.float64 for k in res)


# ---- refusals, before anything is read -------------------------------------------------------------------------------------
def test_what_is_refused_before_anything_is_launched(files):
    with archive.open(files["exact"]) as rd:
        before = rd.bytes_read
        src = rd.bins(1000, 6000, bin=5)
        assert (src.rows, src.n) == (C, 1000)
        y = torch.zeros((K, 1000), dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError, match="same number of bins"):
            wiener.stats_from(src, y[:, :999], 5)
        with pytest.raises(ValueError, match="design rows"):
            wiener.stats_from(src, y, 5, 3, ranges=[(4, 998)])
        with pytest.raises(ValueError, match="design rows"):
            wiener.stats_clips_from(src, y, 5, 0, (2, 3), [(3, 10)])
        with pytest.raises(ValueError, match="multiple of the bin factor"):
            rd.bins(1001, 6000, bin=5)
        with pytest.raises(ValueError, match="multiple of the bin factor"):
            cio.bins(files["container"], 1001, 6000, bin=5)
        with pytest.raises(ValueError, match="leaves no bin"):
            rd.read_gram(1000, 6000, bin=5, lag=1000)
        with pytest.raises(ValueError, match="leaves no bin"):
            rd.read_gram(1000, 6000, bin=5, lag=[0, 1000])
        with pytest.raises(ValueError):
            rd.read_gram(1000, 6000, lag=-1)
        with pytest.raises(ValueError, match="BinSource"):
            wiener.stats_from(torch.zeros((C, 1000), dtype=torch.uint8, device="cuda"), y, 5)
        with pytest.raises(ValueError):
            cascade.cross_validate_from(src, y, 5, num_fold=2)
        assert rd.bytes_read == before
        xs = torch.from_numpy(np.random.RandomState(2).poisson(1.0, (7, 500)).astype(np.uint8)).cuda()
        ys = torch.from_numpy(np.random.RandomState(3).randn(K, 500).astype(np.float32)).cuda()
        flt = wiener.WienerFilter(1e-2).fit(wiener.stats(xs, ys, 5))
        kf = kalman.KalmanFilter(1e-2).fit(kalman.stats(xs, ys))
        with pytest.raises(ValueError, match="fitted on 7 channels, not 12"):
            flt.predict_from(src)
        with pytest.raises(ValueError, match="fitted on 7 channels, not 12"):
            kf.predict_from(src)
        with pytest.raises(ValueError, match="comes after fit"):
            wiener.WienerFilter().predict_from(src)
        assert rd.bytes_read == before
