"""The Wiener cascade on the GPU (include/muahuff_cascade.h, csrc/mh_cascade.hpp, cascade.py).  mhc_moments against NumPy
on small integers -- equal, not close -- over every float offset of p and y, runs, degrees and kinds of ranges, past both
grid caps, and within the order-free float64 bound on general floats; mhc_polyval against the integer result -- equal --
in place and out of place, past its grid cap, and within Horner's bound on general floats; WienerCascade against the
oracle stage by stage; cross_validate against the oracle's explicit loop; and the contract: graph capture and replay, and
return before the stream drains."""
import time

import numpy as np
import pytest
import torch

from muahuff import _cascade, cascade, wiener
from tests import cascade_oracle as co
from tests import wiener_oracle as wo
from tests.test_gpu_wiener import _dev, _devf, _gamma
from tests.test_host_cascade import (D_POLY, K, L, LEAD, MAX_BLOCKS, POLY_MAX_BLOCKS, RUN, SUM_MAX_BLOCKS, SUM_THREADS, T, TILE,
                                     _tiling, layout, nonlinear_data)

pytestmark = pytest.mark.gpu

# The largest relative difference, over the four arrays of every (alpha, degree), between two runs of the oracle's
# cross-validation loop on nonlinear_data() (alphas 0 and 1e-2, degrees None, 2, 4, 5 folds): in float64 throughout, and
# with the linear prediction rounded to float32 before np.polyfit and np.polyval see it, which is what the device's
# polynomial is given.  As measured: 1.05e-7 without a clip, 2.9e-8 at clip 2.  The device is allowed 64 times CV_REF:
# its float32 prediction is a chain of C * L products, not one rounding, and its solver sums in another order.
CV_REF = 1.1e-7


def _pitched(a, lead):
    """a float32 matrix as a pitched device view with an odd pitch, its first element `lead` floats in, nan around the rows"""
    return _devf(a, lead=lead, extra=5 if a.shape[1] % 2 == 0 else 6)


def _f64(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()


def _f32(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()


def _moments(pv, yv, ranges, degree, center=None, inv=None, out=None, accumulate=False):
    """one mhc_moments on views pv, yv [k, cols] -> the device result [ranges, k, 3 * degree + 4]"""
    k, cols = pv.shape
    if out is None:
        out = torch.full((len(ranges), k, _cascade.per(degree)), float("nan"), dtype=torch.float64, device="cuda")
    scratch = torch.full((_cascade.moments_scratch_bytes(cols, k, degree, len(ranges)),), 0xFF, dtype=torch.uint8, device="cuda")
    _cascade.moments(pv, yv, ranges, degree, center, inv, out, scratch, accumulate)
    return out


def _range_sets(cols):
    """one full range; three that tile; empty ones among them; one that starts and ends at odd columns inside a run;
    sixteen"""
    sets = [[(0, cols)], [(0, 0), (cols // 2, cols // 2), (cols // 2, cols)]]
    if cols >= 3:
        sets.append(_tiling(cols, 3))
    if cols > RUN + 1000:
        sets.append([(RUN + 1, RUN + 778)])
    if cols >= 1000:
        sets.append([(3, 777)])
        sets.append(_tiling(cols, 16))
    return sets


def _small_integers(k, cols, seed, top=6):
    """p: even integers, |p| <= top; y: integers, |y| <= 3; center: even integers; inv_scale 0.5: u is an integer"""
    rng = np.random.RandomState(seed)
    p = (2 * rng.randint(-(top // 2), top // 2 + 1, (k, cols))).astype(np.float32)
    y = rng.randint(-3, 4, (k, cols)).astype(np.float32)
    center = (2 * rng.randint(-1, 2, (k,))).astype(np.float64)
    return p, y, center, np.full((k,), 0.5)


# (cols, k, degree): every value of every axis; the float offsets of p and y cycle with the index
MOM_SHAPES = [(1, 1, 1), (RUN + 3, 2, 4), (3 * RUN + 5, 8, 6), (1, 8, 4), (RUN + 3, 1, 6), (3 * RUN + 5, 2, 1), (1, 2, 6), (RUN + 3, 8, 1),
              (3 * RUN + 5, 1, 4)]


@pytest.mark.parametrize("i,shape", list(enumerate(MOM_SHAPES)), ids=["%dx%d-D%d" % (s[1], s[0], s[2]) for s in MOM_SHAPES])
def test_moments_equal_numpy_on_small_integers(i, shape):
    cols, k, degree = shape
    p, y, center, inv = _small_integers(k, cols, 200 + i)
    terms = co.moment_terms(p, y, degree, center, inv)
    assert cols * np.abs(terms).max() < 2.0 ** 53                 # every sum of them is exact, in any order
    assert (terms == np.rint(terms)).all()
    pv, yv = _pitched(p, i % 4), _pitched(y, (3 * i + 1) % 4)
    assert pv.stride(0) % 2 == 1 and yv.stride(0) % 2 == 1 and pv.data_ptr() % 16 == 4 * (i % 4) and yv.data_ptr() % 16 == 4 * ((3 * i + 1) % 4)
    cd, sd = _f64(center), _f64(inv)
    for rs in _range_sets(cols):
        want = np.stack([terms[:, :, a:b].sum(2) for a, b in rs])
        out = _moments(pv, yv, rs, degree, cd, sd)
        again = _moments(pv, yv, rs, degree, cd, sd)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got, want), (rs, np.argwhere(got != want)[:5])
        assert np.array_equal(got[:, :, 0], np.array([[b - a] * k for a, b in rs], np.float64))
        assert np.array_equal(again.cpu().numpy().view(np.uint64), got.view(np.uint64))    # identical bits
        _moments(pv, yv, rs, degree, cd, sd, out=out, accumulate=True)                     # accumulate: twice the result
        assert np.array_equal(out.cpu().numpy(), 2 * want)
        _moments(pv, yv, rs, degree, cd, sd, out=out, accumulate=False)                    # ... and overwrite
        assert np.array_equal(out.cpu().numpy(), want)
    # without center and inv_scale u is p itself
    raw = co.moment_terms(p, y, degree)
    if cols * np.abs(raw).max() < 2.0 ** 53:
        assert np.array_equal(_moments(pv, yv, [(0, cols)], degree).cpu().numpy()[0], raw.sum(2))


def test_a_range_gives_the_same_bits_alone_and_next_to_others():
    """on general floats, where the order of the sums shows: a range's runs are counted from its own start"""
    cols, k, degree = 3 * RUN + 5, 2, 4
    rng = np.random.RandomState(7)
    pv, yv = _pitched(rng.randn(k, cols).astype(np.float32), 1), _pitched(rng.randn(k, cols).astype(np.float32), 2)
    cd, sd = _f64(rng.randn(k)), _f64(1.0 / (1.0 + rng.rand(k)))
    for rs in (_tiling(cols, 3), _tiling(cols, 16), [(0, 0), (5, RUN + 6), (RUN + 7, RUN + 7), (2 * RUN + 1, cols)]):
        both = _moments(pv, yv, rs, degree, cd, sd).cpu().numpy()
        for r, ab in enumerate(rs):
            alone = _moments(pv, yv, [ab], degree, cd, sd).cpu().numpy()
            assert np.array_equal(alone[0].view(np.uint64), both[r].view(np.uint64)), (rs, r)


def test_moments_past_the_first_grid_cap():
    """8 outputs x 257 runs are more (run, output) items than the first kernel's capped grid has workgroups: the stride
    loop's second trip.  The reference is torch's float64 sum on the device, exact on these integers (the terms of 8 x
    4.2 million columns are too many to lay out on the host in a quick test)."""
    k, degree = 8, 1
    cols = (MAX_BLOCKS // k + 1) * RUN
    lay = layout(cols, k, degree, [(0, cols)])
    assert lay[1] > lay[4] == MAX_BLOCKS
    g = torch.Generator(device="cuda").manual_seed(3)
    p = (2 * torch.randint(-3, 4, (k, cols), generator=g, device="cuda")).float()
    y = torch.randint(-3, 4, (k, cols), generator=g, device="cuda").float()
    assert cols * 9 * 3 < 2 ** 53
    u, yd = (p.double() - 2.0) * 0.5, y.double()
    want = torch.stack([torch.full((k,), float(cols), dtype=torch.float64, device="cuda"), u.sum(1), (u * u).sum(1), yd.sum(1), (u * yd).sum(1),
                        (yd * yd).sum(1), ((u - yd) * (u - yd)).sum(1)], 1)
    got = _moments(p, y, [(0, cols)], degree, _f64(np.full(k, 2.0)), _f64(np.full(k, 0.5)))
    assert torch.equal(got[0], want)
    far = [(cols - RUN - 3, cols - 1)]                            # ... and a range that starts far in
    sl = slice(*far[0])
    assert torch.equal(_moments(p, y, far, degree)[0, :, 1], p[:, sl].double().sum(1))


def test_moments_past_the_second_grid_cap():
    """16 ranges x 8 outputs x 22 sums are more elements than the sum kernel's capped grid has threads"""
    cols, k, degree = 1000, 8, 6
    rs = _tiling(cols, 16)
    lay = layout(cols, k, degree, rs)
    assert len(rs) == 16 and lay[5] > lay[6] * SUM_THREADS and lay[6] == SUM_MAX_BLOCKS
    p, y, center, inv = _small_integers(k, cols, 9)
    terms = co.moment_terms(p, y, degree, center, inv)
    assert cols * np.abs(terms).max() < 2.0 ** 53
    got = _moments(_pitched(p, 3), _pitched(y, 0), rs, degree, _f64(center), _f64(inv)).cpu().numpy()
    assert np.array_equal(got, np.stack([terms[:, :, a:b].sum(2) for a, b in rs]))


def test_moments_on_general_floats_are_within_the_order_free_float64_bound():
    """|got - ref| <= n * 2^-53 * sum |term|: the terms are NumPy's bit for bit, and any order of summing n of them in
    float64 stays inside it"""
    cols, k, degree = 3 * RUN + 5, 2, 4
    rng = np.random.RandomState(11)
    p, y = (1.5 * rng.randn(k, cols) + 0.3).astype(np.float32), rng.randn(k, cols).astype(np.float32)
    center = p.astype(np.float64).mean(1)
    inv = 1.0 / p.astype(np.float64).std(1)
    rs = _tiling(cols, 5)
    ref, mag = co.moments(p, y, rs, degree, center, inv)
    pv, yv = _pitched(p, 3), _pitched(y, 1)
    a, b = _moments(pv, yv, rs, degree, _f64(center), _f64(inv)).cpu().numpy(), _moments(pv, yv, rs, degree, _f64(center), _f64(inv)).cpu().numpy()
    n = np.array([hi - lo for lo, hi in rs], np.float64)[:, None, None]
    bound = n * 2.0 ** -53 * mag
    err = np.abs(a - ref)
    print("\nmoments general floats: worst error / bound = %.3g" % (err / bound).max())
    assert (err <= bound).all()
    assert np.array_equal(a[:, :, 0], np.broadcast_to(n[:, :, 0], (len(rs), k)))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # through the public call: the same sums, split into the fields
    m = cascade.moments(pv, yv, rs, degree, _f64(center), _f64(1.0 / inv))
    assert m.degree == degree and m.ranges == [[ab] for ab in rs] and tuple(m.t.shape) == (5, k, 9) and tuple(m.q.shape) == (5, k, 5)
    inv2 = (1.0 / _f64(1.0 / inv)).cpu().numpy()                   # the reciprocal the public call took
    ref2, mag2 = co.moments(p, y, rs, degree, center, inv2)
    got2 = torch.cat([m.t, m.q, m.yy.unsqueeze(-1), m.err.unsqueeze(-1)], -1).cpu().numpy()
    assert (np.abs(got2 - ref2) <= n * 2.0 ** -53 * mag2).all()
    tot = m.total()
    assert tuple(tot.t.shape) == (k, 9) and torch.equal(tot.n.cpu(), torch.full((k,), float(cols), dtype=torch.float64))


# ---- mhc_polyval -------------------------------------------------------------------------------------------------------
def _polyval(pv, coef, center, inv, out):
    _cascade.polyval(pv, _f32(coef), _f32(center), _f32(inv), out)
    return out


# (cols, k, degree): one column, 255, a tile and one, three tiles and five
POLY_SHAPES = [(1, 1, 1), (255, 3, 3), (TILE + 1, 8, 6), (3 * TILE + 5, 1, 3), (1, 8, 6), (255, 1, 6), (TILE + 1, 3, 1), (3 * TILE + 5, 8, 1),
               (3 * TILE + 5, 3, 6)]


@pytest.mark.parametrize("i,shape", list(enumerate(POLY_SHAPES)), ids=["%dx%d-D%d" % (s[1], s[0], s[2]) for s in POLY_SHAPES])
def test_polyval_equals_the_integer_result(i, shape):
    cols, k, degree = shape
    rng = np.random.RandomState(300 + i)
    p = (2 * rng.randint(-2, 3, (k, cols)) + 1).astype(np.float32)             # odd; center odd, inv_scale 0.5: u integer, |u| <= 3
    center, inv = (2 * rng.randint(-1, 1, (k,)) + 1).astype(np.float32), np.full((k,), 0.5, np.float32)
    coef = rng.randint(-7, 8, (k, degree + 1)).astype(np.float32)
    coef[:, 0] = np.where(coef[:, 0] == 0, 3, coef[:, 0])
    want, mag = co.polyval(p, coef, center, inv)
    assert mag.max() < 2 ** 24 and (want == np.rint(want)).all()               # every Horner partial is an exact float32
    for in_place in (False, True):
        pv = _pitched(p, i % 4)
        out = pv if in_place else _pitched(np.full((k, cols), np.nan, np.float32), (i + 1 + i // 4) % 4)
        _polyval(pv, coef, center, inv, out)
        again = _polyval(_pitched(p, i % 4), coef, center, inv, _pitched(np.full((k, cols), np.nan, np.float32), (i + 2) % 4))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (in_place, np.argwhere(got != want)[:5])
        assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32))
        flat = out._base.cpu().numpy()                                          # nothing around the rows was written
        assert np.isnan(flat).sum() == flat.size - k * cols
        if not in_place:
            assert np.array_equal(pv.cpu().numpy(), p)                          # ... and the input is as it was
    # without center and inv_scale u is p itself
    want0, mag0 = co.polyval(p, coef)
    assert mag0.max() < 2 ** 24
    got0 = torch.empty((k, cols), dtype=torch.float32, device="cuda")
    _cascade.polyval(_pitched(p, 1), _f32(coef), None, None, got0)
    assert np.array_equal(got0.cpu().numpy().astype(np.float64), want0)


def test_polyval_past_the_grid_cap():
    """one output, a column more than the capped grid has tiles: the stride loop's second trip"""
    cols = POLY_MAX_BLOCKS * TILE + 1
    assert layout(cols, 1, 1, [(0, 1)])[9:] == [POLY_MAX_BLOCKS + 1, POLY_MAX_BLOCKS]
    p = torch.randint(-100, 101, (1, cols), generator=torch.Generator(device="cuda").manual_seed(4), device="cuda").float()
    out = torch.full((1, cols), float("nan"), dtype=torch.float32, device="cuda")
    _cascade.polyval(p, _f32(np.array([[3, -5]])), None, None, out)
    assert torch.equal(out, 3 * p - 5)


def test_polyval_on_general_floats_is_within_horners_bound():
    """|got - ref| <= gamma_(2 * degree + 2) * sum |c_i| |u|^i in float32 arithmetic; ref is float64 on the same float32
    inputs"""
    cols, k = 3 * TILE + 5, 3
    rng = np.random.RandomState(21)
    p = (1.5 * rng.randn(k, cols) + 0.3).astype(np.float32)
    center, inv = rng.randn(k).astype(np.float32), (1.0 / (1.0 + rng.rand(k))).astype(np.float32)
    for degree in (1, 3, 6):
        coef = rng.randn(k, degree + 1).astype(np.float32)
        ref, mag = co.polyval(p, coef, center, inv)
        pv = _pitched(p, 2)
        a = _polyval(pv, coef, center, inv, torch.empty((k, cols), dtype=torch.float32, device="cuda")).cpu().numpy()
        b = _polyval(pv, coef, center, inv, _pitched(np.zeros((k, cols), np.float32), 1)).cpu().numpy()
        bound = _gamma(2 * degree + 2) * mag
        err = np.abs(a.astype(np.float64) - ref)
        print("\npolyval general floats, degree %d: worst error / bound = %.3g" % (degree, (err / bound).max()))
        assert (err <= bound).all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- WienerCascade -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    x, y = nonlinear_data()
    return x, y, _dev(x, lead=1), _devf(y, lead=2)


def _values(coef, u):
    return np.stack([np.polyval(coef[k], u[k]) for k in range(len(coef))])


@pytest.mark.parametrize("clip", [None, 2])
def test_the_cascade_fits_predicts_and_scores_as_the_oracle(world, clip):
    x, y, xv, yv = world
    degree, n = 3, T - L + 1 - LEAD
    s = wiener.stats(xv, yv, L, LEAD, clip)[0]
    c = cascade.WienerCascade(1e-2, degree).fit(s, xv, yv)
    assert c.coef.is_cuda and c.coef.dtype == torch.float64 and tuple(c.coef.shape) == (K, degree + 1)
    # the polynomial: np.polyfit on the device's own linear prediction, compared by value at the training predictions
    lin = c.linear.predict(xv).cpu().numpy()
    p64, Y = lin[:, :n].astype(np.float64), y[:, L - 1 + LEAD:].astype(np.float64)
    center, inv = c.center.cpu().numpy(), (1.0 / c.scale).cpu().numpy()
    assert np.allclose(center, p64.mean(1), rtol=0, atol=1e-4 * p64.std(1).max()) and np.allclose(c.scale.cpu().numpy(), p64.std(1), rtol=1e-4)
    u = (p64 - center[:, None]) * inv[:, None]
    want = _values([np.polyfit(p64[k], Y[k], degree) for k in range(K)], p64)
    got = _values(c.coef.cpu().numpy(), u)
    d = (np.abs(got - want).max(1) / Y.std(1)).max()
    print("\nfit: the polynomials differ by %.3g of the target's spread" % d)
    assert d <= 64 * D_POLY
    # predict: float64 polyval of the cascade's own coefficients on the float32 linear prediction, within Horner's bound
    # plus the casts of coef (2^-24 of every term), center and inv_scale (which move u by 2^-24 (|center| inv + |u|), and
    # the value by that times sum i |c_i| |u|^(i-1))
    pred = c.predict(xv)
    pr = pred.cpu().numpy()
    assert pr.dtype == np.float32 and pr.shape == (K, T - L + 1)
    coef = c.coef.cpu().numpy()
    ref, mag = co.polyval(lin, coef, center, inv)
    ua = np.abs((lin.astype(np.float64) - center[:, None]) * inv[:, None])
    slope = sum(i * np.abs(coef[:, degree - i:degree - i + 1]) * ua ** (i - 1) for i in range(1, degree + 1))
    bound = (_gamma(2 * degree + 2) + 2.0 ** -24) * mag + 1.01 * 2.0 ** -24 * (np.abs(center * inv)[:, None] + ua) * slope
    err = np.abs(pr.astype(np.float64) - ref)
    print("predict: worst error / bound = %.3g" % (err / bound).max())
    assert (err <= bound).all()
    # score: per range of design rows, against the oracle's metrics on the copied prediction
    rs = [(L - 1, 1000), (1000, 2501), (2501, T - LEAD)]
    for ranges in (None, rs):
        rmse, cc = c.score(xv, yv, ranges)
        cols = [(0, n)] if ranges is None else [(a - (L - 1), b - (L - 1)) for a, b in ranges]
        assert rmse.dtype == torch.float64 and tuple(rmse.shape) == tuple(cc.shape) == (len(cols), K)
        for r, (a, b) in enumerate(cols):
            yt, yp = Y[:, a:b].T, pr[:, a:b].T.astype(np.float64)
            assert np.allclose(rmse[r].cpu().numpy(), wo.rmse(yt, yp), rtol=1e-6, atol=0)
            assert np.allclose(cc[r].cpu().numpy(), wo.pearson(yt, yp), rtol=1e-6, atol=0)
    # on the training rows the polynomial does not lose to the line it contains
    lin_rmse = wo.rmse(Y.T, p64.T)
    assert (c.score(xv, yv)[0][0].cpu().numpy() <= lin_rmse * (1 + 1e-6)).all()
    # a fit on two of three ranges: the statistics and the ranges name the same rows
    parts = wiener.stats(xv, yv, L, LEAD, clip, ranges=rs)
    c2 = cascade.WienerCascade(1e-2, 2).fit(parts[0] + parts[2], xv, yv, [rs[0], rs[2]])
    lin2 = c2.linear.predict(xv).cpu().numpy()[:, :n].astype(np.float64)
    idx = np.r_[0:1000 - (L - 1), 2501 - (L - 1):n]
    want2 = _values([np.polyfit(lin2[k, idx], Y[k, idx], 2) for k in range(K)], lin2[:, idx])
    u2 = (lin2[:, idx] - c2.center.cpu().numpy()[:, None]) * (1.0 / c2.scale).cpu().numpy()[:, None]
    assert (np.abs(_values(c2.coef.cpu().numpy(), u2) - want2).max(1) / Y.std(1)).max() <= 64 * D_POLY
    with pytest.raises(ValueError):
        cascade.WienerCascade(1e-2, 2).fit(parts[0] + parts[2], xv, yv, [rs[0]])


@pytest.mark.parametrize("clip", [None, 2])
def test_cross_validate_gives_the_arrays_of_the_oracles_loop(world, clip):
    x, y, xv, yv = world
    alphas, degrees, F = (0.0, 1e-2), (None, 2, 4), 5
    got = cascade.cross_validate(xv, yv, L, LEAD, clip, alphas, degrees, F)
    want = co.cross_validate(x, y, L, LEAD, clip, alphas, degrees, F)
    assert set(got) == set(want) == {(a, d) for a in alphas for d in degrees}
    worst = 0.0
    for key in want:
        assert set(got[key]) == {"rmse_valid", "rmse_test", "cc_valid", "cc_test"}
        for name, w in want[key].items():
            g = got[key][name]
            assert g.dtype == torch.float64 and tuple(g.shape) == (F, K)
            rel = np.abs(g.cpu().numpy() - w) / np.abs(w)
            worst = max(worst, rel.max())
            assert (rel <= 64 * CV_REF).all(), (key, name, rel.max())
    print("\ncross_validate, clip %s: worst relative difference from the oracle's loop %.3g (allowed %.3g)" % (clip, worst, 64 * CV_REF))
    # the linear decoder's entries are WienerFilter.score on each held-out fold
    n = T - LEAD - (L - 1)
    fr = wiener.fold_ranges(n, F, L - 1)
    st = wiener.stats(xv, yv, L, LEAD, clip, ranges=fr)
    for a in alphas:
        for i in range(F):
            v, t = i, (i + 1) % F
            f = wiener.WienerFilter(a).fit(sum(st[k] for k in range(F) if k not in (v, t)))
            for name, fold in (("valid", v), ("test", t)):
                lo, hi = fr[fold]
                rmse, cc = f.score(xv[:, lo - (L - 1):hi + LEAD], yv[:, lo - (L - 1):hi + LEAD])
                assert torch.allclose(got[(a, None)]["rmse_" + name][i], rmse, rtol=1e-6, atol=0)
                assert torch.allclose(got[(a, None)]["cc_" + name][i], cc, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        cascade.cross_validate(xv, yv, L, LEAD, clip, alphas, degrees, 2)


# ---- the contract -------------------------------------------------------------------------------------------------------
DELAY_BYTES, DELAY_PASSES = 512 << 20, 24     # as tests/test_gpu_async_contract.py: tens of milliseconds on the device


def _pair(pv, coef, center, inv, tmp, yv, rs, degree, out, scratch):
    _cascade.polyval(pv, coef, center, inv, tmp)
    _cascade.moments(tmp, yv, rs, degree, None, None, out, scratch)


def test_the_pair_is_captured_replayed_and_returns_before_the_stream_drains():
    cols, k, degree = RUN + 3, 2, 2
    rng = np.random.RandomState(31)
    p = (2 * rng.randint(-2, 3, (k, cols)) + 1).astype(np.float32)
    y = rng.randint(-3, 4, (k, cols)).astype(np.float32)
    coef_h, center_h, inv_h = rng.randint(-3, 4, (k, degree + 1)).astype(np.float32), np.ones(k, np.float32), np.full(k, 0.5, np.float32)
    rs = _tiling(cols, 3)
    want_poly, mag = co.polyval(p, coef_h, center_h, inv_h)
    terms = co.moment_terms(want_poly.astype(np.float32), y, degree)
    assert mag.max() < 2 ** 24 and cols * np.abs(terms).max() < 2.0 ** 53
    want = np.stack([terms[:, :, a:b].sum(2) for a, b in rs])
    pv, yv = _pitched(p, 1), _pitched(y, 3)
    coef, center, inv = _f32(coef_h), _f32(center_h), _f32(inv_h)
    tmp = torch.zeros((k, cols), dtype=torch.float32, device="cuda")
    out = torch.zeros((len(rs), k, _cascade.per(degree)), dtype=torch.float64, device="cuda")
    scratch = torch.zeros((_cascade.moments_scratch_bytes(cols, k, degree, len(rs)),), dtype=torch.uint8, device="cuda")
    args = (pv, coef, center, inv, tmp, yv, rs, degree, out, scratch)
    ok = lambda: np.array_equal(out.cpu().numpy(), want) and np.array_equal(tmp.cpu().numpy().astype(np.float64), want_poly)  # noqa: E731
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _pair(*args)                                                            # eager, and the warm-up
    side.synchronize()
    assert ok()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _pair(*args)                                                            # the ranges travel by value: no upload to capture
    out.fill_(-1), tmp.fill_(-1), scratch.fill_(0xFF)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert ok()
    # behind a delay on the stream: both calls return while the delay is still running
    out.fill_(-1), tmp.fill_(-1)
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
    assert ok()
