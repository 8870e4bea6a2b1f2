"""mhi_gram on the GPU (include/muahuff_ingest.h, csrc/mh_gram.hpp): the channel-by-channel Gram matrix of uint8 counts on
the int8 matrix cores against NumPy's int64 product -- equal, not close: the value boundaries of the XOR-0x80 operands,
the C/D lane map on data whose every element is distinct, ragged shapes and pitches, every byte alignment of both
operands with 255 around the rows, more columns than one int32 accumulator could sum (in runs of one slice: the runs of
full length, 2^30 in an accumulator, are tests/test_gpu_gram_tiles.py's), a grid past its cap, accumulate, the symmetric
form against the cross form, lags, the float results, the stream order, and capture into a graph and replay."""
import numpy as np
import pytest
import torch

from muahuff import _ingest, gram
from tests.test_host_gram import MAX_BLOCKS, RUN_SLICES, SLICE, layout

pytestmark = pytest.mark.gpu


def _ref(x, y=None):
    y = x if y is None else y
    return x.astype(np.int64) @ y.astype(np.int64).T, x.sum(1, dtype=np.int64), y.sum(1, dtype=np.int64)


def _dev(x, lead=1, extra=37):
    """the matrix as a pitched device view whose first byte sits at `lead` mod 128, every byte around the rows 255"""
    rows, cols = x.shape
    pitch = cols + extra
    buf = torch.full((rows * pitch + lead + 256,), 255, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 128 == 0
    view = buf.as_strided((rows, cols), (pitch, 1), lead)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    return view


def _call(a, b=None, out=None, sa=None, sb=None, accumulate=False, sums=True):
    """one mhi_gram on views a [ra, cols] and b [rb, cols] (None: the symmetric form) -> (gram, sum_a, sum_b) as NumPy"""
    ra, cols = a.shape
    rb = ra if b is None else b.shape[0]
    if out is None:
        out = torch.full((ra, rb), -7, dtype=torch.int64, device="cuda")
        sa = torch.full((ra,), -7, dtype=torch.int64, device="cuda") if sums else None
        sb = torch.full((rb,), -7, dtype=torch.int64, device="cuda") if sums else None
    _ingest.gram(a.data_ptr(), a.stride(0) if ra > 1 else cols, ra, None if b is None else b.data_ptr(),
                 0 if b is None else (b.stride(0) if rb > 1 else cols), 0 if b is None else rb, cols, out, sa, sb, accumulate)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if sa is None else sa.cpu().numpy(), None if sb is None else sb.cpu().numpy()


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)


def _random(rows, cols, seed):
    rng = np.random.RandomState(seed)
    x = np.minimum(rng.poisson(0.8, size=(rows, cols)), 255).astype(np.uint8)
    x[rng.rand(rows, cols) < 0.05] = 255
    x[rng.rand(rows, cols) < 0.05] = 128
    x[rng.rand(rows, cols) < 0.05] = 127
    return x


def test_value_boundaries_symmetric_and_cross():
    """rows constant at 0, 1, 127, 128, 255 plus random rows, 33 x 257"""
    rng = np.random.RandomState(1)
    x = rng.randint(0, 256, (33, 257)).astype(np.uint8)
    for i, v in enumerate((0, 1, 127, 128, 255)):
        x[i] = v
    y = np.ascontiguousarray(x[::-1][:20])
    a, b = _dev(x), _dev(y, lead=3)
    _same(_call(a), _ref(x))
    _same(_call(a, b), _ref(x, y))
    _same(_call(b, a), _ref(y, x))


def test_asymmetric_operands_show_a_swapped_or_mis_mapped_tile():
    """a = 17 rows, row i constant i + 1; b = 35 rows, row j constant (2 j + 3) mod 251; cols = 65: a transposed, swapped
    or permuted C/D tile shows.  Some of these products coincide ((i + 1)(2 j + 3) is not injective), so the same is
    repeated with b's rows constant at the 35 primes from 19 on, where every gram[i][j] is distinct, and on random data."""
    cols = 65
    x = np.repeat((np.arange(17) + 1).astype(np.uint8)[:, None], cols, 1)
    y = np.repeat(((2 * np.arange(35) + 3) % 251).astype(np.uint8)[:, None], cols, 1)
    _same(_call(_dev(x), _dev(y, lead=2)), _ref(x, y))
    primes = [p for p in range(19, 256) if all(p % q for q in range(2, 16))][:35]
    y = np.repeat(np.array(primes, np.uint8)[:, None], cols, 1)
    want = _ref(x, y)
    assert len(primes) == 35 and len(np.unique(want[0])) == 17 * 35
    _same(_call(_dev(x), _dev(y, lead=2)), want)
    x, y = _random(17, cols, 2), _random(35, cols, 3)
    _same(_call(_dev(x), _dev(y, lead=2)), _ref(x, y))


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 130])
def test_shapes_and_pitches(rows, cols):
    x, y = _random(rows, cols, rows + cols), _random(max(rows - 3, 1), cols, rows * cols)
    sym, cross = _ref(x), _ref(x, y)
    for extra in (0, 37):                                   # row_stride == cols and row_stride > cols
        a, b = _dev(x, 1, extra), _dev(y, 5, extra)
        _same(_call(a), sym)
        _same(_call(a, b), cross)
    got = _call(a, b, sums=False)                           # sums not wanted
    assert np.array_equal(got[0], cross[0]) and got[1] is None and got[2] is None


@pytest.mark.parametrize("lead_b", [1, 8, 15, 128 - 15, 127])
@pytest.mark.parametrize("lead_a", [1, 8, 15, 128 - 15, 127])
def test_every_alignment_of_both_operands(lead_a, lead_b):
    """base addresses at 1, 8 and 15 mod 16 and in the last 15 bytes of a 128-byte line, independently; the bytes
    around the rows are 255, so a read of a neighbour shows in the sums"""
    x, y = _random(17, 333, lead_a), _random(19, 333, 100 + lead_b)
    a, b = _dev(x, lead_a, 0), _dev(y, lead_b, 21)
    assert a.data_ptr() % 128 == lead_a and b.data_ptr() % 128 == lead_b
    _same(_call(a, b), _ref(x, y))
    _same(_call(a), _ref(x))


@pytest.mark.parametrize("kind", ["zero", "full", "mixed"])
def test_more_columns_than_an_int32_accumulator_holds(kind):
    """18 x (131072 + 65): more columns than an int32 accumulator could sum in one go (z = x XOR 0x80 is -128 for x = 0, so
    the all-zero matrix is the worst case), so the result is right only if the columns are cut into runs and each run is
    widened.  With one tile the layout cuts them into 33 runs of ONE slice: no accumulator holds more than 2^26 here.
    Runs of full length, 2^30 in an accumulator, are
    tests/test_gpu_gram_tiles.py::test_the_shipped_regime_full_runs_many_tiles_worst_case_values."""
    rows, cols = 18, 131072 + 65
    assert layout(rows, rows, cols, 1)[5] >= 3              # at least three runs of K slices
    assert layout(rows, rows, cols, 1)[4:6] == [1, 33]      # (of one slice each)
    if kind == "mixed":
        x = _random(rows, cols, 9)
        x[0], x[1], x[2, ::2] = 0, 255, 0
    else:
        x = np.full((rows, cols), 0 if kind == "zero" else 255, np.uint8)
    want = _ref(x)
    a = _dev(x)
    _same(_call(a), want)
    _same(_call(a, a), want)


def test_a_grid_past_its_cap_walks_every_run():
    """more runs than the grid has workgroups: every workgroup takes a second item, and the column offsets pass 2^31.
    The matrix is a short pattern repeated, so the expected integers follow from the pattern's own product."""
    rows, P = 18, 4099
    cols = MAX_BLOCKS * SLICE * RUN_SLICES + SLICE + 65
    lay = layout(rows, rows, cols, 1)
    assert lay[6] > lay[7] == MAX_BLOCKS and cols > 2 ** 27
    pat = _random(rows, P, 4)
    pat[0], pat[1] = 0, 255
    reps, tail = cols // P, cols % P
    x = torch.from_numpy(pat).cuda().repeat(1, reps + 1)[:, :cols]
    assert x.stride(1) == 1 and x.stride(0) >= cols
    full, part = _ref(pat), _ref(pat[:, :tail])
    want = tuple(reps * f + p for f, p in zip(full, part))
    _same(_call(x), want)
    del x
    torch.cuda.empty_cache()


def test_accumulate_adds_and_overwrite_cleans_a_poisoned_output():
    x, y = _random(40, 9000, 5), _random(23, 9000, 6)
    a, b = _dev(x), _dev(y)
    want = _ref(x, y)
    out = torch.full((40, 32), 2 ** 62 + 12345, dtype=torch.int64, device="cuda")[:, :23]     # a pitched result
    sa = torch.full((40,), -99, dtype=torch.int64, device="cuda")
    sb = torch.full((23,), 2 ** 40, dtype=torch.int64, device="cuda")
    _same(_call(a, b, out, sa, sb, accumulate=False), want)
    assert (out._base[:, 23:] == 2 ** 62 + 12345).all()      # nothing outside the rows is touched
    # two halves of the columns, the second added to the first
    h = 4500 - 13
    _call(a[:, :h], b[:, :h], out, sa, sb, accumulate=False)
    _same(_call(a[:, h:], b[:, h:], out, sa, sb, accumulate=True), want)
    # the symmetric form likewise
    g = torch.zeros((40, 40), dtype=torch.int64, device="cuda")
    s = torch.zeros((40,), dtype=torch.int64, device="cuda")
    _call(a[:, :h], None, g, s, None, accumulate=True)
    got = _call(a[:, h:], None, g, s, None, accumulate=True)
    assert np.array_equal(got[0], _ref(x)[0]) and np.array_equal(got[1], _ref(x)[1])


def test_the_symmetric_form_is_the_cross_form_with_b_equal_a():
    x = _random(300, 2000, 7)
    a = _dev(x)
    sym, cross = _call(a), _call(a, a)
    _same(sym, cross)
    assert np.array_equal(sym[0], sym[0].T) and np.array_equal(sym[1], sym[2])
    _same(sym, _ref(x))


def test_lags_against_numpy():
    x, y = _random(20, 1000, 8), _random(7, 1000, 9)
    dx, dy = _dev(x), _dev(y)
    lags = [0, 1, 7, 64]
    for yy, dyy in ((None, None), (y, dy)):
        res = gram.gram(dx, dyy, lag=lags)
        other = x if yy is None else yy
        assert res.n == [1000 - lg for lg in lags] and tuple(res.gram.shape) == (4, 20, other.shape[0])
        for k, lg in enumerate(lags):
            want = _ref(x[:, :1000 - lg], other[:, lg:])
            _same((res.gram[k].cpu().numpy(), res.sum_a[k].cpu().numpy(), res.sum_b[k].cpu().numpy()), want)
        one = gram.gram(dx, dyy, lag=7)
        assert one.n == 993 and torch.equal(one.gram, res.gram[2]) and not one.symmetric
    sym = gram.gram(dx)
    assert sym.symmetric and sym.n == 1000
    _same((sym.gram.cpu().numpy(), sym.sum_a.cpu().numpy(), sym.sum_b.cpu().numpy()), _ref(x))
    with pytest.raises(ValueError):
        gram.gram(dx, lag=1000)
    with pytest.raises(ValueError):
        gram.gram(dx, dy[:, :999])


def test_cov_and_corr_against_numpy_on_the_exact_integers():
    """Both sides evaluate (G - s_a s_b^T / n) / (n - ddof) step by step in float64 from the same exact integers (all
    below 2^53 here); every step is correctly rounded on both, so only a contraction into an fma can differ: per element
    within tol = 4 * 2^-53 * (|G_ij| + |s_i s_j| / n) / (n - ddof).  corr = c_ij / sqrt(c_ii c_jj) with c at ddof = 0
    inherits tol_ij / d from its numerator and |corr| * (tol_ii / c_ii + tol_jj / c_jj) from d = sqrt(c_ii c_jj) (twice
    the first-order term of the square root), plus 4 * 2^-53 |corr| for the product, the root and the quotient."""
    x = _random(50, 20000, 10)
    x[3] = 9                                                                 # a row without variance
    res = gram.gram(_dev(x))
    G, s, _ = _ref(x)
    n, u = 20000, 2.0 ** -53
    Gf, sf = G.astype(np.float64), s.astype(np.float64)
    assert np.array_equal(Gf.astype(np.int64), G)
    outer = sf[:, None] * sf[None, :]
    for ddof in (1, 0):
        want = (Gf - outer / n) / (n - ddof)
        tol = 4 * u * (np.abs(Gf) + np.abs(outer) / n) / (n - ddof)
        got = res.cov(ddof=ddof).cpu().numpy()
        assert got.dtype == np.float64 and (np.abs(got - want) <= tol).all()
    d = np.diag(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(d[:, None] * d[None, :])
        corr = np.where(den > 0, want / den, np.nan)
        ctol = tol / den + np.abs(corr) * (np.diag(tol) / d)[:, None] + np.abs(corr) * (np.diag(tol) / d)[None, :] + 4 * u * np.abs(corr)
    got = res.corr().cpu().numpy()
    ok = np.isfinite(corr)
    assert d[3] == 0 and np.isnan(got[3]).all() and np.isnan(got[:, 3]).all() and np.array_equal(np.isnan(got), ~ok)
    assert (np.abs(got[ok] - corr[ok]) <= ctol[ok]).all()
    m = res.mean()[0].cpu().numpy()
    assert np.array_equal(m, sf / n)


def test_the_call_is_ordered_on_the_current_stream_and_host_tensors_are_refused():
    x = _random(16, 200000, 11)
    src = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        buf = torch.zeros((16, 200000), dtype=torch.uint8, device="cuda")
        for _ in range(3):                      # the producer: the last copy is what the product must see
            buf.copy_(src ^ 0xFF)
        buf.copy_(src)
        res = gram.gram(buf)
    side.synchronize()
    _same((res.gram.cpu().numpy(), res.sum_a.cpu().numpy(), res.sum_b.cpu().numpy()), _ref(x))
    with pytest.raises(ValueError, match="no CPU path"):
        gram.gram(torch.from_numpy(x))
    with pytest.raises(ValueError):
        gram.gram(src.to(torch.int32))


def test_captured_calls_replay_on_other_contents():
    """mhi_gram only enqueues -- memset nodes and one kernel --: the pitched cross form (the 2-D memset node) and the
    symmetric form, overwriting, are captured once on a side stream and replayed on three other contents of the same
    input buffers, gram and sums poisoned in between; an accumulate = 1 call replayed twice on a zeroed result gives
    twice the product.  3 x 2 tiles, both last tiles ragged."""
    ra, rb, cols = 260, 129, 200
    a, b = _dev(_random(ra, cols, 30)), _dev(_random(rb, cols, 31), lead=3)
    base = torch.zeros((ra, rb + 3), dtype=torch.int64, device="cuda")
    out, sym = base[:, :rb], torch.zeros((ra, ra), dtype=torch.int64, device="cuda")
    acc = torch.zeros((ra, rb), dtype=torch.int64, device="cuda")
    sums = [torch.zeros((n,), dtype=torch.int64, device="cuda") for n in (ra, rb, ra, ra, ra, rb)]
    targets = [base, sym] + sums[:4]

    def calls(add):
        if add:
            _ingest.gram(a.data_ptr(), a.stride(0), ra, b.data_ptr(), b.stride(0), rb, cols, acc, sums[4], sums[5], True)
        else:
            _ingest.gram(a.data_ptr(), a.stride(0), ra, b.data_ptr(), b.stride(0), rb, cols, out, sums[0], sums[1], False)
            _ingest.gram(a.data_ptr(), a.stride(0), ra, None, 0, 0, cols, sym, sums[2], sums[3], False)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        calls(False), calls(True)                           # warm: the module is loaded
    side.synchronize()
    g, g_add = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls(False)
    with torch.cuda.graph(g_add, stream=side):
        calls(True)
    for seed in (32, 34, 36):
        x, y = _random(ra, cols, seed), _random(rb, cols, seed + 1)
        with torch.cuda.stream(side):
            a.copy_(torch.from_numpy(x).cuda()), b.copy_(torch.from_numpy(y).cuda())
            for t in targets:
                t.fill_(2 ** 62 + 12345)
            g.replay()
        side.synchronize()
        _same((out.cpu().numpy(), sums[0].cpu().numpy(), sums[1].cpu().numpy()), _ref(x, y))
        _same((sym.cpu().numpy(), sums[2].cpu().numpy(), sums[3].cpu().numpy()), _ref(x))
        assert (base[:, rb:] == 2 ** 62 + 12345).all()      # the 2-D memset node keeps to the rows
    with torch.cuda.stream(side):
        for t in (acc, sums[4], sums[5]):
            t.zero_()
        g_add.replay()
        g_add.replay()
    side.synchronize()
    _same((acc.cpu().numpy(), sums[4].cpu().numpy(), sums[5].cpu().numpy()), tuple(2 * w for w in _ref(x, y)))
