"""mhi_gram's geometry on the GPU (csrc/mh_gram.hpp on the layouts of csrc/mh_gram_layout.hpp): what the kernel does on
many tiles, on runs of full length and on columns past 2^32 -- the corners tests/test_gpu_gram.py does not reach.  Every
test first asserts, with tests/test_host_gram.py's layout(), the property of the layout it exists for, and compares int64
with int64: equal, never close.

  cross form with 3 x 2 and 2 x 3 tiles, both last tiles ragged        the t / ntb split of gram_owner
  symmetric form, 6 tile rows, pitched result                          the triangle walk to ti = 5, the mirror's pitch
  more items than workgroups with 15 tiles, runs of one slice          a workgroup's second item is another tile
  61 tile rows, 3 runs of 16 slices, worst-case values                 the shipped regime: 2^30 in an int32 accumulator
  one row of 2^32 + 4099 columns                                       the column offset k past 32 bits

The large inputs are a short pattern repeated or gathered on the device, and what is expected follows from the
pattern's own product on the host: nothing of the size of an input or of a result is built there.  A wrong kernel cannot
fault: no test has a stride term beyond 2^32, and a column offset cut to 32 bits re-reads the start of the same row."""
import numpy as np
import pytest
import torch

from muahuff import _ingest, gram
from tests.test_gpu_gram import _call, _dev, _random, _ref, _same
from tests.test_host_gram import MAX_BLOCKS, RUN_SLICES, SLICE, layout

pytestmark = pytest.mark.gpu

POISON = 2 ** 62 + 12345
NTA, NTB, TILES, SLICES, RUN, RUNS, ITEMS, GRID = range(8)       # the fields of layout()


def _need(nbytes, what):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    assert nbytes < free, "%s needs ~%.1f GB of free HBM; %.1f GB free" % (what, nbytes / 1e9, free / 1e9)


def _exact(x, y=None):
    """x y^T and the row sums as int64, through float64 where every sum is an integer below 2^53"""
    y = x if y is None else y
    assert x.shape[1] * 255 * 255 < 2 ** 53
    g = x.astype(np.float64) @ y.astype(np.float64).T
    return g.astype(np.int64), x.sum(1, dtype=np.int64), y.sum(1, dtype=np.int64)


def _poisoned(rows, cols, pad=0):
    base = torch.full((rows, cols + pad), POISON, dtype=torch.int64, device="cuda")
    return base, base[:, :cols]


def _sums(n):
    return torch.full((n,), POISON, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def cross():
    """a = 260 rows, b = 129 rows, 200 columns, every row distinct; the products both ways"""
    x, y = _random(260, 200, 21), _random(129, 200, 22)
    assert len({r.tobytes() for r in x}) == 260 and len({r.tobytes() for r in y}) == 129
    return x, y, _ref(x, y), _ref(y, x)


def test_cross_form_with_unequal_tile_counts_and_ragged_last_tiles(cross):
    """3 x 2 tiles one way and 2 x 3 the other, the last tile of a 4 rows and of b 1 row: tile t is (t / ntb, t % ntb),
    and a split by nta, a transposed pair or a store past a ragged tile shows on rows that are all distinct"""
    x, y, xy, yx = cross
    assert layout(260, 129, 200, 0)[:RUNS + 1] == [3, 2, 6, 1, 1, 1] and layout(129, 260, 200, 0)[:RUNS + 1] == [2, 3, 6, 1, 1, 1]
    assert 260 % 128 == 4 and 129 % 128 == 1
    a, b = _dev(x), _dev(y, lead=3)
    _same(_call(a, b), xy)
    _same(_call(b, a), yx)


def test_symmetric_form_walks_a_deep_triangle_into_a_pitched_result(cross):
    """643 rows: 6 tile rows, 21 tiles, the last one 3 x 3.  The result's rows are 8 * (643 + 5) bytes apart and
    poisoned: the mirror image goes through the pitch, the overwrite call zeroes through the 2-D memset, and the 5 pad
    elements of every row stay as they were.  Then sum_a = NULL with sum_b given, in both forms."""
    rows, cols, pad = 643, 130, 5
    lay = layout(rows, rows, cols, 1)
    assert lay[NTA] == 6 and lay[TILES] == 21 and lay[RUNS] == 1 and rows > 128
    x = _random(rows, cols, 23)
    want = _ref(x)
    a = _dev(x)
    base, out = _poisoned(rows, rows, pad)
    assert out.stride(0) == rows + pad
    sa, sb = _sums(rows), _sums(rows)
    got = _call(a, None, out, sa, sb)
    _same(got, want)
    assert np.array_equal(got[0], got[0].T)
    assert (base[:, rows:] == POISON).all()
    # sum_a = NULL, sum_b given: the symmetric form
    base, out = _poisoned(rows, rows, pad)
    sb = _sums(rows)
    got = _call(a, None, out, None, sb)
    assert got[1] is None
    _same((got[0], got[2]), (want[0], want[2]))
    assert (base[:, rows:] == POISON).all()
    # and the cross form, 3 x 2 tiles
    x, y, xy, _yx = cross
    base, out = _poisoned(260, 129, 3)
    sb = _sums(129)
    got = _call(_dev(x), _dev(y, lead=3), out, None, sb)
    assert got[1] is None
    _same((got[0], got[2]), (xy[0], xy[2]))
    assert (base[:, 129:] == POISON).all()


def test_a_strided_grid_hands_a_workgroup_another_tile():
    """515 rows x (139 * 4096 + 65) columns, symmetric: 15 tiles and 140 runs of one slice are 2100 items on 2048
    workgroups, so the second item of a workgroup is another tile of another run: its ti / tj and the row sums it leaves
    in LDS are not those of its first.  The matrix is a pattern of 4099 columns repeated."""
    rows, P = 515, 4099
    cols = 139 * SLICE + 65
    lay = layout(rows, rows, cols, 1)
    assert lay[TILES] == 15 and lay[RUN] == 1 and lay[ITEMS] == 2100 > lay[GRID] == MAX_BLOCKS
    assert (lay[GRID] % lay[TILES]) != 0                     # item and item + grid are different tiles
    _need(2 * rows * (cols + P) + (1 << 28), "a 515-row matrix of 569409 columns")
    pat = _random(rows, P, 24)
    pat[0], pat[1] = 0, 255
    reps, tail = cols // P, cols % P
    assert tail > 0
    x = torch.from_numpy(pat).cuda().repeat(1, reps + 1)[:, :cols]
    assert x.stride(1) == 1 and x.stride(0) >= cols
    full, part = _exact(pat), _exact(pat[:, :tail])
    want = tuple(reps * f + p for f, p in zip(full, part))
    got = _call(x)
    _same(got, want)
    assert np.array_equal(got[0], got[0].T)
    del x
    torch.cuda.empty_cache()


def test_the_shipped_regime_full_runs_many_tiles_worst_case_values():
    """7803 rows x 131137 columns, symmetric: 61 tile rows, 1891 tiles, runs of 16 slices (65536, 65536 and 65 columns),
    5673 items on 2048 workgroups.  Row i is pattern row i mod 131 (131 is prime and above the tile's 128 rows: no tile
    repeats another, none is uniform); the pattern's rows are all 0, all 255, 0 / 255 alternating, all 128, all 127 and
    random ones.  x = 0 is z = -128: the all-zero row against itself puts 65536 * 16384 = 2^30 into an int32 accumulator
    in every full run.  Expected: the pattern's own 131 x 131 product, gathered on the device.  Then the cross form of
    the matrix against its first 300 rows: 61 x 3 tiles, runs of 2 slices."""
    rows, cols, M = 7803, 131072 + 65, 131
    lay = layout(rows, rows, cols, 1)
    assert lay[:ITEMS + 1] == [61, 61, 1891, 33, RUN_SLICES, 3, 5673] and lay[ITEMS] > lay[GRID] == MAX_BLOCKS
    assert [min(cols, (r + 1) * RUN_SLICES * SLICE) - r * RUN_SLICES * SLICE for r in range(3)] == [65536, 65536, 65]
    assert RUN_SLICES * SLICE * (-128) * (-128) == 2 ** 30 < 2 ** 31 - 1          # what a full run of zeros accumulates
    clay = layout(rows, 300, cols, 0)
    assert clay[:ITEMS + 1] == [61, 3, 183, 33, 2, 17, 3111] and clay[ITEMS] > clay[GRID]
    _need(rows * cols + 3 * 8 * rows * rows + (1 << 28), "a 7803-row matrix of 131137 columns and its int64 result")
    pat = _random(M, cols, 25)
    pat[0], pat[1], pat[2], pat[3], pat[4] = 0, 255, 255, 128, 127
    pat[2, ::2] = 0
    gp, sp, _ = _exact(pat)
    assert gp[0, 0] == 0 and gp[1, 1] == cols * 255 * 255
    idx = torch.arange(rows, device="cuda") % M
    x = torch.from_numpy(pat).cuda()[idx]
    assert tuple(x.shape) == (rows, cols) and x.is_contiguous()
    d_gp, d_sp = torch.from_numpy(gp).cuda(), torch.from_numpy(sp).cuda()
    want = d_gp[idx[:, None], idx[None, :]]
    out = torch.full((rows, rows), -7, dtype=torch.int64, device="cuda")
    sa, sb = _sums(rows), _sums(rows)
    _ingest.gram(x.data_ptr(), cols, rows, None, 0, 0, cols, out, sa, sb, False)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(sa, d_sp[idx]) and torch.equal(sb, d_sp[idx])
    del out, want
    torch.cuda.empty_cache()
    out = torch.full((rows, 300), -7, dtype=torch.int64, device="cuda")
    sa, sb = _sums(rows), _sums(300)
    _ingest.gram(x.data_ptr(), cols, rows, x.data_ptr(), cols, 300, cols, out, sa, sb, False)
    torch.cuda.synchronize()
    assert torch.equal(out, d_gp[idx[:, None], idx[None, :300]])
    assert torch.equal(sa, d_sp[idx]) and torch.equal(sb, d_sp[idx[:300]])
    del x, out
    torch.cuda.empty_cache()


def _row_products(pat, head, n, lag):
    """sum over t < n of x[t] * x[t + lag] for the row x = pat repeated with its first bytes replaced by `head`"""
    P, H = pat.size, head.size
    p = pat.astype(np.int64)
    reps, tail = n // P, n % P
    prod = p * np.roll(p, -lag)                               # pat[u] * pat[(u + lag) % P]
    periodic = reps * int(prod.sum()) + int(prod[:tail].sum())
    xs = np.tile(p, 2)[:H + lag].copy()                       # the start of the row, before and after the patch
    ps = xs.copy()
    xs[:H] = head
    return periodic + int((xs[:H] * xs[lag:H + lag]).sum()) - int((ps[:H] * ps[lag:H + lag]).sum())


def _cut_row_products(pat, head, n, lag):
    """the same with the column offset k of every load cut to 32 bits: the columns from 2^32 on come from the row's start"""
    P, H, far = pat.size, head.size, 1 << 32
    m = n - far                                               # columns past 2^32
    assert 0 < m <= P and H + lag <= P
    p = pat.astype(np.int64)
    k = far + np.arange(m)
    true = int((p[k % P] * p[(k + lag) % P]).sum())
    start = np.tile(p, 2)[:m + lag].copy()
    start[:H] = head
    return _row_products(pat, head, n, lag) - true + int((start[:m] * start[lag:m + lag]).sum())


def test_columns_past_2_32():
    """One row of 2^32 + 4099 columns: 65537 runs of 16 slices, the column offset of the last one is 2^32.  The row is a
    pattern of 4099 bytes repeated on the device.  The columns past 2^32 are exactly one period, and a sum over one
    period does not tell where the period began: so the first 64 bytes of the row -- what the first step past 2^32
    would re-read if k were cut to 32 bits -- are replaced by 255.  Symmetric form (1 x 1 and the sum) and the cross form
    of the row against itself 7 bytes on; the expected integers follow from the pattern, and for both forms they
    differ from what a 32-bit k would give."""
    P, cols, lag = 4099, 2 ** 32 + 4099, 7
    lay = layout(1, 1, cols, 1)
    assert lay[TILES] == 1 and lay[RUN] == RUN_SLICES and lay[ITEMS] == 65537 and (lay[RUNS] - 1) * RUN_SLICES * SLICE == 2 ** 32
    assert layout(1, 1, cols - lag, 0)[ITEMS] == 65537
    pat = _random(1, P, 26)[0]
    head = np.full(64, 255, np.uint8)
    reps = cols // P
    want = {lg: _row_products(pat, head, cols - lg, lg) for lg in (0, lag)}
    for lg in (0, lag):
        assert want[lg] != _cut_row_products(pat, head, cols - lg, lg)
    s_all = reps * int(pat.sum(dtype=np.int64)) + int(pat[:cols % P].sum(dtype=np.int64)) + int(head.sum()) - int(pat[:64].sum())
    # the sums of the lagged call: a without its last 7 columns, b without its first 7
    last = np.array([pat[t % P] for t in range(cols - lag, cols)], np.int64)
    s_a, s_b = s_all - int(last.sum()), s_all - 7 * 255
    _need(cols + P + (1 << 28), "a row of 2^32 + 4099 columns")
    x = torch.from_numpy(pat).cuda().repeat(reps + 1)[:cols].unsqueeze(0)
    x[0, :64] = 255
    assert tuple(x.shape) == (1, cols) and x.stride(1) == 1
    sym = gram.gram(x)
    torch.cuda.synchronize()
    assert sym.symmetric and sym.n == cols
    assert sym.gram.cpu().tolist() == [[want[0]]] and sym.sum_a.cpu().tolist() == [s_all] and sym.sum_b.cpu().tolist() == [s_all]
    lagged = gram.gram(x, lag=lag)
    torch.cuda.synchronize()
    assert lagged.n == cols - lag and not lagged.symmetric
    assert lagged.gram.cpu().tolist() == [[want[lag]]] and lagged.sum_a.cpu().tolist() == [s_a] and lagged.sum_b.cpu().tolist() == [s_b]
    del x
    torch.cuda.empty_cache()
