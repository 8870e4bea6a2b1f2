"""The five decoder libraries with row strides and columns beyond 4 GiB: the cases of tests/far_decoders.py on the device,
run as tests/test_gpu_far_offsets.py runs its own -- the windows of a case's `pre` image (around every true region and
around every alias, where a term cut to 32 bits would land) are uploaded into an arena that is otherwise never touched, the
call is made with direct ctypes calls on the arena's base pointer, and every window is downloaded and compared WHOLE with
the `post` image.  tests/test_host_far_decoders.py shows without a GPU that no address of any case, cut or not, leaves the
arena.

Then the far column over the whole length, for the five calls that always walk [0, cols): one row, one output, the far
operand is the arena itself, filled and compared on the device in chunks of 2^26 columns from a pattern of the column
number, so no temporary of the arena's size exists.  Each of them states the free HBM it asks for (far_decoders.WHOLE).

Last, the Python layer: wiener.stats, WienerFilter.predict and kalman.KalmanFilter.predict on a view of the arena whose two
channels lie 2^32 + 4099 bytes apart give the bits they give on a compact tensor.

One arena of 2^32 + 2^28 bytes at a time; the second buffer of mhs_box_f32's whole-length case and the double arena of
mhk_scan's k = 2 far column are allocated by their tests alone and freed there."""
import ctypes as ct

import numpy as np
import pytest
import torch

from tests import far_decoders as fd
from tests import far_offsets as fo
from tests.test_gpu_far_offsets import Ctx as _Ctx
from tests.test_gpu_far_offsets import _need

pytestmark = pytest.mark.gpu

_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
          np.dtype(np.int64): torch.int64}


class Ctx(_Ctx):
    """the Ctx of tests/test_gpu_far_offsets.py with the five decoder libraries"""

    def __init__(self, mh, arena):
        super().__init__(mh, arena)
        self.wlib, self.clib, self.slib = mh._wiener.lib(), mh._cascade.lib(), mh._smooth.lib()
        self.qlib, self.klib = mh._sweep.lib(), mh._kalman.lib()

    def canary(self, n, dtype):
        t = torch.full((n * np.dtype(dtype).itemsize,), fo.CANARY, dtype=torch.uint8, device="cuda").view(_TORCH[np.dtype(dtype)])
        self.keep.append(t)
        return t


@pytest.fixture(scope="module")
def mh():
    import muahuff
    from muahuff import _cascade, _kalman, _smooth, _sweep, _wiener, kalman, wiener  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    return muahuff


@pytest.fixture(scope="module")
def arena(mh):
    """2^32 + 2^28 bytes, never filled as a whole but by the whole-length cases"""
    _need(fo.ARENA_BYTES + fo.HEADROOM, "the arena of 2^32 + 2^28 bytes (+ 2 GiB for the small tensors)")
    a = torch.empty(fo.ARENA_BYTES, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


def run_case(mh, arena, case):
    s = case.setup()
    assert arena.dtype == torch.uint8 and arena.numel() == s.pre.size
    for lo, buf, _mark in s.pre.wins:
        arena[lo:lo + buf.size].copy_(torch.from_numpy(buf))
    ctx = Ctx(mh, arena)
    torch.cuda.synchronize()
    s.run(ctx)
    torch.cuda.synchronize()
    assert len(s.post.wins) == len(s.pre.wins)
    for lo, exp, _mark in s.post.wins:
        got = arena[lo:lo + exp.size].cpu().numpy()
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            i = int(bad[0])
            pytest.fail("%s: window [%#x, %#x): %d bytes differ, the first at %#x: got %#x, want %#x"
                        % (case.id, lo, lo + exp.size, bad.size, lo + i, int(got[i]), int(exp[i])))


def _row(row):
    cases = [c for c in fd.CASES if c.row == row]
    assert cases, row
    return pytest.mark.parametrize("case", cases, ids=[c.id for c in cases])


@_row("xty")
def test_xty(mh, arena, case):
    run_case(mh, arena, case)


@_row("fir")
def test_fir(mh, arena, case):
    run_case(mh, arena, case)


@_row("moments")
def test_moments(mh, arena, case):
    run_case(mh, arena, case)


@_row("polyval")
def test_polyval(mh, arena, case):
    run_case(mh, arena, case)


@_row("box_f32")
def test_box_f32(mh, arena, case):
    run_case(mh, arena, case)


@_row("box")
def test_box_far_products(mh, arena, case):
    run_case(mh, arena, case)


@_row("gram_clips")
def test_gram_clips_far_product(mh, arena, case):
    run_case(mh, arena, case)


@_row("xty_clips")
def test_xty_clips(mh, arena, case):
    run_case(mh, arena, case)


@_row("project")
def test_project(mh, arena, case):
    run_case(mh, arena, case)


@_row("scan")
def test_scan(mh, arena, case):
    run_case(mh, arena, case)


# ---- through the Python layer -------------------------------------------------------------------------------------------
PY_T, PY_STRIDE, PY_FIRST = 3000, fo.FAR + 4099, 13


def _far_view(arena, x):
    """x [2, T] as a view of the arena whose channels lie 2^32 + 4099 bytes apart; at the alias of channel 1 lies its
    complement -> (the view, the compact tensor, the compact tensor with the decoy for channel 1)"""
    assert x.shape == (2, PY_T) and PY_T + 16 < 4099 and PY_FIRST + PY_STRIDE + PY_T + 8 <= fo.ARENA_BYTES
    decoy = 255 - x[1]
    for off, row in ((PY_FIRST, x[0]), (PY_FIRST + 4099, decoy), (PY_FIRST + PY_STRIDE, x[1])):
        arena[off - 8:off + PY_T + 8] = 255
        arena[off:off + PY_T] = torch.from_numpy(row).cuda()
    view = arena.as_strided((2, PY_T), (PY_STRIDE, 1), PY_FIRST)
    return view, torch.from_numpy(x).cuda(), torch.from_numpy(np.stack([x[0], decoy])).cuda()


def _world(seed):
    """two channels of counts that follow two slow covariates"""
    rng = np.random.RandomState(seed)
    t = np.arange(PY_T)
    y = np.stack([np.sin(t / 37.0) + 0.3 * rng.randn(PY_T), np.cos(t / 53.0) + 0.3 * rng.randn(PY_T)]).astype(np.float32)
    x = np.minimum(rng.poisson(np.exp(0.8 * y + 0.5)), 255).astype(np.uint8)
    return x, torch.from_numpy(y).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


STATS_FIELDS = ("sum_x", "gram", "xty", "sum_y", "sum_yy")


@pytest.mark.parametrize("clip,window", [(None, 1), (4, 1), (4, 5)])
def test_wiener_stats_on_a_view_with_far_channels(mh, arena, clip, window):
    from muahuff import wiener
    x, y = _world(1)
    view, compact, decoyed = _far_view(arena, x)
    ranges = [(4, 1500), (1500, PY_T - 2)]
    far, near, other = (wiener.stats(v, y, 5, 2, clip, ranges, window=window) for v in (view, compact, decoyed))
    for f, n, o in zip(far, near, other):
        assert f.n == n.n
        for name in STATS_FIELDS:
            assert torch.equal(_bits(getattr(f, name)), _bits(getattr(n, name))), name
        assert not torch.equal(f.gram, o.gram) and not torch.equal(f.xty, o.xty)      # the decoy would have shown


def test_wiener_predict_on_a_view_with_far_channels(mh, arena):
    from muahuff import wiener
    x, y = _world(2)
    view, compact, decoyed = _far_view(arena, x)
    for clip, window in ((None, 1), (4, 5)):
        f = wiener.WienerFilter(1e-2).fit(wiener.stats(compact, y, 5, 2, clip, window=window))
        far, near = f.predict(view), f.predict(compact)
        assert far.dtype == torch.float32 and tuple(far.shape) == (2, PY_T - 4)
        assert torch.equal(_bits(far), _bits(near))
        assert not torch.equal(_bits(far), _bits(f.predict(decoyed)))


def test_kalman_predict_on_a_view_with_far_channels(mh, arena):
    from muahuff import kalman
    x, y = _world(3)
    view, compact, decoyed = _far_view(arena, x)
    f = kalman.KalmanFilter(1e-2).fit(kalman.stats(compact, y, 0, 4))
    for ranges in (None, [(5, 700), (700, 700 + 2 * fd.SCAN_TILE + 9), (2000, PY_T)]):
        far, near = f.predict(view, None, ranges), f.predict(compact, None, ranges)
        inside = torch.isfinite(near[0])
        assert far.dtype == torch.float64 and tuple(far.shape) == (2, PY_T) and bool(inside.any())
        assert torch.equal(_bits(far[:, inside]), _bits(near[:, inside])) and bool(torch.isnan(far[:, ~inside]).all())
        assert not torch.equal(_bits(far[:, inside]), _bits(f.predict(decoyed, None, ranges)[:, inside]))


# ---- the far column over the whole length ------------------------------------------------------------------------------
def _cols(t0, t1):
    return torch.arange(t0, t1, dtype=torch.int64, device="cuda")


def _mix(t, mod, salt=0):
    """a pattern 0 .. mod - 1 of the column number t (int64, below 2^31) that does not repeat 2^29 or 2^30 columns later: the
    last two terms see to that whatever the modulus; every whole-length test asserts it of its own data"""
    return ((((t + salt) * 2654435761 + (t >> 9) * 40503) >> 5) + (t >> 29) * 3 + (t >> 30)) % mod


def _chunks(cols):
    for t0 in range(0, cols, fd.WHOLE_CHUNK):
        yield t0, min(t0 + fd.WHOLE_CHUNK, cols)


def _whole(entry, arena, dtype):
    """the shape of an entry point's whole-length case, its free HBM checked, the arena as `dtype` with canary behind the
    last column -> (cols, the view)"""
    cols, elem, need, what = fd.WHOLE[entry]
    _need(need - fo.ARENA_BYTES, "%s over %d columns (the arena is there; %s)" % (entry, cols, what))
    view = arena.view(dtype)
    assert view.element_size() == elem and cols * elem >= fo.FAR and cols <= view.numel()
    arena[cols * elem:] = fo.CANARY
    return cols, view


def _tail_is_canary(arena, cols, elem):
    assert bool((arena[cols * elem:] == fo.CANARY).all()), "the tail of the arena behind the last column was written"


def _ends_differ(f, cols, n):
    """the data f(t0, t1) of the last n columns -- those past 2^32 bytes -- is not the data of the first n, which is where a
    byte offset cut to 32 bits would look for them"""
    assert (cols - n) * 4 in (fo.FAR, fo.FAR // 2) and not torch.equal(f(0, n), f(cols - n, cols))


def _counts_whole(n, salt):
    """a uint8 row of n counts 0..4 from the pattern"""
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    for t0, t1 in _chunks(n):
        x[t0:t1] = _mix(_cols(t0, t1), 5, salt).to(torch.uint8)
    return x


def _framed64(out, body, tag):
    got = out.cpu().numpy().view(np.uint8)
    exp = np.full(got.size, fo.CANARY, np.uint8)
    exp[8:8 + 8 * body.size] = fo.as_bytes(body)
    assert np.array_equal(got, exp), (tag, out.cpu().numpy(), body)


def test_xty_over_the_whole_length(mh, arena):
    """y is the arena: 2^30 + a run + 77 columns of dyadic covariates; every product and sum is exact"""
    cols, y = _whole("mhw_xty", arena, torch.float32)
    lags, clip = 2, 3
    lib = mh._wiener.lib()
    x = _counts_whole(cols + lags - 1, 11)
    yi = lambda t0, t1: _mix(_cols(t0, t1), 8193, 77) - 4096      # noqa: E731   y = yi / 64
    want = np.zeros((lags, 1, 1), np.float64)
    sums = [0] * lags
    for t0, t1 in _chunks(cols):
        v = yi(t0, t1)
        y[t0:t1] = (v.double() / 64.0).float()
        for l in range(lags):
            xq = torch.clamp(x[t0 + lags - 1 - l:t1 + lags - 1 - l], max=clip).long()
            sums[l] += int((xq * v).sum())
    n = fd.XTY_RUN + 77
    _ends_differ(yi, cols, n)
    assert not torch.equal(x[:n], x[cols - n:cols])
    for l in range(lags):
        assert abs(sums[l]) < 1 << 53
        want[l, 0, 0] = sums[l] / 64.0
    need = ct.c_uint64(0)
    assert lib.mhw_xty_scratch_bytes(1, cols, lags, 1, ct.byref(need)) == 0
    out = torch.full((8 * (lags + 2),), fo.CANARY, dtype=torch.uint8, device="cuda").view(torch.float64)
    scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    rc = lib.mhw_xty(x.data_ptr(), 0, 1, cols, lags, clip, y.data_ptr(), 0, 1, out.data_ptr() + 8, 0, scratch.data_ptr(), scratch.numel(), None)
    assert rc == 0, lib.mhw_last_error()
    torch.cuda.synchronize()
    _framed64(out, want, "mhw_xty")
    _tail_is_canary(arena, cols, 4)


def test_fir_over_the_whole_length(mh, arena):
    """out is the arena: 2^30 + a workgroup tile + 79 outputs of an integer filter"""
    arena.fill_(fo.CANARY)
    cols, out = _whole("mhw_fir", arena, torch.float32)
    lags, clip = 2, 3
    lib = mh._wiener.lib()
    x = _counts_whole(cols + lags - 1, 12)
    w = torch.tensor([3.0, -2.0], dtype=torch.float32, device="cuda")         # lag 0 takes x[i + 1], lag 1 takes x[i]
    bias = torch.tensor([5.0], dtype=torch.float32, device="cuda")
    rc = lib.mhw_fir(x.data_ptr(), 0, 1, cols, lags, clip, w.data_ptr(), bias.data_ptr(), 1, out.data_ptr(), 0, None)
    assert rc == 0, lib.mhw_last_error()
    torch.cuda.synchronize()
    want = lambda t0, t1: 3.0 * torch.clamp(x[t0 + 1:t1 + 1], max=clip).float() - 2.0 * torch.clamp(x[t0:t1], max=clip).float() + 5.0   # noqa: E731
    _ends_differ(want, cols, fd.FIR_TILE - 1 + 79)
    for t0, t1 in _chunks(cols):
        assert torch.equal(out[t0:t1], want(t0, t1)), (t0, t1)
    _tail_is_canary(arena, cols, 4)


def test_polyval_over_the_whole_length_in_place(mh, arena):
    """p and out are the arena: 2^30 + a tile + 5 columns of small integers through an integer polynomial"""
    cols, p = _whole("mhc_polyval", arena, torch.float32)
    lib = mh._cascade.lib()
    src = lambda t0, t1: (_mix(_cols(t0, t1), 7, 13) - 3).float()             # noqa: E731
    for t0, t1 in _chunks(cols):
        p[t0:t1] = src(t0, t1)
    coef = torch.tensor([2.0, -3.0, 1.0], dtype=torch.float32, device="cuda")
    center, inv = torch.tensor([1.0], dtype=torch.float32, device="cuda"), torch.tensor([2.0], dtype=torch.float32, device="cuda")
    rc = lib.mhc_polyval(p.data_ptr(), 0, 1, cols, coef.data_ptr(), 2, center.data_ptr(), inv.data_ptr(), p.data_ptr(), 0, None)
    assert rc == 0, lib.mhc_last_error()
    torch.cuda.synchronize()

    def want(t0, t1):
        u = (src(t0, t1) - 1.0) * 2.0
        return (2.0 * u - 3.0) * u + 1.0                           # integers below 2^24: exact however it is rounded
    _ends_differ(want, cols, fd.POLY_TILE + 5)
    for t0, t1 in _chunks(cols):
        assert torch.equal(p[t0:t1], want(t0, t1)), (t0, t1)
    _tail_is_canary(arena, cols, 4)


def test_box_f32_over_the_whole_length(mh, arena):
    """out is the arena, in a second buffer of the same size: 2^30 + a tile + 5 columns of integers, window 2"""
    arena.fill_(fo.CANARY)
    cols, out = _whole("mhs_box_f32", arena, torch.float32)
    lib = mh._smooth.lib()
    src = lambda t0, t1: (_mix(_cols(t0, t1), 2001, 14) - 1000).float()       # noqa: E731
    inp = torch.empty(fd.ARENA_F32, dtype=torch.float32, device="cuda")
    try:
        for t0, t1 in _chunks(cols):
            inp[t0:t1] = src(t0, t1)
        bias = torch.tensor([7.0], dtype=torch.float32, device="cuda")
        rc = lib.mhs_box_f32(inp.data_ptr(), 0, 1, cols, 2, bias.data_ptr(), out.data_ptr(), 0, None)
        assert rc == 0, lib.mhs_last_error()
        torch.cuda.synchronize()

        def want(t0, t1):
            before = src(max(t0 - 1, 0), t1 - 1)
            if t0 == 0:
                before = torch.cat([torch.zeros(1, dtype=torch.float32, device="cuda"), before])
            return src(t0, t1) + before + 7.0
        _ends_differ(want, cols, fd.BOXF_TILE + 5)
        for t0, t1 in _chunks(cols):
            assert torch.equal(out[t0:t1], want(t0, t1)), (t0, t1)
        _tail_is_canary(arena, cols, 4)
    finally:
        del inp
        torch.cuda.empty_cache()


def test_project_over_the_whole_length(mh, arena):
    """v is the arena as float64: 2^29 + a tile + 5 columns, one channel, one dyadic m"""
    arena.fill_(fo.CANARY)
    cols, v = _whole("mhk_project", arena, torch.float64)
    lib = mh._kalman.lib()
    clip = 3
    x = _counts_whole(cols, 15)
    m = torch.tensor([[1.5]], dtype=torch.float64, device="cuda")
    m0 = torch.tensor([-0.25], dtype=torch.float64, device="cuda")
    rc = lib.mhk_project(x.data_ptr(), 0, 1, cols, clip, m.data_ptr(), m0.data_ptr(), 1, v.data_ptr(), 0, None)
    assert rc == 0, lib.mhk_last_error()
    torch.cuda.synchronize()
    want = lambda t0, t1: 1.5 * torch.clamp(x[t0:t1], max=clip).double() - 0.25      # noqa: E731
    _ends_differ(want, cols, fd.PROJ_TILE + 5)
    for t0, t1 in _chunks(cols):
        assert torch.equal(v[t0:t1], want(t0, t1)), (t0, t1)
    _tail_is_canary(arena, cols, 8)


# ---- mhk_scan's far column with k = 2: an arena of its own, twice as long, last and freed here ------------------------
_SCAN2 = [c for c in fd.CASES if c.row == "scan2"]


@pytest.mark.parametrize("case", _SCAN2, ids=[c.id for c in _SCAN2])
def test_scan_far_column_with_two_rows(mh, case):
    _need(fd.ARENA2_BYTES + fo.HEADROOM, "two rows of the arena's length for mhk_scan with k = 2 (+ 2 GiB for the small tensors)")
    big = torch.empty(fd.ARENA2_BYTES, dtype=torch.uint8, device="cuda")
    try:
        run_case(mh, big, case)
    finally:
        del big
        torch.cuda.empty_cache()
