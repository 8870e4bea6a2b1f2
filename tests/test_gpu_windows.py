"""mhi_windows on the GPU (include/muahuff_ingest.h, csrc/mh_windows.hpp): every form -- a lane per 16 samples (r == 1), a
staged tile with a lane per bin (2 <= r <= 64), a wave per bin (r > 64) -- stacked and summed, against a NumPy cut of the
same matrix, exactly.  The matrix is a pitched view that starts at an odd byte with a pitch that is no multiple of 16;
the outputs are written into canary-framed buffers with strides of their own and compared whole."""
import itertools

import numpy as np
import pytest
import torch

from muahuff import _ingest, windows

pytestmark = pytest.mark.gpu

COLS, LEAD = 40003, 1
STACK, SUM = _ingest.WIN_STACK, _ingest.WIN_SUM
CANARY = 0xA5
MAX_BLOCKS = 4096          # mh_windows_layout.hpp: kWinMaxBlocks, workgroups of 256 lanes (r == 1) or 4 waves


def _matrix(rows, cols=COLS, seed=3):
    rng = np.random.RandomState(seed + rows)
    rec = np.minimum(rng.poisson(0.8, size=(rows, cols)), 255).astype(np.uint8)
    rec[rng.rand(rows, cols) < 0.02] = 255
    for i in range(rows):                                  # runs of 255: sums past every saturation
        a = int(rng.randint(0, cols - 600))
        rec[i, a:a + 1 + int(rng.randint(1, 600))] = 255
    pitch = cols + 37
    buf = torch.full((rows * pitch + LEAD + 64,), 77, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((rows, cols), (pitch, 1), LEAD)
    view.copy_(torch.from_numpy(rec).cuda())
    assert view.data_ptr() % 2 == 1 and pitch % 16
    return rec, view


@pytest.fixture(scope="module")
def mats():
    return {rows: _matrix(rows) for rows in (1, 3, 70)}


def _ref(rec, offs, W, r):
    """int64 [n, rows, nb]: bin b of window k = sum of rec[:, offs[k] + b*r : offs[k] + min(b*r + r, W)]"""
    nb = -(-W // r)
    g = rec[:, np.asarray(offs, np.int64)[:, None] + np.arange(W)]                   # [rows, n, W]
    g = np.concatenate([g, np.zeros(g.shape[:2] + (nb * r - W,), np.uint8)], axis=2)
    return g.reshape(g.shape[0], g.shape[1], nb, r).sum(axis=3, dtype=np.int64).transpose(1, 0, 2)


def _starts(n, W, cols, seed):
    """every residue mod 16, identical and overlapping windows, one that ends exactly at cols"""
    rng = np.random.RandomState(seed)
    top = cols - W
    o = rng.randint(0, top + 1, n).astype(np.int64)
    o = np.minimum(o - o % 16 + np.arange(n) % 16, top)
    if n > 1:
        o[1] = o[0]
    if n > 2:
        o[2] = min(o[0] + 1, top)
    o[-1] = top
    return o


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _framed(nbytes):
    return torch.full((nbytes + 64,), CANARY, dtype=torch.uint8, device="cuda")


def _run_stack(x, offs, idx, n_out, W, r, bits):
    """-> (what the whole framed buffer holds, a function that lays an [n_out, rows, nb] array out the same way, bad)"""
    rows, cols = x.shape
    nb, e = -(-W // r), bits // 8
    rs = nb * e + (4 if e == 4 else 3)                 # a row pitch of its own
    ws = rows * rs + (8 if e == 4 else 5)
    lead = 8 if e == 4 else 3
    buf = _framed(lead + n_out * ws)
    bad = _ingest.verify_state("cuda")
    _ingest.windows(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, cols, _dev(offs), None if idx is None else _dev(idx),
                    n_out, W, r, STACK, buf.data_ptr() + lead, bits, ws, rs, bad)
    got = buf.cpu().numpy()

    def lay(stack, written):
        want = np.full(got.shape, CANARY, np.uint8)
        for s in range(n_out):
            if not written[s]:
                continue
            for i in range(rows):
                o = lead + s * ws + i * rs
                want[o:o + nb * e] = stack[s, i].astype("<u4" if e == 4 else np.uint8).view(np.uint8)
        return want
    return got, lay, bad.cpu().numpy()


def _run_sum(x, offs, W, r, sq, add=False, into=None):
    rows, cols = x.shape
    nb = -(-W // r)
    rs, qs = 4 * (nb + 1), 8 * (nb + 3)
    out, sumsq = into if into is not None else (_framed(8 + rows * rs), _framed(16 + rows * qs) if sq else None)
    bad = _ingest.verify_state("cuda")
    _ingest.windows(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, cols, _dev(offs), None, 0, W, r, SUM,
                    out.data_ptr() + 8, 32, 0, rs, bad, sumsq[16:] if sq else None, qs, add, n_win=len(offs))

    def lay(total, squares):
        a = np.full(out.numel(), CANARY, np.uint8)
        b = np.full(sumsq.numel(), CANARY, np.uint8) if sq else None
        for i in range(rows):
            a[8 + i * rs:8 + i * rs + 4 * nb] = total[i].astype("<u4").view(np.uint8)
            if sq:
                b[16 + i * qs:16 + i * qs + 8 * nb] = squares[i].astype("<u8").view(np.uint8)
        return a, b
    return (out, sumsq), lay, bad.cpu().numpy()


WS = (1, 15, 16, 17, 64, 1000, 4099)
PAIRS = sorted({(W, r) for W in WS for r in (1, 2, 3, 5, 16, 50, 64, 65, 4096, W, W + 1)})
_rows, _nwin = itertools.cycle((1, 3, 70)), itertools.cycle((1, 7, 8, 9, 300, 5))
SHAPES = []
for W, r in PAIRS:
    rows, n = next(_rows), next(_nwin)
    if rows * n * W > 2 * 10 ** 7:
        rows = 3
    SHAPES.append((rows, W, r, n))
# every form with every row count and with n_win on both sides of the SUM owners' unroll of 4
SHAPES += [(70, 4099, 1, 9), (70, 1000, 50, 300), (70, 1000, 65, 9), (1, 4099, 2, 300), (3, 4099, 4096, 8), (70, 17, 3, 300)]


def test_the_shapes_cross_every_form_switch():
    rs = {r for _rows, _W, r, _n in SHAPES}
    assert {1, 2, 64, 65} <= rs and {n for *_x, n in SHAPES} >= {1, 7, 8, 9, 300}
    assert {rows for rows, *_x in SHAPES} == {1, 3, 70}
    assert any(W % r and r < W for _rows, W, r, _n in SHAPES)                # a cut last bin
    assert any(r > W for _rows, W, r, _n in SHAPES)


@pytest.mark.parametrize("rows,W,r,n", SHAPES, ids=lambda v: str(v))
def test_stack_and_sum_against_numpy(mats, rows, W, r, n):
    rec, x = mats[rows]
    offs = _starts(n, W, COLS, W * 131 + r)
    want = _ref(rec, offs, W, r)
    assert offs[-1] + W == COLS and (n < 16 or len(set((offs % 16).tolist())) == 16)
    # STACK: 8-bit saturating in the caller's order, 32-bit exact through a permuting win_idx
    got, lay, bad = _run_stack(x, offs, None, n, W, r, 8)
    assert np.array_equal(got, lay(np.minimum(want, 255), [True] * n)) and bad.tolist() == [0, -1]
    perm = np.random.RandomState(n).permutation(n + 2)[:n]                   # n_out = n + 2: two slots stay untouched
    got, lay, bad = _run_stack(x, offs, perm, n + 2, W, r, 32)
    placed = np.zeros((n + 2,) + want.shape[1:], np.int64)
    placed[perm] = want
    assert np.array_equal(got, lay(placed, np.isin(np.arange(n + 2), perm))) and bad.tolist() == [0, -1]
    # SUM: without and with the squares; two accumulating calls equal one
    total, squares = want.sum(axis=0), (want * want).sum(axis=0)
    (out, _none), lay, bad = _run_sum(x, offs, W, r, False)
    assert np.array_equal(out.cpu().numpy(), lay(total, None)[0]) and bad.tolist() == [0, -1]
    bufs, lay, bad = _run_sum(x, offs, W, r, True)
    a, b = lay(total, squares)
    assert np.array_equal(bufs[0].cpu().numpy(), a) and np.array_equal(bufs[1].cpu().numpy(), b) and bad.tolist() == [0, -1]
    if n > 1:
        h = n // 2
        two, lay, _bad = _run_sum(x, offs[:h], W, r, True)
        _run_sum(x, offs[h:], W, r, True, add=True, into=two)
        assert np.array_equal(two[0].cpu().numpy(), a) and np.array_equal(two[1].cpu().numpy(), b)


def test_no_windows():
    rec, x = _matrix(3, 700)
    none = np.zeros(0, np.int64)
    got, lay, bad = _run_stack(x, none, None, 4, 10, 2, 8)
    assert (got == CANARY).all() and bad.tolist() == [0, -1]                 # STACK: nothing is enqueued
    bufs, lay, bad = _run_sum(x, none, 10, 2, True)
    a, b = lay(np.zeros((3, 5), np.int64), np.zeros((3, 5), np.int64))       # SUM: zero-filled
    assert np.array_equal(bufs[0].cpu().numpy(), a) and np.array_equal(bufs[1].cpu().numpy(), b)
    assert windows.gather(x, [], 10, 2).shape == (0, 3, 5)
    assert not windows.psth(x, [], 10, 2).any()


@pytest.mark.parametrize("W,r", [(33, 1), (33, 5), (330, 100)])
def test_bad_windows_are_skipped_and_counted(mats, W, r):
    rec, x = mats[3]
    offs = _starts(12, W, COLS, 9)
    offs[[4, 7, 10]] = [COLS - W + 1, 2 ** 63 - 1, -5]                       # past the end, sums that wrap, "negative"
    idx = np.arange(12)
    idx[9] = 12                                                              # a slot >= n_out
    ok = np.ones(12, bool)
    ok[[4, 7, 10, 9]] = False
    want = np.zeros((12, 3, -(-W // r)), np.int64)
    want[ok] = _ref(rec, offs[ok], W, r)
    got, lay, bad = _run_stack(x, offs, idx, 12, W, r, 8)
    assert bad.tolist() == [4, 4] and np.array_equal(got, lay(np.minimum(want, 255), ok))
    ok[9] = True                                                             # SUM has no slots: window 9 counts
    want[9] = _ref(rec, offs[9:10], W, r)[0]
    bufs, lay, bad = _run_sum(x, offs, W, r, True)
    a, b = lay(want[ok].sum(axis=0), (want[ok] ** 2).sum(axis=0))
    assert bad.tolist() == [3, 4] and np.array_equal(bufs[0].cpu().numpy(), a) and np.array_equal(bufs[1].cpu().numpy(), b)
    # the device-tensor level reads the counter: device offsets are checked by the kernel
    with pytest.raises(ValueError, match="first is window 4"):
        windows.gather(x, _dev(offs), W, r)
    with pytest.raises(ValueError, match="first is window 4"):
        windows.psth(x, _dev(offs), W, r)
    with pytest.raises(ValueError, match="window 4: offset %d" % (COLS - W + 1)):
        windows.gather(x, offs, W, r)


# ---- the capped grid: 4096 workgroups, then item += gridDim.x * (256 lanes or 4 waves) ---------------------------------
@pytest.mark.parametrize("W,r,n,per", [(1, 1, 15000, 256), (17, 2, 300, 4), (700, 100, 40, 4)])
def test_stack_of_more_items_than_the_capped_grid_holds(mats, W, r, n, per):
    rec, x = mats[70]
    nb = -(-W // r)
    tiles = -(-W // 16) if r == 1 else -(-nb // (1024 // r)) if r <= 64 else nb
    assert n * 70 * tiles > MAX_BLOCKS * per                                 # a second trip of the stride loop
    offs = _starts(n, W, COLS, 21)
    got = windows.gather(x, offs, W, r, saturate=False).cpu().numpy()
    assert np.array_equal(got, _ref(rec, offs, W, r))


@pytest.fixture(scope="module")
def tall():
    return _matrix(17000, 1100)


@pytest.mark.parametrize("W,r,per", [(1000, 1, 256), (17, 2, 4), (66, 65, 4)])
def test_sum_of_more_items_than_the_capped_grid_holds(tall, W, r, per):
    rec, x = tall
    nb = -(-W // r)
    tiles = -(-W // 16) if r == 1 else -(-nb // (1024 // r)) if r <= 64 else nb
    assert 17000 * tiles > MAX_BLOCKS * per
    offs = np.array([3, 1100 - W])
    want = _ref(rec, offs, W, r)
    s, q = windows.psth(x, offs, W, r, moments=2)
    assert s.dtype == torch.int32 and q.dtype == torch.int64
    assert np.array_equal(s.cpu().numpy(), want.sum(axis=0)) and np.array_equal(q.cpu().numpy(), (want ** 2).sum(axis=0))


# ---- the device-tensor level -------------------------------------------------------------------------------------------
def test_gather_and_psth(mats):
    from muahuff.container import ChannelSet
    rec, x = mats[3]
    offs = _starts(40, 100, COLS, 4)
    want = _ref(rec, offs, 100, 7)
    g8, g32 = windows.gather(x, offs, 100, 7), windows.gather(x, _dev(offs), 100, 7, saturate=False)
    assert g8.dtype == torch.uint8 and g32.dtype == torch.int32 and tuple(g8.shape) == (40, 3, 15)
    assert np.array_equal(g8.cpu().numpy(), np.minimum(want, 255)) and np.array_equal(g32.cpu().numpy(), want)
    assert np.array_equal(windows.gather(x, offs, 100).cpu().numpy(), _ref(rec, offs, 100, 1))
    assert np.array_equal(windows.psth(x, offs, 100, 7).cpu().numpy(), want.sum(axis=0))
    sl = x[1:, 50:5000]                                                      # a column slice of a row slice
    assert np.array_equal(windows.psth(sl, [0, 4850], 100, 7).cpu().numpy(), _ref(rec[1:, 50:5000], [0, 4850], 100, 7).sum(axis=0))
    cs = ChannelSet.from_channels([rec[i, :3000] for i in range(3)])
    assert np.array_equal(windows.gather(cs, [5, 2900], 100, 7).cpu().numpy(), np.minimum(_ref(rec[:, :3000], [5, 2900], 100, 7), 255))
    with pytest.raises(ValueError, match="int32"):
        windows.psth(x, np.zeros(90000, np.int64), 100, 100)
    with pytest.raises(ValueError):
        windows.gather(x.t(), offs, 100)
    with pytest.raises(ValueError):
        windows.gather(x, offs, 0)


def test_a_captured_call_replays(mats):
    """mhi_windows only enqueues: captured once, replayed on other offsets in the same buffers"""
    rec, x = mats[3]
    W, r, n = 200, 7, 50
    nb = -(-W // r)
    off = torch.zeros(n, dtype=torch.int64, device="cuda")
    out = torch.zeros((3, nb), dtype=torch.int32, device="cuda")
    sq = torch.zeros((3, nb), dtype=torch.int64, device="cuda")
    bad = _ingest.verify_state("cuda")
    side = torch.cuda.Stream()
    first = _starts(n, W, COLS, 1)
    with torch.cuda.stream(side):
        off.copy_(_dev(first))
        windows.accumulate(x, 3, COLS, off, W, r, out, sq, False, bad)       # warm: the module is loaded
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        windows.accumulate(x, 3, COLS, off, W, r, out, sq, False, bad)
    second = _starts(n, W, COLS, 2)
    with torch.cuda.stream(side):
        off.copy_(_dev(second))
        g.replay()
    side.synchronize()
    want = _ref(rec, second, W, r)
    assert not np.array_equal(first, second)
    assert np.array_equal(out.cpu().numpy(), want.sum(axis=0)) and np.array_equal(sq.cpu().numpy(), (want ** 2).sum(axis=0))
    assert bad.cpu().tolist() == [0, -1]
