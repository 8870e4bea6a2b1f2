"""The LSTM decoder on the device (include/muahuff_lstm.h, muahuff.lstm): mhl_inproj against a float64 matmul, mhl_windows
against the oracle's recurrence on a given p, the saturating case, predict end to end against the oracle on explicit
z-scored windows, identical bits on a second call, at a column offset, at any max_bytes and from a BinSource, both calls
captured into one graph, and fit / cross_validate.  Every comparison with the float64 oracle is held to 16 x D_LSTM_F32
(tests/test_host_lstm.py: the error of float32 torch.nn.LSTM on the CPU over the same cases) of the largest value of the
case; every test prints its figure before it asserts.

As measured on an MI355X (bound 16 x 2.0e-6 = 3.2e-5): mhl_inproj 3.6e-8 .. 3.8e-7 of the largest |p|; mhl_windows
3.1e-8 .. 4.9e-7 of the largest |out|, and 6.2e-6 in case 5, one window of 32 steps at 128 units whose |out| is 0.02; the
saturating case 3.9e-7; predict at 96 x 3000 4.5e-7; the device against the trained module's own float32 forward 2.4e-7."""
import numpy as np
import pytest
import torch

from muahuff import _lstm, lstm, wiener
from muahuff.gram import BinSource
from tests import lstm_oracle as lo
from tests.test_host_lstm import CASES, D_LSTM_F32, IN_TILE, case_inputs, case_reference

pytestmark = pytest.mark.gpu

BOUND = 16 * D_LSTM_F32


def _dev(x, lead=1, extra=37):
    """the matrix as a pitched device view whose first byte sits at `lead` mod 128, every byte around the rows 255"""
    rows, cols = x.shape
    pitch = cols + extra
    buf = torch.full((rows * pitch + lead + 256,), 255, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 128 == 0
    view = buf.as_strided((rows, cols), (pitch, 1), lead)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    return view


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _decoder(i):
    C, T, L, U, K, clip, _silent, _scale = CASES[i]
    x, w, mean, std = case_inputs(i)
    return lstm.LSTMDecoder(U, L, 0, clip).set_weights(*w, mean, std), x


# ---- mhl_inproj ----------------------------------------------------------------------------------------------------------
# (rows, units, cols, clip, byte offset of x, pitched): rows 1, 2, 3 (an odd channel pair), 33, 96, 130; units 1, 7, 32, 33,
# 100, 128 (one g-tile, its edge, many); cols 1, a tile - 1, a tile, a tile + 1, three tiles + 5; clip 1, 3, 255; x at byte
# offsets 1..3 and with pitched rows
INPROJ_CASES = [
    (1, 1, 1, 1, 0, False),
    (2, 7, IN_TILE - 1, 3, 1, False),
    (3, 32, IN_TILE, 255, 2, True),
    (33, 33, IN_TILE + 1, 3, 3, True),
    (96, 100, 3 * IN_TILE + 5, 3, 0, False),
    (130, 128, 3 * IN_TILE + 5, 255, 1, True),
    (3, 7, 5, 1, 3, False),
    (2, 128, IN_TILE + 1, 1, 2, True),
]


def _inproj(xv, wx, bias, clip):
    rows, cols = xv.shape
    G = wx.shape[0]
    buf = torch.full((cols * G + 64,), float("nan"), dtype=torch.float32, device="cuda")
    p = buf[32:32 + cols * G].view(cols, G)
    _lstm.inproj(xv.data_ptr(), xv.stride(0) if rows > 1 else cols, rows, cols, clip, _cuda(wx), _cuda(bias), p)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:32]).all() and torch.isnan(buf[32 + cols * G:]).all()      # nothing around p was written
    return p


@pytest.mark.parametrize("case", INPROJ_CASES, ids=str)
def test_inproj_against_a_float64_matmul(case):
    rows, U, cols, clip, off, pitched = case
    rng = np.random.RandomState(rows * 1000 + U)
    x = np.minimum(rng.poisson(1.5, size=(rows, cols)), 255).astype(np.uint8)
    x[rng.rand(rows, cols) < 0.05] = 255
    wx = (rng.uniform(-1, 1, (4 * U, rows)) / np.sqrt(rows)).astype(np.float32)
    bias = rng.randn(4 * U).astype(np.float32)
    xv = _dev(x, lead=off, extra=37 if pitched else 0)
    assert xv.data_ptr() % 4 == off
    p = _inproj(xv, wx, bias, clip)
    ref = np.minimum(x, clip).astype(np.float64).T @ wx.astype(np.float64).T + bias.astype(np.float64)
    err = np.abs(p.cpu().numpy() - ref).max() / np.abs(ref).max()
    print("inproj %s: %.2e of the largest |p| %.3g (bound %.1e)" % (case, err, np.abs(ref).max(), BOUND))
    assert err <= BOUND
    assert torch.equal(_bits(_inproj(xv, wx, bias, clip)), _bits(p))                   # two calls, identical bits
    # a column's bits depend on the column alone: the same columns from an offset that is no multiple of a tile or a dword
    a = min(cols - 1, 131)
    if a > 0:
        tail = _inproj(xv[:, a:], wx, bias, clip)
        assert torch.equal(_bits(tail), _bits(p[a:]))


# ---- mhl_windows ---------------------------------------------------------------------------------------------------------
def _given_p(i):
    """the pre-activations of case i as a given float32 p: the float64 matmul of the folded weights, rounded once"""
    d, x = _decoder(i)
    wx, b, wh, wd, bd = d.folded()
    q = np.minimum(x, CASES[i][5]).astype(np.float64)
    return d, (q.T @ wx.astype(np.float64).T + b.astype(np.float64)).astype(np.float32), (wh, wd, bd)


def _windows(p, L, wh, wd, bd, pitched):
    K, n = wd.shape[0], p.shape[0] - L + 1
    pitch = n + (5 if pitched else 0)
    buf = torch.full((K * pitch + 16,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf.as_strided((K, n), (pitch, 1), 3)
    _lstm.windows(_cuda(p), L, _cuda(wh), _cuda(wd), _cuda(bd), out)
    torch.cuda.synchronize()
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask.as_strided((K, n), (pitch, 1), 3).fill_(False)
    assert torch.isnan(buf[mask]).all()                                                # nothing but the K x n values was written
    return out


@pytest.mark.parametrize("i", range(1, len(CASES)))
def test_windows_against_the_oracle_on_a_given_p(i):
    C, T, L, U, K, clip, _silent, _scale = CASES[i]
    d, p, (wh, wd, bd) = _given_p(i)
    w = d.get_weights()
    ref = lo.recurrence(p, L, w[1], w[3], w[4])
    out = _windows(p, L, wh, wd, bd, pitched=i % 2 == 0)
    got = out.cpu().numpy()
    assert got.shape == (K, T - L + 1) and np.isfinite(got).all()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("windows case %d (U %d, L %d, K %d, %d windows): %.2e of the largest |out| %.3g (bound %.1e)" % (i, U, L, K, T - L + 1, err, np.abs(ref).max(), BOUND))
    assert err <= BOUND
    assert torch.equal(_bits(_windows(p, L, wh, wd, bd, pitched=i % 2 == 1)), _bits(out))   # two calls, another pitch: identical bits


def test_saturation():
    """case 9: pre-activations past +-100 -- every output finite and, end to end, within the same bound"""
    d, p, (wh, wd, bd) = _given_p(9)
    assert np.abs(p).max() >= 100
    out = d.predict(_dev(case_inputs(9)[0])).cpu().numpy()
    ref = case_reference(9)
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print("saturating case: |p| up to %.0f, %.2e of the largest |out| %.3g (bound %.1e)" % (np.abs(p).max(), err, np.abs(ref).max(), BOUND))
    assert np.isfinite(out).all() and err <= BOUND
    # far past any exponent: p = +-3e38 and +-inf still give finite outputs inside the dense layer's reach
    big = np.where(np.arange(p.size).reshape(p.shape) % 3 == 0, -1.0, 1.0).astype(np.float32) * np.float32(3e38)
    big[::2] = np.sign(big[::2]) * np.float32(np.inf)
    out = _windows(big, CASES[9][2], wh, wd, bd, pitched=False).cpu().numpy()
    assert np.isfinite(out).all() and (np.abs(out) <= np.abs(wd).sum(1, keepdims=True) + np.abs(bd)[:, None] + 1e-6).all()


# ---- predict -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main():
    """case 0 on the device: (decoder, x as a pitched view at an odd address, predict(x)), shared and never written to"""
    d, x = _decoder(0)
    xv = _dev(x, lead=3)
    return d, x, xv, d.predict(xv)


def test_predict_end_to_end_against_the_oracle(main):
    d, x, xv, pred = main
    C, T, L, U, K, clip, silent, _scale = CASES[0]
    ref = case_reference(0)
    got = pred.cpu().numpy()
    assert (C, T, L, U, K, clip) == (96, 3000, 15, 100, 2, 3) and (x[silent] == x[silent, 0]).all()
    assert pred.dtype == torch.float32 and got.shape == (K, T - L + 1) and np.isfinite(got).all()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("predict 96 x 3000, L 15, U 100, K 2, clip 3: %.2e of the largest |out| %.3g (bound %.1e)" % (err, np.abs(ref).max(), BOUND))
    assert err <= BOUND
    y = torch.from_numpy(lo.target(x, L, 0, K, 4)).cuda()
    rmse, cc = d.score(xv, y)
    t = y[:, L - 1:].double().cpu().numpy()
    assert np.allclose(rmse.cpu().numpy(), np.sqrt(((got - t) ** 2).mean(1)), rtol=1e-6)
    assert np.allclose(cc.cpu().numpy(), [np.corrcoef(got[j], t[j])[0, 1] for j in range(K)], rtol=1e-6, atol=1e-9)


def test_predict_is_deterministic_and_does_not_depend_on_tiles_or_batches(main):
    d, x, xv, pred = main
    C, T, L, U, K, clip, _silent, _scale = CASES[0]
    assert torch.equal(_bits(d.predict(xv)), _bits(pred))                              # two calls
    a = 77                                                                            # no multiple of 4, 32, 128 or 512
    assert torch.equal(_bits(d.predict(xv[:, a:])), _bits(pred[:, a:]))
    small = _lstm.inproj_bytes(T, U) // 3 - 1000                                       # at least three batches
    per = small // _lstm.inproj_bytes(1, U) - (L - 1)
    assert -(-(T - L + 1) // per) >= 3 and per % 32 != 0
    assert torch.equal(_bits(d.predict(xv, max_bytes=small)), _bits(pred))
    src = BinSource.of(xv, max_bytes=C * 700)                                          # five batches of the source
    assert torch.equal(_bits(d.predict_from(src)), _bits(pred))
    y = torch.from_numpy(lo.target(x, L, 0, K, 4)).cuda()
    r0, c0 = d.score(xv, y)
    r1, c1 = d.score_from(BinSource.of(xv, max_bytes=C * 700), y)
    assert torch.equal(r0, r1) and torch.equal(c0, c1)


def test_predict_past_the_grid_caps():
    """more (column tile, g-tile) items than mhl_inproj's grid and more window tiles than mhl_windows' grid: the stride loops.
    Held bit for bit against batches that stay under both caps, and against the oracle at both ends."""
    U, L, K, C = 1, 2, 1, 2
    T = _lstm.IN_MAX_BLOCKS * _lstm.IN_TILE_COLS + 1
    assert -(-T // _lstm.IN_TILE_COLS) * 1 > _lstm.IN_MAX_BLOCKS and -(-(T - L + 1) // _lstm.WIN_TILE) > _lstm.WIN_MAX_BLOCKS
    g = torch.Generator(device="cuda").manual_seed(3)
    xd = torch.poisson(torch.full((C, T), 1.2, device="cuda"), generator=g).clamp_(max=255).to(torch.uint8)
    w = lo.weights(C, U, K, 31)
    d = lstm.LSTMDecoder(U, L, 0, 3).set_weights(*w, np.array([1.0, 1.2]), np.array([0.9, 1.1]))
    pred = d.predict(xd)
    per = 100000
    assert per <= _lstm.WIN_MAX_BLOCKS * _lstm.WIN_TILE and per + L - 1 <= _lstm.IN_MAX_BLOCKS * _lstm.IN_TILE_COLS
    assert torch.equal(_bits(d.predict(xd, max_bytes=(per + L - 1) * _lstm.inproj_bytes(1, U))), _bits(pred))
    for sl in (slice(0, 1500), slice(T - 1500, T)):
        ref = lo.predict(xd[:, sl].cpu().numpy(), L, 3, *d.get_weights())
        got = pred[:, sl.start:sl.stop - L + 1].cpu().numpy()
        assert np.abs(got - ref).max() <= BOUND * np.abs(ref).max()


def test_both_calls_in_one_graph(main):
    d, x, xv, pred = main
    C, T, L, U, K, clip, _silent, _scale = CASES[0]
    wx, b, wh, wd, bd = d._device(xv.device)
    p = torch.empty((T, 4 * U), dtype=torch.float32, device="cuda")
    out = torch.empty((K, T - L + 1), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                         # (a first run outside the capture)
        _lstm.inproj(xv.data_ptr(), xv.stride(0), C, T, clip, wx, b, p)
        _lstm.windows(p, L, wh, wd, bd, out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(pred))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                          # a serial chain of two kernels
        _lstm.inproj(xv.data_ptr(), xv.stride(0), C, T, clip, wx, b, p)
        _lstm.windows(p, L, wh, wd, bd, out)
    p.fill_(float("nan")), out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(pred))


# ---- fit -----------------------------------------------------------------------------------------------------------------
def test_fit_trains_and_the_device_predicts_what_the_module_computes():
    C, T, U, L, K = 8, 2000, 8, 5, 2
    x = lo.counts(C, T, 7)
    y = lo.target(x, L, 0, K, 8)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    d = lstm.LSTMDecoder(U, L, 0, 3)
    res = d.fit(xd, yd, ranges=[(L - 1, 1500)], valid=(1500, T), epochs=3, batch_size=32, seed=1)
    print("fit 8 x 2000, U 8, L 5: training loss %s, validation loss %s" % (np.round(res["loss_train"], 4), np.round(res["loss_valid"], 4)))
    assert len(res["loss_train"]) == len(res["loss_valid"]) == 3 and np.isfinite(res["loss_train"] + res["loss_valid"]).all()
    assert res["loss_train"][-1] < res["loss_train"][0]
    assert res["num_params"] == 4 * U * (C + U + 1) + K * (U + 1) == d.num_params()
    # mean and std are those of the clipped counts over the training rows; y's training mean went into dense_bias
    q = np.minimum(x, 3).astype(np.float64)[:, L - 1:1500]
    w = d.get_weights()
    assert np.allclose(w[5], q.mean(1), rtol=1e-12) and np.allclose(w[6], q.std(1), rtol=1e-9)
    # the trained torch module's own forward on explicit float32 windows, against the device
    m, lin = d.module
    u = torch.from_numpy(lo.input_shaping(lo.zscore(x, 3, w[5], w[6]), L, 1)).float().cuda()
    with torch.no_grad(), lstm.own_kernels():
        hs, _ = m(u)
        own = (lin(hs[:, -1]).double().t() + torch.from_numpy(y[:, L - 1:1500].astype(np.float64).mean(1)).cuda().unsqueeze(1)).cpu().numpy()
    got = d.predict(xd).cpu().numpy()
    err = np.abs(got - own).max() / np.abs(own).max()
    print("fit: the device and the module differ by %.2e of the largest |out| %.3g (bound %.1e)" % (err, np.abs(own).max(), BOUND))
    assert err <= BOUND
    # and against the oracle on the exported weights
    ref = lo.predict(x, L, 3, *w)
    assert np.abs(got - ref).max() <= BOUND * np.abs(ref).max()
    # the validation loss is the reference's loss of the device prediction
    v = got[:, 1500 - (L - 1):] - y[:, 1500:]
    assert np.isclose(res["loss_valid"][-1], np.sqrt((v ** 2).mean(0)).mean(), rtol=1e-5)


def test_cross_validate_returns_four_finite_arrays():
    C, T, U, L, K, folds = 8, 2000, 8, 5, 2, 5
    x = lo.counts(C, T, 7)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(lo.target(x, L, 1, K, 8)).cuda()
    res = lstm.cross_validate(xd, yd, L, lead=1, clip=3, num_fold=folds, units=U, epochs=1, batch_size=64, seed=2)
    assert sorted(res) == ["cc_test", "cc_valid", "rmse_test", "rmse_valid"]
    for k, v in res.items():
        assert v.shape == (folds, K) and v.dtype == torch.float64 and bool(torch.isfinite(v).all()), k
    assert len(wiener.folds(xd, folds, L, 1)) == folds
