"""The minibatch loss and gradient of the LSTM decoder on the device (include/muahuff_train.h, muahuff.lstm.loss_and_grad,
LSTMDecoder.fit(engine="device")): out, loss and the five gradients of every case of tests/test_host_train.py against the
float64 oracle (tests/lstm_grad_oracle.py), x a pitched view at byte offsets 1..3 with 255 around the rows, NaN around every
result and around the scratch; identical bits on a second call, at another place of the scratch and under graph replay; a
window's out, loss and dz rows whatever else is in the minibatch; more windows than the recurrence grids, more channel
tiles than the gradient grid and more row items than the projection grid have workgroups; a window of zero loss; and fit / cross_validate with engine="device".  A gradient is held to
16 x D_GRAD_F32 of its tensor's largest |entry|, out and loss to 16 x D_LSTM_F32 (the errors of float32 torch autograd on
the CPU over the same cases); every test prints its figures before it asserts.

As measured on an MI355X (bounds 16 x 4.0e-6 = 6.4e-5 for a gradient and 16 x 2.0e-6 = 3.2e-5 for out and loss): over the ten
cases out 1.4e-7 .. 4.8e-7, loss 2.7e-8 .. 7.8e-8, wx 1.4e-7 .. 1.7e-6, bias 2.7e-7 .. 1.8e-6, wh 1.6e-7 .. 1.9e-6 (the
saturating case has the largest of each), wd 1.3e-7 .. 5.7e-7, bd 0 .. 2.4e-7; a duplicated window 3e-8 .. 8e-8; 32 769
windows (65 538 rows in one chain) wx 2.7e-5, bias 1.6e-5, wh 5.9e-6, wd 8.4e-6, bd 1.9e-5, out 1.3e-7; 32 773 channels out
2.6e-6, wx 3.7e-6, wh 5.5e-6; 35 200 rows at U = 128 (4400 projection items) wx 7.1e-6, bias 7.7e-6, wh 8.3e-6; the first loss of
fit under the two engines 7.2e-9 apart.  The file takes 6.0 s."""
import numpy as np
import pytest
import torch

from muahuff import _train, lstm
from tests import lstm_grad_oracle as go
from tests import lstm_oracle as lo
from tests.test_host_lstm import D_LSTM_F32
from tests.test_host_train import CASES, D_GRAD_F32, GRADS, GRAD_MAX_BLOCKS, IN_MAX_BLOCKS, IN_ROWS, MAX_TILES, case_inputs, case_reference, rel

pytestmark = pytest.mark.gpu

BOUND_GRAD, BOUND_OUT = 16 * D_GRAD_F32, 16 * D_LSTM_F32


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


def _weights(w):
    """Keras layout, float64 numpy -> (wx [4U, C], bias, wh [4U, U], wd [K, U], bd), float32 device tensors"""
    kernel, rec, bias, dk, db = w
    return _cuda(kernel.T), _cuda(bias), _cuda(rec.T), _cuda(dk.T), _cuda(db)


class Arena:
    """the scratch and the seven results of one call inside ONE float32 buffer of NaN, 16 values apart (the scratch `shift`
    values further in)"""

    def __init__(self, C, K, B, L, U, shift=0):
        G = 4 * U
        self.sizes = dict(scratch=_train.scratch_layout(B, L, U)["floats"], out=K * B, loss=B, wx=G * C, bias=G, wh=G * U, wd=K * U, bd=K)
        self.shapes = dict(out=(K, B), loss=(B,), wx=(G, C), bias=(G,), wh=(G, U), wd=(K, U), bd=(K,))
        self.off, at = {}, 16 + shift
        for n, s in self.sizes.items():
            self.off[n] = at
            at += s + 16
        self.buf = torch.empty((at,), dtype=torch.float32, device="cuda")
        self.B, self.L, self.U = B, L, U
        self.fill()

    def fill(self):
        self.buf.fill_(float("nan"))

    def __getitem__(self, n):
        t = self.buf[self.off[n]:self.off[n] + self.sizes[n]]
        return t if n == "scratch" else t.view(self.shapes[n])

    def dz(self):
        o = _train.scratch_layout(self.B, self.L, self.U)["dz"]
        return self["scratch"][o:o + self.B * self.L * 4 * self.U].view(self.B, self.L, 4 * self.U)

    def nothing_else_was_written(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for n, s in self.sizes.items():
            mask[self.off[n]:self.off[n] + s] = False
            assert not bool(torch.isnan(self.buf[self.off[n]:self.off[n] + s]).any()), n     # every value of it was
        assert bool(torch.isnan(self.buf[mask]).all())


def _call(arena, xd, yd, idx, wt, mean, inv, L, lead, clip, scale):
    C, T = xd.shape
    _train.loss_grad(xd.data_ptr(), xd.stride(0) if C > 1 else T, C, T, clip, mean, inv, idx, L, lead, *wt, yd, scale, arena["scratch"],
                     arena["out"], arena["loss"], *[arena[n] for n in GRADS])


def _case(i, shift=0):
    C, T, L, U, K, clip, batch, lead, _silent, _scale = CASES[i]
    inp = case_inputs(i)
    xd, yd = _dev(inp["x"], 1 + i % 3), _cuda(inp["y"])
    idx = torch.from_numpy(inp["idx"]).cuda()
    wt = _weights(inp["w"])
    arena = Arena(C, K, batch, L, U, shift)
    args = (xd, yd, idx, wt, _cuda(inp["mean"]), _cuda(inp["inv"]), L, lead, clip)
    return arena, args, inp


@pytest.mark.parametrize("i", range(len(CASES)))
def test_out_loss_and_gradients_against_the_oracle(i):
    C, T, L, U, K, clip, batch, lead, silent, scale = CASES[i]
    arena, args, inp = _case(i)
    _call(arena, *args, 1.0 / batch)
    torch.cuda.synchronize()
    ref = case_reference(i)
    got = {n: arena[n].double().cpu().numpy() for n in ("out", "loss") + GRADS}
    errs = {n: rel(got[n], ref[n]) for n in got}
    print("case %d: " % i + ", ".join("%s %.2e" % (n, errs[n]) for n in errs) + " of the largest |entry| (bounds %.1e, %.1e)" % (BOUND_OUT, BOUND_GRAD))
    arena.nothing_else_was_written()
    assert all(np.isfinite(g).all() for g in got.values())
    for n in got:
        assert errs[n] <= (BOUND_OUT if n in ("out", "loss") else BOUND_GRAD), (n, errs[n])
    if L == 1:
        assert (got["wh"] == 0).all()                               # no recurrent product
    if silent is not None:
        assert (got["wx"][:, silent] == 0).all()
    # the public call: the same bits, from mean and std
    xd, yd, idx, wt = args[:4]
    out, loss, grads = lstm.loss_and_grad(xd, yd, idx, wt, inp["mean"], inp["std"], L, lead, clip)
    assert torch.equal(_bits(out), _bits(arena["out"])) and torch.equal(_bits(loss), _bits(arena["loss"]))
    assert list(grads) == list(GRADS) and all(torch.equal(_bits(grads[n]), _bits(arena[n])) for n in GRADS)


def test_two_calls_and_another_scratch_give_identical_bits():
    i = 3
    arena, args, _inp = _case(i)
    _call(arena, *args, 1.0 / CASES[i][6])
    first = arena.buf.clone()
    arena.fill()
    _call(arena, *args, 1.0 / CASES[i][6])
    assert torch.equal(_bits(first), _bits(arena.buf))              # NaN sentinels included: the same bits everywhere
    other, args2, _ = _case(i, shift=3)
    _call(other, *args2, 1.0 / CASES[i][6])
    for n in ("scratch", "out", "loss") + GRADS:
        assert torch.equal(_bits(other[n]), _bits(arena[n])), n
    other.nothing_else_was_written()


def test_a_window_does_not_depend_on_its_minibatch():
    i = 5
    C, T, L, U, K, clip, batch, lead, _s, _w = CASES[i]
    arena, args, _inp = _case(i)
    xd, yd, idx, wt, mean, inv = args[:6]
    scale = 1.0 / 7
    _call(arena, *args, scale)
    pick = torch.tensor([40, 3, 3, 69, 0, 33, 31, 32], device="cuda")
    small = Arena(C, K, len(pick), L, U)
    _call(small, xd, yd, idx[pick].contiguous(), wt, mean, inv, L, lead, clip, scale)
    assert torch.equal(_bits(small["out"]), _bits(arena["out"][:, pick])) and torch.equal(_bits(small["loss"]), _bits(arena["loss"][pick]))
    assert torch.equal(_bits(small.dz()), _bits(arena.dz()[pick]))
    small.nothing_else_was_written()
    # a duplicated window contributes twice: [a, b, b] - [a, b] is [b], at equal scale
    a, b = int(idx[40]), int(idx[3])
    res = []
    for ids in ([a, b, b], [a, b], [b]):
        ar = Arena(C, K, len(ids), L, U)
        _call(ar, xd, yd, torch.tensor(ids, device="cuda"), wt, mean, inv, L, lead, clip, scale)
        res.append({n: ar[n].double() for n in GRADS})
    for n in GRADS:
        top = float(res[0][n].abs().max())
        err = float((res[0][n] - res[1][n] - res[2][n]).abs().max()) / top
        print("twice: %s differs by %.2e of the largest |entry|" % (n, err))
        assert err <= BOUND_GRAD and float(res[2][n].abs().max()) > 1e-3 * top


def _small_problem(C, T, batch, seed):
    """U = 1, L = 2, K = 1: the cheapest shape"""
    rng = np.random.RandomState(seed)
    x = lo.counts(C, T, seed)
    w = lo.weights(C, 1, 1, seed + 1)
    mean = rng.uniform(1, 2, C).astype(np.float32).astype(np.float64)
    inv = rng.uniform(0.5, 1.5, C).astype(np.float32).astype(np.float64)
    y = rng.randn(1, T).astype(np.float32)
    idx = rng.randint(1, T, size=batch).astype(np.int64)
    idx[0], idx[-1] = T - 1, 1
    return x, w, mean, inv, y, idx


def test_more_window_tiles_than_the_recurrence_grids():
    C, T, L, U, K, clip = 2, 500, 2, 1, 1, 3
    B = 32 * MAX_TILES + 1
    x, w, mean, inv, y, idx = _small_problem(C, T, B, 11)
    xd, yd, wt, md, iv = _dev(x, 2), _cuda(y), _weights(w), _cuda(mean), _cuda(inv)
    idx_d = torch.from_numpy(idx).cuda()
    scale = 1.0 / B
    arena = Arena(C, K, B, L, U)
    _call(arena, xd, yd, idx_d, wt, md, iv, L, 0, clip, scale)
    arena.nothing_else_was_written()
    # per window: bit for bit against calls under the cap
    for lo_, hi in ((0, 32 * MAX_TILES), (32 * MAX_TILES - 70, B)):
        part = Arena(C, K, hi - lo_, L, U)
        _call(part, xd, yd, idx_d[lo_:hi], wt, md, iv, L, 0, clip, scale)
        assert torch.equal(_bits(part["out"]), _bits(arena["out"][:, lo_:hi])) and torch.equal(_bits(part["loss"]), _bits(arena["loss"][lo_:hi]))
        assert torch.equal(_bits(part.dz()), _bits(arena.dz()[lo_:hi]))
    u = go.gather(go.zscored(x, clip, mean, inv), idx, L)
    ref = go.loss_grad(u, y.astype(np.float64)[:, idx].T, *w, scale)
    for n in ("out", "loss") + GRADS:
        err = rel(arena[n].double().cpu().numpy(), ref[n])
        print("%d windows: %s differs by %.2e of the largest |entry|" % (B, n, err))
        assert err <= (BOUND_OUT if n in ("out", "loss") else BOUND_GRAD), n


def test_more_gradient_tiles_than_the_gradient_grid():
    C, T, L, U, K, clip, B = 32 * GRAD_MAX_BLOCKS + 5, 8, 2, 1, 1, 3, 3
    x, w, mean, inv, y, idx = _small_problem(C, T, B, 21)
    inv[7] = 0.0
    xd, yd, wt = _dev(x, 3, 5), _cuda(y), _weights(w)
    arena = Arena(C, K, B, L, U)
    _call(arena, xd, yd, torch.from_numpy(idx).cuda(), wt, _cuda(mean), _cuda(inv), L, 0, clip, 1.0 / B)
    arena.nothing_else_was_written()
    u = go.gather(go.zscored(x, clip, mean, inv), idx, L)
    ref = go.loss_grad(u, y.astype(np.float64)[:, idx].T, *w, 1.0 / B)
    for n in ("out", "loss") + GRADS:
        err = rel(arena[n].double().cpu().numpy(), ref[n])
        print("%d channels: %s differs by %.2e of the largest |entry|" % (C, n, err))
        assert err <= (BOUND_OUT if n in ("out", "loss") else BOUND_GRAD), n
    assert bool((arena["wx"][:, 7] == 0).all())


def test_more_input_items_than_the_projection_grid():
    """k_train_inproj's items are (128 rows, 32 pre-activations): U = 128 has 16 g-tiles, L = 32 the most rows per window"""
    C, T, L, U, K, clip, B = 2, 200, 32, 128, 1, 3, 1100
    assert -(-B * L // IN_ROWS) * (4 * U // 32) > IN_MAX_BLOCKS
    rng = np.random.RandomState(31)
    x, w = lo.counts(C, T, 31), lo.weights(C, U, K, 32)
    mean = rng.uniform(1, 2, C).astype(np.float32).astype(np.float64)
    inv = rng.uniform(0.5, 1.5, C).astype(np.float32).astype(np.float64)
    y = rng.randn(K, T).astype(np.float32)
    idx = rng.randint(L - 1, T, size=B).astype(np.int64)
    idx[0], idx[-1] = T - 1, L - 1
    arena = Arena(C, K, B, L, U)
    _call(arena, _dev(x, 1), _cuda(y), torch.from_numpy(idx).cuda(), _weights(w), _cuda(mean), _cuda(inv), L, 0, clip, 1.0 / B)
    arena.nothing_else_was_written()
    u = go.gather(go.zscored(x, clip, mean, inv), idx, L)
    ref = go.loss_grad(u, y.astype(np.float64)[:, idx].T, *w, 1.0 / B)
    for n in ("out", "loss") + GRADS:
        err = rel(arena[n].double().cpu().numpy(), ref[n])
        print("%d rows: %s differs by %.2e of the largest |entry|" % (B * L, n, err))
        assert err <= (BOUND_OUT if n in ("out", "loss") else BOUND_GRAD), n


def test_a_window_of_zero_loss_adds_a_zero_gradient():
    """the stated difference from autograd, which gives NaN there: the window's own out becomes its target"""
    i = 1
    C, T, L, U, K, clip, batch, lead, _s, _w = CASES[i]
    arena, args, inp = _case(i)
    xd, yd, idx, wt, mean, inv = args[:6]
    hit = 3
    assert int((inp["idx"] == inp["idx"][hit]).sum()) == 1        # no other window shares its target
    scale = 1.0 / batch
    _call(arena, *args, scale)
    y2 = yd.clone()
    y2[:, int(inp["idx"][hit]) + lead] = arena["out"][:, hit]
    zero = Arena(C, K, batch, L, U)
    _call(zero, xd, y2, idx, wt, mean, inv, L, lead, clip, scale)
    zero.nothing_else_was_written()
    assert float(zero["loss"][hit]) == 0.0 and bool((zero.dz()[hit] == 0).all())
    rest = torch.tensor([b for b in range(batch) if b != hit], device="cuda")
    without = Arena(C, K, batch - 1, L, U)
    _call(without, xd, y2, idx[rest].contiguous(), wt, mean, inv, L, lead, clip, scale)
    for n in GRADS:
        assert bool(torch.isfinite(zero[n]).all()) and torch.equal(zero[n], without[n]), n   # adding 0 changes no value


def test_the_call_replays_from_a_graph():
    i = 6
    arena, args, _inp = _case(i)
    scale = 1.0 / CASES[i][6]
    _call(arena, *args, scale)
    torch.cuda.synchronize()
    eager = arena.buf.clone()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _call(arena, *args, scale)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        arena.fill()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(arena.buf), _bits(eager))


def test_fit_on_the_device_trains_and_is_reproducible():
    C, T, U, L, K = 8, 2000, 8, 5, 2
    x = lo.counts(C, T, 7)
    y = lo.target(x, L, 0, K, 8)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    kw = dict(ranges=[(L - 1, 1500)], valid=(1500, T), batch_size=32, seed=1)
    d = lstm.LSTMDecoder(U, L, 0, 3)
    res = d.fit(xd, yd, epochs=3, engine="device", **kw)
    print("fit on the device 8 x 2000, U 8, L 5: training loss %s, validation loss %s" % (np.round(res["loss_train"], 4), np.round(res["loss_valid"], 4)))
    assert len(res["loss_train"]) == len(res["loss_valid"]) == 3 and np.isfinite(res["loss_train"] + res["loss_valid"]).all()
    assert res["loss_train"][-1] < res["loss_train"][0]
    assert res["num_params"] == 4 * U * (C + U + 1) + K * (U + 1) == d.num_params()
    q = np.minimum(x, 3).astype(np.float64)[:, L - 1:1500]
    w = d.get_weights()
    assert np.allclose(w[5], q.mean(1), rtol=1e-12) and np.allclose(w[6], q.std(1), rtol=1e-9)
    # y's training mean went into dense_bias, on top of the module's own
    ybar = y[:, L - 1:1500].astype(np.float64).mean(1)
    assert np.allclose(w[4], d.module[1].bias.detach().double().cpu().numpy() + ybar, rtol=0, atol=1e-6)
    # the same seed: the same bits
    e = lstm.LSTMDecoder(U, L, 0, 3)
    res2 = e.fit(xd, yd, epochs=3, engine="device", **kw)
    assert all(np.array_equal(a, b) for a, b in zip(w, e.get_weights())) and res2["loss_train"] == res["loss_train"]
    # one minibatch of every training row, one epoch: loss_train[0] is the loss before any update, in both engines
    one = dict(kw, batch_size=2000, epochs=1)
    a = lstm.LSTMDecoder(U, L, 0, 3).fit(xd, yd, engine="autograd", **one)
    f = lstm.LSTMDecoder(U, L, 0, 3)
    b = f.fit(xd, yd, engine="device", **one)
    err = abs(a["loss_train"][0] - b["loss_train"][0]) / abs(a["loss_train"][0])
    print("the first loss: autograd %.7f, device %.7f, apart by %.2e (bound %.1e)" % (a["loss_train"][0], b["loss_train"][0], err, BOUND_OUT))
    assert err <= BOUND_OUT
    assert np.array_equal(f.get_weights()[5], w[5]) and np.array_equal(f.get_weights()[6], w[6])


def test_cross_validate_on_the_device_returns_four_finite_arrays():
    C, T, U, L, K, folds = 8, 2000, 8, 5, 2, 5
    x = lo.counts(C, T, 7)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(lo.target(x, L, 1, K, 8)).cuda()
    res = lstm.cross_validate(xd, yd, L, lead=1, clip=3, num_fold=folds, units=U, epochs=1, batch_size=64, seed=2, engine="device")
    assert sorted(res) == ["cc_test", "cc_valid", "rmse_test", "rmse_valid"]
    for k, v in res.items():
        assert v.shape == (folds, K) and v.dtype == torch.float64 and bool(torch.isfinite(v).all()), k
