"""Behavioural decoding from spike counts: the LSTM decoder -- the reference's LSTMDecoder, one Keras LSTM(units) layer
over the last `lags` bins of every channel followed by Dense(outputs), stateless -- applied on the device to raw uint8
counts x [C, T] without the [T - L + 1, L, C] design tensor of the reference's input_shaping.

DESIGN ROW i, for i in [0, T - L + 1), is the window x[:, i .. i+L-1], oldest bin first; every channel enters as
u[c] = (min(x[c], clip) - mean[c]) / std[c].  From h = c = 0, for s = 0 .. L-1,
    z = Wx^T u[:, i+s] + Wh^T h + b   (4U values, gates in Keras order i, f, c, o);
    i, f, o = sigmoid(z_i), sigmoid(z_f), sigmoid(z_o);  g = tanh(z_c);  c = f c + i g;  h = o tanh(c),
and out = Wd^T h + bd estimates y[:, i + L-1 + lead].  A channel that is constant over the training rows (std = 0) is
dropped: its column of the input weights is zero.

Wx^T u depends on the bin and not on the window: predict() is one mhl_inproj (every bin's input half of the
pre-activations, with the z-scoring folded into the weights) and one mhl_windows (the recurrence of every window and the
dense layer) per batch of columns, the batches sized by what the scratch matrix of pre-activations may take.  fit() trains
minibatch by minibatch with torch's optimizers; the loss of a minibatch and its gradient come from torch autograd on windows
gathered from the uint8 matrix (engine="autograd", the default) or from one mht_loss_grad that reads the counts where they
lie (engine="device", muahuff_train.h; loss_and_grad() is that call on its own).
There is no CPU path: host matrices are refused."""
import contextlib

import numpy as np
import torch

from . import wiener
from .windows import MAX_BYTES, _matrix


def _np64(t, shape, what):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.array(a, dtype=np.float64)
    if a.shape != tuple(shape):
        raise ValueError("%s has the shape %s, not %s" % (what, list(shape), list(a.shape)))
    if not np.isfinite(a).all():
        raise ValueError("%s is not finite" % what)
    return a


def _rmse_cc(p, t):
    """WienerFilter._score's arithmetic on a prediction and its targets, both float64 [K, n]"""
    rmse = torch.sqrt(((p - t) ** 2).mean(1))
    pc, tc = p - p.mean(1, keepdim=True), t - t.mean(1, keepdim=True)
    cc = (pc * tc).sum(1) / torch.sqrt((pc * pc).sum(1) * (tc * tc).sum(1))
    return rmse, cc


@contextlib.contextmanager
def own_kernels():
    """nn.LSTM on torch's own cell kernels, not the vendor RNN library: the same arithmetic on every machine, and nothing
    tuned or cached at run time"""
    was = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        yield
    finally:
        torch.backends.cudnn.enabled = was


def _loss(pred, target):
    """the reference's loss: the mean over the rows of the root of the mean over the outputs of err^2; [n, K] both"""
    return torch.sqrt(((pred - target) ** 2).mean(1)).mean()


def _zscoring(mean, std, dev):
    """-> (mean, inv) float32 [C] on dev, as fit() forms them: inv = 1 / std in float64, 0 where std is 0 (the channel is dropped)"""
    mean = torch.as_tensor(mean, dtype=torch.float64).to(dev)
    std = torch.as_tensor(std, dtype=torch.float64).to(dev)
    keep = std > 0
    inv = torch.where(keep, 1.0 / torch.where(keep, std, torch.ones_like(std)), torch.zeros_like(std)).float()
    return mean.float().contiguous(), inv.contiguous()


def loss_and_grad(x, y, idx, weights, mean, std, lags, lead=0, clip=None, scale=None):
    """The loss of one minibatch of windows and its gradient, in one mht_loss_grad (muahuff_train.h).  x: uint8 device tensor
    [C, T]; y: float32 device tensor [K, T]; idx: int64 device tensor [B], window b being design row idx[b] in WienerFilter's
    numbering (it ends in bin idx[b], its target is y[:, idx[b] + lead]; lags-1 <= idx[b] <= T-1-lead, a repeated row counts
    twice); weights: (wx [4U, C], bias [4U], wh [4U, U], wd [K, U], bd [K]), float32 device tensors in torch.nn.LSTM's and
    nn.Linear's layout, gates i, f, g, o; mean, std [C] of the clipped counts: every channel enters as
    (min(x, clip) - mean) / std, a channel of std 0 is dropped.
    -> (out float32 [K, B], loss float32 [B]: sqrt(mean over K of err^2) per window, dict(wx, bias, wh, wd, bd): the gradient of
    scale * loss.sum() with respect to each of the weights; scale defaults to 1 / B, the reference's mean over the rows).
    A window whose loss is exactly 0 adds nothing to the gradient, where autograd would give NaN."""
    from . import _train
    x, rows, cols = _matrix(x, "lstm.loss_and_grad")
    y, K = wiener._covariates(y, x, cols)
    dev, L, g, q = x.device, int(lags), int(lead), wiener._clip(clip)
    if not (isinstance(idx, torch.Tensor) and idx.dtype == torch.int64 and idx.dim() == 1 and idx.device == dev):
        raise ValueError("idx is an int64 tensor [B] on the device of the counts")
    B = int(idx.numel())
    if not 1 <= B <= _train.MAX_BATCH:
        raise ValueError("%d windows outside 1..%d" % (B, _train.MAX_BATCH))
    if len(weights) != 5 or not all(isinstance(w, torch.Tensor) and w.device == dev for w in weights):
        raise ValueError("weights are (wx, bias, wh, wd, bd), tensors on the device of the counts")
    wx, bias, wh, wd, bd = (w.detach() for w in weights)
    if wh.dim() != 2 or wd.dim() != 2 or int(wd.shape[0]) != K:
        raise ValueError("wh is [4 units, units] and wd [%d, units]" % K)
    U = int(wh.shape[1])
    mean32, inv = _zscoring(mean, std, dev)
    out = torch.empty((K, B), dtype=torch.float32, device=dev)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    grads = {n: torch.empty_like(w) for n, w in zip(("wx", "bias", "wh", "wd", "bd"), (wx, bias, wh, wd, bd))}
    scratch = torch.empty((_train.scratch_layout(B, L, U)["floats"],), dtype=torch.float32, device=dev)
    _train.loss_grad(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, cols, q, mean32, inv, idx.contiguous(), L, g, wx, bias, wh, wd, bd,
                     y, 1.0 / B if scale is None else float(scale), scratch, out, loss, *grads.values())
    return out, loss, grads


class LSTMDecoder:
    """The reference's LSTMDecoder at num_layers = 1, stateless, without dropout.  After set_weights(), from_torch() or
    fit(): kernel [C, 4U], recurrent_kernel [U, 4U], bias [4U], dense_kernel [U, K], dense_bias [K] in Keras layout,
    mean and std [C] of the clipped counts (std = 0: the channel is dropped), all float64 numpy; channels, outputs."""

    def __init__(self, units=100, lags=15, lead=0, clip=None, num_layers=1, stateful=False, dropout=0.0, window=1):
        from ._lstm import MAX_LAGS, MAX_UNITS
        if int(num_layers) != 1:
            raise ValueError("one LSTM layer: num_layers = %d is not built" % int(num_layers))
        if stateful:
            raise ValueError("every window starts from h = c = 0: stateful = True is not built")
        if float(dropout) != 0.0:
            raise ValueError("dropout = %g is not built" % float(dropout))
        if int(window) != 1:
            raise ValueError("a moving-average window is not built for the LSTM decoder")
        self.units, self.lags, self.lead = int(units), int(lags), int(lead)
        if not 1 <= self.units <= MAX_UNITS:
            raise ValueError("units %d outside 1..%d" % (self.units, MAX_UNITS))
        if not 1 <= self.lags <= MAX_LAGS:
            raise ValueError("lags %d outside 1..%d" % (self.lags, MAX_LAGS))
        if self.lead < 0:
            raise ValueError("lead %d is negative" % self.lead)
        self.clip = wiener._clip(clip)
        self.kernel = self.recurrent_kernel = self.bias = self.dense_kernel = self.dense_bias = self.mean = self.std = None
        self.channels = self.outputs = None
        self.module = None                                          # (nn.LSTM, nn.Linear) after fit()
        self._dev = None

    # ---- the weights ---------------------------------------------------------------------------------------------------
    def set_weights(self, kernel, recurrent_kernel, bias, dense_kernel, dense_bias, mean=None, std=None):
        """The weights in Keras layout: kernel [C, 4U], recurrent_kernel [U, 4U], bias [4U] (gates i, f, c, o),
        dense_kernel [U, K], dense_bias [K]; mean, std [C] of the clipped counts (default 0 and 1: the clipped counts
        enter as they are).  std == 0 drops the channel."""
        from ._lstm import MAX_K, MAX_ROWS
        U = self.units
        k = np.asarray(kernel.detach().cpu() if isinstance(kernel, torch.Tensor) else kernel)
        dk = np.asarray(dense_kernel.detach().cpu() if isinstance(dense_kernel, torch.Tensor) else dense_kernel)
        if k.ndim != 2 or dk.ndim != 2:
            raise ValueError("kernel is [channels, 4 units] and dense_kernel [units, outputs]")
        C, K = int(k.shape[0]), int(dk.shape[1])
        if not 1 <= C <= MAX_ROWS or not 1 <= K <= MAX_K:
            raise ValueError("%d channels outside 1..%d or %d outputs outside 1..%d" % (C, MAX_ROWS, K, MAX_K))
        self.kernel = _np64(kernel, (C, 4 * U), "kernel")
        self.recurrent_kernel = _np64(recurrent_kernel, (U, 4 * U), "recurrent_kernel")
        self.bias = _np64(bias, (4 * U,), "bias")
        self.dense_kernel = _np64(dense_kernel, (U, K), "dense_kernel")
        self.dense_bias = _np64(dense_bias, (K,), "dense_bias")
        self.mean = np.zeros(C) if mean is None else _np64(mean, (C,), "mean")
        self.std = np.ones(C) if std is None else _np64(std, (C,), "std")
        if (self.std < 0).any():
            raise ValueError("std is not negative")
        self.channels, self.outputs, self._dev = C, K, None
        return self

    def from_torch(self, lstm, linear, mean=None, std=None):
        """The weights of a one-layer torch.nn.LSTM and the nn.Linear behind it: b_ih + b_hh is the bias, the gate order
        (i, f, g, o) is Keras's."""
        if not isinstance(lstm, torch.nn.LSTM) or not isinstance(linear, torch.nn.Linear):
            raise ValueError("from_torch takes a torch.nn.LSTM and a torch.nn.Linear")
        if lstm.num_layers != 1 or lstm.bidirectional or getattr(lstm, "proj_size", 0) or lstm.dropout:
            raise ValueError("one unidirectional LSTM layer without projection or dropout")
        if lstm.hidden_size != self.units or linear.in_features != self.units:
            raise ValueError("the modules have %d and %d units, not %d" % (lstm.hidden_size, linear.in_features, self.units))
        U = self.units
        zero = torch.zeros(4 * U, dtype=torch.float64)
        b = (lstm.bias_ih_l0.detach().cpu().double() + lstm.bias_hh_l0.detach().cpu().double()) if lstm.bias else zero
        bd = linear.bias.detach() if linear.bias is not None else torch.zeros(linear.out_features)
        return self.set_weights(lstm.weight_ih_l0.detach().t(), lstm.weight_hh_l0.detach().t(), b, linear.weight.detach().t(), bd, mean, std)

    def get_weights(self):
        """-> (kernel, recurrent_kernel, bias, dense_kernel, dense_bias, mean, std), what set_weights took, float64 numpy"""
        if self.kernel is None:
            raise ValueError("get_weights comes after set_weights, from_torch or fit")
        return tuple(a.copy() for a in (self.kernel, self.recurrent_kernel, self.bias, self.dense_kernel, self.dense_bias, self.mean, self.std))

    def folded(self):
        """-> (wx [4U, C], bias [4U], wh [4U, U], wd [K, U], bd [K]), float32 numpy: what mhl_inproj and mhl_windows take.
        The z-scoring is folded in float64: wx[g][c] = kernel[c][g] / std[c] and bias[g] = b[g] - sum over c of
        wx[g][c] mean[c]; a channel of std 0 has a zero column and no part in the bias."""
        if self.kernel is None:
            raise ValueError("predict comes after set_weights, from_torch or fit")
        keep = self.std > 0
        inv = np.where(keep, 1.0 / np.where(keep, self.std, 1.0), 0.0)
        wx = (self.kernel * inv[:, None]).T
        bias = self.bias - wx @ self.mean
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        return f(wx), f(bias), f(self.recurrent_kernel.T), f(self.dense_kernel.T), f(self.dense_bias)

    def num_params(self):
        """Keras's count_params of the model"""
        U = self.units
        return 4 * U * (self.channels + U + 1) + self.outputs * (U + 1)

    def _device(self, dev):
        if self._dev is None or self._dev[0].device != dev:
            self._dev = tuple(torch.from_numpy(a).to(dev) for a in self.folded())
        return self._dev

    # ---- the prediction --------------------------------------------------------------------------------------------------
    def _run(self, ptr, pitch, rows, bins, out, max_bytes, dev):
        """the windows of `bins` columns from the byte address ptr on into out [K, bins - L + 1], in batches whose scratch
        stays under max_bytes; every batch recomputes the L-1 columns of p in front of its first window's last bin"""
        from . import _lstm
        wx, b, wh, wd, bd = self._device(dev)
        L, U = self.lags, self.units
        n = bins - L + 1
        per = max(int(max_bytes) // _lstm.inproj_bytes(1, U) - (L - 1), 1)      # windows of a batch
        scratch = torch.empty((min(per, n) + L - 1, 4 * U), dtype=torch.float32, device=dev)
        for i0 in range(0, n, per):
            m = min(per, n - i0)
            p = scratch[:m + L - 1]
            _lstm.inproj(ptr + i0, pitch, rows, m + L - 1, self.clip, wx, b, p)
            _lstm.windows(p, L, wh, wd, bd, out[:, i0:i0 + m])

    def _fits(self, rows, cols):
        if self.kernel is None:
            raise ValueError("predict comes after set_weights, from_torch or fit")
        if rows != self.channels:
            raise ValueError("the decoder has weights for %d channels, not %d" % (self.channels, rows))
        if cols < self.lags:
            raise ValueError("%d bins are fewer than the %d lags" % (cols, self.lags))

    def predict(self, x, max_bytes=MAX_BYTES):
        """-> float32 [K, T - L + 1]: column i is design row i, the estimate of y[:, i + L-1 + lead], as
        WienerFilter.predict numbers them.  One mhl_inproj and one mhl_windows per batch of columns; the result is the
        same bit for bit for any max_bytes."""
        x, rows, cols = _matrix(x, "LSTMDecoder.predict")
        self._fits(rows, cols)
        out = torch.empty((self.outputs, cols - self.lags + 1), dtype=torch.float32, device=x.device)
        self._run(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, cols, out, max_bytes, x.device)
        return out

    def predict_from(self, src):
        """predict on the bins of a gram.BinSource (archive.Reader.bins, container_io.bins), without holding them: every
        batch of gram.walk keeps the L-1 bins in front of it and fills its own columns of the result."""
        from .gram import walk
        rows, cols = wiener._source(src, "LSTMDecoder.predict_from")
        self._fits(rows, cols)
        L = self.lags
        out = torch.empty((self.outputs, cols - L + 1), dtype=torch.float32, device=src.device)
        for b0, nb, h, view in walk(src, L - 1):
            first = max(b0, L - 1)                                  # the last bin of this batch's first window
            m = b0 + nb - first
            if m > 0:
                lo = first - (L - 1)
                self._run(view.data_ptr() + lo - (b0 - h), view.stride(0) if rows > 1 else int(view.shape[1]), rows, m + L - 1,
                          out[:, lo:lo + m], src.max_bytes, src.device)
        return out

    def _score(self, pred, y):
        """WienerFilter._score: the columns whose target lies inside the recording"""
        n = pred.shape[1] - self.lead
        if n < 1 or y.shape[0] != pred.shape[0]:
            raise ValueError("counts and covariates do not match, or no target lies inside them")
        return _rmse_cc(pred[:, :n].double(), y[:, self.lags - 1 + self.lead:].double())

    def score(self, x, y):
        """-> (rmse [K], cc [K]), float64: the root mean squared error and Pearson's r of the prediction against y over
        the columns where the target exists"""
        x, _rows, cols = _matrix(x, "LSTMDecoder.score")
        y, _K = wiener._covariates(y, x, cols)
        return self._score(self.predict(x), y)

    def score_from(self, src, y):
        """score on the result of predict_from"""
        y, _K = wiener._source_covariates(y, src)
        return self._score(self.predict_from(src), y)

    def score_ranges(self, x, y, ranges):
        """-> (rmse, cc), float64 [ranges, K]: score over ranges [a, b) of design rows in WienerFilter's numbering (row t is
        the window that ends in bin t, its target y[:, t + lead]), each predicted from its own columns alone"""
        x, _rows, cols = _matrix(x, "LSTMDecoder.score_ranges")
        y, _K = wiener._covariates(y, x, cols)
        L, g = self.lags, self.lead
        res = []
        for a, b in wiener._ranges(ranges, L, g, cols):
            if b <= a:
                raise ValueError("a scored range holds a design row")
            res.append(_rmse_cc(self.predict(x[:, a - (L - 1):b]).double(), y[:, a + g:b + g].double()))
        return torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res])

    # ---- the fit ---------------------------------------------------------------------------------------------------------
    def fit(self, x, y, ranges=None, valid=None, epochs=5, batch_size=32, optimizer="RMSprop", lrate=1e-3, shuffle=True, seed=0,
            engine="autograd"):
        """Train on the design rows of `ranges` ([a, b) in WienerFilter's numbering: row t is the window that ends in bin t;
        default all of them) -> the reference's fit_out: dict(loss_train, loss_valid: one value per epoch, num_params).
        x: uint8 device tensor [C, T]; y: float32 device tensor [K, T].  mean and std of the clipped counts over the
        training rows come from wiener.stats at one lag; y is centred on its training mean, which goes into dense_bias.
        The model is nn.LSTM + nn.Linear with Keras's initial weights (Glorot uniform, orthogonal recurrent kernel, forget
        bias 1) and one bias vector, the loss the reference's rmse, the optimizer RMSprop (rho 0.9, eps 1e-7: Keras's),
        Adam or SGD at lrate.  engine="autograd": a minibatch's windows are gathered from x as they are needed and torch
        autograd gives the gradient.  engine="device": the same initial weights, generator, order and optimizer, but the
        loss and the gradient of a minibatch are one mht_loss_grad (muahuff_train.h) on the counts where they lie, written
        into gradient tensors bound to the parameters once: no gather, no autograd graph.  After every epoch the weights
        are exported and, with valid = [a, b) or a list of such ranges, the loss over them is taken from predict()."""
        if engine not in ("autograd", "device"):
            raise ValueError("engine is autograd or device")
        x, rows, cols = _matrix(x, "LSTMDecoder.fit")
        y, K = wiener._covariates(y, x, cols)
        L, g, U, q, dev = self.lags, self.lead, self.units, self.clip, x.device
        if cols - g < L:
            raise ValueError("%d bins leave no design row at lags %d, lead %d" % (cols, L, g))
        epochs, batch_size = int(epochs), int(batch_size)
        if epochs < 1 or batch_size < 1:
            raise ValueError("at least one epoch and one row per minibatch")
        rs = wiener._ranges(ranges, L, g, cols)
        vs = None
        if valid is not None:
            vs = wiener._ranges([valid] if np.ndim(valid[0]) == 0 else valid, L, g, cols)
        st = sum(wiener.stats(x, y, 1, g, q, rs))
        if st.n < 1:
            raise ValueError("the training ranges hold no design row")
        n = float(st.n)
        diag = torch.diagonal(st.gram)
        mean = st.sum_x.double() / n
        keep = (st.n * diag - st.sum_x * st.sum_x) > 0              # exact in int64: n * 255 * 255 * n stays inside it
        if st.n * q * q * st.n >= 2 ** 63:
            keep = (n * diag.double() - st.sum_x.double() ** 2) > 2.0 ** -40 * n * diag.double()
        if not bool(keep.any()):
            raise ValueError("every channel is constant: nothing to fit")
        std = torch.where(keep, torch.sqrt(torch.clamp(diag.double() / n - mean * mean, min=0.0)), torch.zeros_like(mean))
        ybar = st.sum_y / n
        inv = torch.where(keep, 1.0 / torch.where(keep, std, torch.ones_like(std)), torch.zeros_like(std)).float()
        mean32 = mean.float()

        gen = torch.Generator().manual_seed(int(seed))
        lstm = torch.nn.LSTM(rows, U, batch_first=True)
        linear = torch.nn.Linear(U, K)
        with torch.no_grad():
            lim = (6.0 / (rows + 4 * U)) ** 0.5
            lstm.weight_ih_l0.copy_((torch.rand((4 * U, rows), generator=gen) * 2 - 1) * lim)
            qm, rm = torch.linalg.qr(torch.randn((4 * U, U), generator=gen, dtype=torch.float64))
            lstm.weight_hh_l0.copy_((qm * torch.sign(torch.diagonal(rm)).unsqueeze(0)).float())
            lstm.bias_ih_l0.zero_()
            lstm.bias_ih_l0[U:2 * U] = 1.0
            lstm.bias_hh_l0.zero_()
            lim = (6.0 / (U + K)) ** 0.5
            linear.weight.copy_((torch.rand((K, U), generator=gen) * 2 - 1) * lim)
            linear.bias.zero_()
        lstm.bias_hh_l0.requires_grad_(False)                       # one bias vector, as Keras has it
        lstm, linear = lstm.to(dev), linear.to(dev)
        params = [p for p in list(lstm.parameters()) + list(linear.parameters()) if p.requires_grad]
        if optimizer == "RMSprop":
            opt = torch.optim.RMSprop(params, lr=float(lrate), alpha=0.9, eps=1e-7)
        elif optimizer == "Adam":
            opt = torch.optim.Adam(params, lr=float(lrate), eps=1e-7)
        elif optimizer == "SGD":
            opt = torch.optim.SGD(params, lr=float(lrate))
        else:
            raise ValueError("optimizer is RMSprop, Adam or SGD")

        rows_t = torch.cat([torch.arange(a, b, device=dev) for a, b in rs])
        offs = torch.arange(-(L - 1), 1, device=dev)
        xt, yc = x.t(), (y.double() - ybar.unsqueeze(1)).float()
        self.module = (lstm, linear)
        if engine == "device":
            from . import _train
            nb = min(batch_size, int(rows_t.numel()))
            if nb > _train.MAX_BATCH:
                raise ValueError("a minibatch of %d rows is above the %d of engine=device" % (nb, _train.MAX_BATCH))
            wts = [w.detach() for w in (lstm.weight_ih_l0, lstm.bias_ih_l0, lstm.weight_hh_l0, linear.weight, linear.bias)]
            grads = [torch.zeros_like(w) for w in wts]
            for w, gr in zip((lstm.weight_ih_l0, lstm.bias_ih_l0, lstm.weight_hh_l0, linear.weight, linear.bias), grads):
                w.grad = gr                                         # bound once: every mht_loss_grad overwrites them
            scratch = torch.empty((_train.scratch_layout(nb, L, U)["floats"],), dtype=torch.float32, device=dev)
            # out of one minibatch, and the loss of every window of an epoch (summed once, at its end)
            obuf = torch.empty((K * nb,), dtype=torch.float32, device=dev)
            lbuf = torch.empty((int(rows_t.numel()),), dtype=torch.float32, device=dev)
            step = _train.prepared(x.data_ptr(), x.stride(0) if rows > 1 else cols, rows, cols, q, mean32.contiguous(), inv.contiguous(), L, g,
                                   *wts, yc, scratch, *grads)      # checked once: a step is the call and opt.step()
        out = dict(loss_train=[], loss_valid=[], num_params=4 * U * (rows + U + 1) + K * (U + 1))
        for _epoch in range(epochs):
            order = rows_t[torch.randperm(rows_t.numel(), generator=gen).to(dev)] if shuffle else rows_t
            total = torch.zeros((), dtype=torch.float64, device=dev)
            n_rows = int(order.numel())
            for i in range(0, order.numel(), batch_size):
                if engine == "device":
                    B = min(batch_size, n_rows - i)
                    step(order.data_ptr() + 8 * i, B, 1.0 / B, obuf.data_ptr(), lbuf.data_ptr() + 4 * i)
                    opt.step()
                    continue
                t = order[i:i + batch_size]
                u = (torch.clamp(xt[t.unsqueeze(1) + offs.unsqueeze(0)], max=q).float() - mean32) * inv   # [B, L, C]
                with own_kernels():
                    hs, _ = lstm(u)
                loss = _loss(linear(hs[:, -1]), yc[:, t + g].t())
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                total += loss.detach().double() * t.numel()
            if engine == "device":
                total = lbuf.sum(dtype=torch.float64)
            out["loss_train"].append(float(total) / order.numel())
            self.from_torch(lstm, linear, mean, std)
            self.dense_bias = self.dense_bias + ybar.cpu().numpy()
            if vs is not None:
                num, cnt = 0.0, 0
                for a, b in vs:
                    pred = self.predict(x[:, a - (L - 1):b])
                    num += float(torch.sqrt(((pred - y[:, a + g:b + g]) ** 2).mean(0)).double().sum())
                    cnt += b - a
                out["loss_valid"].append(num / max(cnt, 1))
        return out


def cross_validate(x, y, lags, lead=0, clip=None, num_fold=5, units=100, **fit_args):
    """The study's cross-validation of the LSTM decoder -> dict(rmse_valid, rmse_test, cc_valid, cc_test), each float64
    [num_fold, K] on the device: split i validates on fold i, tests on fold i + 1 (cyclically) and trains on the others
    (wiener.folds).  Per split one fit() with fit_args, its validation loss taken on the split's validation fold, and
    one score over the two held-out folds."""
    x, _rows, cols = _matrix(x, "lstm.cross_validate")
    y, K = wiener._covariates(y, x, cols)
    splits = wiener.folds(x, num_fold, lags, lead)
    res = {k: torch.empty((len(splits), K), dtype=torch.float64, device=x.device) for k in ("rmse_valid", "rmse_test", "cc_valid", "cc_test")}
    for i, (train, valid, test) in enumerate(splits):
        d = LSTMDecoder(units, lags, lead, clip)
        d.fit(x, y, ranges=train, valid=valid, **fit_args)
        rmse, cc = d.score_ranges(x, y, [valid, test])
        res["rmse_valid"][i], res["rmse_test"][i] = rmse[0], rmse[1]
        res["cc_valid"][i], res["cc_test"][i] = cc[0], cc[1]
    return res
