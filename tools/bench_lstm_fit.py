"""Training the LSTM decoder: LSTMDecoder.fit(engine="device") -- one mht_loss_grad per minibatch, then torch's optimizer --
against engine="autograd", the route the package had without it: a gather of the float design [B, L, C], nn.LSTM + nn.Linear
on torch's own cell kernels, autograd, the same optimizer.

Same process, the routes alternated after warm-up (20 runs each; median and range), device events around everything a
step enqueues, so the time the host needs to issue the launches counts where the device waits for it.  L = 15, U = 100,
K = 2, clip 3, RMSprop:
  step      one training step (loss, gradients, optimizer step) of both engines at 96 ch x 72 000 bins, batch 32 and 1024,
            and at 1024 ch x 1e6 bins, batch 32; and its parts under engine="device": mht_loss_grad alone, opt.step() alone.
            Condition: at 96 channels, batch 32, the device step's run range lies below the autograd step's.
  epoch     fit(epochs=1) over the first four fifths of 96 x 72 000, validated on the rest (host clock, 3 alternated runs),
            with the final validation loss of both engines
  cv        lstm.cross_validate (5 folds x 5 epochs) at 96 x 72 000, once per engine (host clock)
Prints the table and writes it to --out (default profiles/r25_lstm_fit.txt).

    python tools/bench_lstm_fit.py [--reps 20] [--skip-cv] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import _train, lstm  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_events_out import counts_matrix  # noqa: E402
from bench_wiener import alternate, line  # noqa: E402

L, U, K, CLIP = 15, 100, 2, 3


def covariates(x):
    """float32 [K, T]: a 15-bin moving average of a random projection of the clipped counts, plus noise"""
    g = torch.Generator(device="cuda").manual_seed(3)
    C, T = x.shape
    w = torch.randn((K, C), generator=g, device="cuda") / C ** 0.5
    y = torch.zeros((K, T), device="cuda")
    for t0 in range(0, T, 1 << 18):                                  # in slabs: no float copy of all of x
        y[:, t0:t0 + (1 << 18)] = w @ torch.clamp(x[:, t0:t0 + (1 << 18)], max=CLIP).float()
    y = torch.nn.functional.avg_pool1d(torch.nn.functional.pad(y.unsqueeze(0), (L - 1, 0)), L, 1).squeeze(0)
    return (10 * y + 0.1 * torch.randn((K, T), generator=g, device="cuda")).contiguous()


class Steps:
    """one training step of both engines on the same model, as LSTMDecoder.fit forms it"""

    def __init__(self, x, y, batch):
        rows, T = x.shape
        self.x, self.y, self.rows, self.T, self.B = x, y, rows, T, batch
        torch.manual_seed(5)
        self.m = torch.nn.LSTM(rows, U, batch_first=True).cuda()
        self.lin = torch.nn.Linear(U, K).cuda()
        self.m.bias_hh_l0.requires_grad_(False)
        with torch.no_grad():
            self.m.bias_hh_l0.zero_()
        self.params = [self.m.weight_ih_l0, self.m.bias_ih_l0, self.m.weight_hh_l0, self.lin.weight, self.lin.bias]
        self.opt = torch.optim.RMSprop(self.params, lr=1e-5, alpha=0.9, eps=1e-7)
        self.mean = torch.full((rows,), 0.03, device="cuda")
        self.inv = torch.full((rows,), 5.0, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(7)
        self.t = torch.randint(L - 1, T, (batch,), generator=g, device="cuda")
        self.offs = torch.arange(-(L - 1), 1, device="cuda")
        self.xt = x.t()
        # the device route has its own copy of the model and its own optimizer, its gradient tensors bound once as in
        # fit(engine="device"): nothing is rebound inside a timed step
        self.m2, self.lin2 = copy.deepcopy(self.m), copy.deepcopy(self.lin)
        self.params2 = [self.m2.weight_ih_l0, self.m2.bias_ih_l0, self.m2.weight_hh_l0, self.lin2.weight, self.lin2.bias]
        self.opt2 = torch.optim.RMSprop(self.params2, lr=1e-5, alpha=0.9, eps=1e-7)
        self.wts = [p.detach() for p in self.params2]
        self.grads = [torch.zeros_like(p) for p in self.params2]
        for p, g in zip(self.params2, self.grads):
            p.grad = g
        self.scratch = torch.empty((_train.scratch_layout(batch, L, U)["floats"],), dtype=torch.float32, device="cuda")
        self.out = torch.empty((K, batch), dtype=torch.float32, device="cuda")
        self.loss = torch.empty((batch,), dtype=torch.float32, device="cuda")
        self.run = _train.prepared(x.data_ptr(), x.stride(0), rows, T, CLIP, self.mean, self.inv, L, 0, *self.wts, y, self.scratch, *self.grads)

    def loss_grad(self):
        self.run(self.t.data_ptr(), self.B, 1.0 / self.B, self.out.data_ptr(), self.loss.data_ptr())

    def optimizer(self):
        self.opt2.step()

    def device(self):
        self.loss_grad()
        self.opt2.step()

    def autograd(self):
        t = self.t
        u = (torch.clamp(self.xt[t.unsqueeze(1) + self.offs.unsqueeze(0)], max=CLIP).float() - self.mean) * self.inv
        with lstm.own_kernels():
            hs, _ = self.m(u)
        loss = lstm._loss(self.lin(hs[:, -1]), self.y[:, t].t())
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=float, default=40.0, help="seconds of timed rounds per group of alternated routes")
    ap.add_argument("--skip-cv", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_lstm_fit.txt"))
    a = ap.parse_args()
    info = muahuff.device_info(0)
    lines = ["bench_lstm_fit: %s (%s), %d alternated runs, L = %d, U = %d, K = %d, clip %d, RMSprop" % (info["name"], info["arch"], a.reps, L, U, K, CLIP)]
    res, met = {}, True
    note = lambda what: print(what, file=sys.stderr, flush=True)  # noqa: E731
    shapes = [(96, 72000, 32), (96, 72000, 1024)] + ([] if a.skip_large else [(1024, 1000000, 32)])
    x = y = None
    for rows, T, batch in shapes:
        if x is None or tuple(x.shape) != (rows, T):
            del x, y
            torch.cuda.empty_cache()
            x = counts_matrix(rows, T)
            y = covariates(x)
        s = Steps(x, y, batch)
        say = lambda what: note("%d x %d, batch %d: %s" % (rows, T, batch, what))  # noqa: E731
        # the two engines agree on the loss and the gradient of this minibatch before anything is timed
        t = s.t
        u = (torch.clamp(s.xt[t.unsqueeze(1) + s.offs.unsqueeze(0)], max=CLIP).float() - s.mean) * s.inv
        with lstm.own_kernels():
            hs, _ = s.m(u)
        ref = lstm._loss(s.lin(hs[:, -1]), y[:, t].t())
        ref.backward()
        s.loss_grad()
        err = max(float((g - p.grad).abs().max()) / max(float(p.grad.abs().max()), 1e-30) for g, p in zip(s.grads, s.params))
        lerr = abs(float(s.loss.double().mean()) - float(ref.detach())) / float(ref.detach())
        assert err <= 1e-3 and lerr <= 1e-4, (rows, T, batch, err, lerr)
        say("the engines agree: loss apart by %.2e, gradients by %.2e of their largest |entry|" % (lerr, err))
        tm = alternate([("loss_grad", s.loss_grad), ("optimizer", s.optimizer), ("device", s.device), ("autograd", s.autograd)], a.reps, a.budget, say)
        ok = bool(tm["device"]["max"] < tm["autograd"]["min"])
        if rows == 96 and batch == 32:
            met = ok
        lines.append("%d x %d, batch %d: one training step" % (rows, T, batch))
        lines.append(line("mht_loss_grad alone", tm["loss_grad"]))
        lines.append(line("opt.step() alone", tm["optimizer"]))
        lines.append(line("step, engine=device", tm["device"]))
        lines.append(line("step, engine=autograd", tm["autograd"]))
        lines.append("    autograd / device x%.2f at the medians; the run ranges %s"
                     % (tm["autograd"]["median"] / tm["device"]["median"], "are disjoint, the device's below" if ok else "OVERLAP or autograd is faster"))
        res["%dx%d,b%d" % (rows, T, batch)] = dict(tm, disjoint_and_faster=ok, gradient_difference=err)
        del s
        if (rows, T, batch) == (96, 72000, 1024):
            # one epoch, and the cross-validation, by the host clock
            cut = T * 4 // 5
            ep = {"device": [], "autograd": []}
            valid = {}
            for _ in range(3):
                for eng in ("device", "autograd"):
                    d = lstm.LSTMDecoder(U, L, 0, CLIP)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = d.fit(x, y, ranges=[(L - 1, cut)], valid=(cut, T), epochs=1, batch_size=32, seed=1, engine=eng)
                    torch.cuda.synchronize()
                    ep[eng].append(time.perf_counter() - t0)
                    valid[eng] = (r["loss_train"][-1], r["loss_valid"][-1])
                    say("epoch, %s: %.3f s, training loss %.5f, validation loss %.5f" % (eng, ep[eng][-1], *valid[eng]))
            lines.append("96 x 72000: fit(epochs=1, batch_size=32) over %d rows (%d steps), validated on %d; host clock, 3 alternated runs" % (cut - L + 1, -(-(cut - L + 1) // 32), T - cut))
            for eng in ("device", "autograd"):
                v = sorted(ep[eng])
                lines.append("    engine=%-10s min %8.3f median %8.3f max %8.3f s; training loss %.5f, validation loss %.5f" % (eng, v[0], v[1], v[2], *valid[eng]))
            lines.append("    autograd / device x%.2f at the medians; the final validation losses differ by %.2e (relative)"
                         % (sorted(ep["autograd"])[1] / sorted(ep["device"])[1], abs(valid["device"][1] - valid["autograd"][1]) / valid["autograd"][1]))
            res["epoch"] = dict(seconds=ep, losses=valid)
            if not a.skip_cv:
                cv = {}
                for eng in ("device", "autograd"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = lstm.cross_validate(x, y, L, 0, CLIP, num_fold=5, units=U, epochs=5, batch_size=32, seed=1, engine=eng)
                    torch.cuda.synchronize()
                    cv[eng] = (time.perf_counter() - t0, float(r["rmse_valid"].mean()), float(r["rmse_test"].mean()))
                    say("cross_validate, %s: %.2f s, mean rmse_valid %.5f, rmse_test %.5f" % (eng, *cv[eng]))
                lines.append("96 x 72000: lstm.cross_validate, 5 folds x 5 epochs, batch 32; host clock, one run each")
                for eng in ("device", "autograd"):
                    lines.append("    engine=%-10s %8.2f s; mean rmse_valid %.5f, mean rmse_test %.5f" % (eng, *cv[eng]))
                lines.append("    autograd / device x%.2f" % (cv["autograd"][0] / cv["device"][0]))
                res["cross_validate"] = cv
    lines.append("condition (96 channels, batch 32: the device step's run range below the autograd step's): %s" % ("met" if met else "NOT met"))
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as fh:
        fh.write(text)
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
