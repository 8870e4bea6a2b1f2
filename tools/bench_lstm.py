"""The LSTM decoder (mhl_inproj, mhl_windows; lstm.LSTMDecoder.predict) against the route a user had without it: float32
torch.nn.LSTM + nn.Linear on the device over `unfold`ed, z-scored windows, in chunks of windows so that the [n, L, C]
design of a chunk stays near 1 GiB.

Same process, the routes alternated after warm-up (20 runs each, fewer where 20 rounds of a group would take more than
--budget seconds: the count stands next to every figure; median and range), device events.  Results are compared first.
At 96 ch x 72 000 bins and 1024 ch x 1e6 bins, L = 15, U = 100, K = 2, clip 3:
  inproj   mhl_inproj over all bins, with the share of the 157 TFLOP/s f32 matrix spec that 2 * 4U * C FLOP per bin make
  windows  mhl_windows over all windows, with the share that 2 * 4U * U * L FLOP per window make (step 0 of a window has
           h = 0 and issues no product: the kernel does (L - 1) / L of that)
  predict  LSTMDecoder.predict, both kernels per batch of columns
  torch    the framework route.  Condition: predict's run range lies below torch's, at both shapes.
Prints the table and writes it to --out (default profiles/r24_lstm.txt).

    python tools/bench_lstm.py [--reps 20] [--shapes 96x72000,1024x1000000] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import _lstm, lstm  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_events_out import counts_matrix  # noqa: E402
from bench_wiener import alternate, line  # noqa: E402

L, U, K, CLIP = 15, 100, 2, 3
SPEC = 157e12  # f32 matrix FLOP per second


def torch_route(x, m, lin, mean, inv, out, chunk):
    """float32 nn.LSTM + nn.Linear over the explicit windows of `chunk` design rows at a time"""
    n = x.shape[1] - L + 1
    with torch.no_grad():
        for i0 in range(0, n, chunk):
            k = min(chunk, n - i0)
            u = (torch.clamp(x[:, i0:i0 + k + L - 1], max=CLIP).float() - mean.unsqueeze(1)) * inv.unsqueeze(1)
            hs, _ = m(u.unfold(1, L, 1).permute(1, 2, 0).contiguous())
            out[:, i0:i0 + k] = lin(hs[:, -1]).t()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="96x72000,1024x1000000")
    ap.add_argument("--budget", type=float, default=40.0, help="seconds of timed rounds per group of alternated routes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_lstm.txt"))
    a = ap.parse_args()
    info = muahuff.device_info(0)
    lines = ["bench_lstm: %s (%s), %d alternated runs, L = %d, U = %d, K = %d, clip %d" % (info["name"], info["arch"], a.reps, L, U, K, CLIP)]
    res, met = {}, True
    note = lambda what: print(what, file=sys.stderr, flush=True)  # noqa: E731
    for rows, T in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]:
        x = counts_matrix(rows, T)
        torch.manual_seed(5)
        m = torch.nn.LSTM(rows, U, batch_first=True).cuda()
        lin = torch.nn.Linear(U, K).cuda()
        q = torch.clamp(x, max=CLIP).float()
        mean, std = q.mean(1), q.std(1, unbiased=False)
        del q
        inv = torch.where(std > 0, 1.0 / std, torch.zeros_like(std))
        d = lstm.LSTMDecoder(U, L, 0, CLIP).from_torch(m, lin, mean, std)
        wx, b, wh, wd, bd = d._device(x.device)
        n = T - L + 1
        p = torch.empty((T, 4 * U), dtype=torch.float32, device="cuda")
        out = torch.empty((K, n), dtype=torch.float32, device="cuda")
        want = torch.empty((K, n), dtype=torch.float32, device="cuda")
        chunk = max(1024, (1 << 28) // (L * rows))                   # the float32 design of a chunk is about 1 GiB
        inproj = lambda: _lstm.inproj(x.data_ptr(), x.stride(0), rows, T, CLIP, wx, b, p)  # noqa: E731
        windows = lambda: _lstm.windows(p, L, wh, wd, bd, out)  # noqa: E731
        predict = lambda: d.predict(x)  # noqa: E731
        framework = lambda: torch_route(x, m, lin, mean, inv, want, chunk)  # noqa: E731
        say = lambda what: note("%d x %d: %s" % (rows, T, what))  # noqa: E731
        inproj(), windows()
        try:
            framework()
        except RuntimeError as e:                                    # the vendor RNN library is not usable here: torch's own cell kernels
            say("nn.LSTM failed with the vendor RNN library (%s): timed with torch's own kernels" % str(e).splitlines()[0][:120])
            torch.backends.cudnn.enabled = False
            framework()
        got = predict()
        scale = float(want.abs().max())
        err = float((got - want).abs().max()) / scale
        assert torch.equal(got, out) and err <= 1e-4, (rows, T, err)
        say("results agree: predict and torch differ by %.2e of the largest |out|" % err)
        t = alternate([("inproj", inproj), ("windows", windows), ("predict", predict), ("torch", framework)], a.reps, a.budget, say)
        ok = bool(t["predict"]["max"] < t["torch"]["min"])
        met = met and ok
        f_in, f_win = 2.0 * 4 * U * rows * T, 2.0 * 4 * U * U * L * n
        s_in, s_win = f_in / (t["inproj"]["median"] * 1e-3) / SPEC, f_win / (t["windows"]["median"] * 1e-3) / SPEC
        s_all = (f_in + f_win) / (t["predict"]["median"] * 1e-3) / SPEC
        lines.append("%d x %d: %d windows, p is %.3g GB" % (rows, T, n, _lstm.inproj_bytes(T, U) / 1e9))
        lines.append(line("mhl_inproj", t["inproj"]))
        lines.append(line("mhl_windows", t["windows"]))
        lines.append(line("predict", t["predict"]))
        lines.append(line("torch nn.LSTM, f32" if torch.backends.cudnn.enabled else "torch nn.LSTM, own cells", t["torch"]))
        lines.append("    mhl_inproj %.3g GFLOP = %.3f, mhl_windows %.3g GFLOP = %.3f, predict %.3f of the 157 TFLOP/s f32 matrix spec"
                     % (f_in / 1e9, s_in, f_win / 1e9, s_win, s_all))
        lines.append("    torch / predict x%.2f at the medians; the run ranges %s"
                     % (t["torch"]["median"] / t["predict"]["median"], "are disjoint, predict's below" if ok else "OVERLAP or torch is faster"))
        res["%dx%d" % (rows, T)] = dict(t, disjoint_and_faster=ok, spec_share=dict(inproj=round(s_in, 4), windows=round(s_win, 4), predict=round(s_all, 4)),
                                        max_difference=float(np.float32(err)))
        del x, p, out, want, got
        torch.cuda.empty_cache()
    lines.append("condition (predict below float32 torch.nn.LSTM, run ranges disjoint, both shapes): %s" % ("met" if met else "NOT met"))
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as fh:
        fh.write(text)
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
