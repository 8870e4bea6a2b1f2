"""The Wiener filter's kernels (mhw_xty, mhw_fir; wiener.stats, WienerFilter.fit) against the routes a user has without
them.

uint8 matrices of 1024 ch x 1e7 and 96 ch x 72 000 bins at the synthetic 30 events per second and channel (1 ms bins),
15 lags, 2 covariates.  Same process, event-timed, the routes alternated after warm-up (20 runs each, fewer where 20
rounds of a group would take more than --budget seconds: the count stands next to every figure; median and range):
  xty      mhw_xty: counts times covariates at every lag, float64
  (a)      torch.matmul in float64 on lagged views of a float64 cast, over chunks of columns, summed
  fir      mhw_fir: the prediction, float32
  (b)      torch.nn.functional.conv1d on float32 casts, over chunks of columns
  (c)      one float32 torch.matmul per lag on lagged views of the cast, over chunks of columns
  stats    wiener.stats over all design rows (15 mhi_gram calls, one mhw_xty, the edges)
  fit      WienerFilter(1.0).fit of those statistics
The results are compared first.  Conditions, no margin: median(xty) <= median((a)) and median(fir) <= the smaller of
median((b)) and median((c)), at both shapes.  Reported with no threshold: the share of the 157 TFLOP/s f32 spec that
mhw_fir reaches, counting 2 * k * lags * rows * cols operations.
Prints the table and writes it to --out (default profiles/r18_wiener.txt).

    python tools/bench_wiener.py [--reps 20] [--shapes 1024x10000000,96x72000] [--lags 15] [--k 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import _wiener, wiener  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bin_events import stats as spread  # noqa: E402
from bench_events_out import counts_matrix  # noqa: E402

SPEC = 157e12        # f32 operations per second
CHUNK = 1 << 17      # columns of a chunk: 1 GiB of float64 at 1024 rows


def torch_xty(x, y, L):
    rows, cols = x.shape[0], y.shape[1]
    out = torch.zeros((L, rows, y.shape[0]), dtype=torch.float64, device=x.device)
    for c in range(0, cols, CHUNK):
        n = min(CHUNK, cols - c)
        d = x[:, c:c + n + L - 1].double()
        yd = y[:, c:c + n].double().t()
        for l in range(L):
            out[l] += d[:, L - 1 - l:L - 1 - l + n] @ yd
    return out


def torch_conv(x, wc, bias, L, cols):
    out = torch.empty((wc.shape[0], cols), dtype=torch.float32, device=x.device)
    for c in range(0, cols, CHUNK):
        n = min(CHUNK, cols - c)
        out[:, c:c + n] = torch.nn.functional.conv1d(x[:, c:c + n + L - 1].float().unsqueeze(0), wc, bias)[0]
    return out


def torch_lags(x, w, bias, L, cols):
    out = torch.empty((w.shape[0], cols), dtype=torch.float32, device=x.device)
    for c in range(0, cols, CHUNK):
        n = min(CHUNK, cols - c)
        d = x[:, c:c + n + L - 1].float()
        acc = bias[:, None].expand(-1, n).clone()
        for l in range(L):
            acc += w[:, l, :] @ d[:, L - 1 - l:L - 1 - l + n]
        out[:, c:c + n] = acc
    return out


def alternate(fns, reps, budget, note):
    """fns: [(name, f)] -> {name: stats with "runs"}.  One warm-up round timed on the host clock (synchronised), two more
    if a round is short; then `reps` event-timed rounds name1, name2, ..., name1, ... -- fewer, down to 3, where `reps`
    rounds would take more than `budget` seconds, and where even 3 would, the route's one synchronised warm-up run is all
    it gets and the others alternate without it.  The number of runs behind every figure is kept with it."""
    once = {}
    for k, f in fns:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        once[k] = time.perf_counter() - t0
        note("%s: first run %.3f s" % (k, once[k]))
    slow = {k for k, _ in fns if 3 * once[k] > budget}
    fast = [(k, f) for k, f in fns if k not in slow]
    round_s = sum(once[k] for k, _ in fast)
    n = max(3, min(reps, int(budget / max(round_s, 1e-9))))
    if n * round_s < 1.0:
        for _ in range(2):
            for _, f in fast:
                f()
    torch.cuda.synchronize()
    ev = {k: [] for k, _ in fast}
    for i in range(n):
        for k, f in fast:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
        torch.cuda.synchronize()
        if i % 5 == 4:
            note("round %d of %d" % (i + 1, n))
    out = {k: dict(spread([a.elapsed_time(b) for a, b in v]), runs=n) for k, v in ev.items()}
    for k in slow:
        out[k] = dict(min=round(1e3 * once[k], 4), median=round(1e3 * once[k], 4), max=round(1e3 * once[k], 4), runs=1)
    return out


def line(label, t):
    return "    %-22s min %10.4f median %10.4f max %10.4f ms  (%d run%s)" % (label, t["min"], t["median"], t["max"], t["runs"],
                                                                          "" if t["runs"] == 1 else "s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="1024x10000000,96x72000")
    ap.add_argument("--lags", type=int, default=15)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--budget", type=float, default=90.0, help="seconds of timed rounds per group of alternated routes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_wiener.txt"))
    a = ap.parse_args()
    L, K = a.lags, a.k
    info = muahuff.device_info(0)
    lines = ["bench_wiener: %s (%s), %d alternated runs, %d lags, %d covariates" % (info["name"], info["arch"], a.reps, L, K)]
    res, met_all = {}, True
    for rows, T in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]:
        x = counts_matrix(rows, T)
        g = torch.Generator(device="cuda").manual_seed(5)
        y = torch.randn((K, T), generator=g, device="cuda", dtype=torch.float32)
        w = torch.randn((K, L, rows), generator=g, device="cuda", dtype=torch.float32) / rows
        bias = torch.randn((K,), generator=g, device="cuda", dtype=torch.float32)
        wc = torch.flip(w, [1]).permute(0, 2, 1).contiguous()            # conv1d's [out, in, tap]: tap t is lag L-1-t
        cols = T - L + 1
        yy = y[:, L - 1:]                                                # the target of design row t is y[t]: no lead
        out_xty = torch.empty((L, rows, K), dtype=torch.float64, device="cuda")
        out_fir = torch.empty((K, cols), dtype=torch.float32, device="cuda")
        scratch = torch.empty((_wiener.xty_scratch_bytes(rows, cols, L, K),), dtype=torch.uint8, device="cuda")
        xty = lambda: _wiener.xty(x.data_ptr(), x.stride(0), rows, cols, L, 255, yy.data_ptr(), 4 * y.stride(0), K, out_xty, scratch)  # noqa: E731
        fir = lambda: _wiener.fir(x.data_ptr(), x.stride(0), rows, cols, L, 255, w, bias, K, out_fir)  # noqa: E731
        xty(), fir()
        want = torch_xty(x, yy, L)
        scale = float(want.abs().max())
        assert float((out_xty - want).abs().max()) <= 1e-9 * scale, (rows, T, "xty")
        want = torch_lags(x, w, bias, L, cols)
        assert torch.allclose(out_fir, want, rtol=1e-4, atol=1e-4), (rows, T, "fir")
        assert torch.allclose(torch_conv(x, wc, bias, L, cols), want, rtol=1e-3, atol=1e-3), (rows, T, "conv1d")
        del want
        torch.cuda.empty_cache()
        note = lambda what: print("%d x %d: %s" % (rows, T, what), file=sys.stderr, flush=True)  # noqa: E731
        note("results agree")
        t = alternate([("xty", xty), ("a", lambda: torch_xty(x, yy, L))], a.reps, a.budget, note)
        note("xty timed")
        t.update(alternate([("fir", fir), ("b", lambda: torch_conv(x, wc, bias, L, cols)),
                            ("c", lambda: torch_lags(x, w, bias, L, cols))], a.reps, a.budget, note))
        note("fir timed")
        t.update(alternate([("stats", lambda: wiener.stats(x, y, L))], a.reps, a.budget, note))
        note("stats timed")
        s = wiener.stats(x, y, L)[0]
        t.update(alternate([("fit", lambda: wiener.WienerFilter(1.0).fit(s))], a.reps, a.budget, note))
        del s
        ops = 2.0 * K * L * rows * cols
        best = min(t["b"]["median"], t["c"]["median"])
        cell = dict(t, ops=ops, fir_spec_share=round(ops / (t["fir"]["median"] * 1e-3) / SPEC, 4),
                    a_over_xty=round(t["a"]["median"] / t["xty"]["median"], 2), torch_over_fir=round(best / t["fir"]["median"], 2),
                    xty_met=bool(t["xty"]["median"] <= t["a"]["median"]), fir_met=bool(t["fir"]["median"] <= best))
        met_all = met_all and cell["xty_met"] and cell["fir_met"]
        lines.append("%d x %d" % (rows, T))
        for k, label in (("xty", "mhw_xty"), ("a", "(a) float64 matmul"), ("fir", "mhw_fir"), ("b", "(b) conv1d float32"),
                         ("c", "(c) matmul per lag"), ("stats", "wiener.stats"), ("fit", "WienerFilter.fit")):
            lines.append(line(label, t[k]))
        lines.append("    (a) / xty x%.2f (%s)   faster of (b), (c) / fir x%.2f (%s)   mhw_fir reaches %.4f of the %.0f TFLOP/s f32 spec"
                     % (cell["a_over_xty"], "met" if cell["xty_met"] else "MISSED", cell["torch_over_fir"],
                        "met" if cell["fir_met"] else "MISSED", cell["fir_spec_share"], SPEC / 1e12))
        res["%dx%d" % (rows, T)] = cell
        del x, y, out_fir, scratch
        torch.cuda.empty_cache()
    lines.append("conditions (xty <= (a) and fir <= min((b), (c)) at every shape): %s" % ("met" if met_all else "MISSED"))
    lines.append(json.dumps(dict(cells=res, conditions_met=met_all), sort_keys=True))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
