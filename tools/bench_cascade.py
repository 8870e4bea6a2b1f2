"""The Wiener cascade's kernels and driver (mhc_moments, mhc_polyval; WienerCascade.predict, cascade.cross_validate)
against the routes a user has without them.

Same process, the routes alternated after warm-up (20 runs each, fewer where 20 rounds of a group would take more than
--budget seconds: the count stands next to every figure; median and range):
  1  mhc_moments at degree 4 over five fold ranges of a float32 prediction and target [2, cols], cols = 1e7 and 72 000,
     against (t) the same sums from torch: float64 powers and products over the slices, on the device.  Results compared
     first.  Condition, no margin: median(moments) < median((t)) at both sizes.  Reported: the ratio and the share of
     the 8 TB/s spec on the bytes read (2 arrays x 2 rows x cols x 4).
  2  WienerCascade.predict (mhw_fir, then mhc_polyval in place, degree 3) against WienerFilter.predict (mhw_fir alone) at
     1024 ch x 1e7 bins, 15 lags, 2 outputs, the same weights.  Condition: the two medians differ by no more than
     max - min of WienerFilter.predict's own runs.
  3  cascade.cross_validate (5 folds, 3 alphas, degrees 2..4) at 96 ch x 72 000 bins, 15 lags, against the loop a user
     writes without it: wiener.stats per fold, fit, predict, np.polyfit on the host from a copied prediction, the
     polynomial and the scores per fold with torch.  Host clock around a synchronise, no threshold; and where
     cross_validate's time goes: its pieces timed one by one (stats, solve, mhw_fir, the moments calls, mhc_polyval), the
     rest is host work between them.
Prints the table and writes it to --out (default profiles/r19_cascade.txt).

    python tools/bench_cascade.py [--reps 20] [--parts 1,2,3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import _cascade, cascade, wiener  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_events_out import counts_matrix  # noqa: E402
from bench_wiener import alternate, line  # noqa: E402

SPEC_BW = 8e12       # bytes per second
L, K = 15, 2


def torch_moments(p, y, ranges, degree, center, inv):
    out = torch.empty((len(ranges), p.shape[0], 3 * degree + 4), dtype=torch.float64, device=p.device)
    for r, (a, b) in enumerate(ranges):
        u = (p[:, a:b].double() - center[:, None]) * inv[:, None]
        yd = y[:, a:b].double()
        w = torch.ones_like(u)
        for i in range(2 * degree + 1):
            out[r, :, i] = w.sum(1)
            if i <= degree:
                out[r, :, 2 * degree + 1 + i] = (w * yd).sum(1)
            w = w * u
        out[r, :, 3 * degree + 2] = (yd * yd).sum(1)
        out[r, :, 3 * degree + 3] = ((u - yd) ** 2).sum(1)
    return out


def part1(a, lines, res, note):
    degree, met = 4, True
    for cols in (10 ** 7, 72000 - L + 1):
        g = torch.Generator(device="cuda").manual_seed(5)
        p = torch.randn((K, cols), generator=g, device="cuda", dtype=torch.float32) * 1.5 + 0.3
        y = p + 0.1 * p * p + torch.randn((K, cols), generator=g, device="cuda", dtype=torch.float32)
        center, inv = p.double().mean(1), 1.0 / p.double().std(1)
        ranges = wiener.fold_ranges(cols, 5)
        out = torch.empty((5, K, _cascade.per(degree)), dtype=torch.float64, device="cuda")
        scratch = torch.empty((_cascade.moments_scratch_bytes(cols, K, degree, 5),), dtype=torch.uint8, device="cuda")
        mom = lambda: _cascade.moments(p, y, ranges, degree, center, inv, out, scratch)  # noqa: E731
        mom()
        want = torch_moments(p, y, ranges, degree, center, inv)
        assert torch.allclose(out, want, rtol=1e-9, atol=1e-6), cols
        t = alternate([("moments", mom), ("t", lambda: torch_moments(p, y, ranges, degree, center, inv))], a.reps, a.budget, note)
        nbytes = 2 * K * cols * 4
        cell = dict(t, bytes=nbytes, t_over_moments=round(t["t"]["median"] / t["moments"]["median"], 2),
                    spec_share=round(nbytes / (t["moments"]["median"] * 1e-3) / SPEC_BW, 4), met=bool(t["moments"]["median"] < t["t"]["median"]))
        met = met and cell["met"]
        lines.append("1  moments, degree %d, 5 ranges, [%d, %d]" % (degree, K, cols))
        lines.append(line("mhc_moments", t["moments"]))
        lines.append(line("(t) torch float64", t["t"]))
        lines.append("    (t) / moments x%.2f (%s)   %.1f MB read: %.4f of the 8 TB/s spec at the median" %
                     (cell["t_over_moments"], "met" if cell["met"] else "MISSED", nbytes / 1e6, cell["spec_share"]))
        res["moments_%d" % cols] = cell
    return met


def part2(a, lines, res, note):
    rows, T, degree = 1024, 10 ** 7, 3
    x = counts_matrix(rows, T)
    g = torch.Generator(device="cuda").manual_seed(5)
    f = wiener.WienerFilter(0.0)
    f.weights = (torch.randn((K, L, rows), generator=g, device="cuda", dtype=torch.float32) / rows).double()
    f.bias = torch.randn((K,), generator=g, device="cuda", dtype=torch.float32).double()
    f.lags, f.lead, f.clip, f.channels = L, 0, 255, rows
    c = cascade.WienerCascade(0.0, degree)
    c.linear = f
    lin = f.predict(x)
    c.center, c.scale = lin.double().mean(1), lin.double().std(1)
    c.coef = torch.tensor([[0.01, 0.1, 1.0, 0.05]] * K, dtype=torch.float64, device="cuda")
    u = (lin - c.center.float()[:, None]) * (1.0 / c.scale).float()[:, None]
    want = ((0.01 * u + 0.1) * u + 1.0) * u + 0.05
    assert torch.allclose(c.predict(x), want, rtol=1e-4, atol=1e-5)
    del lin, u, want
    torch.cuda.empty_cache()
    t = alternate([("filter", lambda: f.predict(x)), ("cascade", lambda: c.predict(x))], a.reps, a.budget, note)
    spread = t["filter"]["max"] - t["filter"]["min"]
    diff = t["cascade"]["median"] - t["filter"]["median"]
    cell = dict(t, filter_range=round(spread, 4), cascade_range=round(t["cascade"]["max"] - t["cascade"]["min"], 4), median_difference=round(diff, 4),
                met=bool(abs(diff) <= spread))
    lines.append("2  predict, %d x %d, %d lags, %d outputs, degree %d" % (rows, T, L, K, degree))
    lines.append(line("WienerFilter.predict", t["filter"]))
    lines.append(line("WienerCascade.predict", t["cascade"]))
    lines.append("    medians differ by %.4f ms; WienerFilter.predict's own range %.4f ms, WienerCascade.predict's %.4f ms (%s)" %
                 (diff, cell["filter_range"], cell["cascade_range"], "met" if cell["met"] else "MISSED"))
    res["predict"] = cell
    return cell["met"]


def hand_loop(x, y, lead, alphas, degrees, F):
    """what a user writes today: everything on the device except the polynomial fit"""
    rows, T = x.shape
    n = T - lead - (L - 1)
    fr = wiener.fold_ranges(n, F, L - 1)
    st = wiener.stats(x, y, L, lead, ranges=fr)
    res = {}
    for i in range(F):
        v, t = i, (i + 1) % F
        train = [k for k in range(F) if k not in (v, t)]
        tot = sum(st[k] for k in train)
        for al in alphas:
            f = wiener.WienerFilter(al).fit(tot)
            pred = f.predict(x)[:, :n]
            host = pred.cpu().numpy().astype(np.float64)
            yh = y[:, L - 1 + lead:].cpu().numpy().astype(np.float64)
            idx = np.concatenate([np.arange(fr[k][0], fr[k][1]) for k in train]) - (L - 1)
            for d in degrees:
                coef = torch.tensor(np.stack([np.polyfit(host[k, idx], yh[k, idx], d) for k in range(K)]), dtype=torch.float32, device="cuda")
                q = coef[:, 0:1].expand(-1, n).clone()
                for j in range(1, d + 1):
                    q = q * pred + coef[:, j:j + 1]
                out = []
                for fold in (v, t):
                    lo, hi = fr[fold][0] - (L - 1), fr[fold][1] - (L - 1)
                    pp, tt = q[:, lo:hi].double(), y[:, lo + L - 1 + lead:hi + L - 1 + lead].double()
                    rmse = torch.sqrt(((pp - tt) ** 2).mean(1))
                    pc, tc = pp - pp.mean(1, keepdim=True), tt - tt.mean(1, keepdim=True)
                    out += [rmse, (pc * tc).sum(1) / torch.sqrt((pc * pc).sum(1) * (tc * tc).sum(1))]
                res.setdefault((al, d), []).append(torch.stack(out))
    return {k: torch.stack(v) for k, v in res.items()}                  # [F, 4, K]: rmse_valid, cc_valid, rmse_test, cc_test


def clock(f, reps):
    f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(min=round(min(ts), 4), median=round(float(np.median(ts)), 4), max=round(max(ts), 4), runs=reps)


def part3(a, lines, res, note):
    rows, T, lead, F = 96, 72000, 0, 5
    alphas, degrees = (0.0, 1e-2, 1.0), (2, 3, 4)
    x = counts_matrix(rows, T)
    g = torch.Generator(device="cuda").manual_seed(5)
    z = (torch.randn((K, rows), generator=g, device="cuda") @ torch.roll(x.float(), 2, 1))
    y = (z + 0.15 * z * z + torch.randn((K, T), generator=g, device="cuda")).float().contiguous()
    got = cascade.cross_validate(x, y, L, lead, None, alphas, degrees, F)
    want = hand_loop(x, y, lead, alphas, degrees, F)
    for key, w in want.items():
        for j, name in enumerate(("rmse_valid", "cc_valid", "rmse_test", "cc_test")):
            assert torch.allclose(got[key][name], w[:, j], rtol=1e-4, atol=0), (key, name)
    note("results agree")
    reps = max(3, min(a.reps, 10))
    cv, hand = [], []
    for _ in range(reps):                                               # alternated, host clock around a synchronise
        cv.append(clock(lambda: cascade.cross_validate(x, y, L, lead, None, alphas, degrees, F), 1)["median"])
        hand.append(clock(lambda: hand_loop(x, y, lead, alphas, degrees, F), 1)["median"])
    sp = lambda v: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4), max=round(max(v), 4), runs=len(v))  # noqa: E731
    t = dict(cross_validate=sp(cv), hand=sp(hand))
    # where cross_validate's time goes: its pieces, each timed alone
    n = T - lead - (L - 1)
    fr = wiener.fold_ranges(n, F, L - 1)
    st = wiener.stats(x, y, L, lead, ranges=fr)
    tot = st[2] + st[3] + st[4]
    c = cascade.WienerCascade(1e-2, 4)
    c.linear.fit(tot)
    c.center, c.scale = cascade._linear_spread(tot, c.linear)
    pred = c.linear.predict(x)
    p, tg, _n = c._targets(pred, y)
    tr, held = c._columns(fr[2:], n), c._columns(fr[:2], n)
    m = cascade.moments(p, tg, tr, 4, c.center, c.scale).total()
    tmp = torch.empty_like(pred)
    pieces = dict(stats=(1, lambda: wiener.stats(x, y, L, lead, ranges=fr)),
                  solve=(F * len(alphas), lambda: (wiener.WienerFilter(1e-2).fit(tot), cascade._linear_spread(tot, c.linear))),
                  fir=(F * len(alphas), lambda: c.linear.predict(x)),
                  moments_train=(F * len(alphas), lambda: cascade.moments(p, tg, tr, 4, c.center, c.scale).total()),
                  polyfit=(F * len(alphas) * len(degrees), lambda: cascade.polyfit(m, 3)),
                  polyval=(F * len(alphas) * len(degrees), lambda: c._apply(pred, c_coef, tmp)),
                  moments_held=(F * len(alphas) * len(degrees), lambda: (lambda s: (s.rmse(), s.cc()))(cascade.moments(p, tg, held, 1))))
    c_coef = cascade.polyfit(m, 3)
    split, known = {}, 0.0
    for name, (count, f) in pieces.items():
        one = clock(f, reps)["median"]
        split[name] = dict(calls=count, each_ms=one, total_ms=round(count * one, 4))
        known += count * one
    split["rest"] = dict(calls=1, each_ms=round(t["cross_validate"]["median"] - known, 4), total_ms=round(t["cross_validate"]["median"] - known, 4))
    lines.append("3  cross_validate, %d x %d, %d lags, %d folds, alphas %s, degrees %s (host clock, synchronised)" % (rows, T, L, F, alphas, degrees))
    lines.append(line("cascade.cross_validate", t["cross_validate"]))
    lines.append(line("the loop by hand", t["hand"]))
    lines.append("    by hand / cross_validate x%.2f; cross_validate's pieces, each timed alone (calls x ms = ms):" %
                 (t["hand"]["median"] / t["cross_validate"]["median"]))
    for name, s in split.items():
        lines.append("      %-14s %3d x %9.4f = %10.4f" % (name, s["calls"], s["each_ms"], s["total_ms"]))
    res["cross_validate"] = dict(t, split=split)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--budget", type=float, default=60.0, help="seconds of timed rounds per group of alternated routes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_cascade.txt"))
    a = ap.parse_args()
    info = muahuff.device_info(0)
    lines = ["bench_cascade: %s (%s), %d alternated runs" % (info["name"], info["arch"], a.reps)]
    res, met = {}, True
    note = lambda what: print(what, file=sys.stderr, flush=True)  # noqa: E731
    for part, f in (("1", part1), ("2", part2), ("3", part3)):
        if part in a.parts.split(","):
            met = f(a, lines, res, note) and met
            torch.cuda.empty_cache()
            note("part %s done" % part)
    lines.append("conditions (moments < (t) at both sizes; the two predicts within WienerFilter.predict's own range): %s" % ("met" if met else "MISSED"))
    lines.append(json.dumps(dict(cells={k: v for k, v in res.items()}, conditions_met=met), sort_keys=True, default=str))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
