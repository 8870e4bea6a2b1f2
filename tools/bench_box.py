"""The moving-average window's kernels and drivers (mhs_box, mhs_box_f32; wiener.stats(window=), WienerFilter.predict,
cascade.cross_validate(window=)) against the routes a user has without them.

Same process, the routes alternated after warm-up (20 runs each, fewer where 20 rounds of a group would take more than
--budget seconds: the count stands next to every figure; median and range), device events unless it says host clock:
  1  mhs_box at 1024 ch x 1e7 bins and 96 x 72 000, (window, clip) = (50, 3) on one plane and (200, 39) on two, against two
     torch routes that give the same planes: (c) clamp, int32 cumsum in column chunks, difference, byte split; (p) clamp,
     float32 avg_pool1d, times the window, round, byte split.  Results compared first.  Condition, no margin: median(mhs_box)
     below the median of the FASTER torch route in every cell.  Reported: the bytes moved by design, rows * cols *
     (1 + planes), as a share of the 8 TB/s spec; a third cell, (4, 39), for the small windows of the 50-ms bin width; and
     a plain device copy of the same bytes into one plane, the floor any one-plane form has.
  2  wiener.stats with each window against window = 1 at the same clip, 96 x 72 000 and 1024 x 1e6, 15 lags, 2 covariates
     (host clock around a synchronise).  Reported next to what the call counts predict: (4L - 1) / L mhi_gram calls for two
     planes, 1 for one, plus the box pass.  No condition.
  3  WienerFilter.predict with window = 50 against window = 1 at 1024 x 1e7: the difference; and mhs_box_f32 alone against
     a float64 cumsum difference in torch on the same [2, n].  Condition: median(mhs_box_f32) below that route's.
  4  cascade.cross_validate(window = 50) at 96 x 72 000 (5 folds, 3 alphas, degrees 2..4) against the loop by hand that
     smooths the explicit [n, 1440] float64 design on the device (host clock), and where cross_validate's time goes.
Prints the table and writes it to --out (default profiles/r20_box.txt).

    python tools/bench_box.py [--reps 20] [--parts 1,2,3,4] [--out FILE]
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
from muahuff import _smooth, cascade, smooth, wiener  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_cascade import clock  # noqa: E402
from bench_events_out import counts_matrix  # noqa: E402
from bench_wiener import alternate, line  # noqa: E402

SPEC_BW = 8e12       # bytes per second
L, K = 15, 2
CHUNK = 1 << 18      # columns per chunk of the torch routes: [1024, CHUNK] int32 is 1 GiB


def _split(box, lo, hi, a, b):
    lo[:, a:b] = (box & 255).to(torch.uint8)
    if hi is not None:
        hi[:, a:b] = (box >> 8).to(torch.uint8)


def torch_cumsum(x, n, w, q, lo, hi):
    """(c): per chunk of output columns, clamp the chunk and its halo, int32 cumsum, difference, byte split"""
    for a in range(0, n, CHUNK):
        b = min(a + CHUNK, n)
        cs = torch.cumsum(torch.clamp(x[:, a:b + w - 1], max=q).to(torch.int32), 1, dtype=torch.int32)
        box = cs[:, w - 1:].clone()
        box[:, 1:] -= cs[:, :b - a - 1]
        _split(box, lo, hi, a, b)


def torch_pool(x, n, w, q, lo, hi):
    """(p): per chunk, clamp, float32 avg_pool1d over the window, times the window, round, byte split"""
    for a in range(0, n, CHUNK):
        b = min(a + CHUNK, n)
        seg = torch.clamp(x[:, a:b + w - 1], max=q).to(torch.float32).unsqueeze(0)
        box = torch.round(torch.nn.functional.avg_pool1d(seg, w, 1) * w).squeeze(0).to(torch.int32)
        _split(box, lo, hi, a, b)


def part1(a, lines, res, note):
    met = True
    for rows, T in ((1024, 10 ** 7), (96, 72000)):
        x = counts_matrix(rows, T)
        for w, q in ((50, 3), (200, 39), (4, 39)):
            n, two = T - w + 1, w * q > 255
            lo, hi = smooth.planes(rows, n, two, x.device)
            tl, th = smooth.planes(rows, n, two, x.device)
            box = lambda: smooth.enqueue(x, rows, n, w, q, lo, hi)  # noqa: E731
            box()
            for name, route in (("c", torch_cumsum), ("p", torch_pool)):
                route(x, n, w, q, tl, th)
                assert torch.equal(lo, tl) and (not two or torch.equal(hi, th)), (rows, T, w, q, name)
            t = alternate([("box", box), ("c", lambda: torch_cumsum(x, n, w, q, tl, th)), ("p", lambda: torch_pool(x, n, w, q, tl, th)),
                           ("copy", lambda: tl.copy_(x[:, :n]))], a.reps, a.budget, note)
            best = min(("c", "p"), key=lambda k: t[k]["median"])
            nbytes = rows * n * (1 + (2 if two else 1))
            cell = dict(t, faster=best, bytes=nbytes, faster_over_box=round(t[best]["median"] / t["box"]["median"], 2),
                        spec_share=round(nbytes / (t["box"]["median"] * 1e-3) / SPEC_BW, 4), met=bool(t["box"]["median"] < t[best]["median"]))
            met = met and cell["met"]
            lines.append("1  box sums, %d x %d, window %d, clip %d, %d plane%s" % (rows, T, w, q, 2 if two else 1, "s" if two else ""))
            lines.append(line("mhs_box", t["box"]))
            lines.append(line("(c) torch int32 cumsum", t["c"]))
            lines.append(line("(p) torch avg_pool1d", t["p"]))
            lines.append(line("a plain copy of x", t["copy"]))
            lines.append("    faster torch route (%s) / mhs_box x%.2f (%s)   %.1f MB by design: %.4f of the 8 TB/s spec at the median" %
                         (best, cell["faster_over_box"], "met" if cell["met"] else "MISSED", nbytes / 1e6, cell["spec_share"]))
            res["box_%dx%d_w%d" % (rows, T, w)] = cell
            del lo, hi, tl, th
            torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()
    return met


def part2(a, lines, res, note):
    reps = max(3, min(a.reps, 5))
    for rows, T in ((96, 72000), (1024, 10 ** 6)):
        x = counts_matrix(rows, T)
        g = torch.Generator(device="cuda").manual_seed(5)
        y = torch.randn((K, T), generator=g, device="cuda", dtype=torch.float32)
        for w, q in ((50, 3), (200, 39)):
            two = w * q > 255
            base = clock(lambda: wiener.stats(x, y, L, 0, q), reps)
            win = clock(lambda: wiener.stats(x, y, L, 0, q, window=w), reps)
            n = T - w + 1
            lo, hi = smooth.planes(rows, n, two, x.device)
            box = clock(lambda: smooth.enqueue(x, rows, n, w, q, lo, hi), reps)
            del lo, hi
            predicted = (4 * L - 1) / L if two else 1.0
            cell = dict(window1=base, window=win, box_pass=box, ratio=round(win["median"] / base["median"], 2), gram_calls_ratio=round(predicted, 2))
            lines.append("2  wiener.stats, %d x %d, %d lags, %d covariates, window %d, clip %d (host clock, synchronised)" % (rows, T, L, K, w, q))
            lines.append(line("window = 1", base))
            lines.append(line("window = %d" % w, win))
            lines.append(line("one mhs_box over it all", box))
            lines.append("    window / window 1 x%.2f; the mhi_gram call counts predict x%.2f, plus the box pass" % (cell["ratio"], predicted))
            res["stats_%dx%d_w%d" % (rows, T, w)] = cell
            torch.cuda.empty_cache()
        del x, y
        torch.cuda.empty_cache()
    return True


def torch_box_f64(p, w, bias, out):
    """the float64 cumsum difference on [k, n] with zeros in front, plus the bias"""
    cs = torch.cumsum(p.double(), 1)
    box = cs.clone()
    box[:, w:] -= cs[:, :-w]
    out.copy_(box + bias.double()[:, None])


def part3(a, lines, res, note):
    rows, T, w = 1024, 10 ** 7, 50
    x = counts_matrix(rows, T)
    g = torch.Generator(device="cuda").manual_seed(5)
    f = wiener.WienerFilter(0.0)
    f.weights = (torch.randn((K, L, rows), generator=g, device="cuda", dtype=torch.float32) / rows).double()
    f.bias = torch.zeros((K,), dtype=torch.float64, device="cuda")   # (so that window 1's output is the other's input)
    f.lags, f.lead, f.clip, f.channels, f.window = L, 0, 255, rows, 1
    fw = wiener.WienerFilter(0.0)
    fw.weights, fw.bias = f.weights, f.bias
    fw.lags, fw.lead, fw.clip, fw.channels, fw.window = L, 0, 255, rows, w
    raw = f.predict(x)
    bias32 = torch.randn((K,), generator=g, device="cuda", dtype=torch.float32)
    out, ref = torch.empty_like(raw), torch.empty_like(raw)
    zero = torch.zeros_like(bias32)
    _smooth.box_f32(raw, w, zero, out)
    torch_box_f64(raw, w, zero, ref)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
    assert torch.equal(fw.predict(x), out)
    t = alternate([("w1", lambda: f.predict(x)), ("w50", lambda: fw.predict(x))], a.reps, a.budget, note)
    u = alternate([("box_f32", lambda: _smooth.box_f32(raw, w, bias32, out)), ("t", lambda: torch_box_f64(raw, w, bias32, ref))], a.reps, a.budget, note)
    cell = dict(predict=t, box=u, predict_difference=round(t["w50"]["median"] - t["w1"]["median"], 4),
                t_over_box_f32=round(u["t"]["median"] / u["box_f32"]["median"], 2), met=bool(u["box_f32"]["median"] < u["t"]["median"]))
    lines.append("3  predict, %d x %d, %d lags, %d outputs" % (rows, T, L, K))
    lines.append(line("window = 1", t["w1"]))
    lines.append(line("window = %d" % w, t["w50"]))
    lines.append("    the window adds %.4f ms at the median" % cell["predict_difference"])
    lines.append(line("mhs_box_f32 alone", u["box_f32"]))
    lines.append(line("(t) torch float64 cumsum", u["t"]))
    lines.append("    (t) / mhs_box_f32 x%.2f (%s)" % (cell["t_over_box_f32"], "met" if cell["met"] else "MISSED"))
    res["predict"] = cell
    return cell["met"]


def hand_loop(x, y, w, lead, alphas, degrees, F):
    """what a user writes without stats(window=): the explicit lag-stacked design in float64, smoothed down its rows with
    zeros in front, and per fold z-scoring, the ridge's normal equations, np.polyfit on the host and the scores"""
    rows, T = x.shape
    n = T - lead - (L - 1)
    X = torch.cat([x[:, L - 1 - l:L - 1 - l + n].t() for l in range(L)], 1).double()        # [n, L * rows]
    cs = torch.cumsum(X, 0)
    X = cs.clone()
    X[w:] -= cs[:-w]
    del cs
    Y = y[:, L - 1 + lead:L - 1 + lead + n].t().double()
    fr = wiener.fold_ranges(n, F)
    res = {}
    for i in range(F):
        v, t = i, (i + 1) % F
        idx = torch.cat([torch.arange(fr[k][0], fr[k][1], device=x.device) for k in range(F) if k not in (v, t)])
        Xt, Yt = X[idx], Y[idx]
        mean, std = Xt.mean(0), Xt.std(0, unbiased=False)
        Z = (Xt - mean) / std
        ztz, ybar = Z.t() @ Z, Yt.mean(0)
        zty = Z.t() @ (Yt - ybar)
        for al in alphas:
            wz = torch.linalg.solve(ztz + al * torch.eye(ztz.shape[0], dtype=torch.float64, device=x.device), zty)
            pred = ((X - mean) / std) @ wz + ybar                                       # [n, K]
            host, yh, hidx = pred.cpu().numpy(), Y.cpu().numpy(), idx.cpu().numpy()
            for d in degrees:
                coef = torch.tensor(np.stack([np.polyfit(host[hidx, k], yh[hidx, k], d) for k in range(K)]), dtype=torch.float64, device=x.device)
                q = coef[:, 0].expand(n, -1).clone()
                for j in range(1, d + 1):
                    q = q * pred + coef[:, j]
                out = []
                for fold in (v, t):
                    pp, tt = q[fr[fold][0]:fr[fold][1]], Y[fr[fold][0]:fr[fold][1]]
                    rmse = torch.sqrt(((pp - tt) ** 2).mean(0))
                    pc, tc = pp - pp.mean(0, keepdim=True), tt - tt.mean(0, keepdim=True)
                    out += [rmse, (pc * tc).sum(0) / torch.sqrt((pc * pc).sum(0) * (tc * tc).sum(0))]
                res.setdefault((al, d), []).append(torch.stack(out))
    return {k: torch.stack(v) for k, v in res.items()}                  # [F, 4, K]: rmse_valid, cc_valid, rmse_test, cc_test


def part4(a, lines, res, note):
    rows, T, lead, F, w = 96, 72000, 0, 5, 50
    alphas, degrees = (1e-4, 1e-2, 1.0), (2, 3, 4)
    x = counts_matrix(rows, T)
    g = torch.Generator(device="cuda").manual_seed(5)
    z = (torch.randn((K, rows), generator=g, device="cuda") @ torch.roll(x.float(), 2, 1))
    y = (z + 0.15 * z * z + torch.randn((K, T), generator=g, device="cuda")).float().contiguous()
    got = cascade.cross_validate(x, y, L, lead, None, alphas, degrees, F, window=w)
    want = hand_loop(x, y, w, lead, alphas, degrees, F)
    worst = 0.0
    for key, wv in want.items():
        for j, name in enumerate(("rmse_valid", "cc_valid", "rmse_test", "cc_test")):
            worst = max(worst, float(((got[key][name] - wv[:, j]).abs() / wv[:, j].abs()).max()))
    note("results differ by at most %.3g (relative)" % worst)
    assert worst < 1e-2, worst
    reps = max(3, min(a.reps, 10))
    cv, hand = [], []
    for _ in range(reps):                                               # alternated, host clock around a synchronise
        cv.append(clock(lambda: cascade.cross_validate(x, y, L, lead, None, alphas, degrees, F, window=w), 1)["median"])
        hand.append(clock(lambda: hand_loop(x, y, w, lead, alphas, degrees, F), 1)["median"])
    sp = lambda v: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4), max=round(max(v), 4), runs=len(v))  # noqa: E731
    t = dict(cross_validate=sp(cv), hand=sp(hand))
    n = T - lead - (L - 1)
    fr = wiener.fold_ranges(n, F, L - 1)
    st = wiener.stats(x, y, L, lead, ranges=fr, window=w)
    tot = st[2] + st[3] + st[4]
    fl = wiener.WienerFilter(1e-2).fit(tot)
    pieces = dict(stats=(1, lambda: wiener.stats(x, y, L, lead, ranges=fr, window=w)),
                  stats_window1=(0, lambda: wiener.stats(x, y, L, lead, ranges=fr)),
                  solve=(F * len(alphas), lambda: wiener.WienerFilter(1e-2).fit(tot)),
                  predict=(F * len(alphas), lambda: fl.predict(x)))
    split, known = {}, 0.0
    for name, (count, f) in pieces.items():
        one = clock(f, reps)["median"]
        split[name] = dict(calls=count, each_ms=one, total_ms=round(count * one, 4))
        known += count * one
    split["rest"] = dict(calls=1, each_ms=round(t["cross_validate"]["median"] - known, 4), total_ms=round(t["cross_validate"]["median"] - known, 4))
    lines.append("4  cross_validate, window %d, %d x %d, %d lags, %d folds, alphas %s, degrees %s (host clock, synchronised)" % (w, rows, T, L, F, alphas, degrees))
    lines.append(line("cascade.cross_validate", t["cross_validate"]))
    lines.append(line("the loop by hand", t["hand"]))
    lines.append("    by hand / cross_validate x%.2f; results differ by at most %.3g; cross_validate's pieces, each timed alone (calls x ms = ms;"
                 % (t["hand"]["median"] / t["cross_validate"]["median"], worst))
    lines.append("    stats_window1 is not part of it: the same pass without the window, for comparison; rest: moments, polynomials, host work):")
    for name, s in split.items():
        lines.append("      %-14s %3d x %9.4f = %10.4f" % (name, s["calls"], s["each_ms"], s["total_ms"]))
    res["cross_validate"] = dict(t, split=split, worst_relative_difference=worst)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parts", default="1,2,3,4")
    ap.add_argument("--budget", type=float, default=30.0, help="seconds of timed rounds per group of alternated routes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_box.txt"))
    a = ap.parse_args()
    info = muahuff.device_info(0)
    lines = ["bench_box: %s (%s), %d alternated runs" % (info["name"], info["arch"], a.reps)]
    res, met = {}, True
    note = lambda what: print(what, file=sys.stderr, flush=True)  # noqa: E731
    for part, f in (("1", part1), ("2", part2), ("3", part3), ("4", part4)):
        if part in a.parts.split(","):
            met = f(a, lines, res, note) and met
            torch.cuda.empty_cache()
            note("part %s done" % part)
    lines.append("conditions (mhs_box below the faster torch route in every cell; mhs_box_f32 below the float64 cumsum): %s" % ("met" if met else "MISSED"))
    lines.append(json.dumps(dict(cells={k: v for k, v in res.items()}, conditions_met=met), sort_keys=True, default=str))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
