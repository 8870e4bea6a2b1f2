"""The dynamic-range sweep (mhq_gram_clips, mhq_xty_clips; wiener.stats_clips, cascade.sweep_clips) against the route a
user had without it: the Python loop `for q in clips: wiener.stats(..., clip=q, ranges=folds)` and the loop of
cascade.cross_validate(clip=q).

Same process, the routes alternated after warm-up (20 runs each, fewer where 20 rounds of a group would take more than
--budget seconds: the count stands next to every figure; median and range), device events unless it says host clock.
Results are compared first (torch.equal).
  A  the study's shape: 96 ch x 72 000 bins, 15 lags, 2 covariates, lead 2, five folds, clips 2..39.
     A1 stats_clips against the loop of stats.  Condition: the two routes' run ranges are disjoint, the fused one below.
     A2 the launches alone: ONE mhq_gram_clips against the 190 clamped copies and 2 850 mhi_gram it replaces, ONE
        mhq_xty_clips against 190 mhw_xty, buffers allocated up front.
     A3 sweep_clips against the loop of cross_validate at alphas (0, 1e-4, 1e-2), degrees (2, 3, 4) (host clock), and where
        the rest of sweep_clips' time goes: the solves, mhw_fir, the moments and polynomials.
  B  a device-filling shape: 1024 ch x 1e6 bins, 5 lags, clips (2, 3, 5, 9), one range.  Reported, not gated.
Prints the table and writes it to --out (default profiles/r21_clips.txt).

    python tools/bench_clips.py [--reps 20] [--parts A1,A2,A3,B] [--out FILE]
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
from muahuff import _sweep, _wiener, cascade, wiener  # noqa: E402
from muahuff.gram import enqueue  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_cascade import clock  # noqa: E402
from bench_events_out import counts_matrix  # noqa: E402
from bench_wiener import alternate, line  # noqa: E402

K = 2
FIELDS = ("gram", "sum_x", "xty", "sum_y", "sum_yy")


def world(rows, T, lead):
    """counts with a few values on either side of every clip, covariates that follow them non-linearly (bench_cascade)"""
    x = counts_matrix(rows, T)
    g = torch.Generator(device="cuda").manual_seed(5)
    big = torch.rand((rows, T), generator=g, device="cuda") < 0.01
    x[big] = torch.randint(0, 64, (int(big.sum()),), generator=g, device="cuda").to(torch.uint8)
    z = torch.randn((K, rows), generator=g, device="cuda") @ torch.roll(torch.clamp(x, max=4).float(), lead + 2, 1)
    y = (z + 0.15 * z * z + torch.randn((K, T), generator=g, device="cuda")).float().contiguous()
    return x, y


def loop_stats(x, y, L, lead, clips, ranges):
    return [(q, wiener.stats(x, y, L, lead, clip=q, ranges=ranges)) for q in clips]


def same(a, b):
    for (qa, pa), (qb, pb) in zip(a, b):
        assert qa == qb and len(pa) == len(pb)
        for s, w in zip(pa, pb):
            assert s.n == w.n and all(torch.equal(getattr(s, f), getattr(w, f)) for f in FIELDS), qa


def compare(label, fused, loop, a, lines, res, note, key):
    """the two routes alternated; -> met: the run ranges are disjoint, the fused one below"""
    t = alternate([("fused", fused), ("loop", loop)], a.reps, a.budget, note)
    met = bool(t["fused"]["max"] < t["loop"]["min"])
    ratio = t["loop"]["median"] / t["fused"]["median"]
    lines.append(line(label + ", fused", t["fused"]))
    lines.append(line(label + ", loop", t["loop"]))
    lines.append("    loop / fused x%.2f at the medians; the run ranges %s" % (ratio, "are disjoint, the fused one below" if met else
                                                                               "OVERLAP or the loop is faster"))
    res[key] = dict(t, ratio=round(ratio, 3), disjoint_and_faster=met)
    return met


def part_a(a, lines, res, note, parts):
    rows, T, L, lead, F = 96, 72000, 15, 2, 5
    clips = list(range(2, 40))
    x, y = world(rows, T, lead)
    fr = wiener.fold_ranges(T - lead - (L - 1), F, L - 1)
    met = True
    lines.append("A  %d x %d, %d lags, %d covariates, lead %d, %d folds, clips %d..%d" % (rows, T, L, K, lead, F, clips[0], clips[-1]))
    if "A1" in parts:
        same(wiener.stats_clips(x, y, L, lead, clips, ranges=fr), loop_stats(x, y, L, lead, clips, fr))
        note("A1: the statistics are equal")
        met = compare("A1 the statistics", lambda: wiener.stats_clips(x, y, L, lead, clips, ranges=fr),
                      lambda: loop_stats(x, y, L, lead, clips, fr), a, lines, res, note, "A1_stats") and met
    if "A2" in parts:
        R, n = len(fr), len(clips)
        base = torch.zeros((R, n, L, rows, rows), dtype=torch.int64, device="cuda")
        s0 = torch.zeros((R, n, rows), dtype=torch.int64, device="cuda")
        xt = torch.empty((R, n, L, rows, K), dtype=torch.float64, device="cuda")
        one = torch.empty((L, rows, K), dtype=torch.float64, device="cuda")
        scr = torch.empty((_sweep.xty_clips_scratch_bytes(rows, T, L, K, R, n),), dtype=torch.uint8, device="cuda")
        longest = max(b - c for c, b in fr)
        scr1 = torch.empty((_wiener.xty_scratch_bytes(rows, longest, L, K),), dtype=torch.uint8, device="cuda")
        view = torch.empty((rows, longest + L - 1), dtype=torch.uint8, device="cuda")

        def gram_fused():
            _sweep.gram_clips(x.data_ptr(), x.stride(0), rows, T, fr, clips, L, base, s0)

        def gram_loop():                                            # what wiener._range_stats launches, without its allocations
            for i, q in enumerate(clips):
                for r, (t0, t1) in enumerate(fr):
                    nb = t1 - t0
                    v = view[:, :nb + L - 1]
                    torch.clamp(x[:, t0 - (L - 1):t1], max=q, out=v)
                    enqueue(v, rows, nb, None, 0, base[r, i, 0], s0[r, i], None, True, L - 1)
                    for d in range(1, L):
                        enqueue(v, rows, nb, v, rows, base[r, i, d], None, None, True, L - 1, L - 1 - d)

        def xty_fused():
            _sweep.xty_clips(x.data_ptr(), x.stride(0), rows, T, fr, clips, L, lead, y.data_ptr(), 4 * y.stride(0), K, xt, scr)

        def xty_loop():
            for q in clips:
                for t0, t1 in fr:
                    _wiener.xty(x.data_ptr() + t0 - (L - 1), x.stride(0), rows, t1 - t0, L, q, y.data_ptr() + 4 * (t0 + lead),
                                4 * y.stride(0), K, one, scr1)

        base.zero_(), s0.zero_()
        gram_fused()
        want = base.clone()
        base.zero_(), s0.zero_()
        gram_loop()
        assert torch.equal(base, want)
        note("A2: the count products are equal")
        compare("A2 mhq_gram_clips", gram_fused, gram_loop, a, lines, res, note, "A2_gram")
        compare("A2 mhq_xty_clips", xty_fused, xty_loop, a, lines, res, note, "A2_xty")
        del base, s0, xt, want
    if "A3" in parts:
        alphas, degrees = (0.0, 1e-4, 1e-2), (2, 3, 4)
        got = cascade.sweep_clips(x, y, L, lead, clips, alphas, degrees, F)
        for q in (clips[0], clips[-1]):
            want = cascade.cross_validate(x, y, L, lead, q, alphas, degrees, F)
            assert all(torch.equal(got[q][k][nm], w) for k, arr in want.items() for nm, w in arr.items()), q
        note("A3: the scores are equal")
        reps = max(3, min(a.reps, 5))
        fused, loop = [], []
        for _ in range(reps):                                       # alternated, host clock around a synchronise
            fused.append(clock(lambda: cascade.sweep_clips(x, y, L, lead, clips, alphas, degrees, F), 1)["median"])
            loop.append(clock(lambda: {q: cascade.cross_validate(x, y, L, lead, q, alphas, degrees, F) for q in clips}, 1)["median"])
        sp = lambda v: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4), max=round(max(v), 4), runs=len(v))  # noqa: E731
        t = dict(fused=sp(fused), loop=sp(loop))
        # where the rest goes: one clip's folds by hand, every piece timed alone (host clock), times the clips
        st = wiener.stats(x, y, L, lead, clips[0], ranges=fr)
        tot = st[0] + st[1] + st[2]
        f = wiener.WienerFilter(1e-2).fit(tot)
        per = F * len(alphas)
        stats_ms = clock(lambda: wiener.stats_clips(x, y, L, lead, clips, ranges=fr), reps)["median"]
        solve_ms = clock(lambda: wiener.WienerFilter(1e-2).fit(tot), reps)["median"] * per * len(clips)
        fir_ms = clock(lambda: f.predict(x), reps)["median"] * per * len(clips)
        total = t["fused"]["median"]
        rest = total - stats_ms - solve_ms - fir_ms
        lines.append(line("A3 sweep_clips (host clock)", t["fused"]))
        lines.append(line("A3 loop of cross_validate", t["loop"]))
        lines.append("    loop / fused x%.2f at the medians" % (t["loop"]["median"] / total))
        lines.append("    of sweep_clips' %.1f ms: the statistics %.1f (%.0f %%), %d solves %.1f (%.0f %%), %d mhw_fir %.1f (%.0f %%), the sum of "
                     "fold statistics, moments, polynomials and scores %.1f (%.0f %%); pieces timed alone" %
                     (total, stats_ms, 100 * stats_ms / total, per * len(clips), solve_ms, 100 * solve_ms / total, per * len(clips), fir_ms,
                      100 * fir_ms / total, rest, 100 * rest / total))
        res["A3_sweep"] = dict(t, ratio=round(t["loop"]["median"] / total, 3), stats_ms=stats_ms, solve_ms=solve_ms, fir_ms=fir_ms, rest_ms=rest)
    return met


def part_b(a, lines, res, note):
    rows, T, L, lead = 1024, 10 ** 6, 5, 0
    clips = [2, 3, 5, 9]
    x, y = world(rows, T, lead)
    lines.append("B  %d x %d, %d lags, %d covariates, one range, clips %s (reported, not gated)" % (rows, T, L, K, clips))
    same(wiener.stats_clips(x, y, L, lead, clips), loop_stats(x, y, L, lead, clips, None))
    note("B: the statistics are equal")
    compare("B the statistics", lambda: wiener.stats_clips(x, y, L, lead, clips), lambda: loop_stats(x, y, L, lead, clips, None), a, lines, res,
            note, "B_stats")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parts", default="A1,A2,A3,B")
    ap.add_argument("--budget", type=float, default=60.0, help="seconds of timed rounds per group of alternated routes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_clips.txt"))
    a = ap.parse_args()
    parts = [p for p in a.parts.split(",") if p]
    info = muahuff.device_info(0)
    lines = ["bench_clips: %s (%s), %d alternated runs" % (info["name"], info["arch"], a.reps)]
    res, met = {}, True
    note = lambda s: print("  .. " + s, flush=True)  # noqa: E731
    if any(p.startswith("A") for p in parts):
        met = part_a(a, lines, res, note, parts)
        torch.cuda.empty_cache()
    if "B" in parts:
        part_b(a, lines, res, note)
    lines.append("condition A (A1: run ranges disjoint, stats_clips below the loop): %s" % ("met" if met else "MISSED"))
    lines.append(json.dumps(res, sort_keys=True))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
