"""Decoders fitted from a recording file (archive.Reader.bins -> wiener.stats_from, cascade.cross_validate_from) against
the route a user had before: read() the whole range into a resident matrix, then wiener.stats / cascade.cross_validate
on it.  Same file, same process, fresh Readers, the two routes alternated after one warm-up round (host clock,
synchronised: both routes read the file and synchronise per batch anyway); median and range of --reps runs, and
torch.cuda.max_memory_allocated of each route with the covariates resident in both.  Results are compared first: the
integers equal, the float sums close.

Shapes: an archive of one block of 96 ch x 72 000 steps, and one of --blocks blocks of 1024 ch x (1e6 / blocks) steps.
Settings: bin None and 50, 15 lags, clip 3, windows 1 and 50; five folds, alphas 1e-2 and 1, degrees None and 3.  The
file route's budget is --max-bytes, or a quarter of the binned matrix where that is smaller, so that it always walks
several batches.
cross_validate needs lags * channels <= 16384 features five times over, so at 1024 channels it runs on the first
--cv-channels of them.  Nothing here is a condition: the figures are reported.
Prints the table and writes it to --out (default profiles/r23_file_fit.txt).

    python tools/bench_file_fit.py [--reps 5] [--shapes 96x72000x1,1024x1000000x20] [--max-bytes N] [--dir DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import archive, cascade, wiener  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_events_out import counts_matrix  # noqa: E402

K, LAGS, CLIP, FOLDS, ALPHAS, DEGREES = 2, 15, 3, 5, (1e-2, 1.0), (None, 3)   # no alpha 0: at bin 50 a fold has fewer rows than features


def covariates(x):
    """K mixtures of the first channels two bins earlier, plus noise: float32 on x's bin grid"""
    g = torch.Generator(device="cuda").manual_seed(7)
    n = min(8, x.shape[0])
    mix = torch.randn((K, n), generator=g, device="cuda")
    drive = mix @ torch.roll(x[:n].float(), 2, 1)
    return (drive + 0.5 * torch.randn(drive.shape, generator=g, device="cuda")).contiguous()


def timed(fns, reps, note):
    """[(name, f)] -> {name: min / median / max seconds, peak bytes}, the routes alternated after one warm-up round"""
    ts, peak = {k: [] for k, _f in fns}, {}
    for i in range(reps + 1):
        for k, f in fns:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if i:
                ts[k].append(time.perf_counter() - t0)
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
        note("round %d of %d" % (i, reps))
    return {k: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4), max=round(max(v), 4), runs=len(v), peak_bytes=peak[k])
            for k, v in ts.items()}


def line(label, t):
    return "    %-34s min %9.4f median %9.4f max %9.4f s  (%d runs)  peak %8.1f MiB" % (label, t["min"], t["median"], t["max"], t["runs"],
                                                                                     t["peak_bytes"] / 2 ** 20)


def close(a, b):
    for s, r in zip(a, b):
        assert s.n == r.n and torch.equal(s.gram, r.gram) and torch.equal(s.sum_x, r.sum_x)
        assert torch.allclose(s.xty, r.xty, rtol=1e-9, atol=1e-6)


def shape(a, C, T, blocks, lines, res, note):
    Tb = T // blocks
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        fn = os.path.join(d, "rec.mua")
        with archive.create(fn, C, S=3, exact=True) as w:
            for i in range(blocks):
                w.append(counts_matrix(C, Tb, seed=60 + i).t().contiguous())
        lines.append("archive of %d block%s of %d ch x %d steps (%d bytes)" % (blocks, "" if blocks == 1 else "s", C, Tb, os.path.getsize(fn)))
        for r in (None, 50):
            n = T // (r or 1)
            mb = min(a.max_bytes, C * (n // 4 + 1))
            with archive.open(fn) as rd:
                y = covariates(rd.read(0, n * (r or 1), bin=r)[:, :n])
            cv_ch = None if LAGS * C <= 16384 // 4 else list(range(a.cv_channels))
            for window in (1, 50):
                fr = wiener.fold_ranges(n - (LAGS - 1), FOLDS, LAGS - 1)
                tag = "%dx%d bin %s window %d" % (C, T, r, window)

                def mem_stats():
                    with archive.open(fn) as rd:
                        x = rd.read(0, n * (r or 1), bin=r)[:, :n]
                        return wiener.stats(x, y, LAGS, 0, CLIP, ranges=fr, window=window, max_bytes=mb)

                def file_stats():
                    with archive.open(fn) as rd:
                        return wiener.stats_from(rd.bins(0, T, bin=r, max_bytes=mb), y, LAGS, 0, CLIP, ranges=fr, window=window)

                def mem_cv():
                    with archive.open(fn) as rd:
                        x = rd.read(0, n * (r or 1), cv_ch, bin=r)[:, :n]
                        return cascade.cross_validate(x, y, LAGS, 0, CLIP, ALPHAS, DEGREES, FOLDS, window)

                def file_cv():
                    with archive.open(fn) as rd:
                        return cascade.cross_validate_from(rd.bins(0, T, cv_ch, bin=r, max_bytes=mb), y, LAGS, 0, CLIP, ALPHAS,
                                                           DEGREES, FOLDS, window)

                say = lambda what: note("%s: %s" % (tag, what))  # noqa: E731
                lines.append("%s: %d bins, %d lags, clip %d, %d folds, max_bytes %d" % (tag, n, LAGS, CLIP, FOLDS, mb))
                if "stats" in a.parts and LAGS * C <= 16384:
                    close(file_stats(), mem_stats())
                    say("statistics agree")
                    t = timed([("read() + stats", mem_stats), ("stats_from", file_stats)], a.reps, say)
                    for k in t:
                        lines.append(line(k, t[k]))
                    res["stats " + tag] = t
                if "cv" in a.parts:
                    got, want = file_cv(), mem_cv()
                    worst = max(float(((got[k][m] - want[k][m]).abs() / want[k][m].abs()).max()) for k in want for m in want[k])
                    say("cross-validation agrees to %.3g" % worst)
                    t = timed([("read() + cross_validate", mem_cv), ("cross_validate_from", file_cv)], a.reps, say)
                    for k in t:
                        lines.append(line(k + (" (%d ch)" % len(cv_ch) if cv_ch else ""), t[k]))
                    res["cv " + tag] = dict(t, agree=worst)
            del y
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="96x72000x1,1024x1000000x20")
    ap.add_argument("--parts", default="stats,cv")
    ap.add_argument("--max-bytes", type=int, default=1 << 26)
    ap.add_argument("--cv-channels", type=int, default=96)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_file_fit.txt"))
    a = ap.parse_args()
    a.parts = a.parts.split(",")
    info = muahuff.device_info(0)
    lines = ["bench_file_fit: %s (%s), %d alternated runs, host clock" % (info["name"], info["arch"], a.reps)]
    res = {}
    note = lambda what: print(what, file=sys.stderr, flush=True)  # noqa: E731
    for C, T, blocks in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]:
        shape(a, C, T, blocks, lines, res, note)
    lines.append(json.dumps(res, sort_keys=True))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
