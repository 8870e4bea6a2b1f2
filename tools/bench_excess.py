"""The excess list (mhi_excess_count / mhi_excess_emit, exact=True) on the workload of tools/bench_events_out.py --
1024 ch x 1e7 bins of 1 ms, 30 events per second and channel, S = 3 (threshold 2: about 4.5e-6 of the samples are above
it) -- as a channel-major matrix and as the time-major block of the same counts, both resident on the device.  Same
process, event-timed, the routes alternated after warm-up (20 runs each, medians):

  a  rows count   mhi_excess_count, ROWS form (count kernel + the scan)
  b  unbin count  mhi_unbin_count, CSR form, on the same matrix: the project's own one-read pass over such a matrix
                  (profiles/r14_events_out.txt).  The aim is median(a) <= 1.25 x median(b): both read the matrix once.
  c  rows emit    mhi_excess_emit, ROWS form, behind a count (capacity = the total)
  d  cols pair    mhi_excess_count + mhi_excess_emit, COLS form, on the time-major block
  e  torch        (x > S-1).nonzero() and the values gathered at its indices, at the largest tenth-power fraction of the
                  bins where it runs (reported with the rows pair at that size)

The lists are verified first: rows = cols entry for entry, and both against the torch route where that runs.
Then the cost on an archive append: blocks of 1024 ch x 1e6 steps appended to an archive with and without exact=True
(--append-blocks of them each, the file on --dir), seconds per block by wall clock, synchronised.  On a tree whose
archive.create has no `exact` only the plain figure is measured: that is the parent's number for the comparison.
Prints the table and writes it to --out (default profiles/r15_excess.txt).

    python tools/bench_excess.py [--reps 20] [--C 1024] [--T 10000000] [--append-blocks 4] [--dir DIR] [--out FILE]
"""
import argparse
import inspect
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import _ingest, archive  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bin_events import alternate  # noqa: E402
from bench_events_out import counts_matrix  # noqa: E402

S = 3
THR = S - 1
HAS = hasattr(_ingest, "excess_count")


def torch_list(x):
    nz = torch.nonzero(x > THR)
    return nz, x[nz[:, 0], nz[:, 1]] - THR


def torch_size(x, T):
    """-> (T', note): the bins at which the torch route runs on the first T' columns' worth of rows"""
    Tt, note = T, None
    while True:
        try:
            torch_list(x[:, :Tt].contiguous() if Tt < T else x)
            torch.cuda.synchronize()
            return Tt, note
        except (RuntimeError, torch.cuda.OutOfMemoryError) as exc:
            torch.cuda.empty_cache()
            if Tt < 1000:
                raise
            note = "the torch route does not run at %d bins (%s): it is measured at %d bins" % (Tt, str(exc).splitlines()[0][:120], Tt // 10)
            Tt //= 10


def kernels(a, lines, res):
    C, T = a.C, a.T
    x = counts_matrix(C, T)
    row_off = torch.arange(C, dtype=torch.int64, device="cuda") * T
    meta = torch.zeros(C + 3, dtype=torch.int64, device="cuda")           # offsets[0..C], total, over
    sc_unbin = torch.empty(_ingest.unbin_scratch_bytes(_ingest.UNBIN_CSR, C, T), dtype=torch.uint8, device="cuda")
    sc_rows = torch.empty(_ingest.excess_scratch_bytes(_ingest.EXCESS_ROWS, C, T), dtype=torch.uint8, device="cuda")
    sc_cols = torch.empty(_ingest.excess_scratch_bytes(_ingest.EXCESS_COLS, T, C), dtype=torch.uint8, device="cuda")

    def rows_count():
        _ingest.excess_count(_ingest.EXCESS_ROWS, x, row_off, None, None, C, T, THR, meta[:C + 1], meta[C + 1:C + 2], sc_rows)

    rows_count()
    n = int(meta[C + 1])
    pos = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    val = torch.empty(n + 1, dtype=torch.uint8, device="cuda")
    pos2, val2 = torch.empty_like(pos), torch.empty_like(val)
    off_rows = meta[:C + 1].clone()

    def rows_emit():
        _ingest.excess_emit(_ingest.EXCESS_ROWS, x, row_off, None, None, C, T, THR, pos, val, meta[C + 2:], sc_rows, capacity=n)

    def unbin_count():
        _ingest.unbin_count(_ingest.UNBIN_CSR, x, row_off, C, T, meta[:C + 1], meta[C + 1:C + 2], sc_unbin)

    X = x.t().contiguous()

    def cols_pair():
        _ingest.excess_count(_ingest.EXCESS_COLS, X, None, None, None, T, C, THR, meta[:C + 1], meta[C + 1:C + 2], sc_cols)
        _ingest.excess_emit(_ingest.EXCESS_COLS, X, None, None, None, T, C, THR, pos2, val2, meta[C + 2:], sc_cols, capacity=n)

    lines[0] += ", %d entries (%.3g of the samples)" % (n, n / (C * T))
    pos.fill_(-1)
    pos2.fill_(-1)
    rows_emit()
    cols_pair()
    torch.cuda.synchronize()
    assert int(meta[C + 1]) == n and int(meta[C + 2]) == 0 and int(pos[n]) == -1 and int(pos2[n]) == -1, "total / over / overrun"
    assert torch.equal(meta[:C + 1], off_rows) and torch.equal(pos, pos2) and torch.equal(val[:n], val2[:n]), "rows != cols"
    Tt, note = torch_size(x, T)
    if note:
        lines.append("NOTE: " + note)
    xs = x if Tt == T else x[:, :Tt].contiguous()
    nz, v = torch_list(xs)
    if Tt == T:
        assert torch.equal(nz[:, 1].int(), pos[:n]) and torch.equal(v, val[:n]), "the list differs from the torch route"
    lines.append("verified: rows = cols entry for entry%s" % (", = torch" if Tt == T else "; torch checked at its own size below"))
    del nz, v
    torch.cuda.empty_cache()

    r = alternate([("rows count", rows_count), ("unbin count", unbin_count), ("rows emit", rows_emit), ("cols pair", cols_pair)], a.reps)
    for k in ("rows count", "unbin count", "rows emit", "cols pair"):
        lines.append("%-12s min %9.4f  median %9.4f  max %9.4f ms   %.2f TB/s of matrix read at the median"
                     % (k, r[k]["min"], r[k]["median"], r[k]["max"], (2 if k == "cols pair" else 1) * C * T / r[k]["median"] / 1e9))
    ratio = r["rows count"]["median"] / r["unbin count"]["median"]
    lines.append("median rows count / median unbin count = %.3f (aim <= 1.25): %s" % (ratio, "met" if ratio <= 1.25 else "MISSED"))
    res.update(kernels=r, ratio=round(ratio, 4), aim_met=bool(ratio <= 1.25), entries=n)

    # the torch route at the size it takes, with the rows pair at that size next to it
    ro = torch.arange(C, dtype=torch.int64, device="cuda") * Tt
    sc = torch.empty(_ingest.excess_scratch_bytes(_ingest.EXCESS_ROWS, C, Tt), dtype=torch.uint8, device="cuda")

    def rows_pair_small():
        _ingest.excess_count(_ingest.EXCESS_ROWS, xs, ro, None, None, C, Tt, THR, meta[:C + 1], meta[C + 1:C + 2], sc)
        _ingest.excess_emit(_ingest.EXCESS_ROWS, xs, ro, None, None, C, Tt, THR, pos, val, meta[C + 2:], sc, capacity=n)

    rows_pair_small()
    nz, v = torch_list(xs)
    m = int(nz.shape[0])
    assert int(meta[C + 1]) == m and torch.equal(nz[:, 1].int(), pos[:m]) and torch.equal(v, val[:m]), "rows pair != torch"
    del nz, v
    rt = alternate([("rows pair", rows_pair_small), ("torch", lambda: torch_list(xs))], a.reps)
    lines.append("at %d ch x %d bins (%d entries, = torch entry for entry):" % (C, Tt, m))
    for k in ("rows pair", "torch"):
        lines.append("  %-10s min %9.4f  median %9.4f  max %9.4f ms" % (k, rt[k]["min"], rt[k]["median"], rt[k]["max"]))
    res["torch_size"] = dict(T=Tt, **rt)


def appends(a, lines, res):
    Tb = 1_000_000
    blocks = [counts_matrix(a.C, Tb, seed=20 + i).t().contiguous() for i in range(2)]
    can = "exact" in inspect.signature(archive.create).parameters
    out = {}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for mode in (("plain", "exact") if can else ("plain",)):
            kw = {"exact": True} if mode == "exact" else {}
            times = []
            with archive.create(os.path.join(d, mode + ".mha"), a.C, S=S, pipeline=False, **kw) as w:
                w.append(blocks[0])                                   # calibrates, plans and allocates
                for i in range(a.append_blocks):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    w.append(blocks[(i + 1) % 2])
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
            times.sort()
            out[mode] = dict(min=round(times[0], 4), median=round(times[len(times) // 2], 4), max=round(times[-1], 4),
                             file_bytes=os.path.getsize(os.path.join(d, mode + ".mha")))
            lines.append("append of a %d ch x %d step block, pipeline off, %-5s: min %.4f  median %.4f  max %.4f s per block (%d blocks; file %d bytes)"
                         % (a.C, Tb, mode, out[mode]["min"], out[mode]["median"], out[mode]["max"], a.append_blocks, out[mode]["file_bytes"]))
    if can:
        lines.append("exact - plain at the median = %.4f s per block, %.2f %% of the file"
                     % (out["exact"]["median"] - out["plain"]["median"],
                        100.0 * (out["exact"]["file_bytes"] - out["plain"]["file_bytes"]) / out["plain"]["file_bytes"]))
    res["append"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--T", type=int, default=10_000_000)
    ap.add_argument("--append-blocks", type=int, default=4)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_excess.txt"))
    a = ap.parse_args()
    info = muahuff.device_info(0)
    lines = ["bench_excess: %s (%s), %d ch x %d bins, threshold %d, %d alternated runs" % (info["name"], info["arch"], a.C, a.T, THR, a.reps)]
    res = {}
    if HAS:
        kernels(a, lines, res)
        torch.cuda.empty_cache()
    else:
        lines.append("this tree has no mhi_excess_*: only the plain append is measured")
    if a.append_blocks:
        appends(a, lines, res)
    lines.append(json.dumps(res, sort_keys=True))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
