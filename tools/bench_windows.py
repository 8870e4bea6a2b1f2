"""Trial-aligned windows (mhi_windows; windows.gather / windows.psth, archive.Reader.read_windows) against the torch route.

Resident part: a 1024 ch x 1e6 bin uint8 matrix at the synthetic 30 events per second and channel (1 ms bins), 1000
random triggers, W = 2000.  Cells: r in {1, 10, 50} x {gather, psth, psth(moments=2)}.  Same process, event-timed, the
two routes of a cell alternated after warm-up (20 runs each; median and range).  The torch route on the same matrix:
  gather  x[:, off[:, None] + arange(W)] -> [rows, n, W], permuted to the stacked order [n, rows, W] (contiguous), and
          for r > 1 .view(n, rows, nb, r).sum(-1)
  psth    a further .sum(0); with moments=2 the squares of the stack summed as well
The results are compared first (exactly).  Condition: the fused median is at or below the torch median in EVERY cell,
with no margin -- the torch route moves an 8-byte index per gathered byte and, for the PSTH, writes and re-reads the
stacked intermediate.  Also reported, with no threshold: the fraction of the 8 TB/s spec reached on rows*n*W bytes read
plus the bytes written.

Archive part: 20 blocks of 1024 ch x 1e5 steps in one archive (the file on --dir), 1000 triggers: read_windows against
the loop of read(), wall clock (synchronised) and bytes_read, on fresh Readers; the results are compared.
Prints the table and writes it to --out (default profiles/r16_windows.txt).

    python tools/bench_windows.py [--reps 20] [--C 1024] [--T 1000000] [--n 1000] [--W 2000] [--blocks 20] [--dir DIR] [--out FILE]
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
from muahuff import archive, windows  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bin_events import alternate  # noqa: E402
from bench_events_out import counts_matrix  # noqa: E402

SPEC = 8e12   # bytes per second


def torch_stack(x, off, W, r):
    idx = off[:, None] + torch.arange(W, device=x.device)
    g = x[:, idx].permute(1, 0, 2).contiguous()                        # [n, rows, W]
    return g if r == 1 else g.view(g.shape[0], g.shape[1], W // r, r).sum(-1)


def torch_psth(x, off, W, r, moments):
    s = torch_stack(x, off, W, r)
    if moments == 1:
        return s.sum(0)
    s = s.long()
    return s.sum(0), (s * s).sum(0)


def resident(a, lines, res):
    C, T, n, W = a.C, a.T, a.n, a.W
    x = counts_matrix(C, T)
    off_h = np.random.RandomState(3).randint(0, T - W + 1, n).astype(np.int64)
    off = torch.from_numpy(off_h).cuda()
    ok, cells = True, {}
    for r in (1, 10, 50):
        assert W % r == 0
        nb = W // r
        for form in ("gather", "psth", "psth2"):
            if form == "gather":
                fused = lambda: windows.gather(x, off, W, r)                       # noqa: E731
                ref = lambda: torch_stack(x, off, W, r)                            # noqa: E731
                written = n * C * nb
            else:
                m = 1 if form == "psth" else 2
                fused = lambda: windows.psth(x, off, W, r, moments=m)              # noqa: E731
                ref = lambda: torch_psth(x, off, W, r, m)                          # noqa: E731
                written = C * nb * (4 if m == 1 else 12)
            got, want = fused(), ref()
            pairs = zip(got, want) if isinstance(got, tuple) else [(got, want)]
            assert all(torch.equal(g.long(), w.long()) for g, w in pairs), (r, form)
            del got, want, pairs
            torch.cuda.empty_cache()
            t = alternate([("fused", fused), ("torch", ref)], a.reps)
            f, q = t["fused"], t["torch"]
            frac = (C * n * W + written) / (f["median"] * 1e-3) / SPEC
            met = f["median"] <= q["median"]
            ok &= met
            cells["%s r=%d" % (form, r)] = dict(fused=f, torch=q, spec_fraction=round(frac, 4), met=bool(met))
            lines.append("r=%-3d %-7s fused min %8.4f median %8.4f max %8.4f ms | torch min %9.4f median %9.4f max %9.4f ms | "
                         "x%.1f  %.3f of 8 TB/s  %s" % (r, form, f["min"], f["median"], f["max"], q["min"], q["median"], q["max"],
                                                        q["median"] / f["median"], frac, "met" if met else "MISSED"))
            torch.cuda.empty_cache()
    lines.append("condition (fused median <= torch median in every cell): %s" % ("met" if ok else "MISSED"))
    res.update(cells=cells, condition_met=bool(ok))


def stored(a, lines, res):
    C, Tb, n, W = a.C, 100_000, a.n, a.W
    T = a.blocks * Tb
    trig = np.random.RandomState(4).randint(W // 2, T - W // 2, n).astype(np.int64)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        fn = os.path.join(d, "rec.mua")
        with archive.create(fn, C, S=3) as w:
            for i in range(a.blocks):
                w.append(counts_matrix(C, Tb, seed=40 + i).t().contiguous())
        out = {}
        with archive.open(fn) as rd:            # warm: plans, the module, the allocator
            rd.read_windows(trig[:8], W // 2, W // 2)
            rd.read(0, 4096)
        torch.cuda.synchronize()
        with archive.open(fn) as rd:
            t0 = time.perf_counter()
            got = rd.read_windows(trig, W // 2, W // 2)
            torch.cuda.synchronize()
            out["read_windows"] = dict(seconds=round(time.perf_counter() - t0, 4), bytes_read=rd.bytes_read)
        with archive.open(fn) as rd:
            t0 = time.perf_counter()
            rows = [rd.read(int(t) - W // 2, int(t) + W // 2) for t in trig]
            want = torch.stack(rows)
            torch.cuda.synchronize()
            out["loop"] = dict(seconds=round(time.perf_counter() - t0, 4), bytes_read=rd.bytes_read)
        assert torch.equal(got, want)
    for k in ("read_windows", "loop"):
        lines.append("archive of %d blocks of %d ch x %d steps, %d triggers, W = %d: %-12s %8.4f s  %d bytes read"
                     % (a.blocks, C, Tb, n, W, k, out[k]["seconds"], out[k]["bytes_read"]))
    lines.append("loop / read_windows: x%.1f in time, x%.1f in bytes read" %
                 (out["loop"]["seconds"] / out["read_windows"]["seconds"], out["loop"]["bytes_read"] / out["read_windows"]["bytes_read"]))
    res["archive"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--T", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--W", type=int, default=2000)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_windows.txt"))
    a = ap.parse_args()
    info = muahuff.device_info(0)
    lines = ["bench_windows: %s (%s), %d ch x %d bins, %d triggers, W = %d, %d alternated runs"
             % (info["name"], info["arch"], a.C, a.T, a.n, a.W, a.reps)]
    res = {}
    resident(a, lines, res)
    torch.cuda.empty_cache()
    if a.blocks:
        stored(a, lines, res)
    lines.append(json.dumps(res, sort_keys=True))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
