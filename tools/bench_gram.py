"""The spike-count Gram matrix (mhi_gram; gram.gram, archive.Reader.read_gram) against the routes a user has without it.

Resident part: uint8 matrices of 1024 ch x 1e6, 1024 ch x 1e7 and 96 ch x 72 000 bins at the synthetic 30 events per
second and channel (1 ms bins).  Same process, event-timed, the routes alternated after warm-up (20 runs each; median and
range):
  sym     mhi_gram, symmetric form (b == NULL), with the row sums
  cross   mhi_gram, cross form with y = x
  (a)     torch.matmul in float64 over chunks of columns, summed, then .long(): the exact route a user would write (every
          partial sum stays below 2^53)
  (b)     for information only: torch._int_mm on the XOR-ed int8 view in chunks of <= 131008 columns, widened and summed
          in int64, with the same fix-up -- if the build runs it at all
The integer results are compared first (exactly).  Condition: the median of `sym` at 1024 x 1e7 is below the median of
(a) on the same buffers, no margin.  Reported with no threshold: the ratio to (b), the share of the int8 matrix spec
(rows^2 * cols * 2 operations for both forms: the symmetric form does about half of them).

Archive part: 20 blocks of 1024 ch x 1e5 steps in one archive (the file on --dir): read_gram against read() of the range
and route (a), wall clock (synchronised) and bytes_read, on fresh Readers; the results are compared.

--once ROWSxCOLS runs a single symmetric mhi_gram on such a matrix and nothing else: the run to put under a counter
collection of its own (FETCH_SIZE against rows * cols gives the bytes fetched per byte of matrix).
Prints the table and writes it to --out (default profiles/r17_gram.txt).

    python tools/bench_gram.py [--reps 20] [--shapes 1024x1000000,1024x10000000,96x72000] [--blocks 20] [--dir DIR] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import archive, gram  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bin_events import alternate  # noqa: E402
from bench_events_out import counts_matrix  # noqa: E402

SPEC = 5e15          # int8 operations per second
CHUNK_F64 = 1 << 17  # columns of a float64 chunk: 1 GiB at 1024 rows
CHUNK_I8 = 131008    # columns of an int8 chunk: a multiple of 64 below the int32 bound of 131071


def route_f64(x):
    acc = torch.zeros((x.shape[0], x.shape[0]), dtype=torch.float64, device=x.device)
    for c in range(0, x.shape[1], CHUNK_F64):
        d = x[:, c:c + CHUNK_F64].double()
        acc += d @ d.t()
    return acc.long()


def route_int_mm(x):
    rows, cols = x.shape
    acc = torch.zeros((rows, rows), dtype=torch.int64, device=x.device)
    s = torch.zeros((rows,), dtype=torch.int64, device=x.device)
    for c in range(0, cols, CHUNK_I8):
        part = x[:, c:c + CHUNK_I8]
        k = part.shape[1]
        kp = -(-k // 64) * 64
        if kp != k:                                  # padding columns are x = 0
            part = torch.nn.functional.pad(part, (0, kp - k))
        z = (part ^ 0x80).contiguous().view(torch.int8)
        zz = torch._int_mm(z, z.t().contiguous()).long()
        sp = part.sum(1, dtype=torch.int64)
        acc += zz + 128 * (sp[:, None] + sp[None, :]) - 16384 * kp
        s += sp
    return acc


def resident(a, lines, res):
    ok, cells = None, {}
    for rows, cols in a.shapes:
        x = counts_matrix(rows, cols)
        sym = lambda: gram.gram(x)                                             # noqa: E731
        cross = lambda: gram.gram(x, x)                                        # noqa: E731
        f64 = lambda: route_f64(x)                                             # noqa: E731
        want = f64()
        g = sym()
        assert torch.equal(g.gram, want) and torch.equal(g.sum_a, x.sum(1, dtype=torch.int64)), (rows, cols, "sym")
        g = cross()
        assert torch.equal(g.gram, want) and torch.equal(g.sum_b, x.sum(1, dtype=torch.int64)), (rows, cols, "cross")
        del g
        fns = [("sym", sym), ("cross", cross), ("f64", f64)]
        try:
            assert torch.equal(route_int_mm(x), want)
            fns.append(("int_mm", lambda: route_int_mm(x)))
            note = ""
        except Exception as e:  # noqa: BLE001  (route (b) is for information: say why it did not run)
            note = "route (b) did not run: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:120])
        del want
        torch.cuda.empty_cache()
        t = alternate(fns, a.reps)
        ops = 2.0 * rows * rows * cols
        cell = dict(t, ops=ops)
        for k in ("sym", "cross"):
            cell[k + "_spec_share"] = round(ops / (t[k]["median"] * 1e-3) / SPEC, 4)
        cell["f64_over_sym"] = round(t["f64"]["median"] / t["sym"]["median"], 2)
        met = t["sym"]["median"] < t["f64"]["median"]
        lines.append("%d x %d" % (rows, cols))
        for k, label in (("sym", "mhi_gram symmetric"), ("cross", "mhi_gram cross y=x"), ("f64", "(a) float64 matmul"),
                         ("int_mm", "(b) torch._int_mm")):
            if k in t:
                lines.append("    %-20s min %10.4f median %10.4f max %10.4f ms" % (label, t[k]["min"], t[k]["median"], t[k]["max"]))
        lines.append("    (a) / symmetric x%.2f   share of the %.0f POPS int8 spec: symmetric %.4f, cross %.4f   %s"
                     % (cell["f64_over_sym"], SPEC / 1e15, cell["sym_spec_share"], cell["cross_spec_share"],
                        "below (a)" if met else "NOT below (a)"))
        if "int_mm" in t:
            cell["int_mm_over_sym"] = round(t["int_mm"]["median"] / t["sym"]["median"], 2)
            lines.append("    (b) / symmetric x%.2f" % cell["int_mm_over_sym"])
        elif note:
            lines.append("    " + note)
        cells["%dx%d" % (rows, cols)] = cell
        if (rows, cols) == (1024, 10_000_000):
            ok = bool(met)
        del x
        torch.cuda.empty_cache()
    if ok is not None:
        lines.append("condition (symmetric median below (a) at 1024 x 1e7, results bit-identical): %s" % ("met" if ok else "MISSED"))
    res.update(cells=cells, condition_met=ok)


def stored(a, lines, res):
    C, Tb = 1024, 100_000
    T = a.blocks * Tb
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        fn = os.path.join(d, "rec.mua")
        with archive.create(fn, C, S=3) as w:
            for i in range(a.blocks):
                w.append(counts_matrix(C, Tb, seed=40 + i).t().contiguous())
        out = {}
        with archive.open(fn) as rd:            # warm: plans, the module, the allocator
            rd.read_gram(0, 8192)
            route_f64(rd.read(0, 8192))
        torch.cuda.synchronize()
        with archive.open(fn) as rd:
            t0 = time.perf_counter()
            got = rd.read_gram(0, T, max_bytes=a.max_bytes)
            torch.cuda.synchronize()
            out["read_gram"] = dict(seconds=round(time.perf_counter() - t0, 4), bytes_read=rd.bytes_read)
        with archive.open(fn) as rd:
            t0 = time.perf_counter()
            want = route_f64(rd.read(0, T))
            torch.cuda.synchronize()
            out["read_then_f64"] = dict(seconds=round(time.perf_counter() - t0, 4), bytes_read=rd.bytes_read)
        assert torch.equal(got.gram, want) and got.n == T
    for k in ("read_gram", "read_then_f64"):
        lines.append("archive of %d blocks of %d ch x %d steps, [0, %d): %-14s %8.4f s  %d bytes read"
                     % (a.blocks, C, Tb, T, k, out[k]["seconds"], out[k]["bytes_read"]))
    res["archive"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="1024x1000000,1024x10000000,96x72000")
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--max-bytes", type=int, default=1 << 29)
    ap.add_argument("--once", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_gram.txt"))
    a = ap.parse_args()
    if a.once:
        rows, cols = (int(v) for v in a.once.split("x"))
        x = counts_matrix(rows, cols)
        torch.cuda.synchronize()
        g = gram.gram(x)
        torch.cuda.synchronize()
        print("once: %d x %d = %d bytes of matrix, trace %d" % (rows, cols, rows * cols, int(torch.diagonal(g.gram).sum())))
        return
    a.shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]
    info = muahuff.device_info(0)
    lines = ["bench_gram: %s (%s), %d alternated runs" % (info["name"], info["arch"], a.reps)]
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
