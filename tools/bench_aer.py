"""The pair-list partition (mhi_aer_to_csr) against what it replaces, on the workload of tools/bench_bin_events.py --
1024 ch x 1e7 bins of 1 ms, 30 events per second and channel -- merged into ONE time-ordered list of (tick, channel)
pairs on the device.  Same process, event-timed, the routes alternated after warm-up (20 runs each):

  a  torch      torch.sort(channels, stable=True), a gather of the ticks by its indices, torch.bincount + cumsum for the
                offsets: what a user can write on the device without this library (16-bit channel keys, the cheapest)
  b  aer16      mhi_aer_to_csr, 16-bit channels, into resident buffers
  c  aer32      mhi_aer_to_csr, 32-bit channels
  d  host       once, for scale: EventSet.from_aer on host arrays (NumPy stable argsort + bincount + upload) on the first
                --host-fraction of the pairs

Outputs are verified equal once before timing (a = b = c, entry for entry).  The condition is median(b) <= median(a).
Also reported: the bytes the kernels move per pair by design and the share of the 8 TB/s HBM spec that makes at the
measured median, the tile rule chosen (tests/aer_layout_check.cpp), and a per-kernel split from torch.profiler.
Prints the table and writes it to --out (default profiles/r10_aer.txt).

    python tools/bench_aer.py [--reps 20] [--C 1024] [--T 10000000] [--host-fraction 0.1] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import _ingest, events  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bin_events import alternate  # noqa: E402

SPEC_BPS = 8e12
FIELDS = ("run", "waves", "tile", "nbits", "lds_bytes", "rows", "groups", "rows_alloc", "groups_alloc", "off_matrix",
          "off_partial", "off_drop", "bytes")


def layout(n, C):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "aer_layout_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "hardware-efficient-mua-compression_amd", "csrc"),
                               os.path.join(ROOT, "tests", "aer_layout_check.cpp"), "-o", exe])
        out = subprocess.run([exe, str(n), str(C)], check=True, capture_output=True, text=True).stdout
    return dict(zip(FIELDS, (int(v) for v in out.split())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--T", type=int, default=10_000_000)
    ap.add_argument("--host-fraction", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_aer.txt"))
    a = ap.parse_args()
    C, T, period, origin = a.C, a.T, 30, 1 << 20
    per_ch = int(round(0.03 * T))
    n = C * per_ch
    info = muahuff.device_info(0)
    g = torch.Generator(device="cuda").manual_seed(9)
    # uniform times = a Poisson process per channel; merged and put in time order (stable: ties keep the channel order)
    ticks = torch.randint(0, T * period, (n,), generator=g, device="cuda", dtype=torch.int64) + origin
    ticks, idx = torch.sort(ticks, stable=True)
    ch32 = (idx // per_ch).to(torch.int32)
    del idx
    ch16 = ch32.to(torch.int16)
    torch.cuda.empty_cache()
    lay = layout(n, C)
    lines = ["bench_aer: %s (%s), %d pairs over %d channels (%d ch x %d bins, %.3f events per bin), %d alternated runs"
             % (info["name"], info["arch"], n, C, C, T, n / (C * T), a.reps),
             "tile rule: sub-run W_e = %d pairs per wave, %d waves = tile T_e = %d pairs per workgroup, %d rows in %d groups, "
             "%d ballots per step, %d B of LDS per workgroup, scratch %.1f MB"
             % (lay["run"], lay["waves"], lay["tile"], lay["rows"], lay["groups"], lay["nbits"], lay["lds_bytes"], lay["bytes"] / 1e6)]

    out = torch.empty(n, dtype=torch.int64, device="cuda")
    meta = torch.empty(C + 2, dtype=torch.int64, device="cuda")
    scratch = torch.empty(_ingest.aer_scratch_bytes(n, C), dtype=torch.uint8, device="cuda")

    def route_torch():
        order = torch.sort(ch16, stable=True).indices
        off = torch.zeros(C + 1, dtype=torch.int64, device="cuda")
        off[1:] = torch.cumsum(torch.bincount(ch16, minlength=C), 0)
        return ticks[order], off

    def route_aer(ch):
        _ingest.aer_to_csr(ticks, ch, C, out, meta, meta[C + 1:], scratch)

    want, off = route_torch()
    for ch in (ch16, ch32):
        out.fill_(-1)
        meta.fill_(-1)
        route_aer(ch)
        torch.cuda.synchronize()
        assert torch.equal(meta[:C + 1], off) and int(meta[C + 1]) == 0, "offsets differ from the torch route"
        assert torch.equal(out, want), "ticks differ from the torch route"
    del want, off
    torch.cuda.empty_cache()

    res = alternate([("torch", route_torch), ("aer16", lambda: route_aer(ch16)), ("aer32", lambda: route_aer(ch32))], a.reps)
    torch.cuda.empty_cache()

    # bytes by design: the channel column twice, the tick column once, the ticks out, and the count matrix five times
    # (count writes it, the group sums read it, the bases read and write it, the scatter reads it)
    matrix = 5 * lay["rows"] * C * 4 + 3 * lay["groups"] * C * 4
    for k, cb in (("aer16", 2), ("aer32", 4)):
        r = res[k]
        r["bytes_per_pair"] = round(cb + (cb + 8) + 8 + matrix / n, 3)
        r["bytes"] = int(n * (2 * cb + 16) + matrix)
        r["TBps"] = round(r["bytes"] / r["median"] / 1e9, 3)
        r["of_spec"] = round(r["bytes"] / (r["median"] * 1e-3) / SPEC_BPS, 3)
    res["ratio_b_over_a"] = round(res["aer16"]["median"] / res["torch"]["median"], 4)
    res["condition_met"] = bool(res["aer16"]["median"] <= res["torch"]["median"])

    # per-kernel split of route b
    split = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(3):
                route_aer(ch16)
            torch.cuda.synchronize()
        for e in prof.key_averages():
            if "k_aer" in e.key:
                name = e.key.split("k_aer_")[1].split("(")[0].split("<")[0]
                dev_us = getattr(e, "device_time_total", None)
                if dev_us is None:
                    dev_us = e.cuda_time_total
                split[name] = round(dev_us / max(e.count, 1) / 1e3, 4)
    except Exception as exc:  # the split is a report, not a result
        split = {"unavailable": repr(exc)[:200]}
    res["kernel_ms"] = split

    # d: the host route, once
    m = max(1, int(n * a.host_fraction))
    h_t, h_c = ticks[:m].cpu().numpy(), ch32[:m].cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = events.EventSet.from_aer(h_t, h_c, C, check=False)
    torch.cuda.synchronize()
    res["host"] = {"pairs": m, "fraction": round(m / n, 4), "ms": round(1e3 * (time.perf_counter() - t0), 1)}
    del ev

    def row(name, r):
        return "  %-8s min %9.4f  median %9.4f  max %9.4f ms" % (name, r["min"], r["median"], r["max"])
    lines += ["a " + row("torch", res["torch"]).strip(), "b " + row("aer16", res["aer16"]).strip(),
              "c " + row("aer32", res["aer32"]).strip(),
              "median b / median a = %.4f: %s" % (res["ratio_b_over_a"], "condition met (b <= a)" if res["condition_met"]
                                                  else "CONDITION MISSED (b > a)")]
    for k in ("aer16", "aer32"):
        r = res[k]
        lines.append("%s by design: %.2f B per pair (%.2f GB), %.2f TB/s at the median = %.1f %% of the 8 TB/s spec"
                     % (k, r["bytes_per_pair"], r["bytes"] / 1e9, r["TBps"], 100 * r["of_spec"]))
    lines.append("per-kernel split of b (ms per call, torch.profiler): " + json.dumps(split, sort_keys=True))
    lines.append("d host from_aer, once, on %d pairs (%.2f of the list), with its upload: %.1f ms -> %.0f ms for the list if linear"
                 % (m, res["host"]["fraction"], res["host"]["ms"], res["host"]["ms"] / max(res["host"]["fraction"], 1e-9)))
    lines.append(json.dumps(res, sort_keys=True))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
