"""Counts back to events (mhi_unbin_count + mhi_unbin_emit) against what they replace, on the workload of
tools/bench_bin_events.py -- 1024 ch x 1e7 bins of 1 ms, 30 events per second and channel, about 3.07e8 events -- as a
channel-major matrix of counts and as the time-major block of the same counts, both resident on the device.  Same
process, event-timed, the routes alternated after warm-up (20 runs each):

  a  csr        mhi_unbin_count + mhi_unbin_emit, CSR form, into resident buffers (no read of the total in between: the
                buffers are sized once, as a caller that replays a graph would)
  b  aer        the same in the AER form on the time-major block, 32-bit channels
  c  torch      torch.nonzero, the counts gathered at its indices, torch.repeat_interleave of the tick arithmetic, and a
                row sum + cumsum for the offsets: what a user can write on the device without this library (CSR output)

Outputs are verified equal once before timing (a = c entry for entry; b against the same construction on the block).
The condition is median(a) <= median(c) and median(b) <= median(c) with ranges that do not overlap.  Also reported: the
bytes moved by design -- the matrix twice plus the events written -- and their share of the 8 TB/s HBM spec at the
measured median, and a per-kernel split from torch.profiler.  If the torch route cannot run at the full size, both are
run at the largest tenth-power fraction of the bins where it does, and the file says so; the kernel pair is then also
timed alone at the full size (total, offsets and over checked against row sums).
Prints the table and writes it to --out (default profiles/r14_events_out.txt).

    python tools/bench_events_out.py [--reps 20] [--C 1024] [--T 10000000] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import _ingest  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bin_events import alternate  # noqa: E402

SPEC_BPS = 8e12
ORIGIN, PERIOD, PHASE = 1 << 20, 30, 0


def counts_matrix(C, T, seed=9):
    """[C, T] uint8, Poisson with 0.03 events per bin, generated in slabs of channels"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((C, T), dtype=torch.uint8, device="cuda")
    step = max(1, (1 << 28) // T)
    for c in range(0, C, step):
        n = min(step, C - c)
        x[c:c + n] = torch.poisson(torch.full((n, T), 0.03, device="cuda"), generator=g).clamp_(max=255).to(torch.uint8)
    return x


def torch_csr(x):
    nz = torch.nonzero(x)
    k = x[nz[:, 0], nz[:, 1]].long()
    ticks = torch.repeat_interleave(ORIGIN + nz[:, 1] * PERIOD + PHASE, k)
    off = torch.zeros(x.shape[0] + 1, dtype=torch.int64, device=x.device)
    off[1:] = torch.cumsum(x.sum(dim=1, dtype=torch.int64), 0)
    return ticks, off


def torch_aer(X):
    nz = torch.nonzero(X)
    k = X[nz[:, 0], nz[:, 1]].long()
    return (torch.repeat_interleave(ORIGIN + nz[:, 0] * PERIOD + PHASE, k),
            torch.repeat_interleave(nz[:, 1].to(torch.int32), k))


def largest_size_torch_takes(C, T):
    """-> (T', note): the bins at which the torch route runs, a tenth-power fraction of T"""
    Tt, note = T, None
    while True:
        try:
            x = counts_matrix(C, Tt)
            torch_csr(x)
            torch.cuda.synchronize()
            return x, Tt, note
        except (RuntimeError, torch.cuda.OutOfMemoryError) as exc:
            x = None
            torch.cuda.empty_cache()
            if Tt < 1000:
                raise
            note = "the torch route does not run at %d ch x %d bins (%s): every route is measured at %d bins" % (
                C, Tt, str(exc).splitlines()[0][:160], Tt // 10)
            Tt //= 10


def full_size_pair_alone(C, T, reps, lines):
    """The kernel pair at the size the torch route could not take: checked against row sums (total, offsets, over), then
    the two forms alternated."""
    x = counts_matrix(C, T)
    X = x.t().contiguous()
    row_off = torch.arange(C, dtype=torch.int64, device="cuda") * T
    want_off = torch.zeros(C + 1, dtype=torch.int64, device="cuda")
    want_off[1:] = torch.cumsum(x.sum(dim=1, dtype=torch.int64), 0)
    n = int(want_off[C])
    ticks = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    chans = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    meta = torch.zeros(C + 3, dtype=torch.int64, device="cuda")
    sc_csr = torch.empty(_ingest.unbin_scratch_bytes(_ingest.UNBIN_CSR, C, T), dtype=torch.uint8, device="cuda")
    sc_aer = torch.empty(_ingest.unbin_scratch_bytes(_ingest.UNBIN_AER, T, C), dtype=torch.uint8, device="cuda")

    def route_csr():
        _ingest.unbin_count(_ingest.UNBIN_CSR, x, row_off, C, T, meta[:C + 1], meta[C + 1:C + 2], sc_csr)
        _ingest.unbin_emit(_ingest.UNBIN_CSR, x, row_off, C, T, ORIGIN, PERIOD, PHASE, ticks, None, meta[C + 2:], sc_csr,
                           capacity=n)

    def route_aer():
        _ingest.unbin_count(_ingest.UNBIN_AER, X, None, T, C, None, meta[C + 1:C + 2], sc_aer)
        _ingest.unbin_emit(_ingest.UNBIN_AER, X, None, T, C, ORIGIN, PERIOD, PHASE, ticks, chans, meta[C + 2:], sc_aer,
                           capacity=n)

    for f in (route_csr, route_aer):
        ticks.fill_(-1)
        meta[C + 1:].zero_()
        f()
        torch.cuda.synchronize()
        assert int(meta[C + 1]) == n and int(meta[C + 2]) == 0 and int(ticks[n]) == -1 and int(ticks[:n].min()) >= ORIGIN
    assert torch.equal(meta[:C + 1], want_off), "offsets differ from the row sums"
    res = alternate([("csr", route_csr), ("aer", route_aer)], reps)
    lines.append("the kernel pair alone at %d ch x %d bins, %d events (total, offsets and over checked against row sums):" % (C, T, n))
    for k, per_event in (("csr", 8), ("aer", 12)):
        r = res[k]
        r["bytes"] = 2 * C * T + per_event * n
        r["of_spec"] = round(r["bytes"] / (r["median"] * 1e-3) / SPEC_BPS, 3)
        lines.append("  %-4s min %9.4f  median %9.4f  max %9.4f ms; %.3f GB by design, %.2f TB/s = %.1f %% of the 8 TB/s spec"
                     % (k, r["min"], r["median"], r["max"], r["bytes"] / 1e9, r["bytes"] / r["median"] / 1e9, 100 * r["of_spec"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--T", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_events_out.txt"))
    a = ap.parse_args()
    info = muahuff.device_info(0)
    x, T, note = largest_size_torch_takes(a.C, a.T)
    C = a.C
    X = x.t().contiguous()
    row_off = torch.arange(C, dtype=torch.int64, device="cuda") * T
    want_t, want_off = torch_csr(x)
    n = int(want_t.numel())
    lines = ["bench_events_out: %s (%s), %d ch x %d bins, %d events (%.4f per bin), %d alternated runs"
             % (info["name"], info["arch"], C, T, n, n / (C * T), a.reps)]
    if note:
        lines.append("NOTE: " + note)

    ticks = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    chans = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    meta = torch.zeros(C + 3, dtype=torch.int64, device="cuda")          # ev_off[0..C], total, over
    sc_csr = torch.empty(_ingest.unbin_scratch_bytes(_ingest.UNBIN_CSR, C, T), dtype=torch.uint8, device="cuda")
    sc_aer = torch.empty(_ingest.unbin_scratch_bytes(_ingest.UNBIN_AER, T, C), dtype=torch.uint8, device="cuda")

    def route_csr():
        _ingest.unbin_count(_ingest.UNBIN_CSR, x, row_off, C, T, meta[:C + 1], meta[C + 1:C + 2], sc_csr)
        _ingest.unbin_emit(_ingest.UNBIN_CSR, x, row_off, C, T, ORIGIN, PERIOD, PHASE, ticks, None, meta[C + 2:], sc_csr,
                           capacity=n)

    def route_aer():
        _ingest.unbin_count(_ingest.UNBIN_AER, X, None, T, C, None, meta[C + 1:C + 2], sc_aer)
        _ingest.unbin_emit(_ingest.UNBIN_AER, X, None, T, C, ORIGIN, PERIOD, PHASE, ticks, chans, meta[C + 2:], sc_aer,
                           capacity=n)

    # the outputs first
    ticks.fill_(-1)
    route_csr()
    torch.cuda.synchronize()
    assert int(meta[C + 1]) == n and int(meta[C + 2]) == 0 and int(ticks[n]) == -1, "total / over / overrun"
    assert torch.equal(meta[:C + 1], want_off), "offsets differ from the torch route"
    assert torch.equal(ticks[:n], want_t), "ticks differ from the torch route"
    del want_t, want_off
    ticks.fill_(-1)
    chans.fill_(-1)
    route_aer()
    torch.cuda.synchronize()
    wt, wc = torch_aer(X)
    assert int(meta[C + 1]) == n and int(meta[C + 2]) == 0 and int(ticks[n]) == -1 and int(chans[n]) == -1
    assert torch.equal(ticks[:n], wt) and torch.equal(chans[:n], wc), "the pair list differs from the torch route"
    del wt, wc
    torch.cuda.empty_cache()
    lines.append("verified: csr = torch (ticks, offsets), aer = torch on the time-major block (ticks, channels)")

    res = alternate([("csr", route_csr), ("aer", route_aer), ("torch", lambda: torch_csr(x))], a.reps)
    torch.cuda.empty_cache()
    for k, per_event in (("csr", 8), ("aer", 12)):
        r = res[k]
        r["bytes"] = 2 * C * T + per_event * n
        r["TBps"] = round(r["bytes"] / r["median"] / 1e9, 3)
        r["of_spec"] = round(r["bytes"] / (r["median"] * 1e-3) / SPEC_BPS, 3)
    ok = {k: bool(res[k]["median"] <= res["torch"]["median"] and res[k]["max"] < res["torch"]["min"]) for k in ("csr", "aer")}
    res["condition_met"] = ok

    split = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        for name, f in (("csr", route_csr), ("aer", route_aer)):
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                for _ in range(3):
                    f()
                torch.cuda.synchronize()
            split[name] = {}
            for e in prof.key_averages():
                if "k_unbin" in e.key:
                    kn = e.key.split("k_unbin_")[1].split("(")[0].split("<")[0]
                    dev_us = getattr(e, "device_time_total", None)
                    if dev_us is None:
                        dev_us = e.cuda_time_total
                    split[name][kn] = round(dev_us / max(e.count, 1) / 1e3, 4)
    except Exception as exc:  # the split is a report, not a result
        split = {"unavailable": repr(exc)[:200]}
    res["kernel_ms"] = split

    def row(tag, name):
        r = res[name]
        return "%s %-6s min %10.4f  median %10.4f  max %10.4f ms" % (tag, name, r["min"], r["median"], r["max"])
    lines += [row("a", "csr"), row("b", "aer"), row("c", "torch")]
    for k in ("csr", "aer"):
        r = res[k]
        lines.append("median %s / median torch = %.4f, ranges %s: %s"
                     % (k, r["median"] / res["torch"]["median"], "disjoint" if r["max"] < res["torch"]["min"] else "OVERLAP",
                        "condition met" if ok[k] else "CONDITION MISSED"))
        lines.append("%s by design: the matrix twice + the events = %.3f GB, %.2f TB/s at the median = %.1f %% of the 8 TB/s spec"
                     % (k, r["bytes"] / 1e9, r["TBps"], 100 * r["of_spec"]))
    lines.append("per-kernel split (ms per call, torch.profiler): " + json.dumps(split, sort_keys=True))
    if T < a.T:
        del x, X, ticks, chans, sc_csr, sc_aer, row_off
        torch.cuda.empty_cache()
        res["full_size"] = full_size_pair_alone(C, a.T, a.reps, lines)
    lines.append(json.dumps(res, sort_keys=True))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
