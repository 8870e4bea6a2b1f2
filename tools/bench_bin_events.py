"""The binner (mhi_bin_events) against what it replaces, on 1024 ch x 1e7 bins of 1 ms with 30 events per second and
channel (0.03 per bin), same process, event-timed, the contenders alternated after warm-up (20 runs each):

  A  counts from events   torch.bincount on channel * T + bin keys (128 channels at a time), clamp, cast into a ChannelSet -- what a user
                          writes on the device today -- against ChannelSet.from_events
  B  stream block         StreamEncoder.encode_block_device on a resident time-major block (de-interleave + preset
                          encode + compact) against encode_events_device on the resident events, S = 3 and S = 5
  kernel                  mhi_bin_events alone into a resident buffer, bits 8 / 4 / 2 (4 / 2 chunk-blocked), with the
                          bytes it moves (events read + bins or pieces written) as a fraction of the 8 TB/s HBM spec

Outputs are verified once before timing: from_events equals the bincount route, and the event stream equals the block
stream of the same counts byte for byte.  `ok` = the new path's min..max lies wholly below the old one's.
Prints the table and writes it to --out (default profiles/r09_bin_events.txt).

    python tools/bench_bin_events.py [--reps 20] [--C 1024] [--T 10000000] [--out FILE]
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
from muahuff import _ingest, events, sclv  # noqa: E402
from muahuff.container import ChannelSet  # noqa: E402
from muahuff.stream import StreamEncoder  # noqa: E402

SPEC_BPS = 8e12


def stats(ms):
    return {"min": round(float(np.min(ms)), 4), "median": round(float(np.median(ms)), 4), "max": round(float(np.max(ms)), 4)}


def alternate(fns, reps):
    """fns: [(name, f)] -> {name: stats}; three warm-up rounds, then reps rounds name1, name2, ..., name1, ..."""
    for _ in range(3):
        for _, f in fns:
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k, _ in fns}
    for _ in range(reps):
        for k, f in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
        torch.cuda.synchronize()
    return {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--T", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_bin_events.txt"))
    a = ap.parse_args()
    C, T, period, origin = a.C, a.T, 30, 1 << 20            # a 30 kHz clock, 1 ms bins
    per_ch = int(round(0.03 * T))
    info = muahuff.device_info(0)
    g = torch.Generator(device="cuda").manual_seed(9)
    ticks = torch.empty((C, per_ch), dtype=torch.int64, device="cuda")
    for c0 in range(0, C, 64):                               # uniform times = a Poisson process; sorted per channel
        t = torch.randint(0, T * period, (min(64, C - c0), per_ch), generator=g, device="cuda", dtype=torch.int64)
        ticks[c0:c0 + 64] = torch.sort(t, dim=1).values + origin
    ev = events.EventSet(ticks.view(-1), np.arange(C + 1, dtype=np.uint64) * np.uint64(per_ch))
    n_ev = C * per_ch
    lines = ["bench_bin_events: %s (%s), %d ch x %d bins, %d events (%.3f per bin), period %d ticks, %d alternated runs"
             % (info["name"], info["arch"], C, T, n_ev, n_ev / (C * T), period, a.reps)]
    res = {}

    # ---- A
    G = 128                                                  # channels per bincount: 1.28e9 int64 bins at a time

    def route_bincount():
        cs = ChannelSet.empty([T] * C)
        m = cs.matrix()
        for c0 in range(0, C, G):
            tk = ticks[c0:c0 + G]
            n_c = tk.shape[0]
            b = (tk - origin) // period
            key = b + torch.arange(n_c, device="cuda", dtype=torch.int64)[:, None] * T
            keep = (tk >= origin) & (b < T)
            n = torch.bincount(key[keep], minlength=n_c * T)
            m[c0:c0 + n_c].copy_(n.clamp_(max=255).view(n_c, T))
        return cs

    def route_events():
        return ChannelSet.from_events(ev, origin, period, T)
    want, got = route_bincount(), route_events()
    torch.cuda.synchronize()
    assert torch.equal(want.data, got.data), "from_events != bincount route"
    del want
    torch.cuda.empty_cache()
    res["A"] = alternate([("bincount", lambda: route_bincount()), ("from_events", lambda: route_events())], a.reps)
    torch.cuda.empty_cache()

    # ---- kernel alone
    d_off = torch.from_numpy(got.ch_off.astype(np.int64)).cuda()
    kern = [("bits8", lambda: _ingest.bin_events(ev, origin, period, T, 8, got.data, d_off))]
    block = got.to_time_major()                              # the resident time-major block of the same counts
    encs = {}
    for S in (3, 5):
        se = StreamEncoder(C, S, 6, sclv.table(S))
        se.calibrate(block[:64])
        slot = se._slot(T)
        encs[S] = (se, slot)
        bits = slot["plan"].input_bits
        kern.append(("bits%d" % bits, lambda slot=slot, bits=bits: _ingest.bin_events(
            ev, origin, period, T, bits, slot["cs"].data, slot["d_off"], slot["plan"].chunk_stride)))
    res["kernel"] = alternate(kern, a.reps)
    for k, bits in (("bits8", 8), ("bits4", 4), ("bits2", 2)):
        nbytes = n_ev * 8 + (C * T * bits) // 8
        r = res["kernel"][k]
        r["bytes"] = nbytes
        r["TBps"] = round(nbytes / r["median"] / 1e9, 3)
        r["of_spec"] = round(nbytes / (r["median"] * 1e-3) / SPEC_BPS, 3)

    # ---- B
    for S in (3, 5):
        se, slot = encs[S]
        da, ta, _ = se.encode_block_device(block)
        ref = da.payload[:int(ta.item())].clone()
        db, tb, _ = se.encode_events_device(ev, origin, period, T)
        assert int(tb.item()) == ref.numel() and torch.equal(db.payload[:ref.numel()], ref), "event stream != block stream"
        del ref
        res["B_S%d" % S] = alternate([("block", lambda se=se: se.encode_block_device(block)),
                                      ("events", lambda se=se: se.encode_events_device(ev, origin, period, T))], a.reps)
        se.close()

    def row(name, r):
        return "  %-12s min %9.4f  median %9.4f  max %9.4f ms" % (name, r["min"], r["median"], r["max"])
    for key, old, new in (("A", "bincount", "from_events"), ("B_S3", "block", "events"), ("B_S5", "block", "events")):
        r = res[key]
        r["ok"] = bool(r[new]["max"] < r[old]["min"])
        r["ratio"] = round(r[new]["median"] / r[old]["median"], 4)
        lines += ["%s:" % key, row(old, r[old]), row(new, r[new]),
                  "  %s / %s = %.4f of the medians; ranges %s" % (new, old, r["ratio"], "do not overlap: ok" if r["ok"] else
                                                                  "OVERLAP or the new path is slower: condition missed")]
    lines.append("kernel alone (mhi_bin_events):")
    for k in ("bits8", "bits4", "bits2"):
        r = res["kernel"][k]
        lines.append(row(k, r) + "  %.2f GB moved, %.2f TB/s = %.1f %% of the 8 TB/s spec"
                     % (r["bytes"] / 1e9, r["TBps"], 100 * r["of_spec"]))
    lines.append(json.dumps(res, sort_keys=True))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
