"""Fused decode + re-bin (mh_decode_rebin) against the two-step route on the resident 1024 x 1e7 set (synth, h = 6,
WIN_AFTER_CAL), same process and same payload buffer, event-timed, the contenders alternated after warm-up:
  range        mh_decode_range of the whole recording (the baseline's decode step)
  rebin        mh_rebin of those rows (uint8, saturating)
  fused        mh_decode_rebin straight to the bins (uint8, saturating)
per S and r: min / median / max of each in ms, fused / range and fused / (range + rebin) of the medians, the payload
read bandwidth of the fused call, and `ok` = median(fused) <= median(range), the condition DESIGN section 9 quotes.
The fused output is checked against the two-step one.  Prints one JSON line.

    python tools/bench_decode_rebin.py [--reps 20] [--S 3 8] [--r 5 50 100]
"""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import muahuff  # noqa: E402
from muahuff import MODE_APPROX, WIN_AFTER_CAL, _lib, codec, sclv, synth  # noqa: E402


def stats(ms):
    return {"min": round(float(np.min(ms)), 4), "median": round(float(np.median(ms)), 4), "max": round(float(np.max(ms)), 4)}


def run(S, C, T, rs, reps):
    cs = synth.generate(C, T, seed=S)
    plan = codec.Plan(cs.ch_off, cs.ch_len, S, 6, MODE_APPROX, WIN_AFTER_CAL, sclv.table(S))
    e = plan.encode(cs.data)
    del cs
    torch.cuda.empty_cache()
    seg_off = torch.from_numpy(plan.segments()["off"].astype(np.int64)).cuda()
    words = int(e.seg_words.sum().item())
    rows = plan.decode_range(e.payload, seg_off, e.peak, e.enc, None, 0, T)  # [C, T] view, pitch-strided
    pitch = rows.stride(0)
    vp = ct.c_void_p
    d_off = (torch.arange(C, dtype=torch.int64, device="cuda") * pitch)
    d_len = torch.full((C,), T, dtype=torch.int64, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    res = {"payload_bytes": 4 * words}
    for r in rs:
        nb = (T + r - 1) // r
        two = torch.empty((C, nb), dtype=torch.uint8, device="cuda")
        o_off = torch.arange(C, dtype=torch.int64, device="cuda") * nb
        fused = torch.empty((C, nb), dtype=torch.uint8, device="cuda")

        def f_range():
            plan.decode_range(e.payload, seg_off, e.peak, e.enc, None, 0, T, out=rows)

        def f_rebin():
            _lib.check(_lib.lib().mh_rebin(vp(rows.data_ptr()), vp(d_off.data_ptr()), vp(d_len.data_ptr()), C, T, r, 1,
                                           vp(two.data_ptr()), vp(o_off.data_ptr()), st))

        def f_fused():
            plan.decode_rebin(e.payload, seg_off, e.peak, e.enc, None, 0, T, r, True, out=fused)
        fns = (("range", f_range), ("rebin", f_rebin), ("fused", f_fused))
        for _ in range(3):
            for _, f in fns:
                f()
        torch.cuda.synchronize()
        assert plan.decode_ok() and torch.equal(two, fused), "fused != decode_range + mh_rebin"
        ev = {k: [] for k, _ in fns}
        for _ in range(reps):  # alternated: range, rebin, fused, range, ...
            for k, f in fns:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                ev[k].append((a, b))
        torch.cuda.synchronize()
        ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
        out = {k: stats(v) for k, v in ms.items()}
        med = {k: out[k]["median"] for k in out}
        out["fused_vs_range"] = round(med["fused"] / med["range"], 3)
        out["fused_vs_two_step"] = round(med["fused"] / (med["range"] + med["rebin"]), 3)
        out["fused_payload_GBps"] = round(4 * words / med["fused"] / 1e6, 1)
        out["ok"] = bool(med["fused"] <= med["range"])
        res["r%d" % r] = out
        del two, fused
    plan.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--S", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--r", type=int, nargs="+", default=[5, 50, 100])
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--T", type=int, default=10_000_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"device": muahuff.device_info(0)["name"], "C": args.C, "T": args.T, "reps": args.reps}
    for S in args.S:
        out["S%d" % S] = run(S, args.C, args.T, args.r, args.reps)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
