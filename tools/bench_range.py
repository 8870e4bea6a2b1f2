"""Random access in time on the resident 1024 x 1e7 set (synth, h = 6, WIN_AFTER_CAL) at S = 3 and S = 10: event-timed
medians after warm-up of
  decode       mh_decode of the whole set (the codec's decoder, for reference)
  range_full   mh_decode_range over [0, max_len) of all channels
  range_<n>_<c>  n = 1 000, 16 384, 1 000 000 bins at a random unaligned offset over all 1024 channels and 96 of them
(the *_ms figures repeat one query, whose work list the plan keeps; *_first_call_wall_ms is the host wall time of the
first call of a query, work list built and uploaded)
and (S = 3) container_io.decompress_range from a saved file for the 16 384-bin case over 96 channels: wall time and
bytes_read against the file size.  Every output is checked against the device-side slice of the full decode.
Prints one JSON line.

    python tools/bench_range.py [--reps 10] [--S 3 10]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import muahuff  # noqa: E402
from muahuff import MODE_APPROX, WIN_AFTER_CAL, codec, container_io, sclv, synth  # noqa: E402


def median_ms(fn, reps):
    fn()
    fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return round(float(np.median([a.elapsed_time(b) for a, b in ev])), 4)


def run(S, C, T, reps, rng, do_file):
    res = {}
    cs = synth.generate(C, T, seed=S)
    tab = sclv.table(S)
    plan = codec.Plan(cs.ch_off, cs.ch_len, S, 6, MODE_APPROX, WIN_AFTER_CAL, tab)
    e = plan.encode(cs.data)
    ref = torch.zeros_like(cs.data)
    res["decode_ms"] = median_ms(lambda: plan.decode(e, ref), reps)
    seg_off = torch.from_numpy(plan.segments()["off"].astype(np.int64)).cuda()
    stride = int(plan.ch_off[1] - plan.ch_off[0])
    mat = ref.as_strided((C, T), (stride, 1), int(plan.ch_off[0]))
    assert plan.decode_ok()
    out = {}

    def full():
        out["x"] = plan.decode_range(e.payload, seg_off, e.peak, e.enc, None, 0, T)
    # a query the plan has not seen: work list built on the host (after a stream synchronisation) and uploaded
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    full()
    torch.cuda.synchronize()
    res["range_full_first_call_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    # repeated query: the plan's work list is reused, the call only enqueues the zero fill and the decode
    res["range_full_ms"] = median_ms(full, reps)
    assert plan.decode_ok() and torch.equal(out["x"], mat), "full range != mh_decode"
    del out["x"]
    res["range_full_vs_decode"] = round(res["range_full_ms"] / res["decode_ms"], 3)
    for n in (1000, 16384, 1_000_000):
        a = int(rng.randint(0, T - n)) | 1  # odd: not on a piece boundary
        for nc in (C, 96):
            sel = None if nc == C else sorted(rng.choice(C, nc, replace=False).tolist())

            def rng_dec():
                out["x"] = plan.decode_range(e.payload, seg_off, e.peak, e.enc, sel, a, a + n)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rng_dec()
            torch.cuda.synchronize()
            res["range_%d_%d_first_call_wall_ms" % (n, nc)] = round(1e3 * (time.perf_counter() - t0), 3)
            res["range_%d_%d_ms" % (n, nc)] = median_ms(rng_dec, reps)
            rows = mat if sel is None else mat[torch.tensor(sel, device="cuda")]
            assert plan.decode_ok() and torch.equal(out["x"], rows[:, a:a + n]), (n, nc)
    if do_file:
        dense, tot = plan.compact(e)
        torch.cuda.synchronize()
        total = int(tot.item())
        c = container_io.Compressed(container_io.make_header(S, 6, MODE_APPROX, WIN_AFTER_CAL, plan.seg_chunks, tab),
                                    cs.ch_len.copy(), e.peak.cpu().numpy(), e.enc.cpu().numpy(), e.skipped.cpu().numpy(),
                                    e.ch_bits.cpu().numpy().astype(np.uint64),
                                    e.seg_words.cpu().numpy().astype(np.uint64)[:plan.n_segments],
                                    dense.payload[:total].cpu().numpy().view(np.uint32).copy())
        del dense
        with tempfile.TemporaryDirectory() as d:
            fn = os.path.join(d, "set.muahuff")
            container_io.save(fn, c)
            size = os.path.getsize(fn)
            a, n = int(rng.randint(0, T - 16384)) | 1, 16384
            sel = sorted(rng.choice(C, 96, replace=False).tolist())
            with container_io.open(fn) as f:
                f.plan()  # (the plan is created once per file and cached)
                before = f.bytes_read
                t0 = time.perf_counter()
                got = container_io.decompress_range(f, a, a + n, channels=sel)
                torch.cuda.synchronize()
                res["file_16384_96_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
                res["file_16384_96_bytes_read"] = f.bytes_read - before + f.head_bytes
                res["file_head_bytes"] = f.head_bytes
            res["file_bytes"] = size
            assert torch.equal(got, mat[torch.tensor(sel, device="cuda"), a:a + n]), "file range"
    plan.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--S", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--T", type=int, default=10_000_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.RandomState(1)
    out = {"device": muahuff.device_info(0)["name"], "C": args.C, "T": args.T}
    for S in args.S:
        out["S%d" % S] = run(S, args.C, args.T, args.reps, rng, S == args.S[0])
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
