#!/usr/bin/env python3
"""Cost of the payload checksums: mhi_seg_crc32 (k_seg_crc32) next to mh_compact on the same compacted payload -- both
read the same bytes, in the same process, alternated -- and one archive append / one range read with and without
`checksum`.

    python tools/bench_checksum.py [out.txt]     C, T, TB, BLOCKS, SS, DIR (where the files go) from the environment

Event-timed medians of REPS (20) alternated runs.  libmuahuff.so is not touched by the checksums (the kernel lives in
the companion library), so the runs without `checksum` ARE the calls of the library as it was before; they alternate
with the checksummed ones here instead of in a second process."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import muahuff
from muahuff import _ingest, archive, codec, sclv, synth
from muahuff.stream import StreamEncoder

C = int(os.environ.get("C", "1024"))
T = int(os.environ.get("T", "10000000"))
TB = int(os.environ.get("TB", "1000000"))
BLOCKS = int(os.environ.get("BLOCKS", "6"))
REPS = int(os.environ.get("REPS", "20"))
SS = [int(v) for v in os.environ.get("SS", "3,8").split(",")]
DIR = os.environ.get("DIR") or tempfile.mkdtemp()
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def alternated(fns):
    """median event-timed ms of each of fns, REPS rounds, one call of each per round (3 warm-up rounds)"""
    for _ in range(3):
        for f in fns:
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(REPS)]
    for row in ev:
        for f, (a, b) in zip(fns, row):
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    return [float(np.median([row[k][0].elapsed_time(row[k][1]) for row in ev])) for k in range(len(fns))]


def kernel_pair(name, plan, enc):
    """mh_compact of enc and mhi_seg_crc32 over what it packed"""
    dense, tot = plan.compact(enc)
    torch.cuda.synchronize()
    total = int(tot.item())
    crc = torch.zeros(max(plan.n_segments, 1), dtype=torch.int32, device=plan.device)
    bad = _ingest.verify_state(plan.device)
    off, t2 = dense.seg_off, torch.zeros(1, dtype=torch.int64, device=plan.device)
    ms = alternated([
        lambda: plan.compact(enc, dense=dense.payload, off=off, tot=t2),
        lambda: _ingest.seg_crc32(dense.payload, off, enc.seg_words, plan.n_segments, crc=crc),
        lambda: _ingest.seg_crc32(dense.payload, off, enc.seg_words, plan.n_segments, expect=crc, bad=bad)])
    assert bad.tolist() == [0, -1], bad.tolist()
    gb = total * 4 / 1e9
    say("%s: %d segments, %.3f GB compacted" % (name, plan.n_segments, gb))
    say("    mh_compact (reads and writes them)  %8.3f ms   %6.2f TB/s read" % (ms[0], gb / ms[0]))
    say("    mhi_seg_crc32, compute form         %8.3f ms   %6.2f TB/s read   %.2f x the compaction" % (ms[1], gb / ms[1], ms[1] / ms[0]))
    say("    mhi_seg_crc32, verify form          %8.3f ms   %6.2f TB/s read" % (ms[2], gb / ms[2]))
    return gb, ms


say("payload checksums: %d ch x %d bins (compress), %d ch x %d-step stream blocks; medians of %d alternated runs" % (C, T, C, TB, REPS))
results = []
cs = synth.generate(C, T, seed=5, lo=0.2, hi=3.0)
for S in SS:
    plan = codec.Plan(cs.ch_off, cs.ch_len, S, 6, 1, muahuff.WIN_AFTER_CAL, sclv.table(S))
    enc = plan.encode(cs.data)
    results.append((S, ) + kernel_pair("S=%d, %d x %d" % (S, C, T), plan, enc))
    plan.close()
    del enc
del cs
torch.cuda.empty_cache()

g = torch.Generator(device="cuda").manual_seed(3)
block = (torch.rand((TB, C), device="cuda", generator=g) < 0.3).to(torch.uint8) + \
        (torch.rand((TB, C), device="cuda", generator=g) < 0.1).to(torch.uint8)
se = StreamEncoder(C, 3, 6, sclv.table(3))
se.calibrate(block)
_dense, _tot, slot = se.encode_block_device(block)
gb_block, ms_block = kernel_pair("S=3 stream block, %d x %d" % (C, TB), slot["plan"], slot["enc"])
se.close()

say("against the estimate made before the kernel existed (LDS-bound, about 7 LDS cycles per random ds_read_b32 wave"
    " instruction, one lookup per byte): 0.3-0.5 ms + 0.2 ms VALU for 1.85 GB, a few tens of us for a 1024 x 1e6 block")
for S, gb, ms in results:
    say("    S=%d: %.3f GB in %.3f ms = %.3f ms per 1.85 GB -> %.1f x the estimate's upper end (0.7 ms)"
        % (S, gb, ms[1], ms[1] * 1.85 / gb, ms[1] * 1.85 / gb / 0.7))
say("    stream block: %.3f GB in %.1f us" % (gb_block, ms_block[1] * 1e3))


def append_all(fn, checksum, pipeline):
    t0 = time.perf_counter()
    with archive.create(fn, C, S=3, pipeline=pipeline, checksum=checksum) as w:
        for _ in range(BLOCKS):
            w.append(block)
    return time.perf_counter() - t0


say("archive, %d blocks of %d x %d, S=3, files under %s (page cache, no fsync)" % (BLOCKS, C, TB, DIR))
fns = {k: os.path.join(DIR, "sum%d.mua" % k) for k in (0, 1)}
for k in (0, 1):
    append_all(fns[k], bool(k), True)       # warm-up: plans, pinned buffers, page cache
for rep in range(3):
    for k in (0, 1):
        for pipeline in (True, False):
            wall = append_all(fns[k], bool(k), pipeline)
            say("    append  checksum=%-5s pipeline=%-5s rep %d: %7.3f s  %7.2f ms per block  file %.3f GB"
                % (bool(k), pipeline, rep, wall, wall / BLOCKS * 1e3, os.path.getsize(fns[k]) / 1e9))
del block
readers = {k: archive.open(fns[k]) for k in (0, 1)}
cases = [("no checksums, check=True ", readers[0], True), ("checksums,    check=True ", readers[1], True),
         ("checksums,    check=False", readers[1], False)]
ts = {name: [] for name, _r, _c in cases}
for rep in range(REPS + 1):
    for name, r, check in cases:
        t0 = time.perf_counter()
        r.read(TB - 8192, TB + 8192, check=check)
        torch.cuda.synchronize()
        ts[name].append((time.perf_counter() - t0) * 1e3)
for name, r, _c in cases:
    say("    read of 16384 steps x %d channels across a block boundary, %s: first %.2f ms, then median %.2f ms (min %.2f)"
        % (C, name, ts[name][0], float(np.median(ts[name][1:])), min(ts[name][1:])))
t0 = time.perf_counter()
assert readers[1].verify() == []
say("    verify() of the whole file on the device: %.2f s" % (time.perf_counter() - t0))
for k in (0, 1):
    readers[k].close()
    os.remove(fns[k])
