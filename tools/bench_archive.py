#!/usr/bin/env python3
"""Recording archive: append throughput of the pipelined and the plain writer against the loop of
StreamEncoder.encode_block + container_io.write, and a range read across a block boundary.

    python tools/bench_archive.py [out.txt]      C, TB, BLOCKS, DIR (where the files go) from the environment

GPU idle share = 1 - BLOCKS x (event-timed device work of one block) / wall time of the run: the part of the run in
which no kernel of the recorder was running.  Files are written through the page cache (no fsync) and removed."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from muahuff import archive, container_io, sclv
from muahuff.stream import StreamEncoder

C = int(os.environ.get("C", "1024"))
TB = int(os.environ.get("TB", "1000000"))
BLOCKS = int(os.environ.get("BLOCKS", "20"))
DIR = os.environ.get("DIR") or tempfile.mkdtemp()
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def writer(fn, S, block, pipeline):
    t0 = time.perf_counter()
    with archive.create(fn, C, S=S, pipeline=pipeline) as w:
        for _ in range(BLOCKS):
            w.append(block)
    return time.perf_counter() - t0


def parent_loop(fn, S, block):
    t0 = time.perf_counter()
    se = StreamEncoder(C, S, 6, sclv.table(S))
    se.calibrate(block)
    with open(fn, "wb") as f:
        for _ in range(BLOCKS):
            container_io.write(f, se.encode_block(block))
    se.close()
    return time.perf_counter() - t0


say("recording archive, %d ch x %d steps per block, %d blocks, files under %s (page cache, no fsync)" % (C, TB, BLOCKS, DIR))
for S in (3, 5):
    g = torch.Generator(device="cuda").manual_seed(S)
    block = (torch.rand((TB, C), device="cuda", generator=g) < 0.3).to(torch.uint8) + \
            (torch.rand((TB, C), device="cuda", generator=g) < 0.1).to(torch.uint8)
    se = StreamEncoder(C, S, 6, sclv.table(S))
    se.calibrate(block)
    for _ in range(3):
        se.encode_block_device(block)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        se.encode_block_device(block)
    b.record()
    torch.cuda.synchronize()
    dev_ms = a.elapsed_time(b) / 10
    se.close()
    fn = os.path.join(DIR, "bench_s%d.mua" % S)
    say("S=%d  device work per block (de-interleave + preset encode + compaction): %.3f ms" % (S, dev_ms))
    cases = (("pipeline=True ", lambda: writer(fn, S, block, True)), ("pipeline=False", lambda: writer(fn, S, block, False)),
             ("parent loop   ", lambda: parent_loop(fn, S, block)))
    for name, f in cases:      # warm-up: plans, pinned buffers, page cache
        f()
    for rep in range(2):
        for name, f in cases:
            wall = f()
            size = os.path.getsize(fn)
            say("S=%d  %s  rep %d: %7.3f s  %6.2f GSamples/s  file %.2f GB (%.2f GB/s)  GPU idle %.1f %%"
                % (S, name, rep, wall, BLOCKS * TB * C / wall / 1e9, size / 1e9, size / wall / 1e9,
                   100 * (1 - BLOCKS * dev_ms / 1e3 / wall)))
    # range read across the boundary of blocks 0 and 1 of the pipelined writer's file
    writer(fn, S, block, True)
    del block
    for check in (True, False):
        with archive.open(fn) as ar:
            ts = []
            for _ in range(10):
                t0 = time.perf_counter()
                ar.read(TB - 8192, TB + 8192, check=check)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            say("S=%d  read of 16384 steps x %d channels across a block boundary, check=%s: first %.2f ms, then median %.2f ms "
                "(min %.2f), %.2f MB read from the file" % (S, C, check, ts[0], float(np.median(ts[1:])), min(ts[1:]), ar.bytes_read / 1e6))
    os.remove(fn)
