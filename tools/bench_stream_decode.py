#!/usr/bin/env python3
"""Receiving side of the stream path at 1024 ch x 1e7 steps per block, S = 3 and S = 5, in one process, alternating:

  A  byte path: a byte-layout plan's mh_decode into one byte per sample, channel-major, then mh_interleave -- plan and
     buffers cached, i.e. the best the old kernels can do per block;
  B  StreamDecoder.decode_block_device: segment-offset scan, mh_decode_packed into 2- / 4-bit chunk-blocked pieces,
     mh_interleave_packed.

Both decode the same dense stream (StreamEncoder.encode_block_device) and are checked against each other once.  Each
block is timed with device events after warm-up; min / median / max per block and GB/s on algorithmic bytes (1 + b/8
per sample, b = payload bits per sample).  ITERS / WARMUP / C / T override the defaults (a profiler run uses few)."""
import ctypes as ct
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import muahuff
from muahuff import MODE_APPROX, WIN_FULL, _lib, codec, sclv
from muahuff.container import ChannelSet
from muahuff.stream import StreamDecoder, StreamEncoder

C = int(os.environ.get("C", "1024"))
T = int(os.environ.get("T", "10000000"))
ITERS = int(os.environ.get("ITERS", "10"))
WARMUP = int(os.environ.get("WARMUP", "3"))


def block(S, seed):
    """[T, C] counts: ~Poisson-like rates, a sprinkle of large ones; generated in slabs (no 40-GB float temporaries)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((T, C), dtype=torch.uint8, device="cuda")
    for t0 in range(0, T, 1 << 20):
        n = min(1 << 20, T - t0)
        r = torch.rand((n, C), device="cuda", generator=g)
        x[t0:t0 + n] = (r < 0.3).to(torch.uint8) + (r < 0.1).to(torch.uint8) + (r < 0.001).to(torch.uint8) * 20
    return x


def stats(ms, nbytes):
    ms = np.asarray(ms)
    return "min %.3f  median %.3f  max %.3f ms/block  (%.0f GB/s at the median)" % (
        ms.min(), np.median(ms), ms.max(), nbytes / np.median(ms) / 1e6)


for S in (3, 5):
    x = block(S, S)
    tab = sclv.table(S)
    se = StreamEncoder(C, S, 6, tab)
    se.calibrate(x[:64])
    dense, tot, slot = se.encode_block_device(x)
    torch.cuda.synchronize()
    nseg = slot["plan"].n_segments
    total = int(tot.item())
    payload = dense.payload[:total + 4].clone()
    seg_words, seg_off = dense.seg_words[:nseg].clone(), dense.seg_off[:nseg].clone()
    peak, enc = se.peak.clone(), se.enc.clone()
    seg_chunks = slot["plan"].seg_chunks
    se.close()
    del dense, slot
    torch.cuda.empty_cache()
    b = total * 32.0 / (T * C)
    nbytes = T * C * (1 + b / 8)
    # A: byte-layout plan + buffers, built once
    cs = ChannelSet.empty([T] * C)
    plan_a = codec.Plan(cs.ch_off, cs.ch_len, S, 0, MODE_APPROX, WIN_FULL, tab, seg_chunks=seg_chunks)
    e = codec.Encoded(payload, seg_words, torch.zeros(C, dtype=torch.int64, device="cuda"), peak, enc,
                      torch.zeros(C, dtype=torch.uint8, device="cuda"), seg_off, True)
    d_off = torch.from_numpy(cs.ch_off.astype(np.int64)).cuda()
    out_a = torch.empty((T, C), dtype=torch.uint8, device="cuda")

    def run_a():
        plan_a.decode(e, cs.data)
        _lib.check(_lib.lib().mh_interleave(ct.c_void_p(cs.data.data_ptr()), ct.c_void_p(d_off.data_ptr()), T, C,
                                            ct.c_void_p(out_a.data_ptr()), ct.c_void_p(torch.cuda.current_stream().cuda_stream)))

    # B: the stream decoder (its slot is built by the first call)
    sd = StreamDecoder(C, S, tab, seg_chunks=seg_chunks)

    def run_b():
        return sd.decode_block_device(payload, seg_words, peak, enc, T)

    run_a()
    out_b = run_b()
    torch.cuda.synchronize()
    assert plan_a.decode_ok() and sd.ok()
    assert torch.equal(out_a, out_b), "A and B disagree"
    for t0 in range(0, T, 1 << 20):
        assert torch.equal(out_b[t0:t0 + (1 << 20)], torch.clamp(x[t0:t0 + (1 << 20)], max=S - 1))
    del x
    torch.cuda.empty_cache()
    for _ in range(WARMUP):
        run_a()
        run_b()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)] for k in "AB"}
    for i in range(ITERS):
        for k, f in (("A", run_a), ("B", run_b)):
            ev[k][i][0].record()
            f()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(z) for a, z in ev[k]] for k in "AB"}
    print("S=%d  %d ch x %d steps, %.3f payload bits/sample, %d segments" % (S, C, T, b, nseg), flush=True)
    print("  A byte path (mh_decode + mh_interleave): " + stats(ms["A"], nbytes), flush=True)
    print("  B StreamDecoder.decode_block_device:     " + stats(ms["B"], nbytes), flush=True)
    print("  B / A median: %.3f" % (np.median(ms["B"]) / np.median(ms["A"])), flush=True)
    sd.close()
    plan_a.close()
    del cs, out_a, out_b, payload, e
    torch.cuda.empty_cache()
