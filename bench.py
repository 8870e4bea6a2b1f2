#!/usr/bin/env python3
"""Headline benchmark: MSamples/s for static-Huffman encode+decode of synthetic Poisson MUA.

    python bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over the rank's resident batch: calibrate + encode every
channel's window into the chunked bitstream, then decode it back (both whole-batch kernels,
inputs already in HBM).  N=1 runs BASELINE.json configs[2] (1024 channels x 1e7 bins, the
HBM-roofline run) at the reference's chosen design point S=3, 2^6-sample calibration
histogram, 1 encoder (Compressing data/test_chosen_system.py:22-27); N>1 keeps the same
per-GPU work (weak scaling; configs[3]'s 10 000-channel set is 1250 channels/GPU:
--channels-per-gpu 1250).  Channels shard across ranks with no data-path collective; the RCCL
gather that concatenates the packed bitstream is run once after the timed region and
reported separately under "gather".

Launching: with --gpus N > 1 and no WORLD_SIZE in the environment this process becomes a
launcher -- before any GPU call it starts N ranks (python -m torch.distributed.run, one per
GPU, rendezvous on 127.0.0.1), relays their output and exits with their worst status.  Under
torchrun (WORLD_SIZE set) it is a rank.  A failed or stuck gather is recorded in the JSON line
AND turns the exit status non-zero.

Prints ONE JSON line on rank 0 (contract in the task statement) with two extra objects:
"roofline" (dominant kernel against the 8 TB/s HBM peak, plus per_S: every dynamic range of
the reference's sweep) and "cpu_baseline" (the CPU oracle timed on a bounded sample on this
host's cores).

--dump-outputs DIR writes what the last timed step computed (the encoded container and the decoded
channels, a seeded sample of the large arrays) as DIR/<name>.npy, for comparing two builds output
for output; the inputs depend on the arguments only (synth.generate, --seed).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6.3 TB/s is what a copy reaches
PMC_FILES = ("r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")

RC_GATHER_STUCK, RC_GATHER_FAILED, RC_BAD_LAUNCH = 3, 4, 2


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=250, help="default keeps the timed region above one second")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--channels-per-gpu", type=int, default=1024)
    ap.add_argument("--bins", type=int, default=10_000_000)
    ap.add_argument("--S", type=int, default=3)
    ap.add_argument("--hist-bits", type=int, default=6)
    ap.add_argument("--mode", type=int, default=1, help="1 approx-sort mapper, 0 no-sort")
    ap.add_argument("--seg-chunks", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-channels", type=int, default=96)
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--no-per-S", action="store_true", help="skip the per-dynamic-range sweep (roofline.per_S)")
    ap.add_argument("--no-small-shape", action="store_true", help="skip the short-channel extra (small_shape)")
    ap.add_argument("--gather-deadline", type=int, default=240, help="seconds allowed for the untimed payload gather")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL) for real runs; gloo only to rehearse "
                    "the multi-rank control flow on a box with fewer GPUs than ranks")
    ap.add_argument("--check-launch", action="store_true",
                    help="ranks rendezvous, barrier and report; no codec work and no metric (launcher self-test, runs without a GPU)")
    ap.add_argument("--verify", action="store_true", help="round-trip check after the timed region")
    ap.add_argument("--placement-tries", type=int, default=4,
                    help="payload / output buffers are chosen among this many candidates by a short timing of the real op "
                         "(codec.Plan.alloc_encoded_probed: the part runs the same kernel at one of two levels depending on "
                         "which physical pages hold its buffers); 1 = take the first allocation.  Setup, outside the timed "
                         "region; every candidate's time is reported under \"placement\"")
    ap.add_argument("--total-channels", type=int, default=10_000,
                    help="BASELINE configs[3]: a FIXED set of this many channels x --bins sharded over the ranks "
                         "(strong scaling, reported as the extra block \"configs3\")")
    ap.add_argument("--configs3-steps", type=int, default=3)
    ap.add_argument("--no-configs3", action="store_true", help="skip the configs[3] strong-scaling block")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (encoded container and decoded "
                         "channels) as DIR/<name>.npy, float32 / float64, 64 MB at most (see dump_outputs)")
    return ap.parse_args(argv)


# ---- launcher ------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(a, argv):
    """--gpus N > 1 without a launcher: start the N ranks ourselves.  Nothing here touches the GPU
    (torch.cuda.device_count() does not initialise HIP on this image), and the ranks are CHILD
    processes -- this process is never replaced."""
    if a.dist_backend == "nccl":
        ndev = torch.cuda.device_count()
        if ndev < a.gpus:
            sys.stderr.write("bench.py: --gpus %d needs %d visible GPUs, this box has %d (RCCL runs one rank per GPU; "
                             "--dist-backend gloo only rehearses the control flow)\n" % (a.gpus, a.gpus, ndev))
            return RC_BAD_LAUNCH
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % a.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


# ---- helpers -------------------------------------------------------------------------------------
def cpu_baseline(cs_host, ch_off, ch_len, S, h, mode, tab, seg_chunks, n_ch):
    """The CPU oracle (oracle/mh_oracle.c, kind "port") timed on the first n_ch channels of the
    same workload: 1 thread, then all host cores.  Checker code used as a reported baseline
    only -- it is not on the measured GPU path."""
    import oracle
    OC = oracle.c
    off = np.ascontiguousarray(ch_off[:n_ch])
    ln = np.ascontiguousarray(ch_len[:n_ch])
    p = OC.Params(S, h, mode, OC.WIN_AFTER_CAL, tab, seg_chunks=seg_chunks)
    samples = int((ln - np.minimum(ln, 2 ** h)).sum())
    res = {}
    for tag, nt in (("1", 1), ("all", os.cpu_count() or 1)):
        t0 = time.perf_counter()
        e = OC.encode(cs_host, off, ln, p, nthreads=nt)
        t1 = time.perf_counter()
        OC.decode(e["payload"], off, ln, p, e["peak"], e["enc"], len(cs_host), nthreads=nt)
        t2 = time.perf_counter()
        res[tag] = dict(threads=nt, enc_s=t1 - t0, dec_s=t2 - t1,
                        msamples_s=samples / (t2 - t0) / 1e6)
        if tag == "1" and (t2 - t0) > 25:
            break
    # NumPy single process, measure only: how the reference itself executes (one channel)
    ONP = oracle.np_
    x = cs_host[int(off[0]):int(off[0]) + int(ln[0])]
    t0 = time.perf_counter()
    st = ONP.channel_stats(np.minimum(x, S - 1), S, 2 ** h, bool(mode))
    t_np = time.perf_counter() - t0
    res["numpy_measure_msamples_s"] = (st["e"] - st["c"]) / t_np / 1e6
    return samples, res


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def pmc_traffic(kernel, C, T, S, h, seg_chunks):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes (FETCH_SIZE and
    WRITE_SIZE cannot be collected while timing; they come from separate --pmc runs of this
    same command, tools/collect_pmc_traffic.sh).  None when the workload differs."""
    for name in PMC_FILES:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                d = json.load(f)
            w = d["workload"]
            if (w["channels_per_gpu"], w["bins"], w["S"], w["hist_bits"], w["seg_chunks"]) != (C, T, S, h, seg_chunks):
                continue
            return d["kernels"][kernel]["hbm_bytes"], "profiles/%s (rocprofv3 --pmc, gfx950 FETCH x2)" % name
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def event_times(fn, reps, warm=2):
    """ms per call of fn() (enqueues work on torch's current stream), one HIP event pair per call."""
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a_, b_ in ev:
        a_.record()
        fn()
        b_.record()
    torch.cuda.synchronize()
    return [a_.elapsed_time(b_) for a_, b_ in ev]


def stats(ms):
    v = np.asarray(ms, dtype=np.float64)
    return {"min": float(v.min()), "median": float(np.median(v)), "mean": float(v.mean()), "max": float(v.max())}


def per_S_sweep(cs, out, h, mode, seg_chunks, reps=5, tries=3):
    """Encode / decode of the same resident batch at every dynamic range of the reference's sweep
    (S = 2..10 with all K encoders of that S, get_BR_with_approx_sort.py:107,120-125): event-timed
    ops against their algorithmic bytes.  Outside the timed region."""
    import muahuff
    from muahuff import codec, sclv
    rows = []
    for S in range(2, 11):
        tab = sclv.table(S)
        plan = codec.Plan(cs.ch_off, cs.ch_len, S, h, mode, muahuff.WIN_AFTER_CAL, tab, seg_chunks=seg_chunks)
        enc, _ = plan.alloc_encoded_probed(cs.data, tries=tries, reps=3)
        e_ms = event_times(lambda: plan.encode(cs.data, out=enc), reps)
        d_ms = event_times(lambda: plan.decode(enc, out), reps)
        n = plan.window_samples
        b = float(enc.ch_bits.sum().item()) / n
        ab = n * (1.0 + b / 8.0)
        em, dm = float(np.median(e_ms)), float(np.median(d_ms))
        rows.append({"S": S, "K": int(tab.shape[0]), "bits_per_sample": b, "encode_ms": em, "decode_ms": dm,
                     "encode_GBps": ab / em / 1e6, "decode_GBps": ab / dm / 1e6,
                     "encode_frac": ab / em / 1e6 / HBM_PEAK_GBS, "decode_frac": ab / dm / 1e6 / HBM_PEAK_GBS})
        plan.close()
        del enc
    return rows


def choose_buffers(plan, data, tries):
    """Input copy, payload and output buffer of the timed region.  The part runs the same kernel at one of two levels
    (encode 1.97 / 2.1 ms, decode 1.94 / 2.0-2.1 ms) depending on which physical pages hold the buffers it reads and
    writes, about one (input, payload) pair in four being on the fast one -- and what the decoder
    gets depends on the payload it reads as well as on the output it writes.  So: up to 4 input copies x 4 payload buffers
    timed with the encoder alone; the three best pairs x 4 output buffers timed as the headline runs them, encode and
    decode alternating; the best triple is kept.  Setup, outside the timed region; every number goes into the line.
    -> (data, Encoded, out, report)"""
    from muahuff.codec import _median_ms
    if tries <= 1:
        return data, plan.alloc_encoded(), torch.empty_like(data), {"what": "first allocations (--placement-tries 1)"}
    inputs = [data] + [data.clone() for _ in range(min(3, tries - 1))]
    table, pairs = [], []
    for i, dat in enumerate(inputs):
        row = []
        for _ in range(min(4, tries)):
            e = plan.alloc_encoded()
            ms = _median_ms(lambda: plan.encode(dat, out=e), 4)
            row.append(ms)
            pairs.append((ms, i, e))
        table.append(row)
    pairs.sort(key=lambda t: t[0])
    top = pairs[:3]
    del pairs, e
    torch.cuda.empty_cache()
    outs = [torch.empty_like(data) for _ in range(min(4, tries))]
    joint, best = [], None
    for _, i, e in top:
        row = []
        for o in outs:
            def step():
                plan.encode(inputs[i], out=e)
                plan.decode(e, o)
            ms = _median_ms(step, 3)
            row.append(ms)
            if best is None or ms < best[0]:
                best = (ms, i, e, o)
        joint.append(row)
    report = {"what": "input copy, payload and output buffer of the timed region chosen among candidates alive at the same "
                      "time: every (input copy, payload) pair timed with 4 encodes (ms per pair), then the three best "
                      "pairs x every output candidate timed as 3 x (encode, decode) (ms per pair and output); setup, untimed",
              "encode_ms_per_input_and_payload_candidate": table,
              "encode_plus_decode_ms_per_top_pair_and_output_candidate": joint,
              "chosen_encode_plus_decode_ms": best[0]}
    return inputs[best[1]], best[2], best[3], report


DUMP_BYTES = 64 << 20


def _sample_positions(starts, lengths, cap, seed):
    """Positions of the elements of the runs [starts[i], starts[i] + lengths[i]), in order: all of them when there are
    at most `cap`, else a sorted sample drawn by a generator seeded by `seed` and the element count (the same
    arguments always give the same positions)."""
    cum = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    n = int(cum[-1])
    if n <= cap:
        j = np.arange(n, dtype=np.int64)
    else:
        j = np.unique(np.random.default_rng(list(seed) + [n]).integers(0, n, size=cap, dtype=np.int64))
    r = np.searchsorted(cum, j, side="right") - 1
    return np.asarray(starts, dtype=np.int64)[r] + (j - cum[r])


def dump_outputs(d, plan, cs, enc, out, seed, rank, world):
    """--dump-outputs: what the last timed step handed its caller -- the Encoded container of plan.encode and the
    channel bytes plan.decode wrote -- as d/<name>.npy, so that two builds can be compared output for output.
    Integers are stored as float64 (exact below 2^53), bytes as float32.  Each array has a fixed share of the
    64 MB budget: it is written whole when it fits, else as a seeded sample (_sample_positions, seed = (--seed, rank)).
    payload_words holds only the words the segments use (seg_words; the rest of a slot is never written), decoded
    the bytes of the channels.  With several ranks each writes its own shard as <name>_rank<r>.npy, in a
    1/world share.  -> {file name: shape}"""
    os.makedirs(d, exist_ok=True)
    share = (DUMP_BYTES - (64 << 10)) // world     # (64 KB left for the .npy headers)
    seed = (seed, rank)
    written = {}

    def save(name, a):
        fn = name if world == 1 else "%s_rank%d" % (name, rank)
        np.save(os.path.join(d, fn + ".npy"), a)
        written[fn] = list(a.shape)

    n_seg = plan.n_segments
    seg_words = enc.seg_words.cpu().numpy()[:n_seg]
    for name, t, n, dt, frac in (("ch_bits", enc.ch_bits, plan.C, np.float64, 1 / 8),
                                 ("peak", enc.peak, plan.C, np.float32, 1 / 24),
                                 ("enc", enc.enc, plan.C, np.float32, 1 / 24),
                                 ("skipped", enc.skipped, plan.C, np.float32, 1 / 24),
                                 ("seg_words", enc.seg_words, n_seg, np.float64, 1 / 8)):
        host = t.cpu().numpy()[:n]
        save(name, host[_sample_positions([0], [n], int(share * frac) // np.dtype(dt).itemsize, seed)].astype(dt))
    for name, buf, starts, lengths, dt, frac in (
            ("payload_words", enc.payload, plan.segments()["off"], seg_words, np.float64, 3 / 8),
            ("decoded", out, cs.ch_off, cs.ch_len, np.float32, 1 / 4)):
        pos = _sample_positions(starts, lengths, int(share * frac) // np.dtype(dt).itemsize, seed)
        if pos.size and not (0 <= int(pos.min()) and int(pos.max()) < buf.numel()):
            raise RuntimeError("dump_outputs: %s positions outside the buffer" % name)
        v = buf.index_select(0, torch.from_numpy(pos).to(buf.device)).cpu().numpy()
        save(name, (v.view(np.uint32) if v.dtype == np.int32 else v).astype(dt))
    return written


def small_shape(S, h, mode, seg_chunks, reps=20):
    """The reference's real shape: 50 ms bins give 2e4-7e4 samples per channel
    (Data/get_all_binned_data.py:16; training set ~2400 channels, get_BR_with_approx_sort.py:24,89-90).
    2400 channels x 72 000 bins, same design point, event-timed ops.  Not the headline."""
    import muahuff
    from muahuff import codec, sclv, synth
    C, T = 2400, 72_000
    tab = sclv.table(S)
    cs = synth.generate(C, T, seed=5)
    plan = codec.Plan(cs.ch_off, cs.ch_len, S, h, mode, muahuff.WIN_AFTER_CAL, tab, seg_chunks=seg_chunks)
    enc = plan.alloc_encoded()
    out = torch.empty_like(cs.data)
    e_ms = event_times(lambda: plan.encode(cs.data, out=enc), reps, warm=3)
    d_ms = event_times(lambda: plan.decode(enc, out), reps, warm=3)

    side = torch.cuda.Stream()

    def back_to_back(f, n=50):
        """ms per op of n launches of the same op replayed as ONE hipGraph between one pair of events: the GPU-side
        cost of the op in a pipeline over many recordings, free of the host's per-call time.  (An event pair around a
        single launch also times the idle queue's start-up: an EMPTY kernel reads 5.8 us that way and 1.5 us back to
        back -- tools/enc_probe, profiles/r03_short_channels.txt.)"""
        with torch.cuda.stream(side):
            f()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(n):
                    f()
            g.replay()
            ts = []
            for _ in range(5):
                a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a_.record()
                g.replay()
                b_.record()
                b_.synchronize()
                ts.append(a_.elapsed_time(b_) / n)
        torch.cuda.synchronize()
        del g
        return float(np.median(ts))

    e_bb = back_to_back(lambda: plan.encode(cs.data, out=enc))
    d_bb = back_to_back(lambda: plan.decode(enc, out))
    # the reference's own computation on this shape (calibrate + window histogram + bits, its [c, c+T/2) window)
    plan_m = codec.Plan(cs.ch_off, cs.ch_len, S, h, mode, muahuff.WIN_REF_HALF, tab)
    m_out = plan_m.measure(cs.data)
    m_ms = float(np.median(event_times(lambda: plan_m.measure(cs.data, out=m_out), reps, warm=3)))
    m_n = plan_m.window_samples
    plan_m.close()
    n = plan.window_samples
    b = float(enc.ch_bits.sum().item()) / n
    ab = n * (1.0 + b / 8.0)
    em, dm = float(np.median(e_ms)), float(np.median(d_ms))
    plan.close()
    # the widest dynamic range of the reference's sweep on the same shape (S = 10, all 35 encoders): long codes are
    # where short channels are furthest from the roofline
    S10 = 10
    tab10 = sclv.table(S10)
    plan10 = codec.Plan(cs.ch_off, cs.ch_len, S10, h, mode, muahuff.WIN_AFTER_CAL, tab10, seg_chunks=seg_chunks)
    enc10 = plan10.alloc_encoded()
    e10 = float(np.median(event_times(lambda: plan10.encode(cs.data, out=enc10), reps, warm=3)))
    d10 = float(np.median(event_times(lambda: plan10.decode(enc10, out), reps, warm=3)))
    e10_bb = back_to_back(lambda: plan10.encode(cs.data, out=enc10))
    d10_bb = back_to_back(lambda: plan10.decode(enc10, out))
    b10 = float(enc10.ch_bits.sum().item()) / n
    ab10 = n * (1.0 + b10 / 8.0)
    plan10.close()
    pm10 = codec.Plan(cs.ch_off, cs.ch_len, S10, h, mode, muahuff.WIN_REF_HALF, tab10)
    mo10 = pm10.measure(cs.data)
    m10 = float(np.median(event_times(lambda: pm10.measure(cs.data, out=mo10), reps, warm=3)))
    pm10.close()
    s10 = {"S": S10, "K": int(tab10.shape[0]), "bits_per_sample": b10, "encode_us": e10 * 1e3, "decode_us": d10 * 1e3,
           "encode_frac": ab10 / e10 / 1e6 / HBM_PEAK_GBS, "decode_frac": ab10 / d10 / 1e6 / HBM_PEAK_GBS,
           "measure_us": m10 * 1e3, "measure_frac": m_n / m10 / 1e6 / HBM_PEAK_GBS,
           "back_to_back": {"encode_us": e10_bb * 1e3, "decode_us": d10_bb * 1e3,
                            "encode_frac": ab10 / e10_bb / 1e6 / HBM_PEAK_GBS, "decode_frac": ab10 / d10_bb / 1e6 / HBM_PEAK_GBS}}
    return {"workload": "2400 channels x 72 000 bins (50 ms bins), S=%d, 2^%d calibration" % (S, h),
            "samples": n, "bits_per_sample": b, "encode_us": em * 1e3, "decode_us": dm * 1e3,
            "encode_GBps": ab / em / 1e6, "decode_GBps": ab / dm / 1e6,
            "encode_frac": ab / em / 1e6 / HBM_PEAK_GBS, "decode_frac": ab / dm / 1e6 / HBM_PEAK_GBS,
            "measure_us": m_ms * 1e3, "measure_GBps": m_n / m_ms / 1e6, "measure_frac": m_n / m_ms / 1e6 / HBM_PEAK_GBS,
            "back_to_back": {"encode_us": e_bb * 1e3, "decode_us": d_bb * 1e3,
                             "encode_frac": ab / e_bb / 1e6 / HBM_PEAK_GBS, "decode_frac": ab / d_bb / 1e6 / HBM_PEAK_GBS,
                             "what": "50 launches of the op captured in one hipGraph, replayed between one pair of events / 50, median of 5"},
            "S10": s10,
            "timing": "HIP events around each op (calibrate/table kernel + codec kernel), median of %d; an event pair "
                      "around ONE launch includes the idle queue's start-up (an empty kernel reads 5.8 us that way, "
                      "1.5 us back to back), hence the second set" % reps}


def configs3_block(a, rank, world, dist, coll_dev, tab):
    """BASELINE configs[3] / north_star's scaling claim: ONE fixed set of --total-channels channels x --bins
    (10 000 x 1e7 = 100 GB of counts) sharded in contiguous channel blocks over the ranks -- 1250 channels per GPU
    at N = 8, all 10 000 on one GPU at N = 1 (100 GB in + 100 GB out + 26 GB of slots fit the 288 GB part) -- so the
    per-N lines of this block are STRONG scaling of the same job.  Every rank generates its own shard
    (synth.generate(first_channel=lo): channel c is the same whoever owns it), encodes and decodes it; time =
    max over ranks, barrier + synchronize on both sides, as for the headline.  Runs after the headline's buffers
    are free.  -> dict for the JSON line (all ranks must call it; rank 0 uses the result)."""
    import muahuff
    from muahuff import codec, dist as mdist, synth
    S, h, T = a.S, a.hist_bits, a.bins
    lo, hi = mdist.shard_channels(a.total_channels, world, rank)
    n_ch = hi - lo
    # counts + decoded output + slots (maxlen bits per sample, headers, alignment) + slack
    need = int(n_ch * T * (2.0 + float(tab.max()) / 8.0 * 1.05)) + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    fits = torch.tensor([1.0 if (n_ch > 0 and free >= need) else 0.0], dtype=torch.float64, device=coll_dev)
    if dist is not None:
        dist.all_reduce(fits, op=dist.ReduceOp.MIN)
    if float(fits.item()) == 0.0:
        return {"skipped": "rank %d: shard of %d channels needs %.0f GB, %.0f GB free" % (rank, n_ch, need / 1e9, free / 1e9)}

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    cs = synth.generate(n_ch, T, seed=a.seed, first_channel=lo)
    plan = codec.Plan(cs.ch_off, cs.ch_len, S, h, a.mode, muahuff.WIN_AFTER_CAL, tab, seg_chunks=a.seg_chunks)
    enc = plan.alloc_encoded()
    out = torch.empty_like(cs.data)
    plan.encode(cs.data, out=enc)
    plan.decode(enc, out)
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.configs3_steps):
        plan.encode(cs.data, out=enc)
        plan.decode(enc, out)
    barrier()
    dt = time.perf_counter() - t0
    acc = torch.tensor([float(plan.window_samples), float(enc.ch_bits.sum().item()), float(enc.seg_words.sum().item())],
                       dtype=torch.float64, device=coll_dev)
    tmax = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
    if dist is not None:
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    ok = None
    if a.verify:  # channel blocks, so that the check needs no second copy of the shard
        ok, c = True, 2 ** h
        for c0 in range(0, n_ch, 64):
            c1 = min(n_ch, c0 + 64)
            vin = cs.matrix()[c0:c1, c:]
            vout = cs.matrix(out)[c0:c1, c:]
            ok = ok and bool(torch.equal(torch.clamp(vin, max=S - 1), vout))
        okt = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=coll_dev)
        if dist is not None:
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        ok = bool(okt.item() == 1.0)
    plan.close()
    del cs, enc, out
    torch.cuda.empty_cache()
    samples, bits, words = (float(v) for v in acc.tolist())
    dt = float(tmax.item())
    res = {"workload": "BASELINE configs[3]: synthetic Poisson MUA, %d channels x %.0e bins in all, sharded over %d GPU(s)"
                       % (a.total_channels, T, world),
           "scaling": "strong", "total_channels": a.total_channels, "channels_rank0": n_ch, "steps": a.configs3_steps,
           "ms_per_step": dt / a.configs3_steps * 1e3, "MSamples_s": samples * a.configs3_steps / dt / 1e6,
           "bits_per_sample": bits / samples, "payload_bytes_total": words * 4.0}
    if ok is not None:
        res["verified_roundtrip"] = ok
    return res


def configs3_guarded(a, rank, world, dist, coll_dev, tab, local, deadline):
    """configs3_block in a helper thread under a deadline: the extra block can never cost the run its headline line (an
    allocation failure or a stuck collective becomes {"error": ...}) -- but it does cost the exit status.
    -> (block or error dict, stuck?)"""
    import threading
    box = {}

    def run():
        try:
            torch.cuda.set_device(local)
            box["v"] = configs3_block(a, rank, world, dist, coll_dev, tab)
        except Exception as e:  # noqa: BLE001 -- reported in the line
            box["v"] = {"error": repr(e)}

    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(deadline)
    if th.is_alive():
        return {"error": "configs3 block did not finish within %ds" % deadline}, True
    return box["v"], False


# ---- one rank ------------------------------------------------------------------------------------
def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse(argv)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a, argv))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d; launch N ranks with `python bench.py --gpus N` (it starts "
                         "them itself) or `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`\n"
                         % (a.gpus, world))
        sys.exit(RC_BAD_LAUNCH)
    dist = None
    coll_dev = "cuda" if a.dist_backend == "nccl" else "cpu"
    if a.check_launch:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world > 1:
            dist.init_process_group("gloo")
            t = torch.tensor([float(rank)], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            dist.barrier()
            ok = float(t.item()) == world * (world - 1) / 2
            n_ranks = dist.get_world_size()
            dist.destroy_process_group()
        else:
            ok, n_ranks = True, 1
        if rank == 0:
            print(json.dumps({"check_launch": bool(ok), "n_gpus": world, "ranks": n_ranks}), flush=True)
        sys.exit(0 if ok else RC_BAD_LAUNCH)
    ndev = torch.cuda.device_count()
    if a.dist_backend == "nccl" and world > ndev:
        sys.stderr.write("bench.py: %d ranks but %d visible GPUs (one rank per GPU with RCCL)\n" % (world, ndev))
        sys.exit(RC_BAD_LAUNCH)
    local = local % max(ndev, 1) if a.dist_backend == "gloo" else local
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(a.dist_backend)

    import muahuff
    from muahuff import codec, sclv, synth

    S, h, C, T = a.S, a.hist_bits, a.channels_per_gpu, a.bins
    tab = sclv.table(S)
    cs = synth.generate(C, T, seed=a.seed, first_channel=rank * C)
    plan = codec.Plan(cs.ch_off, cs.ch_len, S, h, a.mode, muahuff.WIN_AFTER_CAL, tab, seg_chunks=a.seg_chunks)
    # Buffers of the timed region: chosen by placement (see --placement-tries, choose_buffers).
    from muahuff.container import ChannelSet
    data_, enc, out, placement = choose_buffers(plan, cs.data, a.placement_tries)
    cs = ChannelSet(data_, cs.ch_off, cs.ch_len)
    del data_
    torch.cuda.empty_cache()
    plan.encode(cs.data, out=enc)
    out.zero_()
    samples = plan.window_samples

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.steps)]

    def step(i=None):
        if i is not None:
            ev[i][0].record()
        plan.encode(cs.data, out=enc)
        if i is not None:
            ev[i][1].record()
        plan.decode(enc, out)
        if i is not None:
            ev[i][2].record()

    for _ in range(a.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i)
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # before anything below reuses `out` (per_S_sweep decodes into it) or frees the buffers
    dumped = dump_outputs(a.dump_outputs, plan, cs, enc, out, a.seed, rank, world) if a.dump_outputs else None
    devices, rank_words = None, None
    if dist is not None:
        devices = [None] * world
        dist.all_gather_object(devices, "%s cuda:%d" % (torch.cuda.get_device_name(local), local))
        rank_words = [None] * world   # words every rank's encoder wrote (sum of seg_words): what the gather must move
        dist.all_gather_object(rank_words, int(enc.seg_words.sum().item()))

    # auxiliary, outside the timed region: mh_measure on the same resident batch with the
    # reference's own window rule [c, c+T/2) -- the only thing the reference itself computes
    plan_m = codec.Plan(cs.ch_off, cs.ch_len, S, h, a.mode, muahuff.WIN_REF_HALF, tab)
    meas = plan_m.measure(cs.data)
    meas_ms = float(np.median(event_times(lambda: plan_m.measure(cs.data, out=meas), 5, warm=1)))
    meas_samples = plan_m.window_samples
    ref_bits_per_sample = float(meas.bits.sum().item()) / max(meas_samples, 1)
    plan_m.close()

    enc_all = [ev[i][0].elapsed_time(ev[i][1]) for i in range(a.steps)]
    dec_all = [ev[i][1].elapsed_time(ev[i][2]) for i in range(a.steps)]
    enc_ms, dec_ms = float(np.mean(enc_all)), float(np.mean(dec_all))
    bits = int(enc.ch_bits.sum().item())
    words = int(enc.seg_words.sum().item())
    b = bits / samples                 # payload bits/sample (== the reference's histogram.SCLV)
    cb = words * 32 / samples          # container bits/sample (headers + padding included)

    gather, rc = None, 0
    if dist is not None and not a.no_gather:
        # Untimed extra: concatenate the packed bitstreams on rank 0 (RCCL point-to-point over
        # xGMI; device tensors end to end).  Run under a deadline in a helper thread so that a
        # stuck collective can never cost the run its JSON line -- but it does cost the exit status.
        import threading
        from muahuff import dist as mdist
        box = {}

        def do_gather():
            torch.cuda.set_device(local)
            dense, tot = plan.compact(enc)
            barrier()
            g0 = time.perf_counter()
            src = dense.payload if coll_dev == "cuda" else dense.payload.cpu()
            pay, offs = mdist.gather_payload(src, int(tot.item()), dst=0)
            barrier()
            g = time.perf_counter() - g0
            box["v"] = dict(ms=g * 1e3, bytes_total=int(offs[-1]) * 4, payload_device=str(src.device),
                            words_per_rank=[int(v) for v in np.diff(offs)],
                            GBps_into_root=(int(offs[-1]) - int(offs[1])) * 4 / g / 1e9)
            if rank == 0 and a.verify:  # the root's copy of its own shard travelled through the same slicing
                box["v"]["root_shard_intact"] = bool(torch.equal(pay[:int(offs[1])].to(dense.payload.device),
                                                                 dense.payload[:int(offs[1])]))
            del pay, src, dense
            # the same gather pipelined behind the encoder: 4 channel blocks per rank, block b is on the
            # wire while block b+1 encodes (dist.gather_payload_pipelined); every block has its own buffers
            try:
                nblk = 4
                plans, encs, bufs = [], [], []
                for k in range(nblk):
                    b0, b1 = mdist.shard_channels(C, nblk, k)
                    pb = codec.Plan(cs.ch_off[b0:b1], cs.ch_len[b0:b1], S, h, a.mode, muahuff.WIN_AFTER_CAL, tab,
                                    seg_chunks=a.seg_chunks)
                    plans.append(pb)
                    encs.append(pb.alloc_encoded())
                    bufs.append(torch.empty(pb.payload_cap_words, dtype=torch.int32, device=pb.device))

                def blocks():
                    for pb, eb, db in zip(plans, encs, bufs):
                        pb.encode(cs.data, out=eb)
                        d_, tot_ = pb.compact(eb, dense=db)
                        yield (d_.payload if coll_dev == "cuda" else d_.payload.cpu()), tot_

                for _ in blocks():  # warm-up of the block plans, untimed
                    pass
                barrier()
                g0 = time.perf_counter()
                pay2, offs2 = mdist.gather_payload_pipelined(blocks(), dst=0)
                barrier()
                g2 = time.perf_counter() - g0
                box["v"]["pipelined"] = dict(blocks=nblk, ms_encode_and_gather=g2 * 1e3,
                                             bytes_total=int(offs2[-1, 0]) * 4)
                for pb in plans:
                    pb.close()
            except Exception as e:  # the plain gather above stands; the failure is reported and fails the run
                box["v"]["pipelined"] = {"error": repr(e)}
                box["rc"] = RC_GATHER_FAILED

        def guarded():
            try:
                do_gather()
            except Exception as e:
                box.setdefault("v", {})["error"] = repr(e)
                box["rc"] = RC_GATHER_FAILED

        th = threading.Thread(target=guarded, daemon=True)
        th.start()
        th.join(a.gather_deadline)
        if th.is_alive():
            gather, rc = {"error": "gather did not finish within %ds" % a.gather_deadline}, RC_GATHER_STUCK
        else:
            gather, rc = box.get("v"), box.get("rc", 0)

    ok = None
    if a.verify:
        c = 2 ** h
        vin = cs.matrix()[:, c:]
        vout = cs.matrix(out)[:, c:]
        ok = bool(torch.equal(torch.clamp(vin, max=S - 1), vout))
        if dist is not None:  # every rank's shard, not just rank 0's
            okt = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
            ok = bool(okt.item() == 1.0)
        del vin, vout

    c3 = None
    if world > 1 and not a.no_configs3 and rc != RC_GATHER_STUCK:  # (N = 1 runs it last, once the per-S sweep no longer needs the headline's buffers)
        plan.close()
        del cs, enc, out, plan
        torch.cuda.empty_cache()
        c3, c3_stuck = configs3_guarded(a, rank, world, dist, coll_dev, tab, local, a.gather_deadline)
        if c3_stuck:
            rc = RC_GATHER_STUCK
        elif "error" in c3:
            rc = rc or RC_GATHER_FAILED

    if rank == 0:
        total_samples = samples * world
        ms_step = dt / a.steps * 1e3
        value = total_samples * a.steps / dt / 1e6
        # dominant kernel = the slower of the two ops of a step
        if enc_ms >= dec_ms:
            kname, kms, abytes, kall = "k_encode2", enc_ms, samples * (1.0 + b / 8.0), enc_all
        else:
            kname, kms, abytes, kall = "k_decode2", dec_ms, samples * (b / 8.0 + 1.0), dec_all
        achieved = abytes / (kms * 1e-3) / 1e9
        traffic, traffic_src = pmc_traffic(kname, C, T, S, h, a.seg_chunks)
        both = {}
        for nm, ms_all in (("k_encode2", enc_all), ("k_decode2", dec_all)):
            ab_ = samples * (1.0 + b / 8.0)
            m_ = float(np.mean(ms_all))
            both[nm] = {"op_ms": stats(ms_all), "achieved": ab_ / (m_ * 1e-3) / 1e9,
                        "frac": ab_ / (m_ * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "traffic": pmc_traffic(nm, C, T, S, h, a.seg_chunks)[0]}
        info = muahuff.device_info(local)
        roof = {"bound": "hbm", "kernel": kname, "achieved": achieved, "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                # the PMC passes cannot run inside a timed run: the figure is read from the committed profile of this
                # same command, not measured by THIS run
                "traffic_measured": False,
                # MI355X_MICROARCH.md: "8.0 TB/s spec; 6.29 TB/s measured (float4 copy, 79%)"
                "peak_measured_copy": 6290.0, "frac_of_measured_copy": achieved / 6290.0,
                "traffic_source": traffic_src, "algorithmic_bytes": abytes,
                "algorithmic_bytes_per_sample": abytes / samples,
                "op_ms": stats(kall), "ops": both,
                "frac_best_step": abytes / (min(kall) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "timing": "HIP events on the launch stream around the op (calibrate + codec kernel), mean over the timed steps"}
        if not a.no_per_S and world == 1:
            roof["per_S"] = per_S_sweep(cs, out, h, a.mode, a.seg_chunks, tries=max(1, a.placement_tries - 1))
        line = {
            "metric": "MSamples/s encode+decode (static-Huffman MUA codec)",
            "value": value, "unit": "MSamples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": "BASELINE configs[2]: synthetic Poisson MUA, %d channels x %.0e bins per GPU, "
                                   "S=%d, 2^%d-sample calibration, K=%d encoder(s), %s mapper, window [c,T)"
                                   % (C, T, S, h, tab.shape[0], "approx-sort" if a.mode else "no-sort"),
                       "channels_per_gpu": C, "bins": T, "S": S, "hist_bits": h, "K": int(tab.shape[0]),
                       "seg_chunks": a.seg_chunks, "parallelism": "channels sharded x%d, no data-path collective" % world},
            "bits_per_sample": {"payload": b, "container": cb,
                                # the reference's figure of merit for the same bits (get_BR_with_approx_sort.py:289-292)
                                # if these were 50 ms bins: BR = 1000 / (BP / bits_per_sample)
                                "BR_bits_per_s_per_channel_at_BP50": float(codec.bit_rate(bits, samples, 50))},
            "kernels_ms": {"encode_op": enc_ms, "decode_op": dec_ms, "encode_op_stats": stats(enc_all),
                           "decode_op_stats": stats(dec_all),
                           "encode_MSamples_s": samples / enc_ms / 1e3, "decode_MSamples_s": samples / dec_ms / 1e3,
                           "measure_op": meas_ms, "measure_MSamples_s": meas_samples / meas_ms / 1e3,
                           "measure_GBps": meas_samples / meas_ms / 1e6,
                           "measure_window": "[c, c+T/2) reference rule, bits/sample %.4f" % ref_bits_per_sample},
            "roofline": roof,
            "placement": placement,
            "device": info["name"] + " " + info["arch"],
        }
        if dist is not None:
            line["rccl_ranks"] = dist.get_world_size()
            line["dist_backend"] = a.dist_backend
            line["rank_devices"] = devices
            line["rank_payload_words"] = rank_words
        if gather:
            line["gather"] = gather
        if ok is not None:
            line["verified_roundtrip"] = ok
        if dumped is not None:
            line["dump_outputs"] = {"dir": a.dump_outputs, "rank0_arrays": dumped}
        if not a.no_small_shape and world == 1:
            line["small_shape"] = small_shape(S, h, a.mode, a.seg_chunks)
        if c3 is not None:
            line["configs3"] = c3
        if not a.no_cpu_baseline and world == 1:
            nch = min(a.cpu_sample_channels, C)
            nbytes = int(cs.ch_off[nch - 1] + cs.ch_len[nch - 1]) + 64
            host = cs.data[:nbytes].cpu().numpy()
            smp, res = cpu_baseline(host, cs.ch_off, cs.ch_len, S, h, a.mode, tab, a.seg_chunks, nch)
            line["cpu_baseline"] = {"value": res["1"]["msamples_s"], "unit": "MSamples/s", "cores": 1,
                                    "kind": "port",
                                    "sample": "first %d channels x %d bins of the same workload (%.2e samples), "
                                              "oracle/mh_oracle.c encode+decode" % (nch, T, smp),
                                    "all_cores": res.get("all"), "single": res["1"],
                                    "numpy_measure_msamples_s": res["numpy_measure_msamples_s"],
                                    "host_cpus": os.cpu_count(), "cpu_model": cpu_model()}
        if world == 1 and not a.no_configs3:  # last: the headline's buffers make room for the 10 000-channel set
            plan.close()
            del cs, enc, out, plan
            torch.cuda.empty_cache()
            line["configs3"], c3_stuck = configs3_guarded(a, rank, world, None, coll_dev, tab, local, a.gather_deadline)
            if c3_stuck:
                rc = RC_GATHER_STUCK
            elif "error" in line["configs3"]:
                rc = rc or RC_GATHER_FAILED
        print(json.dumps(line), flush=True)
    sys.stdout.flush()
    if rc == RC_GATHER_STUCK:
        os._exit(rc)  # a collective is stuck: the line is out, leave without joining it -- and fail
    if dist is not None:
        dist.destroy_process_group()
    if ok is False:
        rc = rc or 5
    sys.exit(rc)


if __name__ == "__main__":
    main()
