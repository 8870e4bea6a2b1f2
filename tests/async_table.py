"""The asynchronous class of every entry point of include/muahuff.h, and the plan layouts the asynchronous-contract
tests run on (a plain module, not a conftest).

CLASS gives each mh_* function one of

  host          no device work: pure host arithmetic, queries, validation of host arrays
  capturable    only enqueues work on `stream`: no synchronisation, allocation or free, so the call can be captured
                into a hipGraph.  The "Conventions" comment of the header names exactly this set.
  synchronises  documented to synchronise or to allocate / free: plan and sweep creation and destruction, the status
                read, and the range calls, which build their work list on the host

tests/test_host_async_contract.py checks without a GPU that the table covers exactly the declared symbols, that the
header names the capturable set, and that the host planner puts every LAYOUT in the form it names;
tests/test_gpu_async_contract.py runs stream order, graph capture and plan state against the CPU oracle.
"""
from dataclasses import dataclass

CHUNK = 16384

HOST, CAPTURABLE, SYNCHRONISES = "host", "capturable", "synchronises"

CLASS = {
    "mh_version": HOST,
    "mh_last_error": HOST,
    "mh_device_info": HOST,
    "mh_codebook": HOST,
    "mh_approx_sort_perm": HOST,
    "mh_plan_create": SYNCHRONISES,
    "mh_plan_create_packed": SYNCHRONISES,
    "mh_plan_destroy": SYNCHRONISES,
    "mh_plan_info": HOST,
    "mh_plan_segments": HOST,
    "mh_plan_query": HOST,
    "mh_measure": CAPTURABLE,
    "mh_encode": CAPTURABLE,
    "mh_encode_preset": CAPTURABLE,
    "mh_decode": CAPTURABLE,
    "mh_decode_packed": CAPTURABLE,
    "mh_decode_status": SYNCHRONISES,
    "mh_validate_stream": HOST,
    "mh_decode_range": SYNCHRONISES,
    "mh_decode_rebin": SYNCHRONISES,
    "mh_validate_segments": HOST,
    "mh_compact": CAPTURABLE,
    "mh_synth_poisson": CAPTURABLE,
    "mh_rebin": CAPTURABLE,
    "mh_deinterleave": CAPTURABLE,
    "mh_deinterleave_packed": CAPTURABLE,
    "mh_interleave": CAPTURABLE,
    "mh_interleave_packed": CAPTURABLE,
    "mh_sweep_create": SYNCHRONISES,
    "mh_sweep_destroy": SYNCHRONISES,
    "mh_sweep_info": HOST,
    "mh_sweep_run": CAPTURABLE,
    "mh_power_draws": CAPTURABLE,
    "mh_reduce_rows": CAPTURABLE,
}


def of_class(cls):
    return sorted(n for n, c in CLASS.items() if c == cls)


@dataclass(frozen=True)
class Layout:
    """One byte-layout plan: channel lengths and the design point (the K rows are the whole SCLV table of S,
    tests/golden/tables.json), and the planner form it is meant to land in (csrc/mh_planner.hpp, PlanHost)."""
    name: str
    lens: tuple
    S: int
    h: int
    mode: int
    window: int
    seg_chunks: int
    # the form
    wave: bool            # use_wave_tasks
    measure_fused: bool   # mh_measure is one launch
    fused_cal: bool       # the wave-task encoder calibrates in the wave (mh_encode is one launch)
    tickets_fit: bool     # ... and keeps the channel's ticket word in d_acc
    cal_tiled: bool       # 2^h above kCalDirect: the calibration histogram goes through d_calhist
    heads: int = 0        # head segments (format revision 3)
    skipped: int = 0      # channels skipped by the MH_WIN_REF_HALF rule
    short: int = 0        # channels shorter than their calibration window 2^h


K_CAL_DIRECT = 4096               # mh::kCalDirect
K_FUSED_MEASURE_CHANNELS = 4096   # mh::kFusedMeasureChannels

LAYOUTS = (
    # (a) short channels, 2^h <= kCalDirect: one-launch measure, wave tasks, in-wave calibration, ticket words
    Layout("a", (7, 1000, CHUNK, CHUNK + 1, 40000, 3 * CHUNK), S=3, h=6, mode=1, window=2, seg_chunks=1,
           wave=True, measure_fused=True, fused_cal=True, tickets_fit=True, cal_tiled=False, short=1),
    # (b) workgroup tasks (every channel has exactly four segments) and more than kFusedMeasureChannels channels: the
    #     three-launch measure (k_calibrate, histogram, k_finalize), k_lut_preset in front of the preset encoder
    Layout("b", (3 * CHUNK + 1,) * (K_FUSED_MEASURE_CHANNELS + 4), S=4, h=6, mode=1, window=3, seg_chunks=1,
           wave=False, measure_fused=False, fused_cal=False, tickets_fit=False, cal_tiled=False),
    # (c) wave tasks with 2^h above kCalDirect: tiled calibration histogram (d_calhist, cleared per call), k_calibrate
    #     as a launch of its own, the plan's default (peak, enc) words between the launches
    Layout("c", (7, 1000, CHUNK, CHUNK + 1, 40000, 3 * CHUNK), S=10, h=13, mode=0, window=2, seg_chunks=1,
           wave=True, measure_fused=False, fused_cal=False, tickets_fit=True, cal_tiled=True, short=2),
    # (d) head segments: the first channel's window [64, 64 + 16 chunks + 64) starts off a 128-sample boundary and is
    #     long enough for a head; one channel shorter than its calibration window (40 < 2^6) and one that the
    #     MH_WIN_REF_HALF rule skips (c + T/2 > T) -- the short one is skipped by that rule too.  Workgroup tasks.
    Layout("d", (2 * (64 + 16 * CHUNK), 40, 100, 16 * CHUNK), S=7, h=6, mode=1, window=0, seg_chunks=1,
           wave=False, measure_fused=True, fused_cal=False, tickets_fit=False, cal_tiled=False, heads=1, skipped=2,
           short=1),
)

BY_NAME = {l.name: l for l in LAYOUTS}
