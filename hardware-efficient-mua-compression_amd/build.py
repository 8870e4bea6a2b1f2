"""Build recipe for libmuahuff.so (hand-written gfx950 HIP kernels + C ABI).

hipcc cross-compiles for gfx950 without a GPU present.  The shared object is built in-tree
(next to this file) so that it travels with the source snapshot to the GPU box.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "libmuahuff.so")
SOURCES = ["csrc/muahuff.hip"]
HEADERS = ["csrc/exports.map", "csrc/mh_kernels.hpp", "csrc/mh_device.hpp", "csrc/mh_codec2.hpp", "csrc/mh_range.hpp", "csrc/mh_rebin_decode.hpp", "csrc/mh_layout.hpp", "csrc/mh_packed_measure.hpp",
           "csrc/mh_planner.hpp", "csrc/mh_plan_arena.hpp", "csrc/mh_select.hpp", "csrc/mh_worklist.hpp", "csrc/mh_analysis.hpp",
           "csrc/mh_msg.hpp", "csrc/mh_validate.hpp", "csrc/mh_sweep_planner.hpp", "csrc/mh_launch.hpp", "../include/muahuff.h"]
# the companion (include/muahuff_ingest.h), what stands around the codec: spike time stamps -> binned counts in front,
# payload checksums behind
INGEST_SO = os.path.join(HERE, "libmuahuff_ingest.so")
INGEST_SOURCES = ["csrc/mh_ingest.hip"]
INGEST_HEADERS = ["csrc/exports_ingest.map", "csrc/mh_ingest.hpp", "csrc/mh_aer.hpp", "csrc/mh_aer_layout.hpp",
                  "csrc/mh_crc.hpp", "csrc/mh_crc_tables.hpp", "csrc/mh_unbin.hpp", "csrc/mh_unbin_layout.hpp",
                  "csrc/mh_excess.hpp", "csrc/mh_excess_layout.hpp", "csrc/mh_windows.hpp", "csrc/mh_windows_layout.hpp",
                  "csrc/mh_gram.hpp", "csrc/mh_gram_layout.hpp", "csrc/mh_ingest_check.hpp",
                  "csrc/mh_device.hpp", "csrc/mh_msg.hpp", "csrc/mh_launch.hpp", "../include/muahuff.h",
                  "../include/muahuff_ingest.h"]
# the second companion (include/muahuff_wiener.h): a lagged linear decoder on the counts, its cross products and its prediction
WIENER_SO = os.path.join(HERE, "libmuahuff_wiener.so")
WIENER_SOURCES = ["csrc/mh_wiener.hip"]
WIENER_HEADERS = ["csrc/exports_wiener.map", "csrc/mh_wiener.hpp", "csrc/mh_wiener_layout.hpp", "csrc/mh_msg.hpp",
                  "../include/muahuff.h", "../include/muahuff_wiener.h"]
# the third companion (include/muahuff_cascade.h): the power sums of a prediction against its target and the polynomial
# stage of the Wiener cascade
CASCADE_SO = os.path.join(HERE, "libmuahuff_cascade.so")
CASCADE_SOURCES = ["csrc/mh_cascade.hip"]
CASCADE_HEADERS = ["csrc/exports_cascade.map", "csrc/mh_cascade.hpp", "csrc/mh_cascade_layout.hpp", "csrc/mh_msg.hpp",
                   "../include/muahuff.h", "../include/muahuff_cascade.h"]
# the fourth companion (include/muahuff_smooth.h): the box sums of the decoders' moving-average window, as byte planes of
# the counts and on a float prediction
SMOOTH_SO = os.path.join(HERE, "libmuahuff_smooth.so")
SMOOTH_SOURCES = ["csrc/mh_smooth.hip"]
SMOOTH_HEADERS = ["csrc/exports_smooth.map", "csrc/mh_smooth.hpp", "csrc/mh_smooth_layout.hpp", "csrc/mh_msg.hpp",
                  "../include/muahuff.h", "../include/muahuff_smooth.h"]
# the fifth companion (include/muahuff_sweep.h): the Wiener statistics of every clip, lag difference and range in one pass
SWEEP_SO = os.path.join(HERE, "libmuahuff_sweep.so")
SWEEP_SOURCES = ["csrc/mh_sweep.hip"]
SWEEP_HEADERS = ["csrc/exports_sweep.map", "csrc/mh_sweep.hpp", "csrc/mh_sweep_layout.hpp", "csrc/mh_gram_layout.hpp",
                 "csrc/mh_wiener_layout.hpp", "csrc/mh_device.hpp", "csrc/mh_msg.hpp", "../include/muahuff.h",
                 "../include/muahuff_sweep.h"]
# the sixth companion (include/muahuff_kalman.h): the prediction of a Kalman filter decoder, a constant projection of the
# counts and the scan of an affine recurrence
KALMAN_SO = os.path.join(HERE, "libmuahuff_kalman.so")
KALMAN_SOURCES = ["csrc/mh_kalman.hip"]
KALMAN_HEADERS = ["csrc/exports_kalman.map", "csrc/mh_kalman.hpp", "csrc/mh_kalman_layout.hpp", "csrc/mh_msg.hpp",
                  "../include/muahuff.h", "../include/muahuff_kalman.h"]
# the seventh companion (include/muahuff_lstm.h): the prediction of an LSTM decoder, the input half of the gate
# pre-activations once per bin and the recurrence over every window
LSTM_SO = os.path.join(HERE, "libmuahuff_lstm.so")
LSTM_SOURCES = ["csrc/mh_lstm.hip"]
LSTM_HEADERS = ["csrc/exports_lstm.map", "csrc/mh_lstm.hpp", "csrc/mh_lstm_layout.hpp", "csrc/mh_msg.hpp",
                "../include/muahuff.h", "../include/muahuff_lstm.h"]


def stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    return any(os.path.getmtime(os.path.join(HERE, f)) > t for f in SOURCES + HEADERS)


def build(force=False, verbose=False):
    """libmuahuff.so, exporting the C ABI of include/muahuff.h and nothing else (csrc/exports.map)."""
    if not force and not stale():
        return SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, "csrc", "exports.map")]
    cmd += [os.path.join(HERE, s) for s in SOURCES] + ["-o", SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return SO


def build_ingest(force=False, verbose=False):
    """libmuahuff_ingest.so, exporting the C ABI of include/muahuff_ingest.h and nothing else
    (csrc/exports_ingest.map); the flags of libmuahuff.so."""
    if not force and os.path.exists(INGEST_SO):
        t = os.path.getmtime(INGEST_SO)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in INGEST_SOURCES + INGEST_HEADERS):
            return INGEST_SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, "csrc", "exports_ingest.map")]
    cmd += [os.path.join(HERE, s) for s in INGEST_SOURCES] + ["-o", INGEST_SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return INGEST_SO


def build_wiener(force=False, verbose=False):
    """libmuahuff_wiener.so, exporting the C ABI of include/muahuff_wiener.h and nothing else
    (csrc/exports_wiener.map); the flags of libmuahuff.so."""
    if not force and os.path.exists(WIENER_SO):
        t = os.path.getmtime(WIENER_SO)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in WIENER_SOURCES + WIENER_HEADERS):
            return WIENER_SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, "csrc", "exports_wiener.map")]
    cmd += [os.path.join(HERE, s) for s in WIENER_SOURCES] + ["-o", WIENER_SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return WIENER_SO


def build_cascade(force=False, verbose=False):
    """libmuahuff_cascade.so, exporting the C ABI of include/muahuff_cascade.h and nothing else
    (csrc/exports_cascade.map); the flags of libmuahuff.so."""
    if not force and os.path.exists(CASCADE_SO):
        t = os.path.getmtime(CASCADE_SO)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in CASCADE_SOURCES + CASCADE_HEADERS):
            return CASCADE_SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, "csrc", "exports_cascade.map")]
    cmd += [os.path.join(HERE, s) for s in CASCADE_SOURCES] + ["-o", CASCADE_SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return CASCADE_SO


def build_smooth(force=False, verbose=False):
    """libmuahuff_smooth.so, exporting the C ABI of include/muahuff_smooth.h and nothing else
    (csrc/exports_smooth.map); the flags of libmuahuff.so."""
    if not force and os.path.exists(SMOOTH_SO):
        t = os.path.getmtime(SMOOTH_SO)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in SMOOTH_SOURCES + SMOOTH_HEADERS):
            return SMOOTH_SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, "csrc", "exports_smooth.map")]
    cmd += [os.path.join(HERE, s) for s in SMOOTH_SOURCES] + ["-o", SMOOTH_SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return SMOOTH_SO


def build_sweep(force=False, verbose=False):
    """libmuahuff_sweep.so, exporting the C ABI of include/muahuff_sweep.h and nothing else
    (csrc/exports_sweep.map); the flags of libmuahuff.so."""
    if not force and os.path.exists(SWEEP_SO):
        t = os.path.getmtime(SWEEP_SO)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in SWEEP_SOURCES + SWEEP_HEADERS):
            return SWEEP_SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, "csrc", "exports_sweep.map")]
    cmd += [os.path.join(HERE, s) for s in SWEEP_SOURCES] + ["-o", SWEEP_SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return SWEEP_SO


def build_kalman(force=False, verbose=False):
    """libmuahuff_kalman.so, exporting the C ABI of include/muahuff_kalman.h and nothing else
    (csrc/exports_kalman.map); the flags of libmuahuff.so."""
    if not force and os.path.exists(KALMAN_SO):
        t = os.path.getmtime(KALMAN_SO)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in KALMAN_SOURCES + KALMAN_HEADERS):
            return KALMAN_SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, "csrc", "exports_kalman.map")]
    cmd += [os.path.join(HERE, s) for s in KALMAN_SOURCES] + ["-o", KALMAN_SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return KALMAN_SO


def build_lstm(force=False, verbose=False):
    """libmuahuff_lstm.so, exporting the C ABI of include/muahuff_lstm.h and nothing else
    (csrc/exports_lstm.map); the flags of libmuahuff.so."""
    if not force and os.path.exists(LSTM_SO):
        t = os.path.getmtime(LSTM_SO)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in LSTM_SOURCES + LSTM_HEADERS):
            return LSTM_SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, "csrc", "exports_lstm.map")]
    cmd += [os.path.join(HERE, s) for s in LSTM_SOURCES] + ["-o", LSTM_SO]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return LSTM_SO


def build_example(force=False):
    """examples/abi_roundtrip: a plain-C client of include/muahuff.h (gcc, HIP runtime only)."""
    src = os.path.join(ROOT, "examples", "abi_roundtrip.c")
    exe = os.path.join(ROOT, "examples", "abi_roundtrip")
    if not force and os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(src), os.path.getmtime(SO)):
        return exe
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"), src, "-o", exe,
                           "-L" + HERE, "-lmuahuff", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath,$ORIGIN/../" + os.path.basename(HERE), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    return exe


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    print(build_ingest(force=True, verbose=True))
    print(build_wiener(force=True, verbose=True))
    print(build_cascade(force=True, verbose=True))
    print(build_smooth(force=True, verbose=True))
    print(build_sweep(force=True, verbose=True))
    print(build_kalman(force=True, verbose=True))
    print(build_lstm(force=True, verbose=True))
