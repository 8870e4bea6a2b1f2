"""Build recipe for libmuahuff.so (hand-written gfx950 HIP kernels + C ABI).

hipcc cross-compiles for gfx950 without a GPU present.  The shared object is built in-tree
(next to this file) so that it travels with the source snapshot to the GPU box.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# one row per shared object: name, .hip source, export map, public header.  libmuahuff.so first, then its companions in
# the order they were added: ingest (spike time stamps -> binned counts in front of the codec, payload checksums behind),
# wiener (a lagged linear decoder on the counts), cascade (power sums and the polynomial stage of the Wiener cascade),
# smooth (the box sums of the decoders' moving-average window), sweep (the Wiener statistics of every clip, lag
# difference and range in one pass), kalman (a constant projection of the counts and the scan of an affine recurrence),
# lstm (the input half of the gate pre-activations once per bin and the recurrence over every window)
LIBRARIES = [("muahuff", "csrc/muahuff.hip", "csrc/exports.map", "../include/muahuff.h")] + \
            [("muahuff_" + n, "csrc/mh_%s.hip" % n, "csrc/exports_%s.map" % n, "../include/muahuff_%s.h" % n)
             for n in ("ingest", "wiener", "cascade", "smooth", "sweep", "kalman", "lstm")]
# the libraries of the training side, built by the same recipe: train (the loss of a minibatch of the LSTM decoder's windows
# and its gradient with respect to the weights)
TRAINING = [("muahuff_train", "csrc/mh_train.hip", "csrc/exports_train.map", "../include/muahuff_train.h")]
_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def reached(source):
    """Every file `source` reaches through #include "...", transitively, resolved like the compiler's -I csrc -I include
    (after the including file's own directory); paths relative to this directory, in the order met."""
    found, todo = [], [source]
    while todo:
        f = todo.pop(0)
        for inc in _INCLUDE.findall(open(os.path.join(HERE, f)).read()):
            for d in (os.path.dirname(f), "csrc", "../include"):
                g = os.path.normpath(os.path.join(d, inc))
                if os.path.exists(os.path.join(HERE, g)):
                    if g not in found:
                        found.append(g)
                        todo.append(g)
                    break
    return found


def _row(name):
    return next(row for row in LIBRARIES + TRAINING if row[0] == name)


def so_path(name):
    return os.path.join(HERE, "lib%s.so" % name)


def headers(name):
    """What besides its source decides whether lib<name>.so is stale: its export map, every header its source reaches and
    its public header."""
    _, source, exports, public = _row(name)
    return [exports] + [h for h in reached(source) if h != public] + [public]


def _names(name):
    return so_path(name), [_row(name)[1]], headers(name)


SO, SOURCES, HEADERS = _names("muahuff")
INGEST_SO, INGEST_SOURCES, INGEST_HEADERS = _names("muahuff_ingest")
WIENER_SO, WIENER_SOURCES, WIENER_HEADERS = _names("muahuff_wiener")
CASCADE_SO, CASCADE_SOURCES, CASCADE_HEADERS = _names("muahuff_cascade")
SMOOTH_SO, SMOOTH_SOURCES, SMOOTH_HEADERS = _names("muahuff_smooth")
SWEEP_SO, SWEEP_SOURCES, SWEEP_HEADERS = _names("muahuff_sweep")
KALMAN_SO, KALMAN_SOURCES, KALMAN_HEADERS = _names("muahuff_kalman")
LSTM_SO, LSTM_SOURCES, LSTM_HEADERS = _names("muahuff_lstm")
TRAIN_SO, TRAIN_SOURCES, TRAIN_HEADERS = _names("muahuff_train")


def stale(name="muahuff"):
    """Is lib<name>.so missing, or older than its source or one of headers(name)?"""
    so = so_path(name)
    if not os.path.exists(so):
        return True
    t = os.path.getmtime(so)
    return any(os.path.getmtime(os.path.join(HERE, f)) > t for f in [_row(name)[1]] + headers(name))


def build_library(name, force=False, verbose=False):
    """lib<name>.so, exporting the C ABI of its public header and nothing else (its export map); every library with the
    same flags."""
    so = so_path(name)
    if not force and not stale(name):
        return so
    _, source, exports, _ = _row(name)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"),
           "-Wl,--version-script=" + os.path.join(HERE, exports)]
    cmd += [os.path.join(HERE, source), "-o", so]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return so


def build(force=False, verbose=False):
    """libmuahuff.so, exporting the C ABI of include/muahuff.h and nothing else (csrc/exports.map)."""
    return build_library("muahuff", force, verbose)


def build_ingest(force=False, verbose=False):
    return build_library("muahuff_ingest", force, verbose)


def build_wiener(force=False, verbose=False):
    return build_library("muahuff_wiener", force, verbose)


def build_cascade(force=False, verbose=False):
    return build_library("muahuff_cascade", force, verbose)


def build_smooth(force=False, verbose=False):
    return build_library("muahuff_smooth", force, verbose)


def build_sweep(force=False, verbose=False):
    return build_library("muahuff_sweep", force, verbose)


def build_kalman(force=False, verbose=False):
    return build_library("muahuff_kalman", force, verbose)


def build_lstm(force=False, verbose=False):
    return build_library("muahuff_lstm", force, verbose)


def build_train(force=False, verbose=False):
    return build_library("muahuff_train", force, verbose)


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
    print(build_train(force=True, verbose=True))
