"""The driver's entry points on the GPU box, as one process and as two."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    return subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_build_then_smoke_in_one_process():
    """build() loads the library before anything has imported torch; smoke() must still find the GPU
    (one HIP runtime per process: _lib.lib() imports torch first)."""
    r = _run(["__graft_entry__.py", "smoke"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "smoke ok" in r.stdout and "bit-exact vs oracle" in r.stdout


def test_smoke_alone():
    r = _run(["-c", "import __graft_entry__ as g; g.smoke()"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "smoke ok" in r.stdout


def test_bench_dump_outputs_repeat_and_hold_the_decoded_input(tmp_path):
    """bench.py --dump-outputs: two runs with the same arguments write the same arrays; at this size they are whole,
    so decoded must be the generated input clamped to S - 1 (bytes before the window untouched: 0) and ch_bits must
    give the line's payload bits/sample."""
    import json

    import numpy as np

    from muahuff import synth
    C, T, S, h = 8, 200_000, 3, 6
    args = ["bench.py", "--gpus", "1", "--channels-per-gpu", str(C), "--bins", str(T), "--steps", "3", "--warmup", "1",
            "--no-per-S", "--no-small-shape", "--no-cpu-baseline", "--no-configs3", "--placement-tries", "1"]
    dumps = []
    for d in ("a", "b"):
        r = _run(args + ["--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        names = sorted(line["dump_outputs"]["rank0_arrays"])
        dumps.append({n: np.load(str(tmp_path / d / (n + ".npy"))) for n in names})
    a, b = dumps
    assert sorted(a) == ["ch_bits", "decoded", "enc", "payload_words", "peak", "seg_words", "skipped"]
    assert all(np.array_equal(a[n], b[n]) for n in a)
    cs = synth.generate(C, T, seed=0)
    host = cs.matrix().cpu().numpy()
    dec = a["decoded"].reshape(C, T)
    assert a["decoded"].dtype == np.float32
    assert np.array_equal(dec[:, :2 ** h], np.zeros((C, 2 ** h), np.float32))
    assert np.array_equal(dec[:, 2 ** h:], np.minimum(host[:, 2 ** h:], S - 1).astype(np.float32))
    assert a["ch_bits"].sum() / (C * (T - 2 ** h)) == line["bits_per_sample"]["payload"]
    assert a["payload_words"].size == a["seg_words"].sum()
