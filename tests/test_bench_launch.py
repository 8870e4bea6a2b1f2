"""bench.py --gpus N starts its own N ranks (no GPU needed for these checks): the launcher
rendezvous self-test over gloo, the fail-fast paths and their non-zero exit codes."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env)


def test_gpus_2_spawns_two_ranks_that_rendezvous():
    r = _run(["--gpus", "2", "--check-launch", "--dist-backend", "gloo"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line == {"check_launch": True, "n_gpus": 2, "ranks": 2}


@pytest.mark.skipif(torch.cuda.device_count() >= 2, reason="would really launch on a multi-GPU box")
def test_more_ranks_than_gpus_fails_fast_and_loudly():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], timeout=120)
    assert r.returncode == 2
    assert "needs 2 visible GPUs" in r.stderr and not r.stdout.strip()


def test_world_size_mismatch_is_an_error_not_a_single_gpu_number():
    r = _run(["--gpus", "2", "--check-launch"], env_extra={"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"}, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE=3" in r.stderr
    r = _run(["--gpus", "1", "--check-launch"], env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, timeout=120)
    assert r.returncode == 2


def test_dump_outputs_is_float_seeded_and_within_budget(tmp_path):
    """--dump-outputs (bench.dump_outputs, run here on host tensors laid out like the bench's): float32 / float64
    arrays of 64 MB at most in all; small arrays whole, large ones a sample that the same seed repeats exactly;
    payload words taken only from the used part of each segment's slot, decoded bytes only from the channels."""
    import types

    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    C, T, n_seg, slot, used = 3, 30_000_000, 5, 1_200_000, 1_000_000
    ch_off = np.arange(C, dtype=np.uint64) * np.uint64(T + 16)
    out = torch.full((C * (T + 16),), 255, dtype=torch.uint8)
    for c in range(C):
        out[int(ch_off[c]):int(ch_off[c]) + T] = torch.arange(T, dtype=torch.int64).remainder_(251).to(torch.uint8)
    seg_off = np.arange(n_seg, dtype=np.uint64) * np.uint64(slot)
    word = (torch.arange(n_seg * slot, dtype=torch.int64) * 2654435761) & 0xFFFFFFFF
    payload = torch.where(word == 0xFFFFFFFF, word - 1, word)          # 0xFFFFFFFF marks the unused tails below
    for s in range(n_seg):
        payload[s * slot + used:(s + 1) * slot] = 0xFFFFFFFF
    enc = types.SimpleNamespace(payload=payload.to(torch.int32), seg_words=torch.full((n_seg,), used, dtype=torch.int64),
                                ch_bits=torch.tensor([7, 1 << 40, 0]), peak=torch.tensor([1, 2, 0], dtype=torch.uint8),
                                enc=torch.zeros(C, dtype=torch.uint8), skipped=torch.tensor([0, 0, 1], dtype=torch.uint8))
    plan = types.SimpleNamespace(C=C, n_segments=n_seg, segments=lambda: {"off": seg_off})
    cs = types.SimpleNamespace(ch_off=ch_off, ch_len=np.full(C, T, dtype=np.uint64))

    def dump(d, seed=0, rank=0, world=1):
        names = bench.dump_outputs(str(tmp_path / d), plan, cs, enc, out, seed, rank, world)
        files = {n: np.load(str(tmp_path / d / (n + ".npy"))) for n in names}
        assert sum(os.path.getsize(str(tmp_path / d / (n + ".npy"))) for n in names) <= bench.DUMP_BYTES // world
        assert all(v.dtype in (np.float32, np.float64) and list(v.shape) == names[n] for n, v in files.items())
        return files

    a, b, other = dump("a"), dump("b"), dump("c", seed=1)
    assert sorted(a) == ["ch_bits", "decoded", "enc", "payload_words", "peak", "seg_words", "skipped"]
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert not np.array_equal(a["decoded"], other["decoded"])
    assert a["ch_bits"].tolist() == [7, 1 << 40, 0] and a["skipped"].tolist() == [0, 0, 1]
    assert a["seg_words"].tolist() == [used] * n_seg
    assert 0 < len(a["payload_words"]) < n_seg * used and 0 < len(a["decoded"]) < C * T     # sampled
    assert a["payload_words"].max() < 0xFFFFFFFF and a["payload_words"].max() > 0x7FFFFFFF  # used words, as uint32
    assert a["decoded"].max() <= 250
    r1 = dump("r", rank=1, world=2)
    assert sorted(r1) == sorted(n + "_rank1" for n in a)
